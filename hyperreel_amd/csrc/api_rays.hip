// C ABI, camera rays, light-field rays and the training feed: hr_generate_rays, hr_generate_rays_ndc, hr_generate_rays_fisheye (one set of checks, one
// routine: generate_pixels), hr_generate_rays_lightfield, hr_generate_rays_epi, hr_rayset_* (kernels: rays_kernel.hip, importance_kernel.hip;
// arithmetic: hr_camera.h, hr_lightfield.h, hr_sample_rng.h, hr_importance.h).
// No model handle.  The set owns its device memory; hr_rayset_batch / hr_rayset_order / hr_rayset_sample enqueue one kernel and nothing else.
#include <hip/hip_runtime.h>

#include <vector>

#include "hr_camera.h"
#include "hr_importance.h"
#include "hr_lightfield.h"
#include "hr_model.h"

struct HR_HIDDEN hr_rayset {
    int n_images = 0, width = 0, height = 0, ray_dim = 0;
    bool has_ndc = false;
    hr_ndc ndc = {};
    bool lightfield = false;              // made by hr_rayset_create_lightfield: the images are views of `lf`
    hr_lightfield lf = {};
    std::vector<HrRayImage> images;       // every == 0: not set yet (no rays)
    std::vector<int64_t> prefix;          // [n_images + 1]
    DevMem<HrRayImage> images_dev;
    DevMem<int64_t> prefix_dev;
    DevMem<uint8_t> pixels;
    int bpp = 3;                          // bytes of a stored pixel: 3 (HR_PIXELS_RGB8) or 4 (HR_PIXELS_RGBA8_WHITE)
    bool stored = false;                  // an image's pixels are in the store: the format is fixed
    // the importance rule (hr_rayset_set_image_importance): a listed image's pixel list and what it was made with
    struct Listed {
        DevMem<uint32_t> list;
        int prev = -1;
        int64_t num_take = 0;
        float threshold = 0.0f, dir_z_below = 0.0f;
    };
    std::vector<Listed> listed;           // [n_images]; images[i].list points into listed[i].list
    DevMem<uint32_t> importance_ws;       // hr_importance_workspace_words(width * height), allocated by the first such call
};

namespace {

int check_ndc(const hr_ndc* ndc, const char* who)
{
    if (ndc && (ndc->width < 1 || ndc->height < 1 || ndc->fx == 0.0f || ndc->fy == 0.0f))
        return fail(HR_E_INVALID, "%s: bad hr_ndc (width %d, height %d, fx %g, fy %g)", who, (int)ndc->width, (int)ndc->height, (double)ndc->fx,
                    (double)ndc->fy);
    return HR_OK;
}

// NULL: no distortion.  A pair whose model is not increasing on [0, pi / 2] has no inverse to compute
int check_fisheye(const hr_fisheye* fe, const char* who)
{
    if (fe && !hr_fisheye_invertible(fe->k1, fe->k2))
        return fail(HR_E_INVALID, "%s: hr_fisheye (k1 %g, k2 %g) is not invertible: 1 + 3 k1 t^2 + 5 k2 t^4 must stay positive on [0, pi / 2]", who,
                    (double)fe->k1, (double)fe->k2);
    return HR_OK;
}

// NULL or all-zero: no distortion given, the pinhole camera
bool undistorted(const hr_fisheye* fe) { return !fe || (fe->k1 == 0.0f && fe->k2 == 0.0f); }

// the arguments every camera pixel-list call shares
int check_pixel_call(const hr_camera* cam, int ray_dim, int64_t first, int64_t n, const float* rays, const char* who)
{
    if (!cam || (n > 0 && !rays)) return fail(HR_E_INVALID, "%s: null argument", who);
    if (ray_dim != 6 && ray_dim != 8) return fail(HR_E_INVALID, "%s: ray_dim must be 6 or 8", who);
    if (cam->width < 1 || cam->height < 1 || cam->fx == 0.0f || cam->fy == 0.0f) return fail(HR_E_INVALID, "%s: bad camera", who);
    const int64_t size = (int64_t)cam->width * cam->height;
    if (first < 0 || n < 0 || first > size || n > size - first) return fail(HR_E_INVALID, "%s: pixel range outside the image", who);
    return HR_OK;
}

// fisheye, ndc: NULL where the entry point has none.  A NULL or all-zero fisheye is the pinhole camera
int generate_pixels(const hr_camera* cam, const hr_fisheye* fisheye, const hr_ndc* ndc, int ray_dim, int64_t first, int64_t n, float* rays_dev,
                    void* stream, const char* who)
{
    if (int rc = check_fisheye(fisheye, who)) return rc;
    if (int rc = check_pixel_call(cam, ray_dim, first, n, rays_dev, who)) return rc;
    if (int rc = check_ndc(ndc, who)) return rc;
    if (n == 0) return HR_OK;              // an empty range: nothing to launch
    hr_launch_generate_rays(*cam, undistorted(fisheye) ? nullptr : fisheye, ndc, ray_dim, first, n, rays_dev, (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

int check_lightfield(const hr_lightfield* lf, float a, float b, const char* who)
{
    if (!lf) return fail(HR_E_INVALID, "%s: null hr_lightfield", who);
    if (lf->width < 1 || lf->height < 1 || lf->aspect == 0.0f)
        return fail(HR_E_INVALID, "%s: bad hr_lightfield (width %d, height %d, aspect %g)", who, (int)lf->width, (int)lf->height, (double)lf->aspect);
    if (!isfinite(lf->aspect) || !isfinite(lf->st_scale) || !isfinite(lf->uv_scale) || !isfinite(lf->near) || !isfinite(lf->far) || !isfinite(a) ||
        !isfinite(b))
        return fail(HR_E_INVALID, "%s: non-finite scalar (aspect %g, st_scale %g, uv_scale %g, near %g, far %g; position %g, %g)", who,
                    (double)lf->aspect, (double)lf->st_scale, (double)lf->uv_scale, (double)lf->near, (double)lf->far, (double)a, (double)b);
    return HR_OK;
}

int generate_lightfield(const hr_lightfield* lf, bool epi, float a, float b, int64_t first, int64_t n, float* rays_dev, void* stream, const char* who)
{
    if (int rc = check_lightfield(lf, a, b, who)) return rc;
    const int64_t size = (int64_t)lf->width * lf->height;
    if (first < 0 || n < 0 || first > size || n > size - first)
        return fail(HR_E_INVALID, "%s: rows [%lld, %lld + %lld) outside the list's %lld rays", who, (long long)first, (long long)first, (long long)n,
                    (long long)size);
    if (n > 0 && !rays_dev) return fail(HR_E_INVALID, "%s: null output", who);
    if (n == 0) return HR_OK;              // an empty range: nothing to launch
    hr_launch_generate_rays_lightfield(*lf, epi, a, b, first, n, rays_dev, (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

int check_rows(const hr_rayset* set, int64_t first, int64_t n, const char* who)
{
    if (!set) return fail(HR_E_INVALID, "%s: null set", who);
    const int64_t size = set->prefix[set->n_images];
    if (first < 0 || n < 0 || first > size || n > size - first)
        return fail(HR_E_INVALID, "%s: rows [%lld, %lld + %lld) outside the set's %lld rays", who, (long long)first, (long long)first,
                    (long long)n, (long long)size);
    if (n > ((int64_t)1 << 38)) return fail(HR_E_INVALID, "%s: more than 2^38 rows in one call", who);
    return HR_OK;
}

HrRaySetArgs set_args(const hr_rayset* s, int64_t first, int64_t n, uint64_t seed, uint64_t epoch)
{
    HrRaySetArgs a = HrRaySetArgs();
    a.images = s->images_dev;
    a.prefix = s->prefix_dev;
    a.pixels = s->pixels;
    a.rgba = s->bpp == 4;
    a.n_images = s->n_images; a.width = s->width; a.height = s->height; a.ray_dim = s->ray_dim;
    a.has_ndc = s->has_ndc ? 1 : 0;
    a.ndc = s->ndc;
    a.lightfield = s->lightfield ? 1 : 0;
    a.lf = s->lf;
    a.size = s->prefix[s->n_images];
    a.first = first; a.n = n;
    a.key = hr_perm_key(seed, epoch);
    return a;
}

}  // namespace

int hr_generate_rays_lightfield(const hr_lightfield* lf, float s, float t, int64_t first_pixel, int64_t n_pixels, float* rays_dev, void* stream)
{
    return generate_lightfield(lf, false, s, t, first_pixel, n_pixels, rays_dev, stream, "hr_generate_rays_lightfield");
}

int hr_generate_rays_epi(const hr_lightfield* lf, float v, float t, int64_t first, int64_t n, float* rays_dev, void* stream)
{
    return generate_lightfield(lf, true, v, t, first, n, rays_dev, stream, "hr_generate_rays_epi");
}

int hr_generate_rays(const hr_camera* cam, int32_t ray_dim, int64_t first_pixel, int64_t n_pixels, float* rays_dev, void* stream)
{
    return generate_pixels(cam, nullptr, nullptr, ray_dim, first_pixel, n_pixels, rays_dev, stream, "hr_generate_rays");
}

int hr_generate_rays_ndc(const hr_camera* cam, const hr_ndc* ndc, int32_t ray_dim, int64_t first_pixel, int64_t n_pixels, float* rays_dev,
                         void* stream)
{
    return generate_pixels(cam, nullptr, ndc, ray_dim, first_pixel, n_pixels, rays_dev, stream, "hr_generate_rays_ndc");
}

int hr_generate_rays_fisheye(const hr_camera* cam, const hr_fisheye* fisheye, const hr_ndc* ndc, int32_t ray_dim, int64_t first_pixel,
                             int64_t n_pixels, float* rays_dev, void* stream)
{
    return generate_pixels(cam, fisheye, ndc, ray_dim, first_pixel, n_pixels, rays_dev, stream, "hr_generate_rays_fisheye");
}

// the set's tables and pixel store; `s` is deleted on failure
static int rayset_alloc(hr_rayset* s, hr_rayset** out, const char* who)
{
    const int n_images = s->n_images, width = s->width, height = s->height;
    s->images.assign((size_t)n_images, HrRayImage());
    s->listed.resize((size_t)n_images);
    s->prefix.assign((size_t)n_images + 1, 0);
    hipError_t e = s->images_dev.alloc(sizeof(HrRayImage) * (size_t)n_images);
    if (e == hipSuccess) e = s->prefix_dev.alloc(sizeof(int64_t) * ((size_t)n_images + 1));
    if (e == hipSuccess) e = s->pixels.alloc((size_t)n_images * height * width * 3);
    if (e == hipSuccess) e = hipMemcpy(s->images_dev, s->images.data(), sizeof(HrRayImage) * (size_t)n_images, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->prefix_dev, s->prefix.data(), sizeof(int64_t) * ((size_t)n_images + 1), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        delete s;
        return fail(HR_E_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    *out = s;
    return HR_OK;
}

int hr_rayset_create(int32_t n_images, int32_t width, int32_t height, int32_t ray_dim, const hr_ndc* ndc, hr_rayset** out)
{
    if (!out) return fail(HR_E_INVALID, "hr_rayset_create: null argument");
    *out = nullptr;
    if (n_images < 1 || width < 1 || height < 1) return fail(HR_E_INVALID, "hr_rayset_create: bad shape (%d images of %d x %d)", (int)n_images, (int)width, (int)height);
    if (ray_dim != 6 && ray_dim != 8) return fail(HR_E_INVALID, "hr_rayset_create: ray_dim must be 6 or 8");
    if (int rc = check_ndc(ndc, "hr_rayset_create")) return rc;
    hr_rayset* s = new hr_rayset();
    s->n_images = n_images; s->width = width; s->height = height; s->ray_dim = ray_dim;
    s->has_ndc = ndc != nullptr;
    if (ndc) s->ndc = *ndc;
    return rayset_alloc(s, out, "hr_rayset_create");
}

int hr_rayset_create_lightfield(int32_t n_views, const hr_lightfield* lf, hr_rayset** out)
{
    if (!out) return fail(HR_E_INVALID, "hr_rayset_create_lightfield: null argument");
    *out = nullptr;
    if (int rc = check_lightfield(lf, 0.0f, 0.0f, "hr_rayset_create_lightfield")) return rc;
    if (n_views < 1) return fail(HR_E_INVALID, "hr_rayset_create_lightfield: %d views", (int)n_views);
    hr_rayset* s = new hr_rayset();
    s->n_images = n_views; s->width = lf->width; s->height = lf->height; s->ray_dim = 6;
    s->lightfield = true;
    s->lf = *lf;
    return rayset_alloc(s, out, "hr_rayset_create_lightfield");
}

void hr_rayset_destroy(hr_rayset* set) { delete set; }

int hr_rayset_set_pixel_format(hr_rayset* set, int32_t format)
{
    if (!set) return fail(HR_E_INVALID, "hr_rayset_set_pixel_format: null set");
    if (format != HR_PIXELS_RGB8 && format != HR_PIXELS_RGBA8_WHITE)
        return fail(HR_E_INVALID, "hr_rayset_set_pixel_format: unknown format %d (HR_PIXELS_RGB8 = %d, HR_PIXELS_RGBA8_WHITE = %d)", (int)format,
                    (int)HR_PIXELS_RGB8, (int)HR_PIXELS_RGBA8_WHITE);
    if (set->stored)
        return fail(HR_E_STATE, "hr_rayset_set_pixel_format: the set already holds an image: a set is RGB or RGBA as a whole, choose before the first "
                    "hr_rayset_set_image / hr_rayset_set_view");
    const int bpp = format == HR_PIXELS_RGBA8_WHITE ? 4 : 3;
    if (bpp == set->bpp) return HR_OK;
    DevMem<uint8_t> store;                 // built aside: the set keeps its store when this fails
    HR_HIP(store.alloc((size_t)set->n_images * set->height * set->width * (size_t)bpp));
    set->pixels = std::move(store);
    set->bpp = bpp;
    return HR_OK;
}

// slot i of the set (`what`: "image" / "view") and its subsample rule
static int check_slot(const hr_rayset* set, int i, int every, int offset, const char* who, const char* what)
{
    if (i < 0 || i >= set->n_images) return fail(HR_E_INVALID, "%s: %s %d of %d", who, what, i, set->n_images);
    if (every < 1 || offset < 0) return fail(HR_E_INVALID, "%s: subsample rule every %d, offset %d (every >= 1, offset >= 0)", who, every, offset);
    return HR_OK;
}

// A listed image's list holds the difference to its `prev` image as that one was when the list was made: replacing `prev` afterwards
// would leave it stale
static int check_not_a_prev(const hr_rayset* set, int i, const char* who)
{
    for (int j = 0; j < set->n_images; ++j)
        if (set->images[j].list && set->listed[j].prev == i)
            return fail(HR_E_INVALID, "%s: image %d is the previous frame of image %d, whose importance list was made from it and would be stale: "
                        "set images in load order", who, i, j);
    return HR_OK;
}

// table entry of image i (its pixels are in the store), then the prefix sums from i on
static int rayset_commit_tables(hr_rayset* set, int i, const HrRayImage& image)
{
    set->images[i] = image;
    if (!image.list) set->listed[i] = hr_rayset::Listed();             // a list the slot held before goes
    for (int j = i; j < set->n_images; ++j) {
        const HrRayImage& im = set->images[j];
        const int64_t kept = im.every < 1 ? 0 : im.list ? im.count : hr_subsample_count(set->width, set->height, im.every, im.offset);
        set->prefix[j + 1] = set->prefix[j] + kept;
    }
    HR_HIP(hipMemcpy(set->images_dev + i, &set->images[i], sizeof(HrRayImage), hipMemcpyHostToDevice));
    HR_HIP(hipMemcpy(set->prefix_dev + i, &set->prefix[i], sizeof(int64_t) * (size_t)(set->n_images + 1 - i), hipMemcpyHostToDevice));
    return HR_OK;
}

static int rayset_store_pixels(hr_rayset* set, int i, const uint8_t* rgb_host_or_dev)
{
    const size_t bytes = (size_t)set->height * set->width * (size_t)set->bpp;
    HR_HIP(hipMemcpy(set->pixels + (size_t)i * bytes, rgb_host_or_dev, bytes, hipMemcpyDefault));
    set->stored = true;
    return HR_OK;
}

// pixels and table entry of image i, then the prefix sums from i on
static int rayset_commit(hr_rayset* set, int i, const HrRayImage& image, const uint8_t* rgb_host_or_dev)
{
    if (int rc = rayset_store_pixels(set, i, rgb_host_or_dev)) return rc;
    return rayset_commit_tables(set, i, image);
}

// the checks hr_rayset_set_image_fisheye makes of its camera and distortion (messages name hr_rayset_set_image)
static int check_set_camera(const hr_rayset* set, const hr_camera* cam, const hr_fisheye* fisheye)
{
    if (cam->width != set->width || cam->height != set->height || cam->fx == 0.0f || cam->fy == 0.0f)
        return fail(HR_E_INVALID, "hr_rayset_set_image: bad camera (%d x %d in a set of %d x %d, fx %g, fy %g)", (int)cam->width, (int)cam->height,
                    set->width, set->height, (double)cam->fx, (double)cam->fy);
    return check_fisheye(fisheye, "hr_rayset_set_image_fisheye");
}

int hr_rayset_set_image(hr_rayset* set, int32_t i, const hr_camera* cam, int32_t every, int32_t offset, const uint8_t* rgb_host_or_dev)
{
    return hr_rayset_set_image_fisheye(set, i, cam, nullptr, every, offset, rgb_host_or_dev);
}

// (messages name hr_rayset_set_image: the plain call is this one without a distortion)
int hr_rayset_set_image_fisheye(hr_rayset* set, int32_t i, const hr_camera* cam, const hr_fisheye* fisheye, int32_t every, int32_t offset,
                                const uint8_t* rgb_host_or_dev)
{
    if (!set || !cam || !rgb_host_or_dev) return fail(HR_E_INVALID, "hr_rayset_set_image: null argument");
    if (set->lightfield) return fail(HR_E_INVALID, "hr_rayset_set_image: the set holds light-field views (hr_rayset_create_lightfield): use hr_rayset_set_view");
    if (int rc = check_slot(set, i, every, offset, "hr_rayset_set_image", "image")) return rc;
    if (int rc = check_set_camera(set, cam, fisheye)) return rc;
    if (int rc = check_not_a_prev(set, i, "hr_rayset_set_image")) return rc;
    HrRayImage im = HrRayImage();
    im.cam = *cam;
    if (!undistorted(fisheye)) { im.fe = *fisheye; im.has_fe = 1; }
    im.every = every; im.offset = offset;
    return rayset_commit(set, i, im, rgb_host_or_dev);
}

int hr_rayset_set_image_importance(hr_rayset* set, int32_t i, const hr_camera* cam, const hr_fisheye* fisheye, int32_t prev, int64_t num_take,
                                   float dir_z_below, const uint8_t* rgb_host_or_dev)
{
    const char* who = "hr_rayset_set_image_importance";
    if (!set || !cam || !rgb_host_or_dev) return fail(HR_E_INVALID, "%s: null argument", who);
    if (set->lightfield)
        return fail(HR_E_INVALID, "%s: the set holds light-field views (hr_rayset_create_lightfield): the importance rule is for posed video frames", who);
    if (set->bpp != 3)
        return fail(HR_E_INVALID, "%s: the set holds RGBA pixels (hr_rayset_set_pixel_format): the importance rule compares 8-bit RGB frames, as the "
                    "reference's importance datasets load them", who);
    if (int rc = check_slot(set, i, 1, 0, who, "image")) return rc;
    const int64_t n_pixels = (int64_t)set->width * set->height;
    if (n_pixels >= ((int64_t)1 << 31)) return fail(HR_E_INVALID, "%s: %lld pixels per image: pixel indices are 31-bit", who, (long long)n_pixels);
    if (prev == i) return fail(HR_E_INVALID, "%s: prev == i (%d): an image is not its own previous frame", who, (int)i);
    if (prev < 0 || prev >= set->n_images) return fail(HR_E_INVALID, "%s: prev %d outside the set's %d images", who, (int)prev, set->n_images);
    if (set->images[prev].every < 1)
        return fail(HR_E_INVALID, "%s: prev image %d is not set yet: set images in load order, the previous frame first", who, (int)prev);
    if (num_take < 1)
        return fail(HR_E_INVALID, "%s: num_take %lld < 1 (with 0 the reference's diff_sorted[-0] is the MINIMUM difference and its rule silently keeps "
                    "nearly every pixel: refused, not reproduced)", who, (long long)num_take);
    if (num_take > n_pixels) return fail(HR_E_INVALID, "%s: num_take %lld > the image's %lld pixels", who, (long long)num_take, (long long)n_pixels);
    if (int rc = check_set_camera(set, cam, fisheye)) return rc;
    if (int rc = check_not_a_prev(set, i, who)) return rc;

    // built aside: the list and, once per set, the workspace
    hr_rayset::Listed made;
    made.prev = prev; made.num_take = num_take; made.dir_z_below = dir_z_below;
    const uint32_t cap = (uint32_t)(num_take > 1 ? num_take - 1 : 1);
    HR_HIP(made.list.alloc(sizeof(uint32_t) * (size_t)cap));
    if (!set->importance_ws) HR_HIP(set->importance_ws.alloc(sizeof(uint32_t) * hr_importance_workspace_words(n_pixels)));
    if (int rc = rayset_store_pixels(set, i, rgb_host_or_dev)) return rc;

    HrRayImage im = HrRayImage();
    im.cam = *cam;
    if (!undistorted(fisheye)) { im.fe = *fisheye; im.has_fe = 1; }
    im.every = 1; im.offset = 0;
    HrImportanceArgs a = HrImportanceArgs();
    a.image = im;
    a.cur = set->pixels + (size_t)i * (size_t)n_pixels * 3;
    a.prev = set->pixels + (size_t)prev * (size_t)n_pixels * 3;
    a.width = set->width; a.height = set->height;
    a.has_ndc = set->has_ndc ? 1 : 0;
    a.ndc = set->ndc;
    a.rank = (uint32_t)hr_importance_rank(n_pixels, num_take);
    a.has_dir = isnan(dir_z_below) ? 0 : 1;
    a.dir_z_below = dir_z_below;
    a.list = made.list; a.list_cap = cap;
    a.workspace = set->importance_ws;
    HR_HIP(hr_launch_importance_select(a, nullptr));
    uint32_t back[4] = {};               // threshold key, pad, the 64-bit kept count: one copy, which also waits for the kernels
    HR_HIP(hipMemcpy(back, set->importance_ws + HR_IMP_WS_THRESHOLD, sizeof(back), hipMemcpyDeviceToHost));
    made.threshold = hr_importance_key_value(back[0]);
    im.count = (int64_t)(((uint64_t)back[3] << 32) | back[2]);
    if (im.count > (int64_t)cap) return fail(HR_E_HIP, "%s: %lld pixels kept where %u fit", who, (long long)im.count, cap);
    im.list = made.list;
    set->listed[i] = std::move(made);
    return rayset_commit_tables(set, i, im);
}

int hr_rayset_image_pixels(const hr_rayset* set, int32_t i, int64_t first, int64_t n, int32_t* out_dev, void* stream)
{
    if (!set) return fail(HR_E_INVALID, "hr_rayset_image_pixels: null set");
    if (i < 0 || i >= set->n_images) return fail(HR_E_INVALID, "hr_rayset_image_pixels: image %d of %d", (int)i, set->n_images);
    const int64_t kept = set->prefix[i + 1] - set->prefix[i];
    if (first < 0 || n < 0 || first > kept || n > kept - first)
        return fail(HR_E_INVALID, "hr_rayset_image_pixels: pixels [%lld, %lld + %lld) outside the image's %lld kept", (long long)first, (long long)first,
                    (long long)n, (long long)kept);
    if (n > 0 && !out_dev) return fail(HR_E_INVALID, "hr_rayset_image_pixels: null output");
    if (n == 0) return HR_OK;
    const HrRayImage& im = set->images[i];
    hr_launch_image_pixels(im.list, set->width, set->height, im.every, im.offset, first, n, out_dev, (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

int hr_rayset_image_info(const hr_rayset* set, int32_t i, struct hr_rayset_image_info* out)
{
    if (!set || !out) return fail(HR_E_INVALID, "hr_rayset_image_info: null argument");
    if (i < 0 || i >= set->n_images) return fail(HR_E_INVALID, "hr_rayset_image_info: image %d of %d", (int)i, set->n_images);
    const HrRayImage& im = set->images[i];
    const hr_rayset::Listed& l = set->listed[i];
    out->count = set->prefix[i + 1] - set->prefix[i];
    out->every = im.every; out->offset = im.offset;
    out->is_list = im.list ? 1 : 0;
    out->prev = im.list ? l.prev : -1;
    out->num_take = im.list ? l.num_take : 0;
    out->threshold = im.list ? l.threshold : 0.0f;
    out->dir_z_below = im.list ? l.dir_z_below : __builtin_nanf("");
    return HR_OK;
}

int hr_rayset_set_view(hr_rayset* set, int32_t i, float s, float t, int32_t every, int32_t offset, const uint8_t* rgb_host_or_dev)
{
    if (!set || !rgb_host_or_dev) return fail(HR_E_INVALID, "hr_rayset_set_view: null argument");
    if (!set->lightfield) return fail(HR_E_INVALID, "hr_rayset_set_view: the set holds posed images (hr_rayset_create): use hr_rayset_set_image");
    if (int rc = check_slot(set, i, every, offset, "hr_rayset_set_view", "view")) return rc;
    if (!isfinite(s) || !isfinite(t)) return fail(HR_E_INVALID, "hr_rayset_set_view: non-finite position (%g, %g)", (double)s, (double)t);
    HrRayImage im = HrRayImage();
    im.every = every; im.offset = offset;
    im.s = s; im.t = t;
    return rayset_commit(set, i, im, rgb_host_or_dev);
}

int64_t hr_rayset_size(const hr_rayset* set)
{
    if (!set) return fail(HR_E_INVALID, "hr_rayset_size: null set");
    return set->prefix[set->n_images];
}

int hr_rayset_batch(const hr_rayset* set, int64_t first, int64_t n, uint64_t seed, uint64_t epoch, const int64_t* indices_dev,
                    float* coords_dev, float* rgb_dev, float* weight_dev, void* stream)
{
    if (int rc = check_rows(set, first, n, "hr_rayset_batch")) return rc;
    HrRaySetArgs a = set_args(set, first, n, seed, epoch);
    a.indices = indices_dev;
    a.coords = coords_dev; a.rgb = rgb_dev; a.weight = weight_dev;
    hr_launch_rayset_batch(a, (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

int hr_rayset_order(const hr_rayset* set, int64_t first, int64_t n, uint64_t seed, uint64_t epoch, int64_t* elements_dev, void* stream)
{
    if (int rc = check_rows(set, first, n, "hr_rayset_order")) return rc;
    if (n > 0 && !elements_dev) return fail(HR_E_INVALID, "hr_rayset_order: null argument");
    HrRaySetArgs a = set_args(set, first, n, seed, epoch);
    a.elements = elements_dev;
    hr_launch_rayset_batch(a, (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

int hr_rayset_sample(const hr_rayset* set, int64_t n, uint64_t seed, uint64_t step, const uint64_t* step_dev, float* coords_dev, float* rgb_dev,
                     float* weight_dev, int64_t* elements_dev_or_null, void* stream)
{
    if (!set) return fail(HR_E_INVALID, "hr_rayset_sample: null set");
    if (n < 0) return fail(HR_E_INVALID, "hr_rayset_sample: %lld rows", (long long)n);
    if (n > ((int64_t)1 << 38)) return fail(HR_E_INVALID, "hr_rayset_sample: more than 2^38 rows in one call");
    if (n == 0) return HR_OK;              // nothing to launch
    if (!coords_dev && !rgb_dev && !weight_dev && !elements_dev_or_null) return fail(HR_E_INVALID, "hr_rayset_sample: every output is NULL");
    if (set->prefix[set->n_images] < 1) return fail(HR_E_INVALID, "hr_rayset_sample: the set holds no rays to draw from");
    HrRaySetArgs a = set_args(set, 0, n, 0, 0);
    a.coords = coords_dev; a.rgb = rgb_dev; a.weight = weight_dev;
    a.elements = elements_dev_or_null;
    hr_launch_rayset_sample(a, seed, step, step_dev, (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}
