// C ABI, camera rays, light-field rays and the training feed: hr_generate_rays, hr_generate_rays_ndc, hr_generate_rays_fisheye (one set of checks, one
// routine: generate_pixels), hr_generate_rays_lightfield, hr_generate_rays_epi, hr_rayset_* (kernels: rays_kernel.hip; arithmetic: hr_camera.h,
// hr_lightfield.h, hr_sample_rng.h).
// No model handle.  The set owns its device memory; hr_rayset_batch / hr_rayset_order / hr_rayset_sample enqueue one kernel and nothing else.
#include <hip/hip_runtime.h>

#include <vector>

#include "hr_camera.h"
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

// slot i of the set (`what`: "image" / "view") and its subsample rule
static int check_slot(const hr_rayset* set, int i, int every, int offset, const char* who, const char* what)
{
    if (i < 0 || i >= set->n_images) return fail(HR_E_INVALID, "%s: %s %d of %d", who, what, i, set->n_images);
    if (every < 1 || offset < 0) return fail(HR_E_INVALID, "%s: subsample rule every %d, offset %d (every >= 1, offset >= 0)", who, every, offset);
    return HR_OK;
}

// pixels and table entry of image i, then the prefix sums from i on
static int rayset_commit(hr_rayset* set, int i, const HrRayImage& image, const uint8_t* rgb_host_or_dev)
{
    const size_t bytes = (size_t)set->height * set->width * 3;
    HR_HIP(hipMemcpy(set->pixels + (size_t)i * bytes, rgb_host_or_dev, bytes, hipMemcpyDefault));
    set->images[i] = image;
    for (int j = i; j < set->n_images; ++j) {
        const HrRayImage& im = set->images[j];
        set->prefix[j + 1] = set->prefix[j] + (im.every > 0 ? hr_subsample_count(set->width, set->height, im.every, im.offset) : 0);
    }
    HR_HIP(hipMemcpy(set->images_dev + i, &set->images[i], sizeof(HrRayImage), hipMemcpyHostToDevice));
    HR_HIP(hipMemcpy(set->prefix_dev + i, &set->prefix[i], sizeof(int64_t) * (size_t)(set->n_images + 1 - i), hipMemcpyHostToDevice));
    return HR_OK;
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
    if (cam->width != set->width || cam->height != set->height || cam->fx == 0.0f || cam->fy == 0.0f)
        return fail(HR_E_INVALID, "hr_rayset_set_image: bad camera (%d x %d in a set of %d x %d, fx %g, fy %g)", (int)cam->width, (int)cam->height,
                    set->width, set->height, (double)cam->fx, (double)cam->fy);
    if (int rc = check_fisheye(fisheye, "hr_rayset_set_image_fisheye")) return rc;
    HrRayImage im = HrRayImage();
    im.cam = *cam;
    if (!undistorted(fisheye)) { im.fe = *fisheye; im.has_fe = 1; }
    im.every = every; im.offset = offset;
    return rayset_commit(set, i, im, rgb_host_or_dev);
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
