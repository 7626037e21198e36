// C ABI, camera rays and the training feed: hr_generate_rays_ndc, hr_rayset_* (kernels: rays_kernel.hip; arithmetic: hr_camera.h).
// No model handle.  The set owns its device memory; hr_rayset_batch / hr_rayset_order enqueue one kernel and nothing else.
#include <hip/hip_runtime.h>

#include <vector>

#include "hr_camera.h"
#include "hr_model.h"

struct HR_HIDDEN hr_rayset {
    int n_images = 0, width = 0, height = 0, ray_dim = 0;
    bool has_ndc = false;
    hr_ndc ndc = {};
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
    a.size = s->prefix[s->n_images];
    a.first = first; a.n = n;
    a.key = hr_perm_key(seed, epoch);
    return a;
}

}  // namespace

int hr_generate_rays_ndc(const hr_camera* cam, const hr_ndc* ndc, int32_t ray_dim, int64_t first_pixel, int64_t n_pixels, float* rays_dev,
                         void* stream)
{
    if (!cam || (n_pixels > 0 && !rays_dev)) return fail(HR_E_INVALID, "hr_generate_rays_ndc: null argument");
    if (ray_dim != 6 && ray_dim != 8) return fail(HR_E_INVALID, "hr_generate_rays_ndc: ray_dim must be 6 or 8");
    if (cam->width < 1 || cam->height < 1 || cam->fx == 0.0f || cam->fy == 0.0f) return fail(HR_E_INVALID, "hr_generate_rays_ndc: bad camera");
    if (first_pixel < 0 || n_pixels < 0 || first_pixel + n_pixels > (int64_t)cam->width * cam->height)
        return fail(HR_E_INVALID, "hr_generate_rays_ndc: pixel range outside the image");
    if (int rc = check_ndc(ndc, "hr_generate_rays_ndc")) return rc;
    if (!ndc) hr_launch_generate_rays(*cam, ray_dim, first_pixel, n_pixels, rays_dev, (hipStream_t)stream);     // the same kernel: the same bits
    else hr_launch_generate_rays_ndc(*cam, ndc, ray_dim, first_pixel, n_pixels, rays_dev, (hipStream_t)stream);
    HR_HIP(hipGetLastError());
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
    s->images.assign((size_t)n_images, HrRayImage());
    s->prefix.assign((size_t)n_images + 1, 0);
    hipError_t e = s->images_dev.alloc(sizeof(HrRayImage) * (size_t)n_images);
    if (e == hipSuccess) e = s->prefix_dev.alloc(sizeof(int64_t) * ((size_t)n_images + 1));
    if (e == hipSuccess) e = s->pixels.alloc((size_t)n_images * height * width * 3);
    if (e == hipSuccess) e = hipMemcpy(s->images_dev, s->images.data(), sizeof(HrRayImage) * (size_t)n_images, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->prefix_dev, s->prefix.data(), sizeof(int64_t) * ((size_t)n_images + 1), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        delete s;
        return fail(HR_E_HIP, "hr_rayset_create: %s", hipGetErrorString(e));
    }
    *out = s;
    return HR_OK;
}

void hr_rayset_destroy(hr_rayset* set) { delete set; }

int hr_rayset_set_image(hr_rayset* set, int32_t i, const hr_camera* cam, int32_t every, int32_t offset, const uint8_t* rgb_host_or_dev)
{
    if (!set || !cam || !rgb_host_or_dev) return fail(HR_E_INVALID, "hr_rayset_set_image: null argument");
    if (i < 0 || i >= set->n_images) return fail(HR_E_INVALID, "hr_rayset_set_image: image %d of %d", (int)i, set->n_images);
    if (every < 1 || offset < 0) return fail(HR_E_INVALID, "hr_rayset_set_image: subsample rule every %d, offset %d (every >= 1, offset >= 0)", (int)every, (int)offset);
    if (cam->width != set->width || cam->height != set->height || cam->fx == 0.0f || cam->fy == 0.0f)
        return fail(HR_E_INVALID, "hr_rayset_set_image: bad camera (%d x %d in a set of %d x %d, fx %g, fy %g)", (int)cam->width, (int)cam->height,
                    set->width, set->height, (double)cam->fx, (double)cam->fy);
    const size_t bytes = (size_t)set->height * set->width * 3;
    HR_HIP(hipMemcpy(set->pixels + (size_t)i * bytes, rgb_host_or_dev, bytes, hipMemcpyDefault));
    set->images[i].cam = *cam;
    set->images[i].every = every;
    set->images[i].offset = offset;
    for (int j = i; j < set->n_images; ++j) {
        const HrRayImage& im = set->images[j];
        set->prefix[j + 1] = set->prefix[j] + (im.every > 0 ? hr_subsample_count(set->width, set->height, im.every, im.offset) : 0);
    }
    HR_HIP(hipMemcpy(set->images_dev + i, &set->images[i], sizeof(HrRayImage), hipMemcpyHostToDevice));
    HR_HIP(hipMemcpy(set->prefix_dev + i, &set->prefix[i], sizeof(int64_t) * (size_t)(set->n_images + 1 - i), hipMemcpyHostToDevice));
    return HR_OK;
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
