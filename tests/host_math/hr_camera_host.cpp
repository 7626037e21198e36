// TEST-ONLY host build of hyperreel_amd/csrc/hr_camera.h (the camera arithmetic the ray kernels call), so that the CPU
// suite can compare it with the reference's fixtures without a GPU.  Nothing in the product links or loads this file.
#include <vector>

#include "../../hyperreel_amd/csrc/hr_camera.h"

extern "C" {

int hc_sizeof_camera() { return (int)sizeof(hr_camera); }
int hc_sizeof_ndc() { return (int)sizeof(hr_ndc); }

// rays (n_pixels, 6) for pixels [first, first + n_pixels) of the row-major image
void hc_pixel_rays(const hr_camera* cam, const hr_ndc* ndc, int64_t first, int64_t n_pixels, float* out)
{
    for (int64_t t = 0; t < n_pixels; ++t) {
        const int64_t p = first + t;
        hr_pixel_ray(*cam, ndc, (int)(p % cam->width), (int)(p / cam->width), out + 6 * t);
    }
}

// the rays of the kept pixels of one image, in order: out (count, 6); returns count
int64_t hc_subsampled_rays(const hr_camera* cam, const hr_ndc* ndc, int every, int offset, float* out)
{
    const int64_t n = hr_subsample_count(cam->width, cam->height, every, offset);
    for (int64_t k = 0; k < n; ++k) {
        int x, y;
        hr_subsample_pixel(cam->width, cam->height, every, offset, k, &x, &y);
        hr_pixel_ray(*cam, ndc, x, y, out + 6 * k);
    }
    return n;
}

int64_t hc_subsample_count(int w, int h, int every, int offset) { return hr_subsample_count(w, h, every, offset); }

// xy (count, 2) int32
void hc_subsample_pixels(int w, int h, int every, int offset, int64_t first, int64_t n, int32_t* xy)
{
    for (int64_t k = 0; k < n; ++k) hr_subsample_pixel(w, h, every, offset, first + k, xy + 2 * k, xy + 2 * k + 1);
}

uint64_t hc_perm_key(uint64_t seed, uint64_t epoch) { return hr_perm_key(seed, epoch); }

void hc_perm(uint64_t n, uint64_t key, uint64_t first, uint64_t count, uint64_t* out)
{
    for (uint64_t i = 0; i < count; ++i) out[i] = hr_perm(n, key, first + i);
}

// number of n in [n_lo, n_hi] for which i -> hr_perm(n, key, i) is NOT a bijection of [0, n) (an image outside, or hit twice)
int64_t hc_perm_not_bijective(uint64_t n_lo, uint64_t n_hi, uint64_t key)
{
    int64_t bad = 0;
    std::vector<unsigned char> seen;
    for (uint64_t n = n_lo; n <= n_hi; ++n) {
        seen.assign(n, 0);
        bool ok = true;
        for (uint64_t i = 0; i < n && ok; ++i) {
            const uint64_t j = hr_perm(n, key, i);
            if (j >= n || seen[j]) ok = false; else seen[j] = 1;
        }
        bad += ok ? 0 : 1;
    }
    return bad;
}

}
