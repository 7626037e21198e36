// TEST-ONLY host build of the fisheye part of hyperreel_amd/csrc/hr_camera.h (hr_fisheye_undistort, hr_pixel_ray_fisheye and what they
// call), so that the CPU suite can hold it to the float64 oracle of tests/fisheye_common.py and the GPU suite can ask the kernels for
// the same bits.  Nothing in the product links or loads this file.
#include "../../hyperreel_amd/csrc/hr_camera.h"

extern "C" {

int hf_sizeof_fisheye() { return (int)sizeof(hr_fisheye); }
int hf_newton_steps() { return HR_FISHEYE_NEWTON_STEPS; }
int hf_invertible(float k1, float k2) { return hr_fisheye_invertible(k1, k2) ? 1 : 0; }

// theta after `steps` Newton steps from theta_d, for n values
void hf_theta(float k1, float k2, const float* theta_d, int64_t n, int steps, float* out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = hr_fisheye_theta(k1, k2, theta_d[i], steps);
}

void hf_tan(const float* x, int64_t n, float* out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = hr_tan_quadrant(x[i]);
}

// xy (n, 2) -> out (n, 2)
void hf_undistort(float k1, float k2, const float* xy, int64_t n, float* out)
{
    for (int64_t i = 0; i < n; ++i) hr_fisheye_undistort(k1, k2, xy[2 * i], xy[2 * i + 1], out + 2 * i, out + 2 * i + 1);
}

// rays (n_pixels, 6) for pixels [first, first + n_pixels) of the row-major image; fe and ndc may be NULL
void hf_pixel_rays(const hr_camera* cam, const hr_fisheye* fe, const hr_ndc* ndc, int64_t first, int64_t n_pixels, float* out)
{
    for (int64_t t = 0; t < n_pixels; ++t) {
        const int64_t p = first + t;
        hr_pixel_ray_fisheye(*cam, fe, ndc, (int)(p % cam->width), (int)(p / cam->width), out + 6 * t);
    }
}

// the pinhole function itself, for the zero pair's bit-for-bit check
void hf_pinhole_rays(const hr_camera* cam, const hr_ndc* ndc, int64_t first, int64_t n_pixels, float* out)
{
    for (int64_t t = 0; t < n_pixels; ++t) {
        const int64_t p = first + t;
        hr_pixel_ray(*cam, ndc, (int)(p % cam->width), (int)(p / cam->width), out + 6 * t);
    }
}

// the rays of the kept pixels of one image, in order: out (count, 6); returns count
int64_t hf_subsampled_rays(const hr_camera* cam, const hr_fisheye* fe, const hr_ndc* ndc, int every, int offset, float* out)
{
    const int64_t n = hr_subsample_count(cam->width, cam->height, every, offset);
    for (int64_t k = 0; k < n; ++k) {
        int x, y;
        hr_subsample_pixel(cam->width, cam->height, every, offset, k, &x, &y);
        hr_pixel_ray_fisheye(*cam, fe, ndc, x, y, out + 6 * k);
    }
    return n;
}

}
