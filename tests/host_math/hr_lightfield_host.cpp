// TEST-ONLY host build of hyperreel_amd/csrc/hr_lightfield.h (the two-plane arithmetic the light-field ray kernels call), so that the
// CPU suite can compare it with the reference's fixtures without a GPU.  Nothing in the product links or loads this file.
#include "../../hyperreel_amd/csrc/hr_lightfield.h"

extern "C" {

int hl_sizeof_lightfield() { return (int)sizeof(hr_lightfield); }

// out[i] = element i of torch.linspace(start, end, steps, dtype=float32)
void hl_linspace(float start, float end, int steps, float* out)
{
    for (int i = 0; i < steps; ++i) out[i] = hr_linspace(start, end, steps, i);
}

// rays (n, 6) for pixels [first, first + n) of the row-major view at (s, t)
void hl_view_rays(const hr_lightfield* lf, float s, float t, int64_t first, int64_t n, float* out)
{
    for (int64_t k = 0; k < n; ++k) {
        const int64_t p = first + k;
        hr_lightfield_ray(*lf, s, t, (int)(p % lf->width), (int)(p / lf->width), out + 6 * k);
    }
}

// rays (n, 6) for rows [first, first + n) of the epipolar slice at (v, t)
void hl_epi_rays(const hr_lightfield* lf, float v, float t, int64_t first, int64_t n, float* out)
{
    for (int64_t k = 0; k < n; ++k) {
        const int64_t p = first + k;
        hr_epi_ray(*lf, v, t, (int)(p % lf->width), (int)(p / lf->width), out + 6 * k);
    }
}

}
