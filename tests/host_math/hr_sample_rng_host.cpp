// TEST-ONLY host build of hyperreel_amd/csrc/hr_sample_rng.h (the draw of hr_rayset_sample), so that the CPU suite can compare it with a
// numpy restatement of Philox4x32-10 and the GPU suite can compare the kernel's elements with it bit for bit.  Nothing in the product
// links or loads this file.
#include "../../hyperreel_amd/csrc/hr_sample_rng.h"

extern "C" {

void hs_philox(uint64_t key, uint64_t ctr_lo, uint64_t ctr_hi, uint32_t* out)
{
    const HrPhilox r = hr_philox4x32_10(key, ctr_lo, ctr_hi);
    for (int i = 0; i < 4; ++i) out[i] = r.w[i];
}

// the 64-bit draws of rows [first, first + n) of step `step`
void hs_draws(uint64_t seed, uint64_t step, uint64_t first, uint64_t n, uint64_t* out)
{
    for (uint64_t i = 0; i < n; ++i) out[i] = hr_sample_draw(seed, step, first + i);
}

// ... and their set elements
void hs_elements(uint64_t size, uint64_t seed, uint64_t step, uint64_t first, uint64_t n, uint64_t* out)
{
    for (uint64_t i = 0; i < n; ++i) out[i] = hr_sample_element(size, seed, step, first + i);
}

}
