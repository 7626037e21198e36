// TEST-ONLY host build of hr_background_coin (hyperreel_amd/csrc/hr_sample_rng.h), so that the CPU suite can check the coin the training
// kernels flip and compare the library's exported host function with it.  Nothing in the product links or loads this file.
#include "../../hyperreel_amd/csrc/hr_sample_rng.h"

extern "C" {

// coins of steps [first, first + n) of `seed`: 1 white, 0 black
void hb_coins(uint64_t seed, uint64_t first, uint64_t n, uint8_t* out)
{
    for (uint64_t i = 0; i < n; ++i) out[i] = (uint8_t)hr_background_coin(seed, first + i);
}

// top bit of the first word of the sampler's row 0 of the same (seed, step): what the coin must NOT be a copy of
void hb_sampler_first_bits(uint64_t seed, uint64_t first, uint64_t n, uint8_t* out)
{
    for (uint64_t i = 0; i < n; ++i) out[i] = (uint8_t)(hr_philox4x32_10(seed, 0, first + i).w[0] >> 31);
}

uint64_t hb_domain(void) { return HR_BG_COIN_DOMAIN; }

}
