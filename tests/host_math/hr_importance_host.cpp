// TEST-ONLY host build of hyperreel_amd/csrc/hr_importance.h (the arithmetic of the importance subsample rule), so that the CPU suite can
// compare it with torch's evaluation of the reference's expression and the GPU suite can build its oracle from it.  Nothing in the
// product links or loads this file.
#include "../../hyperreel_amd/csrc/hr_importance.h"

extern "C" {

// cur, prev: (n, 3) bytes -> out (n) float32
void hi_diff(const uint8_t* cur, const uint8_t* prev, int64_t n, float* out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = hr_importance_diff(cur + 3 * i, prev + 3 * i);
}

void hi_keys(const uint8_t* cur, const uint8_t* prev, int64_t n, uint32_t* out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = hr_importance_key(cur + 3 * i, prev + 3 * i);
}

int64_t hi_rank(int64_t n_pixels, int64_t num_take) { return hr_importance_rank(n_pixels, num_take); }

}
