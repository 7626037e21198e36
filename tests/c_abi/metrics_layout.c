/* Layout of hr_image_scores as C sees it, for tests/test_metrics_host.py (against the ctypes struct of hyperreel_amd/lib.py). */
#include <stddef.h>

#include "../../include/hyperreel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
int hs_scores_sizeof(void) { return (int)sizeof(hr_image_scores); }
int hs_scores_offset(int i)
{
    switch (i) {
        case 0: return (int)offsetof(hr_image_scores, sse);
        case 1: return (int)offsetof(hr_image_scores, ssim_sum);
        default: return -1;
    }
}
int hs_ssim_channels(void) { return (int)(sizeof(((hr_image_scores*)0)->ssim_sum) / sizeof(double)); }
int hs_abi_version(void) { return HR_ABI_VERSION; }
#ifdef __cplusplus
}
#endif
