/* Layout of hr_lightfield as C sees it, for tests/test_lightfield_host.py (against the ctypes struct of hyperreel_amd/plan.py). */
#include <stddef.h>

#include "../../include/hyperreel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
int hf_lightfield_sizeof(void) { return (int)sizeof(hr_lightfield); }
int hf_lightfield_offset(int i)
{
    switch (i) {
        case 0: return (int)offsetof(hr_lightfield, width);
        case 1: return (int)offsetof(hr_lightfield, height);
        case 2: return (int)offsetof(hr_lightfield, aspect);
        case 3: return (int)offsetof(hr_lightfield, st_scale);
        case 4: return (int)offsetof(hr_lightfield, uv_scale);
        case 5: return (int)offsetof(hr_lightfield, near);
        case 6: return (int)offsetof(hr_lightfield, far);
        default: return -1;
    }
}
int hf_abi_version(void) { return HR_ABI_VERSION; }
#ifdef __cplusplus
}
#endif
