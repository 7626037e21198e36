/* Layout of hr_maps as C sees it, for tests/test_maps_host.py (against the ctypes struct of hyperreel_amd/plan.py). */
#include <stddef.h>

#include "../../include/hyperreel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
int hm_maps_sizeof(void) { return (int)sizeof(hr_maps); }
int hm_maps_offset(int i)
{
    switch (i) {
        case 0: return (int)offsetof(hr_maps, distances_dev);
        case 1: return (int)offsetof(hr_maps, points_dev);
        case 2: return (int)offsetof(hr_maps, acc_dev);
        default: return -1;
    }
}
#ifdef __cplusplus
}
#endif
