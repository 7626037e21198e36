// The deterministic build (train_det_kernel.hip: 64-bit fixed-point accumulators) of the time-dependent colour modes' training kernels
// (train_time_kernel.hip).  Exports hr_launch_train_time_det.
#define HR_TRAIN_TIME 1
#define HR_TRAIN_DET 1
#include <cstring>
#include "train_kernel.hip"
