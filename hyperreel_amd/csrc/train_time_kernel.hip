// The sample stage's training kernels for the time-dependent colour modes (shadingMode RGBtLinear / RGBtFourier / RGBIdentity):
// the same source as train_kernel.hip with HR_TRAIN_TIME -- the ray's basis vector is the time basis, basis_mat has 3 nb rows, the
// activation and its derivative are the mode's (hr_train.h).  A translation unit and namespace of its own: the default build's code
// objects stay as they are.  Exports hr_launch_train_time.
#define HR_TRAIN_TIME 1
#include <cstring>
#include "train_kernel.hip"
