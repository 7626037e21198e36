// hr_sample_time_kernel (sample_time_kernel.inc) for the time-dependent colour modes and RGBIdentity with the plain density (TD 1).
#include "sample_time_kernel.inc"

bool hr_launch_samples_time(const hr_config& cfg, const HrSampleArgs& args, const hr_maps& maps, const HrTimeIO& io, hipStream_t stream)
{
    return hr_launch_samples_time_td<1>(cfg, args, maps, io, stream);
}
