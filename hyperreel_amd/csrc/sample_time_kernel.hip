// hr_sample_time_kernel (sample_time_kernel.inc) for the time-dependent colour modes and RGBIdentity with the plain density (TD 1), and
// the launcher of both forms.
#include "sample_time_kernel.inc"

bool hr_launch_samples_time_density(const hr_config& cfg, const HrSampleArgs& args, const hr_maps& maps, const HrTimeIO& io, hipStream_t stream);

bool hr_launch_samples_time(const hr_config& cfg, const HrSampleArgs& args, const hr_maps& maps, const HrTimeIO& io, bool density, hipStream_t stream)
{
    if (density) return hr_launch_samples_time_density(cfg, args, maps, io, stream);
    return hr_launch_samples_time_td<1>(cfg, args, maps, io, stream);
}
