// hr_sample_time_kernel (sample_time_kernel.inc) with a density mode (TD 3: DensityLinear / DensityFourier under any shading the time
// kernel serves).  A translation unit of its own: the two forms compile side by side.
#include "sample_time_kernel.inc"

bool hr_launch_samples_time_density(const hr_config& cfg, const HrSampleArgs& args, const hr_maps& maps, const HrTimeIO& io, hipStream_t stream)
{
    return hr_launch_samples_time_td<3>(cfg, args, maps, io, stream);
}
