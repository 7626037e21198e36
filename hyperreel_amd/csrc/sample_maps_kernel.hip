// The sample kernel of hr_render_maps / hr_render_frame_maps: hr_sample_kernel (sample_kernel.hip) plus the ray's depth, expected
// point and opacity (hr_sample_body's MAPS reductions).  Its own template and translation unit: hr_sample_kernel's code objects and
// kernel arguments stay as they are (the maps pointers are an argument of this kernel only), and its instantiations compile in parallel.
#include "sample_kernel.inc"

template <int ZP, bool HALF, int PC, int NB>
__global__ __launch_bounds__(256, (HrGatherTune<ZP, HALF>::MIN_BLOCKS)) void hr_sample_maps_kernel(const hr_config* __restrict__ cfgp, const HrSampleArgs a,
                                                                                                    const hr_maps maps)
{
    // the configuration lives in device memory (2 KB: too large to index dynamically as a by-value kernel argument
    // without the compiler copying it to scratch); uniform reads of it become scalar loads
    const hr_config& cfg = *cfgp;
#define HR_SAMPLE_MAPS true
#define HR_SAMPLE_MAPS_PTR (&maps)
#include "sample_kernel_body.inc"
#undef HR_SAMPLE_MAPS_PTR
#undef HR_SAMPLE_MAPS
}

void hr_launch_samples_maps(const hr_config& cfg, const HrSampleArgs& args, const hr_maps& maps, hipStream_t stream)
{
    if (args.n_rays <= 0) return;
    const HrSamplePlan P = hr_sample_plan(cfg, args.planes, args.ca_total, args.nq, args.rows_per_ray, args.n_rays, args.rows_out != nullptr);
    hr_sample_dispatch(P, cfg.grid_dtype == HR_GRID_FP16, [&](auto zp, auto half, auto pc, auto nb) {
        hr_launch_sample_kernel(P, &hr_sample_maps_kernel<zp(), half(), pc(), nb()>, stream, args.cfg_dev, args, maps);
    });
}
