// Stand-alone sample kernel: the sample stage (sample_core.inc) over a head that the MLP kernel left in the HBM
// workspace.  Used where the fused frame kernel (fused_impl.inc) does not apply: diagnostics (hr_render_fields),
// point_prediction cascades, heads too wide for the LDS hand-over, the exact-fp32 MLP.  Body and launch plan: sample_kernel.inc.
#include "sample_kernel.inc"

template <int ZP, bool HALF, int PC, int NB>
__global__ __launch_bounds__(256, (HrGatherTune<ZP, HALF>::MIN_BLOCKS)) void hr_sample_kernel(const hr_config* __restrict__ cfgp, const HrSampleArgs a)
{
    // the configuration lives in device memory (2 KB: too large to index dynamically as a by-value kernel argument
    // without the compiler copying it to scratch); uniform reads of it become scalar loads
    const hr_config& cfg = *cfgp;
#define HR_SAMPLE_MAPS false
#define HR_SAMPLE_MAPS_PTR nullptr
#include "sample_kernel_body.inc"
#undef HR_SAMPLE_MAPS_PTR
#undef HR_SAMPLE_MAPS
}

void hr_launch_samples(const hr_config& cfg, const HrSampleArgs& args, hipStream_t stream)
{
    if (args.n_rays <= 0) return;
    const HrSamplePlan P = hr_sample_plan(cfg, args.planes, args.ca_total, args.nq, args.rows_per_ray, args.n_rays, args.rows_out != nullptr);
    hr_sample_dispatch(P, cfg.grid_dtype == HR_GRID_FP16, [&](auto zp, auto half, auto pc, auto nb) {
        hr_launch_sample_kernel(P, &hr_sample_kernel<zp(), half(), pc(), nb()>, stream, args.cfg_dev, args);
    });
}
