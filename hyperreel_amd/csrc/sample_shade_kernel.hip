// The sample stage of a model with an MLP shading mode, around the shading kernel (shade_kernel.hip):
//   hr_sample_shade_export_kernel  hr_sample_kernel's statements up to the sample's weight; per sorted sample it writes the 27 appearance
//                                  features (basis_mat folded into the gather, three rows at a time), the view direction and the live flag
//   hr_sample_shade_import_kernel  hr_sample_maps_kernel with the colour of a sample whose exported row is flagged live read from the
//                                  shading kernel's output: affine colour terms, composite, background, global transforms, clamp, maps and
//                                  diagnostics are the statements every other model runs
// Their own templates and translation unit (the precedent of sample_maps_kernel.hip): hr_sample_kernel's and hr_sample_maps_kernel's code
// objects and kernel arguments stay as they are -- the workspace pointers are an argument of these kernels only.  Compiled for the
// generic gather (PC 0, NB 4: what hr_sample_form_plan names for both forms) and at most 64 samples per ray (hr_model_set_shading_mlp).
#include "sample_kernel.inc"

// (the export form at 2 workgroups per SIMD-quad: the float16 gather inside the rolled loop over basis_mat's row triples spills 16
//  registers at the sample kernel's 128)
template <int ZP, bool HALF>
__global__ __launch_bounds__(256, 2) void hr_sample_shade_export_kernel(const hr_config* __restrict__ cfgp, const HrSampleArgs a,
                                                                                                            const HrShadeIO io)
{
    constexpr int PC = 0, NB = 4;
    const hr_config& cfg = *cfgp;
#define HR_SAMPLE_MAPS false
#define HR_SAMPLE_MAPS_PTR nullptr
#define HR_SAMPLE_SHADE 1
#define HR_SAMPLE_SHADE_PTR (&io)
#include "sample_kernel_body.inc"
#undef HR_SAMPLE_SHADE_PTR
#undef HR_SAMPLE_SHADE
#undef HR_SAMPLE_MAPS_PTR
#undef HR_SAMPLE_MAPS
}

template <int ZP, bool HALF>
__global__ __launch_bounds__(256, (HrGatherTune<ZP, HALF>::MIN_BLOCKS)) void hr_sample_shade_import_kernel(const hr_config* __restrict__ cfgp, const HrSampleArgs a,
                                                                                                            const hr_maps maps, const HrShadeIO io)
{
    constexpr int PC = 0, NB = 4;
    const hr_config& cfg = *cfgp;
#define HR_SAMPLE_MAPS true
#define HR_SAMPLE_MAPS_PTR (&maps)
#define HR_SAMPLE_SHADE 2
#define HR_SAMPLE_SHADE_PTR (&io)
#include "sample_kernel_body.inc"
#undef HR_SAMPLE_SHADE_PTR
#undef HR_SAMPLE_SHADE
#undef HR_SAMPLE_MAPS_PTR
#undef HR_SAMPLE_MAPS
}

void hr_launch_samples_shade_export(const hr_config& cfg, const HrSampleArgs& args, float* rows, hipStream_t stream)
{
    if (args.n_rays <= 0) return;
    const HrSampleFormPlan P = hr_sample_form_plan(cfg, args.planes, args.ca_total, args.nq, args.rows_per_ray, args.n_rays, false, HrSampleForm{HR_SAMPLE_SHADE, false, true});
    HrShadeIO io = {};
    io.rows = rows;
    io.m_off = P.x_off;
    hr_sample_dispatch(P, cfg.grid_dtype == HR_GRID_FP16, [&](auto zp, auto half, auto pc, auto nb) {
        if constexpr (pc() == 0 && nb() == 4 && zp() <= HR_SHADE_MAX_Z)
            hr_launch_sample_kernel(P, &hr_sample_shade_export_kernel<zp(), half()>, stream, args.cfg_dev, args, io);
    });
}

void hr_launch_samples_shade_import(const hr_config& cfg, const HrSampleArgs& args, const hr_maps& maps, float* rows, const float* rgbk, hipStream_t stream)
{
    if (args.n_rays <= 0) return;
    const HrSampleFormPlan P = hr_sample_form_plan(cfg, args.planes, args.ca_total, args.nq, args.rows_per_ray, args.n_rays, false, HrSampleForm{HR_SAMPLE_SHADE, true, false});
    HrShadeIO io = {};
    io.rows = rows;
    io.rgbk = rgbk;
    hr_sample_dispatch(P, cfg.grid_dtype == HR_GRID_FP16, [&](auto zp, auto half, auto pc, auto nb) {
        if constexpr (pc() == 0 && nb() == 4 && zp() <= HR_SHADE_MAX_Z)
            hr_launch_sample_kernel(P, &hr_sample_shade_import_kernel<zp(), half()>, stream, args.cfg_dev, args, maps, io);
    });
}
