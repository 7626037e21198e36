// The sample kernel of a model with a time-dependent decode mode (DESIGN 3m; definitions: hr_time_decode.h):
//   shadingMode RGBtLinear | RGBtFourier   the ray's decode matrix is basis_mat folded with the ray's TIME basis (hr_fill_decode_time),
//                                          one matrix per ray in LDS as for SH; the activation is relu(x + 0.5)
//   shadingMode RGBIdentity                RGB's matrix, the activation |x + 0.5|
//   densityMode DensityLinear | Fourier    (TD 3) the ray's density row (hr_fill_density_row) weights the gathered density channels where
//                                          every other model sums them -- whatever the shading (RGB and SH included)
// hr_sample_maps_kernel's statements (sample_kernel_body.inc) with hr_sample_body's TD forms: image, per-ray maps and diagnostics in one
// kernel, every plane class and texel format, the second factor's taps decided at run time (NB 4: a line inside hr_render_frame).  Its own
// template, instantiated per TD in a translation unit each (sample_time_kernel.hip, sample_time_density_kernel.hip): the code objects and
// kernel arguments of hr_sample_kernel, hr_sample_maps_kernel, the frame kernels and the training kernels stay as they are -- the
// descriptor is an argument of this kernel only.
#include "sample_kernel.inc"

template <int ZP, bool HALF, int PC, int TD>
__global__ __launch_bounds__(256, (HrGatherTune<ZP, HALF>::MIN_BLOCKS)) void hr_sample_time_kernel(const hr_config* __restrict__ cfgp, const HrSampleArgs a,
                                                                                                    const hr_maps maps, const HrTimeIO io)
{
    constexpr int NB = 4;
    const hr_config& cfg = *cfgp;
#define HR_SAMPLE_MAPS true
#define HR_SAMPLE_MAPS_PTR (&maps)
#define HR_SAMPLE_TIME TD
#define HR_SAMPLE_TIME_PTR io
#include "sample_kernel_body.inc"
#undef HR_SAMPLE_TIME_PTR
#undef HR_SAMPLE_TIME
#undef HR_SAMPLE_MAPS_PTR
#undef HR_SAMPLE_MAPS
}

// false: the model's density-slot table was made for another plan than this launch's (nothing launched)
template <int TD>
static bool hr_launch_samples_time_td(const hr_config& cfg, const HrSampleArgs& args, const hr_maps& maps, const HrTimeIO& io_in, hipStream_t stream)
{
    if (args.n_rays <= 0) return true;
    const HrSampleFormPlan P = hr_sample_form_plan(cfg, args.planes, args.ca_total, args.nq, args.rows_per_ray, args.n_rays, false, {(TD & 2) != 0 ? HR_SAMPLE_TIME_DENSITY : HR_SAMPLE_TIME, true, false});
    if ((TD & 2) != 0 && io_in.d_slots != P.d_slots) return false;
    HrTimeIO io = io_in;
    io.d_slots = P.d_slots;
    io.d_off = P.x_off;
    hr_sample_dispatch(P, cfg.grid_dtype == HR_GRID_FP16, [&](auto zp, auto half, auto pc, auto nb) {
        if constexpr (decltype(nb)::value == 4)      // (the plan never asks for the line form)
            hr_launch_sample_kernel(P, &hr_sample_time_kernel<zp(), half(), pc(), TD>, stream, args.cfg_dev, args, maps, io);
    });
    return true;
}
