// The stand-alone sample kernel's launch plan, shared by sample_kernel.hip (hr_sample_kernel: the image) and sample_maps_kernel.hip
// (hr_sample_maps_kernel: the image and the per-ray maps of hr_render_maps); the kernels' statements are sample_kernel_body.inc.
// Each translation unit instantiates its own kernel template.
#define HR_GATHER_FENCED 1
#include "sample_core.inc"

static size_t hr_sample_lds_bytes(int nq, int ca_total, int ZP, int rows_per_ray)
{
    const int RPB = 256 / ZP;
    size_t bytes = ((size_t)RPB * rows_per_ray * (nq * 4 + 4) + (size_t)RPB * 3 * ca_total + (ZP > 64 ? 256 : 0)) * sizeof(float);
    return bytes;
}

// What hr_launch_samples chooses for a launch: samples per ray rounded up (ZP), plane class, line form, grid and LDS
struct HrSamplePlan {
    int zp, pclass;
    bool all_lines, big_lds;
    unsigned blocks;
    size_t lds;
};

static HrSamplePlan hr_sample_plan(const hr_config& cfg, const HrSampleArgs& args)
{
    HrSamplePlan P;
    const int ZP = P.zp = hr_round_zp(cfg.z_channels);
    const int RPB = 256 / ZP;
    P.blocks = (unsigned)((args.n_rays + RPB - 1) / RPB);
    P.lds = hr_sample_lds_bytes(args.nq, args.ca_total, ZP, args.rows_per_ray);
    // few samples x many head columns can exceed the 64 KiB a kernel gets by default (e.g. 32 rays x 8 x 64 floats)
    P.big_lds = P.lds > 64 * 1024;
    // the shipped [8, 4, 4] / [8, 0, 0] decompositions get the class-specialised gather of their texel format (sample_core.inc); ZP >= 8
    // keeps a quad inside one ray, video nets additionally need two keyframes
    P.pclass = (args.rows_out == nullptr && (!cfg.video || cfg.num_keyframes >= 2)) ? hr_plane_class(args.planes, args.ca_total, hr_plane_fits_gather) : 0;
    // every second factor a line (static nets; a keyframe net inside hr_render_frame): the gather compiled for two line taps
    P.all_lines = P.pclass != 0;
    for (int j = 0; j < 3; ++j)
        if (args.planes[j].cd4 + args.planes[j].ca4 > 0 && args.planes[j].bw != 1) P.all_lines = false;
    return P;
}

// Launches KERNEL<ZP, HALF, PC, NB> of plan P with the kernel arguments that follow (Z > 256 is rejected by hr_model_create)
#define HR_SAMPLE_DISPATCH(KERNEL, P, cfg, stream, ...) \
    do { \
        const HrSamplePlan& P_ = (P); \
        HR_SAMPLE_DISPATCH_Z_(KERNEL, P_, cfg, stream, __VA_ARGS__); \
    } while (0)
#define HR_SAMPLE_DISPATCH_N_(KERNEL, P_, stream, Z_, H_, C_, N_, ...) \
    do { \
        if (P_.big_lds) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&KERNEL<Z_, H_, C_, N_>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)P_.lds); \
        hipLaunchKernelGGL((KERNEL<Z_, H_, C_, N_>), dim3(P_.blocks), dim3(256), P_.lds, stream, __VA_ARGS__); \
    } while (0)
#define HR_SAMPLE_DISPATCH_T_(KERNEL, P_, stream, Z_, H_, C_, ...) \
    do { \
        if (C_ != 0 && P_.all_lines) HR_SAMPLE_DISPATCH_N_(KERNEL, P_, stream, Z_, H_, C_, (C_ != 0 ? 2 : 4), __VA_ARGS__); \
        else HR_SAMPLE_DISPATCH_N_(KERNEL, P_, stream, Z_, H_, C_, 4, __VA_ARGS__); \
    } while (0)
#define HR_SAMPLE_DISPATCH_H_(KERNEL, P_, stream, Z_, H_, ...) \
    do { \
        if (P_.pclass == 1) HR_SAMPLE_DISPATCH_T_(KERNEL, P_, stream, Z_, H_, 1, __VA_ARGS__); \
        else if (P_.pclass == 2) HR_SAMPLE_DISPATCH_T_(KERNEL, P_, stream, Z_, H_, 2, __VA_ARGS__); \
        else HR_SAMPLE_DISPATCH_T_(KERNEL, P_, stream, Z_, H_, 0, __VA_ARGS__); \
    } while (0)
#define HR_SAMPLE_DISPATCH_ZH_(KERNEL, P_, cfg, stream, Z_, ...) \
    do { \
        if ((cfg).grid_dtype == HR_GRID_FP16) HR_SAMPLE_DISPATCH_H_(KERNEL, P_, stream, Z_, true, __VA_ARGS__); \
        else HR_SAMPLE_DISPATCH_H_(KERNEL, P_, stream, Z_, false, __VA_ARGS__); \
    } while (0)
#define HR_SAMPLE_DISPATCH_Z_(KERNEL, P_, cfg, stream, ...) \
    do { \
        switch (P_.zp) { \
            case 8: HR_SAMPLE_DISPATCH_ZH_(KERNEL, P_, cfg, stream, 8, __VA_ARGS__); break; \
            case 16: HR_SAMPLE_DISPATCH_ZH_(KERNEL, P_, cfg, stream, 16, __VA_ARGS__); break; \
            case 32: HR_SAMPLE_DISPATCH_ZH_(KERNEL, P_, cfg, stream, 32, __VA_ARGS__); break; \
            case 64: HR_SAMPLE_DISPATCH_ZH_(KERNEL, P_, cfg, stream, 64, __VA_ARGS__); break; \
            case 128: HR_SAMPLE_DISPATCH_ZH_(KERNEL, P_, cfg, stream, 128, __VA_ARGS__); break; \
            case 256: HR_SAMPLE_DISPATCH_ZH_(KERNEL, P_, cfg, stream, 256, __VA_ARGS__); break; \
            default: break; \
        } \
    } while (0)
