// The stand-alone sample kernel's launch plan, shared by sample_kernel.hip (hr_sample_kernel: the image) and sample_maps_kernel.hip
// (hr_sample_maps_kernel: the image and the per-ray maps of hr_render_maps); the kernels' statements are sample_kernel_body.inc.
// Each translation unit instantiates its own kernel template.
#define HR_GATHER_FENCED 1
#include "sample_core.inc"

// Launches the instantiation hr_sample_dispatch picked for plan P (hr_plan.h) with the kernel arguments that follow
template <class K, class... A>
static void hr_launch_sample_kernel(const HrSamplePlan& P, K kernel, hipStream_t stream, const A&... args)
{
    if (P.big_lds) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds);
    hipLaunchKernelGGL(kernel, dim3(P.blocks), dim3(256), P.lds, stream, args...);
}
