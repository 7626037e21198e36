// Image scores (hr_image_metrics): tile geometry and launchers shared by metrics_kernel.hip and api_metrics.hip.
#ifndef HR_METRICS_H
#define HR_METRICS_H

#include <hip/hip_runtime.h>

#include <cstdint>

// One workgroup of the SSIM kernel owns HR_MET_TW x HR_MET_TH pixels and stages them with a halo of HR_MET_R on every side.
#define HR_MET_R 5                                   // radius of the 11-tap Gaussian (sigma 1.5, truncate 3.5)
#define HR_MET_TW 32
#define HR_MET_TH 16
#define HR_MET_SSE_BLOCK 4096                        // floats per workgroup of the squared-error-only kernel

// partial sums of one workgroup, and the layout of hr_image_scores: { sse, ssim_sum[3] }
struct HrMetricPartial {
    double v[4];
};

// workgroups (= workspace slots) of a call
static inline int64_t hr_metric_tiles(int h, int w)
{
    return (int64_t)((w + HR_MET_TW - 1) / HR_MET_TW) * ((h + HR_MET_TH - 1) / HR_MET_TH);
}
static inline int64_t hr_metric_sse_blocks(int h, int w)
{
    return ((int64_t)h * w * 3 + HR_MET_SSE_BLOCK - 1) / HR_MET_SSE_BLOCK;
}

void hr_launch_image_ssim(const float* pred, const float* gt, int h, int w, HrMetricPartial* partial, double* out, hipStream_t stream);
void hr_launch_image_sse(const float* pred, const float* gt, int h, int w, HrMetricPartial* partial, double* out, hipStream_t stream);

#endif
