// C ABI, image scores: hr_image_metrics / hr_image_metrics_workspace (kernels: metrics_kernel.hip).  No model handle, no allocation,
// no synchronisation: the call enqueues two kernels on `stream`.
#include <hip/hip_runtime.h>

#include "hr_metrics.h"
#include "hr_model.h"

static_assert(sizeof(hr_image_scores) == sizeof(HrMetricPartial), "a workspace slot has the layout of the result");

size_t hr_image_metrics_workspace(int32_t h, int32_t w)
{
    if (h < 1 || w < 1) return 0;
    const int64_t tiles = hr_metric_tiles(h, w), blocks = hr_metric_sse_blocks(h, w);
    return sizeof(HrMetricPartial) * (size_t)(tiles > blocks ? tiles : blocks);      // one size serves both values of want_ssim
}

int hr_image_metrics(const float* pred_dev, const float* gt_dev, int32_t h, int32_t w, int32_t want_ssim, hr_image_scores* out_dev,
                     void* workspace_dev, void* stream)
{
    if (h < 1 || w < 1) return fail(HR_E_INVALID, "hr_image_metrics: bad image shape %d x %d", (int)h, (int)w);
    if (!pred_dev || !gt_dev || !out_dev || !workspace_dev) return fail(HR_E_INVALID, "hr_image_metrics: null argument");
    if (want_ssim && (h < 2 * HR_MET_R + 1 || w < 2 * HR_MET_R + 1))
        return fail(HR_E_INVALID, "hr_image_metrics: SSIM needs at least 11 x 11 pixels (the 11-tap window), got %d x %d", (int)h, (int)w);
    if (hr_metric_tiles(h, w) > 0x7fffffff || hr_metric_sse_blocks(h, w) > 0x7fffffff) return fail(HR_E_INVALID, "hr_image_metrics: image too large");
    HrMetricPartial* ws = reinterpret_cast<HrMetricPartial*>(workspace_dev);
    double* out = reinterpret_cast<double*>(out_dev);
    if (want_ssim) hr_launch_image_ssim(pred_dev, gt_dev, h, w, ws, out, (hipStream_t)stream);
    else hr_launch_image_sse(pred_dev, gt_dev, h, w, ws, out, (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}
