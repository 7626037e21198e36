// C ABI, training image loss: hr_image_loss / hr_image_loss_workspace (kernels: loss_kernel.hip).  No model handle, no allocation,
// no synchronisation: the call enqueues two kernels on `stream`.
#include <hip/hip_runtime.h>

#include "hr_loss.h"
#include "hr_model.h"

size_t hr_image_loss_workspace(int64_t n_rays)
{
    if (n_rays < 1) return 0;
    return sizeof(HrLossPartial) * (size_t)hr_loss_blocks(n_rays);
}

int hr_image_loss(const float* pred_dev, const float* gt_dev, const float* weight_dev, int64_t n_rays, int32_t type, float delta,
                  const float* upstream_dev, hr_loss_out* out_dev, float* d_pred_dev, void* workspace_dev, void* stream)
{
    if (n_rays < 1) return fail(HR_E_INVALID, "hr_image_loss: bad batch size %lld", (long long)n_rays);
    if (!hr_loss_type_valid(type)) return fail(HR_E_INVALID, "hr_image_loss: unknown loss type %d", (int)type);
    if (!pred_dev || !gt_dev || !out_dev || !workspace_dev) return fail(HR_E_INVALID, "hr_image_loss: null argument");
    if ((type & 0xff) == HR_LOSS_HUBER && !(delta > 0.0f)) return fail(HR_E_INVALID, "hr_image_loss: huber needs delta > 0, got %g", (double)delta);
    if (hr_loss_blocks(n_rays) > 0x7fffffff) return fail(HR_E_INVALID, "hr_image_loss: batch too large");
    hr_launch_image_loss(pred_dev, gt_dev, weight_dev, n_rays, type, delta, upstream_dev, out_dev, d_pred_dev,
                         reinterpret_cast<HrLossPartial*>(workspace_dev), (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}
