// Image-loss arithmetic shared by the loss kernel (loss_kernel.hip: hr_image_loss) and, compiled by the host compiler, by the CPU suite
// (tests/host_math/hr_loss_host.cpp): one element of INRSystem.training_step's
//     image_loss = self.loss(results['rgb'] * weight, rgb * weight, **batch)             (nlf/__init__.py:665)
// for the loss modules of losses.py that accept that call (huber | mse | weighted_mse | mae | weighted_mae), and its derivative with
// respect to the prediction in the order torch's autograd forms it.  The library is built with -ffp-contract=off, the host restatement
// too: p*w - g*w is two fp32 products and one fp32 subtraction, as two torch multiplies and the loss's own subtraction are.
#ifndef HR_LOSS_H
#define HR_LOSS_H

#include <math.h>
#include <stdint.h>

#include "../../include/hyperreel_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HR_LOSS_FN __host__ __device__ __forceinline__
#else
#define HR_LOSS_FN static inline
#endif

#define HR_LOSS_RAYS_PER_BLOCK 1024                  // 256 threads x 4 rays: one workspace slot per block

// partial sums of one workgroup: { sum of the terms, sum of (pred - gt)^2 }
struct HrLossPartial {
    double v[2];
};

HR_LOSS_FN int hr_loss_type_valid(int32_t type)
{
    return (type & ~(0xff | HR_LOSS_PREMULTIPLIED)) == 0 && (type & 0xff) <= HR_LOSS_HUBER;
}

// workgroups (= workspace slots) of a call
HR_LOSS_FN int64_t hr_loss_blocks(int64_t n_rays) { return (n_rays + HR_LOSS_RAYS_PER_BLOCK - 1) / HR_LOSS_RAYS_PER_BLOCK; }

// the factor of the mean, 1 / (3 B): torch divides the upstream gradient by the element count in fp32 (mean), or multiplies by
// 2. / numel formed in double and rounded once (mse_loss_backward) -- the same float either way
HR_LOSS_FN float hr_loss_mean_scale(int64_t n_rays) { return (float)(1.0 / (double)(3 * n_rays)); }

HR_LOSS_FN float hr_loss_sign(float d) { return (float)((d > 0.0f) - (d < 0.0f)); }          // sign(0) = 0, as torch

// One element.  p, g: prediction and target; w: the ray's weight (1 when the caller has none); s: hr_loss_mean_scale.
//   premultiplied == 0 (step_loss): d = p*w - g*w, and dd/dp = w;
//   premultiplied != 0 (the reference's call form: p and g already carry the weight): d = p - g, dd/dp = 1; w enters the weighted terms only.
// *term: the element's term of the mean; *sq: (p - g)^2 of the values as passed (psnr_gpu's squared error, metrics.py:37-45);
// *grad: d mean / d p, i.e. s * dterm/dd * dd/dp in the order of torch's backward nodes (loss, then the multiply by the weight).
HR_LOSS_FN void hr_loss_element(int32_t type, float delta, float s, float p, float g, float w, float* term, float* sq, float* grad)
{
    const int pre = (type & HR_LOSS_PREMULTIPLIED) != 0;
    const float e = p - g;
    const float d = pre ? e : p * w - g * w;
    const float c = pre ? 1.0f : w;
    float t, gd;
    switch (type & 0xff) {
        case HR_LOSS_MSE:                                            // nn.MSELoss: (2 / N) * d * grad_out
            t = d * d;
            gd = (2.0f * s) * d;
            break;
        case HR_LOSS_WEIGHTED_MSE:                                   // mean(weight * square(d)): (grad_out / N * weight) * (2 * d)
            t = w * (d * d);
            gd = (s * w) * (2.0f * d);
            break;
        case HR_LOSS_MAE:                                            // nn.L1Loss: grad_out / N * sign(d)
            t = fabsf(d);
            gd = s * hr_loss_sign(d);
            break;
        case HR_LOSS_WEIGHTED_MAE:                                   // mean(weight * abs(d))
            t = w * fabsf(d);
            gd = (s * w) * hr_loss_sign(d);
            break;
        default: {                                                   // HR_LOSS_HUBER, nn.HuberLoss: |d| == delta takes the linear branch
            const float z = fabsf(d);
            t = z < delta ? 0.5f * z * z : delta * (z - 0.5f * delta);
            gd = d <= -delta ? -s * delta : (d >= delta ? s * delta : s * d);
            break;
        }
    }
    *term = t;
    *sq = e * e;
    *grad = gd * c;
}

// the two sums of a call -> *out; the mean is formed in double and rounded once
HR_LOSS_FN void hr_loss_result(double loss_sum, double sse, int64_t n_rays, hr_loss_out* out)
{
    out->loss_sum = loss_sum;
    out->sse = sse;
    out->loss = (float)(loss_sum / (double)(3 * n_rays));
    out->pad = 0.0f;
}

#if defined(__HIPCC__)
void hr_launch_image_loss(const float* pred, const float* gt, const float* weight, int64_t n_rays, int32_t type, float delta, const float* upstream,
                          hr_loss_out* out, float* d_pred, HrLossPartial* partial, hipStream_t stream);
#endif

#endif
