// Training image loss on the device: the mean of hr_loss_element's terms over a (B, 3) batch, the unweighted squared error of
// the same batch and, when asked for, d loss / d pred -- one read of pred, gt and weight for all three.
//
// One thread owns four consecutive rays: twelve floats of pred and of gt (three 16-byte loads each where the pointers allow), four weights
// (one 16-byte load), twelve floats of d_pred.  A workgroup of 256 threads covers HR_LOSS_RAYS_PER_BLOCK rays.  The last, partial group of
// a batch and batches whose pointers are not 16-byte aligned take scalar, predicated accesses: nothing outside (B, 3) is read or written.
// Which thread owns which ray does not depend on the alignment, so neither does the order of the sums.
//
// Reduction: fixed order, no atomics.  A thread adds its terms in double in element order; lanes meet in shuffle order, the four waves in
// order; every workgroup writes its slot of the caller's workspace on every call; hr_loss_finish_kernel (one workgroup) adds the slots in
// a fixed order and writes *out.  Two calls give the same bits.
#include "hr_loss.h"

namespace {

// v[0..1] of the 256 threads -> lane 0 of wave 0 holds the sums.  Lanes in shuffle order, then the four waves in order.
__device__ __forceinline__ void block_sum2(double (&v)[2], double (*red)[2])
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_down(v[i], off, 64);
    }
    if ((tid & 63) == 0) {
        red[tid >> 6][0] = v[0];
        red[tid >> 6][1] = v[1];
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) v[i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
    }
}

}  // namespace

// VEC: pred, gt, weight (when given) and d_pred (when given) are 16-byte aligned.  GRAD: d_pred is written.
template <bool VEC, bool GRAD>
__global__ __launch_bounds__(256) void hr_image_loss_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ weight,
                                                            int64_t n_rays, int32_t type, float delta, float s, const float* __restrict__ upstream,
                                                            HrLossPartial* __restrict__ partial, float* __restrict__ d_pred)
{
    __shared__ double red[4][2];
    const int64_t r0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;                // this thread's first ray
    double acc[2] = {0.0, 0.0};
    if (r0 < n_rays) {
        const int n = n_rays - r0 >= 4 ? 4 : (int)(n_rays - r0);                     // rays of this thread inside the batch
        const float up = (GRAD && upstream) ? upstream[0] : 1.0f;
        float p[12], g[12], w[4] = {1.0f, 1.0f, 1.0f, 1.0f}, dp[12];
        if (VEC && n == 4) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const float4 a = *reinterpret_cast<const float4*>(pred + 3 * r0 + 4 * q), b = *reinterpret_cast<const float4*>(gt + 3 * r0 + 4 * q);
                p[4 * q] = a.x; p[4 * q + 1] = a.y; p[4 * q + 2] = a.z; p[4 * q + 3] = a.w;
                g[4 * q] = b.x; g[4 * q + 1] = b.y; g[4 * q + 2] = b.z; g[4 * q + 3] = b.w;
            }
            if (weight) {
                const float4 a = *reinterpret_cast<const float4*>(weight + r0);
                w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = k < n;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    p[3 * k + c] = in ? pred[3 * (r0 + k) + c] : 0.0f;
                    g[3 * k + c] = in ? gt[3 * (r0 + k) + c] : 0.0f;
                }
                if (in && weight) w[k] = weight[r0 + k];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float term, sq, grad;
                hr_loss_element(type, delta, s, p[3 * k + c], g[3 * k + c], w[k], &term, &sq, &grad);
                if (k < n) {
                    acc[0] += (double)term;
                    acc[1] += (double)sq;
                }
                dp[3 * k + c] = grad * up;
            }
        }
        if (GRAD) {
            if (VEC && n == 4) {
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    *reinterpret_cast<float4*>(d_pred + 3 * r0 + 4 * q) = make_float4(dp[4 * q], dp[4 * q + 1], dp[4 * q + 2], dp[4 * q + 3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k < n) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) d_pred[3 * (r0 + k) + c] = dp[3 * k + c];
                    }
                }
            }
        }
    }
    block_sum2(acc, red);
    if (threadIdx.x == 0) {
        partial[blockIdx.x].v[0] = acc[0];
        partial[blockIdx.x].v[1] = acc[1];
    }
}

// One workgroup: thread t adds slots t, t + 256, ... in increasing index, then the 256 sums meet in block_sum2's fixed order.
__global__ __launch_bounds__(256) void hr_loss_finish_kernel(const HrLossPartial* __restrict__ partial, int64_t n_slots, int64_t n_rays,
                                                             hr_loss_out* __restrict__ out)
{
    __shared__ double red[4][2];
    double acc[2] = {0.0, 0.0};
    for (int64_t i = threadIdx.x; i < n_slots; i += 256) {
        acc[0] += partial[i].v[0];
        acc[1] += partial[i].v[1];
    }
    block_sum2(acc, red);
    if (threadIdx.x == 0) hr_loss_result(acc[0], acc[1], n_rays, out);
}

void hr_launch_image_loss(const float* pred, const float* gt, const float* weight, int64_t n_rays, int32_t type, float delta, const float* upstream,
                          hr_loss_out* out, float* d_pred, HrLossPartial* partial, hipStream_t stream)
{
    const int64_t blocks = hr_loss_blocks(n_rays);
    const float s = hr_loss_mean_scale(n_rays);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(gt) | reinterpret_cast<uintptr_t>(weight) |
                           reinterpret_cast<uintptr_t>(d_pred);                      // a NULL pointer constrains nothing
    const bool vec = (bits & 15) == 0;
    const dim3 grid((unsigned)blocks), block(256);
    if (d_pred) {
        if (vec) hipLaunchKernelGGL((hr_image_loss_kernel<true, true>), grid, block, 0, stream, pred, gt, weight, n_rays, type, delta, s, upstream, partial, d_pred);
        else hipLaunchKernelGGL((hr_image_loss_kernel<false, true>), grid, block, 0, stream, pred, gt, weight, n_rays, type, delta, s, upstream, partial, d_pred);
    } else {
        if (vec) hipLaunchKernelGGL((hr_image_loss_kernel<true, false>), grid, block, 0, stream, pred, gt, weight, n_rays, type, delta, s, upstream, partial, d_pred);
        else hipLaunchKernelGGL((hr_image_loss_kernel<false, false>), grid, block, 0, stream, pred, gt, weight, n_rays, type, delta, s, upstream, partial, d_pred);
    }
    hipLaunchKernelGGL(hr_loss_finish_kernel, dim3(1), dim3(256), 0, stream, partial, blocks, n_rays, out);
}
