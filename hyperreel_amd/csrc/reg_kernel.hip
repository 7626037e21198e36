// The reference's TensoRF regulariser (nlf/regularizers/tensorf.py:57-89) over every plane and line of a training step in ONE streaming
// launch: hr_tensorf_reg.  Per (1, C, H, W) tensor the three sums of hr_plane_reg_fwd_kernel (pack_kernels.hip)
//   Sh = sum (x[y] - x[y-1])^2,  Sw = sum (x[x] - x[x-1])^2,  Sl = sum |x|
// and, in the same pass, the gradient of  wh kh Sh + ww kw Sw + wl kl Sl  ADDED to the parameter's gradient buffer -- it is linear in the
// weights and does not depend on the sums, so nothing has to wait for a reduction.  The per-plane path reads each plane twice and writes
// and re-reads a gradient-sized temporary; this reads the plane once from HBM (the rows above and below come from L2: a workgroup's
// 4096 consecutive elements and its neighbours' overlap by one row each side) and read-modify-writes the gradient once.
//
// Mapping: bandwidth-bound, no reuse beyond the neighbouring rows, so no LDS staging.  A workgroup of 256 threads owns HR_REG_BLOCK = 4096
// consecutive elements of ONE tensor (hr_adam_kernel's prefix table); a thread handles 4 consecutive elements of a row per iteration
// with 16-byte loads and stores when W % 4 == 0 and both buffers are 16-byte aligned, one element per iteration otherwise.  The weights
// are read from device memory when the kernel runs (a replayed graph sees the host's last write).  The sums leave the workgroup as three
// plain stores into its own slot of the plan's workspace; a one-workgroup finishing launch adds them in a fixed order in double.  No
// float atomics and nothing to clear: two calls on the same inputs give the same bits.
#include "hr_kernels.h"

namespace {

struct RegCoef {
    float ch, cw, cl;           // weight * static factor of the three terms (0: absent)
    bool tv;                    // any difference term: the neighbours are read
    int add_grad;
};

// one element: x in [0, W), y in [0, H); up / down / left / right are read only where the element has that neighbour
__device__ __forceinline__ float reg_elem(float v, float up, float down, float left, float right, bool has_up, bool has_down, bool has_left,
                                          bool has_right, const RegCoef& k, float& sh, float& sw, float& sl)
{
    float gh = 0.0f, gw = 0.0f;
    if (has_up) { const float d = v - up; sh = __builtin_fmaf(d, d, sh); gh += d; }
    if (has_down) gh -= down - v;
    if (has_left) { const float d = v - left; sw = __builtin_fmaf(d, d, sw); gw += d; }
    if (has_right) gw -= right - v;
    sl += fabsf(v);
    const float sgn = (v > 0.0f) ? 1.0f : ((v < 0.0f) ? -1.0f : 0.0f);
    return k.ch * (2.0f * gh) + k.cw * (2.0f * gw) + k.cl * sgn;
}

__global__ __launch_bounds__(256) void hr_tensorf_reg_kernel(const HrRegBatch b, const float* __restrict__ wts, float* __restrict__ partials,
                                                             const int add_grad)
{
    const int blk = blockIdx.x, tid = threadIdx.x;
    int t = 0;
    while (t + 1 < b.count && blk >= b.first_block[t + 1]) ++t;
    const float* __restrict__ p = b.p[t];
    float* __restrict__ g = b.g[t];
    const int64_t n = b.n[t];
    const int H = b.H[t], W = b.W[t];
    RegCoef k;
    k.ch = b.sh[t] >= 0 ? wts[b.sh[t]] * b.kh[t] : 0.0f;
    k.cw = b.sw[t] >= 0 ? wts[b.sw[t]] * b.kw[t] : 0.0f;
    k.cl = b.sl[t] >= 0 ? wts[b.sl[t]] * b.kl[t] : 0.0f;
    k.tv = b.sh[t] >= 0 || b.sw[t] >= 0;
    k.add_grad = add_grad;
    // where the block starts inside its tensor: 64-bit once per workgroup, 32-bit per element
    const int64_t base = (int64_t)(blk - b.first_block[t]) * HR_REG_BLOCK;
    const int64_t row0 = base / W;
    const unsigned x_base = (unsigned)(base - row0 * W), y_base = (unsigned)(row0 % H);
    const unsigned m = (unsigned)((n - base) < (int64_t)HR_REG_BLOCK ? (n - base) : (int64_t)HR_REG_BLOCK);     // this block's elements (the last one is ragged)
    float sh = 0.0f, sw = 0.0f, sl = 0.0f;
    if (b.vec4[t]) {
        // x_base and m are multiples of 4 here (W % 4 == 0): a thread's four elements lie in one row and never pass the end
#pragma unroll
        for (int it = 0; it < HR_REG_BLOCK / 1024; ++it) {
            const unsigned o = (unsigned)(it * 256 + tid) * 4u;
            if (o >= m) break;
            const unsigned xo = x_base + o, dr = xo / (unsigned)W;
            const int x = (int)(xo - dr * (unsigned)W), y = (int)((y_base + dr) % (unsigned)H);
            const int64_t i = base + o;
            const float4 v4 = *reinterpret_cast<const float4*>(p + i);
            const bool has_up = k.tv && y > 0, has_down = k.tv && y < H - 1;
            float4 u4 = {0.f, 0.f, 0.f, 0.f}, d4 = {0.f, 0.f, 0.f, 0.f};
            float left = 0.0f, right = 0.0f;
            if (has_up) u4 = *reinterpret_cast<const float4*>(p + i - W);
            if (has_down) d4 = *reinterpret_cast<const float4*>(p + i + W);
            if (k.tv && x > 0) left = p[i - 1];
            if (k.tv && x + 4 < W) right = p[i + 4];
            float4 r;
            r.x = reg_elem(v4.x, u4.x, d4.x, left, v4.y, has_up, has_down, k.tv && x > 0, k.tv, k, sh, sw, sl);
            r.y = reg_elem(v4.y, u4.y, d4.y, v4.x, v4.z, has_up, has_down, k.tv, k.tv, k, sh, sw, sl);
            r.z = reg_elem(v4.z, u4.z, d4.z, v4.y, v4.w, has_up, has_down, k.tv, k.tv, k, sh, sw, sl);
            r.w = reg_elem(v4.w, u4.w, d4.w, v4.z, right, has_up, has_down, k.tv, k.tv && x + 4 < W, k, sh, sw, sl);
            if (add_grad) {
                float4 g4 = *reinterpret_cast<const float4*>(g + i);
                g4.x += r.x; g4.y += r.y; g4.z += r.z; g4.w += r.w;
                *reinterpret_cast<float4*>(g + i) = g4;
            }
        }
    } else {
#pragma unroll 4
        for (int it = 0; it < HR_REG_BLOCK / 256; ++it) {
            const unsigned o = (unsigned)(it * 256 + tid);
            if (o >= m) break;
            const unsigned xo = x_base + o, dr = xo / (unsigned)W;
            const int x = (int)(xo - dr * (unsigned)W), y = (int)((y_base + dr) % (unsigned)H);
            const int64_t i = base + o;
            const float v = p[i];
            const bool has_up = k.tv && y > 0, has_down = k.tv && y < H - 1, has_left = k.tv && x > 0, has_right = k.tv && x < W - 1;
            const float up = has_up ? p[i - W] : 0.0f, down = has_down ? p[i + W] : 0.0f;
            const float left = has_left ? p[i - 1] : 0.0f, right = has_right ? p[i + 1] : 0.0f;
            const float r = reg_elem(v, up, down, left, right, has_up, has_down, has_left, has_right, k, sh, sw, sl);
            if (add_grad) g[i] += r;
        }
    }
    for (int d = 32; d > 0; d >>= 1) { sh += __shfl_xor(sh, d, 64); sw += __shfl_xor(sw, d, 64); sl += __shfl_xor(sl, d, 64); }
    __shared__ float part[4][3];
    if ((tid & 63) == 0) { part[tid >> 6][0] = sh; part[tid >> 6][1] = sw; part[tid >> 6][2] = sl; }
    __syncthreads();
    if (tid < 3) partials[(size_t)blk * 3 + tid] = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
}

// loss[0] = sum_s w[s] * loss[1 + s],  loss[1 + s] = sum over the terms of slot s of k * S: one workgroup, every partial added in a
// fixed order (thread-strided, then a tree), in double
__global__ __launch_bounds__(256) void hr_tensorf_reg_finish_kernel(const HrRegBatch b, const float* __restrict__ wts,
                                                                    const float* __restrict__ partials, float* __restrict__ loss)
{
    __shared__ double red[3][256];
    __shared__ double slot_sum[HR_REG_SLOTS];
    const int tid = threadIdx.x;
    if (tid < HR_REG_SLOTS) slot_sum[tid] = 0.0;
    __syncthreads();
    for (int t = 0; t < b.count; ++t) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int k = b.first_block[t] + tid; k < b.first_block[t + 1]; k += 256) {
            s0 += (double)partials[(size_t)k * 3];
            s1 += (double)partials[(size_t)k * 3 + 1];
            s2 += (double)partials[(size_t)k * 3 + 2];
        }
        red[0][tid] = s0; red[1][tid] = s1; red[2][tid] = s2;
        __syncthreads();
        for (int d = 128; d > 0; d >>= 1) {
            if (tid < d) { red[0][tid] += red[0][tid + d]; red[1][tid] += red[1][tid + d]; red[2][tid] += red[2][tid + d]; }
            __syncthreads();
        }
        if (tid == 0) {
            if (b.sh[t] >= 0) slot_sum[b.sh[t]] += (double)b.kh[t] * red[0][0];
            if (b.sw[t] >= 0) slot_sum[b.sw[t]] += (double)b.kw[t] * red[1][0];
            if (b.sl[t] >= 0) slot_sum[b.sl[t]] += (double)b.kl[t] * red[2][0];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double total = 0.0;
        for (int s = 0; s < HR_REG_SLOTS; ++s) {
            total += (double)wts[s] * slot_sum[s];
            loss[1 + s] = (float)slot_sum[s];
        }
        loss[0] = (float)total;
    }
}

}  // namespace

void hr_launch_tensorf_reg(const HrRegBatch& b, const float* weights, float* partials, float* loss, int add_grad, hipStream_t stream)
{
    const int blocks = b.first_block[b.count];
    if (blocks > 0) hipLaunchKernelGGL(hr_tensorf_reg_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, b, weights, partials, add_grad);
    hipLaunchKernelGGL(hr_tensorf_reg_finish_kernel, dim3(1), dim3(256), 0, stream, b, weights, partials, loss);
}
