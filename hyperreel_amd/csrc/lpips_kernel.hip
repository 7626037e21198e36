// LPIPS on the device (the definition and the layouts: hr_lpips.h).
//
// Convolution: an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32: every output is one fmaf chain over K that starts at the bias).
// M = the output pixels of BOTH images, N = cout, K = k * k * cin in NHWC im2col order.  A workgroup of four wavefronts owns
// HR_LP_BM x HR_LP_BN = 128 pixels x 64 channels; wavefront (wm, wn) owns 64 x 32 of it as two 32 x 32 accumulators.  Per step of
// HR_LP_BK = 32 of K the workgroup gathers the 128 x 32 activation tile into LDS ([pixel][k], rows of 36 floats: 16-byte aligned and
// off the 32-float period), double-buffered, one barrier per step: the next step's global loads are issued before the current step's
// MFMAs and stored after them.  The weights never pass through LDS: they were packed at create time into the lanes' own order
// (hr_lpips.h), so a lane's 16-byte load is its B operand of four MFMAs, and the next step's are in flight under the current ones.
// Layers with cin % 32 == 0 (all but each net's first) gather with 16-byte loads -- a step of K lies inside one filter tap; the first
// layer gathers value by value from the two (h * w, 3) frames and applies the input scaling, leaving the padding at zero.
//
// Head: sixteen lanes per pixel of a tap, the channels across them, norms and the weighted squared difference in double; every
// workgroup writes its slot, and one last workgroup adds the slots of each tap in a fixed order: no atomics, the same bits on every call.
#include "hr_lpips.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = HR_LP_BM, BN = HR_LP_BN, BK = HR_LP_BK;
constexpr int LDA = BK + 4;                      // floats per LDS row
static_assert(BM == 128 && BN == 64 && BK == 32, "the thread maps below are written for this tile");

__global__ __launch_bounds__(256) void hr_lpips_pack_kernel(const float* __restrict__ w, HrLpLayer l, int64_t n, float* __restrict__ packed)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t s = hr_lp_pack_src(l, i);
    packed[i] = s < 0 ? 0.0f : w[s];
}

// pixel m of the GEMM -> the input row of its window's corner, (image * H + iy0, ix0); m >= M: far outside
__device__ __forceinline__ void pixel_origin(const HrLpConvArgs& a, int m, int M, int& img, int& iy0, int& ix0)
{
    if (m >= M) { img = 0; iy0 = -(1 << 28); ix0 = 0; return; }
    const int per = a.Ho * a.Wo;
    img = m / per;
    const int r = m - img * per;
    const int oy = r / a.Wo, ox = r - oy * a.Wo;
    iy0 = oy * a.stride - a.pad;
    ix0 = ox * a.stride - a.pad;
}

template <bool FIRST>
__global__ __launch_bounds__(256) void hr_lpips_conv_kernel(const HrLpConvArgs a)
{
    __shared__ __attribute__((aligned(16))) float sa[2][BM * LDA];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv & 1, wn = wv >> 1;
    const int M = 2 * a.Ho * a.Wo;
    const int m_block = (int)blockIdx.x * BM;
    const int K = a.k * a.k * a.cin;
    const int nk = (K + BK - 1) / BK;
    const int nt = (int)blockIdx.y * 2 + wn;                                  // this wavefront's tile of 32 channels
    const float4* wp = a.wp + ((int64_t)nt * (nk * 4)) * 64 + lane;           // + g * 64 per K group

    // vector gather: thread -> 16 bytes (q) of four pixels
    const int q = tid & 7, mr = tid >> 3;
    int v_img[4] = {}, v_iy0[4] = {}, v_ix0[4] = {};
    if (!FIRST) {
#pragma unroll
        for (int i = 0; i < 4; ++i) pixel_origin(a, m_block + mr + 32 * i, M, v_img[i], v_iy0[i], v_ix0[i]);
    }
    // scalar gather: thread -> sixteen consecutive k (half a step: kh, the same for a whole wavefront) of one pixel
    const int ml = tid & 127, kh = __builtin_amdgcn_readfirstlane(tid >> 7);
    int f_img = 0, f_iy0 = 0, f_ix0 = 0;
    if (FIRST) pixel_origin(a, m_block + ml, M, f_img, f_iy0, f_ix0);
    const float* f_src = f_img ? a.in2 : a.in;

    float4 stage[4];
    auto gather = [&](int kc) {
        if (!FIRST) {
            const int kk = kc * BK;
            const int tap = kk / a.cin, c0 = kk - tap * a.cin;
            const int ky = tap / a.k, kx = tap - ky * a.k;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int iy = v_iy0[i] + ky, ix = v_ix0[i] + kx;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                    v = *reinterpret_cast<const float4*>(a.in + ((int64_t)(v_img[i] * a.H + iy) * a.W + ix) * a.cin + c0 + 4 * q);
                stage[i] = v;
            }
        } else {
            float* s = reinterpret_cast<float*>(stage);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int kk = kc * BK + kh * 16 + i;                         // wavefront-uniform: decoded on the scalar unit
                const int tap = kk / 3, c = kk - tap * 3;
                const int ky = tap / a.k, kx = tap - ky * a.k;
                const float shift = c == 0 ? -0.030f : (c == 1 ? -0.088f : -0.188f);
                const float scale = c == 0 ? 0.458f : (c == 1 ? 0.448f : 0.450f);
                const int iy = f_iy0 + ky, ix = f_ix0 + kx;
                float v = 0.0f;                                               // the padding, and K's own padding: zero after the scaling
                if (kk < K && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                    const float x = f_src[((int64_t)iy * a.W + ix) * 3 + c];
                    v = ((2.0f * x - 1.0f) - shift) / scale;
                }
                s[i] = v;
            }
        }
    };
    auto scatter = [&](int buf) {
        if (!FIRST) {
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(&sa[buf][(mr + 32 * i) * LDA + 4 * q]) = stage[i];
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(&sa[buf][ml * LDA + kh * 16 + 4 * i]) = stage[i];
        }
    };

    f32x16 acc0, acc1;
    {
        const float b = a.bias[nt * 32 + (lane & 31)];
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = b; acc1[r] = b; }
    }

    float4 bcur[4], bnext[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) { bcur[g] = wp[g * 64]; bnext[g] = bcur[g]; }
    gather(0);
    scatter(0);
    __syncthreads();

    const int arow = (wm * 64 + (lane & 31)) * LDA + 4 * (lane >> 5);
    for (int kc = 0; kc < nk; ++kc) {
        const int buf = kc & 1;
        const bool more = kc + 1 < nk;
        if (more) {
#pragma unroll
            for (int g = 0; g < 4; ++g) bnext[g] = wp[((kc + 1) * 4 + g) * 64];
            gather(kc + 1);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 a0 = *reinterpret_cast<const float4*>(&sa[buf][arow + 8 * g]);
            const float4 a1 = *reinterpret_cast<const float4*>(&sa[buf][arow + 32 * LDA + 8 * g]);
            const float4 b = bcur[g];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b.x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b.y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b.y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b.z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b.z, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b.w, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b.w, acc1, 0, 0, 0);
        }
        if (more) {
            scatter(buf ^ 1);                    // last read during step kc - 1, which every wavefront left at that step's barrier
#pragma unroll
            for (int g = 0; g < 4; ++g) bcur[g] = bnext[g];
        }
        __syncthreads();
    }

    // C/D map of the 32x32 forms: column (channel) = lane & 31, row (pixel) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int n = nt * 32 + (lane & 31);
    const int m0 = m_block + wm * 64 + 4 * (lane >> 5);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2);
        const int ma = m0 + row, mb = ma + 32;
        if (ma < M) a.out[(int64_t)ma * a.cout + n] = fmaxf(acc0[r], 0.0f);
        if (mb < M) a.out[(int64_t)mb * a.cout + n] = fmaxf(acc1[r], 0.0f);
    }
}

// floor-mode max pool of (2, H, W, C) NHWC, four channels per thread: every window lies inside the input
__global__ __launch_bounds__(256) void hr_lpips_pool_kernel(const float4* __restrict__ in, float4* __restrict__ out, int H, int W, int C4, int Ho, int Wo,
                                                            int k, int stride, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C4);
    int64_t p = i / C4;
    const int ox = (int)(p % Wo);
    p /= Wo;
    const int oy = (int)(p % Ho), img = (int)(p / Ho);
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (int dy = 0; dy < k; ++dy) {
        for (int dx = 0; dx < k; ++dx) {
            const float4 v = in[((int64_t)(img * H + oy * stride + dy) * W + ox * stride + dx) * C4 + c];
            m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
        }
    }
    out[i] = m;
}

// v summed over the 16 lanes of a group; a + b == b + a: every lane of the group ends with the same bits
__device__ __forceinline__ double group_sum_all(double v)
{
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// feat: (2, pixels, C) -- the tap of both images; C a multiple of 64, at most 512.  Sixteen lanes per pixel, four pixels per wavefront at
// a time: lane q of a group holds channels 4 (16 j + q) .. + 3, j < NJ = C / 64, as 16-byte loads (NJ a template argument: the taps with
// many pixels have few channels, and keep few registers).  A pixel past the end is all zeros: it adds 0.
template <int NJ>
__global__ __launch_bounds__(256) void hr_lpips_head_kernel(const float* __restrict__ feat, const float* __restrict__ lin, int64_t pixels,
                                                            double* __restrict__ slots)
{
    constexpr int C = NJ * 64;
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane & 15, grp = lane >> 4;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 wl[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) wl[j] = reinterpret_cast<const float4*>(lin)[j * 16 + q];
    double sum = 0.0;                                                         // of this group's pixels, the same in its sixteen lanes
#pragma unroll
    for (int i = 0; i < HR_LP_HEAD_PIX / 16; ++i) {
        const int64_t p = (int64_t)blockIdx.x * HR_LP_HEAD_PIX + i * 16 + wv * 4 + grp;
        const bool live = p < pixels;
        const float4* f0 = reinterpret_cast<const float4*>(feat + (live ? p : 0) * C) + q;
        const float4* f1 = reinterpret_cast<const float4*>(feat + (pixels + (live ? p : 0)) * C) + q;
        float4 x[NJ], y[NJ];
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            x[j] = live ? f0[j * 16] : zero;
            y[j] = live ? f1[j * 16] : zero;
            s0 += ((double)x[j].x * (double)x[j].x + (double)x[j].y * (double)x[j].y) + ((double)x[j].z * (double)x[j].z + (double)x[j].w * (double)x[j].w);
            s1 += ((double)y[j].x * (double)y[j].x + (double)y[j].y * (double)y[j].y) + ((double)y[j].z * (double)y[j].z + (double)y[j].w * (double)y[j].w);
        }
        const double r0 = 1.0 / (sqrt(group_sum_all(s0)) + 1e-10), r1 = 1.0 / (sqrt(group_sum_all(s1)) + 1e-10);
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const double dx = (double)x[j].x * r0 - (double)y[j].x * r1, dy = (double)x[j].y * r0 - (double)y[j].y * r1;
            const double dz = (double)x[j].z * r0 - (double)y[j].z * r1, dw = (double)x[j].w * r0 - (double)y[j].w * r1;
            t += ((double)wl[j].x * (dx * dx) + (double)wl[j].y * (dy * dy)) + ((double)wl[j].z * (dz * dz) + (double)wl[j].w * (dw * dw));
        }
        sum += group_sum_all(t);
    }
    const double g0 = __shfl(sum, 0, 64), g1 = __shfl(sum, 16, 64), g2 = __shfl(sum, 32, 64), g3 = __shfl(sum, 48, 64);
    if (lane == 0) red[wv] = ((g0 + g1) + g2) + g3;
    __syncthreads();
    if (threadIdx.x == 0) slots[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// One workgroup: per tap, thread t adds slots t, t + 256, ... in increasing index, lanes meet in shuffle order, then the four wavefronts in order
__global__ __launch_bounds__(256) void hr_lpips_finish_kernel(const HrLpHeadTaps t, double* __restrict__ out)
{
    __shared__ double red[HR_LP_TAPS][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int k = 0; k < HR_LP_TAPS; ++k) {
        double v = 0.0;
        for (int64_t i = threadIdx.x; i < t.n_slots[k]; i += 256) v += t.slots[k][i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) red[k][wv] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int k = 0; k < HR_LP_TAPS; ++k) {
            const double layer = (((red[k][0] + red[k][1]) + red[k][2]) + red[k][3]) / t.pixels[k];
            out[k] = layer;
            total += layer;
        }
        out[HR_LP_TAPS] = total;
    }
}

}  // namespace

void hr_launch_lpips_pack(const float* w_oihw, const HrLpLayer& l, float* packed, hipStream_t stream)
{
    const int64_t n = hr_lp_packed_elems(l);
    hipLaunchKernelGGL(hr_lpips_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, w_oihw, l, n, packed);
}

void hr_launch_lpips_conv(const HrLpConvArgs& a, bool first, hipStream_t stream)
{
    const int64_t M = 2 * (int64_t)a.Ho * a.Wo;
    const dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)(a.cout / BN));
    if (first) hipLaunchKernelGGL(hr_lpips_conv_kernel<true>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(hr_lpips_conv_kernel<false>, grid, dim3(256), 0, stream, a);
}

void hr_launch_lpips_pool(const float* in, float* out, int H, int W, int C, int Ho, int Wo, int k, int stride, hipStream_t stream)
{
    const int64_t n = 2 * (int64_t)Ho * Wo * (C / 4);
    hipLaunchKernelGGL(hr_lpips_pool_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, reinterpret_cast<const float4*>(in),
                       reinterpret_cast<float4*>(out), H, W, C / 4, Ho, Wo, k, stride, n);
}

void hr_launch_lpips_head(const float* feat, const float* lin, int64_t pixels, int C, double* slots, int64_t n_slots, hipStream_t stream)
{
    const dim3 grid((unsigned)n_slots), block(256);
    switch (C / 64) {                            // every tap of hr_lpips.h's two tables
    case 1: hipLaunchKernelGGL(hr_lpips_head_kernel<1>, grid, block, 0, stream, feat, lin, pixels, slots); break;
    case 2: hipLaunchKernelGGL(hr_lpips_head_kernel<2>, grid, block, 0, stream, feat, lin, pixels, slots); break;
    case 3: hipLaunchKernelGGL(hr_lpips_head_kernel<3>, grid, block, 0, stream, feat, lin, pixels, slots); break;
    case 4: hipLaunchKernelGGL(hr_lpips_head_kernel<4>, grid, block, 0, stream, feat, lin, pixels, slots); break;
    case 6: hipLaunchKernelGGL(hr_lpips_head_kernel<6>, grid, block, 0, stream, feat, lin, pixels, slots); break;
    default: hipLaunchKernelGGL(hr_lpips_head_kernel<8>, grid, block, 0, stream, feat, lin, pixels, slots); break;
    }
}

void hr_launch_lpips_finish(const HrLpHeadTaps& t, double* out, hipStream_t stream)
{
    hipLaunchKernelGGL(hr_lpips_finish_kernel, dim3(1), dim3(256), 0, stream, t, out);
}
