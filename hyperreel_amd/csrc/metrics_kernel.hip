// Image scores on the device: the squared-error sum and the SSIM sum of two (h * w, 3) float32 frames, i.e. what the
// reference computes on the host after `.cpu().numpy()` with scikit-image (metrics.py:25-35: peak_signal_noise_ratio(data_range=1),
// structural_similarity(win_size=11, gaussian_weights=True, multichannel=True, data_range=1)).
//
// SSIM kernel: one workgroup per HR_MET_TW x HR_MET_TH tile.  The tile and its 5-pixel halo of BOTH images are read once, as contiguous
// floats of the channel-interleaved rows, into LDS; the squared error of the tile's own pixels comes from those same loads.  A row of
// 42 pixels is 126 floats and is filtered AS floats: the horizontal Gaussian of interleaved data is an 11-tap filter with stride 3, so
// every LDS access of both passes has consecutive lanes on consecutive dwords (no bank conflicts) and the channel is just j % 3.
// Moments are accumulated about a per-tile constant (the tile's centre pixel, per image and channel): variances and the covariance are
// shift-invariant, and uxx - ux * ux no longer cancels where the frame is bright and flat (C2 is 9e-4); the means get the constant back.
// Frames that are not multiples of the tile are handled by predication: nothing outside the two frames is read.
//
// Reduction: fixed order, no float atomics.  Every workgroup writes its slot {sse, S sum per channel} (double) of the caller's workspace on
// every call; hr_metric_finish_kernel (one workgroup) adds the slots in a fixed order in double.  Two calls give the same bits.
#include "hr_metrics.h"

namespace {

constexpr int R = HR_MET_R, TW = HR_MET_TW, TH = HR_MET_TH;
constexpr int SW = TW + 2 * R;                   // staged pixels per row (42)
constexpr int SH = TH + 2 * R;                   // staged rows (26)
constexpr int SF = SW * 3;                       // floats per staged row (126)
constexpr int HF = TW * 3;                       // horizontally filtered floats per row (96)
constexpr int VR = 8;                            // consecutive output rows one thread of the vertical pass owns (its window slides in registers)
static_assert(TH % VR == 0 && (TH / VR) * HF <= 256, "vertical pass: one thread per (column, run of VR rows)");

// exp(-k^2 / (2 * 1.5^2)), k = 0..5, normalised over k = -5..5 in float64 and rounded to float32 (scipy.ndimage's kernel for sigma 1.5, truncate 3.5)
constexpr float G0 = 0.26601171493530273f, G1 = 0.21300554275512695f, G2 = 0.10936068743467331f, G3 = 0.036000773310661316f,
                G4 = 0.0075987582094967365f, G5 = 0.001028380123898387f;
constexpr float C1 = 1e-4f, C2 = 9e-4f;          // (0.01 * data_range)^2, (0.03 * data_range)^2, data_range = 1

// the 11 taps v[0..10]; symmetric pairs first, then small to large
__device__ __forceinline__ float gauss11(const float* v)
{
    float s = G5 * (v[0] + v[10]);
    s = __builtin_fmaf(G4, v[1] + v[9], s);
    s = __builtin_fmaf(G3, v[2] + v[8], s);
    s = __builtin_fmaf(G2, v[3] + v[7], s);
    s = __builtin_fmaf(G1, v[4] + v[6], s);
    return __builtin_fmaf(G0, v[5], s);
}

__device__ __forceinline__ float pick3(const float (&c)[3], int ch) { return ch == 0 ? c[0] : (ch == 1 ? c[1] : c[2]); }

// v[0..3] of the 256 threads -> one slot.  Lanes in shuffle order, then the four waves in order.
__device__ __forceinline__ void block_sum4(double (&v)[4], double (*red)[4], HrMetricPartial* slot)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_down(v[i], off, 64);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) red[tid >> 6][i] = v[i];
    }
    __syncthreads();
    if (tid < 4) slot->v[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

}  // namespace

__global__ __launch_bounds__(256) void hr_image_ssim_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int h, int w, int tiles_x,
                                                            HrMetricPartial* __restrict__ partial)
{
    __shared__ float sx[SH * SF], sy[SH * SF];   // the two staged tiles, shifted by the tile constant
    __shared__ float hm[5][SH * HF];             // horizontally filtered x, y, x*x, y*y, x*y
    __shared__ double red[4][4];
    const int tid = threadIdx.x;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * TW, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * TH;

    // the tile constant: its centre pixel, clamped into the frame (x0 < w and y0 < h by the grid)
    const int yc = min(y0 + TH / 2, h - 1), xc = min(x0 + TW / 2, w - 1);
    const int64_t pc = ((int64_t)yc * w + xc) * 3;
    float cx[3], cy[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { cx[c] = pred[pc + c]; cy[c] = gt[pc + c]; }

    double acc[4] = {0.0, 0.0, 0.0, 0.0};        // sse, S sums of the three channels
    for (int i = tid; i < SH * SF; i += 256) {
        const int r = i / SF, f = i - r * SF;
        const int col = f / 3, ch = f - col * 3;
        const int yy = y0 - R + r, xx = x0 - R + col;
        float a = 0.0f, b = 0.0f;                // outside the frame: never inside the window of a scored pixel
        if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
            const int64_t g = ((int64_t)yy * w + xx) * 3 + ch;
            const float xv = pred[g], yv = gt[g];
            if (r >= R && r < R + TH && col >= R && col < R + TW) {       // the tile's own pixels: no halo, no crop
                const float d = xv - yv;
                acc[0] += (double)(d * d);
            }
            a = xv - pick3(cx, ch);
            b = yv - pick3(cy, ch);
        }
        sx[i] = a;
        sy[i] = b;
    }
    __syncthreads();

    for (int i = tid; i < SH * HF; i += 256) {
        const int r = i / HF, j = i - r * HF;
        const float* px = sx + r * SF + j;
        const float* py = sy + r * SF + j;
        float vx[11], vy[11], p[11];
#pragma unroll
        for (int k = 0; k < 11; ++k) { vx[k] = px[3 * k]; vy[k] = py[3 * k]; }
        hm[0][i] = gauss11(vx);
        hm[1][i] = gauss11(vy);
#pragma unroll
        for (int k = 0; k < 11; ++k) p[k] = vx[k] * vx[k];
        hm[2][i] = gauss11(p);
#pragma unroll
        for (int k = 0; k < 11; ++k) p[k] = vy[k] * vy[k];
        hm[3][i] = gauss11(p);
#pragma unroll
        for (int k = 0; k < 11; ++k) p[k] = vx[k] * vy[k];
        hm[4][i] = gauss11(p);
    }
    __syncthreads();

    if (tid < (TH / VR) * HF) {                  // 192 threads = waves 0..2: the branch is wave-uniform
        const int g = tid / HF, j = tid - g * HF;
        const int col = j / 3, ch = j - col * 3;
        float u[5][VR];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            float v[VR + 2 * R];
#pragma unroll
            for (int q = 0; q < VR + 2 * R; ++q) v[q] = hm[m][(g * VR + q) * HF + j];
#pragma unroll
            for (int o = 0; o < VR; ++o) u[m][o] = gauss11(v + o);
        }
        const float sx_c = pick3(cx, ch), sy_c = pick3(cy, ch);
        const int x = x0 + col;
        const bool x_in = x >= R && x < w - R;
        double s = 0.0;
#pragma unroll
        for (int o = 0; o < VR; ++o) {
            const int y = y0 + g * VR + o;
            const float ux = u[0][o] + sx_c, uy = u[1][o] + sy_c;
            const float vx = u[2][o] - u[0][o] * u[0][o];
            const float vy = u[3][o] - u[1][o] * u[1][o];
            const float vxy = u[4][o] - u[0][o] * u[1][o];
            const float a1 = 2.0f * ux * uy + C1, a2 = 2.0f * vxy + C2;
            const float b1 = ux * ux + uy * uy + C1, b2 = vx + vy + C2;
            const float S = (a1 * a2) / (b1 * b2);
            if (x_in && y >= R && y < h - R) s += (double)S;
        }
        acc[1] = ch == 0 ? s : 0.0;
        acc[2] = ch == 1 ? s : 0.0;
        acc[3] = ch == 2 ? s : 0.0;
    }
    block_sum4(acc, red, partial + blockIdx.x);
}

// want_ssim == 0: the squared-error sum alone, any h, w >= 1.  n floats, HR_MET_SSE_BLOCK per workgroup; VEC: both pointers 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void hr_image_sse_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int64_t n,
                                                           HrMetricPartial* __restrict__ partial)
{
    __shared__ double red[4][4];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * HR_MET_SSE_BLOCK;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (VEC) {
#pragma unroll
        for (int it = 0; it < HR_MET_SSE_BLOCK / 1024; ++it) {
            const int64_t i = base + (int64_t)(it * 256 + tid) * 4;
            if (i + 3 < n) {
                const float4 a = *reinterpret_cast<const float4*>(pred + i), b = *reinterpret_cast<const float4*>(gt + i);
                const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
                acc[0] += (double)(d0 * d0);
                acc[0] += (double)(d1 * d1);
                acc[0] += (double)(d2 * d2);
                acc[0] += (double)(d3 * d3);
            } else {
                for (int64_t k = i; k < n; ++k) {               // the frame's last 1..3 floats
                    const float d = pred[k] - gt[k];
                    acc[0] += (double)(d * d);
                }
            }
        }
    } else {
#pragma unroll
        for (int it = 0; it < HR_MET_SSE_BLOCK / 256; ++it) {
            const int64_t i = base + it * 256 + tid;
            if (i < n) {
                const float d = pred[i] - gt[i];
                acc[0] += (double)(d * d);
            }
        }
    }
    block_sum4(acc, red, partial + blockIdx.x);
}

// One workgroup: thread t adds slots t, t + 256, ... in increasing index, then the 256 sums meet in block_sum4's fixed order.
__global__ __launch_bounds__(256) void hr_metric_finish_kernel(const HrMetricPartial* __restrict__ partial, int64_t n_slots, double* __restrict__ out)
{
    __shared__ double red[4][4];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < n_slots; i += 256) {
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] += partial[i].v[c];
    }
    block_sum4(acc, red, reinterpret_cast<HrMetricPartial*>(out));
}

void hr_launch_image_ssim(const float* pred, const float* gt, int h, int w, HrMetricPartial* partial, double* out, hipStream_t stream)
{
    const int tiles_x = (w + TW - 1) / TW;
    const int64_t tiles = hr_metric_tiles(h, w);
    hipLaunchKernelGGL(hr_image_ssim_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, pred, gt, h, w, tiles_x, partial);
    hipLaunchKernelGGL(hr_metric_finish_kernel, dim3(1), dim3(256), 0, stream, partial, tiles, out);
}

void hr_launch_image_sse(const float* pred, const float* gt, int h, int w, HrMetricPartial* partial, double* out, hipStream_t stream)
{
    const int64_t n = (int64_t)h * w * 3, blocks = hr_metric_sse_blocks(h, w);
    const bool vec = ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(gt)) & 15) == 0;
    if (vec) hipLaunchKernelGGL(hr_image_sse_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, pred, gt, n, partial);
    else hipLaunchKernelGGL(hr_image_sse_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, pred, gt, n, partial);
    hipLaunchKernelGGL(hr_metric_finish_kernel, dim3(1), dim3(256), 0, stream, partial, blocks, out);
}
