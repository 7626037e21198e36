// LPIPS v0.1 in eval mode (hr_lpips): the definition, the two backbones as layer tables, every layer's size, the minimum frame,
// the workspace and the packed weight layout.  Plain C++ shared by lpips_kernel.hip, api_lpips.hip and the host build that the CPU tests ask.
//
// Definition.  pred, gt: (h * w, 3) float32 in [0, 1], HWC.  Per value v of channel c:  x = 2 v - 1,  then  (x - shift[c]) / scale[c]
// with shift = (-.030, -.088, -.188), scale = (.458, .448, .450); the first convolution reads this (its zero padding is zero AFTER the
// scaling).  The backbone runs on both images; after each of five ReLUs a "tap" f (C_k channels, H_k x W_k) is taken:
//     n = f / (sqrt(sum_c f^2) + 1e-10)   per image and pixel,      d = (n_pred - n_gt)^2,
//     layer[k] = mean over H_k x W_k of sum_c lin_k[c] d[c],        total = sum_k layer[k].
// alex: conv 3->64 11x11 s4 p2, ReLU, tap, maxpool 3 s2; conv 64->192 5x5 p2, ReLU, tap, maxpool 3 s2; conv 192->384 3x3 p1, ReLU, tap;
//       conv 384->256 3x3 p1, ReLU, tap; conv 256->256 3x3 p1, ReLU, tap.
// vgg:  torchvision VGG-16 features: 3x3 p1 convolutions with ReLU, 2-2-3-3-3 of them with 64 / 128 / 256 / 512 / 512 channels, a tap after
//       the last ReLU of each group and maxpool 2 s2 after the first four taps.
// Pools are floor mode: an odd size drops its last row or column.
#ifndef HR_LPIPS_H
#define HR_LPIPS_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HR_LP_FN __host__ __device__ __forceinline__
#else
#define HR_LP_FN static inline
#endif

#define HR_LP_ALEX 0
#define HR_LP_VGG 1
#define HR_LP_TAPS 5
#define HR_LP_MAX_LAYERS 17                 // vgg: 13 convolutions and 4 pools
#define HR_LP_MAX_CONVS 13

#define HR_LP_CONV 0
#define HR_LP_POOL 1

// the convolution kernel's tile: HR_LP_BM output pixels x HR_LP_BN channels per workgroup, HR_LP_BK of K per step
#define HR_LP_BM 128
#define HR_LP_BN 64
#define HR_LP_BK 32
#define HR_LP_HEAD_PIX 32                   // pixels per workgroup (= per workspace slot) of the head kernel

struct HrLpLayer {
    int kind;                               // HR_LP_CONV (with bias and ReLU) or HR_LP_POOL (max)
    int cin, cout;                          // a pool keeps cin
    int k, stride, pad;
    int tap;                                // the tap taken from this layer's output, or -1
};

HR_LP_FN int hr_lp_net_known(int net) { return net == HR_LP_ALEX || net == HR_LP_VGG; }
HR_LP_FN int hr_lp_n_layers(int net) { return net == HR_LP_ALEX ? 7 : (net == HR_LP_VGG ? 17 : 0); }
HR_LP_FN int hr_lp_n_convs(int net) { return net == HR_LP_ALEX ? 5 : (net == HR_LP_VGG ? 13 : 0); }
HR_LP_FN int hr_lp_min_size(int net) { return net == HR_LP_ALEX ? 31 : 16; }      // the smallest h and w whose every tap is at least 1 x 1

HR_LP_FN HrLpLayer hr_lp_conv(int cin, int cout, int k, int stride, int pad, int tap)
{
    HrLpLayer l = {HR_LP_CONV, cin, cout, k, stride, pad, tap};
    return l;
}
HR_LP_FN HrLpLayer hr_lp_pool(int c, int k, int stride)
{
    HrLpLayer l = {HR_LP_POOL, c, c, k, stride, 0, -1};
    return l;
}

// layer i of `net` (0 <= i < hr_lp_n_layers(net))
HR_LP_FN HrLpLayer hr_lp_layer(int net, int i)
{
    if (net == HR_LP_ALEX) {
        switch (i) {
        case 0: return hr_lp_conv(3, 64, 11, 4, 2, 0);
        case 1: return hr_lp_pool(64, 3, 2);
        case 2: return hr_lp_conv(64, 192, 5, 1, 2, 1);
        case 3: return hr_lp_pool(192, 3, 2);
        case 4: return hr_lp_conv(192, 384, 3, 1, 1, 2);
        case 5: return hr_lp_conv(384, 256, 3, 1, 1, 3);
        default: return hr_lp_conv(256, 256, 3, 1, 1, 4);
        }
    }
    // vgg: groups of 2, 2, 3, 3, 3 convolutions, a pool between groups
    const int group_convs[5] = {2, 2, 3, 3, 3}, group_c[5] = {64, 128, 256, 512, 512};
    int at = 0, cin = 3;
    for (int g = 0; g < 5; ++g) {
        for (int j = 0; j < group_convs[g]; ++j, ++at) {
            if (at == i) return hr_lp_conv(cin, group_c[g], 3, 1, 1, j == group_convs[g] - 1 ? g : -1);
            cin = group_c[g];
        }
        if (g < 4) {
            if (at == i) return hr_lp_pool(cin, 2, 2);
            ++at;
        }
    }
    return hr_lp_pool(0, 1, 1);
}

// one axis through a layer (both kinds: floor)
HR_LP_FN int hr_lp_out_size(const HrLpLayer& l, int in)
{
    const int span = in + 2 * l.pad - l.k;
    return span < 0 ? 0 : span / l.stride + 1;
}

// Sizes of one call.  hs / ws: layer i's output; the workspace: two activation buffers of buf_elems floats (a layer reads one and
// writes the other), then the head's slots, one double per HR_LP_HEAD_PIX pixels of a tap.
struct HrLpPlan {
    int n_layers;
    int hs[HR_LP_MAX_LAYERS], ws[HR_LP_MAX_LAYERS];
    int tap_layer[HR_LP_TAPS];
    int64_t tap_slots[HR_LP_TAPS], tap_slot_at[HR_LP_TAPS];
    int64_t buf_elems;
    int64_t n_slots;
    size_t bytes;
};

// 0: `net` unknown, the frame below the minimum, or so large that a layer's 2 * H * W pixels (both images) pass int32
HR_LP_FN int hr_lp_plan(int net, int h, int w, HrLpPlan* p)
{
    if (!hr_lp_net_known(net) || h < hr_lp_min_size(net) || w < hr_lp_min_size(net)) return 0;
    if (2 * (int64_t)h * (int64_t)w > 0x7fffff00LL) return 0;
    p->n_layers = hr_lp_n_layers(net);
    p->buf_elems = 0;
    p->n_slots = 0;
    int ch = h, cw = w;
    for (int i = 0; i < p->n_layers; ++i) {
        const HrLpLayer l = hr_lp_layer(net, i);
        ch = hr_lp_out_size(l, ch);
        cw = hr_lp_out_size(l, cw);
        if (ch < 1 || cw < 1) return 0;
        p->hs[i] = ch;
        p->ws[i] = cw;
        const int64_t elems = 2 * (int64_t)ch * cw * l.cout;
        if (elems > p->buf_elems) p->buf_elems = elems;
        if (l.tap >= 0) {
            p->tap_layer[l.tap] = i;
            p->tap_slots[l.tap] = ((int64_t)ch * cw + HR_LP_HEAD_PIX - 1) / HR_LP_HEAD_PIX;
            p->tap_slot_at[l.tap] = p->n_slots;
            p->n_slots += p->tap_slots[l.tap];
        }
    }
    p->buf_elems = (p->buf_elems + 63) / 64 * 64;            // the second buffer and the slots start 256-byte aligned
    p->bytes = (size_t)p->buf_elems * 2 * sizeof(float) + (size_t)p->n_slots * sizeof(double);
    return 1;
}

// ---- packed convolution weights: the B operand of v_mfma_f32_32x32x2_f32, as the kernel's lanes read it
// K = k * k * cin in im2col order of NHWC activations, kk = (ky * k + kx) * cin + c, zero-padded to Kp, a multiple of HR_LP_BK.  The packed
// array is [cout / 32][Kp / 8][64 lanes][4]: lane l of channel tile nt and K group g holds W[n = 32 nt + (l & 31)][kk = 8 g + 4 (l >> 5) + j]
// in element j -- one 16-byte load per lane feeds four MFMAs (MFMA j of a group sums kk = 8 g + j from lanes 0..31 and 8 g + 4 + j from
// lanes 32..63; the A operand is read from LDS in the same order).
HR_LP_FN int hr_lp_k(const HrLpLayer& l) { return l.k * l.k * l.cin; }
HR_LP_FN int hr_lp_kp(const HrLpLayer& l) { return (hr_lp_k(l) + HR_LP_BK - 1) / HR_LP_BK * HR_LP_BK; }
HR_LP_FN int64_t hr_lp_packed_elems(const HrLpLayer& l) { return (int64_t)l.cout * hr_lp_kp(l); }

// packed index -> index into the OIHW tensor (cout, cin, k, k) as torch holds it, or -1 for a padding zero
HR_LP_FN int64_t hr_lp_pack_src(const HrLpLayer& l, int64_t dst)
{
    const int j = (int)(dst & 3), lane = (int)((dst >> 2) & 63);
    const int64_t tile = dst >> 8;
    const int groups = hr_lp_kp(l) / 8;
    const int g = (int)(tile % groups), nt = (int)(tile / groups);
    const int n = 32 * nt + (lane & 31), kk = 8 * g + 4 * (lane >> 5) + j;
    if (kk >= hr_lp_k(l)) return -1;
    const int c = kk % l.cin, t = kk / l.cin, kx = t % l.k, ky = t / l.k;
    return (((int64_t)n * l.cin + c) * l.k + ky) * l.k + kx;
}

// ... and the other way: where W[n][c][ky][kx] lands
HR_LP_FN int64_t hr_lp_pack_dst(const HrLpLayer& l, int n, int c, int ky, int kx)
{
    const int kk = (ky * l.k + kx) * l.cin + c;
    const int g = kk >> 3, half = (kk >> 2) & 1, j = kk & 3;
    const int64_t tile = (int64_t)(n >> 5) * (hr_lp_kp(l) / 8) + g;
    return (tile * 64 + (half * 32 + (n & 31))) * 4 + j;
}

#if defined(__HIPCC__)
// ---- launchers (lpips_kernel.hip)
struct HrLpConvArgs {
    const float* in;                        // (2, H, W, cin) NHWC; the first layer: pred (H * W, 3)
    const float* in2;                       // the first layer: gt
    const float4* wp;                       // packed weights
    const float* bias;
    float* out;                             // (2, Ho, Wo, cout) NHWC, after the ReLU
    int H, W, cin, Ho, Wo, cout, k, stride, pad;
};
struct HrLpHeadTaps {
    const double* slots[HR_LP_TAPS];
    int64_t n_slots[HR_LP_TAPS];
    double pixels[HR_LP_TAPS];
};
void hr_launch_lpips_pack(const float* w_oihw, const HrLpLayer& l, float* packed, hipStream_t stream);
void hr_launch_lpips_conv(const HrLpConvArgs& a, bool first, hipStream_t stream);
void hr_launch_lpips_pool(const float* in, float* out, int H, int W, int C, int Ho, int Wo, int k, int stride, hipStream_t stream);
void hr_launch_lpips_head(const float* feat, const float* lin, int64_t pixels, int C, double* slots, int64_t n_slots, hipStream_t stream);
void hr_launch_lpips_finish(const HrLpHeadTaps& t, double* out, hipStream_t stream);
#endif

#endif  // HR_LPIPS_H
