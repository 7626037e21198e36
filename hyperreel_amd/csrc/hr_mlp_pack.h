// The MLP's weights as the kernels read them: ONE statement of the tile layout, the K order, the row map, the roundings and the
// power-of-two scalings, shared by the host packer (hr_pack_mlp_layer: pack_mlp at finalize and after calibration, api_mlp.hip), the
// device packer of the training step (hr_pack_split_bf16_kernel, pack_kernels.hip) and, compiled by the plain host compiler, the CPU
// suite (tests/host_math/hr_mlp_pack_host.cpp).  IEEE operations and integer arithmetic only: no _Float16, no __bf16, no libm.
//
// Layout.  Linear l computes D[n][m] = sum_k W[n][k] X[m][k] (the "swapped" GEMM: the weights are the MFMA's A operand, a tile of rays
// the B operand).  W[n][k] is the torch matrix (out, in) seen through two maps:
//   K order   kernel index kk -> torch column.  Layer 0: the input features, padded with zeros to k0p = mlp_in rounded up to 16.
//             Skip layers (torch input cat([input, x])): [input padded to k0p | hidden].  Other layers: the hidden index.
//   row map   last layer only: kernel row n = k * P_live + c' is the user's row k * P_user + live_cols[c'] (head columns no stage
//             reads are not computed); rows from N up to the tile boundary are zero, and so is their bias.
// Split arithmetics (bf16x3, f16x3, f16x2, f16f8), the A operand of v_mfma_f32_32x32x16_{f16,bf16}, 16-bit words:
//   wsplit[kt][t][part][lane][j],  kt < Kp/16, t < nt = ceil(N/32), part: 0 = hi, 1 = lo, 64 lanes, j < 8
//     = W'[n = 32 t + (lane & 31)][kk = 16 kt + 8 (lane >> 5) + j],   hi = r(w'), lo = r(w' - hi),  w' = w * 2^s
//   r = bf16 (s = 0) or IEEE half, round to nearest even.  The fp16 modes' s puts the layer's largest |w| into [2^13, 2^14): the
//   weights of these MLPs are ~1/sqrt(fan_in), and unscaled the low half w - half(w) (~2^-12 w) would be a subnormal half with an
//   ABSOLUTE rounding error of 2^-25; scaled, every low half of a weight above max|w| * 2^-16 is normal.  The kernels multiply the
//   accumulator by winv = 2^-s (exact).
//   f16f8: over the HIDDEN k-steps (kt >= kseg: those past the input segment of the first / skip layer, which keeps three f16
//   products) the 16 bytes of a lane's lo part are the fp8 (OCP e4m3) images of the SAME 8 weights its hi part holds:
//   e4m3((w' - half(w')) * 2^6) x 8, then e4m3(w' * 2^-6) x 8.
// Exact fp32 (v_mfma_f32_16x16x4_f32), floats:
//   wpack[kt][t][lane][s],  t < nt = ceil(N/16), s < 4  = W[n = 16 t + (lane & 15)][kk = 16 kt + 4 (lane >> 4) + s]
// Bias: nt * tile_n floats, b[row map] * 2^s (the split kernels' accumulators START from it, in the accumulator's unit), zero padded.
#ifndef HR_MLP_PACK_H
#define HR_MLP_PACK_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/hyperreel_hip.h"
#include "hr_plan.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HR_PACK_FN __host__ __device__ inline
#else
#define HR_PACK_FN static inline
#endif

// ---------------------------------------------------------------- geometry
// Per-sample head columns the path actually reads (hr_model_finalize drops the others from the last Linear): col[c] = position of
// user column c among the live ones, or -1.
struct HrColMap {
    int col[64];
};

// Linear l as the kernels compute it, in output tiles of tile_n features
struct HrMlpLayer {
    int N_user, Kt;          // the torch matrix (out, in)
    int N, Kp, nt;           // rows the kernels compute, padded K, output tiles
    int first, skip, last;
    int mlp_in, k0p;         // input features; padded to a multiple of 16
    int n_out;               // head columns of one MLP row
    int P_user, P_live;
    int live_cols[64];       // last layer: live column c' of a sample -> the user's column
};

static inline int layer_in(const hr_config& c, int l)
{
    if (l == 0) return c.mlp_in;
    return c.mlp_hidden + (((c.mlp_skip_mask >> l) & 1) ? c.mlp_in : 0);
}

static inline int layer_out(const hr_config& c, int l) { return (l == c.mlp_layers - 1) ? samples_per_row(c) * c.preds_per_z : c.mlp_hidden; }

// output features of a tile in `precision` (HR_MLP_*)
static inline int hr_pack_tile_n(int precision) { return precision == HR_MLP_FP32 ? 16 : 32; }

static inline HrMlpLayer mlp_layer(const hr_config& c, int p_live, const HrColMap& map, int l, int tile_n)
{
    HrMlpLayer g = {};
    g.mlp_in = c.mlp_in;
    g.k0p = (c.mlp_in + 15) & ~15;
    g.n_out = samples_per_row(c) * p_live;
    g.P_user = c.preds_per_z;
    g.P_live = p_live;
    for (int i = 0, j = 0; i < g.P_user && i < 64; ++i)
        if (map.col[i] >= 0) g.live_cols[j++] = i;
    g.first = (l == 0);
    g.skip = (c.mlp_skip_mask >> l) & 1;
    g.last = (l == c.mlp_layers - 1);
    g.N_user = layer_out(c, l);
    g.Kt = layer_in(c, l);
    g.N = g.last ? g.n_out : g.N_user;
    g.Kp = g.first ? g.k0p : (g.skip ? g.k0p + c.mlp_hidden : c.mlp_hidden);
    g.nt = (g.N + tile_n - 1) / tile_n;
    return g;
}

// f16f8: the first k-step whose lo part holds fp8 images (Kp / 16: none)
HR_PACK_FN int hr_pack_kseg(const HrMlpLayer& g) { return g.first ? g.Kp / 16 : (g.skip ? g.k0p / 16 : 0); }

// ---------------------------------------------------------------- source index
// the user's row (of the weight matrix and of the bias) behind kernel row n, or -1 (padding)
HR_PACK_FN int hr_pack_bias_row(const HrMlpLayer& g, int n)
{
    if (n >= g.N) return -1;
    return g.last ? (n / g.P_live) * g.P_user + g.live_cols[n % g.P_live] : n;
}

// index into the torch (out, in) matrix of (kernel row n, kernel K index kk), or -1 (a zero of the padding)
HR_PACK_FN int64_t hr_pack_src_index(const HrMlpLayer& g, int n, int kk)
{
    int col = -1;                                                 // torch in-feature index
    if (g.first) {
        if (kk < g.mlp_in) col = kk;
    } else if (g.skip) {
        if (kk < g.k0p) { if (kk < g.mlp_in) col = kk; }
        else col = g.mlp_in + (kk - g.k0p);                       // cat([input, x]), mlp.py:166-168
    } else {
        col = kk;
    }
    const int row = hr_pack_bias_row(g, n);
    return (row >= 0 && col >= 0 && col < g.Kt) ? (int64_t)row * g.Kt + col : -1;
}

// ---------------------------------------------------------------- tile indices
// split tiles: 16-bit word of (k-step kt, output tile t, part, lane, j), and the matrix element (n, kk) it holds
HR_PACK_FN size_t hr_split_tile_index(const HrMlpLayer& g, int kt, int t, int part, int lane, int j) { return (((((size_t)kt * g.nt + t) * 2 + part) * 64 + lane) * 8) + j; }
HR_PACK_FN int hr_split_tile_n(int t, int lane) { return 32 * t + (lane & 31); }
HR_PACK_FN int hr_split_tile_k(int kt, int lane, int j) { return 16 * kt + 8 * (lane >> 5) + j; }
// f16f8, kt >= hr_pack_kseg: BYTE of image `which` (0: the residual's, 1: the weight's) of the same element
HR_PACK_FN size_t hr_f8_tile_byte(const HrMlpLayer& g, int kt, int t, int lane, int j, int which) { return hr_split_tile_index(g, kt, t, 1, lane, 0) * 2 + 8 * which + j; }
// fp32 tiles: float of (kt, t, lane, s) and its element
HR_PACK_FN size_t hr_f32_tile_index(const HrMlpLayer& g, int kt, int t, int lane, int s) { return ((((size_t)kt * g.nt + t) * 64 + lane) * 4) + s; }
HR_PACK_FN int hr_f32_tile_n(int t, int lane) { return 16 * t + (lane & 15); }
HR_PACK_FN int hr_f32_tile_k(int kt, int lane, int s) { return 16 * kt + 4 * (lane >> 4) + s; }

// ---------------------------------------------------------------- conversions (round to nearest even; NaN stays NaN)
HR_PACK_FN uint32_t hr_float_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
HR_PACK_FN float hr_bits_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
// 2^e, -126 <= e <= 127
HR_PACK_FN float hr_exp2i(int e) { return hr_bits_float((uint32_t)(e + 127) << 23); }

HR_PACK_FN uint16_t hr_bf16_rne(float f)
{
    uint32_t u = hr_float_bits(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);   // NaN: quiet, never rounded into -0 / inf
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
HR_PACK_FN float hr_bf16_to_float(uint16_t h) { return hr_bits_float((uint32_t)h << 16); }

// IEEE half; overflow -> infinity like the hardware conversion
HR_PACK_FN uint16_t hr_f16_rne(float f)
{
    const uint32_t u = hr_float_bits(f), a = u & 0x7FFFFFFFu;
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    if (a > 0x7F800000u) return (uint16_t)(sign | 0x7E00u);
    if (a >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);                      // 65520 = the tie between 65504 and 2^16, and beyond
    if (a < 0x38800000u)                                                          // below 2^-14: quantum 2^-24, the ulp of [0.5, 1)
        return (uint16_t)(sign | (hr_float_bits(hr_bits_float(a) + 0.5f) - 0x3F000000u));
    return (uint16_t)(sign | ((a - 0x38000000u + 0xFFFu + ((a >> 13) & 1u)) >> 13));
}
HR_PACK_FN float hr_f16_to_float(uint16_t h)
{
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
    if (e == 0) return hr_bits_float(sign | hr_float_bits((float)m * hr_exp2i(-24)));
    if (e == 31) return hr_bits_float(sign | 0x7F800000u | (m << 13));
    return hr_bits_float(sign | ((e + 112u) << 23) | (m << 13));
}

// OCP e4m3 (what v_mfma_scale_f32_32x32x64_f8f6f4 reads with cbsz / blgp = 0): 1-4-3, bias 7, no infinities, 0x7f = NaN, largest 448
// (beyond it, infinity included: +-448), subnormals down to 2^-9.  The packed weights stay below 2^8 by construction, so nothing
// saturates in the packer.
HR_PACK_FN uint8_t hr_e4m3_rne(float f)
{
    const uint32_t u = hr_float_bits(f), a = u & 0x7FFFFFFFu;
    const uint8_t sign = (uint8_t)((u >> 24) & 0x80u);
    if (a > 0x7F800000u) return 0x7F;
    if (a >= 0x43E00000u) return (uint8_t)(sign | 0x7Eu);                         // 448 and beyond (464, the tie with the NaN code, goes to even = 448)
    if (a < 0x3C800000u)                                                          // below 2^-6: quantum 2^-9, the ulp of [2^14, 2^15)
        return (uint8_t)(sign | (hr_float_bits(hr_bits_float(a) + 16384.0f) - 0x46800000u));
    return (uint8_t)(sign | ((a - 0x3C000000u + 0x7FFFFu + ((a >> 20) & 1u)) >> 20));
}

// ---------------------------------------------------------------- power-of-two scalings
// e of x = f * 2^e, f in [0.5, 1), for a finite x > 0 (a subnormal x: -126, beyond every clamp below)
HR_PACK_FN int hr_frexp_exponent(float x) { return (int)((hr_float_bits(x) >> 23) & 0xFFu) - 126; }
HR_PACK_FN bool hr_positive_finite(float x) { return x > 0.0f && (hr_float_bits(x) & 0x7FFFFFFFu) < 0x7F800000u; }

// fp16 modes: s of the packed weights w * 2^s from the layer's largest |w| (see the layout above); bf16 halves and fp32: 0
HR_PACK_FN int hr_weight_shift(float w_max)
{
    if (!hr_positive_finite(w_max)) return 0;
    const int s = 14 - hr_frexp_exponent(w_max);
    return s < -14 ? -14 : (s > 40 ? 40 : s);
}

// f16 + fp8 split: how far above the calibration's largest activation of a layer the fp8 image of that layer's output still is finite
// (e4m3 keeps 4 significant bits over the 15 octaves below that; the correction products it feeds are 2^-11 of the result)
#define HR_F8_HEADROOM 16.0f
// exponent Ea of the fp8 images e4m3(x * 2^-Ea) of a hidden Linear's output from the calibration's largest |pre-activation| of that
// layer: act_max * HR_F8_HEADROOM <= 448 * 2^Ea, clamped to +-30; 0 without a finite positive maximum
HR_PACK_FN int hr_f8_exponent(float act_max)
{
    const float mx = act_max * HR_F8_HEADROOM;
    if (!hr_positive_finite(mx)) return 0;
    const float q = mx / 448.0f;                             // q = f * 2^e, f in [0.5, 1): mx <= 448 * 2^e
    if (q == 0.0f) return 0;
    const int e = hr_frexp_exponent(q);
    return e < -30 ? -30 : (e > 30 ? 30 : e);
}

// ---------------------------------------------------------------- one element
struct HrSplitPair {
    uint16_t hi, lo;
};
// v = w * 2^s (exact)
HR_PACK_FN HrSplitPair hr_split_bf16(float v)
{
    const uint16_t hi = hr_bf16_rne(v);
    return HrSplitPair{hi, hr_bf16_rne(v - hr_bf16_to_float(hi))};
}
HR_PACK_FN HrSplitPair hr_split_f16(float v)
{
    const uint16_t hi = hr_f16_rne(v);
    return HrSplitPair{hi, hr_f16_rne(v - hr_f16_to_float(hi))};
}
// f16f8, hidden k-steps: the two fp8 images of the element -- [0] of the residual, [1] of the weight
struct HrF8Pair {
    uint8_t image[2];
};
HR_PACK_FN HrF8Pair hr_split_f8(float v) { return HrF8Pair{{hr_e4m3_rne((v - hr_f16_to_float(hr_f16_rne(v))) * 64.0f), hr_e4m3_rne(v * 0.015625f)}}; }
// element (n, kk) of the matrix the tiles hold and element n of its bias, unscaled
HR_PACK_FN float hr_pack_element(const HrMlpLayer& g, const float* w, int n, int kk)
{
    const int64_t at = hr_pack_src_index(g, n, kk);
    return at >= 0 ? w[at] : 0.0f;
}
HR_PACK_FN float hr_pack_bias(const HrMlpLayer& g, const float* b, int n) { return n < g.N ? b[hr_pack_bias_row(g, n)] : 0.0f; }

// ---------------------------------------------------------------- a whole layer, on the host
struct HrPackedLayer {
    std::vector<uint8_t> tiles;      // wsplit (16-bit words) or wpack (floats) as bytes
    std::vector<float> bias;         // nt * tile_n
    float winv;                      // 2^-s
};

// g: mlp_layer(..., hr_pack_tile_n(precision)); w (N_user, Kt), b (N_user): the torch tensors
static inline void hr_pack_mlp_layer(const HrMlpLayer& g, int precision, const std::vector<float>& w, const std::vector<float>& b, HrPackedLayer& out)
{
    const bool split = precision != HR_MLP_FP32, f8lo = precision == HR_MLP_F16F8;
    const bool half = precision == HR_MLP_F16X3 || precision == HR_MLP_F16X2 || f8lo;
    int s = 0;
    if (half) {
        float mx = 0.0f;
        for (float v : w) { const float a = hr_bits_float(hr_float_bits(v) & 0x7FFFFFFFu); mx = (a > mx) ? a : mx; }
        s = hr_weight_shift(mx);
    }
    const float wmul = hr_exp2i(s);
    out.winv = hr_exp2i(-s);
    const int ksteps = g.Kp / 16, kseg = f8lo ? hr_pack_kseg(g) : ksteps;
    out.tiles.assign((size_t)ksteps * g.nt * 64 * (split ? 2 * 8 * sizeof(uint16_t) : 4 * sizeof(float)), 0);
    uint16_t* const words = reinterpret_cast<uint16_t*>(out.tiles.data());
    float* const floats = reinterpret_cast<float*>(out.tiles.data());
    for (int kt = 0; kt < ksteps; ++kt)
        for (int t = 0; t < g.nt; ++t)
            for (int lane = 0; lane < 64; ++lane) {
                if (!split) {
                    for (int e = 0; e < 4; ++e)
                        floats[hr_f32_tile_index(g, kt, t, lane, e)] = hr_pack_element(g, w.data(), hr_f32_tile_n(t, lane), hr_f32_tile_k(kt, lane, e));
                    continue;
                }
                for (int j = 0; j < 8; ++j) {
                    const float v = hr_pack_element(g, w.data(), hr_split_tile_n(t, lane), hr_split_tile_k(kt, lane, j)) * wmul;
                    const HrSplitPair p = half ? hr_split_f16(v) : hr_split_bf16(v);
                    words[hr_split_tile_index(g, kt, t, 0, lane, j)] = p.hi;
                    if (kt < kseg) { words[hr_split_tile_index(g, kt, t, 1, lane, j)] = p.lo; continue; }
                    const HrF8Pair f = hr_split_f8(v);
                    out.tiles[hr_f8_tile_byte(g, kt, t, lane, j, 0)] = f.image[0];
                    out.tiles[hr_f8_tile_byte(g, kt, t, lane, j, 1)] = f.image[1];
                }
            }
    out.bias.assign((size_t)g.nt * hr_pack_tile_n(precision), 0.0f);
    for (int i = 0; i < g.N; ++i) out.bias[i] = hr_pack_bias(g, b.data(), i) * wmul;
}

#endif  // HR_MLP_PACK_H
