// TensoRF's per-sample colour networks (`renderModule` of shadingMode MLP_Fea / MLP: nlf/nets/tensorf_base.py:38-69 MLPRender_Fea,
// :106-135 MLPRender, called at nlf/nets/tensorf_no_sample.py:208-219): ONE statement of the input layout, of the weight tiles the
// shading kernel (shade_kernel.hip) reads, and a scalar float restatement of the function.  Shared by the kernel, by the host packer
// (hr_model_finalize) and, compiled by the plain host compiler, by the CPU suite (tests/host_math/hr_shade_host.cpp).
//
// Function.  For a sample with appearance features f (27, after basis_mat) and view direction v (3):
//   MLP_Fea: in = [f, v, PE(f, fea_pe), PE(v, view_pe)]        MLP: in = [f, v, PE(v, view_pe)]
//   PE(p, F) = cat[sin(q), cos(q)],  q[i * F + j] = p[i] * 2^j  (utils/tensorf_utils.py:232-239; the products are exact in fp32);
//   a PE with F == 0 is left out
//   rgb = sigmoid(L4(relu(L2(relu(L0(in))))))   (Sequential indices 0, 2, 4; hidden width feature_c)
// sin / cos arguments reach 32 |f|: the accurate sinf / cosf, not the hardware's v_sin / v_cos.
//
// Tiles (v_mfma_f32_16x16x4_f32, the layout of hr_mlp_pack.h's fp32 tiles): Linear l computes Y[m][n] = sum_k X[m][k] W[n][k] with
//   wpack[kt][t][lane][s],  kt < Kp / 16, t < nt, s < 4   = W[n = 16 t + (lane & 15)][k = 16 kt + 4 (lane >> 4) + s]
// zero where n or k is beyond the torch matrix.  Kp: the input width padded to 16 (layer 0), the hidden width padded to 16 (layers 1,
// 2); nt: ceil(feature_c / 16) (layers 0, 1), 1 (layer 2: 3 outputs).  Bias: nt * 16 floats, zero padded.
#ifndef HR_SHADE_H
#define HR_SHADE_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/hyperreel_hip.h"
#include "hr_plan.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HR_SHADE_FN __host__ __device__ inline
#else
#define HR_SHADE_FN static inline
#endif

struct HrShadeNet {
    int shading;                 // HR_SHADING_MLP_FEA | HR_SHADING_MLP
    int view_pe, fea_pe, feature_c;
    int k0, k0p, hp, nt_h;       // hr_shade_plan's
};

static inline HrShadeNet hr_shade_net(int shading, const hr_shading_mlp& d)
{
    const int fea_pe = shading == HR_SHADING_MLP_FEA ? d.fea_pe : 0;
    const HrShadePlan P = hr_shade_plan(shading, d.view_pe, fea_pe, d.feature_c, 1);
    return HrShadeNet{shading, d.view_pe, fea_pe, d.feature_c, P.k0, P.k0p, P.hp, P.nt_h};
}

// ---------------------------------------------------------------- input layout
// Column c of the network's input row.  kind: 0 the value itself, 1 its sine, 2 its cosine, 3 padding (zero); src: 0..26 = f[src],
// 27..29 = v[src - 27]; freq: the argument is value * 2^freq
struct HrShadeCol {
    int kind, src, freq;
};
HR_SHADE_FN HrShadeCol hr_shade_column(const HrShadeNet& g, int c)
{
    if (c < HR_SHADE_FEAT + 3) return HrShadeCol{0, c, 0};
    c -= HR_SHADE_FEAT + 3;
    const int nf = HR_SHADE_FEAT * g.fea_pe;       // one half (sin or cos) of PE(f)
    if (c < 2 * nf) {
        const int kind = c < nf ? 1 : 2, q = c < nf ? c : c - nf;
        return HrShadeCol{kind, q / g.fea_pe, q % g.fea_pe};
    }
    c -= 2 * nf;
    const int nv = 3 * g.view_pe;
    if (c < 2 * nv) {
        const int kind = c < nv ? 1 : 2, q = c < nv ? c : c - nv;
        return HrShadeCol{kind, HR_SHADE_FEAT + q / g.view_pe, q % g.view_pe};
    }
    return HrShadeCol{3, 0, 0};
}
// row: the sample's [f 0..26 | v 27..29]
HR_SHADE_FN float hr_shade_input(const HrShadeNet& g, int c, const float* row)
{
    const HrShadeCol col = hr_shade_column(g, c);
    if (col.kind == 3) return 0.0f;
    const float p = row[col.src];
    if (col.kind == 0) return p;
    const float q = p * (float)(1 << col.freq);
    return col.kind == 1 ? sinf(q) : cosf(q);
}

// ---------------------------------------------------------------- weight tiles
struct HrShadeLayer {
    int N, K;                    // the torch matrix (out, in)
    int Kp, nt;                  // padded K, 16-column output tiles
};
HR_SHADE_FN HrShadeLayer hr_shade_layer(const HrShadeNet& g, int l)
{
    if (l == 0) return HrShadeLayer{g.feature_c, g.k0, g.k0p, g.nt_h};
    if (l == 1) return HrShadeLayer{g.feature_c, g.feature_c, g.hp, g.nt_h};
    return HrShadeLayer{3, g.feature_c, g.hp, 1};
}
HR_SHADE_FN size_t hr_shade_tile_floats(const HrShadeLayer& L) { return (size_t)(L.Kp / 16) * L.nt * 64 * 4; }
HR_SHADE_FN size_t hr_shade_tile_index(const HrShadeLayer& L, int kt, int t, int lane, int s) { return ((((size_t)kt * L.nt + t) * 64 + lane) * 4) + s; }
HR_SHADE_FN int hr_shade_tile_n(int t, int lane) { return 16 * t + (lane & 15); }
HR_SHADE_FN int hr_shade_tile_k(int kt, int lane, int s) { return 16 * kt + 4 * (lane >> 4) + s; }

// w (N, K), b (N): the torch tensors -> tiles (hr_shade_tile_floats) and bias (nt * 16)
static inline void hr_shade_pack_layer(const HrShadeLayer& L, const float* w, const float* b, std::vector<float>& tiles, std::vector<float>& bias)
{
    tiles.assign(hr_shade_tile_floats(L), 0.0f);
    for (int kt = 0; kt < L.Kp / 16; ++kt)
        for (int t = 0; t < L.nt; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int s = 0; s < 4; ++s) {
                    const int n = hr_shade_tile_n(t, lane), k = hr_shade_tile_k(kt, lane, s);
                    if (n < L.N && k < L.K) tiles[hr_shade_tile_index(L, kt, t, lane, s)] = w[(size_t)n * L.K + k];
                }
    bias.assign((size_t)L.nt * 16, 0.0f);
    for (int n = 0; n < L.N; ++n) bias[n] = b[n];
}

// ---------------------------------------------------------------- the function, one row, scalar float
// w[l] (out, in) / b[l]: the torch tensors of Sequential indices 0, 2, 4.  Sums run over k in ascending order, one fused multiply-add
// per product, the bias added last (the kernel's accumulators start from zero too).  scratch: 2 * (k0 + feature_c) floats
static inline void hr_shade_row(const HrShadeNet& g, const float* const w[3], const float* const b[3], const float* f, const float* v, float* rgb,
                                float* scratch)
{
    float row[HR_SHADE_FEAT + 3];
    for (int i = 0; i < HR_SHADE_FEAT; ++i) row[i] = f[i];
    for (int i = 0; i < 3; ++i) row[HR_SHADE_FEAT + i] = v[i];
    float* x = scratch;
    float* h0 = x + g.k0;
    float* h1 = h0 + g.feature_c;
    for (int c = 0; c < g.k0; ++c) x[c] = hr_shade_input(g, c, row);
    auto linear = [](const float* W, const float* B, const float* in, int K, int N, float* out, bool relu) {
        for (int n = 0; n < N; ++n) {
            float acc = 0.0f;
            for (int k = 0; k < K; ++k) acc = fmaf(in[k], W[(size_t)n * K + k], acc);
            acc = acc + B[n];
            out[n] = relu ? (acc > 0.0f ? acc : 0.0f) : acc;
        }
    };
    linear(w[0], b[0], x, g.k0, g.feature_c, h0, true);
    linear(w[1], b[1], h0, g.feature_c, g.feature_c, h1, true);
    float o[3];
    linear(w[2], b[2], h1, g.feature_c, 3, o, false);
    for (int i = 0; i < 3; ++i) rgb[i] = 1.0f / (1.0f + expf(-o[i]));
}

#endif  // HR_SHADE_H
