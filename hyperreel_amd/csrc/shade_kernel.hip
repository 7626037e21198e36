// The per-sample colour network of the MLP shading modes (hr_shade.h: layout, tiles, the function), one launch for the three Linears.
//
// CDNA4 mapping (that of mlp_kernel.hip, whose fp32 tile layout the weights share)
//   * a workgroup (4 waves) owns a span of HR_SHADE_SPAN rows -- samples of a render chunk, or rows of hr_stage_shade.  It lists the
//     span's live rows in LDS in ascending order (wave ballots and a prefix over the waves' counts: no atomics, the same list every
//     run) and walks the list in tiles of 64, so the MFMA tiles of a sparse chunk are full of live rows; a span without a live row costs
//     the flags' read.  hr_stage_shade's rows are all live.  The tile's activations stay in LDS: the encoded input [64][k0p + 4],
//     overwritten in place by the hidden activations [64][hp + 4] (every wave has read its A fragments before any writes); nothing
//     goes to HBM between the layers;
//   * every GEMM runs on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation).  In the hidden layers wave w owns the
//     16-column tiles w, w + 4, ... (NT of them, any hidden width up to 256: tiles past the width are not stored); in the last Linear
//     (3 outputs, one tile) wave w owns rows 16 w .. 16 w + 15;
//   * A fragments: one ds_read_b128 per 16x16 tile and 4 k-steps, rows padded by 4 floats; B fragments: pre-tiled weights, one
//     coalesced global_load_dwordx4 per tile and 4 k-steps, served from L2;
//   * no atomics; a row's result depends on nothing but the row, so the bits do not depend on the launch's size, on the tile a row
//     falls into or on the rows that share it.
#include "hr_kernels.h"
#include "hr_shade.h"

typedef float floatx4 __attribute__((ext_vector_type(4)));

template <int NT>
__device__ __forceinline__ void hr_shade_accumulate(floatx4 (&acc)[4][NT], const float* __restrict__ src, int stride, int nkt,
                                                    const float4* __restrict__ wp, int tiles_total, const int (&tile)[NT], int lane)
{
    const float* arow = src + (lane & 15) * stride + 4 * (lane >> 4);
    for (int kt = 0; kt < nkt; ++kt) {
        float4 av[4];
        float4 bv[NT];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) av[mt] = *reinterpret_cast<const float4*>(arow + mt * 16 * stride + kt * 16);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = wp[((size_t)kt * tiles_total + tile[nt]) * 64 + lane];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt].x, bv[nt].x, acc[mt][nt], 0, 0, 0);
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt].y, bv[nt].y, acc[mt][nt], 0, 0, 0);
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt].z, bv[nt].z, acc[mt][nt], 0, 0, 0);
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt].w, bv[nt].w, acc[mt][nt], 0, 0, 0);
            }
        }
    }
}

template <int NT>
__global__ __launch_bounds__(256) void hr_shade_kernel(const HrShadeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const HrShadeNet& g = a.net;
    const int S = a.stride;
    float* X = lds;                  // [64][S]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int64_t span0 = (int64_t)blockIdx.x * HR_SHADE_SPAN;

    // ---- the span's live rows, ascending: s_idx[0 .. n_live).  Render chunks: the rows whose flag the export form set (hr_shade_live;
    //      nothing reads the colour of another row); hr_stage_shade: every row
    constexpr int PASSES = HR_SHADE_SPAN / 256;
    __shared__ int s_idx[HR_SHADE_SPAN];
    __shared__ int s_cnt[PASSES * 4];
    unsigned long long bal[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const int64_t row = span0 + p * 256 + tid;
        const bool live = row < a.n_rows && (a.live_col < 0 || a.feat[row * a.feat_ld + a.live_col] != 0.0f);
        bal[p] = __builtin_amdgcn_ballot_w64(live);
        if (lane == 0) s_cnt[p * 4 + wave] = __builtin_popcountll(bal[p]);
    }
    __syncthreads();
    int n_live = 0;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        int before = n_live;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += s_cnt[p * 4 + w];
            n_live += s_cnt[p * 4 + w];
        }
        if ((bal[p] >> lane) & 1ull) s_idx[before + __builtin_popcountll(bal[p] & ((1ull << lane) - 1ull))] = p * 256 + tid;
    }
    __syncthreads();

    for (int t0 = 0; t0 < n_live; t0 += HR_SHADE_TILE_M) {      // (n_live is the same in every lane of the workgroup: the barriers below are uniform)
    // ---- the tile's rows [f | v] -> columns 0 .. 29 (slots past the list's end: zeros)
    for (int i = tid; i < HR_SHADE_TILE_M * (HR_SHADE_FEAT + 3); i += 256) {
        const int r = i / (HR_SHADE_FEAT + 3), c = i - r * (HR_SHADE_FEAT + 3);
        float v = 0.0f;
        if (t0 + r < n_live) {
            const int64_t row = span0 + s_idx[t0 + r];
            v = c < HR_SHADE_FEAT ? a.feat[row * a.feat_ld + c] : a.vdir[row * a.vdir_ld + (c - HR_SHADE_FEAT)];
        }
        X[r * S + c] = v;
    }
    __syncthreads();
    // ---- positional encodings -> columns 30 .. k0p - 1
    for (int r = wave * 16; r < wave * 16 + 16; ++r) {
        float* xr = X + r * S;
        for (int c = HR_SHADE_FEAT + 3 + lane; c < g.k0p; c += 64) xr[c] = hr_shade_input(g, c, xr);
    }
    __syncthreads();

    // ---- the two hidden Linears, ReLU
    for (int l = 0; l < 2; ++l) {
        floatx4 acc[4][NT];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = floatx4{0.f, 0.f, 0.f, 0.f};
        int tile[NT], tile_ld[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            tile[nt] = wave + 4 * nt;
            tile_ld[nt] = min(tile[nt], g.nt_h - 1);     // tiles past the width compute a copy of the last one, never stored
        }
        hr_shade_accumulate<NT>(acc, X, S, (l == 0 ? g.k0p : g.hp) / 16, a.wpack[l], g.nt_h, tile_ld, lane);
        __syncthreads();             // every wave has finished reading X
        const float* bias = a.bias[l];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            if (tile[nt] >= g.nt_h) continue;            // (wave-uniform)
            const int col = tile[nt] * 16 + (lane & 15);
            const float b = bias[col];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = acc[mt][nt][r] + b;
                    X[(mt * 16 + 4 * (lane >> 4) + r) * S + col] = v > 0.0f ? v : 0.0f;      // ReLU
                }
            }
        }
        __syncthreads();
    }

    // ---- the last Linear (3 outputs: one tile; wave w owns rows 16 w ..), sigmoid, store
    {
        floatx4 acc = floatx4{0.f, 0.f, 0.f, 0.f};
        const float* arow = X + (wave * 16 + (lane & 15)) * S + 4 * (lane >> 4);
        const float4* wp = a.wpack[2];
        for (int kt = 0; kt < g.hp / 16; ++kt) {
            const float4 av = *reinterpret_cast<const float4*>(arow + kt * 16);
            const float4 bv = wp[(size_t)kt * 64 + lane];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc, 0, 0, 0);
        }
        const int col = lane & 15;
        if (col < 3) {
            const float b = a.bias[2][col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int slot = t0 + wave * 16 + 4 * (lane >> 4) + r;
                if (slot < n_live) a.rgb[(span0 + s_idx[slot]) * 3 + col] = 1.0f / (1.0f + expf(-(acc[r] + b)));     // torch.sigmoid
            }
        }
    }
    __syncthreads();                 // the next tile overwrites X
    }
}

template <int NT>
static bool hr_launch_shade_nt(const HrShadeArgs& a, unsigned blocks, size_t lds, hipStream_t stream)
{
    static HrLdsOptIn opt;
    if (!hr_lds_opt_in(opt, reinterpret_cast<const void*>(&hr_shade_kernel<NT>), lds)) return false;
    hipLaunchKernelGGL(hr_shade_kernel<NT>, dim3(blocks), dim3(256), lds, stream, a);
    return true;
}

bool hr_launch_shade(const HrShadeArgs& a, hipStream_t stream)
{
    if (a.n_rows <= 0) return true;
    const HrShadePlan P = hr_shade_plan(a.net.shading, a.net.view_pe, a.net.fea_pe, a.net.feature_c, 1);
    const unsigned blocks = (unsigned)hr_shade_blocks(a.n_rows);
    switch (P.nt_wave) {
        case 1: return hr_launch_shade_nt<1>(a, blocks, P.lds, stream);
        case 2: return hr_launch_shade_nt<2>(a, blocks, P.lds, stream);
        case 3: return hr_launch_shade_nt<3>(a, blocks, P.lds, stream);
        case 4: return hr_launch_shade_nt<4>(a, blocks, P.lds, stream);
        default: return false;       // refused by hr_model_set_shading_mlp
    }
}
