// K1 (split-precision form) -- the sample-prediction MLP with every fp32 GEMM evaluated as
// three 16-bit MFMA products (reference: BaseMLP.forward, nlf/nets/mlp.py:159-172).  This file is the body of three
// translation units: mlp_f16x3_kernel.hip (fp16 halves: 11+11 mantissa bits, the default arithmetic wherever the
// activations provably stay below 65504 -- hr_model_finalize checks, DESIGN 3a), mlp_bf16x3_kernel.hip (bf16 halves: the
// fp32 exponent range, 8+8 mantissa bits) and mlp_f16x2_kernel.hip (fp16, weights unsplit).  The text below says
// bf16; HR_SPLIT_E / HR_SPLIT_MFMA / HR_SPLIT_KERNEL / HR_SPLIT_LAUNCH carry the element type.
//
// Why: the fp32-input MFMA (v_mfma_f32_16x16x4_f32) runs at 1/16 of the bf16 MFMA rate, and
// the MLP is 97 % of the FLOPs of a frame.  Writing x = x_hi + x_lo and w = w_hi + w_lo with
// bf16 halves (round-to-nearest-even, lo = bf16(x - hi)) gives
//        x*w = x_hi*w_hi + x_hi*w_lo + x_lo*w_hi + O(2^-18 |x w|)
// and every partial product is exact in the fp32 accumulator of v_mfma_f32_32x32x16_bf16, so
// three bf16 MFMAs reproduce the fp32 GEMM to ~2^-17 relative per product -- measured: raw
// head within 8e-6 (relative to max |head|) of the fp32 chain and RGB within 1e-5 of the
// reference on every model family (tests/test_gpu_parity.py), i.e. >= 10x inside the 1e-4 bar
// -- at 3/16 of the fp32-MFMA issue time.
//
// Structure (per workgroup: 32*MT rays, 4 waves):
//   * "swapped" GEMM: D[n][m] = sum_k W[n][k] X[m][k], weights as the A operand and rays as
//     the B operand.  In the 32x32 accumulator layout a lane then holds 4 consecutive output
//     features of ONE ray per register quad, so the epilogue packs them into one 8-byte LDS
//     store (hi) + one (lo), and the last layer stores 16-byte float4s;
//   * activations live in LDS only, already split: Xh/Xl[32*MT][W+8] bf16 (16-byte row pad ->
//     the 16 rows of a ds_read_b128 lane group fall on distinct bank slots);
//   * weights are split and tiled once by hr_model_finalize into the exact lane order of the
//     MFMA A operand: one coalesced 16-byte load per lane per tile, from L2.  A wave owns
//     64 output features (2 n-tiles) and ALL rays of the workgroup (MT m-tiles), so per 16-wide
//     k-step it issues 4 global loads + 2*MT ds_read_b128 for 6*MT MFMAs.  MT = 4 (128 rays,
//     one workgroup per CU, 128 accumulator VGPRs) halves the weight bytes that cross the
//     CU's vector L1 per MFMA relative to MT = 2 (64 rays, two workgroups per CU);
//   * weights run 3 k-steps ahead of their use in a 4-slot register ring, activations one.
#include <cstdlib>

#ifndef HR_SPLIT_PRODUCTS
#define HR_SPLIT_PRODUCTS 3   // 2: the weights are taken as a single 16-bit value (x_lo*w + x_hi*w), see mlp_f16x2_kernel.hip
#endif

#include "hr_kernels.h"
#include "hr_math.h"

// issue priority inside / outside the MFMA bursts.  Stand-alone MLP kernel: 1 / 0 (the co-resident workgroup's epilogue
// fills the gaps).  Fused frame kernel: 3 / 2 -- the MLP waves are the critical path of a tile, the sample waves of
// the same workgroup (priority 0) take whatever issue slots they leave.
#ifndef HR_MFMA_PRIO_HI
#define HR_MFMA_PRIO_HI 1
#define HR_MFMA_PRIO_LO 0
#endif

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef HR_SPLIT_E bf16x8 __attribute__((ext_vector_type(8)));
typedef HR_SPLIT_E bf16x4 __attribute__((ext_vector_type(4)));

template <int NT>
struct HrWOps {
    bf16x8 h[NT], l[NT];   // weights (A operand), hi/lo halves of NT n-tiles
};
template <int MT>
struct HrXOps {
    bf16x8 h[MT], l[MT];   // activations (B operand), hi/lo halves of MT m-tiles
};

// PR: products of the contraction this operand set is for.  3: x_hi w_hi + x_hi w_lo + x_lo w_hi; 2: the weights are a single
// 16-bit value
constexpr int HR_PR_DEFAULT = HR_SPLIT_PRODUCTS;

template <int NT, int PR = HR_PR_DEFAULT>
__device__ __forceinline__ void hr_load_w(HrWOps<NT>& o, const bf16x8* __restrict__ wp, int wkt, int tiles_total,
                                          const int (&tile)[NT], int lane)
{
#ifdef HR_W_LOAD_AUX       // the weight stream as buffer loads (scalar base + 32-bit lane offsets: no 64-bit address arithmetic per load), with a cache-policy
                           // hint (0 = default, 16 = sc1: past the L1, 2 = nt).  The stand-alone MLP kernels define it as 0 (round 4: K1 -2.6 % on the DoNeRF
                           // frame, -3.5 % on technicolor; sc1 the same, nt slower); the frame kernel keeps flat loads (buffer loads there: 1.99 vs 1.96 ms)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16x8*>(wp), 0, 0x7FFFFFFF, 0x00020000);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int base = ((wkt * tiles_total + tile[nt]) * 2 * 64 + lane) * 16;
        o.h[nt] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, base, 0, HR_W_LOAD_AUX));
        if constexpr (PR == 3) o.l[nt] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, base + 64 * 16, 0, HR_W_LOAD_AUX));
    }
    return;
#endif
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const size_t base = (((size_t)wkt * tiles_total + tile[nt]) * 2) * 64 + lane;
        o.h[nt] = wp[base];
        if constexpr (PR == 3) o.l[nt] = wp[base + 64];
    }
}

template <int MT, int PR = HR_PR_DEFAULT>
__device__ __forceinline__ void hr_load_x(HrXOps<MT>& o, const HR_SPLIT_E* __restrict__ xh, const HR_SPLIT_E* __restrict__ xl,
                                          int stride, int kt, int lane)
{
    const int xoff = (lane & 31) * stride + kt * 16 + 8 * (lane >> 5);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        o.h[mt] = *reinterpret_cast<const bf16x8*>(xh + xoff + mt * 32 * stride);
        if constexpr (PR != 1) o.l[mt] = *reinterpret_cast<const bf16x8*>(xl + xoff + mt * 32 * stride);
    }
}

// 6*MT MFMAs of one k-step; products are the outer loop so that consecutive MFMAs write
// different accumulators (no back-to-back dependent issue)
template <int NT, int MT, int PR = HR_PR_DEFAULT>
__device__ __forceinline__ void hr_mfma3(floatx16 (&acc)[NT][MT], const HrWOps<NT>& w, const HrXOps<MT>& x)
{
    // raised issue priority for the MFMA burst: the co-resident workgroup's epilogue/prologue
    // VALU work then fills the gaps instead of delaying the matrix pipe (measured: 1.483 -> 1.395 ms)
    __builtin_amdgcn_s_setprio(HR_MFMA_PRIO_HI);
    if constexpr (PR == 3) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                acc[nt][mt] = HR_SPLIT_MFMA(w.l[nt], x.h[mt], acc[nt][mt], 0, 0, 0);
    }
    if constexpr (PR != 1) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                acc[nt][mt] = HR_SPLIT_MFMA(w.h[nt], x.l[mt], acc[nt][mt], 0, 0, 0);
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
            acc[nt][mt] = HR_SPLIT_MFMA(w.h[nt], x.h[mt], acc[nt][mt], 0, 0, 0);
    __builtin_amdgcn_s_setprio(HR_MFMA_PRIO_LO);
}

// acc += W[:, segment] * X[segment]^T over NKT (multiple of 4, compile-time) 16-wide k-steps.
// Weights come from L2 (several hundred cycles): a 4-slot register ring keeps them 3 k-steps
// ahead of their use; activations come from LDS and run one step ahead.
template <int NKT, int NT, int MT>
__device__ __forceinline__ void hr_accumulate3_pipe(floatx16 (&acc)[NT][MT], const HR_SPLIT_E* xh, const HR_SPLIT_E* xl, int stride,
                                                    const bf16x8* wp, int kt0, int tiles_total, const int (&tile)[NT], int lane)
{
    static_assert(NKT % 4 == 0 && NKT >= 4, "k-steps must come in fours");
    HrWOps<NT> w0, w1, w2, w3;
    HrXOps<MT> x0, x1;
    hr_load_w<NT>(w0, wp, kt0, tiles_total, tile, lane);
    hr_load_w<NT>(w1, wp, kt0 + 1, tiles_total, tile, lane);
    hr_load_w<NT>(w2, wp, kt0 + 2, tiles_total, tile, lane);
    hr_load_x<MT>(x0, xh, xl, stride, 0, lane);
#pragma unroll 1
    for (int kt = 0; kt < NKT - 4; kt += 4) {
        hr_load_w<NT>(w3, wp, kt0 + kt + 3, tiles_total, tile, lane);
        hr_load_x<MT>(x1, xh, xl, stride, kt + 1, lane);
        hr_mfma3<NT, MT>(acc, w0, x0);
        hr_load_w<NT>(w0, wp, kt0 + kt + 4, tiles_total, tile, lane);
        hr_load_x<MT>(x0, xh, xl, stride, kt + 2, lane);
        hr_mfma3<NT, MT>(acc, w1, x1);
        hr_load_w<NT>(w1, wp, kt0 + kt + 5, tiles_total, tile, lane);
        hr_load_x<MT>(x1, xh, xl, stride, kt + 3, lane);
        hr_mfma3<NT, MT>(acc, w2, x0);
        hr_load_w<NT>(w2, wp, kt0 + kt + 6, tiles_total, tile, lane);
        hr_load_x<MT>(x0, xh, xl, stride, kt + 4, lane);
        hr_mfma3<NT, MT>(acc, w3, x1);
    }
    // last four k-steps: nothing left to prefetch beyond NKT-1
    hr_load_w<NT>(w3, wp, kt0 + NKT - 1, tiles_total, tile, lane);
    hr_load_x<MT>(x1, xh, xl, stride, NKT - 3, lane);
    hr_mfma3<NT, MT>(acc, w0, x0);
    hr_load_x<MT>(x0, xh, xl, stride, NKT - 2, lane);
    hr_mfma3<NT, MT>(acc, w1, x1);
    hr_load_x<MT>(x1, xh, xl, stride, NKT - 1, lane);
    hr_mfma3<NT, MT>(acc, w2, x0);
    hr_mfma3<NT, MT>(acc, w3, x1);
}

// Same contraction with a ring of R weight slots (R-1 k-steps ahead), fully unrolled so that every slot
// index is a compile-time constant.
template <int NKT, int NT, int MT, int R>
__device__ __forceinline__ void hr_accumulate3_ring(floatx16 (&acc)[NT][MT], const HR_SPLIT_E* xh, const HR_SPLIT_E* xl, int stride,
                                                    const bf16x8* wp, int kt0, int tiles_total, const int (&tile)[NT], int lane)
{
    HrWOps<NT> w[R];
    HrXOps<MT> x[2];
#pragma unroll
    for (int i = 0; i < R - 1; ++i)
        if (i < NKT) hr_load_w<NT>(w[i], wp, kt0 + i, tiles_total, tile, lane);
    hr_load_x<MT>(x[0], xh, xl, stride, 0, lane);
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
        if (kt + R - 1 < NKT) hr_load_w<NT>(w[(kt + R - 1) % R], wp, kt0 + kt + R - 1, tiles_total, tile, lane);
        if (kt + 1 < NKT) hr_load_x<MT>(x[(kt + 1) & 1], xh, xl, stride, kt + 1, lane);
        hr_mfma3<NT, MT>(acc, w[kt % R], x[kt & 1]);
    }
}


// The same with ONE activation slot and a rolled loop over pairs of k-steps (two weight slots, one k-step ahead): for a GEMM that
// runs while other accumulators are being held (the frame kernel's last Linear, second pass)
template <int NKT, int NT, int MT>
__device__ __forceinline__ void hr_accumulate3_lean(floatx16 (&acc)[NT][MT], const HR_SPLIT_E* xh, const HR_SPLIT_E* xl, int stride,
                                                    const bf16x8* wp, int kt0, int tiles_total, const int (&tile)[NT], int lane)
{
    static_assert(NKT % 2 == 0, "k-steps in pairs");
    HrWOps<NT> w0, w1;
    HrXOps<MT> x;
    hr_load_w<NT>(w0, wp, kt0, tiles_total, tile, lane);
#pragma unroll 1
    for (int kt = 0; kt < NKT; kt += 2) {
        hr_load_w<NT>(w1, wp, kt0 + kt + 1, tiles_total, tile, lane);
        hr_load_x<MT>(x, xh, xl, stride, kt, lane);
        hr_mfma3<NT, MT>(acc, w0, x);
        hr_load_w<NT>(w0, wp, kt0 + min(kt + 2, NKT - 1), tiles_total, tile, lane);     // (the last one is a re-load: no branch in the loop)
        hr_load_x<MT>(x, xh, xl, stride, kt + 1, lane);
        hr_mfma3<NT, MT>(acc, w1, x);
    }
}

#ifdef HR_SPLIT_F8LO
// ---------------------------------------------------------------------------------------------------------
// f16 + fp8 split (mlp_f16f8_kernel.hip): the leading product x_hi*w_hi stays a v_mfma_f32_32x32x16_f16, the two CORRECTION products
// x*w_lo and x_lo*w_hi -- each 2^-11 of the leading one, so 4 bits of them are bits 12..15 of the result -- go through ONE
// v_mfma_scale_f32_32x32x64_f8f6f4 per PAIR of k-steps: of its K = 64, half the byte positions carry w_lo8 * x8 and the other half
// w_hi8 * x_lo8 over the pair's 32 k, fp8 e4m3, with power-of-two (E8M0) scales putting the sum back into the accumulator's unit.
// Matrix-pipe time per pair and tile: 2 x 32 + 64 = 128 cycles against 6 x 32 = 192 (tools/mfma_f8_ubench.hip: 128.1 / 96.1 ticks per 2 / 1 k-steps).
//
// Operand layout of the K = 64 form, measured (tools/f8_layout_probe.hip, profiles/r04_f8_operand_layout_probe.txt): lane l holds row l % 32; byte j of its
// 32 meets byte j of the other operand's lane with the same l / 32 (bytes 0..15 form block 0, scaled by what lanes 0..31 pass, bytes 16..31 block 1,
// scaled by lanes 32..63).  The images are scaled so that BOTH products need the same factor, which makes the blocks irrelevant: any byte position
// may carry either product as long as the two operands agree.  So the 16 bytes a lane loads as the "lo" half of a k-step (its 8 features:
// 16 kt + 8 (l / 32) + 0..7, the addressing of the f16 low half they replace) are
//      weights  [ w_lo8 x 8 | w_hi8 x 8 ],  w_lo8 = e4m3((w' - half(w')) * 2^6),  w_hi8 = e4m3(w' * 2^-6)        (w' = w * 2^s: max in [2^13, 2^14))
//      rays     [ x8    x 8 | x_lo8 x 8 ],  x8    = e4m3(x * 2^-Ea),              x_lo8 = e4m3((x - half(x)) * 2^(12 - Ea))
// and the even and the odd k-step's 16 bytes are the two halves of the instruction's 32-byte operand: scale 2^-6 on the weights, 2^Ea on the rays.
// Ea (HrMlpArgs::xexp, per layer) comes from the activation-range calibration; an activation beyond 448 * 2^Ea saturates its fp8 images
// (MODE.FP16_OVFL is set: without it v_cvt_scalef32_pk_fp8_f32 returns NaN there) and sets bit 1 of the model's sticky status word.
#ifndef HR_F8_AHEAD_SMALL
#define HR_F8_AHEAD_SMALL 1       // weight look-ahead (k-steps) where registers are scarce: the frame kernel's 168-VGPR plan (RING == 3)
#endif
typedef int hr_v8i __attribute__((ext_vector_type(8)));
typedef int hr_v4i __attribute__((ext_vector_type(4)));

template <int NT>
__device__ __forceinline__ void hr_load_w8(bf16x8 (&h)[NT], hr_v8i (&q)[NT], int half, const bf16x8* __restrict__ wp, int wkt, int tiles_total, const int (&tile)[NT],
                                           int lane)
{
#ifdef HR_W_LOAD_AUX
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16x8*>(wp), 0, 0x7FFFFFFF, 0x00020000);
#endif
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        hr_v4i qq;
#ifdef HR_W_LOAD_AUX
        const int base = ((wkt * tiles_total + tile[nt]) * 2 * 64 + lane) * 16;
        h[nt] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, base, 0, HR_W_LOAD_AUX));
        qq = __builtin_bit_cast(hr_v4i, __builtin_amdgcn_raw_buffer_load_b128(rs, base + 64 * 16, 0, HR_W_LOAD_AUX));
#else
        const size_t base = (((size_t)wkt * tiles_total + tile[nt]) * 2) * 64 + lane;
        h[nt] = wp[base];
        qq = __builtin_bit_cast(hr_v4i, wp[base + 64]);
#endif
        if (half) q[nt].hi = qq; else q[nt].lo = qq;
    }
}

template <int MT>
__device__ __forceinline__ void hr_load_x8(bf16x8 (&h)[MT], hr_v8i (&q)[MT], int half, const HR_SPLIT_E* __restrict__ xh, const HR_SPLIT_E* __restrict__ xl, int stride,
                                           int kt, int lane, bool want_h, bool want_q)
{
    const int xoff = (lane & 31) * stride + kt * 16 + 8 * (lane >> 5);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        if (want_h) h[mt] = *reinterpret_cast<const bf16x8*>(xh + xoff + mt * 32 * stride);
        if (want_q) {
            const hr_v4i qq = *reinterpret_cast<const hr_v4i*>(xl + xoff + mt * 32 * stride);
            if (half) q[mt].hi = qq; else q[mt].lo = qq;
        }
    }
}

// The weight slots of hr_accumulate_f8 (AHEAD + 1 for the f16 halves, two pair slots for the fp8 operand).  A caller may own them and have
// the first AHEAD k-steps loaded BEFORE the GEMM starts (hr_prefetch_f8: the weights of the next layer do not depend on this layer's
// output, so their L2 latency -- ~1.5 k cycles in front of every layer's first MFMA, K1's phase trace -- runs under the epilogue).
template <int NT, int AHEAD>
struct HrF8Ring {
    static constexpr int NPQ = AHEAD <= 3 ? 2 : (AHEAD + 3) / 2;   // pair slots of the fp8 operand (two suffice up to 3 k-steps: a load whose slot is still being read goes out behind the step's MFMAs)
    bf16x8 wh[AHEAD + 1][NT];
    hr_v8i wq[NPQ][NT];
};
template <int NT, int AHEAD>
__device__ __forceinline__ void hr_prefetch_f8(HrF8Ring<NT, AHEAD>& ring, const bf16x8* wp, int kt0, int tiles_total, const int (&tile)[NT], int lane)
{
    constexpr int NPQ = HrF8Ring<NT, AHEAD>::NPQ;
#pragma unroll
    for (int s = 0; s < AHEAD; ++s) hr_load_w8<NT>(ring.wh[s % (AHEAD + 1)], ring.wq[(s >> 1) % NPQ], s & 1, wp, kt0 + s, tiles_total, tile, lane);
}

// AHEAD: k-steps the weight loads run ahead of their use (AHEAD + 1 slots for the f16 halves, two pair slots for the fp8 operand); the
// rays' f16 halves one k-step ahead in two slots, their fp8 operand in ONE slot that is re-loaded half by half as soon as the
// instruction reading it has been issued.  Fully unrolled: every slot index is a compile-time constant.
// PRE: the ring is the caller's and already holds k-steps 0 .. AHEAD - 1 (hr_prefetch_f8).
template <int NKT, int NT, int MT, int AHEAD, bool PRE = false>
__device__ __forceinline__ void hr_accumulate_f8(floatx16 (&acc)[NT][MT], const HR_SPLIT_E* xh, const HR_SPLIT_E* xl, int stride, const bf16x8* wp, int kt0,
                                                 int tiles_total, const int (&tile)[NT], int lane, int sw, int sx, HrF8Ring<NT, AHEAD>* pre = nullptr)
{
    static_assert(NKT % 2 == 0 && AHEAD >= 1 && AHEAD <= 7 && AHEAD <= NKT, "k-steps in pairs");
    constexpr int R = AHEAD + 1;
    constexpr int NPQ = HrF8Ring<NT, AHEAD>::NPQ;
    HrF8Ring<NT, AHEAD> own;
    HrF8Ring<NT, AHEAD>& ring = PRE ? *pre : own;
    bf16x8 (&wh)[R][NT] = ring.wh;
    hr_v8i (&wq)[NPQ][NT] = ring.wq;
    bf16x8 xv[2][MT];
    hr_v8i xq[MT];
    if constexpr (!PRE) hr_prefetch_f8<NT, AHEAD>(ring, wp, kt0, tiles_total, tile, lane);
    hr_load_x8<MT>(xv[0], xq, 0, xh, xl, stride, 0, lane, true, true);
#pragma unroll
    for (int s = 0; s < NKT; ++s) {
        // the loads that may go out before this step's MFMAs: everything whose slot was last read by an instruction already issued
        const int ws = s + AHEAD;                                  // weights of k-step s + AHEAD: pair P = ws / 2, whose slot pair P - NPQ read at step 2 (P - NPQ) + 1
        const bool w_early = (2 * (ws >> 1) <= s + 2 * NPQ - 2);
        const bool xq_early = (2 * ((s + 1) >> 1) <= s);           // (the rays' single fp8 slot: pair P - 1 read it at step 2 P - 1)
        if (ws < NKT && w_early) hr_load_w8<NT>(wh[ws % R], wq[(ws >> 1) % NPQ], ws & 1, wp, kt0 + ws, tiles_total, tile, lane);
        if (s + 1 < NKT) hr_load_x8<MT>(xv[(s + 1) & 1], xq, (s + 1) & 1, xh, xl, stride, s + 1, lane, true, xq_early);
        __builtin_amdgcn_s_setprio(HR_MFMA_PRIO_HI);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                acc[nt][mt] = HR_SPLIT_MFMA(wh[s % R][nt], xv[s & 1][mt], acc[nt][mt], 0, 0, 0);
        if (s & 1) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
                    acc[nt][mt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wq[(s >> 1) % NPQ][nt], xq[mt], acc[nt][mt], 0, 0, 0, sw, 0, sx);
        }
        __builtin_amdgcn_s_setprio(HR_MFMA_PRIO_LO);
        if (ws < NKT && !w_early) hr_load_w8<NT>(wh[ws % R], wq[(ws >> 1) % NPQ], ws & 1, wp, kt0 + ws, tiles_total, tile, lane);
        if (s + 1 < NKT && !xq_early) hr_load_x8<MT>(xv[(s + 1) & 1], xq, (s + 1) & 1, xh, xl, stride, s + 1, lane, false, true);
    }
}
#endif

// The accumulators of one n-tile start from the layer's bias instead of from zero: acc[mt][4 g + i] = bias'[32 tile + 8 g + 4 (lane / 32) + i],
// bias' = bias * 2^s packed by hr_model_finalize (2^s: the factor the packed weights carry; exact), so that the epilogue's  acc * 2^-s + b  is
// acc * 2^-s  -- the bias loads leave the head of the epilogue, where their L2 latency was exposed behind a barrier (K1's phase trace: the
// epilogues are latency-, not issue-bound), and the zero-fill goes with them.  Issued BEFORE the GEMM's first weight loads.
template <int MT>
__device__ __forceinline__ void hr_acc_init_bias(floatx16 (&acc)[MT], const float* __restrict__ bias, int tile_n, int lane)
{
    const float* b = bias + tile_n * 32 + 4 * (lane >> 5);        // (bias is padded to whole tiles)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 v = *reinterpret_cast<const float4*>(b + 8 * g);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            acc[mt][4 * g + 0] = v.x; acc[mt][4 * g + 1] = v.y; acc[mt][4 * g + 2] = v.z; acc[mt][4 * g + 3] = v.w;
        }
    }
}

// RING: weight slots (k-steps of look-ahead + 1).  4 = the pipelined loop above (206 VGPRs with 2x2 tiles); 3 = the
// unrolled ring, for kernels that must fit 168 VGPRs (three wavefronts per SIMD in the fused frame kernel).
template <int RING, int NKT, int NT, int MT>
__device__ __forceinline__ void hr_accumulate_hidden(floatx16 (&acc)[NT][MT], const HR_SPLIT_E* xh, const HR_SPLIT_E* xl, int stride,
                                                     const bf16x8* wp, int kt0, int tiles_total, const int (&tile)[NT], int lane, int sw, int sx)
{
#ifdef HR_SPLIT_F8LO
    hr_accumulate_f8<NKT, NT, MT, (RING >= 4 ? 3 : HR_F8_AHEAD_SMALL)>(acc, xh, xl, stride, wp, kt0, tiles_total, tile, lane, sw, sx);
#else
    (void)sw; (void)sx;
    if constexpr (RING == 4) hr_accumulate3_pipe<NKT, NT, MT>(acc, xh, xl, stride, wp, kt0, tiles_total, tile, lane);
    else hr_accumulate3_ring<NKT, NT, MT, RING>(acc, xh, xl, stride, wp, kt0, tiles_total, tile, lane);
#endif
}

// Input segment (k0p/16 = 1..4 k-steps): short, no ring.
template <int NT, int MT>
__device__ __forceinline__ void hr_accumulate3(floatx16 (&acc)[NT][MT], const HR_SPLIT_E* xh, const HR_SPLIT_E* xl, int stride, int nkt,
                                               const bf16x8* wp, int kt0, int tiles_total, const int (&tile)[NT], int lane)
{
    for (int kt = 0; kt < nkt; ++kt) {
        HrWOps<NT> w;
        HrXOps<MT> x;
        hr_load_w<NT>(w, wp, kt0 + kt, tiles_total, tile, lane);
        hr_load_x<MT>(x, xh, xl, stride, kt, lane);
        hr_mfma3<NT, MT>(acc, w, x);
    }
}

// v[0..3]: this lane's feature quad g, v[4..7]: its quad g + 1 (8 features further).  After the exchange with the partner lane
// (lane ^ 32) the lower lane stores features 8g .. 8g+7 and the upper lane 8(g+1) .. 8(g+1)+7 at `idx` (its own 8-block): 16 bytes
// per half.  Same roundings as hr_split_store4: hi = E(v), lo = E(v - hi).
__device__ __forceinline__ void hr_split_store8(HR_SPLIT_E* xh, HR_SPLIT_E* xl, int idx, const float (&v)[8])
{
    typedef unsigned u2 __attribute__((ext_vector_type(2)));
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    bf16x4 ha, la, hb, lb;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        ha[i] = (HR_SPLIT_E)v[i];
        la[i] = (HR_SPLIT_E)(v[i] - (float)ha[i]);
        hb[i] = (HR_SPLIT_E)v[4 + i];
        lb[i] = (HR_SPLIT_E)(v[4 + i] - (float)hb[i]);
    }
    const u2 ha2 = __builtin_bit_cast(u2, ha), hb2 = __builtin_bit_cast(u2, hb), la2 = __builtin_bit_cast(u2, la), lb2 = __builtin_bit_cast(u2, lb);
    // permlane32_swap(x, y) -> {[x_low | y_low], [x_high | y_high]}: first result = (lower lanes: own quad g; upper lanes: the
    // partner's quad g + 1), second = (lower: the partner's quad g; upper: own quad g + 1) -- ascending feature order in both halves
    const auto h0 = __builtin_amdgcn_permlane32_swap(ha2.x, hb2.x, false, false), h1 = __builtin_amdgcn_permlane32_swap(ha2.y, hb2.y, false, false);
    const auto l0 = __builtin_amdgcn_permlane32_swap(la2.x, lb2.x, false, false), l1 = __builtin_amdgcn_permlane32_swap(la2.y, lb2.y, false, false);
    *reinterpret_cast<u4*>(xh + idx) = u4{h0[0], h1[0], h0[1], h1[1]};
    *reinterpret_cast<u4*>(xl + idx) = u4{l0[0], l1[0], l0[1], l1[1]};
}

#ifdef HR_SPLIT_F8LO
// The f16 + fp8 form of hr_split_store8: the f16 half as there (16 bytes at xh + row + f0), and in place of the f16 low half (16 bytes at xl + row + f0)
// the two fp8 images of the same 8 features -- x8 = e4m3(v / x8s), then x_lo8 = e4m3((v - half(v)) / xl8s), 8 bytes each -- as ONE 16-byte store
// (hr_accumulate_f8 reads them back with the addressing of the half they replace).  f0: first feature (multiple of 8).
// v - half(word.lo / .hi) in ONE instruction (v_fma_mix_f32: the half operand is widened exactly; half * -1 + v is the exact residual, it has at most
// 13 significant bits) -- instead of v_cvt_f32_f16 + v_sub_f32 per value
template <int HI>
__device__ __forceinline__ float hr_residual_mix(unsigned word, float v)
{
    float d;
    if constexpr (HI) asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(word), "v"(v));
    else asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(word), "v"(v));
    return d;
}

__device__ __forceinline__ void hr_split_store8_f8(HR_SPLIT_E* xh, HR_SPLIT_E* xl, int row, int f0, const float (&v)[8], float x8s, float xl8s)
{
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    typedef short s2 __attribute__((ext_vector_type(2)));
    typedef HR_SPLIT_E e2 __attribute__((ext_vector_type(2)));
    // the f16 halves, two per instruction (v_cvt_pk_f16_f32, round to nearest even like the scalar conversion) ...
    unsigned hw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const e2 p = {(HR_SPLIT_E)v[2 * i], (HR_SPLIT_E)v[2 * i + 1]};
        hw[i] = __builtin_bit_cast(unsigned, p);
    }
    // ... and what they leave of each value
    float la[4], lb[4];
    la[0] = hr_residual_mix<0>(hw[0], v[0]); la[1] = hr_residual_mix<1>(hw[0], v[1]);
    la[2] = hr_residual_mix<0>(hw[1], v[2]); la[3] = hr_residual_mix<1>(hw[1], v[3]);
    lb[0] = hr_residual_mix<0>(hw[2], v[4]); lb[1] = hr_residual_mix<1>(hw[2], v[5]);
    lb[2] = hr_residual_mix<0>(hw[3], v[6]); lb[3] = hr_residual_mix<1>(hw[3], v[7]);
    s2 xa = {0, 0}, xb = {0, 0}, qa = {0, 0}, qb = {0, 0};
    xa = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(xa, v[0], v[1], x8s, false);
    xa = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(xa, v[2], v[3], x8s, true);
    xb = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(xb, v[4], v[5], x8s, false);
    xb = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(xb, v[6], v[7], x8s, true);
    qa = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(qa, la[0], la[1], xl8s, false);
    qa = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(qa, la[2], la[3], xl8s, true);
    qb = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(qb, lb[0], lb[1], xl8s, false);
    qb = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(qb, lb[2], lb[3], xl8s, true);      // (a multiplication + v_cvt_pk_fp8_f32 instead: 1.765 vs 1.732 ms per frame)
    const auto h0 = __builtin_amdgcn_permlane32_swap(hw[0], hw[2], false, false), h1 = __builtin_amdgcn_permlane32_swap(hw[1], hw[3], false, false);
    const auto x0 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, xa), __builtin_bit_cast(unsigned, xb), false, false);
    const auto q0 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, qa), __builtin_bit_cast(unsigned, qb), false, false);
    *reinterpret_cast<u4*>(xh + row + f0) = u4{h0[0], h1[0], h0[1], h1[1]};
    *reinterpret_cast<u4*>(xl + row + f0) = u4{x0[0], x0[1], q0[0], q0[1]};
}
#endif

__device__ __forceinline__ void hr_split_store4(HR_SPLIT_E* xh, HR_SPLIT_E* xl, int idx, float v0, float v1, float v2, float v3)
{
    bf16x4 h, l;
    h[0] = (HR_SPLIT_E)v0; h[1] = (HR_SPLIT_E)v1; h[2] = (HR_SPLIT_E)v2; h[3] = (HR_SPLIT_E)v3;
    l[0] = (HR_SPLIT_E)(v0 - (float)h[0]);
    l[1] = (HR_SPLIT_E)(v1 - (float)h[1]);
    l[2] = (HR_SPLIT_E)(v2 - (float)h[2]);
    l[3] = (HR_SPLIT_E)(v3 - (float)h[3]);
    *reinterpret_cast<bf16x4*>(xh + idx) = h;
    *reinterpret_cast<bf16x4*>(xl + idx) = l;
}



// ---------------------------------------------------------------------------------------------------------
// One tile of 32*MT rays through all layers, by the NW wavefronts with threadIdx.x < 64*NW.
// SYNC: how those wavefronts meet (`barrier()`), and `before_input_store()` -- called once per tile before the MLP input
//       is written to Xih/Xil.
// SINK: where the raw head goes: `begin()` before the first store of the tile, `store(r, row, n0, v)` for the 4 features
//       n0..n0+3 of tile row r (= ray `row`), `end()` after the last one.
// The stand-alone kernel uses the block barrier and the HBM workspace; the fused frame kernel an LDS counter barrier
// among the MLP wavefronts and the LDS head tile that the sample wavefronts of the same workgroup consume.
struct HrMlpTrace {
    unsigned long long* tr;
    int tri;
};
#define HR_STAMP() do { if (trace.tr && lane == 0 && trace.tri < 64) trace.tr[trace.tri] = __builtin_readcyclecounter(); ++trace.tri; } while (0)

template <int W, int MT, int NW, int RING, class SYNC, class SINK>
__device__ __forceinline__ void hr_mlp_tile(const hr_config& cfg, const HrMlpArgs& a, int64_t ray0, int64_t n_rays, HR_SPLIT_E* Xih, HR_SPLIT_E* Xil,
                                            HR_SPLIT_E* Xh, HR_SPLIT_E* Xl, SYNC& sync, SINK& sink, HrMlpTrace& trace)
{
    constexpr int TM = 32 * MT;           // rays per tile
    constexpr int XS = W + 8;             // bf16 elements per activation row
    constexpr int NT = (W / 32) / NW;     // hidden-layer tiles per wave
    constexpr int NTHREADS = 64 * NW;
    static_assert(W == 256 && (NT == 1 || NT == 2), "hidden width 256 with 4 or 8 waves");
    const int k0p = a.k0p;
    const int XSI = k0p + 8;
    float* stage = reinterpret_cast<float*>(Xh);             // fp32 features, only before layer 0
    int tid = threadIdx.x;
    // opaque to the optimiser: in a persistent caller (the frame kernel's tile loop) everything derived from the thread index -- a dozen
    // LDS / weight address components -- would otherwise be hoisted out of the loop, held across it and spilled (24 dwords of scratch);
    // recomputing them per tile is a few dozen VALU instructions
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform, and the compiler should know: tile indices and weight addresses then live in SGPRs
#ifdef HR_SPLIT_F8LO
    // MODE.FP16_OVFL: out-of-range fp8 conversions SATURATE (+-448) instead of returning NaN (tools/f8_ovfl_probe.hip, profiles/r04_f8_ovfl_probe.txt) --
    // an activation beyond the calibrated range then costs the accuracy of its correction term, not the pixel.  (The same bit makes an
    // overflowing f16 conversion 65504 instead of inf; the half-range check below reports either.)  Per wavefront; the frame kernel's sample
    // wavefronts never come here.
    __builtin_amdgcn_s_setreg(1 | (23 << 6), 1);
#endif

    // ---- prologue: ray parameterisation + positional encoding (fp32), then split.  All wavefronts share it: thread t works
    //      on ray t % TM and evaluates every (NTHREADS / TM)-th sin/cos pair (hr_ray_features' part / nparts)
    {
        constexpr int NPARTS = NTHREADS / TM;
        const int rt = tid % TM, part = tid / TM;
        const int64_t r = ray0 + rt;
        float* row = stage + rt * k0p;
        int n = 0;
        if (r < n_rays) n = hr_ray_features(cfg, a.rays + (a.ray_index ? (int64_t)a.ray_index[r] : r) * cfg.ray_dim, row, part, NPARTS);
        if (part == 0)
            for (int i = n; i < k0p; ++i) row[i] = 0.0f;
    }
    sync.barrier();
    sync.before_input_store();
#ifdef HR_SPLIT_RANGE_CHECK
    // fp16 halves: everything that is stored as a half -- the input features here, the hidden activations in the epilogues --
    // must stay below 65504.  hr_model_finalize / hr_model_calibrate decide that from a calibration pass; this is the running check
    // on the rays that are actually rendered: a sticky bit in the model's status word (HR_OPT_MLP_OVERFLOW), two v_max3 per 4 values
    float amax = 0.0f;
    bool over8 = false;
#define HR_RANGE4(v0, v1, v2, v3) amax = fmaxf(fmaxf(amax, fmaxf(fabsf(v0), fabsf(v1))), fmaxf(fabsf(v2), fabsf(v3)))
#else
#define HR_RANGE4(v0, v1, v2, v3) do {} while (0)
#endif
    for (int i = tid; i < TM * (k0p / 4); i += NTHREADS) {
        const int r = i / (k0p / 4), c4 = i - r * (k0p / 4);
        const float4 v = *reinterpret_cast<const float4*>(stage + r * k0p + 4 * c4);
        HR_RANGE4(v.x, v.y, v.z, v.w);
        hr_split_store4(Xih, Xil, r * XSI + 4 * c4, v.x, v.y, v.z, v.w);
    }
    sync.barrier();
    HR_STAMP();                                              // 1: prologue done

    const int L = cfg.mlp_layers;
#ifdef HR_SPLIT_F8LO
    // the first k-steps of the NEXT hidden layer's weights are requested as soon as this layer's GEMM has issued its last loads -- they do not
    // depend on its output -- and arrive under the barrier and the epilogue (hr_prefetch_f8)
#ifndef HR_F8_AHEAD_BIG
#define HR_F8_AHEAD_BIG 3          // weight look-ahead (k-steps) of the stand-alone kernel; 5 and 7 measured level (DESIGN 10)
#endif
    constexpr int F8A = (RING >= 4 ? HR_F8_AHEAD_BIG : HR_F8_AHEAD_SMALL);
    constexpr bool PREN = (RING >= 4);       // (not in the frame kernel's 168-register plan: the ring would have to live through its epilogues)
    HrF8Ring<NT, F8A> ring8;
#endif
    // ---- hidden layers: wave w owns output features [w*W/NW, (w+1)*W/NW)
    for (int l = 0; l + 1 < L; ++l) {
        int lt = tid;
        asm volatile("" : "+v"(lt));                          // (as above, per layer: nothing lane-derived is carried around the layer loop)
        const int lane = lt & 63;
        const bool skip = (cfg.mlp_skip_mask >> l) & 1;
        const bf16x8* wp = reinterpret_cast<const bf16x8*>(a.wsplit[l]);
        const int tiles_total = a.n_tiles[l];
        const float* bias = a.bias[l];
        const float winv = a.winv[l];
#ifdef HR_SPLIT_F8LO
        // E8M0 scales of the fp8 correction product (see hr_accumulate_f8): 2^-6 on the weights, 2^Ea on the rays, for both blocks; Ea belongs to
        // the layer that WROTE the activations
        const int sw8 = 127 - 6;
        const int sx8 = 127 + (l > 0 ? a.xexp[l - 1] : 0);
        const float x8s = __builtin_ldexpf(1.0f, a.xexp[l]), xl8s = __builtin_ldexpf(1.0f, a.xexp[l] - 12);     // what this layer's epilogue divides by
        const float amax_before = amax;
        amax = 0.0f;
#else
        const int sw8 = 0, sx8 = 0;
#endif
        floatx16 acc[NT][MT];
        int tile[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) tile[nt] = wave * NT + nt;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) hr_acc_init_bias<MT>(acc[nt], bias, tile[nt], lane);
        int kt0 = 0;
        if (l == 0 || skip) {
            hr_accumulate3<NT, MT>(acc, Xih, Xil, XSI, k0p / 16, wp, 0, tiles_total, tile, lane);
            kt0 = k0p / 16;
        }
#ifdef HR_SPLIT_F8LO
        // (every hidden layer l >= 1 finds its first k-steps in the ring: layer l - 1 requested them below)
        if (l > 0) hr_accumulate_f8<W / 16, NT, MT, F8A, PREN>(acc, Xh, Xl, XS, wp, kt0, tiles_total, tile, lane, sw8, sx8, &ring8);
        if (PREN && l + 2 < L) {             // the next layer is a hidden one too: its hidden segment starts behind the input segment of a skip layer
            const bool skip_n = (cfg.mlp_skip_mask >> (l + 1)) & 1;
            hr_prefetch_f8<NT, F8A>(ring8, reinterpret_cast<const bf16x8*>(a.wsplit[l + 1]), skip_n ? k0p / 16 : 0, a.n_tiles[l + 1], tile, lane);
        }
#else
        if (l > 0) hr_accumulate_hidden<RING, W / 16, NT, MT>(acc, Xh, Xl, XS, wp, kt0, tiles_total, tile, lane, sw8, sx8);
#endif
        HR_STAMP();                          // 2+3l: GEMM of layer l issued
        sync.barrier();                      // all waves have finished reading Xh/Xl
        HR_STAMP();                          // 3+3l: barrier passed
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int hb = lane >> 5;
            const int nbase = tile[nt] * 32 + 4 * hb;
            (void)nbase;
            // Feature quads g and g + 1 of a lane are 8 apart; its partner lane (+-32: same ray, the other half of every 8-block)
            // holds the quads in between.  One v_permlane32_swap per packed word hands the lower lane the partner's quad g and
            // the upper lane the partner's quad g + 1: each lane then owns 8 CONSECUTIVE features and writes them as one 16-byte
            // ds_write_b128 per half -- rows are 4 bank-quads apart, so the 16 lanes of a write group cover all 64 banks, where
            // the 8-byte stores of one quad collided two ways (34 % of the kernel's LDS cycles were bank conflicts)
#pragma unroll
            for (int gp = 0; gp < 4; gp += 2) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    float v[8];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        v[i] = acc[nt][mt][4 * gp + i] * winv;               // the accumulator started from bias * 2^s (hr_acc_init_bias); * 2^-s is exact
                        v[4 + i] = acc[nt][mt][4 * gp + 4 + i] * winv;
                    }
#pragma unroll
                    for (int i = 0; i < 8; ++i) {            // nn.LeakyReLU(0.01), mlp.py:149-154: for a slope in [0, 1] (hr_model_create checks) v > 0 ? v : v s  ==  max(v, v s),
                        const float t = v[i] * cfg.leaky_slope;   // bit for bit (zeros keep their sign, NaN stays NaN) -- two instructions instead of three
                        asm("v_max_f32 %0, %1, %2" : "=v"(v[i]) : "v"(v[i]), "v"(t));
                    }
                    HR_RANGE4(v[0], v[1], v[2], v[3]);
                    HR_RANGE4(v[4], v[5], v[6], v[7]);
                    // training forward (HrSinkTrain): the layer's output is also what its backward needs -- this lane's two feature quads
                    // of one ray, v[0..3] = features nbase + 8 gp .., v[4..7] = the quad 8 further
                    if constexpr (SINK::TAPS) sink.tap(l, ray0 + mt * 32 + (lane & 31), nbase + 8 * gp, v);
#ifdef HR_SPLIT_F8LO
                    hr_split_store8_f8(Xh, Xl, (mt * 32 + (lane & 31)) * XS, tile[nt] * 32 + 8 * (gp + hb), v, x8s, xl8s);
#else
                    hr_split_store8(Xh, Xl, (mt * 32 + (lane & 31)) * XS + tile[nt] * 32 + 8 * (gp + hb), v);
#endif
                }
            }
        }
#ifdef HR_SPLIT_F8LO
        over8 = over8 || !(amax < 448.0f * x8s);             // an activation whose fp8 image saturated (or a NaN)
        amax = fmaxf(amax, amax_before);
#endif
        sync.barrier();
        HR_STAMP();                              // 4+3l: epilogue + barrier done
    }

#ifdef HR_SPLIT_RANGE_CHECK
    if (a.flags) {
        const unsigned bits = (__builtin_amdgcn_ballot_w64(!(amax < 65504.0f)) != 0ull ? 1u : 0u) |       // bit 0: the half range (NaN counts)
                              (__builtin_amdgcn_ballot_w64(over8) != 0ull ? 2u : 0u);                      // bit 1: an fp8 image saturated (f16 + fp8 split only)
        if (a.redo_list) {
            // verified fast path: the tile's rays are rendered again by the next arithmetic up (f16f8 -> f16x3 -> bf16x3, whose halves have the
            // fp32 range).  One entry per ray: the wavefronts agree on the tile's bits through a barrier, thread 0 writes the list.  The
            // sticky bit is only raised for rays that could NOT be listed (a full list): those pixels are the caller's to repair
            // (models.py, _overflow_guard)
            const bool b0 = sync.any((bits & 1u) != 0u), b1 = sync.any((bits & 2u) != 0u);
            if ((b0 || b1) && threadIdx.x == 0) {
                const int cnt = (int)((n_rays - ray0 < TM) ? (n_rays - ray0) : TM);
                const unsigned pos = atomicAdd(a.redo_count, (unsigned)cnt);
                for (int i = 0; i < cnt; ++i) {
                    if (pos + (unsigned)i < (unsigned)a.redo_cap) a.redo_list[pos + i] = a.ray_index ? a.ray_index[ray0 + i] : (int)(a.ray0 + ray0 + i);
                    else { atomicOr(a.flags, (b0 ? 1u : 0u) | (b1 ? 2u : 0u) | 4u); break; }
                }
            }
        } else if (bits && lane == 0) {
            atomicOr(a.flags, bits);
        }
    }
#endif
#undef HR_RANGE4
    // ---- last Linear: N = Z*P_live features in tiles of 32.  With 4 waves: full passes of 2 tiles
    //      per wave, and a remainder of up to 4 tiles as one tile per wave so that the waves stay
    //      balanced (DoNeRF after dead-column pruning: 11 tiles = 8 + 3).  With 8 waves: one tile per
    //      wave per pass.
    {
        int lt = tid;
        asm volatile("" : "+v"(lt));
        const int lane = lt & 63;
        const int l = L - 1;
        const bool skip = (cfg.mlp_skip_mask >> l) & 1;
        const bf16x8* wp = reinterpret_cast<const bf16x8*>(a.wsplit[l]);
        const int tiles_total = a.n_tiles[l];
        const float* bias = a.bias[l];
        const float winv = a.winv[l];
#ifdef HR_SPLIT_F8LO
        const int sw8 = 127 - 6;
        const int sx8 = 127 + a.xexp[l - 1];
#else
        const int sw8 = 0, sx8 = 0;
#endif
        bool begun = false;
        auto store_tile = [&](int tile_n, const floatx16 (&acc)[MT]) {
            if (!begun) { sink.begin(); begun = true; }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n0 = tile_n * 32 + 8 * g + 4 * (lane >> 5);
                if (n0 >= a.n_out) continue;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const int r = mt * 32 + (lane & 31);
                    float4 v;                                     // (the accumulator started from bias * 2^s)
                    v.x = acc[mt][4 * g + 0] * winv;
                    v.y = acc[mt][4 * g + 1] * winv;
                    v.z = acc[mt][4 * g + 2] * winv;
                    v.w = acc[mt][4 * g + 3] * winv;
                    sink.store(r, ray0 + r, n0, v);
                }
            }
        };
        int t0 = 0;
        if constexpr (SINK::HOLD) {
            // Hand-over through a single-buffered tile (the frame kernel): ALL of this wavefront's output tiles -- at most three, the
            // launcher guarantees tiles_total <= 3 NW -- are accumulated before the sink is opened, so that the consumers of the previous
            // tile are only waited for when nothing but the stores is left to do (they would otherwise idle through the second pass's GEMM)
            static_assert(NT == 2, "four MLP wavefronts");
            const bool hasA = (tiles_total > NW) && (2 * wave < tiles_total);
            const int tA[2] = {2 * wave, 2 * wave + 1};
            floatx16 accA[2][MT];
            if (hasA) {
                const int tile_ld[2] = {tA[0], min(tA[1], tiles_total - 1)};
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) hr_acc_init_bias<MT>(accA[nt], bias, tile_ld[nt], lane);
                hr_accumulate_hidden<RING, W / 16, 2, MT>(accA, Xh, Xl, XS, wp, 0, tiles_total, tile_ld, lane, sw8, sx8);
            }
            HR_STAMP();
            const int tB = ((tiles_total > NW) ? 2 * NW : 0) + wave;
            const bool hasB = tB < tiles_total;
            floatx16 accB[1][MT];
            if (hasB) {
                const int tile[1] = {tB};
                hr_acc_init_bias<MT>(accB[0], bias, tB, lane);
#ifdef HR_SPLIT_F8LO
                hr_accumulate_f8<W / 16, 1, MT, 1>(accB, Xh, Xl, XS, wp, 0, tiles_total, tile, lane, sw8, sx8);
#else
                hr_accumulate3_lean<W / 16, 1, MT>(accB, Xh, Xl, XS, wp, 0, tiles_total, tile, lane);
#endif
            }
            HR_STAMP();
            sink.begin();
            if (hasA) {
                store_tile(tA[0], accA[0]);
                if (tA[1] < tiles_total) store_tile(tA[1], accA[1]);
            }
            if (hasB) store_tile(tB, accB[0]);
            HR_STAMP();
            sink.end();
            return;
        }
        if constexpr (NT == 2) {
#pragma unroll 1
            for (; tiles_total - t0 > NW; t0 += 2 * NW) {              // two tiles per wave
                const int tile[2] = {t0 + wave * 2, t0 + wave * 2 + 1};
                if (tile[0] >= tiles_total) continue;                   // wave-uniform
                const int tile_ld[2] = {tile[0], min(tile[1], tiles_total - 1)};
                floatx16 acc[2][MT];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) hr_acc_init_bias<MT>(acc[nt], bias, tile_ld[nt], lane);
                int kt0 = 0;
                if (skip) {
                    hr_accumulate3<2, MT>(acc, Xih, Xil, XSI, k0p / 16, wp, 0, tiles_total, tile_ld, lane);
                    kt0 = k0p / 16;
                }
                hr_accumulate_hidden<RING, W / 16, 2, MT>(acc, Xh, Xl, XS, wp, kt0, tiles_total, tile_ld, lane, sw8, sx8);
                HR_STAMP();                      // last layer: GEMM of this pass issued
                store_tile(tile[0], acc[0]);
                if (tile[1] < tiles_total) store_tile(tile[1], acc[1]);
                HR_STAMP();                      // last layer: stores of this pass issued
            }
        }
#pragma unroll 1
        for (; t0 < tiles_total; t0 += NW) {                            // one tile per wave
            if (t0 + wave >= tiles_total) continue;
            const int tile[1] = {t0 + wave};
            floatx16 acc[1][MT];
            hr_acc_init_bias<MT>(acc[0], bias, tile[0], lane);
            int kt0 = 0;
            if (skip) {
                hr_accumulate3<1, MT>(acc, Xih, Xil, XSI, k0p / 16, wp, 0, tiles_total, tile, lane);
                kt0 = k0p / 16;
            }
            hr_accumulate_hidden<RING, W / 16, 1, MT>(acc, Xh, Xl, XS, wp, kt0, tiles_total, tile, lane, sw8, sx8);
            HR_STAMP();
            store_tile(tile[0], acc[0]);
            HR_STAMP();
        }
        if (!begun) sink.begin();              // a wavefront without a tile still takes part in the hand-over protocol
        sink.end();
    }
}
#undef HR_STAMP
