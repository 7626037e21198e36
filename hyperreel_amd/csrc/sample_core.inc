// K2+K3 -- everything after the MLP, one lane per (ray, sample).  Shared by the stand-alone sample kernel
// (sample_kernel.hip: the head comes from the HBM workspace) and the fused frame kernel (fused_impl.inc: the head is handed
// over in LDS by the MLP waves of the same workgroup):
//   head activations -> ray/primitive intersection -> near/far mask -> per-ray sort ->
//   points -> contraction -> advect -> offset   (reference: Intersect.forward,
//   nlf/intersect/base.py:142-259; nlf/embedding/point.py:371-396,780-831)
//   -> VM feature gather -> density -> alpha/transmittance -> colour decode -> composite
//   (TensorVMNoSample.forward, nlf/nets/tensorf_no_sample.py:128-280;
//    TensorVMKeyframeTime.forward, nlf/nets/tensorf_dynamic.py:645-839;
//    raw2alpha, utils/tensorf_utils.py:242-253).
//
// CDNA4 mapping
//   * the Z samples of a ray sit in adjacent lanes of ONE wavefront (ZP = 8/16/32/64 lanes; z_channels
//     above 64 spread a ray over 2 or 4 wavefronts of the block and add LDS hand-overs),
//     so the per-ray sort is an in-register bitonic network over DPP/bpermute shuffles,
//     the transmittance is a wave-level segmented prefix product and the final colour a
//     segmented butterfly sum -- no LDS round trips, no atomics, no global intermediates;
//   * the block's slice of the MLP head is staged once through LDS with coalesced
//     dwordx4 loads; each lane then reads its P values at an odd dword stride (conflict free);
//   * feature grids are stored channel-last with density and appearance channels of a
//     plane interleaved in one texel, so the 4 bilinear taps of a sample are 2 contiguous
//     runs of 2 texels and every fetch is a 16-byte vector load; density and appearance
//     features come from the same fetch (one pass over the grid instead of the
//     reference's two);
//   * the SH / RGB decode matrix is folded with the ray's SH basis once per ray into LDS
//     (3 x C_app), so the per-sample decode is 3*C_app FMAs regardless of SH degree.
#include <cstdlib>

#include "hr_kernels.h"
#include "hr_math.h"
#include "hr_mask.h"
#include "hr_time_decode.h"

#define HR_FMA(a, b, c) __builtin_fmaf((a), (b), (c))

// ZP > 64 (z_channels 65..256): the lanes of one ray span ZP/64 wavefronts of the block, and the steps
// that cross a wavefront go through a 256-float LDS scratch `s_x`.  Returns the value thread
// `src_tid` of the block holds.
__device__ __forceinline__ float hr_block_exchange(float v, int src_tid, float* s_x)
{
    __syncthreads();
    s_x[threadIdx.x] = v;
    __syncthreads();
    return s_x[src_tid];
}

template <int CTRL>
__device__ __forceinline__ float hr_dpp_f(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ int hr_dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }

// Cross-lane moves of the per-ray sort / scan / sum as pure VALU operations (DPP, v_permlane16_swap): the generic
// __shfl_* forms go through the LDS crossbar (ds_bpermute_b32: ~100 cycles of latency each, 42 of them per sample slot).
// DPP controls (gfx9): quad_perm 0x00-0xff, row_shr:n 0x110+n, row_ror:n 0x120+n, wave_shl:1 0x130, wave_shr:1 0x138,
// row_bcast:15 0x142 (lane 15 of every row -> the next row).
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float hr_dpp_old(float old, float v)       // lanes without a source (or masked rows) keep `old`
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
}

// the value lane (l ^ D) holds, D in {1, 2, 4, 8, 16}
template <int D>
__device__ __forceinline__ float hr_lane_xor(float v)
{
    static_assert(D == 1 || D == 2 || D == 4 || D == 8 || D == 16 || D == 32, "distances inside a wavefront");
    if constexpr (D == 1) return hr_dpp_f<0xB1>(v);
    else if constexpr (D == 2) return hr_dpp_f<0x4E>(v);
    else if constexpr (D == 8) return hr_dpp_f<0x128>(v);                  // row_ror:8 == xor 8 inside a row of 16
    else if constexpr (D == 4) {
        const float up = hr_dpp_f<0x12C>(v), dn = hr_dpp_f<0x124>(v);      // row_ror:12 reads lane l + 4, row_ror:4 lane l - 4 (mod 16)
        return ((int)threadIdx.x & 4) ? dn : up;
    } else if constexpr (D == 16) {
        // v_permlane16_swap_b32: odd rows of the first operand <-> even rows of the second; with v in both, the first result
        // holds row r-1 in the odd rows, the second row r+1 in the even rows
        const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
        return __builtin_bit_cast(float, ((int)threadIdx.x & 16) ? r[0] : r[1]);
    } else {
        // v_permlane32_swap_b32: the upper half of the first operand <-> the lower half of the second
        const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
        return __builtin_bit_cast(float, ((int)threadIdx.x & 32) ? r[0] : r[1]);
    }
}

template <int ZP>
__device__ __forceinline__ float hr_bitonic_sort(float v, int k, float* s_x)
{
#pragma unroll
    for (int size = 2; size <= ZP; size <<= 1) {
#pragma unroll
        for (int j = size >> 1; j > 0; j >>= 1) {
            float o;
            if (j == 1) o = hr_lane_xor<1>(v);
            else if (j == 2) o = hr_lane_xor<2>(v);
            else if (j == 4) o = hr_lane_xor<4>(v);
            else if (j == 8) o = hr_lane_xor<8>(v);
            else if (j == 16) o = hr_lane_xor<16>(v);
            else if (j == 32) o = hr_lane_xor<32>(v);
            else o = hr_block_exchange(v, (int)threadIdx.x ^ j, s_x);
            const bool up = ((k & size) == 0);
            const bool lower = ((k & j) == 0);
            // the instructions themselves: fminf / fmaxf first canonicalise both operands (v_max_f32 x, x) because the partner
            // arrives through a cross-lane move the compiler cannot see through -- same result, one or two instructions per stage
            float mn, mx;
            asm("v_min_f32 %0, %1, %2" : "=v"(mn) : "v"(v), "v"(o));
            asm("v_max_f32 %0, %1, %2" : "=v"(mx) : "v"(v), "v"(o));
            v = (lower == up) ? mn : mx;
        }
    }
    return v;
}

// sort_z (utils/intersect_utils.py:12-16) of one ray's distances.  The anchors of the shipped intersections are monotone along the ray -- ascending
// for the sphere / cylinder families (masked samples, 0, sit in front already), descending for the z-plane families -- and the MLP's offsets rarely
// reorder them (8 192 rays of each benchmark frame: every ray of DoNeRF / immersive already ascending, every ray of technicolor / Neural-3D
// exactly reversed).  The sorted array is a function of the values alone, so: one comparison with the next lane and a wave-wide vote; an ascending
// wavefront skips the network (15 compare-exchange stages at Z = 32: ~115 vector instructions, a third of them DPP), a descending one reverses
// its rays' lanes (3 instructions); anything else -- NaNs included -- takes the network as before.  Bit for bit the network's result.
template <int ZP>
__device__ __forceinline__ float hr_sort_ray(float v, int k, float* s_x)
{
    if constexpr (ZP > 64) return hr_bitonic_sort<ZP>(v, k, s_x);
    else {
        const float nxt = hr_dpp_f<0x130>(v);                       // wave_shl:1: the next lane's value
        const bool last = (k == ZP - 1);
        if (__builtin_amdgcn_ballot_w64(!(last || v <= nxt)) == 0ull) return v;
        if (__builtin_amdgcn_ballot_w64(!(last || v >= nxt)) == 0ull) {
            // lane k <- lane ZP - 1 - k of the same ray: mirror inside the row (half row), then swap rows (halves)
            if constexpr (ZP == 8) v = hr_dpp_f<0x141>(v);          // row_half_mirror
            else v = hr_dpp_f<0x140>(v);                            // row_mirror
            if constexpr (ZP >= 32) v = hr_lane_xor<16>(v);
            if constexpr (ZP == 64) v = hr_lane_xor<32>(v);
            return v;
        }
        return hr_bitonic_sort<ZP>(v, k, s_x);
    }
}

// weighted sum of the 4 bilinear taps for one float4 channel group, in ATen's order
// (nw, ne, sw, se; grid_sampler_2d)
__device__ __forceinline__ float4 hr_bilerp4(const float4 v00, const float4 v01, const float4 v10, const float4 v11,
                                              float w00, float w01, float w10, float w11)
{
    float4 r;
    r.x = HR_FMA(v11.x, w11, HR_FMA(v10.x, w10, HR_FMA(v01.x, w01, v00.x * w00)));
    r.y = HR_FMA(v11.y, w11, HR_FMA(v10.y, w10, HR_FMA(v01.y, w01, v00.y * w00)));
    r.z = HR_FMA(v11.z, w11, HR_FMA(v10.z, w10, HR_FMA(v01.z, w01, v00.z * w00)));
    r.w = HR_FMA(v11.w, w11, HR_FMA(v10.w, w10, HR_FMA(v01.w, w01, v00.w * w00)));
    return r;
}

__device__ __forceinline__ float4 hr_lerp4(const float4 v0, const float4 v1, float w0, float w1)
{
    float4 r;
    r.x = HR_FMA(v1.x, w1, v0.x * w0);
    r.y = HR_FMA(v1.y, w1, v0.y * w0);
    r.z = HR_FMA(v1.z, w1, v0.z * w0);
    r.w = HR_FMA(v1.w, w1, v0.w * w0);
    return r;
}

// One float4 channel group of a sample: plane tap x (line | time-plane) tap, then density partial
// sum (q < cd) or appearance decode through the ray's matrix M.
// DEN (the time kernel's density modes, DESIGN 3m): the density channels are weighted by the ray's density row -- Dj: the row's slots of
// this plane pair -- instead of summed.
template <bool DEN = false>
__device__ __forceinline__ void hr_consume_group(const HrGridPlane& g, int q, int cd, const float4 pa, const float4 pb, const float* M,
                                                 int CA, float& sig_feat, float& pre0, float& pre1, float& pre2, const float* Dj = nullptr)
{
    const float fx = pa.x * pb.x, fy = pa.y * pb.y, fz = pa.z * pb.z, fw = pa.w * pb.w;
    if (q < cd) {
        if constexpr (DEN) {
            const float4 d = *reinterpret_cast<const float4*>(Dj + 4 * q);
            sig_feat = HR_FMA(d.w, fw, HR_FMA(d.z, fz, HR_FMA(d.y, fy, HR_FMA(d.x, fx, sig_feat))));
        } else {
            sig_feat = sig_feat + fx; sig_feat = sig_feat + fy; sig_feat = sig_feat + fz; sig_feat = sig_feat + fw;
        }
    } else {
        const int ch = g.app_off + 4 * (q - cd);
        const float4 m0 = *reinterpret_cast<const float4*>(M + ch);
        const float4 m1 = *reinterpret_cast<const float4*>(M + CA + ch);
        const float4 m2 = *reinterpret_cast<const float4*>(M + 2 * CA + ch);
        pre0 = HR_FMA(m0.w, fw, HR_FMA(m0.z, fz, HR_FMA(m0.y, fy, HR_FMA(m0.x, fx, pre0))));
        pre1 = HR_FMA(m1.w, fw, HR_FMA(m1.z, fz, HR_FMA(m1.y, fy, HR_FMA(m1.x, fx, pre1))));
        pre2 = HR_FMA(m2.w, fw, HR_FMA(m2.z, fz, HR_FMA(m2.y, fy, HR_FMA(m2.x, fx, pre2))));
    }
}

typedef _Float16 hr_half8 __attribute__((ext_vector_type(8)));

// The three plane pairs of a VM decomposition sample the SAME three axis coordinates: plane j spans axes
// (MAT[j][0], MAT[j][1]) and its line / time plane runs along VEC[j] (tensorf_base.py:231-232, tensorf_dynamic.py:48),
// every axis always at that axis' grid size.  So a sample needs three 1-D taps (+ one along the keyframes), computed
// once, instead of three per plane pair.
struct HrAxisTaps {
    hr_axis_tap ax[3];          // x @ grid[0], y @ grid[1], z @ grid[2]
    hr_axis_tap t;              // keyframe axis (video) -- unused otherwise
};

template <int J> struct HrPlaneAxes {
    static constexpr int A0 = (J == 2) ? 1 : 0;           // MAT_MODE[j][0]: 0, 0, 1
    static constexpr int A1 = (J == 0) ? 1 : 2;           // MAT_MODE[j][1]: 1, 2, 2
    static constexpr int V = 2 - J;                       // VEC_MODE[j] = MAT_MODE_TIME[j][0]: 2, 1, 0
};

// How the gather is compiled per kernel variant.  fp32 texels: the lanes of a quad (or pair) cooperate on one sample
// at a time (hr_gather_plane_coop below); float16 texels: every lane gathers its own sample, one 16-byte load per two
// channel groups.  Both at 4 workgroups/CU.  Measured sample stage, ms per 800x800 frame:
//                            own-sample, group-major   own-sample, 2 groups/tap   cooperative
//   DoNeRF Z=32 static              1.18                      1.39                   1.12
//   technicolor Z=32 keyframe       1.13                       -                     0.94
//   immersive Z=32 keyframe         1.58                      1.75                   1.34
//   neural_3d Z=64 keyframe         4.55 (L1 hit rate 61 %)   3.95                   2.93
template <int ZP, bool HALF>
struct HrGatherTune {
    static constexpr int MIN_BLOCKS = 4;     // generic gather: 110-120 VGPRs, 5 workgroups/CU (96) spills in both texel formats.  The class
                                             // gathers take 64-78 (two line taps) / 86-88 (keyframe blend) registers and run 6 / 5 per CU as they are.
                                             // Round 6, DoNeRF (78): capped at 72 (3 spills) 0.70 ms, at 64 (21 spills) 1.12 against 0.68; held to
                                             // 5 / 4 per CU by LDS 0.745 / 0.883 (profiles/r06_k2_occupancy_ab*.txt); the keyframe form capped at 80:
                                             // 7-9 spills, slower in round 5 (0.78 vs 0.76 ms)
};

// acc[j] (+)= w * texel[q0 + j] for the first min(nb, G) channel groups of one tap; `off` is the
// BYTE offset of the tap's texel.  FIRST: acc = v * w, else acc = fma(v, w, acc) (ATen's bilinear order).
template <bool HALF, int G, bool FIRST>
__device__ __forceinline__ void hr_tap(const void* base, unsigned off, int q0, int nb, float w, float4 (&acc)[G])
{
    auto put = [&](int j, const float4 v) {
        if (FIRST) {
            acc[j].x = v.x * w; acc[j].y = v.y * w; acc[j].z = v.z * w; acc[j].w = v.w * w;
        } else {
            acc[j].x = HR_FMA(v.x, w, acc[j].x); acc[j].y = HR_FMA(v.y, w, acc[j].y);
            acc[j].z = HR_FMA(v.z, w, acc[j].z); acc[j].w = HR_FMA(v.w, w, acc[j].w);
        }
    };
    if constexpr (!HALF) {
        const float4* p = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(base) + (size_t)(off + 16u * (unsigned)q0));
        float4 v[G];
#pragma unroll
        for (int j = 0; j < G; ++j)
            if (j < nb) v[j] = p[j];
#pragma unroll
        for (int j = 0; j < G; ++j)
            if (j < nb) put(j, v[j]);
    } else {
        const hr_half8* p = reinterpret_cast<const hr_half8*>(reinterpret_cast<const char*>(base) + (size_t)(off + 16u * (unsigned)(q0 >> 1)));
        constexpr int NO = (G + 1) / 2;
        hr_half8 h[NO];
#pragma unroll
        for (int o = 0; o < NO; ++o)
            if (2 * o < nb) h[o] = p[o];
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            if (2 * o < nb) put(2 * o, make_float4((float)h[o][0], (float)h[o][1], (float)h[o][2], (float)h[o][3]));
            if (2 * o + 1 < nb && 2 * o + 1 < G) put(2 * o + 1, make_float4((float)h[o][4], (float)h[o][5], (float)h[o][6], (float)h[o][7]));
        }
    }
}

// All channel groups of one plane pair for a sample at normalised coordinates pn: bilinear
// plane tap x (line | time-plane) tap, density partial sum and appearance decode.
// HALF: float16 texels, one 16-byte load brings two channel groups (half the load instructions and
// half the bytes); values are widened to fp32 before any arithmetic.
// (Measured alternatives, both slower than this plain loop at 5 waves/SIMD: a 4-lanes-per-sample
//  gather with LDS hand-over, 1.66 vs 1.27 ms per frame; compile-time unrolled batches of 12-16
//  loads in flight at 4 waves/SIMD, 1.37 ms.  The gather sits at ~1.1 vector-L1 accesses per
//  clock per CU, i.e. it is bound by the tag-lookup rate for scattered 16-byte reads.)
template <bool HALF, int G, int J, bool DEN = false>
__device__ __forceinline__ void hr_gather_plane(const HrGridPlane& g, const HrAxisTaps& at, const float* M, int CA,
                                                float& sig_feat, float& pre0, float& pre1, float& pre2, const float* Dj = nullptr)
{
    const int ng = g.cd4 + g.ca4;
    const int cd = g.cd4;
    if (ng == 0) return;
    const int tex = g.tex;
    const hr_axis_tap tx = at.ax[HrPlaneAxes<J>::A0];
    const hr_axis_tap ty = at.ax[HrPlaneAxes<J>::A1];
    // ATen: nw = (x1-ix)(y1-iy), ne = (ix-x0)(y1-iy), sw = (x1-ix)(iy-y0), se = (ix-x0)(iy-y0)
    const float w00 = tx.w0 * ty.w0, w01 = tx.w1 * ty.w0, w10 = tx.w0 * ty.w1, w11 = tx.w1 * ty.w1;
    const bool line = (g.bw == 1);
    // line: grid x == 0 on a width-1 image puts weight exactly 1 on column 0 -> 2 taps along the axis;
    // time plane: x = spatial coordinate, y = keyframe time -> 4 taps
    const hr_axis_tap bxp = at.ax[HrPlaneAxes<J>::V];
    const hr_axis_tap byp = at.t;
    const float v00 = bxp.w0 * byp.w0, v01 = bxp.w1 * byp.w0, v10 = bxp.w0 * byp.w1, v11 = bxp.w1 * byp.w1;
    // BYTE offsets of the taps' texels, unsigned 32-bit: a load is then `uniform base + zero-extended VGPR offset` and
    // needs no 64-bit address arithmetic
    const unsigned esz = HALF ? 2u : 4u, texb = (unsigned)tex * esz;
    const unsigned ia00 = (unsigned)(ty.i0 * g.aw + tx.i0) * texb, ia01 = (unsigned)(ty.i0 * g.aw + tx.i1) * texb;
    const unsigned ia10 = (unsigned)(ty.i1 * g.aw + tx.i0) * texb, ia11 = (unsigned)(ty.i1 * g.aw + tx.i1) * texb;
    const unsigned ib00 = line ? (unsigned)bxp.i0 * texb : (unsigned)(byp.i0 * g.bw + bxp.i0) * texb;
    const unsigned ib01 = line ? (unsigned)bxp.i1 * texb : (unsigned)(byp.i0 * g.bw + bxp.i1) * texb;
    const unsigned ib10 = (unsigned)(byp.i1 * g.bw + bxp.i0) * texb, ib11 = (unsigned)(byp.i1 * g.bw + bxp.i1) * texb;
    if constexpr (HALF) {
        // float16 texels: one 16-byte load brings two channel groups; octet-major order (all taps of an octet, then the
        // next octet) keeps 96 VGPRs without spills and measured 0.86 vs 1.08 ms against the tap-major form below
        const char* A = reinterpret_cast<const char*>(g.a);
        const char* B = reinterpret_cast<const char*>(g.b);
        auto ld = [](const char* p, int o) { return *reinterpret_cast<const hr_half8*>(p + (size_t)(16u * (unsigned)o)); };
        auto lo4 = [](const hr_half8 h) { return make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]); };
        auto hi4 = [](const hr_half8 h) { return make_float4((float)h[4], (float)h[5], (float)h[6], (float)h[7]); };
        const int no = (ng + 1) >> 1;
        for (int o = 0; o < no; ++o) {
            const hr_half8 a00 = ld(A + ia00, o), a01 = ld(A + ia01, o), a10 = ld(A + ia10, o), a11 = ld(A + ia11, o);
            const hr_half8 b00 = ld(B + ib00, o), b01 = ld(B + ib01, o);
            hr_half8 b10 = b00, b11 = b01;
            if (!line) { b10 = ld(B + ib10, o); b11 = ld(B + ib11, o); }
            {
                const float4 pa = hr_bilerp4(lo4(a00), lo4(a01), lo4(a10), lo4(a11), w00, w01, w10, w11);
                const float4 pb = line ? hr_lerp4(lo4(b00), lo4(b01), bxp.w0, bxp.w1)
                                       : hr_bilerp4(lo4(b00), lo4(b01), lo4(b10), lo4(b11), v00, v01, v10, v11);
                hr_consume_group<DEN>(g, 2 * o, cd, pa, pb, M, CA, sig_feat, pre0, pre1, pre2, Dj);
            }
            if (2 * o + 1 < ng) {
                const float4 pa = hr_bilerp4(hi4(a00), hi4(a01), hi4(a10), hi4(a11), w00, w01, w10, w11);
                const float4 pb = line ? hr_lerp4(hi4(b00), hi4(b01), bxp.w0, bxp.w1)
                                       : hr_bilerp4(hi4(b00), hi4(b01), hi4(b10), hi4(b11), v00, v01, v10, v11);
                hr_consume_group<DEN>(g, 2 * o + 1, cd, pa, pb, M, CA, sig_feat, pre0, pre1, pre2, Dj);
            }
        }
        return;
    }
    // Tap-major order: per pass, up to G channel groups of ONE tap's texel are read back to back (a
    // contiguous 64-byte run for fp32 texels, 32 bytes for fp16), then the next tap.  The accumulators carry
    // ATen's summation order (nw, ne, sw, se).  Group-major order (all taps of one group, then the next group)
    // touches 6-8 different cache lines per lane between two reads of the same texel and measured an L1 hit
    // rate of only 61 % on the keyframe model with 64 samples per ray (12x the L2 requests of DoNeRF).
    for (int q0 = 0; q0 < ng; q0 += G) {
        const int nb = ng - q0;
        float4 pa[G], pb[G];
        hr_tap<HALF, G, true>(g.a, ia00, q0, nb, w00, pa);
        hr_tap<HALF, G, false>(g.a, ia01, q0, nb, w01, pa);
        hr_tap<HALF, G, false>(g.a, ia10, q0, nb, w10, pa);
        hr_tap<HALF, G, false>(g.a, ia11, q0, nb, w11, pa);
        if (line) {
            hr_tap<HALF, G, true>(g.b, ib00, q0, nb, bxp.w0, pb);
            hr_tap<HALF, G, false>(g.b, ib01, q0, nb, bxp.w1, pb);
        } else {
            hr_tap<HALF, G, true>(g.b, ib00, q0, nb, v00, pb);
            hr_tap<HALF, G, false>(g.b, ib01, q0, nb, v01, pb);
            hr_tap<HALF, G, false>(g.b, ib10, q0, nb, v10, pb);
            hr_tap<HALF, G, false>(g.b, ib11, q0, nb, v11, pb);
        }
#pragma unroll
        for (int j = 0; j < G; ++j)
            if (j < nb) hr_consume_group<DEN>(g, q0 + j, cd, pa[j], pb[j], M, CA, sig_feat, pre0, pre1, pre2, Dj);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Quad-cooperative gather (fp32 texels).  The vector-memory address unit charges a scattered 16-byte lane access
// about a cycle, but serves the 4 lanes of a quad reading 64 CONTIGUOUS bytes at more than twice that rate
// (tools/gather_ubench.hip, L1-resident: 1.4 vs 3.0 lane-loads per clock per CU; L2-resident 1.0 vs 1.7).
// So for the gather the four lanes of a quad stop working on their own samples and take one channel group each
// of ONE sample at a time: the owner's taps are broadcast inside the quad with DPP moves, each lane loads its
// float4 of every tap (one 64-byte run per tap and quad), forms plane x line for its group, and the four partial
// results (density sum, three decode dot products) are summed with two DPP steps and kept by the owner.
// The quad's lanes are consecutive samples of one ray (ZP >= 8), so they share the ray's decode matrix M.

struct HrTaps {                 // one plane pair's taps of one sample: BYTE offsets of the texels (unsigned 32-bit, so
    unsigned ia[4];             //   that a load is `uniform base + zero-extended VGPR offset`: no 64-bit address
    float wa[4];                //   arithmetic per load) and weights.  plane: nw, ne, sw, se
    unsigned ib[4];             // line: low, high (2 used) / time plane: 4
    float wb[4];
};

template <int J>
__device__ __forceinline__ HrTaps hr_make_taps(const HrGridPlane& g, const HrAxisTaps& at)
{
    HrTaps t;
    const unsigned tex = (unsigned)g.tex * 4u;            // bytes per fp32 texel
    const hr_axis_tap tx = at.ax[HrPlaneAxes<J>::A0];
    const hr_axis_tap ty = at.ax[HrPlaneAxes<J>::A1];
    t.wa[0] = tx.w0 * ty.w0; t.wa[1] = tx.w1 * ty.w0; t.wa[2] = tx.w0 * ty.w1; t.wa[3] = tx.w1 * ty.w1;
    t.ia[0] = (unsigned)(ty.i0 * g.aw + tx.i0) * tex; t.ia[1] = (unsigned)(ty.i0 * g.aw + tx.i1) * tex;
    t.ia[2] = (unsigned)(ty.i1 * g.aw + tx.i0) * tex; t.ia[3] = (unsigned)(ty.i1 * g.aw + tx.i1) * tex;
    const bool line = (g.bw == 1);
    const hr_axis_tap bxp = at.ax[HrPlaneAxes<J>::V];
    const hr_axis_tap byp = at.t;
    if (line) {
        t.ib[0] = (unsigned)bxp.i0 * tex; t.ib[1] = (unsigned)bxp.i1 * tex; t.ib[2] = 0; t.ib[3] = 0;
        t.wb[0] = bxp.w0; t.wb[1] = bxp.w1; t.wb[2] = 0.0f; t.wb[3] = 0.0f;
    } else {
        t.ib[0] = (unsigned)(byp.i0 * g.bw + bxp.i0) * tex; t.ib[1] = (unsigned)(byp.i0 * g.bw + bxp.i1) * tex;
        t.ib[2] = (unsigned)(byp.i1 * g.bw + bxp.i0) * tex; t.ib[3] = (unsigned)(byp.i1 * g.bw + bxp.i1) * tex;
        t.wb[0] = bxp.w0 * byp.w0; t.wb[1] = bxp.w1 * byp.w0; t.wb[2] = bxp.w0 * byp.w1; t.wb[3] = bxp.w1 * byp.w1;
    }
    return t;
}

// One owner at a time.  LPS = lanes per sample: 4 (the quad serves owner lane T of the quad) or 2 (each pair serves
// its own lane T; used for plane pairs with exactly two channel groups so that no lane idles).
// A step is split in two so that the loads of the NEXT owner can be in flight while this owner's texels are consumed
// (a sample wavefront of the frame kernel shares its SIMD with only one other: nothing else hides the 1-2 k cycles of an
// L2 / Infinity-Cache hit): hr_coop_issue broadcasts the owner's taps and issues this lane's loads, hr_coop_consume does
// the arithmetic.  The float4 arithmetic is written on float2 halves: v_pk_mul_f32 / v_pk_fma_f32 / v_pk_add_f32 do two
// IEEE operations per issue slot with the same roundings as the scalar forms.
typedef float hr_f2 __attribute__((ext_vector_type(2)));
typedef float hr_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ hr_f2 hr_fma2(hr_f2 a, hr_f2 b, hr_f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ hr_f2 hr_splat2(float w) { return hr_f2{w, w}; }

// base + m . (lo, hi) as ONE chain of multiply-adds (FIRST: base is known to be zero, the chain starts with a multiply).  The library is built
// without packed fp32 instructions (build.py): two half sums and their addition would cost two instructions more per output.
template <bool FIRST>
__device__ __forceinline__ float hr_dot4(const hr_f4 m, const hr_f2 lo, const hr_f2 hi, float base)
{
    const float t = FIRST ? m.x * lo.x : HR_FMA(m.x, lo.x, base);
    return HR_FMA(m.w, hi.y, HR_FMA(m.z, hi.x, HR_FMA(m.y, lo.y, t)));
}

template <int NB>
struct HrCoopLoad {             // one lane's share of one owner's taps: its channel group of every texel
    hr_f4 a[4];                 // plane: nw, ne, sw, se
    hr_f4 b[NB];                // line: low, high (NB = 2) / time plane: 4
    float wa[4], wb[NB];
    int q;                      // the channel group
    bool v;                     // owner valid and q < ng
};

// NB: taps of the second factor the code is compiled for: 2 = a line (static nets only), 4 = line or time plane (runtime)
template <int LPS, int T, int NB>
__device__ __forceinline__ void hr_coop_issue(const HrGridPlane& g, const HrTaps& mine, bool my_valid, int q0, HrCoopLoad<NB>& L)
{
    // quad_perm selecting the owner: [T,T,T,T] for quads, [T,T,2+T,2+T] for pairs
    constexpr int B = (LPS == 4) ? T * 0x55 : (T | (T << 2) | ((2 + T) << 4) | ((2 + T) << 6));
    const int ng = g.cd4 + g.ca4;
    const bool line = (NB == 2) || (g.bw == 1);
    L.q = q0 + ((int)threadIdx.x & (LPS - 1));            // this lane's channel group
    L.v = (hr_dpp_i<B>(my_valid ? 1 : 0) != 0) && (L.q < ng);
    unsigned ia[4], ib[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        ia[i] = (unsigned)hr_dpp_i<B>((int)mine.ia[i]);
        L.wa[i] = hr_dpp_f<B>(mine.wa[i]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        ib[i] = (unsigned)hr_dpp_i<B>((int)mine.ib[i]);
        L.wb[i] = hr_dpp_f<B>(mine.wb[i]);
    }
    if constexpr (NB == 4) {
        if (!line) {
#pragma unroll
            for (int i = 2; i < 4; ++i) {
                ib[i] = (unsigned)hr_dpp_i<B>((int)mine.ib[i]);
                L.wb[i] = hr_dpp_f<B>(mine.wb[i]);
            }
        }
    }
    if (L.v) {
        const char* A = reinterpret_cast<const char*>(g.a);
        const char* Bp = reinterpret_cast<const char*>(g.b);
        const unsigned qb = 16u * (unsigned)L.q;
        auto ld = [qb](const char* p, unsigned off) { return *reinterpret_cast<const hr_f4*>(p + (size_t)(off + qb)); };
#pragma unroll
        for (int i = 0; i < 4; ++i) L.a[i] = ld(A, ia[i]);
        L.b[0] = ld(Bp, ib[0]);
        L.b[1] = ld(Bp, ib[1]);
        if constexpr (NB == 4) {
            if (!line) { L.b[2] = ld(Bp, ib[2]); L.b[3] = ld(Bp, ib[3]); }
        }
    }
}

template <int LPS, int T, int NB, bool DEN = false>
__device__ __forceinline__ void hr_coop_consume(const HrGridPlane& g, const HrCoopLoad<NB>& L, const float* M, int CA,
                                                float& sig_feat, float& pre0, float& pre1, float& pre2, const float* Dj = nullptr)
{
    const int j = (int)threadIdx.x & (LPS - 1);
    const bool line = (NB == 2) || (g.bw == 1);
    float s = 0.0f, p0 = 0.0f, p1 = 0.0f, p2 = 0.0f;
    if (L.v) {
        // bilinear taps in ATen's order (nw, ne, sw, se; grid_sampler_2d), two channels per instruction
        const hr_f2 w0 = hr_splat2(L.wa[0]), w1 = hr_splat2(L.wa[1]), w2 = hr_splat2(L.wa[2]), w3 = hr_splat2(L.wa[3]);
        const hr_f2 pa_lo = hr_fma2(L.a[3].xy, w3, hr_fma2(L.a[2].xy, w2, hr_fma2(L.a[1].xy, w1, L.a[0].xy * w0)));
        const hr_f2 pa_hi = hr_fma2(L.a[3].zw, w3, hr_fma2(L.a[2].zw, w2, hr_fma2(L.a[1].zw, w1, L.a[0].zw * w0)));
        const hr_f2 v0 = hr_splat2(L.wb[0]), v1 = hr_splat2(L.wb[1]);
        hr_f2 pb_lo = hr_fma2(L.b[1].xy, v1, L.b[0].xy * v0);
        hr_f2 pb_hi = hr_fma2(L.b[1].zw, v1, L.b[0].zw * v0);
        if constexpr (NB == 4) {
            if (!line) {
                const hr_f2 v2 = hr_splat2(L.wb[2]), v3 = hr_splat2(L.wb[3]);
                pb_lo = hr_fma2(L.b[3].xy, v3, hr_fma2(L.b[2].xy, v2, pb_lo));
                pb_hi = hr_fma2(L.b[3].zw, v3, hr_fma2(L.b[2].zw, v2, pb_hi));
            }
        }
        const hr_f2 f_lo = pa_lo * pb_lo, f_hi = pa_hi * pb_hi;          // plane x line, 4 channels
        if (L.q < g.cd4) {                                               // density: sum over the channels
            if constexpr (DEN) {                                         // (density modes: through the ray's density row)
                s = hr_dot4<true>(*reinterpret_cast<const hr_f4*>(Dj + 4 * L.q), f_lo, f_hi, 0.0f);
            } else {
                const hr_f2 t = f_lo + f_hi;
                s = t.x + t.y;
            }
        } else {                                                         // appearance: through the ray's decode matrix
            const int ch = g.app_off + 4 * (L.q - g.cd4);
            const hr_f4 m0 = *reinterpret_cast<const hr_f4*>(M + ch);
            const hr_f4 m1 = *reinterpret_cast<const hr_f4*>(M + CA + ch);
            const hr_f4 m2 = *reinterpret_cast<const hr_f4*>(M + 2 * CA + ch);
            p0 = hr_dot4<true>(m0, f_lo, f_hi, 0.0f); p1 = hr_dot4<true>(m1, f_lo, f_hi, 0.0f); p2 = hr_dot4<true>(m2, f_lo, f_hi, 0.0f);
        }
    }
    // sum over the cooperating lanes: neighbour, then (quads) the other pair
    s += hr_dpp_f<0xB1>(s); p0 += hr_dpp_f<0xB1>(p0); p1 += hr_dpp_f<0xB1>(p1); p2 += hr_dpp_f<0xB1>(p2);
    if (LPS == 4) { s += hr_dpp_f<0x4E>(s); p0 += hr_dpp_f<0x4E>(p0); p1 += hr_dpp_f<0x4E>(p1); p2 += hr_dpp_f<0x4E>(p2); }
    if (j == T) { sig_feat += s; pre0 += p0; pre1 += p1; pre2 += p2; }
}

// All owners of one plane pair.  PIPE 2: owner T+1's loads are issued before owner T is consumed (two HrCoopLoad sets
// live: ~70 more VGPRs -- for kernels that run at <= 3 wavefronts per SIMD); PIPE 1: one owner at a time.
template <int LPS, int PIPE, int NB, bool DEN = false>
__device__ __forceinline__ void hr_gather_coop_owners(const HrGridPlane& g, const HrTaps& mine, bool valid, const float* M, int CA,
                                                      float& sig_feat, float& pre0, float& pre1, float& pre2, const float* Dj = nullptr)
{
    const int ng = g.cd4 + g.ca4;
    for (int q0 = 0; q0 < ng; q0 += LPS) {                // one round unless the texel has more than LPS channel groups
        if constexpr (PIPE == 1) {
            // (the scheduling fences keep the compiler from overlapping the owners on its own: at 4 wavefronts per SIMD
            //  there are no registers for a second set of texels, and the other wavefronts hide the latency)
            HrCoopLoad<NB> L;
            hr_coop_issue<LPS, 0, NB>(g, mine, valid, q0, L); hr_coop_consume<LPS, 0, NB, DEN>(g, L, M, CA, sig_feat, pre0, pre1, pre2, Dj);
            __builtin_amdgcn_sched_barrier(0);
            hr_coop_issue<LPS, 1, NB>(g, mine, valid, q0, L); hr_coop_consume<LPS, 1, NB, DEN>(g, L, M, CA, sig_feat, pre0, pre1, pre2, Dj);
            if constexpr (LPS == 4) {
                __builtin_amdgcn_sched_barrier(0);
                hr_coop_issue<LPS, 2, NB>(g, mine, valid, q0, L); hr_coop_consume<LPS, 2, NB, DEN>(g, L, M, CA, sig_feat, pre0, pre1, pre2, Dj);
                __builtin_amdgcn_sched_barrier(0);
                hr_coop_issue<LPS, 3, NB>(g, mine, valid, q0, L); hr_coop_consume<LPS, 3, NB, DEN>(g, L, M, CA, sig_feat, pre0, pre1, pre2, Dj);
            }
            __builtin_amdgcn_sched_barrier(0);
        } else {
            HrCoopLoad<NB> L0, L1;
            hr_coop_issue<LPS, 0, NB>(g, mine, valid, q0, L0);
            hr_coop_issue<LPS, 1, NB>(g, mine, valid, q0, L1);
            hr_coop_consume<LPS, 0, NB, DEN>(g, L0, M, CA, sig_feat, pre0, pre1, pre2, Dj);
            if constexpr (LPS == 4) {
                hr_coop_issue<LPS, 2, NB>(g, mine, valid, q0, L0);
                hr_coop_consume<LPS, 1, NB, DEN>(g, L1, M, CA, sig_feat, pre0, pre1, pre2, Dj);
                hr_coop_issue<LPS, 3, NB>(g, mine, valid, q0, L1);
                hr_coop_consume<LPS, 2, NB, DEN>(g, L0, M, CA, sig_feat, pre0, pre1, pre2, Dj);
                hr_coop_consume<LPS, 3, NB, DEN>(g, L1, M, CA, sig_feat, pre0, pre1, pre2, Dj);
            } else {
                hr_coop_consume<LPS, 1, NB, DEN>(g, L1, M, CA, sig_feat, pre0, pre1, pre2, Dj);
            }
        }
    }
}

template <int J, int PIPE, int NB, bool DEN = false>
__device__ __forceinline__ void hr_gather_plane_coop(const HrGridPlane& g, const HrAxisTaps& at, bool valid, const float* M, int CA,
                                                     float& sig_feat, float& pre0, float& pre1, float& pre2, const float* Dj = nullptr)
{
    const int ng = g.cd4 + g.ca4;
    if (ng == 0) return;
    if (ng == 1) {               // a single 16-byte group per texel: nothing to share
        if (valid) hr_gather_plane<false, 1, J, DEN>(g, at, M, CA, sig_feat, pre0, pre1, pre2, Dj);
        return;
    }
    const HrTaps mine = hr_make_taps<J>(g, at);
    if (ng == 2) hr_gather_coop_owners<2, (PIPE > 2) ? 2 : 1, NB, DEN>(g, mine, valid, M, CA, sig_feat, pre0, pre1, pre2, Dj);
    else hr_gather_coop_owners<4, PIPE, NB, DEN>(g, mine, valid, M, CA, sig_feat, pre0, pre1, pre2, Dj);
}

// ---------------------------------------------------------------------------------------------------------
// Plane class "844": the decomposition every benchmark family ships -- n_lamb_sigma = n_lamb_sh = [8, 4, 4], fp32 texels
// (plane pair 0: 2 density + 2 appearance groups = 64-byte texels, a quad per sample; pairs 1, 2: 1 + 1 groups = 32-byte
// texels, a lane pair per sample).  With the texel size, the lane roles and the decode-matrix stride known at compile time
// the cooperative gather sheds most of its bookkeeping (VALU instructions per sample slot, PMC SQ_INSTS_VALU):
//   * the four taps of a plane are ONE broadcast offset: hr_make_tap_c clamps the taps to (i, i + 1), so the other three
//     texels are immediate offsets (+TEXB) from two uniform base pointers (row y0 and row y0 + 1): 1 instead of 4 offset
//     broadcasts and address additions per plane, 1 instead of 2 per line;
//   * partial sums stay per owner in registers and are reduced across the quad / pair ONCE per sample (a 4x4 / 2x2
//     transpose-add with DPP) instead of after every owner;
//   * texel offsets are 24-bit multiply-adds and shifts (no quarter-rate 32-bit integer multiplies).
template <int J>
struct HrPc844 {
    static constexpr int CD4 = (J == 0) ? 2 : 1;
    static constexpr int NG = 2 * CD4;                     // channel groups = cooperating lanes
    static constexpr int TEXB = 16 * NG;                   // bytes per texel
    static constexpr int SH = (J == 0) ? 6 : 5;            // log2(TEXB)
    static constexpr int APP_OFF = (J == 0) ? 0 : ((J == 1) ? 8 : 12);   // first decode-matrix slot of this pair's appearance channels
};

struct HrAxisTapsC {
    hr_axis_tap_c ax[3];        // x @ grid[0], y @ grid[1], z @ grid[2]
    hr_axis_tap_c t;            // keyframe axis (video)
};

template <int NB>
struct HrTapsC {                // one plane pair's taps of one sample
    unsigned oa, ob;            // byte offsets of the (y0, x0) texel of the plane and of the low texel of the line / time plane
    float wa[4];                // nw, ne, sw, se
    float wb[NB];               // line: low, high; time plane: 4
};

// float16 texels of the same decomposition: plane pair 0 = two 16-byte octets (8 density | 8 appearance channels), a lane
// pair per sample; pairs 1, 2 = ONE octet (4 density | 4 appearance), every lane gathers its own sample
template <int J>
struct HrPc844h {
    static constexpr int NG = (J == 0) ? 2 : 1;            // octets per texel = cooperating lanes
    static constexpr int TEXB = 16 * NG;
    static constexpr int SH = (J == 0) ? 5 : 4;
    static constexpr int APP_OFF = HrPc844<J>::APP_OFF;
};

template <int J, int NB, class PC = HrPc844<J>>
__device__ __forceinline__ HrTapsC<NB> hr_make_taps_c(const HrGridPlane& g, const HrAxisTapsC& at)
{
    HrTapsC<NB> t;
    const hr_axis_tap_c tx = at.ax[HrPlaneAxes<J>::A0], ty = at.ax[HrPlaneAxes<J>::A1], bx = at.ax[HrPlaneAxes<J>::V];
    t.oa = ((unsigned)__umul24((unsigned)ty.i0, (unsigned)g.aw) + (unsigned)tx.i0) << PC::SH;
    t.wa[0] = tx.w0 * ty.w0; t.wa[1] = tx.w1 * ty.w0; t.wa[2] = tx.w0 * ty.w1; t.wa[3] = tx.w1 * ty.w1;
    const bool line = (NB == 2) || (g.bw == 1);
    if (line) {
        t.ob = (unsigned)bx.i0 << PC::SH;
        t.wb[0] = bx.w0; t.wb[1] = bx.w1;
        if constexpr (NB == 4) { t.wb[2] = 0.0f; t.wb[3] = 0.0f; }
    } else if constexpr (NB == 4) {
        t.ob = ((unsigned)__umul24((unsigned)at.t.i0, (unsigned)g.bw) + (unsigned)bx.i0) << PC::SH;
        t.wb[0] = bx.w0 * at.t.w0; t.wb[1] = bx.w1 * at.t.w0; t.wb[2] = bx.w0 * at.t.w1; t.wb[3] = bx.w1 * at.t.w1;
    }
    return t;
}

// What a density lane multiplies its features with: its "decode matrix row" is 1 1 1 1 (1 x 8 for an octet of halfs), so that density and
// appearance lanes run the SAME instructions on the same registers -- a divergent if / else costs both sides' instructions plus, for every
// register only one side writes, a zero fill on the other (the round-5 form: ~100 of K2's 1 300 vector instructions per sample slot).
// Rows 1, 2 of that "matrix" (at +CA, +2 CA floats) are zeros.  HR_GATHER_ONES floats of the CALLER's LDS, filled by hr_gather_ones_init()
// before the barrier that publishes the ray's decode matrix (sample_kernel.hip, fused_impl.inc, train_kernel.hip) -- the caller's, not a
// __shared__ variable of this file: static LDS in front of the frame kernel's dynamic tile moved every LDS address of its MLP role and cost
// that role, which lives on exactly 168 registers, the four accumulator tiles it then spilled (1.85 vs 1.71 ms per frame).
// (HR_GATHER_ONES itself: hr_plan.h, which sizes the frame kernel's LDS with it)
__device__ __forceinline__ void hr_gather_ones_init(float* ones)
{
    const int t = (int)threadIdx.x;
    if (t < HR_GATHER_ONES) ones[t] = t < 8 ? 1.0f : 0.0f;
}

// a value nobody reads before it is written (no instruction; tells the compiler the register needs no zero on the paths that skip the write)
#define HR_UNDEF(x) asm volatile("" : "=v"(x))
#ifdef HR_GATHER_FENCED            // sample_kernel.hip: the kernel that lives on 80 registers
#define HR_GATHER_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define HR_GATHER_SCHED_FENCE() do {} while (0)
#endif
#define HR_TAP_MASKED 0xffffffffu      // HrTapsC::oa of a masked sample (a texel offset is < 2^31: 46 340^2 texels of 64 bytes would be needed)

// owner T of the quad / pair: broadcast its taps, load this lane's channel group of the 6 (8) texels, accumulate into x:
// appearance lanes (Mj: the lane's 4 columns of the ray's decode matrix): the three decode dot products; density lanes (Mj: hr_gather_ones):
// x[0] = the sum over the channels, x[1] = x[2] = 0 -- no cross-lane traffic besides the broadcasts
// FIRST: nothing has been added to x yet: the sums are written, not added (`0 + x` is an instruction the compiler has to keep -- it differs
// from x for x = -0 -- and x need not be zeroed for the owners whose sample is masked: hr_coop_collect's results of those are never read)
template <int J, int T, int NB, int CA, bool FIRST = true>
__device__ __forceinline__ void hr_coop844_owner(const HrGridPlane& g, const HrTapsC<NB>& mine, const float* Mj, float (&x)[3])
{
    using PC = HrPc844<J>;
    constexpr int LPS = PC::NG;
    constexpr int B = (LPS == 4) ? T * 0x55 : (T | (T << 2) | ((2 + T) << 4) | ((2 + T) << 6));
    const int j = (int)threadIdx.x & (LPS - 1);
    const bool line = (NB == 2) || (g.bw == 1);
    const unsigned oa_t = (unsigned)hr_dpp_i<B>((int)mine.oa);           // HR_TAP_MASKED: the owner's sample is masked (one broadcast for offset and validity)
    const bool v = oa_t != HR_TAP_MASKED;
    const unsigned qb = 16u * (unsigned)j;
    const unsigned oa = oa_t + qb;
    const unsigned ob = (unsigned)hr_dpp_i<B>((int)mine.ob) + qb;
    float wa[4], wb[NB];
#pragma unroll
    for (int i = 0; i < 4; ++i) wa[i] = hr_dpp_f<B>(mine.wa[i]);
    wb[0] = hr_dpp_f<B>(mine.wb[0]);
    wb[1] = hr_dpp_f<B>(mine.wb[1]);
    if constexpr (NB == 4) {
        if (!line) { wb[2] = hr_dpp_f<B>(mine.wb[2]); wb[3] = hr_dpp_f<B>(mine.wb[3]); }
    }
    if (v) {
        const char* A0 = reinterpret_cast<const char*>(g.a);
        const char* A1 = A0 + (size_t)((unsigned)g.aw << PC::SH);          // row y0 + 1 (uniform)
        const char* B0 = reinterpret_cast<const char*>(g.b);
        auto ld = [](const char* p, unsigned off) { return *reinterpret_cast<const hr_f4*>(p + (size_t)off); };
        const hr_f4 a0 = ld(A0, oa), a1 = ld(A0 + PC::TEXB, oa), a2 = ld(A1, oa), a3 = ld(A1 + PC::TEXB, oa);
        const hr_f4 b0 = ld(B0, ob), b1 = ld(B0 + PC::TEXB, ob);
        // bilinear taps in ATen's order (nw, ne, sw, se; grid_sampler_2d)
        const hr_f2 w0 = hr_splat2(wa[0]), w1 = hr_splat2(wa[1]), w2 = hr_splat2(wa[2]), w3 = hr_splat2(wa[3]);
        const hr_f2 pa_lo = hr_fma2(a3.xy, w3, hr_fma2(a2.xy, w2, hr_fma2(a1.xy, w1, a0.xy * w0)));
        const hr_f2 pa_hi = hr_fma2(a3.zw, w3, hr_fma2(a2.zw, w2, hr_fma2(a1.zw, w1, a0.zw * w0)));
        const hr_f2 v0 = hr_splat2(wb[0]), v1 = hr_splat2(wb[1]);
        hr_f2 pb_lo = hr_fma2(b1.xy, v1, b0.xy * v0);
        hr_f2 pb_hi = hr_fma2(b1.zw, v1, b0.zw * v0);
        if constexpr (NB == 4) {
            if (!line) {
                const char* B1 = B0 + (size_t)((unsigned)g.bw << PC::SH);  // keyframe t0 + 1
                const hr_f4 b2 = ld(B1, ob), b3 = ld(B1 + PC::TEXB, ob);
                const hr_f2 v2 = hr_splat2(wb[2]), v3 = hr_splat2(wb[3]);
                pb_lo = hr_fma2(b3.xy, v3, hr_fma2(b2.xy, v2, pb_lo));
                pb_hi = hr_fma2(b3.zw, v3, hr_fma2(b2.zw, v2, pb_hi));
            }
        }
        const hr_f2 f_lo = pa_lo * pb_lo, f_hi = pa_hi * pb_hi;          // plane x line, 4 channels
        // (the matrix rows are read AFTER the 24 texel registers are dead: hoisted above the taps they cost the stand-alone kernel a wavefront
        // per SIMD -- 90 registers instead of 78)
        HR_GATHER_SCHED_FENCE();
        const hr_f4 m0 = *reinterpret_cast<const hr_f4*>(Mj);
        const hr_f4 m1 = *reinterpret_cast<const hr_f4*>(Mj + CA);
        const hr_f4 m2 = *reinterpret_cast<const hr_f4*>(Mj + 2 * CA);
        x[0] = hr_dot4<FIRST>(m0, f_lo, f_hi, x[0]);
        x[1] = hr_dot4<FIRST>(m1, f_lo, f_hi, x[1]);
        x[2] = hr_dot4<FIRST>(m2, f_lo, f_hi, x[2]);
    }
}

// x[T][i]: this lane's partial sums for owner T (density lanes: x[T][0] = density features; appearance lanes: x[T][0..2] = decode dot products)
// -> every owner's lane receives ITS sample's density feature sum (r[0]) and decode sums (r[1..3]).
// Quads (LPS 4: lanes 0, 1 density, lanes 2, 3 appearance): the neighbours add their partials, each keeping the owners of its parity; then the
// pairs trade -- a density lane's owner gets the appearance pair's sums, an appearance lane's owner the density pair's.
// Pairs (LPS 2: even lane density, odd lane appearance): one trade.
template <int LPS>
__device__ __forceinline__ void hr_coop_collect(const float (&x)[LPS][3], float (&r)[4])
{
    const int j = (int)threadIdx.x & (LPS - 1);
    const bool odd = (j & 1) != 0;
    if constexpr (LPS == 2) {
        const float send = odd ? x[0][0] : x[1][0];                       // odd: owner 0's first decode sum; even: owner 1's density
        const float recv = hr_dpp_f<0xB1>(send);
        r[0] = odd ? recv : x[0][0];
        r[1] = odd ? x[1][0] : recv;
        const float t1 = hr_dpp_f<0xB1>(x[0][1]), t2 = hr_dpp_f<0xB1>(x[0][2]);
        r[2] = odd ? x[1][1] : t1;
        r[3] = odd ? x[1][2] : t2;
    } else {
        const bool hi = (j & 2) != 0;
        float k0[3], k1[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            k0[i] = odd ? x[1][i] : x[0][i];
            k1[i] = odd ? x[3][i] : x[2][i];
            const float g0 = odd ? x[0][i] : x[1][i], g1 = odd ? x[2][i] : x[3][i];
            k0[i] += hr_dpp_f<0xB1>(g0);                                   // owner (j & 1)
            k1[i] += hr_dpp_f<0xB1>(g1);                                   // owner 2 + (j & 1)
        }
        const float send = hi ? k0[0] : k1[0];                            // appearance pair: owner (j & 1)'s first decode sum; density pair: owner 2 + (j & 1)'s density
        const float recv = hr_dpp_f<0x4E>(send);
        r[0] = hi ? recv : k0[0];
        r[1] = hi ? k1[0] : recv;
        const float t1 = hr_dpp_f<0x4E>(k0[1]), t2 = hr_dpp_f<0x4E>(k0[2]);
        r[2] = hi ? k1[1] : t1;
        r[3] = hi ? k1[2] : t2;
    }
}

// PC 1: [8, 4, 4]; PC 2: plane pair 0 only ([8, 0, 0], decode-matrix stride 8).  WRITES the four results.
// DEN (the time kernel's density modes, DESIGN 3m): `ones` is the ray's density row in the decode matrix's shape -- row 0: the weight of
// density slot 0 .. CA - 1 (the classes' density and appearance slots coincide), rows 1, 2: zeros -- and a density lane reads ITS four slots.
template <int NB, int PC, bool DEN = false>
__device__ __forceinline__ void hr_gather_844(const HrGridPlane* pl, const HrAxisTapsC& at, bool valid, const float* M, const float* ones,
                                              float& sig_feat, float& pre0, float& pre1, float& pre2)
{
    constexpr int CA = (PC == 2) ? 8 : 16;
    float out[4];
    const int lane = (int)threadIdx.x;
    {   // plane pair 0: a quad per sample, lane j <-> channel group j (0, 1 density; 2, 3 appearance)
        HrTapsC<NB> mine = hr_make_taps_c<0, NB>(pl[0], at);
        mine.oa = valid ? mine.oa : HR_TAP_MASKED;
        const float* Mj = (lane & 2) ? M + HrPc844<0>::APP_OFF + 4 * (lane & 1) : (DEN ? ones + 4 * (lane & 1) : ones);
        float x[4][3];
#pragma unroll
        for (int t = 0; t < 4; ++t) { HR_UNDEF(x[t][0]); HR_UNDEF(x[t][1]); HR_UNDEF(x[t][2]); }
        hr_coop844_owner<0, 0, NB, CA>(pl[0], mine, Mj, x[0]);
        hr_coop844_owner<0, 1, NB, CA>(pl[0], mine, Mj, x[1]);
        hr_coop844_owner<0, 2, NB, CA>(pl[0], mine, Mj, x[2]);
        hr_coop844_owner<0, 3, NB, CA>(pl[0], mine, Mj, x[3]);
        hr_coop_collect<4>(x, out);
    }
    if constexpr (PC == 1) {   // plane pairs 1 and 2: a lane pair per sample (lane 0 density, lane 1 appearance); one collection for both
        float x[2][3], r[4];
#pragma unroll
        for (int t = 0; t < 2; ++t) { HR_UNDEF(x[t][0]); HR_UNDEF(x[t][1]); HR_UNDEF(x[t][2]); }
        HrTapsC<NB> m1 = hr_make_taps_c<1, NB>(pl[1], at);
        m1.oa = valid ? m1.oa : HR_TAP_MASKED;
        const float* M1 = (lane & 1) ? M + HrPc844<1>::APP_OFF : (DEN ? ones + HrPc844<1>::APP_OFF : ones);
        hr_coop844_owner<1, 0, NB, CA>(pl[1], m1, M1, x[0]);
        hr_coop844_owner<1, 1, NB, CA>(pl[1], m1, M1, x[1]);
        HrTapsC<NB> m2 = hr_make_taps_c<2, NB>(pl[2], at);
        m2.oa = valid ? m2.oa : HR_TAP_MASKED;
        const float* M2 = (lane & 1) ? M + HrPc844<2>::APP_OFF : (DEN ? ones + HrPc844<2>::APP_OFF : ones);
        hr_coop844_owner<2, 0, NB, CA, false>(pl[2], m2, M2, x[0]);
        hr_coop844_owner<2, 1, NB, CA, false>(pl[2], m2, M2, x[1]);
        hr_coop_collect<2>(x, r);
        out[0] += r[0]; out[1] += r[1]; out[2] += r[2]; out[3] += r[3];
    }
    // a masked sample's sums were never written (its owner passes skip): nothing of them may reach the caller
    sig_feat = valid ? out[0] : 0.0f; pre0 = valid ? out[1] : 0.0f; pre1 = valid ? out[2] : 0.0f; pre2 = valid ? out[3] : 0.0f;
}

// ---------------------------------------------------------------------------------------------------------
// The same two classes with float16 texels.  A 16-byte load is an OCTET of channels; halfs are widened inside the
// multiply-adds (v_fma_mix_f32: half texel x fp32 weight + fp32 sum), so the arithmetic is the fp32 one on the rounded grid.

// d = half(texel word, low or high half) * w + c in ONE instruction (v_fma_mix_f32: the half operand is widened exactly,
// product and sum are one fused fp32 operation).  Left to itself the compiler widens first (v_cvt_f32_f16) and then uses
// packed fp32 multiply-adds: 1.5 instructions per channel and tap instead of 1.
template <int HI>
__device__ __forceinline__ float hr_fma_mix(unsigned word, float w, float c)
{
    float d;
    if constexpr (HI) asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(word), "v"(w), "v"(c));
    else asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(word), "v"(w), "v"(c));
    return d;
}
template <int HI>
__device__ __forceinline__ float hr_mul_mix(unsigned word, float w)           // fma(x, w, +0): the product (only a zero's sign can differ)
{
    float d;
    if constexpr (HI) asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(word), "v"(w));
    else asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(word), "v"(w));
    return d;
}

typedef unsigned hr_u4 __attribute__((ext_vector_type(4)));     // one octet: 8 halfs in 4 words

// one octet through the bilinear plane taps (ATen's order nw, ne, sw, se) and the line / time-plane taps -> 8 features,
// f[i] = channels (2i, 2i + 1): the two halfs of texel word i
template <int NB>
__device__ __forceinline__ void hr_oct_features(const hr_u4 a0, const hr_u4 a1, const hr_u4 a2, const hr_u4 a3,
                                                const hr_u4 b0, const hr_u4 b1, const hr_u4 b2, const hr_u4 b3,
                                                const float (&wa)[4], const float (&wb)[NB], bool line, hr_f2 (&f)[4])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        hr_f2 pa, pb;
        pa.x = hr_fma_mix<0>(a3[i], wa[3], hr_fma_mix<0>(a2[i], wa[2], hr_fma_mix<0>(a1[i], wa[1], hr_mul_mix<0>(a0[i], wa[0]))));
        pa.y = hr_fma_mix<1>(a3[i], wa[3], hr_fma_mix<1>(a2[i], wa[2], hr_fma_mix<1>(a1[i], wa[1], hr_mul_mix<1>(a0[i], wa[0]))));
        pb.x = hr_fma_mix<0>(b1[i], wb[1], hr_mul_mix<0>(b0[i], wb[0]));
        pb.y = hr_fma_mix<1>(b1[i], wb[1], hr_mul_mix<1>(b0[i], wb[0]));
        if constexpr (NB == 4) {
            if (!line) {
                pb.x = hr_fma_mix<0>(b3[i], wb[3], hr_fma_mix<0>(b2[i], wb[2], pb.x));
                pb.y = hr_fma_mix<1>(b3[i], wb[3], hr_fma_mix<1>(b2[i], wb[2], pb.y));
            }
        }
        f[i] = pa * pb;
    }
}

// sum of the 4 channels in f[0], f[1]
__device__ __forceinline__ float hr_sum4(const hr_f2* f) { const hr_f2 t = f[0] + f[1]; return t.x + t.y; }

// dot products of N4 groups of 4 features with the three rows of the decode matrix (row stride CA)
template <int N4, int CA, bool FIRST = false>
__device__ __forceinline__ void hr_decode_features(const hr_f2* f, const float* Mj, float& d0, float& d1, float& d2)
{
    float* const d[3] = {&d0, &d1, &d2};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float r = FIRST ? 0.0f : *d[i];
#pragma unroll
        for (int q = 0; q < N4; ++q) {
            const hr_f4 m = *reinterpret_cast<const hr_f4*>(Mj + i * CA + 4 * q);
            r = (FIRST && q == 0) ? hr_dot4<true>(m, f[0], f[1], 0.0f) : hr_dot4<false>(m, f[2 * q], f[2 * q + 1], r);
        }
        *d[i] = r;
    }
}

// plane pair 0, owner T of the lane pair: lane j loads octet j (0: density, 1: appearance) of the owner's 6 (8) texels; x as in
// hr_coop844_owner (density lane: Mj = hr_gather_ones -- eight ones: x[0] = the sum of the octet's features)
template <int T, int NB, int CA>
__device__ __forceinline__ void hr_coop844h_owner(const HrGridPlane& g, const HrTapsC<NB>& mine, const float* Mj, float (&x)[3])
{
    using PC = HrPc844h<0>;
    constexpr int B = T | (T << 2) | ((2 + T) << 4) | ((2 + T) << 6);
    const int j = (int)threadIdx.x & 1;
    const bool line = (NB == 2) || (g.bw == 1);
    const unsigned oa_t = (unsigned)hr_dpp_i<B>((int)mine.oa);
    const bool v = oa_t != HR_TAP_MASKED;
    const unsigned qb = 16u * (unsigned)j;
    const unsigned oa = oa_t + qb;
    const unsigned ob = (unsigned)hr_dpp_i<B>((int)mine.ob) + qb;
    float wa[4], wb[NB];
#pragma unroll
    for (int i = 0; i < 4; ++i) wa[i] = hr_dpp_f<B>(mine.wa[i]);
    wb[0] = hr_dpp_f<B>(mine.wb[0]);
    wb[1] = hr_dpp_f<B>(mine.wb[1]);
    if constexpr (NB == 4) {
        if (!line) { wb[2] = hr_dpp_f<B>(mine.wb[2]); wb[3] = hr_dpp_f<B>(mine.wb[3]); }
    }
    if (v) {
        const char* A0 = reinterpret_cast<const char*>(g.a);
        const char* A1 = A0 + (size_t)((unsigned)g.aw << PC::SH);
        const char* B0 = reinterpret_cast<const char*>(g.b);
        auto ld = [](const char* p, unsigned off) { return *reinterpret_cast<const hr_u4*>(p + (size_t)off); };
        const hr_u4 a0 = ld(A0, oa), a1 = ld(A0 + PC::TEXB, oa), a2 = ld(A1, oa), a3 = ld(A1 + PC::TEXB, oa);
        const hr_u4 b0 = ld(B0, ob), b1 = ld(B0 + PC::TEXB, ob);
        hr_u4 b2 = b0, b3 = b1;
        if constexpr (NB == 4) {
            if (!line) {
                const char* B1 = B0 + (size_t)((unsigned)g.bw << PC::SH);
                b2 = ld(B1, ob); b3 = ld(B1 + PC::TEXB, ob);
            }
        }
        hr_f2 f[4];
        hr_oct_features<NB>(a0, a1, a2, a3, b0, b1, b2, b3, wa, wb, line, f);
        HR_GATHER_SCHED_FENCE();                                            // (as in hr_coop844_owner)
        hr_decode_features<2, CA, true>(f, Mj, x[0], x[1], x[2]);           // x is this owner's alone: written, not added
    }
}

// plane pairs 1, 2: the lane's own sample, one octet per texel (4 density | 4 appearance channels)
template <int J, int NB, int CA, bool DEN = false>
__device__ __forceinline__ void hr_own844h(const HrGridPlane& g, const HrTapsC<NB>& t, bool valid, const float* M, float (&out)[4], const float* D = nullptr)
{
    using PC = HrPc844h<J>;
    const bool line = (NB == 2) || (g.bw == 1);
    if (valid) {
        const char* A0 = reinterpret_cast<const char*>(g.a);
        const char* A1 = A0 + (size_t)((unsigned)g.aw << PC::SH);
        const char* B0 = reinterpret_cast<const char*>(g.b);
        auto ld = [](const char* p, unsigned off) { return *reinterpret_cast<const hr_u4*>(p + (size_t)off); };
        const hr_u4 a0 = ld(A0, t.oa), a1 = ld(A0 + PC::TEXB, t.oa), a2 = ld(A1, t.oa), a3 = ld(A1 + PC::TEXB, t.oa);
        const hr_u4 b0 = ld(B0, t.ob), b1 = ld(B0 + PC::TEXB, t.ob);
        hr_u4 b2 = b0, b3 = b1;
        if constexpr (NB == 4) {
            if (!line) {
                const char* B1 = B0 + (size_t)((unsigned)g.bw << PC::SH);
                b2 = ld(B1, t.ob); b3 = ld(B1 + PC::TEXB, t.ob);
            }
        }
        hr_f2 f[4];
        hr_oct_features<NB>(a0, a1, a2, a3, b0, b1, b2, b3, t.wa, t.wb, line, f);
        if constexpr (DEN) out[0] = hr_dot4<false>(*reinterpret_cast<const hr_f4*>(D + PC::APP_OFF), f[0], f[1], out[0]);
        else out[0] += hr_sum4(f);
        hr_decode_features<1, CA>(f + 2, M + PC::APP_OFF, out[1], out[2], out[3]);
    }
}

template <int NB, int PC, bool DEN = false>
__device__ __forceinline__ void hr_gather_844h(const HrGridPlane* pl, const HrAxisTapsC& at, bool valid, const float* M, const float* ones,
                                               float& sig_feat, float& pre0, float& pre1, float& pre2)
{
    constexpr int CA = (PC == 2) ? 8 : 16;
    float out[4];
    {
        HrTapsC<NB> mine = hr_make_taps_c<0, NB, HrPc844h<0>>(pl[0], at);
        mine.oa = valid ? mine.oa : HR_TAP_MASKED;
        const float* Mj = ((int)threadIdx.x & 1) ? M + HrPc844h<0>::APP_OFF : ones;
        float x[2][3];
#pragma unroll
        for (int t = 0; t < 2; ++t) { HR_UNDEF(x[t][0]); HR_UNDEF(x[t][1]); HR_UNDEF(x[t][2]); }
        hr_coop844h_owner<0, NB, CA>(pl[0], mine, Mj, x[0]);
        hr_coop844h_owner<1, NB, CA>(pl[0], mine, Mj, x[1]);
        hr_coop_collect<2>(x, out);
    }
    if constexpr (PC == 1) {
        hr_own844h<1, NB, CA, DEN>(pl[1], hr_make_taps_c<1, NB, HrPc844h<1>>(pl[1], at), valid, M, out, ones);
        hr_own844h<2, NB, CA, DEN>(pl[2], hr_make_taps_c<2, NB, HrPc844h<2>>(pl[2], at), valid, M, out, ones);
    }
    // (a masked sample's sums were never written)
    sig_feat = valid ? out[0] : 0.0f; pre0 = valid ? out[1] : 0.0f; pre1 = valid ? out[2] : 0.0f; pre2 = valid ? out[3] : 0.0f;
}

#ifdef HR_PHASE_MARK     // tools/phase_table: comments in the assembly that delimit the phases
#define HR_SPH(i) do { __builtin_amdgcn_sched_barrier(0); asm volatile("; HRPHASE " #i ::: "memory"); } while (0)
#else
#define HR_SPH(i) do {} while (0)
#endif

// AlphaGridMask.sample_alpha(p) > 0 (utils/tensorf_utils.py:459-484; the test the reference carries at tensorf_no_sample.py:171-177)
__device__ __forceinline__ bool hr_occupancy_test(const HrSampleArgs& a, const float* p)
{
    const float gx = (p[0] - a.occ_lo[0]) * a.occ_inv[0] - 1.0f, gy = (p[1] - a.occ_lo[1]) * a.occ_inv[1] - 1.0f,
                gz = (p[2] - a.occ_lo[2]) * a.occ_inv[2] - 1.0f;
    // grid_sample's unnormalised coordinates (hr_make_tap's arithmetic).  Strictly inside a lattice cell all eight
    // trilinear weights are positive, so for a 0/1 volume `sample_alpha > 0` is one bit of a 1 MB table instead of eight
    // scattered reads of a 32 MB volume; on a lattice plane or outside the volume the exact sample decides
    const float ix = ((gx + 1.0f) / 2.0f) * (float)(a.occ_w - 1), iy = ((gy + 1.0f) / 2.0f) * (float)(a.occ_h - 1),
                iz = ((gz + 1.0f) / 2.0f) * (float)(a.occ_d - 1);
    const float fx = floorf(ix), fy = floorf(iy), fz = floorf(iz);
    const int cx = (int)fx, cy = (int)fy, cz = (int)fz;
    const bool interior = a.occ_cells && (ix > fx) && (iy > fy) && (iz > fz) && cx >= 0 && cy >= 0 && cz >= 0 &&
                          cx < a.occ_w - 1 && cy < a.occ_h - 1 && cz < a.occ_d - 1;
    if (interior) {
        const unsigned cell = ((unsigned)cz * (unsigned)(a.occ_h - 1) + (unsigned)cy) * (unsigned)(a.occ_w - 1) + (unsigned)cx;
        return (a.occ_cells[cell >> 5] >> (cell & 31u)) & 1u;
    }
    return hr_volume_sample(a.occ, a.occ_w, a.occ_h, a.occ_d, gx, gy, gz) > 0.0f;
}

// The ray's composited colour -> background, per-ray colour transforms, eval-mode clamp, store (tensorf_no_sample.py:236-247).
// scale_shift_color_one reads SAMPLE 0's head values (tensorf_utils.py:275-281): `hk0` = the ray's head row
__device__ __forceinline__ void hr_write_pixel(const hr_config& cfg, const HrSampleArgs& a, int64_t ray, const float* hk0, float c0, float c1, float c2, float acc_w)
{
    if (cfg.white_bg) {                        // tensorf_no_sample.py:236-237
        const float bg = 1.0f - acc_w;
        c0 += bg; c1 += bg; c2 += bg;
    }
    if (cfg.f_color_scale_global.offset >= 0 && cfg.f_color_scale_global.channels == 9) {
        // transform_color_one with the matrix from the HEAD (`color_transform_global`, tensorf_utils.py:308-320): sample 0's nine values, row-major
        const hr_head_field& fs = cfg.f_color_scale_global;
        const hr_head_field& fh = cfg.f_color_shift_global;
        float t[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) t[i] = hr_apply_act(fs.act, hk0[fs.offset + i]);
        const float n0 = c0 + ((c0 * t[0] + c1 * t[1]) + c2 * t[2]);
        const float n1 = c1 + ((c0 * t[3] + c1 * t[4]) + c2 * t[5]);
        const float n2 = c2 + ((c0 * t[6] + c1 * t[7]) + c2 * t[8]);
        c0 = n0 + hr_apply_act(fh.act, hk0[fh.offset + 0]);
        c1 = n1 + hr_apply_act(fh.act, hk0[fh.offset + 1]);
        c2 = n2 + hr_apply_act(fh.act, hk0[fh.offset + 2]);
    }
    else if (cfg.f_color_scale_global.offset >= 0) {   // scale_shift_color_one (tensorf_utils.py:275-281): sample 0's head
        const hr_head_field& fs = cfg.f_color_scale_global;
        const hr_head_field& fh = cfg.f_color_shift_global;
        c0 = c0 * (hr_apply_act(fs.act, hk0[fs.offset + 0]) + 1.0f) + hr_apply_act(fh.act, hk0[fh.offset + 0]);
        c1 = c1 * (hr_apply_act(fs.act, hk0[fs.offset + 1]) + 1.0f) + hr_apply_act(fh.act, hk0[fh.offset + 1]);
        c2 = c2 * (hr_apply_act(fs.act, hk0[fs.offset + 2]) + 1.0f) + hr_apply_act(fh.act, hk0[fh.offset + 2]);
    }
    else if (a.color_table) {                     // transform_color_one (tensorf_utils.py:308-320, point.py:588-594)
        // camera id = round(rays[..., -2]); ids outside the table are clamped (the reference would raise)
        int id = (int)rintf(a.rays[ray * cfg.ray_dim + cfg.ray_dim - 2]);
        id = min(max(id, 0), cfg.color_table_views - 1);
        const float* e = a.color_table + 12 * id;
        float t[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) t[i] = hr_apply_act(cfg.color_table_t_act, e[i]);
        const float n0 = c0 + ((c0 * t[0] + c1 * t[1]) + c2 * t[2]);
        const float n1 = c1 + ((c0 * t[3] + c1 * t[4]) + c2 * t[5]);
        const float n2 = c2 + ((c0 * t[6] + c1 * t[7]) + c2 * t[8]);
        c0 = n0 + hr_apply_act(cfg.color_table_s_act, e[9]);
        c1 = n1 + hr_apply_act(cfg.color_table_s_act, e[10]);
        c2 = n2 + hr_apply_act(cfg.color_table_s_act, e[11]);
    }
    a.rgb[ray * 3 + 0] = fminf(fmaxf(c0, 0.0f), 1.0f);   // eval-mode clamp, :246-247
    a.rgb[ray * 3 + 1] = fminf(fmaxf(c1, 0.0f), 1.0f);
    a.rgb[ray * 3 + 2] = fminf(fmaxf(c2, 0.0f), 1.0f);
}

// ---------------------------------------------------------------------------------------------------------
// The per-lane body, in two steps with a synchronisation of the ray's lanes between them (the caller's: a block
// barrier in the stand-alone kernel, program order in the fused kernel where a ray never leaves its wavefront).

struct HrRayLane {              // what a lane knows about its ray
    float ro[3], rd[3], vd[3];
    float t_ray;
    // hr_ray_constants: what every sample of the ray needs and none of them changes
    float oc[3];                // the contracted origin (hr_contract_point of ro)
    float base_t, time_off;     // advect: the ray's keyframe time and its distance to it
    float quad[3];              // sphere / cylinder with the model's constant centre-scale: o.o, d.d, o.d (hr_quadratic_ray_terms)
};
// In the lane-per-sample mapping a per-RAY quantity costs what a per-sample one does (an instruction is issued for the wavefront) -- ~70 of
// the stage's vector instructions per sample slot.  The stand-alone kernel therefore computes the record ONCE per ray, one lane per ray of
// the workgroup, and passes it through LDS (sample_kernel.hip); the frame kernel's sample wavefronts, which share no barrier, call
// hr_ray_constants per lane.  HR_RAY_RECORD floats: ro, rd, t_ray, oc, base_t, time_off, quad (vd = rd), padded to 4 x 16 bytes.
#define HR_RAY_RECORD 16

__device__ __forceinline__ HrRayLane hr_load_ray(const hr_config& cfg, const HrSampleArgs& a, int64_t ray, bool ray_ok)
{
    HrRayLane L;
    L.ro[0] = L.ro[1] = L.ro[2] = 0.f;
    L.rd[0] = L.rd[1] = 0.f; L.rd[2] = 1.f;
    L.vd[0] = L.vd[1] = 0.f; L.vd[2] = 1.f;
    L.t_ray = 0.0f;
    if (ray_ok) {
        const float* r = a.rays + ray * cfg.ray_dim;
        L.ro[0] = r[0] - cfg.isect_origin[0];        // base.py:143-149
        L.ro[1] = r[1] - cfg.isect_origin[1];
        L.ro[2] = r[2] - cfg.isect_origin[2];
        L.rd[0] = r[3]; L.rd[1] = r[4]; L.rd[2] = r[5];
        L.vd[0] = r[3]; L.vd[1] = r[4]; L.vd[2] = r[5];  // viewdirs, point.py:868-869
        L.t_ray = r[cfg.ray_dim - 1];                // rays[..., -1], point.py:783
    }
    return L;
}

__device__ __forceinline__ void hr_ray_constants(const hr_config& cfg, HrRayLane& L)
{
    L.oc[0] = L.oc[1] = L.oc[2] = 0.0f;
    if (cfg.contract_type != HR_CONTRACT_IDENTITY) hr_contract_point(cfg, L.ro[0], L.ro[1], L.ro[2], L.oc);
    L.base_t = 0.0f; L.time_off = 0.0f;
    if (cfg.advect) {
        L.base_t = hr_base_time(cfg, L.t_ray);
        L.time_off = L.t_ray - L.base_t;
    }
    L.quad[0] = L.quad[1] = L.quad[2] = 0.0f;
    if ((cfg.isect_type == HR_ISECT_SPHERE || cfg.isect_type == HR_ISECT_CYLINDER) && cfg.origin_scale == 0.0f)
        hr_quadratic_ray_terms(cfg, L.ro, L.rd, cfg.origin_initial[0], cfg.origin_initial[1], cfg.origin_initial[2], L.quad);
}

__device__ __forceinline__ void hr_store_ray_record(const HrRayLane& L, float* rec)
{
    hr_f4* r4 = reinterpret_cast<hr_f4*>(rec);
    r4[0] = hr_f4{L.ro[0], L.ro[1], L.ro[2], L.rd[0]};
    r4[1] = hr_f4{L.rd[1], L.rd[2], L.t_ray, L.oc[0]};
    r4[2] = hr_f4{L.oc[1], L.oc[2], L.base_t, L.time_off};
    r4[3] = hr_f4{L.quad[0], L.quad[1], L.quad[2], 0.0f};
}

__device__ __forceinline__ HrRayLane hr_read_ray_record(const float* rec)
{
    const hr_f4* r4 = reinterpret_cast<const hr_f4*>(rec);
    const hr_f4 a = r4[0], b = r4[1], c = r4[2], d = r4[3];
    HrRayLane L;
    L.ro[0] = a.x; L.ro[1] = a.y; L.ro[2] = a.z; L.rd[0] = a.w; L.rd[1] = b.x; L.rd[2] = b.y;
    L.vd[0] = a.w; L.vd[1] = b.x; L.vd[2] = b.y;
    L.t_ray = b.z;
    L.oc[0] = b.w; L.oc[1] = c.x; L.oc[2] = c.y; L.base_t = c.z; L.time_off = c.w;
    L.quad[0] = d.x; L.quad[1] = d.y; L.quad[2] = d.z;
    return L;
}

// decode matrix of this ray: M[c][ch] (RGB: basis_mat rows; SH: sum_j sh_j(d) * basis row c*9+j); the ray's ZP lanes
// fill it together (lane k: slots k, k + ZP, ...)
template <int ZP>
__device__ __forceinline__ void hr_fill_decode(const hr_config& cfg, const HrSampleArgs& a, const HrRayLane& L, int k, float* M)
{
    const int CA = a.ca_total;
    float sh[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bool is_sh = cfg.shading == HR_SHADING_SH;
    if (is_sh) hr_sh_deg2(L.vd[0], L.vd[1], L.vd[2], sh);
    for (int pos = k; pos < CA; pos += ZP) {              // (no integer division by the runtime CA)
        // padded slot -> column of basis_mat (the reference concatenates only real channels): a table made at finalize;
        // the values a slot folds are contiguous in the column-major copy of basis_mat
        const int col = a.slot_col[pos];
        float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
        if (col >= 0) {
            const float* b = a.basis_t + (size_t)col * a.basis_ld;
            if (is_sh) {
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    v0 = HR_FMA(sh[j], b[j], v0);
                    v1 = HR_FMA(sh[j], b[9 + j], v1);
                    v2 = HR_FMA(sh[j], b[18 + j], v2);
                }
            } else {
                v0 = b[0]; v1 = b[1]; v2 = b[2];
            }
        }
        M[pos] = v0; M[CA + pos] = v1; M[2 * CA + pos] = v2;
    }
}

// The RGBt modes' decode matrix (DESIGN 3m): M[c][ch] = sum_j basis_j(t, time_offset) * basis_mat[c nb + j][col(ch)] -- hr_fill_decode's
// SH form with the ray's time basis (hr_time_decode.h) in the place of sh_j(d).  The nb values a slot folds per colour are contiguous in the
// column-major copy of basis_mat; the basis is evaluated inside the fold (a lane fills at most ceil(CA / ZP) slots: no per-lane array).
template <int ZP>
__device__ __forceinline__ void hr_fill_decode_time(const HrSampleArgs& a, const HrTimeIO& io, float t, float time_off, int k, float* M)
{
    const int CA = a.ca_total;
    const int nb = hr_time_nb(io.c_fourier, io.fpk);
    for (int pos = k; pos < CA; pos += ZP) {
        const int col = a.slot_col[pos];
        float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
        if (col >= 0) {
            const float* b = a.basis_t + (size_t)col * a.basis_ld;
            v0 = hr_time_fold(io.c_fourier, io.fpk, t, time_off, io.fac, b, 1);
            v1 = hr_time_fold(io.c_fourier, io.fpk, t, time_off, io.fac, b + nb, 1);
            v2 = hr_time_fold(io.c_fourier, io.fpk, t, time_off, io.fac, b + 2 * nb, 1);
        }
        M[pos] = v0; M[CA + pos] = v1; M[2 * CA + pos] = v2;
    }
}

// The density modes' row of a ray: D[slot] = sum_j basis_j * basis_mat_density[j][col(slot)]; io.dslot_col maps the row's io.d_slots
// floats to columns (-1: a padded channel, or rows 1, 2 of the class gathers' matrix-shaped block -- zero)
template <int ZP>
__device__ __forceinline__ void hr_fill_density_row(const HrTimeIO& io, float t, float time_off, int k, float* D)
{
    for (int pos = k; pos < io.d_slots; pos += ZP) {
        const int col = io.dslot_col[pos];
        D[pos] = col >= 0 ? hr_time_fold(io.d_fourier, io.fpk, t, time_off, io.fac, io.dbasis_t + (size_t)col * io.d_ld, 1) : 0.0f;
    }
}

// Everything from the head values of sample k to the ray's colour.  PIPE: depth of the gather's load pipeline, NB: 2 = compiled for static nets only, 4 = static or keyframe, PC: plane class (hr_plane_class: 1 = [8, 4, 4], 2 = [8, 0, 0], 0 = generic).  `hrow`: this ray's head row(s) in LDS (row stride
// HS floats; RPR rows when the head comes from a point MLP); `M`: the ray's decode matrix in LDS; `ones`: hr_gather_ones_init's block; `s_x`: 256-float
// scratch of the block for rays that span several wavefronts (ZP > 64, stand-alone kernel only).
// MAPS (hr_sample_maps_kernel only): also the ray's weighted sums of distance and point and its sum of weights -- the reference's
// fields=['distances', 'points'] and acc_map (tensorf_no_sample.py:232, 254-278) -- into `*maps`, which no other instantiation reads.
// SHADE (sample_shade_kernel.hip only; MLP shading modes, DESIGN 3l): 1 = the export form -- `M` holds all 27 rows of basis_mat, the
// sample's 27 appearance features, its view direction and its live flag go to `shade->rows` (hr_plan.h: HR_SHADE_ROW floats per sorted
// sample) and nothing else is written; 2 = the import form -- the colour of a sample the export form found above the weight threshold
// (the row's live flag) is read from `shade->rgbk` (the shading kernel's output) instead of being decoded, everything after it is unchanged.
// TD (sample_time_kernel.hip only; the time-dependent decode modes, DESIGN 3m): bit 0 = the colour's activation is chosen among all
// shadings the time kernel serves (hr_time_color), bit 1 = a density mode -- `ones` is the ray's density row (class gathers: in the decode
// matrix's shape, generic gather: one weight per density slot, plane pair after plane pair) and weights the density channels.
template <int ZP, bool HALF, int PIPE, int NB, int PC, bool MAPS = false, int SHADE = 0, int TD = 0>
__device__ __forceinline__ void hr_sample_body(const hr_config& cfg, const HrSampleArgs& a, const HrRayLane& L, int64_t ray, bool ray_ok, int k,
                                               const float* hrow, int HS, const float* M, const float* ones, float* s_x,
                                               const hr_maps* maps = nullptr, const HrShadeIO* shade = nullptr)
{
    constexpr bool DEN = (TD & 2) != 0;
    const int tid = threadIdx.x;
    const int Z = cfg.z_channels;
    const int P = cfg.preds_per_z;
    const int CA = a.ca_total;
    const int RPR = a.rows_per_ray;
    constexpr int ZW = (ZP < 64) ? ZP : 64;        // lanes of a ray inside one wavefront
    constexpr int WPR = (ZP + 63) / 64;            // wavefronts per ray
    const bool lane_ok = ray_ok && (k < Z);
    const float* ro = L.ro;
    const float* rd = L.rd;

    // sample k's P head values: row k / M of the ray, columns (k % M) * P ..  (M == Z when RPR == 1)
    const int kk = lane_ok ? k : 0;
    const float* hk = hrow + kk * P;
    if (RPR != 1) {                                        // cascades only: integer division by a runtime value
        const int Mz = Z / RPR;
        hk = hrow + (kk / Mz) * HS + (kk % Mz) * P;
    }

    // ---- distances: intersect + mask, then sort along the ray (base.py:152-210)
    float dist = __builtin_inff();
    // verified fast path (a.redo_list, DESIGN 3i): which of this sample's comparisons are within the band of flipping
    // (always evaluated -- ~25 vector instructions per sample; a pointer that may be NULL at run time would put the struct into scratch memory)
    HrRisk risk_ = HR_RISK_INIT(a.redo_band, a.redo_band_q, a.redo_band_off, a.redo_amp_cut);
    HrRisk* const risk = &risk_;
    if (lane_ok) dist = hr_sample_distance(cfg, hk, k, ro, rd, risk, L.quad);
    HR_SPH(0);
    // verified fast path: the points' margin grows with the largest |d distance / d length| among the ray's live samples (the sort below
    // moves distances between lanes; the margin does not follow them)
    float band_p = 0.0f;
    if constexpr (ZP <= 64) {
        if (a.redo_list) {
            // the largest amp among the ray's live lanes, in every lane: rotations inside the row of 16 with the maximum taken IN the DPP instruction
            // (v_max_f32_dpp: one instruction per step; amp >= 0, no NaN: nothing to canonicalise), then across the rows
            float amp = (lane_ok && dist != 0.0f) ? risk_.amp : 0.0f;
#define HR_MAX_DPP(ctrl) asm("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 " ctrl " row_mask:0xf bank_mask:0xf" : "+v"(amp))
            if constexpr (ZW >= 2) HR_MAX_DPP("quad_perm:[1,0,3,2]");
            if constexpr (ZW >= 4) HR_MAX_DPP("quad_perm:[2,3,0,1]");
            if constexpr (ZW == 8) { float o = hr_lane_xor<4>(amp); asm("v_max_f32 %0, %0, %1" : "+v"(amp) : "v"(o)); }      // (two rays share a row: no rotation)
            if constexpr (ZW >= 16) { HR_MAX_DPP("row_ror:4"); HR_MAX_DPP("row_ror:8"); }
#undef HR_MAX_DPP
            if constexpr (ZW >= 32) { float o = hr_lane_xor<16>(amp); asm("v_max_f32 %0, %0, %1" : "+v"(amp) : "v"(o)); }
            if constexpr (ZW >= 64) { float o = hr_lane_xor<32>(amp); asm("v_max_f32 %0, %0, %1" : "+v"(amp) : "v"(o)); }
            band_p = a.redo_band_q * amp + a.redo_band_off;
        }
    }
    if (cfg.sort) dist = hr_sort_ray<ZP>(dist, k, s_x);
    HR_SPH(1);

    // ---- points, contraction, advect, offset
    const float* oc = L.oc;                        // (per-ray: hr_ray_constants)
    const float base_t = L.base_t, time_off = L.time_off;
    float p[3] = {0.f, 0.f, 0.f};
    float dist_c = 0.0f;
    if (lane_ok) hr_sample_point(cfg, hk, dist, ro, rd, oc, time_off, p, &dist_c);

    // deltas (tensorf_no_sample.py:137-144)
    float dist_next;
    if constexpr (ZP > 64) dist_next = hr_block_exchange(dist_c, min(tid + 1, 255), s_x);
    else dist_next = hr_dpp_f<0x130>(dist_c);                  // wave_shl:1 -- the next lane's value (the ray's last sample does not use it)
    const float delta = (k == Z - 1) ? 1e10f : (dist_next - dist_c);
    HR_SPH(2);

    // ---- feature gather
    bool valid = lane_ok && hr_sample_valid(cfg, p, dist_c, risk, band_p) && (a.rows_out == nullptr);
    if (a.occ && valid) valid = hr_occupancy_test(a, p);     // opt-in occupancy early-reject: empty space is neither gathered nor composited (sigma = 0)
    float sig_feat = 0.0f;
    float pre0 = 0.0f, pre1 = 0.0f, pre2 = 0.0f;
    if constexpr (SHADE == 1) {            // export form: the own-sample gather once per three rows of basis_mat, each triple stored at once
        HrAxisTaps at = {};
        if (valid) {
            at.ax[0] = hr_make_tap(hr_normalize_coord(cfg, p[0], 0), cfg.grid[0]);
            at.ax[1] = hr_make_tap(hr_normalize_coord(cfg, p[1], 1), cfg.grid[1]);
            at.ax[2] = hr_make_tap(hr_normalize_coord(cfg, p[2], 2), cfg.grid[2]);
            at.t = hr_make_tap(cfg.video ? hr_normalize_time(cfg, base_t) : 0.0f, cfg.video ? cfg.num_keyframes : 2);
        }
        float* row = shade->rows + (ray * Z + k) * HR_SHADE_ROW;
#pragma unroll 1
        for (int t3 = 0; t3 < HR_SHADE_FEAT / 3; ++t3) {
            float sg = 0.0f, f0 = 0.0f, f1 = 0.0f, f2 = 0.0f;
            if (valid) {
                const float* Mt = M + 3 * t3 * CA;
                hr_gather_plane<HALF, 1, 0>(a.planes[0], at, Mt, CA, sg, f0, f1, f2);
                hr_gather_plane<HALF, 1, 1>(a.planes[1], at, Mt, CA, sg, f0, f1, f2);
                hr_gather_plane<HALF, 1, 2>(a.planes[2], at, Mt, CA, sg, f0, f1, f2);
            }
            if (t3 == 0) sig_feat = sg;
            if (lane_ok) { row[3 * t3 + 0] = f0; row[3 * t3 + 1] = f1; row[3 * t3 + 2] = f2; }
        }
    } else if constexpr (PC != 0) {        // plane classes [8, 4, 4] / [8, 0, 0] (hr_gather_844 / hr_gather_844h)
        float pn[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (valid) {
            pn[0] = hr_normalize_coord(cfg, p[0], 0);
            pn[1] = hr_normalize_coord(cfg, p[1], 1);
            pn[2] = hr_normalize_coord(cfg, p[2], 2);
            pn[3] = cfg.video ? hr_normalize_time(cfg, base_t) : 0.0f;
        }
        HrAxisTapsC at;
        at.ax[0] = hr_make_tap_in(pn[0], cfg.grid[0]);      // valid => inside the aabb; masked => the centre
        at.ax[1] = hr_make_tap_in(pn[1], cfg.grid[1]);
        at.ax[2] = hr_make_tap_in(pn[2], cfg.grid[2]);
        at.t = hr_make_tap_c(pn[3], (NB == 4 && cfg.video) ? cfg.num_keyframes : 2);
        HR_SPH(3);
        if constexpr (HALF) hr_gather_844h<NB, PC, DEN>(a.planes, at, valid, M, ones, sig_feat, pre0, pre1, pre2);
        else hr_gather_844<NB, PC, DEN>(a.planes, at, valid, M, ones, sig_feat, pre0, pre1, pre2);
        HR_SPH(4);
    } else if constexpr (!HALF) {      // all lanes take part: the quad's lanes serve each other's samples
        float pn[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (valid) {
            pn[0] = hr_normalize_coord(cfg, p[0], 0);
            pn[1] = hr_normalize_coord(cfg, p[1], 1);
            pn[2] = hr_normalize_coord(cfg, p[2], 2);
            pn[3] = cfg.video ? hr_normalize_time(cfg, base_t) : 0.0f;
        }
        HrAxisTaps at;
        at.ax[0] = hr_make_tap(pn[0], cfg.grid[0]);
        at.ax[1] = hr_make_tap(pn[1], cfg.grid[1]);
        at.ax[2] = hr_make_tap(pn[2], cfg.grid[2]);
        at.t = hr_make_tap(pn[3], cfg.video ? cfg.num_keyframes : 2);
        HR_SPH(3);
        if constexpr (DEN) {               // density row: plane pair j's slots behind those of the pairs before it
            const float* D1 = ones + 4 * a.planes[0].cd4;
            hr_gather_plane_coop<0, PIPE, NB, true>(a.planes[0], at, valid, M, CA, sig_feat, pre0, pre1, pre2, ones);
            hr_gather_plane_coop<1, PIPE, NB, true>(a.planes[1], at, valid, M, CA, sig_feat, pre0, pre1, pre2, D1);
            hr_gather_plane_coop<2, PIPE, NB, true>(a.planes[2], at, valid, M, CA, sig_feat, pre0, pre1, pre2, D1 + 4 * a.planes[1].cd4);
        } else {
        hr_gather_plane_coop<0, PIPE, NB>(a.planes[0], at, valid, M, CA, sig_feat, pre0, pre1, pre2);
        HR_SPH(4);
        hr_gather_plane_coop<1, PIPE, NB>(a.planes[1], at, valid, M, CA, sig_feat, pre0, pre1, pre2);
        HR_SPH(5);
        hr_gather_plane_coop<2, PIPE, NB>(a.planes[2], at, valid, M, CA, sig_feat, pre0, pre1, pre2);
        HR_SPH(6);
        }
    } else if (valid) {
        float pn[4];
        pn[0] = hr_normalize_coord(cfg, p[0], 0);
        pn[1] = hr_normalize_coord(cfg, p[1], 1);
        pn[2] = hr_normalize_coord(cfg, p[2], 2);
        pn[3] = cfg.video ? hr_normalize_time(cfg, base_t) : 0.0f;
        HrAxisTaps at;
        at.ax[0] = hr_make_tap(pn[0], cfg.grid[0]);
        at.ax[1] = hr_make_tap(pn[1], cfg.grid[1]);
        at.ax[2] = hr_make_tap(pn[2], cfg.grid[2]);
        at.t = hr_make_tap(pn[3], cfg.video ? cfg.num_keyframes : 2);
        if constexpr (DEN) {
            const float* D1 = ones + 4 * a.planes[0].cd4;
            hr_gather_plane<HALF, 1, 0, true>(a.planes[0], at, M, CA, sig_feat, pre0, pre1, pre2, ones);
            hr_gather_plane<HALF, 1, 1, true>(a.planes[1], at, M, CA, sig_feat, pre0, pre1, pre2, D1);
            hr_gather_plane<HALF, 1, 2, true>(a.planes[2], at, M, CA, sig_feat, pre0, pre1, pre2, D1 + 4 * a.planes[1].cd4);
        } else {
        hr_gather_plane<HALF, 1, 0>(a.planes[0], at, M, CA, sig_feat, pre0, pre1, pre2);
        hr_gather_plane<HALF, 1, 1>(a.planes[1], at, M, CA, sig_feat, pre0, pre1, pre2);
        hr_gather_plane<HALF, 1, 2>(a.planes[2], at, M, CA, sig_feat, pre0, pre1, pre2);
        }
    }

    // ---- density -> alpha -> transmittance -> weight (raw2alpha, tensorf_utils.py:242-253)
    const float sigma = valid ? hr_density(cfg, sig_feat) : 0.0f;
    const float alpha = lane_ok ? (1.0f - HR_EXP(-sigma * (delta * cfg.distance_scale))) : 0.0f;
    float inc = lane_ok ? ((1.0f - alpha) + 1e-10f) : 1.0f;
    const int kw = k & (ZW - 1);                   // position inside this wavefront's part of the ray
    constexpr bool ROWS = (ZP == 16 || ZP == 32 || ZP == 64);  // a ray = one, two or four whole rows of 16 lanes: scans as DPP row operations
    if constexpr (ROWS) {
        inc = inc * hr_dpp_old<0x111>(1.0f, inc);  // inclusive product inside each row (row_shr:1, 2, 4, 8; no source -> 1)
        inc = inc * hr_dpp_old<0x112>(1.0f, inc);
        inc = inc * hr_dpp_old<0x114>(1.0f, inc);
        inc = inc * hr_dpp_old<0x118>(1.0f, inc);
        if constexpr (ZP >= 32) inc = inc * hr_dpp_old<0x142, 0xA>(1.0f, inc);    // odd rows: times the row before's product (row_bcast:15)
        if constexpr (ZP == 64) inc = inc * hr_dpp_old<0x143, 0xC>(1.0f, inc);    // upper half: times the lower half's product (row_bcast:31)
    } else {
#pragma unroll
        for (int d = 1; d < ZW; d <<= 1) {
            const float o = __shfl_up(inc, d, 64);
            if (kw >= d) inc = inc * o;
        }
    }
    float before = 1.0f;                           // product over the ray's earlier wavefronts
    if constexpr (ZP > 64) {
        __syncthreads();
        if ((tid & 63) == 63) s_x[tid >> 6] = inc;
        __syncthreads();
        const int w = tid >> 6, w0 = (w / WPR) * WPR;
        for (int i = w0; i < w; ++i) before = before * s_x[i];
        inc = inc * before;
    }
    float T = ROWS ? hr_dpp_old<0x138>(1.0f, inc) : __shfl_up(inc, 1, 64);       // wave_shr:1 -- the previous lane's value
    if (kw == 0) T = before;                       // == 1 for the ray's first sample
    const float weight = alpha * T;
    HR_SPH(7);
    if constexpr (SHADE == 1) {                    // export form: the rest of the sample's row, and nothing else
        if (lane_ok) {
            float* row = shade->rows + (ray * Z + k) * HR_SHADE_ROW;
            row[HR_SHADE_FEAT + 0] = L.vd[0]; row[HR_SHADE_FEAT + 1] = L.vd[1]; row[HR_SHADE_FEAT + 2] = L.vd[2];
            row[HR_SHADE_FEAT + 3] = hr_shade_live(weight, cfg.weight_thresh) ? 1.0f : 0.0f;
            row[HR_SHADE_FEAT + 4] = 0.0f;
        }
        return;
    }

    // ---- colour decode (+ per-sample scale/shift) and front-to-back sum
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    if (lane_ok) {
        float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
        if (cfg.weight_thresh > 0.0f) risk->hit = risk->hit || (fabsf(weight - cfg.weight_thresh) <= 1e-4f);
        if constexpr (SHADE == 2) {
            // import form: renderModule's colour (tensorf_no_sample.py:208-219) from the shading kernel.  The mask is the one the export form
            // took from ITS weight (the same arithmetic, the density summed in another order) and the shading kernel's tiles were chosen
            // by -- a colour is read exactly where one was computed
            if (shade->rows[(ray * Z + k) * HR_SHADE_ROW + HR_SHADE_FEAT + 3] != 0.0f) {
                const float* c = shade->rgbk + (ray * Z + k) * 3;
                r0 = c[0]; r1 = c[1]; r2 = c[2];
            }
        } else if (weight > cfg.weight_thresh) {   // app_mask, tensorf_no_sample.py:201
            if constexpr ((TD & 1) != 0) {         // the time kernel: SH and the RGBt modes relu(x + 0.5), RGBIdentity |x + 0.5| (hr_time_decode.h), RGB below
                if (cfg.shading != HR_SHADING_RGB) {
                    r0 = hr_time_color(cfg.shading, pre0); r1 = hr_time_color(cfg.shading, pre1); r2 = hr_time_color(cfg.shading, pre2);
                } else {
                    r0 = HR_RCP(1.0f + HR_EXP(-pre0)); r1 = HR_RCP(1.0f + HR_EXP(-pre1)); r2 = HR_RCP(1.0f + HR_EXP(-pre2));
                }
            } else
            if (cfg.shading == HR_SHADING_SH) {    // SHRender, tensorf_utils.py:334-338
                r0 = fmaxf(pre0 + 0.5f, 0.0f); r1 = fmaxf(pre1 + 0.5f, 0.0f); r2 = fmaxf(pre2 + 0.5f, 0.0f);
            } else {                               // RGBRender, tensorf_utils.py:341-343
                r0 = HR_RCP(1.0f + HR_EXP(-pre0)); r1 = HR_RCP(1.0f + HR_EXP(-pre1)); r2 = HR_RCP(1.0f + HR_EXP(-pre2));
            }
        }
        if (cfg.f_color_scale.offset >= 0) {       // scale_shift_color_all, tensorf_utils.py:267-273
            const hr_head_field& fs = cfg.f_color_scale;
            const hr_head_field& fh = cfg.f_color_shift;
            r0 = r0 * (hr_apply_act_post(fs.act, hk[fs.offset + 0]) + 1.0f) + hr_apply_act_post(fh.act, hk[fh.offset + 0]);
            r1 = r1 * (hr_apply_act_post(fs.act, hk[fs.offset + 1]) + 1.0f) + hr_apply_act_post(fh.act, hk[fh.offset + 1]);
            r2 = r2 * (hr_apply_act_post(fs.act, hk[fs.offset + 2]) + 1.0f) + hr_apply_act_post(fh.act, hk[fh.offset + 2]);
        }
        c0 = weight * r0; c1 = weight * r1; c2 = weight * r2;
    }
    float acc_w = lane_ok ? weight : 0.0f;
    if constexpr (ROWS) {                          // sums towards the ray's LAST lane: row_shr adds, then row_bcast:15 into the second row
#define HR_ROW_SUM(x) do { x += hr_dpp_f<0x111>(x); x += hr_dpp_f<0x112>(x); x += hr_dpp_f<0x114>(x); x += hr_dpp_f<0x118>(x); \
                           if (ZP >= 32) x += hr_dpp_old<0x142, 0xA>(0.0f, x); \
                           if (ZP == 64) x += hr_dpp_old<0x143, 0xC>(0.0f, x); } while (0)
        HR_ROW_SUM(c0); HR_ROW_SUM(c1); HR_ROW_SUM(c2); HR_ROW_SUM(acc_w);
#undef HR_ROW_SUM
    } else {
#pragma unroll
        for (int d = ZW >> 1; d > 0; d >>= 1) {
            c0 += __shfl_xor(c0, d, 64);
            c1 += __shfl_xor(c1, d, 64);
            c2 += __shfl_xor(c2, d, 64);
            acc_w += __shfl_xor(acc_w, d, 64);
        }
    }
    if constexpr (ZP > 64) {                       // add the ray's wavefronts in order
        __syncthreads();
        if ((tid & 63) == 0) {
            float* o = s_x + 4 * (tid >> 6);
            o[0] = c0; o[1] = c1; o[2] = c2; o[3] = acc_w;
        }
        __syncthreads();
        const int w0 = ((tid >> 6) / WPR) * WPR;
        c0 = s_x[4 * w0 + 0]; c1 = s_x[4 * w0 + 1]; c2 = s_x[4 * w0 + 2]; acc_w = s_x[4 * w0 + 3];
        for (int i = 1; i < WPR; ++i) {
            c0 += s_x[4 * (w0 + i) + 0]; c1 += s_x[4 * (w0 + i) + 1]; c2 += s_x[4 * (w0 + i) + 2]; acc_w += s_x[4 * (w0 + i) + 3];
        }
    }
    // the lane that holds the ray's sums writes the pixel: the last one after the row sums, the first one after a butterfly
    if (ray_ok && k == (ROWS ? ZP - 1 : 0) && a.rows_out == nullptr) hr_write_pixel(cfg, a, ray, hrow, c0, c1, c2, acc_w);
    if constexpr (MAPS) {                          // the maps: weight * distance, weight * point, summed as the colour is; acc_w is the sum of the weights
        float md = 0.0f, mp0 = 0.0f, mp1 = 0.0f, mp2 = 0.0f;
        if (lane_ok) { md = weight * dist_c; mp0 = weight * p[0]; mp1 = weight * p[1]; mp2 = weight * p[2]; }
        if constexpr (ROWS) {
#define HR_ROW_SUM(x) do { x += hr_dpp_f<0x111>(x); x += hr_dpp_f<0x112>(x); x += hr_dpp_f<0x114>(x); x += hr_dpp_f<0x118>(x); \
                           if (ZP >= 32) x += hr_dpp_old<0x142, 0xA>(0.0f, x); \
                           if (ZP == 64) x += hr_dpp_old<0x143, 0xC>(0.0f, x); } while (0)
            HR_ROW_SUM(md); HR_ROW_SUM(mp0); HR_ROW_SUM(mp1); HR_ROW_SUM(mp2);
#undef HR_ROW_SUM
        } else {
#pragma unroll
            for (int d = ZW >> 1; d > 0; d >>= 1) {
                md += __shfl_xor(md, d, 64);
                mp0 += __shfl_xor(mp0, d, 64);
                mp1 += __shfl_xor(mp1, d, 64);
                mp2 += __shfl_xor(mp2, d, 64);
            }
        }
        if constexpr (ZP > 64) {                   // the ray's wavefronts in order, through s_x[16 ..] (the colour's 4 x 4 floats stay untouched)
            float* q = s_x + 16;
            if ((tid & 63) == 0) {
                float* o = q + 4 * (tid >> 6);
                o[0] = md; o[1] = mp0; o[2] = mp1; o[3] = mp2;
            }
            __syncthreads();
            const int w0 = ((tid >> 6) / WPR) * WPR;
            md = q[4 * w0 + 0]; mp0 = q[4 * w0 + 1]; mp1 = q[4 * w0 + 2]; mp2 = q[4 * w0 + 3];
            for (int i = 1; i < WPR; ++i) {
                md += q[4 * (w0 + i) + 0]; mp0 += q[4 * (w0 + i) + 1]; mp1 += q[4 * (w0 + i) + 2]; mp2 += q[4 * (w0 + i) + 3];
            }
        }
        if (ray_ok && k == (ROWS ? ZP - 1 : 0) && a.rows_out == nullptr) {
            if (maps->distances_dev) maps->distances_dev[ray] = md;
            if (maps->acc_dev) maps->acc_dev[ray] = acc_w;
            if (maps->points_dev) {
                maps->points_dev[ray * 3 + 0] = mp0;
                maps->points_dev[ray * 3 + 1] = mp1;
                maps->points_dev[ray * 3 + 2] = mp2;
            }
        }
    }
    if constexpr (ZP <= 64) {
        if (a.redo_list) {                         // one list entry per ray with a sample at risk, written by the lane that wrote the pixel
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(risk_.hit && lane_ok);
            const int first = (tid & 63) & ~(ZW - 1);
            const unsigned long long mine = (bal >> first) & ((ZW == 64) ? ~0ull : ((1ull << ZW) - 1ull));
            if (mine != 0ull && ray_ok && k == (ROWS ? ZP - 1 : 0)) {
                const unsigned pos = atomicAdd(a.redo_count, 1u);
                if (pos < (unsigned)a.redo_cap) a.redo_list[pos] = (int)(a.ray0 + ray);
                else if (a.flags) atomicOr(a.flags, 4u);          // more rays than the list holds: HR_OPT_REDO_OVERFLOW
            }
        }
    }

    HR_SPH(8);
    // ---- coarse pass of a cascade: emit the point MLP's input row of this (sorted) sample (point.py:142-157)
    if (a.rows_out && lane_ok) {
        float* row = a.rows_out + (ray * Z + k) * a.row_dim;
        const float* r = a.rays + ray * cfg.ray_dim;
        int c = 0;
        for (int i = 0; i < a.n_row_inputs; ++i) {
            const int kind = a.row_kind[i];
            for (int j = 0; j < a.row_len[i]; ++j)
                row[c++] = (kind == HR_PIN_POINTS) ? (j == 0 ? p[0] : j == 1 ? p[1] : p[2])
                           : (kind == HR_PIN_VIEWDIRS) ? r[3 + j] : (kind == HR_PIN_ORIGINS) ? r[j] : r[cfg.ray_dim - 1];
        }
    }

    // ---- optional diagnostics
    if (lane_ok) {
        const int64_t s = ray * Z + k;
        if (a.fields.distances_dev) a.fields.distances_dev[s] = dist_c;
        if (a.fields.points_dev) {
            a.fields.points_dev[s * 3 + 0] = p[0];
            a.fields.points_dev[s * 3 + 1] = p[1];
            a.fields.points_dev[s * 3 + 2] = p[2];
        }
        if (a.fields.sigma_dev) a.fields.sigma_dev[s] = sigma;
        if (a.fields.weights_dev) a.fields.weights_dev[s] = weight;
    }
}
