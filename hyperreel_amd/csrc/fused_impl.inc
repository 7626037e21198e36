// The frame kernel: K1 (sample-prediction MLP) and K2+K3 (intersect .. composite) in ONE persistent launch in which the
// raw head -- the (B, Z*P) tensor the reference materialises between RayPredictionEmbedding and Intersect
// (nlf/embedding/ray.py:332-337 -> nlf/intersect/base.py:142-259) -- never leaves the CU's LDS.
//
// CDNA4 mapping
//   * one workgroup per CU, resident for the whole launch, walking its share of the 64-ray tiles; the workgroup's
//     wavefronts are specialised:
//       wavefronts 0-3   "MLP":    the six layers of the tile on the matrix cores (mlp_split_core.inc), one per SIMD;
//       wavefronts 4-..  "sample": NS wavefronts running the per-sample stage (sample_core.inc) of the PREVIOUS tile
//                                  on the vector ALU / texture path of the same SIMDs.
//     The matrix pipe and the VALU of a SIMD issue from different wavefronts concurrently (MI355X_MICROARCH.md, wave
//     scheduling): the MLP wavefronts run at priority 2-3, the sample wavefronts take the issue slots they leave.
//   * LDS (<= 160 KiB):   Xh | Xl   hidden activations of the MLP tile, split halves      2 x 64 x 264 x 2 B = 67.6 KB
//                         H         the tile's head, [64 rays][HS floats], fp32            DoNeRF: 64 x 356 x 4 = 91.1 KB
//                         (Xih|Xil  the MLP's input tile, overlaid on the first rows of H -- see below)
//                         M         decode matrices of the rays in flight                  NS x RPW x 3 x CA x 4 B
//                         sync      four counters
//     The MLP wavefronts write the last Linear's 32x32 accumulator tiles straight into H (16-byte LDS stores, row stride
//     HS = 4 mod 8 words: conflict free); a sample lane (ray, k) reads its P values at H[ray][k*P ..].
//   * hand-over protocol, all counters monotonic in LDS, polled by whole wavefronts (s_sleep between polls):
//       bar      arrivals of the 4 MLP wavefronts (their private barrier: s_barrier would also stop the sample waves)
//       ready    tiles whose head is complete in H                         MLP -> sample
//       first    sample wavefronts that finished the FIRST ray group of a tile   sample -> MLP
//       done     sample wavefronts that finished a tile                          sample -> MLP
//     H is single-buffered: the MLP wavefronts run layers 0..L-2 of tile i+1 while the sample wavefronts consume tile
//     i, and wait for `done` only before the first store of the last Linear.  The MLP's input tile (10 KB) is overlaid
//     on the rows of H that the sample wavefronts read FIRST (wavefront w starts with ray group w), and is written only
//     after `first` says those rows have been consumed; it is dead again before the last Linear overwrites it.
//   * tiles are dealt XCD-aware: workgroup b runs on XCD b % 8, and each XCD gets one contiguous eighth of the ray list
//     (neighbouring rays share texels in that XCD's L2).
//
// Applies when the head tile fits (hr_frame_plan, hr_plan.h); everything else takes the two-kernel path.
#ifndef HR_MFMA_PRIO_HI
#define HR_MFMA_PRIO_HI 3
#define HR_MFMA_PRIO_LO 2
#endif
#include "mlp_split_core.inc"
#include "sample_core.inc"

struct HrFusedArgs {
    HrMlpArgs m;
    HrSampleArgs s;
    int n_tiles;            // tiles (32 x MT rays) of the launch
    int HS;                 // floats per head row in LDS
    int m_copies;           // decode matrices per sample wavefront in LDS: 1 (RGB shading: basis_mat itself) or rays per pass (SH: per ray)
};

__device__ __forceinline__ unsigned hr_lds_peek(const unsigned* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// wait until the counter has reached `target` (wrap-safe), then acquire
__device__ __forceinline__ void hr_wait_ge(const unsigned* p, unsigned target)
{
    while ((int)(hr_lds_peek(p) - target) < 0) __builtin_amdgcn_s_sleep(2);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// one arrival of this wavefront on a counter, after everything it has issued so far has completed
__device__ __forceinline__ void hr_arrive(unsigned* p)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <int NW>
struct HrSyncGroup {                       // the NW MLP wavefronts of the workgroup
    unsigned* bar;
    unsigned target;                       // arrivals after which the next barrier opens (per-wavefront copy)
    const unsigned* first;                 // what the input-tile store waits for: `first` (one head buffer) or `done` (two)
    unsigned need_first;
    __device__ __forceinline__ void barrier()
    {
        target += NW;
        hr_arrive(bar);
        hr_wait_ge(bar, target);
    }
    // the input tile overlays head rows the sample wavefronts read first: wait until they have
    __device__ __forceinline__ void before_input_store() { hr_wait_ge(first, need_first); }
    __device__ __forceinline__ bool any(bool pred) { return pred; }        // (the frame kernel keeps no ray lists: every wavefront speaks for itself)
};

template <int NW, bool HOLD_>
struct HrSinkLds {
    float* H;
    int HS;
    const unsigned* done;
    unsigned need_done;
    unsigned* ready;
    HrSyncGroup<NW>* sync;
    static constexpr bool HOLD = HOLD_;    // true: every output tile of a wavefront is accumulated before begin() (mlp_split_core.inc)
    static constexpr bool TAPS = false;
    __device__ __forceinline__ void begin() { hr_wait_ge(done, need_done); }   // the previous tile's head has been consumed
    __device__ __forceinline__ void store(int r, int64_t, int n0, const float4 v) { *reinterpret_cast<float4*>(H + r * HS + n0) = v; }
    __device__ __forceinline__ void end()
    {
        sync->barrier();                   // every MLP wavefront's stores are in H (and its reads of Xh/Xl are over)
        if (threadIdx.x == 0) __hip_atomic_fetch_add(ready, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};

// ZP: lanes per ray (8/16/32/64).  HALF: float16 texels.  NS: sample wavefronts (4: two wavefronts per SIMD and 256
// VGPRs each; 8: three per SIMD, 168 VGPRs, the MLP's weight ring one slot shorter).
// MT: 32-ray m-tiles per tile.  2 (64 rays): heads of up to 364 columns -- the static nets.  1 (32 rays): the keyframe families'
//     480-column heads (TensorVMKeyframeTime, nlf/nets/tensorf_dynamic.py:645-839; 960 columns at 64 samples per ray): half the
//     rays per pass over the weights, and room for TWO head buffers.
// NB: 2 = static nets (plane x line), 4 = static or keyframe (plane x time plane).
// NBUF: head buffers.  2: the MLP wavefronts write tile i + 1 while the sample wavefronts read tile i -- no hand-over stall on
//     either side, the MLP's input tile is overlaid on the buffer it is about to fill.  1: the single-buffer protocol above.
template <int ZP, bool HALF, int NS, int PC, int MT, int NB, int NBUF>
__global__ __launch_bounds__(64 * (4 + NS)) void HR_FUSED_KERNEL(const hr_config* __restrict__ cfgp, const HrFusedArgs fa)
{
    const hr_config& cfg = *cfgp;
    constexpr int W = 256, NW = 4, TM = 32 * MT, XS = W + 8;
    constexpr int RING = (NS > 4 && MT == 2) ? 3 : 4;
    static_assert(NBUF == 1 || NBUF == 2, "one or two head buffers");
    // (Measured and not kept: twelve sample wavefronts at 128 registers -- three per SIMD -- with the ray groups of all tiles handed
    //  out through an LDS ticket: technicolor 2.22 vs 2.16 ms, immersive 2.52 vs 2.45, DoNeRF on 32-ray tiles 2.20 vs 1.93 on
    //  64-ray tiles; with 32-ray tiles the MLP wavefronts, streaming every weight once per 32 rays, are what the tile waits for.)
    constexpr int RPW = 64 / ZP;                 // rays per sample wavefront and pass (one "ray group")
    constexpr int GPT = TM / RPW;                // ray groups per tile
    constexpr int GPW = GPT / NS;                // ray groups per sample wavefront and tile
    static_assert(ZP <= 64 && GPT % NS == 0, "a ray stays inside one wavefront; groups divide evenly");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int CA = fa.s.ca_total;
    const int HS = fa.HS;
    HR_SPLIT_E* Xh = reinterpret_cast<HR_SPLIT_E*>(lds_raw);        // [TM][W+8] hidden activations, hi
    HR_SPLIT_E* Xl = Xh + TM * XS;                               //            lo
    float* H0 = reinterpret_cast<float*>(Xl + TM * XS);          // [NBUF][TM][HS] head tile(s); the MLP's input tile [TM][k0p+8] x (hi, lo) is
                                                                 //   overlaid on the first rows of the buffer of the tile being computed
    float* s_M = H0 + NBUF * TM * HS;                            // [NS][m_copies][3][CA]
    unsigned* sy = reinterpret_cast<unsigned*>(s_M + NS * fa.m_copies * 3 * CA);   // bar, ready, first, done
    float* s_ones = reinterpret_cast<float*>(sy + 8);            // [HR_GATHER_ONES] the class-specialised gather's constant block (sample_core.inc)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < 8) sy[tid] = 0u;
    hr_gather_ones_init(s_ones);
    __syncthreads();                             // the only block-wide barrier of the kernel

    // ---- this workgroup's tiles: XCD x = b % 8 owns the contiguous part [nt*x/X, nt*(x+1)/X) and deals it round-robin
    //      to its workgroups (b / 8)
    const int nwg = (int)gridDim.x, b = (int)blockIdx.x;
    const int X = nwg < 8 ? nwg : 8;
    const int xcd = b & 7, idx = b >> 3;
    const int wx = (nwg - xcd + 7) >> 3;         // workgroups on this XCD
    const int t_lo = (int)(((int64_t)fa.n_tiles * xcd) / X), t_hi = (int)(((int64_t)fa.n_tiles * (xcd + 1)) / X);

    if (wave < NW) {
        // =============================================================== MLP wavefronts
        __builtin_amdgcn_s_setprio(HR_MFMA_PRIO_LO);
        HrSyncGroup<NW> sync{&sy[0], 0u, (NBUF == 2) ? &sy[3] : &sy[2], 0u};
        HrSinkLds<NW, MT == 2> sink{H0, HS, &sy[3], 0u, &sy[1], &sync};
        HrMlpTrace trace{nullptr, 0};
        unsigned it = 0;
        for (int tile = t_lo + idx; tile < t_hi; tile += wx, ++it) {
            float* H = H0 + (it & (NBUF - 1)) * (TM * HS);
            HR_SPLIT_E* Xih = reinterpret_cast<HR_SPLIT_E*>(H);
            HR_SPLIT_E* Xil = Xih + TM * (fa.m.k0p + 8);
            sink.H = H;
            if constexpr (NBUF == 2) {             // this tile's buffer was last read by tile it-2
                sync.need_first = it >= 2 ? (unsigned)NS * (it - 1) : 0u;
                sink.need_done = sync.need_first;
            } else {
                sync.need_first = (unsigned)NS * it;      // tile it-1: every sample wavefront is past its first group
                sink.need_done = (unsigned)NS * it;       // tile it-1: consumed
            }
            hr_mlp_tile<W, MT, NW, RING>(cfg, fa.m, (int64_t)tile * TM, fa.m.n_rays, Xih, Xil, Xh, Xl, sync, sink, trace);
        }
    } else {
        // =============================================================== sample wavefronts
        const int sw = wave - NW;
        const int rig = lane / ZP;               // ray of the group this lane works on
        const int k = lane % ZP;
        // RGB shading: the decode matrix is basis_mat itself, the same for every ray -- each sample wavefront fills its copy
        // once, before the first tile (SH: per ray, folded with the ray's view direction)
        const bool per_ray_M = (cfg.shading == HR_SHADING_SH);
        float* M = s_M + (sw * fa.m_copies + (per_ray_M ? rig : 0)) * 3 * CA;
        if (!per_ray_M) {
            if (rig == 0) hr_fill_decode<ZP>(cfg, fa.s, hr_load_ray(cfg, fa.s, 0, false), k, M);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        unsigned it = 0;
        for (int tile = t_lo + idx; tile < t_hi; tile += wx, ++it) {
            hr_wait_ge(&sy[1], it + 1u);         // the tile's head is in H
            // ray groups sw, sw + NS, ... of the tile
#pragma unroll 1
            for (int j = 0; j < GPW; ++j) {
                const int g = sw + NS * j;
                const int row = g * RPW + rig;
                const int64_t ray = (int64_t)tile * TM + row;
                const bool ray_ok = ray < fa.s.n_rays;
                HrRayLane L = hr_load_ray(cfg, fa.s, ray, ray_ok);
                hr_ray_constants(cfg, L);
                if (per_ray_M) {
                    hr_fill_decode<ZP>(cfg, fa.s, L, k, M);
                    // the ray's lanes share M; they are one wavefront, whose LDS operations execute in order
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
                HR_SPH(10);
                const float* H = H0 + (it & (NBUF - 1)) * (TM * HS);
                hr_sample_body<ZP, HALF, (NS > 4) ? 1 : 2, NB, PC>(cfg, fa.s, L, ray, ray_ok, k, H + row * HS, HS, M, s_ones, nullptr);
                if (NBUF == 1 && g < NS) hr_arrive(&sy[2]);   // rows under the MLP's next input tile are free
                else if (per_ray_M) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // M is rewritten by the next group
            }
            hr_arrive(&sy[3]);
        }
    }
}

// ---------------------------------------------------------------- launcher
template <int ZP, bool HALF, int NS, int PC, int MT, int NB, int NBUF>
static bool hr_launch_fused_t(const hr_config& cfg, const HrFusedArgs& fa, size_t lds, int grid, hipStream_t stream)
{
    static HrLdsOptIn opt;
    if (!hr_lds_opt_in(opt, reinterpret_cast<const void*>(&HR_FUSED_KERNEL<ZP, HALF, NS, PC, MT, NB, NBUF>), lds)) return false;
    hipLaunchKernelGGL((HR_FUSED_KERNEL<ZP, HALF, NS, PC, MT, NB, NBUF>), dim3(grid), dim3(64 * (4 + NS)), lds, stream, fa.s.cfg_dev, fa);
    return true;
}

// Launches the instantiation plan P (hr_frame_plan, hr_plan.h: it fits, and there are rays) names; false: the runtime refused its LDS
bool HR_FUSED_LAUNCH(const hr_config& cfg, const HrMlpArgs& ma, const HrSampleArgs& sa, const HrFramePlan& P, hipStream_t stream)
{
    static_assert(sizeof(HR_SPLIT_E) == sizeof(uint16_t), "launch_frame sizes the plan's tiles for 16-bit split elements");
    const bool half = (cfg.grid_dtype == HR_GRID_FP16);
    HrFusedArgs fa;
    fa.m = ma;
    fa.s = sa;
    fa.HS = P.head_stride, fa.m_copies = P.m_copies, fa.n_tiles = P.n_tiles;
    if (P.tile_rays == 64) {
#define HR_FUSED_CASE(Z_, H_, N_) return hr_launch_fused_t<Z_, H_, N_, 1, 2, 2, 1>(cfg, fa, P.lds, P.grid, stream)
#define HR_FUSED_TEX(Z_, N_) do { if (half) HR_FUSED_CASE(Z_, true, N_); else HR_FUSED_CASE(Z_, false, N_); } while (0)
        if (P.zp == 32) {
            if (P.ns == 4) HR_FUSED_TEX(32, 4); else HR_FUSED_TEX(32, 8);
        } else {
            if (P.ns == 4) HR_FUSED_TEX(16, 4); else HR_FUSED_TEX(16, 8);
        }
#undef HR_FUSED_TEX
#undef HR_FUSED_CASE
    }
#define HR_FUSED_CASE(Z_, H_, P_, B_) return hr_launch_fused_t<Z_, H_, 8, P_, 1, 4, B_>(cfg, fa, P.lds, P.grid, stream)
#define HR_FUSED_TEX(Z_, B_) do { if (half) { if (P.pclass == 1) HR_FUSED_CASE(Z_, true, 1, B_); else HR_FUSED_CASE(Z_, true, 2, B_); } \
                                  else { if (P.pclass == 1) HR_FUSED_CASE(Z_, false, 1, B_); else HR_FUSED_CASE(Z_, false, 2, B_); } } while (0)
    if (P.zp == 32) HR_FUSED_TEX(32, 2); else HR_FUSED_TEX(64, 1);
#undef HR_FUSED_TEX
#undef HR_FUSED_CASE
    return false;
}
