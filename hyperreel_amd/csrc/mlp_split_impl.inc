// K1 (split-precision form), stand-alone kernel: one 32*MT-ray tile per workgroup, the raw head goes to the HBM
// workspace in the HQ layout (hr_kernels.h).  The tile arithmetic itself is mlp_split_core.inc, shared with the fused
// frame kernel (fused_impl.inc).  This file is the body of three translation units: mlp_bf16x3_kernel.hip (bf16
// halves: the fp32-range fallback), mlp_f16x3_kernel.hip (fp16 halves), mlp_f16x2_kernel.hip (fp16, weights unsplit) and
// mlp_f16f8_kernel.hip (fp16 leading product + fp8 corrections: what HR_MLP_AUTO resolves to, verified -- DESIGN 3c).
#include "mlp_split_core.inc"

struct HrSyncBlock {                       // the whole block is the MLP group
    __device__ __forceinline__ void barrier() { __syncthreads(); }
    __device__ __forceinline__ bool any(bool pred) { return __syncthreads_or(pred ? 1 : 0) != 0; }     // a barrier that ORs a predicate over the group
    __device__ __forceinline__ void before_input_store() {}
};

struct HrSinkWorkspace {                   // HQ layout: the 32 lanes of a half-wave write 512 contiguous bytes.  (Plain stores
    float* head;                           // on purpose: non-temporal ones shave 4 % off this kernel but evict the head from the
    int nq;                                // caches the sample kernel then reads it through: 2.90 vs 2.73 ms per frame end to end.)
    int64_t n_rays;
    static constexpr bool HOLD = false;    // tiles are stored as they are produced
    static constexpr bool TAPS = false;    // no per-layer activation output
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void store(int, int64_t row, int n0, const float4 v)
    {
        if (row < n_rays) *reinterpret_cast<float4*>(head + hr_head_index(row, n0, nq)) = v;
    }
    __device__ __forceinline__ void end() {}
};

// W: hidden width (256).  MT: 32-ray m-tiles per workgroup (2 -> 64 rays, 4 -> 128).  NW: waves
// per workgroup (4 or 8); a wave owns NT = 8 / NW tiles of 32 hidden features.
template <int W, int MT, int NW>
__global__ __launch_bounds__(64 * NW, (MT == 2) ? 2 : 1) void HR_SPLIT_KERNEL(const hr_config cfg, const HrMlpArgs a)
{
    constexpr int TM = 32 * MT;           // rays per workgroup
    constexpr int XS = W + 8;             // bf16 elements per activation row
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int XSI = a.k0p + 8;
    HR_SPLIT_E* Xih = reinterpret_cast<HR_SPLIT_E*>(lds_raw);       // [TM][k0p+8] MLP input, hi
    HR_SPLIT_E* Xil = Xih + TM * XSI;                            //              lo
    HR_SPLIT_E* Xh = Xil + TM * XSI;                             // [TM][W+8] hidden activations, hi
    HR_SPLIT_E* Xl = Xh + TM * XS;                               //            lo
    // optional per-wave phase timeline (hr_debug_trace_mlp): s_memtime stamps, 64 slots per wave
    HrMlpTrace trace;
    trace.tr = a.trace ? a.trace + ((size_t)blockIdx.x * NW + (threadIdx.x >> 6)) * 64 : nullptr;
    trace.tri = 0;
    if (trace.tr && (threadIdx.x & 63) == 0) trace.tr[0] = __builtin_readcyclecounter();    // 0: start
    trace.tri = 1;
    HrSyncBlock sync;
    // second pass of the verified fast path: the launch is sized for the list's capacity, *n_rays_dev rays are there (block-uniform exit,
    // before any barrier)
    int64_t n_rays = a.n_rays;
    if (a.n_rays_dev) {
        const unsigned nd_raw = *a.n_rays_dev;
        if (a.n_rays_copy && blockIdx.x == 0 && threadIdx.x == 0) *a.n_rays_copy = nd_raw;
        const int64_t nd = (int64_t)nd_raw > a.list_off ? (int64_t)nd_raw - a.list_off : 0;
        n_rays = nd < n_rays ? nd : n_rays;
    }
    if ((int64_t)blockIdx.x * TM >= n_rays) return;
    HrSinkWorkspace sink{a.head, a.nq, n_rays};
    hr_mlp_tile<W, MT, NW, 4>(cfg, a, (int64_t)blockIdx.x * TM, n_rays, Xih, Xil, Xh, Xl, sync, sink, trace);
}

template <int W, int MT, int NW>
static void hr_launch_mlp_split_t(const hr_config& cfg, const HrMlpArgs& args, hipStream_t stream)
{
    constexpr int TM = 32 * MT;
    const size_t lds = (size_t)TM * 2 * ((args.k0p + 8) + (W + 8)) * sizeof(HR_SPLIT_E);
    const unsigned blocks = (unsigned)((args.n_rays + TM - 1) / TM);
    static HrLdsOptIn opt;
    (void)hr_lds_opt_in(opt, reinterpret_cast<const void*>(&HR_SPLIT_KERNEL<W, MT, NW>), lds);
    hipLaunchKernelGGL((HR_SPLIT_KERNEL<W, MT, NW>), dim3(blocks), dim3(64 * NW), lds, stream, cfg, args);
}

#ifdef HR_SPLIT_TRAIN_KERNEL
// The same kernel as the FORWARD of a training step (INRSystem.training_step, nlf/__init__.py:658-690 -> BaseMLP.forward,
// nlf/nets/mlp.py:159-172): one launch for the six layers instead of six GEMM launches through HBM.  Besides the head it writes what
// the backward needs -- the output of every hidden Linear after its LeakyReLU, fp32, row-major, into the caller's buffers (the
// input of the next layer's weight gradient, and the sign mask of this layer's).
struct HrSinkTrain {
    float* head;
    int nq;
    int64_t n_rays;
    HrMlpTaps taps;
    static constexpr bool HOLD = false;
    static constexpr bool TAPS = true;
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void store(int, int64_t row, int n0, const float4 v)
    {
        if (row < n_rays) *reinterpret_cast<float4*>(head + hr_head_index(row, n0, nq)) = v;
    }
    __device__ __forceinline__ void end() {}
    __device__ __forceinline__ void tap(int l, int64_t row, int f0, const float (&v)[8])       // v[0..3]: features f0 .., v[4..7]: f0 + 8 ..
    {
        if (row >= n_rays || !taps.act[l]) return;
        float* p = taps.act[l] + row * taps.ld[l] + taps.off[l] + f0;
        if (((taps.ld[l] | taps.off[l]) & 3) == 0) {              // 16-byte aligned quads (the host pads a skip layer's row: train.py, HipMLP)
            *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
            *reinterpret_cast<float4*>(p + 8) = make_float4(v[4], v[5], v[6], v[7]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) { p[i] = v[i]; p[8 + i] = v[4 + i]; }
        }
    }
};

template <int W, int MT, int NW>
__global__ __launch_bounds__(64 * NW, NW / 2) void HR_SPLIT_TRAIN_KERNEL(const hr_config cfg, const HrMlpArgs a, const HrMlpTaps taps)
{
    constexpr int TM = 32 * MT;
    constexpr int XS = W + 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int XSI = a.k0p + 8;
    HR_SPLIT_E* Xih = reinterpret_cast<HR_SPLIT_E*>(lds_raw);
    HR_SPLIT_E* Xil = Xih + TM * XSI;
    HR_SPLIT_E* Xh = Xil + TM * XSI;
    HR_SPLIT_E* Xl = Xh + TM * XS;
    HrMlpTrace trace{nullptr, 0};
    HrSyncBlock sync;
    HrSinkTrain sink{a.head, a.nq, a.n_rays, taps};
    hr_mlp_tile<W, MT, NW, 4>(cfg, a, (int64_t)blockIdx.x * TM, a.n_rays, Xih, Xil, Xh, Xl, sync, sink, trace);
}

void HR_SPLIT_TRAIN_LAUNCH(const hr_config& cfg, const HrMlpArgs& args, const HrMlpTaps& taps, hipStream_t stream)
{
    if (args.n_rays <= 0 || cfg.mlp_hidden != 256) return;
    constexpr int TM = 64;
    const size_t lds = (size_t)TM * 2 * ((args.k0p + 8) + (256 + 8)) * sizeof(HR_SPLIT_E);
    const unsigned blocks = (unsigned)((args.n_rays + TM - 1) / TM);
    static HrLdsOptIn opt;
    (void)hr_lds_opt_in(opt, reinterpret_cast<const void*>(&HR_SPLIT_TRAIN_KERNEL<256, 2, 4>), lds);
    hipLaunchKernelGGL((HR_SPLIT_TRAIN_KERNEL<256, 2, 4>), dim3(blocks), dim3(256), lds, stream, cfg, args, taps);
}
#endif

void HR_SPLIT_LAUNCH(const hr_config& cfg, const HrMlpArgs& args, hipStream_t stream)
{
    if (args.n_rays <= 0) return;
    // 64 rays per workgroup, 4 wavefronts: two workgroups per CU hide each other's epilogues (1.50 ms per 640k rays;
    // 128 rays / one workgroup per CU: half the L1 weight traffic but nothing to overlap with, 1.83 ms; 8 wavefronts
    // per workgroup: no gain).  Other hidden widths are rejected by hr_model_create.
#ifdef HR_SPLIT_LIST_NW8
    // the verified fast path's second pass: a handful of tiles, each alone on its CU -- what counts is the latency of ONE tile through the six
    // layers.  Eight wavefronts (32 hidden features each) halve every wavefront's share; same arithmetic, same bits (a whole frame this way is
    // level with four wavefronts: 1.943 vs 1.946 ms, profiles/r05_k1_nw8_ab.txt)
    if (cfg.mlp_hidden == 256 && args.ray_index) { hr_launch_mlp_split_t<256, 2, 8>(cfg, args, stream); return; }
#endif
    if (cfg.mlp_hidden == 256) hr_launch_mlp_split_t<256, 2, 4>(cfg, args, stream);
}
