// Host-side decisions shared by hr_model_finalize, the render launchers and the training launcher: plane-pair geometry, plane class,
// the training step's launch plan.  Plain C++ (no HIP types); the CPU suite compiles it as it is (tests/host_math/hr_plan_host.cpp).
#ifndef HR_PLAN_H
#define HR_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/hyperreel_hip.h"
#include "hr_grid.h"

// z_channels rounded up to a power of two, at least 8: the sample count the per-ray kernels are compiled for (8 ... 256)
static inline int hr_round_zp(int z_channels)
{
    int zp = 8;
    while (zp < z_channels) zp <<= 1;
    return zp;
}

// f(std::integral_constant<int, ZP>()) for the compiled sample counts (more than 256 samples are rejected by hr_model_create)
template <class F>
static inline void hr_with_zp(int zp, F&& f)
{
    switch (zp) {
        case 8: f(std::integral_constant<int, 8>()); break;
        case 16: f(std::integral_constant<int, 16>()); break;
        case 32: f(std::integral_constant<int, 32>()); break;
        case 64: f(std::integral_constant<int, 64>()); break;
        case 128: f(std::integral_constant<int, 128>()); break;
        case 256: f(std::integral_constant<int, 256>()); break;
        default: break;
    }
}

// The three plane pairs of a configuration: everything of HrGridPlane but the texel pointers (cleared).  Plane j spans the axes
// MAT_MODE[j] = (0, 1), (0, 2), (1, 2) (tensorf_base.py:231); its line runs along VEC_MODE[j] = 2 - j, a keyframe net's time plane
// along MAT_MODE_TIME[j][0] = 2 - j, one row per keyframe (tensorf_dynamic.py:48).  A pair without channels keeps tex == 0.
// Returns false when the sampled pairs' appearance channels do not add up to basis_mat's columns (a keyframe net with appearance
// but no density components on a pair: the reference itself fails on it with a shape error).
static inline bool hr_plane_geometry(const hr_config& c, HrGridPlane out[3], int* ca_total, int* n_basis_cols)
{
    int app_off = 0, real_off = 0, n_app_sum = 0;
    for (int j = 0; j < 3; ++j) {
        HrGridPlane& g = out[j];
        g = HrGridPlane();
        const int nd = c.n_den[j];
        // tensorf_dynamic.py:310-311,355-356: a pair whose DENSITY plane has no components is skipped for appearance too
        const int na = (c.video && nd == 0) ? 0 : c.n_app[j];
        g.cd4 = (nd + 3) / 4;
        g.ca4 = (na + 3) / 4;
        g.ax = (j == 2) ? 1 : 0;
        g.ay = (j == 0) ? 1 : 2;
        g.bx = 2 - j;
        g.aw = c.grid[g.ax];
        g.ah = c.grid[g.ay];
        g.bw = c.video ? c.grid[g.bx] : 1;
        g.bh = c.video ? c.num_keyframes : c.grid[g.bx];
        g.app_off = app_off;
        g.app_real = na;
        g.app_real_off = real_off;
        app_off += 4 * g.ca4;
        real_off += na;
        n_app_sum += c.n_app[j];
        g.tex = 4 * (g.cd4 + g.ca4);
        if (c.grid_dtype == HR_GRID_FP16) g.tex = (g.tex + 7) & ~7;      // whole 16-byte loads of 8 halfs
    }
    *ca_total = app_off;
    *n_basis_cols = n_app_sum;
    return real_off == n_app_sum;
}

// What a class-specialised kernel needs of a plane pair besides the decomposition.  The render gathers clamp their taps to (i, i + 1):
static inline bool hr_plane_fits_gather(const HrGridPlane& p) { return p.aw >= 2 && p.ah >= 2 && p.bh >= 2 && (p.bw == 1 || p.bw >= 2); }
// the training step's class path (hr_bwd_slot) addresses texel elements by 32-bit offsets
static inline bool hr_plane_fits_train(const HrGridPlane& p)
{
    return (int64_t)p.aw * p.ah * p.tex < (1ll << 30) && (int64_t)p.bw * p.bh * p.tex < (1ll << 30);
}

// 1: [8, 4, 4] (all three plane pairs), 2: [8, 0, 0] (plane pair 0 only: the technicolor models), 0: anything else.  float16 texels
// have the same group structure (hr_gather_844h).
template <class Fits>
static inline int hr_plane_class(const HrGridPlane* pl, int ca_total, Fits fits)
{
    auto ok = [&](int j, int cd4, int off) {
        return pl[j].cd4 == cd4 && pl[j].ca4 == cd4 && pl[j].tex == 8 * cd4 && pl[j].app_off == off && fits(pl[j]);
    };
    if (!ok(0, 2, 0)) return 0;
    if (ok(1, 1, 8) && ok(2, 1, 12) && ca_total == 16) return 1;
    if (pl[1].cd4 + pl[1].ca4 == 0 && pl[2].cd4 + pl[2].ca4 == 0 && ca_total == 8) return 2;
    return 0;
}

// ---------------------------------------------------------------- the training step (train_kernel.hip)
// Phase A walks a ray serially and is bound by the latency of that walk (every sample's gather waits on its point), not by
// issue slots: a batch of 16 384 rays in full wavefronts is ONE wavefront per CU with nothing to hide the latency behind.
// HR_TRAIN_RPW rays per wavefront (the other lanes idle) gives every SIMD several wavefronts instead.
#ifndef HR_TRAIN_RPW
#define HR_TRAIN_RPW 16
#endif
// Phase B.  HR_TRAIN_LPS = 16 adjacent lanes per sample, one texel channel each (a plane pair has 8 or 16 channels per
// texel in every shipped model), so that the atomics of one tap are one contiguous run; a workgroup of the global-atomics kernel is
// 16 such groups and walks the samples of RPB whole rays (1 ray when it has 16 samples or more).
#define HR_TRAIN_LPS 16
// rays per trip of the lines kernel: four samples per 16-lane group between the barriers (the per-trip staging of the decode
// matrices, its barriers and the fold into basis_mat's gradient are then a quarter; measured 1 / 2 / 4 / 8 samples: DoNeRF
// sample-stage backward 0.84 / 0.80 / 0.78 / 0.77 ms, immersive 1.46 / 1.32 / 1.24 / 1.21, neural_3d 2.56 / 2.32 / 2.19 / 2.14 --
// profiles/r03_c_train_experiments.txt)
#ifndef HR_TRAIN_TRIP_MULT
#define HR_TRAIN_TRIP_MULT 4
#endif
#define HR_TRAIN_LINES_RPB(ZP) (HR_TRAIN_TRIP_MULT * (((1024 / HR_TRAIN_LPS) + (ZP) - 1) / (ZP)))
#define HR_TRAIN_LINES_LDS_CAP ((size_t)150 * 1024)      // dynamic LDS the lines kernel may ask for (a workgroup has 160 KiB)

struct HrTrainPlanIn {
    int64_t n_rays;
    bool backward;              // a d_rgb was given: phases B and C run
    bool taps, dp, perm;        // the tape has room for the axis taps / the point gradient / the grouped ray order
    bool deterministic;         // the fixed-point build: global atomics for everything
    size_t acc_bytes;           // sizeof(hr_acc_t)
    int cus;                    // compute units of the device: only grid sizes depend on it
};

// Everything hr_launch_train decides.  The atomics part is always filled in: the launcher falls back to it when the runtime refuses
// the lines kernel's LDS request (hr_lds_opt_in).
struct HrTrainPlan {
    int zp;
    // phase A: hr_train_kernel<zp> above 64 samples (HR_TRAIN_RPW rays per wavefront; leaves no taps on the tape), else
    // hr_train_lanes_kernel<zp, a_nb, a_pc> (256 / zp rays per workgroup)
    int thread_per_ray, rays_per_group;
    int a_pc, a_nb;             // hr_plane_class of the render gathers; NB = 2: compiled for static nets only
    unsigned a_blocks;
    size_t a_lds;
    int backward, taps;         // taps: phase A leaves them, phase B reads them and the point-backward tail runs
    // phase B, hr_train_gather_bwd_lines_kernel<zp, keyed, b_pc>: the contended part of the gradient in LDS
    int lines, keyed;           // keyed: two rows of each time plane (rays grouped by keyframe interval, hr_train_bucket_kernel), else whole lines
    int b_pc;                   // the class path of hr_bwd_class_sample, 0 without taps
    int passes;                 // 1: every pair; 2: pair 0, then pairs 1 + 2 adding to tape.dp; 0 without `lines`
    unsigned pass_pairs[2];
    int pass_add_dp[2];
    size_t pass_lds[2];
    size_t lines_lds;           // the largest request considered, whether or not it fits the cap (the opt-in asks for it)
    unsigned lines_blocks;
    size_t bucket_lds;
    // phase B, hr_train_gather_bwd_kernel<zp>: global atomics
    int atomics_rpb;
    unsigned atomics_blocks;
    size_t atomics_lds;
    unsigned tail_blocks;       // one thread per sample: hr_train_point_bwd_kernel (with taps), hr_train_dist_bwd_kernel
};

static inline HrTrainPlan hr_train_plan(const hr_config& cfg, const HrGridPlane* planes, int ca_total, int n_basis_cols, const HrTrainPlanIn& in)
{
    HrTrainPlan P = HrTrainPlan();
    const int64_t n = in.n_rays;
    const int zp = P.zp = hr_round_zp(cfg.z_channels);
    auto ceil_div = [](int64_t a, int64_t b) { return (a + b - 1) / b; };
    auto at_most = [](int64_t a, int64_t b) { return (unsigned)(a < b ? a : b); };

    // ---- phase A: a lane per sample where a ray fits one wavefront
    P.thread_per_ray = zp > 64;
    P.rays_per_group = P.thread_per_ray ? HR_TRAIN_RPW : 256 / zp;
    P.a_pc = hr_plane_class(planes, ca_total, hr_plane_fits_gather);
    P.a_nb = (P.a_pc == 1 && !cfg.video) ? 2 : 4;
    P.a_blocks = (unsigned)ceil_div(n, P.rays_per_group);
    P.a_lds = P.thread_per_ray ? 0 : sizeof(float) * P.rays_per_group * 3 * ca_total;      // the rays' decode matrices
    P.backward = in.backward;
    P.taps = in.taps && !P.thread_per_ray;
    const bool dp = in.dp && !P.thread_per_ray;

    // ---- phase B, global atomics
    const int groups = 256 / HR_TRAIN_LPS;
    P.atomics_rpb = zp >= groups ? 1 : groups / zp;
    // four 256-thread workgroups per CU are resident (128 registers); four rounds of them: the blocks differ in cost
    P.atomics_blocks = at_most(ceil_div(n, P.atomics_rpb), 16 * (int64_t)in.cus);
    P.atomics_lds = sizeof(float) * (P.atomics_rpb * 3 * ca_total) + in.acc_bytes * (P.atomics_rpb * 3 * ca_total + 27 * n_basis_cols);

    // ---- phase B, windows in LDS
    bool any = false, keyed = false;
    for (int j = 0; j < 3; ++j)
        if (planes[j].cd4 + planes[j].ca4 > 0) { any = true; keyed = keyed || planes[j].bw != 1; }
    P.keyed = keyed;
    P.b_pc = (P.taps && dp && n * cfg.z_channels < (1ll << 30)) ? hr_plane_class(planes, ca_total, hr_plane_fits_train) : 0;
    const int rpb = HR_TRAIN_LINES_RPB(zp);
    P.lines_blocks = at_most(ceil_div(n, rpb), in.cus);
    P.bucket_lds = sizeof(int) * (size_t)(cfg.num_keyframes + 1);
    // decode matrices and their gradient, basis_mat's gradient, the rays' time taps; then the windows of plane pairs `pairs`
    const size_t base = sizeof(float) * (2 * rpb * 3 * ca_total + 27 * n_basis_cols + 4 * rpb);
    auto request = [&](unsigned pairs) {
        size_t bytes = base;
        for (int j = 0; j < 3; ++j) {
            const HrGridPlane& g = planes[j];
            if (g.cd4 + g.ca4 == 0 || !((pairs >> j) & 1u)) continue;
            bytes += sizeof(float) * (size_t)(keyed ? 2 * g.bw : g.bh) * g.tex;
        }
        return bytes;
    };
    P.lines_lds = request(7u);
    unsigned pairs[2] = {7u, 0u};
    bool fits = !in.deterministic && any;
    if (fits && keyed) {
        // keyframe net: needs the taps on the tape (two passes re-read them) and the grouped order; all pairs in one pass if
        // their rows fit, else pair 0 (the wide one) and pairs 1 + 2
        fits = P.taps && dp && in.perm && n <= 0x7fffffff && cfg.video && cfg.num_keyframes >= 2 && cfg.num_keyframes <= 8192;
        if (fits && P.lines_lds > HR_TRAIN_LINES_LDS_CAP) {
            pairs[0] = 1u;
            pairs[1] = 6u;
            const size_t l0 = request(1u), l1 = request(6u);
            P.lines_lds = l0 > l1 ? l0 : l1;
        }
    }
    if (fits && P.lines_lds <= HR_TRAIN_LINES_LDS_CAP) {
        P.lines = 1;
        for (int p = 0; p < 2 && pairs[p]; ++p) {
            P.pass_pairs[p] = pairs[p];
            P.pass_add_dp[p] = p;
            P.pass_lds[p] = request(pairs[p]);
            P.passes = p + 1;
        }
    }
    P.tail_blocks = (unsigned)ceil_div(n * cfg.z_channels, 256);
    return P;
}

#endif  // HR_PLAN_H
