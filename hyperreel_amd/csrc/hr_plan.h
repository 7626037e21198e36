// Host-side decisions shared by hr_model_create / finalize, the render launchers and the training launcher: plane-pair geometry, plane
// class, the render call's launch plans (live head columns, launch sizing, the sample stage in every form, the frame kernel, the route, a frame's time tap),
// the training step's launch plan, the MLP's arithmetic (which one, whether verified, the margins' rules).  Plain C++ (no HIP types, no
// hr_model, no getenv); the CPU suite compiles it as it is (tests/host_math/hr_plan_host.cpp).
#ifndef HR_PLAN_H
#define HR_PLAN_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/hyperreel_hip.h"
#include "hr_grid.h"
#include "hr_math.h"
#include "hr_time_decode.h"

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

// ---------------------------------------------------------------- rendering (api_model.hip, api_render.hip, sample_kernel.inc, fused_impl.inc)
// Which of the P per-sample head columns does the path read?  Columns that are not read are dropped from the last Linear (fewer
// MFMAs, smaller head).  Shipped cases: the three sphere / cylinder origin channels when origin_scale_factor == 0
// (primitive.py:410-412 multiplies them by zero) and `point_sigma` in models whose point_offset stage reads `sigma` instead.
// col[i]: user column i -> live column (-1: dropped; prune off keeps every column below preds_per_z); *kcfg: the configuration the
// kernels see, preds_per_z = *p_live and the fields' offsets remapped.
static inline void hr_live_columns(const hr_config& c, bool prune, int col[64], int* p_live, hr_config* kcfg)
{
    bool live[64] = {};
    auto mark = [&](const hr_head_field& f, int first, int count) {
        if (f.offset < 0) return;
        for (int i = first; i < first + count && f.offset + i < 64; ++i) live[f.offset + i] = true;
    };
    int z_anchor = 0;                 // a z_vals channel that is always read
    if (c.isect_type == HR_ISECT_SPHERE || c.isect_type == HR_ISECT_CYLINDER) {
        z_anchor = 3;
        mark(c.f_z_vals, 3, 1);
        if (c.origin_scale != 0.0f) mark(c.f_z_vals, 0, 3);
    } else if (c.isect_type == HR_ISECT_DEFORMABLE_VOXEL_GRID) {
        z_anchor = 3;
        mark(c.f_z_vals, 3, 1);
        if (c.dvg_normal_scale != 0.0f) mark(c.f_z_vals, 0, 3);
    } else if (c.isect_type == HR_ISECT_SPHERE_NEW || c.isect_type == HR_ISECT_CYLINDER_NEW) {
        z_anchor = 7;
        mark(c.f_z_vals, 6, 2);
        // kept contiguous up to the anchor so that offset + channel stays valid after compaction
        if (c.resize_scale != 0.0f || c.origin_scale != 0.0f) mark(c.f_z_vals, 3, 3);
        if (c.origin_scale != 0.0f) mark(c.f_z_vals, 0, 3);
    } else {
        mark(c.f_z_vals, 0, 1);
    }
    mark(c.f_isect_sigma, 0, 1);
    if (c.point_offset) {
        mark(c.f_point_offset, 0, 3);
        mark(c.f_offset_sigma, 0, 1);
    }
    mark(c.f_color_scale, 0, 3);
    mark(c.f_color_shift, 0, 3);
    mark(c.f_color_scale_global, 0, c.f_color_scale_global.channels == 9 ? 9 : 3);    // 9: the head is a 3x3 `color_transform_global`
    mark(c.f_color_shift_global, 0, 3);
    if (c.advect && c.use_spatial_flow) mark(c.f_spatial_flow, 0, 3);
    int n = 0;
    for (int i = 0; i < 64; ++i) {
        const bool keep = (i < c.preds_per_z) && (live[i] || !prune);
        col[i] = keep ? n++ : -1;
    }
    *p_live = n;
    *kcfg = c;
    kcfg->preds_per_z = n;
    auto remap = [&](hr_head_field& f, int anchor) {   // anchor: a channel of the field that is always live
        if (f.offset < 0) return;
        f.offset = col[f.offset + anchor] - anchor;
    };
    remap(kcfg->f_z_vals, z_anchor);   // may become negative: only the live channels are read then
    remap(kcfg->f_isect_sigma, 0);
    if (c.point_offset) { remap(kcfg->f_point_offset, 0); remap(kcfg->f_offset_sigma, 0); }
    else { kcfg->f_point_offset.offset = -1; kcfg->f_offset_sigma.offset = -1; }
    remap(kcfg->f_color_scale, 0);
    remap(kcfg->f_color_shift, 0);
    remap(kcfg->f_color_scale_global, 0);
    remap(kcfg->f_color_shift_global, 0);
    if (c.advect && c.use_spatial_flow) remap(kcfg->f_spatial_flow, 0); else kcfg->f_spatial_flow.offset = -1;
}

// samples whose head values one MLP row produces: all Z of a ray, or Z / casc_in_z per coarse point
static inline int samples_per_row(const hr_config& c) { return c.casc_in_z > 0 ? c.z_channels / c.casc_in_z : c.z_channels; }
static inline int rows_per_ray(const hr_config& c) { return c.casc_in_z > 0 ? c.casc_in_z : 1; }
// float4 quads of one head row with p_live live columns per sample
static inline int hr_head_quads(const hr_config& c, int p_live) { return (samples_per_row(c) * p_live + 3) / 4; }

// ---- launch sizing
// Rays per launch when the caller reserves nothing.  131072 rays per launch measured best among 16k..640k (DoNeRF: a 185 MB head).  The head of a chunk
// should still be in the 256 MB Infinity Cache when the sample kernel reads it: wide heads (Neural-3D: 64 samples x 15 columns = 3840 bytes per ray) get
// fewer rays per launch -- measured on the 800x800 frames (profiles/r04_z_chunk_sweep.txt): neural_3d 4.44 ms at 131 072 rays (503 MB), 4.18 at 65 536
// (252 MB), 4.24 at 49 152; the 1920-byte heads (technicolor, immersive: 252 MB at 131 072) are best there.  (The cap, 163 840 = 231 MB of DoNeRF head: the
// largest that still sits in the cache next to the grids' hot lines -- and with hr_even_chunk an 800x800 frame is 4 launches of 160 000 rays instead of
// 4 x 131 072 + 115 712: 1.717 vs 1.729 ms, profiles/r06_chunk_sweep.txt; 213 376: 1.824)
static inline int64_t hr_default_chunk(int64_t nq, int rows_per_ray)
{
    int64_t rays = (256ll << 20) / (nq * 16 * rows_per_ray);
    if (rays >= 16384) rays &= ~(int64_t)16383;
    return rays > 163840 ? 163840 : (rays < 4096 ? 4096 : rays);
}

// rays per launch of a call of n rays: as many launches as the workspace of `chunk` rays demands, of equal size (a short last launch
// leaves the chip half empty for a whole kernel)
static inline int64_t hr_even_chunk(int64_t chunk, int64_t n)
{
    if (n <= chunk) return chunk;
    const int64_t k = (n + chunk - 1) / chunk;
    const int64_t per = (((n + k - 1) / k) + 63) & ~(int64_t)63;
    return per < chunk ? per : chunk;
}

// Verified fast path: entries of the ray list one hr_render call of n rays may fill: a sixteenth of its rays, at least 32 768 (never
// more than the rays there are, or the buffer's buffer_cap).  The second pass's launches are sized for it -- ~1.7 ns per workgroup that
// finds nothing to do -- and the calibration gives the fast path up above a twentieth (HR_VERIFY_LISTED_LIMIT)
static inline int hr_redo_list_cap(int64_t n, int buffer_cap)
{
    int64_t cap = n / 16 > 32768 ? n / 16 : 32768;
    cap = (cap + 63) & ~(int64_t)63;
    if (cap > n) cap = (n + 63) & ~(int64_t)63;
    return (int)(cap < buffer_cap ? cap : buffer_cap);
}

// ... and of its third pass's list: 128 tiles (rays outside the calibrated range are the exception)
static inline int hr_wide_cap(int64_t chunk) { return (int)(chunk < 8192 ? chunk : 8192); }

// ---- the stand-alone sample kernel (sample_kernel.inc)
// dynamic LDS of a workgroup: 256 / ZP rays x head rows x (a row's floats + 4), the rays' decode matrices, and above 64 samples (a ray
// spans several wavefronts) 256 floats of cross-wave scratch
static inline size_t hr_sample_lds_bytes(int nq, int ca_total, int ZP, int rows_per_ray)
{
    const int RPB = 256 / ZP;
    return ((size_t)RPB * rows_per_ray * (nq * 4 + 4) + (size_t)RPB * 3 * ca_total + (ZP > 64 ? 256 : 0)) * sizeof(float);
}

#define HR_LDS_PER_WORKGROUP ((size_t)160 * 1024)
// The kind of a model's sample stage: its kernels (hr_sample_form_plan, below); the frame kernel and verification are DECODE's alone (hr_render_route, hr_mlp_choice)
enum HrSampleKind {
    HR_SAMPLE_DECODE = 0,        // RGB / SH through basis_mat: hr_sample_kernel, hr_sample_maps_kernel
    HR_SAMPLE_SHADE,             // MLP_Fea / MLP: export form, colour network, import form
    HR_SAMPLE_TIME,              // RGBtLinear / RGBtFourier / RGBIdentity with the plain density: hr_sample_time_kernel, TD 1
    HR_SAMPLE_TIME_DENSITY       // a density mode under any shading hr_model_set_time_decode admits it with: TD 3
};
static inline bool hr_shading_is_mlp(int shading) { return shading == HR_SHADING_MLP_FEA || shading == HR_SHADING_MLP; }
static inline HrSampleKind hr_sample_kind(int shading, bool time_density)      // time_density: a density mode of hr_model_set_time_decode (no part of hr_config)
{
    return time_density ? HR_SAMPLE_TIME_DENSITY : hr_shading_is_time_family(shading) ? HR_SAMPLE_TIME : hr_shading_is_mlp(shading) ? HR_SAMPLE_SHADE : HR_SAMPLE_DECODE;
}

// What hr_launch_samples chooses for a launch: samples per ray rounded up (ZP), plane class, line form, grid and LDS
struct HrSamplePlan {
    int zp, pclass, all_lines, big_lds;
    unsigned blocks;
    size_t lds;
};

// planes: as the kernel gets them (inside hr_render_frame a keyframe net's time planes are lines); rows_emitted: the coarse level of a
// cascade, whose kernel writes the point MLP's input rows
static inline HrSamplePlan hr_sample_plan(const hr_config& cfg, const HrGridPlane* planes, int ca_total, int nq, int rows_per_ray, int64_t n_rays,
                                          bool rows_emitted)
{
    HrSamplePlan P = HrSamplePlan();
    const int ZP = P.zp = hr_round_zp(cfg.z_channels);
    const int RPB = 256 / ZP;
    P.blocks = (unsigned)((n_rays + RPB - 1) / RPB);
    P.lds = hr_sample_lds_bytes(nq, ca_total, ZP, rows_per_ray);
    // few samples x many head columns can exceed the 64 KiB a kernel gets by default (e.g. 32 rays x 8 x 64 floats)
    P.big_lds = P.lds > 64 * 1024;
    // the shipped [8, 4, 4] / [8, 0, 0] decompositions get the class-specialised gather of their texel format (sample_core.inc); ZP >= 8
    // keeps a quad inside one ray, video nets additionally need two keyframes
    P.pclass = (!rows_emitted && (!cfg.video || cfg.num_keyframes >= 2)) ? hr_plane_class(planes, ca_total, hr_plane_fits_gather) : 0;
    // every second factor a line (static nets; a keyframe net inside hr_render_frame): the gather compiled for two line taps
    P.all_lines = P.pclass != 0;
    for (int j = 0; j < 3; ++j)
        if (planes[j].cd4 + planes[j].ca4 > 0 && planes[j].bw != 1) P.all_lines = 0;
    return P;
}

// f(ZP, HALF, PC, NB) as integral constants: the instantiation KERNEL<ZP, HALF, PC, NB> of plan P.  Per ZP and texel format the
// compiled set is (PC, NB) in {(0, 4), (1, 2), (1, 4), (2, 2), (2, 4)}: the generic gather has no line form.
template <class F>
static inline void hr_sample_dispatch(const HrSamplePlan& P, bool half, F&& f)
{
    auto cls = [&](auto zp, auto h, auto pc) {
        if constexpr (decltype(pc)::value != 0)
            if (P.all_lines) return f(zp, h, pc, std::integral_constant<int, 2>());
        f(zp, h, pc, std::integral_constant<int, 4>());
    };
    auto tex = [&](auto zp, auto h) {
        if (P.pclass == 1) cls(zp, h, std::integral_constant<int, 1>());
        else if (P.pclass == 2) cls(zp, h, std::integral_constant<int, 2>());
        else cls(zp, h, std::integral_constant<int, 0>());
    };
    hr_with_zp(P.zp, [&](auto zp) { if (half) tex(zp, std::true_type()); else tex(zp, std::false_type()); });
}

// ---- hr_render_frame: the time tap every ray of a frame shares, as hr_sample_body computes it from a ray's last column (hr_math.h)
struct HrTimeTap { int i0, i1; float w0, w1; };      // clamped keyframe rows; their weights, zero for a row that does not exist
static inline HrTimeTap hr_frame_time_tap(const hr_config& c, float time)
{
    const float base_t = c.advect ? hr_base_time(c, time) : 0.0f;
    const hr_axis_tap t = hr_make_tap(hr_normalize_time(c, base_t), c.num_keyframes);
    return HrTimeTap{t.i0, t.i1, t.w0, t.w1};
}

// ---- the frame kernel (fused_impl.inc)
#define HR_GATHER_ONES (2 * 16 + 8)      // floats of the class-specialised gather's constant block in the caller's LDS (sample_core.inc)

struct HrFramePlanIn {
    int64_t n_rays;
    int frame_mode;             // HR_OPT_FRAME_KERNEL: 0 = never, 1 = where it fits and is expected to be the faster plan, 2 = wherever it fits
    int sample_waves;           // HR_OPT_SAMPLE_WAVES: 0 (the plan's choice), 4 or 8
    bool cascade;               // a level of a point_prediction cascade (several head rows per ray, or rows emitted)
    bool verified;              // the verified fast path is on: a two-pass plan over the HBM workspace
    bool split_mlp;             // the active arithmetic is a split one (the exact-fp32 MLP, v_mfma_f32_16x16x4_f32, keeps its own kernel)
    size_t split_elem;          // bytes of a split element (HR_SPLIT_E)
    int nq, k0p, last_tiles;    // float4 quads of a head row; mlp_in padded to a multiple of 16; 32-column output tiles of the last Linear
    int cus;                    // compute units of the device: only the grid depends on it
};

// Everything HR_FUSED_LAUNCH needs to pick and launch HR_FUSED_KERNEL<zp, HALF, ns, pclass, tile_rays / 32, nb, nbuf>
struct HrFramePlan {
    int fits;                   // 0: the call takes the two-kernel path
    int zp, pclass;
    int tile_rays;              // 64: the static nets whose head fits next to the activations; 32: wider heads, the video gather
    int ns, nb, nbuf;           // sample wavefronts, taps of a second factor (2: lines), head buffers
    int m_copies;               // decode matrices per sample wavefront in LDS
    int head_stride;            // floats per head row in LDS
    int n_tiles, grid;
    size_t lds;
};

// planes: as the kernel gets them (see hr_sample_plan)
static inline HrFramePlan hr_frame_plan(const hr_config& cfg, const HrGridPlane* planes, int ca_total, const HrFramePlanIn& in)
{
    HrFramePlan P = HrFramePlan();
    const int ZP = P.zp = hr_round_zp(cfg.z_channels), L = cfg.mlp_layers;
    if (!in.frame_mode || in.cascade || in.verified || !in.split_mlp || in.n_rays > ((int64_t)1 << 36)) return P;
    // (0 layers: ZeroMLP; a skip connection into the last Linear: the input tile is gone by then)
    if (cfg.mlp_hidden != 256 || L < 2 || ((cfg.mlp_skip_mask >> (L - 1)) & 1)) return P;
    // the shipped decompositions [8, 4, 4] / [8, 0, 0], in either texel format: the class-specialised gathers (others: two-kernel path)
    if ((P.pclass = hr_plane_class(planes, ca_total, hr_plane_fits_gather)) == 0) return P;
    P.head_stride = in.nq * 4;
    while ((P.head_stride & 7) != 4) P.head_stride += 4;    // 16-byte row stride = 4 mod 8 words: the 8 lanes of a ds_write_b128 group hit 8 bank quads
    const bool per_ray_M = (cfg.shading == HR_SHADING_SH);      // RGB shading keeps ONE decode matrix per sample wavefront (basis_mat itself)
    const int RPW = 64 / (ZP < 64 ? ZP : 64);                   // rays per sample wavefront and pass
    auto fit = [&](int tile_rays, int nbuf, int ns, int nb, int overlay_rows) {
        const size_t lds = (size_t)tile_rays * 2 * (256 + 8) * in.split_elem + (size_t)nbuf * tile_rays * P.head_stride * sizeof(float) +
                           (size_t)ns * (per_ray_M ? RPW : 1) * 3 * ca_total * sizeof(float) + 32 + HR_GATHER_ONES * sizeof(float);
        // the MLP's input tile is overlaid on head rows: it must stay inside the rows that are free when it is written
        const size_t xin = (size_t)tile_rays * 2 * (in.k0p + 8) * in.split_elem;
        if (lds > HR_LDS_PER_WORKGROUP || xin > (size_t)overlay_rows * P.head_stride * sizeof(float)) return false;
        P.fits = 1, P.tile_rays = tile_rays, P.ns = ns, P.nb = nb, P.nbuf = nbuf, P.lds = lds, P.m_copies = per_ray_M ? RPW : 1;
        P.n_tiles = (int)((in.n_rays + tile_rays - 1) / tile_rays);
        P.grid = P.n_tiles < in.cus ? P.n_tiles : in.cus;
        return true;
    };
    // ---- 64-ray tiles, one head buffer: the static nets whose head fits next to the activations (a wavefront holds at most three
    //      output tiles of the last Linear).  The overlay sits under the first ray groups' rows.
    // Eight sample wavefronts by default (1.97 vs 2.75 ms per DoNeRF frame with four, profiles/r05_frame_waves_ab.txt).  For part of round 5 the
    // default was four: with eight, repeated launches of the SAME frame differed in one ray of ~1e5 now and then -- traced to packed-fp32
    // instructions the compiler formed in the sample role, and removed by building without them (hyperreel_amd/build.py).
    const int NS = (in.sample_waves == 4) ? 4 : 8;
    if (!cfg.video && P.pclass == 1 && (ZP == 16 || ZP == 32) && in.last_tiles <= 12 && fit(64, 1, NS, 2, NS * RPW)) return P;
    // ---- 32-ray tiles: wider heads (the keyframe families' 480 / 960 columns) and the video gather.  32 samples per ray: two head
    //      buffers (the overlay has the whole buffer about to be filled); 64 samples per ray: one (the 123 KB tile leaves no room).
    //      Every weight then crosses the CU once per 32 rays instead of once per 64, and the two-kernel plan is as fast or faster
    //      (800x800 frames: technicolor 2.16 vs 2.06 ms, immersive 2.45 vs 2.46, neural_3d 4.92 vs 4.39): this plan is what
    //      frame_mode 2 asks for -- no head workspace traffic -- not the default
    if (in.frame_mode < 2 || (ZP != 32 && ZP != 64)) return P;
    (void)fit(32, ZP == 32 ? 2 : 1, 8, 4, ZP == 32 ? 32 : 8 * RPW);
    return P;
}

// ---- which plan a render call takes (render_impl, api_render.hip; HR_OPT_FRAME_KERNEL_ACTIVE asks with 64 rays and nothing else)
enum HrRoute { HR_ROUTE_FRAME = 0, HR_ROUTE_VERIFIED, HR_ROUTE_CHUNKED };
struct HrRouteIn {
    int64_t n_rays;
    bool fields, maps;                  // diagnostics / per-ray maps requested (maps: some pointer set)
    HrSampleKind kind;
    bool mlp_verified, occupancy;       // HrMlpState::verified; an occupancy volume is set
    bool band_stale, capturing;         // the margins are out of date; the stream is being captured (asked of a verified model with a stale band only)
    bool frame_fits;                    // hr_frame_plan(...).fits
};
// tier of a chunked route: 0 = the model's primary arithmetic, 1 = the f16x3 tiles.  calibrate_first: measure the band (calibrate_band),
// refresh mlp_verified and band_stale, ask again (route and tier are then those of a call that cannot measure)
struct HrRenderRoute { int route, tier, calibrate_first; };
// The frame kernel: the image alone of a DECODE model, where it fits.  The verified fast path: not with diagnostics (ONE arithmetic for every
// output), an occupancy volume (a head-dependent decision the band does not cover) or a stale band inside a stream capture (measuring synchronises)
static inline HrRenderRoute hr_render_route(const HrRouteIn& in)
{
    const bool decode = in.kind == HR_SAMPLE_DECODE;
    if (!in.fields && !in.maps && decode && in.frame_fits) return {HR_ROUTE_FRAME, 0, 0};
    const bool eligible = in.mlp_verified && !in.fields && !in.occupancy && in.n_rays < ((int64_t)1 << 31) && decode;
    const HrRenderRoute chunked = {HR_ROUTE_CHUNKED, in.mlp_verified ? 1 : 0, 0};
    if (eligible && in.band_stale) return {chunked.route, chunked.tier, in.capturing ? 0 : 1};
    return (eligible && in.n_rays > 0) ? HrRenderRoute{HR_ROUTE_VERIFIED, 0, 0} : chunked;
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

// The plane pairs' gradient accumulators in ONE pool, pair after pair, plane then line / time plane: offsets and counts in elements of
// `elem` bytes, every accumulator starting on a multiple of `align` bytes (a multiple of elem).  The float pool of the default build
// (256-byte starts) and the packed 64-bit fixed-point pool of the deterministic one.  A pair without channels takes nothing.
struct HrGradPool {
    size_t off_a[3], off_b[3], n_a[3], n_b[3];
    size_t total;
};
static inline HrGradPool hr_grad_pool(const HrGridPlane* planes, size_t elem, size_t align)
{
    HrGradPool p = {};
    const size_t step = align / elem;
    for (int j = 0; j < 3; ++j) {
        const HrGridPlane& g = planes[j];
        if (g.tex == 0) continue;
        p.n_a[j] = (size_t)g.aw * g.ah * g.tex;
        p.n_b[j] = (size_t)g.bw * g.bh * g.tex;
        p.off_a[j] = p.total; p.total += (p.n_a[j] + step - 1) / step * step;
        p.off_b[j] = p.total; p.total += (p.n_b[j] + step - 1) / step * step;
    }
    return p;
}

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
    // rows of basis_mat's gradient in LDS: SH's 27 as ever (RGB's 3 fit in them), an RGBtFourier model's 3 nb when that is more
    const int basis_rows = cfg.app_dim > 27 ? cfg.app_dim : 27;
    P.atomics_lds = sizeof(float) * (P.atomics_rpb * 3 * ca_total) + in.acc_bytes * (P.atomics_rpb * 3 * ca_total + basis_rows * n_basis_cols);

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
    const size_t base = sizeof(float) * (2 * rpb * 3 * ca_total + basis_rows * n_basis_cols + 4 * rpb);
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

// ---------------------------------------------------------------- MLP arithmetic (api_mlp.hip)
// largest activation a model may show in calibration for the fp16 split arithmetic to be used: a factor 8 below the IEEE-half maximum,
// because calibration sees 4096 rays and a frame has 640 000
static const float HR_F16_CALIBRATION_LIMIT = 65504.0f / 8.0f;
static const float HR_BAND_FLOOR = 1e-6f;          // four float32 ulps of the largest |zc| (2)
static const float HR_VERIFY_LISTED_LIMIT = 0.05f; // fraction of the calibration rays the first pass may list (a call's list holds a sixteenth of its rays)
static const float HR_VERIFY_RGB_LIMIT = 6e-5f;   // on <= 65 536 calibration rays; the shipped families measure 1.5e-5 - 5e-5 here and 2.3e-5 - 5.4e-5 on their 640 000-ray frames

// The verified fast path: f16f8 + a list-driven second pass in f16x3.  What it needs: a ray's samples inside one wavefront
// (the list entry is written from a wave-level vote), no cascade (the point MLP's rows are internal).  (An occupancy volume adds a
// head-dependent decision the band does not cover: hr_render then takes the f16x3 tiles throughout, see hr_render_fields.)
// The per-sample margins (hr_math.h, HrRisk) are derived for: axis planes, sphere / cylinder with fixed origins, the euclidean distance;
// the identity, affine and MIP-NeRF contractions.
static inline bool hr_mlp_can_verify(const hr_config& c, bool cascade_level)
{
    const bool isect_ok = c.isect_type == HR_ISECT_Z_PLANE || c.isect_type == HR_ISECT_VOXEL_GRID || c.isect_type == HR_ISECT_EUCLIDEAN_UNIFIED ||
                          ((c.isect_type == HR_ISECT_SPHERE || c.isect_type == HR_ISECT_CYLINDER) && c.origin_scale == 0.0f);
    return !cascade_level && c.z_channels <= 64 && c.mlp_layers >= 2 && c.mlp_hidden == 256 && isect_ok && c.contract_type != HR_CONTRACT_DONERF;
}

// The f16f8 kernels evaluate the windowed positional encoding with v_sin_f32 / v_cos_f32 of x / 2pi formed in fp32 (HR_FAST_SINCOS,
// hr_math.h): the phase error of that product grows as ~6e-8 |x| rad, and beyond 512 pi the instructions return 0 and 1.  The largest
// argument of a group is pe_base_mult * freq_mult^n_freqs times the parameterised ray coordinate (hr_ray_features forms it by the same
// repeated product); up to HR_FAST_SINCOS_MAX_FREQ = 16 the phase error of a coordinate of order one stays at the ~1e-6 HR_SINCOS grants
// the instructions anyway (6e-8 x 16).  The five benchmark families have at most 4.  Beyond it f16f8 is not run (hr_mlp_choice).
static const float HR_FAST_SINCOS_MAX_FREQ = 16.0f;
static inline bool hr_mlp_fast_sincos_ok(const hr_config& c)
{
    for (int g = 0; g < c.n_groups && g < HR_MAX_GROUPS; ++g) {
        const hr_param_group& pg = c.groups[g];
        if (pg.pe_type != HR_PE_WINDOWED || pg.pe_n_freqs <= 0) continue;
        float f = 1.0f;
        for (int j = 0; j < pg.pe_n_freqs; ++j) f = f * pg.pe_freq_mult;
        if (!(fabsf(pg.pe_base_mult * f) <= HR_FAST_SINCOS_MAX_FREQ)) return false;
    }
    return true;
}

// Which arithmetic a model's MLP runs.  act_max[l]: the calibration's largest |input feature| (l = 0) and |pre-activation| of hidden
// Linear l - 1; all zero before a measurement, and read only when needs_calibration comes back set -- the caller then measures and asks
// again.  HR_MLP_AUTO becomes the verified fast path (f16f8, verified) when every one of them is finite and below
// HR_F16_CALIBRATION_LIMIT and the model can be verified, f16x3 when it cannot, and bf16x3 (fp32 exponent range) when they are not;
// a FORCED fp16 mode that fails the test is HR_E_RANGE, a forced f16f8v on a model that cannot be verified (or a width the range
// kernel does not cover: range_supported) HR_E_INVALID.  A windowed encoding beyond HR_FAST_SINCOS_MAX_FREQ (hr_mlp_fast_sincos_ok)
// takes f16f8 away: HR_MLP_AUTO and a forced f16f8 / f16f8v are f16x3 there (IEEE sincosf, nothing verified; HR_E_RANGE as for a forced
// f16x3) -- a fall-back that HR_OPT_MLP_PRECISION_ACTIVE reports, not a refusal: shipped nets are beyond the limit (stanford_z_plane_mem:
// two-plane coordinates at 2^6) and render under a forced f16f8.
struct HrMlpChoice {
    int active_precision, verified;
    bool needs_calibration;
    int status;                   // HR_OK | HR_E_RANGE | HR_E_INVALID
};
static inline HrMlpChoice hr_mlp_choice(const hr_config& c, HrSampleKind kind, bool cascade_level, bool range_supported, const float* act_max)
{
    const int want = c.mlp_precision;
    if (c.mlp_layers == 0 || want == HR_MLP_FP32 || want == HR_MLP_BF16X3)
        return {(c.mlp_layers == 0 && want == HR_MLP_AUTO) ? HR_MLP_F16X3 : want, 0, false, HR_OK};
    if (want == HR_MLP_AUTO && c.mlp_hidden != 256) return {HR_MLP_FP32, 0, false, HR_OK};      // the split kernels are written for 256-wide layers
    if (!range_supported) return {want, 0, true, HR_E_INVALID};
    bool fits = true;
    for (int l = 0; l < c.mlp_layers; ++l) fits = fits && isfinite(act_max[l]) && act_max[l] < HR_F16_CALIBRATION_LIMIT;
    // f16f8, and so verification, only for the DECODE kind (the verified path's margins are not derived for the colour network, DESIGN 3l, nor
    // its calibration -- its colour bar, its list passes through the stand-alone sample kernel -- for the time kernel, 3m): f16x3 there
    const bool f8_ok = kind == HR_SAMPLE_DECODE && hr_mlp_fast_sincos_ok(c), can_verify = f8_ok && hr_mlp_can_verify(c, cascade_level);
    if (want == HR_MLP_AUTO) {
        if (!fits) return {HR_MLP_BF16X3, 0, true, HR_OK};
        return {can_verify ? HR_MLP_F16F8 : HR_MLP_F16X3, can_verify ? 1 : 0, true, HR_OK};
    }
    if ((want == HR_MLP_F16F8 || want == HR_MLP_F16F8V) && !f8_ok) return {HR_MLP_F16X3, 0, true, fits ? HR_OK : HR_E_RANGE};
    if (want == HR_MLP_F16F8V && !can_verify) return {want, 0, true, HR_E_INVALID};
    if (!fits) return {want, 0, true, HR_E_RANGE};
    return {want == HR_MLP_F16F8V ? HR_MLP_F16F8 : want, want == HR_MLP_F16F8V ? 1 : 0, true, HR_OK};
}
// ... of a model without a density mode: the kind the shading alone gives
static inline HrMlpChoice hr_mlp_choice(const hr_config& c, bool cascade_level, bool range_supported, const float* act_max) { return hr_mlp_choice(c, hr_sample_kind(c.shading, false), cascade_level, range_supported, act_max); }

// The caller's calibration rays that stay with the model (the band of the verified fast path is measured on them, again after
// hr_model_update_config): every stride-th of the n, at most 65 536
struct HrCalibSample {
    int64_t stride, keep;
};
static inline HrCalibSample hr_calib_sample(int64_t n)
{
    const int64_t stride = (n + 65535) / 65536;
    return {stride, (n + stride - 1) / stride};
}

// The margins of the verified fast path (hr_math.h, HrRisk: of zc, of a point coordinate per unit of amplification, of the point-offset /
// flow heads) from the largest differences the two arithmetics showed on the calibration rays (hr_verify_info): 4 x, never below the floor
struct HrBand {
    float band, band_q, band_off;
};
static inline HrBand hr_band_margins(float max_d_zc, float max_d_dist_n, float max_d_geo_n, float max_d_off)
{
    return {fmaxf(HR_BAND_FLOOR, 4.0f * fmaxf(max_d_zc, max_d_dist_n)), fmaxf(HR_BAND_FLOOR, 4.0f * max_d_geo_n), 4.0f * max_d_off};
}

// hr_verify_info::listed_frac: `listed` of the n_used well-conditioned calibration rays were listed by the first pass (not measured on
// fewer than 64).  The CALLER's rays (calibrated == 2) are what will be rendered: the ill-conditioned ones among all N are listed too
// (synthetic rays point anywhere; half of them graze a z-plane net's planes, which says nothing about its cameras)
static inline float hr_listed_frac(int calibrated, int64_t N, int64_t n_used, unsigned listed)
{
    float frac = n_used >= 64 ? (float)((double)listed / (double)n_used) : 0.0f;
    if (calibrated == 2) frac = (float)(((double)(N - n_used) + (double)frac * (double)n_used) / (double)N);
    return frac;
}

// hr_verify_info::fallback -- HR_MLP_AUTO gives the fast path up (f16x3 throughout: it lists nothing and has neither problem) with
// 1: more than a twentieth of the rays would be rendered twice (a call's list holds a sixteenth), 2: the cheap arithmetic's own error is
// too large a share of the 1e-4 budget on this model (or not a number)
static inline int hr_verify_fallback(float listed_frac, float max_d_rgb)
{
    if (!(max_d_rgb <= HR_VERIFY_RGB_LIMIT)) return 2;
    return listed_frac > HR_VERIFY_LISTED_LIMIT ? 1 : 0;
}

// ---------------------------------------------------------------- MLP shading (shade_kernel.hip, sample_shade_kernel.hip; layout: hr_shade.h)
// A model whose colour comes from TensoRF's per-sample network (HR_SHADING_MLP_FEA / HR_SHADING_MLP) renders a chunk in three launches
// after the ray MLP: the sample stage in its export form (per sorted sample a 32-float row: 27 features, the view direction, a live
// flag, a zero), the shading kernel over all rows of the chunk, and the sample stage in its import form, which composites the
// network's colours exactly as it composites decoded ones.
#define HR_SHADE_FEAT 27
#define HR_SHADE_ROW 32           // floats of an exported row: [f 0..26 | v 27..29 | live 30 | 0]
#define HR_SHADE_MAX_PE 6
#define HR_SHADE_MAX_C 256
#define HR_SHADE_MAX_Z 64
#define HR_SHADE_TILE_M 64        // rows of one MFMA tile of the shading kernel
#define HR_SHADE_SPAN 512         // consecutive rows a workgroup of the shading kernel owns: their live rows, compacted, fill its tiles

// width of the network's input: tensorf_base.py:43 (MLPRender_Fea), :111 (MLPRender)
static inline int hr_shade_width(int shading, int view_pe, int fea_pe)
{
    return HR_SHADE_FEAT + 3 + 2 * 3 * view_pe + (shading == HR_SHADING_MLP_FEA ? 2 * HR_SHADE_FEAT * fea_pe : 0);
}

struct HrShadePlan {
    int k0, k0p;                // input width, padded to a multiple of 16 (the k-step of the fp32 tiles)
    int hp, nt_h;               // hidden width padded to 16, its 16-column tiles
    int nt_wave;                // column tiles per wavefront in the hidden layers: ceil(nt_h / 4), 1..4 (the kernel's template argument)
    int rows_per_tile;          // HR_SHADE_TILE_M; a workgroup compacts the live rows of HR_SHADE_SPAN rows into such tiles
    int stride;                 // LDS row stride in floats: max(k0p, hp) + 4 (the hidden activations overwrite the input rows in place)
    size_t lds;                 // dynamic LDS of a workgroup
    size_t ws_bytes_per_ray;    // workspace of a chunk per ray: the exported rows and the network's colours
    int launches;               // launches per chunk besides the ray MLP's
};
static inline HrShadePlan hr_shade_plan(int shading, int view_pe, int fea_pe, int feature_c, int z_channels)
{
    HrShadePlan P = HrShadePlan();
    P.k0 = hr_shade_width(shading, view_pe, fea_pe);
    P.k0p = (P.k0 + 15) & ~15;
    P.hp = (feature_c + 15) & ~15;
    P.nt_h = P.hp / 16;
    P.nt_wave = (P.nt_h + 3) / 4;
    P.rows_per_tile = HR_SHADE_TILE_M;
    P.stride = (P.k0p > P.hp ? P.k0p : P.hp) + 4;
    P.lds = (size_t)HR_SHADE_TILE_M * P.stride * sizeof(float);
    P.ws_bytes_per_ray = (size_t)z_channels * (HR_SHADE_ROW + 3) * sizeof(float);
    P.launches = 3;
    return P;
}
// workgroups of the shading kernel over n rows
static inline int64_t hr_shade_blocks(int64_t n_rows) { return (n_rows + HR_SHADE_SPAN - 1) / HR_SHADE_SPAN; }
// rays per launch of an MLP-shaded model when the caller reserves nothing: the chunk's shading workspace stays within 256 MB
static inline int64_t hr_shade_default_chunk(int64_t head_chunk, const HrShadePlan& P)
{
    int64_t rays = ((int64_t)256 << 20) / (int64_t)P.ws_bytes_per_ray;
    rays &= ~(int64_t)63;
    if (rays < 64) rays = 64;
    return rays < head_chunk ? rays : head_chunk;
}
// the export form's live flag: the reference's app_mask, weight > rm_weight_mask_thre (strict; tensorf_no_sample.py:201).  Tiles of the
// shading kernel without a flagged row are skipped, and the import form masks by the flag, not by its own weight (the two forms sum
// the density in different orders: their weights agree to rounding, not always in a comparison)
static constexpr inline bool hr_shade_live(float weight, float thresh) { return weight > thresh; }

// ---------------------------------------------------------------- time-dependent decode modes (sample_time_kernel.hip; definitions: hr_time_decode.h)
// A model with `shadingMode: RGBtLinear | RGBtFourier | RGBIdentity` or `densityMode: DensityLinear | DensityFourier` renders every chunk
// with its own sample kernel (hr_sample_maps_kernel's statements; never the frame kernel or the verified fast path).  Per ray it keeps in
// LDS: the decode matrix folded with the ray's time basis (per_ray_M: the RGBt modes, as SH -- hr_sample_lds_bytes has always counted a
// matrix per ray) and, with a density mode, the ray's density row: in the decode matrix's shape (3 x ca_total, rows 1, 2 zero) for the
// class gathers, whose density lanes read it where they read the ones block, and one weight per density slot for the generic gather.
static inline bool hr_time_per_ray_M(int shading) { return hr_shading_relu_half(shading); }
static inline int hr_time_density_slots(const HrGridPlane* planes, int ca_total, int pclass)
{
    return pclass != 0 ? 3 * ca_total : 4 * (planes[0].cd4 + planes[1].cd4 + planes[2].cd4);
}

// ---------------------------------------------------------------- the sample stage of one launch, in every form (launch_samples, api_render.hip)
// A launch's form: the model's kind and which of its kernels -- DECODE: with the per-ray maps or without; SHADE: the export or the import form
struct HrSampleForm { HrSampleKind kind; bool maps, exported; };
// hr_sample_plan extended by the form's own block behind the plan's LDS: its float offset, and the floats of a ray's density row
struct HrSampleFormPlan : HrSamplePlan { int x_off, d_slots; };
// The one planner: hr_sample_plan for DECODE (rows_emitted is that kind's alone).  SHADE: the generic gather; its export form keeps all rows of basis_mat.
// The time kernel decides the second factor's taps at run time (no line form; the class is kept); with a density mode it keeps the workgroup's density rows
static inline HrSampleFormPlan hr_sample_form_plan(const hr_config& cfg, const HrGridPlane* planes, int ca_total, int nq, int rows_per_ray, int64_t n_rays,
                                                   bool rows_emitted, const HrSampleForm& form)
{
    HrSampleFormPlan P = {hr_sample_plan(cfg, planes, ca_total, nq, rows_per_ray, n_rays, rows_emitted && form.kind == HR_SAMPLE_DECODE), 0, 0};
    if (form.kind == HR_SAMPLE_SHADE) P.pclass = 0;
    if (form.kind != HR_SAMPLE_DECODE) P.all_lines = 0;
    if (form.kind == HR_SAMPLE_TIME_DENSITY) P.d_slots = hr_time_density_slots(planes, ca_total, P.pclass);
    const int block = form.kind == HR_SAMPLE_TIME_DENSITY ? (256 / P.zp) * P.d_slots : (form.kind == HR_SAMPLE_SHADE && form.exported) ? HR_SHADE_FEAT * ca_total : -1;
    if (block >= 0) P.x_off = (int)(P.lds / sizeof(float)), P.lds += sizeof(float) * (size_t)block;
    P.big_lds = P.lds > 64 * 1024;
    return P;
}

// true: a level of configuration c with p_live live head columns is refused for a sample stage of `kind`; *bytes: the request of the kind's largest
// form.  The margin set aside next to it: 4096 bytes for the kernel's static words (the ray records, hr_gather_ones) and the 256-float cross-wave
// scratch, reserved for every sample count although hr_sample_lds_bytes asks for it only above 64 samples -- the bound has always counted it.
static inline bool hr_sample_lds_refused(const hr_config& c, int p_live, HrSampleKind kind, size_t* bytes)
{
    HrGridPlane pl[3];
    int ca_total = 0, n_basis_cols = 0;
    (void)hr_plane_geometry(c, pl, &ca_total, &n_basis_cols);      // (an inconsistent geometry is refused by hr_model_finalize)
    const HrSamplePlan P = hr_sample_form_plan(c, pl, ca_total, hr_head_quads(c, p_live), rows_per_ray(c), 1, false, HrSampleForm{kind, false, true});
    *bytes = P.lds;
    return *bytes + 4096 + (P.zp > 64 ? 0 : 256 * sizeof(float)) > HR_LDS_PER_WORKGROUP;
}
static inline bool hr_sample_lds_refused(const hr_config& c, int p_live, size_t* bytes) {      // hr_model_create: the kind the shading alone gives
    return hr_sample_lds_refused(c, p_live, hr_sample_kind(c.shading, false), bytes);
}

#endif  // HR_PLAN_H
