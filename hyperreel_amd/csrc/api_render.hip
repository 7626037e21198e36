// C ABI, rendering: kernel arguments from the model, the launch plans of hr_render (chunked two-kernel, frame kernel, cascade front,
// verified fast path) and the single-stage entry points.
#include <hip/hip_runtime.h>

#include "hr_model.h"

// tier: 0 = the model's primary arithmetic; the verified fast path's later passes: 1 = its f16x3 tiles, 2 = its bf16x3 tiles (fill_mlp_args(..., tier))
void launch_mlp(const hr_model* m, const hr_config& c, const HrMlpArgs& a, hipStream_t st, int tier)
{
    if (c.mlp_layers == 0) return;               // ZeroMLP: the workspace already holds the (all-zero) head
    const int prec = tier == 1 ? HR_MLP_F16X3 : (tier == 2 ? HR_MLP_BF16X3 : m->mlp.active_precision);
    if (prec == HR_MLP_BF16X3) hr_launch_mlp_bf16x3(c, a, st);
    else if (prec == HR_MLP_F16X3) hr_launch_mlp_f16x3(c, a, st);
    else if (prec == HR_MLP_F16X2) hr_launch_mlp_f16x2(c, a, st);
    else if (prec == HR_MLP_F16F8) hr_launch_mlp_f16f8(c, a, st);
    else hr_launch_mlp(c, a, st);
}

void fill_mlp_args(const hr_model* m, HrMlpArgs& a, const float* rays, int64_t n, int tier)
{
    const HrMlpTiles& t = m->mlp.pack->tiles[tier];
    a.rays = rays;
    a.n_rays = n;
    a.head = m->head;
    for (int l = 0; l < HR_MAX_LAYERS; ++l) {
        a.wpack[l] = t.wpack[l];
        a.wsplit[l] = t.wsplit[l];
        a.bias[l] = t.bias[l];
        a.winv[l] = t.winv[l];
        a.xexp[l] = tier > 0 ? 0 : m->mlp.xexp[l];
        a.n_tiles[l] = t.n_tiles[l];
    }
    a.ray0 = 0;
    a.ray_index = nullptr;
    a.n_rays_dev = nullptr;
    a.list_off = 0;
    a.n_rays_copy = nullptr;
    a.redo_list = nullptr;
    a.redo_count = nullptr;
    a.redo_cap = 0;
    a.n_out = m->mlp.pack->n_out;
    a.nq = (m->mlp.pack->n_out + 3) / 4;
    a.k0p = m->mlp.pack->k0p;
    a.trace = nullptr;
    a.flags = m->flags;
}

// Plane pair j as the render kernels get it.  Inside hr_render_frame on a keyframe net all rays of the call share one time, and that time
// sits on a keyframe row (advect_points quantises it, utils/flow_utils.py:10-35): the time plane is then handed over as the LINE that
// row is -- the gather's line form, 2 taps instead of 4 (the other row's weight is the 1e-7 left by rounding, see hr_render_frame).
static HrGridPlane render_plane(const hr_model* m, int j)
{
    HrGridPlane g = m->planes[j];
    if (m->frame_row >= 0 && m->frame_line[j]) {
        g.b = m->frame_line[j];
        g.bh = g.bw;
        g.bw = 1;
    }
    return g;
}

void fill_sample_args(const hr_model* m, HrSampleArgs& a, const float* rays, int64_t n, float* rgb)
{
    a.cfg_dev = m->kcfg_dev;
    a.rays = rays;
    a.head = m->head;
    a.nq = (m->mlp.pack->n_out + 3) / 4;
    a.n_rays = n;
    a.rgb = rgb;
    a.fields = hr_fields();
    for (int j = 0; j < 3; ++j) a.planes[j] = render_plane(m, j);
    a.basis = m->basis;
    a.basis_t = m->basis_t;
    a.slot_col = m->slot_col;
    a.basis_ld = m->basis_ld;
    a.n_basis_cols = m->n_basis_cols;
    a.ca_total = m->ca_total;
    // the table is read in place from the uploaded copy (12 floats per camera, no re-layout)
    a.color_table = nullptr;
    if (m->cfg.color_table_views > 0) {
        auto it = m->raw.find("color_embedding");
        if (it != m->raw.end()) a.color_table = it->second.p;
    }
    a.ray0 = 0;
    a.ray_index = nullptr;
    a.n_rays_dev = nullptr;
    a.list_off = 0;
    a.zero_word = nullptr;
    a.redo_list = nullptr;
    a.redo_count = nullptr;
    a.redo_cap = 0;
    a.redo_band = a.redo_band_q = a.redo_band_off = a.redo_amp_cut = 0.0f;
    a.flags = m->flags;
    a.occ = m->occ;
    a.occ_cells = m->occ_cells;
    a.occ_w = m->occ_n[0]; a.occ_h = m->occ_n[1]; a.occ_d = m->occ_n[2];
    for (int i = 0; i < 3; ++i) { a.occ_lo[i] = m->occ_lo[i]; a.occ_inv[i] = m->occ_inv[i]; }
    a.rows_per_ray = rows_per_ray(m->cfg);
    a.rows_out = nullptr;
    a.row_dim = a.n_row_inputs = 0;
    for (int i = 0; i < 4; ++i) a.row_kind[i] = a.row_len[i] = 0;
}

static void fill_shade_args(const hr_model* m, HrShadeArgs& a, const float* feat, int64_t feat_ld, const float* vdir, int64_t vdir_ld, int64_t n_rows,
                            float* rgb)
{
    const HrShadeNet& g = m->shade_net;
    a.net = g;
    a.stride = hr_shade_plan(g.shading, g.view_pe, g.fea_pe, g.feature_c, 1).stride;
    a.feat = feat; a.feat_ld = feat_ld;
    a.vdir = vdir; a.vdir_ld = vdir_ld;
    a.live_col = -1;
    a.n_rows = n_rows;
    a.rgb = rgb;
    for (int l = 0; l < 3; ++l) { a.wpack[l] = m->shade_w[l]; a.bias[l] = m->shade_b[l]; }
}

static void fill_time_io(const hr_model* m, HrTimeIO& io, bool density)
{
    io = HrTimeIO();
    io.fpk = m->time_set ? m->time_desc.frames_per_keyframe : 1;
    io.fac = m->time_set ? hr_time_scale(m->cfg.num_keyframes, m->time_desc.num_frames) : 0.0f;
    io.c_fourier = m->cfg.shading == HR_SHADING_RGBT_FOURIER;
    if (!density) return;
    io.d_fourier = m->time_desc.density_mode == HR_DENSITY_FOURIER;
    io.dbasis_t = m->dbasis_t, io.dslot_col = m->dslot_col;
    io.d_ld = m->d_ld, io.d_slots = m->d_slots;
}

// the caller's maps (NULL: none) from the launch's first ray r0 on
static hr_maps maps_from(const hr_maps* maps, int64_t r0)
{
    hr_maps mp = maps ? *maps : hr_maps();
    if (mp.distances_dev) mp.distances_dev += r0;
    if (mp.points_dev) mp.points_dev += r0 * 3;
    if (mp.acc_dev) mp.acc_dev += r0;
    return mp;
}

// Cascade, everything before the final sample kernel: coarse MLP -> coarse intersect (emits the point MLP's input
// rows, one per coarse sample) -> point MLP over n * casc_in_z rows.  Leaves the fine head in m->head.
static void launch_cascade_front(hr_model* m, const float* rays, int64_t n, hipStream_t st)
{
    hr_model* c0 = m->coarse.get();
    HrMlpArgs ma;
    fill_mlp_args(c0, ma, rays, n);
    launch_mlp(c0, c0->kcfg, ma, st);
    HrSampleArgs sa;
    fill_sample_args(c0, sa, rays, n, nullptr);
    sa.rows_out = m->rows;
    sa.row_dim = m->cfg.casc_row_dim;
    sa.n_row_inputs = m->cfg.casc_n_inputs;
    for (int i = 0; i < 4; ++i) { sa.row_kind[i] = m->cfg.casc_input_kind[i]; sa.row_len[i] = m->cfg.casc_input_dim[i]; }
    hr_launch_samples(c0->kcfg, sa, st);
    hr_config kc = m->kcfg;
    kc.ray_dim = m->cfg.casc_row_dim;            // the point MLP's "rays" are the rows
    HrMlpArgs mb;
    fill_mlp_args(m, mb, m->rows, n * m->cfg.casc_in_z);
    launch_mlp(m, kc, mb, st);
}

// The MLP stage of a chunked launch (tier 1: the whole launch with the f16x3 tiles -- one arithmetic for every output)
void launch_front(hr_model* m, const float* rays, int64_t n, hipStream_t st, int tier)
{
    if (m->coarse) {
        launch_cascade_front(m, rays, n, st);
        return;
    }
    HrMlpArgs ma;
    fill_mlp_args(m, ma, rays, n, tier);
    launch_mlp(m, m->kcfg, ma, st, tier);
}

// What hr_render_route decides a call of n rays by, as the model stands (`capturing` is the caller's to ask); *frame: the frame kernel's plan
HrRouteIn render_route_facts(const hr_model* m, int64_t n, bool fields, bool maps, HrFramePlan* frame)
{
    const int prec = m->mlp.active_precision, L = m->cfg.mlp_layers;
    const bool split = prec == HR_MLP_BF16X3 || prec == HR_MLP_F16X3 || prec == HR_MLP_F16X2 || prec == HR_MLP_F16F8;      // their elements: 16 bits (HrMlpTiles::wsplit)
    const HrFramePlanIn in = {n, m->opt_frame_kernel, m->opt_sample_waves, m->coarse || m->is_coarse, m->mlp.verified != 0, split, sizeof(uint16_t),
                              (m->mlp.pack->n_out + 3) / 4, m->mlp.pack->k0p, L > 0 ? m->mlp.pack->tiles[0].n_tiles[L - 1] : 0, m->n_cus};
    const HrGridPlane planes[3] = {render_plane(m, 0), render_plane(m, 1), render_plane(m, 2)};
    const HrFramePlan P = hr_frame_plan(m->kcfg, planes, m->ca_total, in);
    if (frame) *frame = P;
    return {n, fields, maps, hr_model_sample_kind(m), m->mlp.verified != 0, (bool)m->occ, m->mlp.band_stale, false, P.fits != 0};
}

// The frame kernel (fused_impl.inc) of plan P for the whole ray list; false: the runtime refused the kernel's LDS request (nothing launched)
static bool launch_frame(hr_model* m, const HrFramePlan& P, const float* rays, int64_t n, float* rgb, hipStream_t st)
{
    const int prec = m->mlp.active_precision;
    HrMlpArgs ma;
    fill_mlp_args(m, ma, rays, n);
    ma.head = nullptr;
    HrSampleArgs sa;
    fill_sample_args(m, sa, rays, n, rgb);
    sa.head = nullptr;
    const auto launch = prec == HR_MLP_BF16X3 ? hr_launch_frame_bf16x3 : prec == HR_MLP_F16X3 ? hr_launch_frame_f16x3 : prec == HR_MLP_F16X2 ? hr_launch_frame_f16x2 : hr_launch_frame_f16f8;
    return launch(m->kcfg, ma, sa, P, st);
}

static int check_render(const hr_model* m, const float* rays, int64_t n, const float* rgb)
{
    if (!m) return fail(HR_E_INVALID, "null model");
    if (!m->finalized) return fail(HR_E_STATE, "hr_model_finalize has not been called");
    if (n < 0) return fail(HR_E_INVALID, "negative ray count");
    if (n > 0 && (!rays || !rgb)) return fail(HR_E_INVALID, "null ray / rgb buffer");
    return HR_OK;
}

// The sample stage of one launch, by the model's kind (hr_plan.h: the launchers plan their form with hr_sample_form_plan).  maps: hr_render_maps' (non-NULL:
// some pointer set).  r0: the launch's first ray in the caller's buffers, as args.rgb is offset (0 for the list-driven passes, whose rays are indices into the call)
// false: the launch's pixels are not written (SHADE: the shading kernel's LDS request was refused; TIME_DENSITY: the density row's table was made for another plan)
static bool launch_samples(const hr_model* m, const HrSampleArgs& sa, const hr_maps* maps, int64_t r0, hipStream_t st)
{
    const hr_maps mp = maps_from(maps, r0);
    switch (const HrSampleKind kind = hr_model_sample_kind(m)) {
        case HR_SAMPLE_DECODE:
            if (maps) hr_launch_samples_maps(m->kcfg, sa, mp, st);
            else hr_launch_samples(m->kcfg, sa, st);
            return true;
        case HR_SAMPLE_SHADE: {     // the chunk's samples exported, shaded by the colour network, composited by the import form
            HrSampleArgs ex = sa;
            ex.fields = hr_fields();                    // diagnostics are the import form's
            hr_launch_samples_shade_export(m->kcfg, ex, m->shade_rows, st);
            HrShadeArgs ha;
            fill_shade_args(m, ha, m->shade_rows, HR_SHADE_ROW, m->shade_rows + HR_SHADE_FEAT, HR_SHADE_ROW, sa.n_rays * m->cfg.z_channels, m->shade_rgb);
            ha.live_col = HR_SHADE_FEAT + 3;
            if (!hr_launch_shade(ha, st)) return false;
            hr_launch_samples_shade_import(m->kcfg, sa, mp, m->shade_rows, m->shade_rgb, st);
            return true;
        }
        case HR_SAMPLE_TIME:
        case HR_SAMPLE_TIME_DENSITY:        // one kernel for image, maps and diagnostics
            HrTimeIO io;
            fill_time_io(m, io, kind == HR_SAMPLE_TIME_DENSITY);
            return (kind == HR_SAMPLE_TIME_DENSITY ? hr_launch_samples_time_density : hr_launch_samples_time)(m->kcfg, sa, mp, io, st);
    }
    return false;
}

// The verified fast path over one call's rays: first pass in f16f8 with the rays at risk listed on the device, then the list
// again with the f16x3 tiles (in slices of the chunk's head workspace), then whatever left the half range there with the bf16x3 tiles.
// list_cap: entries of the list this call may use.  maps: every pass writes the maps of the rays it writes pixels of (launch_samples)
void render_verified(hr_model* m, const HrBand& band, const float* rays_dev, int64_t n_rays, float* rgb_dev, int list_cap, hipStream_t st, const hr_maps* maps)
{
    const hr_config& c = m->cfg;
    const int64_t per = hr_even_chunk(m->chunk, n_rays);
    for (int64_t r0 = 0; r0 < n_rays; r0 += per) {
        const int64_t n = (n_rays - r0 < per) ? (n_rays - r0) : per;
        const float* rays = rays_dev + r0 * c.ray_dim;
        HrMlpArgs ma;
        fill_mlp_args(m, ma, rays, n, 0);
        ma.ray0 = r0;                                  // tiles that raise a range bit list their rays (indices start at r0)
        ma.redo_list = m->redo_list;
        ma.redo_count = m->redo_count;
        ma.redo_cap = list_cap;
        launch_mlp(m, m->kcfg, ma, st, 0);
        HrSampleArgs sa;
        fill_sample_args(m, sa, rays, n, rgb_dev + r0 * 3);
        sa.ray0 = r0;
        sa.redo_list = m->redo_list;
        sa.redo_count = m->redo_count;
        sa.redo_cap = list_cap;
        sa.redo_band = band.band;
        sa.redo_band_q = band.band_q;
        sa.redo_band_off = band.band_off;
        sa.redo_amp_cut = HR_VERIFY_AMP_CUT;
        launch_samples(m, sa, maps, r0, st);
    }
    // second pass: the listed rays (count on the device: the launches are sized for the capacity, blocks past the count leave at once) through
    // the f16x3 tiles, gathered from / scattered to the caller's buffers by index.  The head workspace is free again; a list longer than it is
    // walked in slices.  The counter is cleared for the next call by the FIRST slice's sample kernel, which like every later launch of the
    // pass reads the copy the first slice's MLP kernel made (a memset node between calls does not survive hipGraph replay)
    for (int64_t off = 0; off < list_cap; off += m->chunk) {
        const int64_t cap = (list_cap - off < m->chunk) ? (list_cap - off) : m->chunk;
        HrMlpArgs ma;
        fill_mlp_args(m, ma, rays_dev, cap, 1);
        ma.ray_index = m->redo_list + off;
        ma.list_off = off;
        ma.n_rays_dev = off == 0 ? m->redo_count : m->redo_count + 1;
        ma.n_rays_copy = off == 0 ? m->redo_count + 1 : nullptr;
        ma.redo_list = m->wide_list;                   // a tile of THIS pass in which an activation leaves the half range goes on to the third
        ma.redo_count = m->redo_count + 2;
        ma.redo_cap = m->wide_cap;
        launch_mlp(m, m->kcfg, ma, st, 1);
        HrSampleArgs sa;
        fill_sample_args(m, sa, rays_dev, cap, rgb_dev);
        sa.ray_index = m->redo_list + off;
        sa.list_off = off;
        sa.n_rays_dev = m->redo_count + 1;
        sa.zero_word = off == 0 ? m->redo_count : nullptr;
        launch_samples(m, sa, maps, 0, st);
    }
    // third pass: those tiles' rays with the bf16x3 tiles -- halves with the fp32 exponent range, nothing to overflow.  What a captured
    // viewer loop gets where the host's guard (models.py: a sticky bit read between calls) cannot reach
    HrMlpArgs ma;
    fill_mlp_args(m, ma, rays_dev, m->wide_cap, 2);
    ma.ray_index = m->wide_list;
    ma.n_rays_dev = m->redo_count + 2;
    ma.n_rays_copy = m->redo_count + 3;
    launch_mlp(m, m->kcfg, ma, st, 2);
    HrSampleArgs sa;
    fill_sample_args(m, sa, rays_dev, m->wide_cap, rgb_dev);
    sa.ray_index = m->wide_list;
    sa.n_rays_dev = m->redo_count + 3;
    sa.zero_word = m->redo_count + 2;
    launch_samples(m, sa, maps, 0, st);
}

// hr_render, hr_render_fields and hr_render_maps (and their hr_render_frame forms) in one: `fields` non-NULL = diagnostics (one arithmetic,
// the f16x3 tiles throughout, for every output), `maps` non-NULL = the per-ray maps on the plan hr_render takes, except the frame kernel
static int render_impl(hr_model* m, const float* rays_dev, int64_t n_rays, float* rgb_dev, const hr_fields* fields, const hr_maps* maps,
                       hipStream_t st)
{
    int rc = check_render(m, rays_dev, n_rays, rgb_dev);
    if (rc != HR_OK) return rc;
    if (maps && !maps->distances_dev && !maps->points_dev && !maps->acc_dev) maps = nullptr;
    const hr_config& c = m->cfg;
    const int Z = c.z_channels;
    // the plan the call takes: hr_render_route (whether the stream is being captured matters to a verified model with a stale band alone)
    HrFramePlan frame;
    HrRouteIn in = render_route_facts(m, n_rays, fields != nullptr, maps != nullptr, &frame);
    if (in.mlp_verified && in.band_stale) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
        in.capturing = cs != hipStreamCaptureStatusNone;
    }
    HrRenderRoute route = hr_render_route(in);
    if (route.calibrate_first) {
        rc = calibrate_band(m, st);
        if (rc != HR_OK) return rc;
        in.mlp_verified = m->mlp.verified != 0, in.band_stale = m->mlp.band_stale;      // HR_MLP_AUTO may just have given the fast path up
        route = hr_render_route(in);
    }
    switch (route.route) {
        case HR_ROUTE_VERIFIED:
            render_verified(m, m->mlp.band, rays_dev, n_rays, rgb_dev, hr_redo_list_cap(n_rays, m->redo_cap), st, maps);
            break;
        case HR_ROUTE_FRAME:
            if (n_rays <= 0 || launch_frame(m, frame, rays_dev, n_rays, rgb_dev, st)) break;
            [[fallthrough]];                               // the runtime refused the frame kernel's LDS request: launch by launch
        case HR_ROUTE_CHUNKED: {
            // (the sample stage of chunk i on a second stream under the MLP of chunk i + 1 is slower than back-to-back launches, 3.0-3.9
            //  vs 2.79 ms per 800x800 frame: the two kernels do not interleave on the CUs -- DESIGN 10)
            const int64_t per = hr_even_chunk(m->chunk, n_rays);
            for (int64_t r0 = 0; r0 < n_rays; r0 += per) {
                const int64_t n = (n_rays - r0 < per) ? (n_rays - r0) : per;
                const float* rays = rays_dev + r0 * c.ray_dim;
                launch_front(m, rays, n, st, route.tier);
                HrSampleArgs sa;
                fill_sample_args(m, sa, rays, n, rgb_dev + r0 * 3);
                if (fields) {
                    if (fields->distances_dev) sa.fields.distances_dev = fields->distances_dev + r0 * Z;
                    if (fields->points_dev) sa.fields.points_dev = fields->points_dev + r0 * Z * 3;
                    if (fields->sigma_dev) sa.fields.sigma_dev = fields->sigma_dev + r0 * Z;
                    if (fields->weights_dev) sa.fields.weights_dev = fields->weights_dev + r0 * Z;
                    if (fields->head_dev)
                        hr_launch_head_export(m->head, fields->head_dev + r0 * (int64_t)Z * c.preds_per_z, n, Z, c.preds_per_z, m->p_live,
                                              (m->mlp.pack->n_out + 3) / 4, rows_per_ray(c), m->col_map, st);
                }
                if (!launch_samples(m, sa, maps, r0, st))
                    return fail(HR_E_HIP, hr_model_time_kernel(m) ? "the density row's table does not fit the launch's plan" : "the shading kernel's LDS request was refused");
            }
            break;
        }
    }
    HR_HIP(hipGetLastError());
    return HR_OK;
}

int hr_render_fields(hr_model* m, const float* rays_dev, int64_t n_rays, float* rgb_dev, const hr_fields* fields, void* stream)
{
    return render_impl(m, rays_dev, n_rays, rgb_dev, fields, nullptr, (hipStream_t)stream);
}

int hr_render_maps(hr_model* m, const float* rays_dev, int64_t n_rays, float* rgb_dev, const hr_maps* maps, void* stream)
{
    return render_impl(m, rays_dev, n_rays, rgb_dev, nullptr, maps, (hipStream_t)stream);
}

int hr_render(hr_model* m, const float* rays_dev, int64_t n_rays, float* rgb_dev, void* stream)
{
    return render_impl(m, rays_dev, n_rays, rgb_dev, nullptr, nullptr, (hipStream_t)stream);
}

int hr_render_frame_maps(hr_model* m, const float* rays_dev, int64_t n_rays, float time, float* rgb_dev, const hr_maps* maps, void* stream)
{
    if (!m) return fail(HR_E_INVALID, "null model");
    const hr_config& c = m->cfg;
    hipStream_t st = (hipStream_t)stream;
    m->frame_row = -1;
    if (c.video && c.num_keyframes >= 2 && !m->coarse && !m->is_coarse && c.grid_dtype != HR_GRID_FP16 && m->finalized) {
        const HrTimeTap t = hr_frame_time_tap(c, time);      // the time tap every ray of the frame shares
        for (int j = 0; j < 3; ++j) {
            const HrGridPlane& p = m->planes[j];
            if (p.bw <= 1 || p.cd4 + p.ca4 == 0) continue;
            const int row_floats = p.bw * p.tex;
            if (!m->frame_line[j]) continue;
            hr_launch_blend_rows(reinterpret_cast<const float*>(p.b), m->frame_line[j], row_floats, t.i0, t.i1, t.w0, t.w1, st);
            m->frame_row = 0;
        }
    }
    const int rc = render_impl(m, rays_dev, n_rays, rgb_dev, nullptr, maps, st);
    m->frame_row = -1;
    return rc;
}

int hr_render_frame(hr_model* m, const float* rays_dev, int64_t n_rays, float time, float* rgb_dev, void* stream)
{
    return hr_render_frame_maps(m, rays_dev, n_rays, time, rgb_dev, nullptr, stream);
}

int hr_stage_mlp(hr_model* m, const float* rays_dev, int64_t n_rays, void* stream)
{
    int rc = check_render(m, rays_dev, n_rays, rays_dev);
    if (rc != HR_OK) return rc;
    if (n_rays > m->chunk) return fail(HR_E_INVALID, "n_rays exceeds the reserved chunk (%lld)", (long long)m->chunk);
    launch_front(m, rays_dev, n_rays, (hipStream_t)stream);   // cascades: everything up to the fine head
    HR_HIP(hipGetLastError());
    return HR_OK;
}

int hr_stage_samples(hr_model* m, const float* rays_dev, int64_t n_rays, float* rgb_dev, void* stream)
{
    int rc = check_render(m, rays_dev, n_rays, rgb_dev);
    if (rc != HR_OK) return rc;
    if (n_rays > m->chunk) return fail(HR_E_INVALID, "n_rays exceeds the reserved chunk (%lld)", (long long)m->chunk);
    HrSampleArgs sa;
    fill_sample_args(m, sa, rays_dev, n_rays, rgb_dev);
    if (!launch_samples(m, sa, nullptr, 0, (hipStream_t)stream))    // (an MLP shading mode: export, colour network, import)
        return fail(HR_E_HIP, "the shading kernel's LDS request was refused");
    HR_HIP(hipGetLastError());
    return HR_OK;
}

int hr_stage_shade(hr_model* m, const float* feat_dev, const float* viewdirs_dev, int64_t n, float* rgb_dev, void* stream)
{
    if (!m) return fail(HR_E_INVALID, "null model");
    if (!m->finalized) return fail(HR_E_STATE, "hr_model_finalize has not been called");
    if (!hr_shading_is_mlp(m->cfg.shading)) return fail(HR_E_INVALID, "hr_stage_shade: the model's shading is not HR_SHADING_MLP_FEA / HR_SHADING_MLP");
    if (n < 0) return fail(HR_E_INVALID, "negative row count");
    if (n > 0 && (!feat_dev || !viewdirs_dev || !rgb_dev)) return fail(HR_E_INVALID, "null feature / view direction / rgb buffer");
    if (hr_shade_blocks(n) >= ((int64_t)1 << 31)) return fail(HR_E_INVALID, "hr_stage_shade: too many rows for one launch");
    HrShadeArgs ha;
    fill_shade_args(m, ha, feat_dev, HR_SHADE_FEAT, viewdirs_dev, 3, n, rgb_dev);
    if (!hr_launch_shade(ha, (hipStream_t)stream)) return fail(HR_E_HIP, "the shading kernel's LDS request was refused");
    HR_HIP(hipGetLastError());
    return HR_OK;
}

int hr_debug_trace_mlp(hr_model* m, const float* rays_dev, int64_t n_rays, unsigned long long* trace_dev, void* stream)
{
    int rc = check_render(m, rays_dev, n_rays, rays_dev);
    if (rc != HR_OK) return rc;
    if (n_rays > m->chunk) return fail(HR_E_INVALID, "n_rays exceeds the reserved chunk (%lld)", (long long)m->chunk);
    if (m->coarse) return fail(HR_E_INVALID, "hr_debug_trace_mlp does not support cascades");
    HrMlpArgs ma;
    fill_mlp_args(m, ma, rays_dev, n_rays);
    ma.trace = trace_dev;
    launch_mlp(m, m->kcfg, ma, (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}
