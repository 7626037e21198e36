// TEST-ONLY host build of hyperreel_amd/csrc/hr_plan.h (plane-pair geometry, plane class, the render call's and the training step's
// launch plans, the MLP's arithmetic), so that the suites ask the library's own code which branch a case takes.  Nothing in the product links or loads this file.
#include "../../hyperreel_amd/csrc/hr_plan.h"
#include "../../hyperreel_amd/csrc/hr_train.h"

extern "C" {

int hp_sizeof_plane() { return (int)sizeof(HrGridPlane); }
int hp_sizeof_plan() { return (int)sizeof(HrTrainPlan); }
int hp_sizeof_sample_plan() { return (int)sizeof(HrSamplePlan); }
int hp_sizeof_sample_form_plan() { return (int)sizeof(HrSampleFormPlan); }
int hp_sizeof_frame_plan() { return (int)sizeof(HrFramePlan); }
int hp_sizeof_time_tap() { return (int)sizeof(HrTimeTap); }
int hp_round_zp(int z_channels) { return hr_round_zp(z_channels); }

int hp_plane_geometry(const hr_config* c, HrGridPlane* out, int* ca_total, int* n_basis_cols)
{
    return hr_plane_geometry(*c, out, ca_total, n_basis_cols) ? 1 : 0;
}

// train: the size predicate of the training step's class path instead of the render gathers'
int hp_plane_class(const HrGridPlane* planes, int ca_total, int train)
{
    return train ? hr_plane_class(planes, ca_total, hr_plane_fits_train) : hr_plane_class(planes, ca_total, hr_plane_fits_gather);
}

// The plan of hr_train_backward for n_rays rays of a finalized model of *c: a backward step whose tape has taps, point gradient
// and grouped order (the workspace provides them), float or 64-bit fixed-point accumulators.  256 compute units: no branch depends
// on the count, only grid sizes do.
void hp_train_plan(const hr_config* c, long long n_rays, int deterministic, HrTrainPlan* out)
{
    HrGridPlane planes[3];
    int ca_total = 0, n_basis_cols = 0;
    (void)hr_plane_geometry(*c, planes, &ca_total, &n_basis_cols);
    const HrTrainPlanIn in = {n_rays, true, true, true, true, deterministic != 0, deterministic ? sizeof(long long) : sizeof(float), 256};
    *out = hr_train_plan(*c, planes, ca_total, n_basis_cols, in);
}

// The training tape bound to `base` for ns samples: byte offsets of the nine fields from base in HrTrainTape's order {ds, src, dfeat, dpre,
// ddc, dts, taps, dp, perm} (-1: not bound); rows: the coarse level's three-plane form.  Returns the words per sample of the full form.
int hp_tape_layout(float* base, long long ns, int rows, long long* off)
{
    const HrTrainTape t = rows ? hr_tape_bind_rows(base, ns) : hr_tape_bind(base, ns);
    const void* f[9] = {t.ds, t.src, t.dfeat, t.dpre, t.ddc, t.dts, t.taps, t.dp, t.perm};
    for (int i = 0; i < 9; ++i) off[i] = f[i] ? (long long)((const char*)f[i] - (const char*)base) : -1;
    return HR_TAPE_WORDS;
}

// hr_grad_pool of a model of *c: out = {off_a[3], off_b[3], n_a[3], n_b[3], total} in elements
void hp_grad_pool(const hr_config* c, size_t elem, size_t align, size_t* out)
{
    HrGridPlane planes[3];
    int ca_total = 0, n_basis_cols = 0;
    (void)hr_plane_geometry(*c, planes, &ca_total, &n_basis_cols);
    const HrGradPool p = hr_grad_pool(planes, elem, align);
    for (int j = 0; j < 3; ++j) { out[j] = p.off_a[j]; out[3 + j] = p.off_b[j]; out[6 + j] = p.n_a[j]; out[9 + j] = p.n_b[j]; }
    out[12] = p.total;
}

// ---- rendering
void hp_live_columns(const hr_config* c, int prune, int* col, int* p_live, hr_config* kcfg) { hr_live_columns(*c, prune != 0, col, p_live, kcfg); }
long long hp_default_chunk(long long nq, int rows) { return hr_default_chunk(nq, rows); }
long long hp_even_chunk(long long chunk, long long n) { return hr_even_chunk(chunk, n); }
int hp_redo_list_cap(long long n, int buffer_cap) { return hr_redo_list_cap(n, buffer_cap); }
int hp_wide_cap(long long chunk) { return hr_wide_cap(chunk); }
size_t hp_sample_lds_bytes(int nq, int ca_total, int zp, int rows) { return hr_sample_lds_bytes(nq, ca_total, zp, rows); }
void hp_frame_time_tap(const hr_config* c, float time, HrTimeTap* out) { *out = hr_frame_time_tap(*c, time); }

// What a model of *c (a level of a cascade: its own config) is rendered with: live columns with pruning on, the geometry of
// hr_model_finalize; frame_lines: inside hr_render_frame, where a float32 keyframe net's time planes are handed over as lines
// (render_plane, api_render.hip)
struct Level {
    int p_live, nq, ca_total;
    HrGridPlane planes[3];
};
static Level level_of(const hr_config& c, int frame_lines)
{
    Level v;
    int col[64], n_basis_cols = 0;
    hr_config kcfg;
    hr_live_columns(c, true, col, &v.p_live, &kcfg);
    v.nq = hr_head_quads(c, v.p_live);
    (void)hr_plane_geometry(c, v.planes, &v.ca_total, &n_basis_cols);
    if (frame_lines && c.video && c.num_keyframes >= 2 && c.grid_dtype != HR_GRID_FP16)
        for (HrGridPlane& g : v.planes)
            if (g.bw > 1 && g.cd4 + g.ca4 > 0) { g.bh = g.bw; g.bw = 1; }
    return v;
}

int hp_sample_kind(int shading, int time_density) { return hr_sample_kind(shading, time_density != 0); }

// 1: hr_model_create refuses the level for the sample kernel's LDS; *bytes: the kernel's request
int hp_sample_lds_refused(const hr_config* c, size_t* bytes)
{
    return hr_sample_lds_refused(*c, level_of(*c, 0).p_live, bytes) ? 1 : 0;
}

// the plan of a launch of form (kind, maps, exported) and the instantiation <ZP, HALF, PC, NB> hr_sample_dispatch names for it
void hp_sample_form_plan(const hr_config* c, long long n_rays, int frame_lines, int kind, int maps, int exported, HrSampleFormPlan* out, int* inst)
{
    const Level v = level_of(*c, frame_lines);
    *out = hr_sample_form_plan(*c, v.planes, v.ca_total, v.nq, rows_per_ray(*c), n_rays, false, HrSampleForm{(HrSampleKind)kind, maps != 0, exported != 0});
    hr_sample_dispatch(*out, c->grid_dtype == HR_GRID_FP16, [&](auto zp, auto half, auto pc, auto nb) {
        inst[0] = decltype(zp)::value; inst[1] = decltype(half)::value; inst[2] = decltype(pc)::value; inst[3] = decltype(nb)::value;
    });
}

// hr_render_route: out = {route, tier, calibrate_first}
void hp_render_route(long long n_rays, int fields, int maps, int kind, int mlp_verified, int occupancy, int band_stale, int capturing, int frame_fits, int* out)
{
    const HrRenderRoute r = hr_render_route(HrRouteIn{n_rays, fields != 0, maps != 0, (HrSampleKind)kind, mlp_verified != 0, occupancy != 0, band_stale != 0,
                                                      capturing != 0, frame_fits != 0});
    out[0] = r.route; out[1] = r.tier; out[2] = r.calibrate_first;
}

// hr_sample_plan as the launcher calls it
void hp_sample_plan_raw(const hr_config* c, const HrGridPlane* planes, int ca_total, int nq, int rows, long long n_rays, int rows_emitted, HrSamplePlan* out)
{
    *out = hr_sample_plan(*c, planes, ca_total, nq, rows, n_rays, rows_emitted != 0);
}

// the stand-alone sample kernel's plan and the instantiation <ZP, HALF, PC, NB> hr_sample_dispatch picks for it
void hp_sample_plan(const hr_config* c, long long n_rays, int rows_emitted, int frame_lines, HrSamplePlan* out, int* inst)
{
    const Level v = level_of(*c, frame_lines);
    *out = hr_sample_plan(*c, v.planes, v.ca_total, v.nq, rows_per_ray(*c), n_rays, rows_emitted != 0);
    hr_sample_dispatch(*out, c->grid_dtype == HR_GRID_FP16, [&](auto zp, auto half, auto pc, auto nb) {
        inst[0] = decltype(zp)::value; inst[1] = decltype(half)::value; inst[2] = decltype(pc)::value; inst[3] = decltype(nb)::value;
    });
}

// the frame kernel's plan on a device of 256 compute units, 16-bit split elements, the split kernels' 32-column output tiles
void hp_frame_plan(const hr_config* c, long long n_rays, int frame_mode, int sample_waves, int cascade, int verified, int split_mlp, int frame_lines,
                   HrFramePlan* out)
{
    const Level v = level_of(*c, frame_lines);
    HrFramePlanIn in = HrFramePlanIn();
    in.n_rays = n_rays;
    in.frame_mode = frame_mode;
    in.sample_waves = sample_waves;
    in.cascade = cascade != 0;
    in.verified = verified != 0;
    in.split_mlp = split_mlp != 0;
    in.split_elem = 2;
    in.nq = v.nq;
    in.k0p = (c->mlp_in + 15) & ~15;
    in.last_tiles = (samples_per_row(*c) * v.p_live + 31) / 32;
    in.cus = 256;
    *out = hr_frame_plan(*c, v.planes, v.ca_total, in);
}

// ---- MLP arithmetic
// out = {active_precision, verified, needs_calibration, status}
void hp_mlp_choice(const hr_config* c, int cascade_level, int range_supported, const float* act_max, int* out)
{
    const HrMlpChoice ch = hr_mlp_choice(*c, cascade_level != 0, range_supported != 0, act_max);
    out[0] = ch.active_precision; out[1] = ch.verified; out[2] = ch.needs_calibration ? 1 : 0; out[3] = ch.status;
}
// out = {HR_F16_CALIBRATION_LIMIT, HR_BAND_FLOOR, HR_VERIFY_LISTED_LIMIT, HR_VERIFY_RGB_LIMIT}
void hp_mlp_limits(float* out) { out[0] = HR_F16_CALIBRATION_LIMIT; out[1] = HR_BAND_FLOOR; out[2] = HR_VERIFY_LISTED_LIMIT; out[3] = HR_VERIFY_RGB_LIMIT; }
void hp_calib_sample(long long n, long long* out)
{
    const HrCalibSample k = hr_calib_sample(n);
    out[0] = k.stride; out[1] = k.keep;
}
void hp_band_margins(float d_zc, float d_dist_n, float d_geo_n, float d_off, float* out)
{
    const HrBand b = hr_band_margins(d_zc, d_dist_n, d_geo_n, d_off);
    out[0] = b.band; out[1] = b.band_q; out[2] = b.band_off;
}
float hp_listed_frac(int calibrated, long long N, long long n_used, unsigned listed) { return hr_listed_frac(calibrated, N, n_used, listed); }
int hp_verify_fallback(float listed_frac, float max_d_rgb) { return hr_verify_fallback(listed_frac, max_d_rgb); }

}  // extern "C"
