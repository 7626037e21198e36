// C ABI, the MLP's arithmetic.  The rules are hr_plan.h's ("MLP arithmetic": hr_mlp_choice, hr_calib_sample, hr_band_margins, hr_listed_frac,
// hr_verify_fallback); this file measures what they are asked about and packs what they answer.  Everything decided lives in ONE value,
// the model's HrMlpState (hr_model.h).  A new one is built aside -- build_mlp_state: activation range, arithmetic, tiles -- and
// set_mlp_state puts it in the model's place and measures the verified fast path's margins on it (calibrate_band, which builds its result
// aside as well); any error on the way leaves the model's state as it was (include/hyperreel_hip.h, hr_model_calibrate).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hr_model.h"

// fp8 image of hidden Linear l's output (f16 + fp8 split only): e4m3(x * 2^-Ea) with the calibration's largest |pre-activation| of that layer
// (act_max[l + 1]) times HR_F8_HEADROOM at or below 448 (hr_f8_exponent, hr_mlp_pack.h) -- beyond 448 * 2^Ea the image saturates and the
// kernels say so (HR_OPT_MLP_F8_SATURATED).  Depends on the calibration only, not on the packed weights: a calibration that keeps the
// arithmetic refreshes it without re-packing.
static void f8_exponents(const hr_config& c, HrMlpState& s)
{
    for (int l = 0; l < HR_MAX_LAYERS; ++l) {
        const bool hidden_f8 = s.active_precision == HR_MLP_F16F8 && l + 1 < c.mlp_layers;
        s.xexp[l] = hidden_f8 ? hr_f8_exponent(s.act_max[l + 1]) : 0;
    }
}

// One packing of the MLP's weights in `precision` -> t (layout, roundings and scalings: hr_mlp_pack.h)
static int pack_mlp_as(hr_model* m, const int precision, HrMlpTiles& t)
{
    const hr_config& c = m->cfg;
    char name[64];
    t.bytes = 0;
    HrPackedLayer pk;
    for (int l = 0; l < c.mlp_layers; ++l) {
        const HrMlpLayer g = mlp_layer(c, m->p_live, m->col_map, l, hr_pack_tile_n(precision));
        std::vector<float> w((size_t)g.N_user * g.Kt), b(g.N_user);
        snprintf(name, sizeof(name), "mlp.%d.weight", l);
        HR_HIP(hipMemcpy(w.data(), m->raw[name].p, w.size() * sizeof(float), hipMemcpyDeviceToHost));
        snprintf(name, sizeof(name), "mlp.%d.bias", l);
        HR_HIP(hipMemcpy(b.data(), m->raw[name].p, b.size() * sizeof(float), hipMemcpyDeviceToHost));
        hr_pack_mlp_layer(g, precision, w, b, pk);
        void* tiles = nullptr;
        if (precision == HR_MLP_FP32) { HR_HIP(t.wpack[l].alloc(pk.tiles.size())); tiles = t.wpack[l]; }
        else { HR_HIP(t.wsplit[l].alloc(pk.tiles.size())); tiles = t.wsplit[l]; }
        HR_HIP(hipMemcpy(tiles, pk.tiles.data(), pk.tiles.size(), hipMemcpyHostToDevice));
        HR_HIP(t.bias[l].alloc(pk.bias.size() * sizeof(float)));
        HR_HIP(hipMemcpy(t.bias[l], pk.bias.data(), pk.bias.size() * sizeof(float), hipMemcpyHostToDevice));
        t.winv[l] = pk.winv;
        t.n_tiles[l] = g.nt;
        t.bytes += (int64_t)(pk.tiles.size() + pk.bias.size() * sizeof(float));
    }
    return HR_OK;
}

// The one re-pack (install_mlp_state has the synchronise that goes with it): s gets fresh tiles for its arithmetic -- the primary ones
// and, verified fast path, the f16x3 and bf16x3 tiles of its later passes -- and the fp8 exponents that go with them.  The tiles s held
// (the model's own, while s is being built) are not touched.
static int pack_mlp(hr_model* m, HrMlpState& s)
{
    f8_exponents(m->cfg, s);
    const auto pk = std::make_shared<HrMlpPack>();
    const HrMlpLayer g = mlp_layer(m->cfg, m->p_live, m->col_map, 0, 16);
    pk->k0p = g.k0p;
    pk->n_out = g.n_out;
    int rc = pack_mlp_as(m, s.active_precision, pk->tiles[0]);
    if (rc != HR_OK) return rc;
    if (s.verified) {
        rc = pack_mlp_as(m, HR_MLP_F16X3, pk->tiles[1]);
        if (rc != HR_OK) return rc;
        rc = pack_mlp_as(m, HR_MLP_BF16X3, pk->tiles[2]);
        if (rc != HR_OK) return rc;
        if (!m->redo_count) HR_HIP(m->redo_count.alloc(4 * sizeof(unsigned)));
        HR_HIP(hipMemset(m->redo_count, 0, 4 * sizeof(unsigned)));
        // the margins of the decisions at risk (HrRisk): here their floor; the model's own are measured by calibrate_band once the workspace exists
        s.band = {HR_BAND_FLOOR, HR_BAND_FLOOR, 0.0f};
        s.band_stale = true;
    }
    pk->bytes = pk->tiles[0].bytes + pk->tiles[1].bytes + pk->tiles[2].bytes;
    s.pack = pk;
    return HR_OK;
}

// Activation range of the MLP on `rays_dev` (NULL: 4096 synthetic rays -- origins uniform in the scene box, unit directions,
// times in [0, 1)) -> s.act_max; the rays stay with s (the caller's: hr_calib_sample of them) for the band of the verified fast path
static int measure_range(hr_model* m, const float* rays_dev, int64_t n, hipStream_t st, HrMlpState& s)
{
    const hr_config& c = m->cfg;
    const auto kept = std::make_shared<HrCalibRays>();
    DevMem<float> d_max;
    hipError_t e = hipSuccess;
    const int rd = m->coarse ? c.casc_row_dim : c.ray_dim;
    const bool synthetic = !rays_dev;
    if (rays_dev) {
        const HrCalibSample k = hr_calib_sample(n);
        e = kept->p.alloc(sizeof(float) * k.keep * rd);
        if (e == hipSuccess) e = hipMemcpy2DAsync(kept->p, sizeof(float) * rd, rays_dev, sizeof(float) * rd * k.stride, sizeof(float) * rd, k.keep,
                                                  hipMemcpyDeviceToDevice, st);
        kept->n = k.keep;
    } else {
        n = kept->n = 4096;
        e = kept->p.alloc(sizeof(float) * n * rd);
        if (e == hipSuccess) {
            // where rays start: the model's own box, or (cascade rows, whose first columns are points) the same box.  Real cameras may stand
            // outside it, and a parameterisation such as the Pluecker moment o x d grows with |o|: a caller who has the real rays passes
            // them (hr_model_calibrate), and the host checks the kernels' sticky overflow bit on the first rendered batches and
            // falls back to bf16x3 (models.py, _overflow_guard).  (Origins in a box three times as large were tried for this default: with
            // uniformly random directions the two-plane families then show activations of 1.8e4 that no camera of theirs produces,
            // and AUTO would give up f16x3 -- and its zero flipped rays, DESIGN 3a -- on every one of them.)
            hr_launch_synthetic_rays(kept->p, n, rd, c.aabb, c.aabb + 3, 0x5eedu, st);
            rays_dev = kept->p;
        }
    }
    if (e == hipSuccess) e = d_max.alloc(sizeof(float) * HR_MAX_LAYERS);
    if (e == hipSuccess) e = hipMemsetAsync(d_max, 0, sizeof(float) * HR_MAX_LAYERS, st);
    if (e == hipSuccess) {
        HrRangeArgs ra;
        ra.rays = rays_dev;
        ra.n_rays = n;
        ra.act_max = d_max;
        char name[64];
        for (int l = 0; l < HR_MAX_LAYERS; ++l) {
            ra.w[l] = ra.b[l] = nullptr;
            if (l < c.mlp_layers) {
                snprintf(name, sizeof(name), "mlp.%d.weight", l);
                ra.w[l] = m->raw[name].p;
                snprintf(name, sizeof(name), "mlp.%d.bias", l);
                ra.b[l] = m->raw[name].p;
            }
        }
        hr_config kc = m->kcfg;
        if (m->coarse) kc.ray_dim = c.casc_row_dim;              // the point MLP's "rays" are the rows (launch_cascade_front)
        hr_launch_mlp_range(kc, ra, st);
        e = hipMemcpyAsync(s.act_max, d_max, sizeof(float) * HR_MAX_LAYERS, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(HR_E_HIP, "activation-range calibration: %s", hipGetErrorString(e)); }
    s.calibrated = synthetic ? 1 : 2;
    s.calib = kept;
    return HR_OK;
}

// A new state for the model in s, built aside: the activation range on `rays_dev` (measure_range) where hr_mlp_choice asks for it, the
// arithmetic it then names, and the tiles -- the model's own when keep_tiles is set and the arithmetic is the one it runs (then only the
// fp8 exponents follow the new range), freshly packed otherwise.  The model is read, not written.
int build_mlp_state(hr_model* m, const float* rays_dev, int64_t n, hipStream_t st, bool keep_tiles, HrMlpState& s)
{
    const hr_config& c = m->cfg;
    const HrMlpState& cur = m->mlp;
    s = HrMlpState();
    s.band = cur.band;
    s.vinfo.fallback = cur.vinfo.fallback;       // (calibrate_band keeps the reason while the fast path stays off)
    const bool level = m->coarse || m->is_coarse, supported = hr_mlp_range_supported(c);
    const HrSampleKind kind = hr_model_sample_kind(m);
    HrMlpChoice ch = hr_mlp_choice(c, kind, level, supported, s.act_max);
    if (ch.status == HR_OK && ch.needs_calibration) {
        const int rc = measure_range(m, rays_dev, n, st, s);
        if (rc != HR_OK) return rc;
        ch = hr_mlp_choice(c, kind, level, supported, s.act_max);
    }
    if (ch.status == HR_E_RANGE) {
        const int want = c.mlp_precision;
        float mx = 0.0f;
        for (int l = 0; l < c.mlp_layers; ++l) mx = fmaxf(mx, s.act_max[l]);
        return fail(HR_E_RANGE, "mlp_precision %s was requested, but the MLP's activations reach %.4g on the calibration rays (limit %.4g = "
                    "65504 / 8): IEEE-half operands would overflow.  Use HR_MLP_AUTO (falls back to bf16x3) or HR_MLP_BF16X3",
                    want == HR_MLP_F16X3 ? "f16x3" : (want == HR_MLP_F16X2 ? "f16x2" : "f16f8"), (double)mx, (double)HR_F16_CALIBRATION_LIMIT);
    }
    if (ch.status != HR_OK && !supported)
        return fail(HR_E_INVALID, "activation-range calibration does not cover mlp_in %d / mlp_hidden %d", c.mlp_in, c.mlp_hidden);
    if (ch.status != HR_OK)
        return fail(HR_E_INVALID, "mlp_precision f16f8v (verified) needs a plain ray MLP of width 256, at most 64 samples per ray and an intersection "
                    "the margins are derived for (axis planes, sphere / cylinder with fixed origins, euclidean; not DoNeRFContract)");
    s.active_precision = ch.active_precision;
    s.verified = ch.verified;
    if (!keep_tiles || !cur.pack || s.active_precision != cur.active_precision || s.verified != cur.verified) return pack_mlp(m, s);
    f8_exponents(c, s);
    s.pack = cur.pack;
    s.band_stale = true;
    return HR_OK;
}

// The one place a state reaches the model.  Fresh tiles: the device is first synchronised -- their upload, and whatever was launched
// before, is done.  s holds the state before afterwards.
static int install_mlp_state(hr_model* m, HrMlpState& s)
{
    if (s.pack != m->mlp.pack) HR_HIP(hipDeviceSynchronize());
    std::swap(m->mlp, s);
    return HR_OK;
}

// A state built aside goes in, and its margins are measured on it (the launch helpers read the model's state); an error puts the state
// before back whole.
int set_mlp_state(hr_model* m, HrMlpState& s, hipStream_t st)
{
    int rc = install_mlp_state(m, s);
    if (rc != HR_OK) return rc;
    rc = calibrate_band(m, st);
    if (rc != HR_OK) std::swap(m->mlp, s);
    return rc;
}

int hr_model_calibrate(hr_model* m, const float* rays_dev, int64_t n_rays, float* act_max, void* stream)
{
    if (!m) return fail(HR_E_INVALID, "null model");
    if (!m->finalized) return fail(HR_E_STATE, "hr_model_calibrate before hr_model_finalize");
    if (m->coarse || m->is_coarse) return fail(HR_E_INVALID, "hr_model_calibrate: cascades are calibrated by hr_model_finalize (the point MLP's rows are internal)");
    if (!rays_dev || n_rays <= 0) return fail(HR_E_INVALID, "hr_model_calibrate needs rays");
    HrMlpState s;
    int rc = build_mlp_state(m, rays_dev, n_rays, (hipStream_t)stream, true, s);
    if (rc != HR_OK) return rc;
    HR_HIP(hipMemset(m->flags, 0, sizeof(unsigned)));
    rc = set_mlp_state(m, s, (hipStream_t)stream);
    if (rc == HR_OK && act_max)
        for (int l = 0; l < m->cfg.mlp_layers; ++l) act_max[l] = m->mlp.act_max[l];
    return rc;
}

// The margins of the verified fast path for THIS model: both arithmetics' heads on the calibration rays, pushed through the
// model's own activations, anchors, contraction and intersection by the probe kernel (band_kernel.hip) in the normalisation the sample
// stage's per-sample margins use (hr_math.h, HrRisk); margin = 4 x the largest difference, never below HR_BAND_FLOOR.  Then the
// well-conditioned calibration rays once through the verified path and once through the f16x3 tiles: the fraction listed, and how far the
// two images are apart.  HR_MLP_AUTO gives the fast path up (hr_verify_fallback: f16x3 throughout, one more re-pack).  Synchronises `st`.
// The result is built in a copy of the model's state and replaces it at the end (install_mlp_state): an error leaves margins,
// hr_verify_info and band_stale as they were, and the next render measures again.
int calibrate_band(hr_model* m, hipStream_t st)
{
    HrMlpState s = m->mlp;          // (the launch helpers below read m->mlp's tiles, arithmetic and fp8 exponents: s keeps those equal to it until the fallback, which launches nothing)
    hr_verify_info& vi = s.vinfo;
    const int fallback_before = vi.fallback;
    vi = hr_verify_info();
    vi.verified = s.verified;
    vi.band_floor = HR_BAND_FLOOR;
    vi.fallback = (fallback_before && !s.verified) ? fallback_before : 0;
    s.band_stale = false;
    if (!s.verified || m->coarse || m->is_coarse) return install_mlp_state(m, s);
    if (!s.calib || s.calib->n <= 0 || !m->head) return fail(HR_E_STATE, "verified fast path without calibration rays / workspace");
    {   // (the temporaries are freed before a fallback re-packs)
        const hr_config& c = m->cfg;
        const int Z = c.z_channels, P = c.preds_per_z;
        const int64_t N = s.calib->n, nc_max = N < m->chunk ? N : m->chunk;
        DevMem<float> ha, hb, rgb, rgb2, sel;
        DevMem<unsigned> stats;
        DevMem<unsigned char> ok_dev;
        DevMem<hr_config> pcfg;
        HR_HIP(ha.alloc(sizeof(float) * nc_max * Z * P));
        HR_HIP(hb.alloc(sizeof(float) * nc_max * Z * P));
        HR_HIP(stats.alloc(sizeof(unsigned) * HR_BAND_WORDS));
        HR_HIP(ok_dev.alloc((size_t)N));
        HR_HIP(pcfg.alloc(sizeof(hr_config)));
        HR_HIP(hipMemsetAsync(stats, 0, sizeof(unsigned) * HR_BAND_WORDS, st));
        HR_HIP(hipMemsetAsync(ok_dev, 1, (size_t)N, st));
        hr_config probe_cfg = c;                       // user column order; the probe applies the near / far mask itself
        probe_cfg.isect_mask_off = 1;
        HR_HIP(hipMemcpyAsync(pcfg, &probe_cfg, sizeof(hr_config), hipMemcpyHostToDevice, st));
        HR_HIP(hipStreamSynchronize(st));          // (probe_cfg is a local)
        for (int64_t r0 = 0; r0 < N; r0 += nc_max) {
            const int64_t n = (N - r0 < nc_max) ? (N - r0) : nc_max;
            const float* rays = s.calib->p + r0 * c.ray_dim;
            for (int tier = 0; tier < 2; ++tier) {
                HrMlpArgs ma;
                fill_mlp_args(m, ma, rays, n, tier);
                launch_mlp(m, m->kcfg, ma, st, tier);
                hr_launch_head_export(m->head, tier == 0 ? ha : hb, n, Z, P, m->p_live, (s.pack->n_out + 3) / 4, rows_per_ray(c), m->col_map, st);
            }
            HrBandArgs ba;
            ba.cfg_dev = pcfg;
            ba.rays = rays;
            ba.head_a = ha;
            ba.head_b = hb;
            ba.n_rays = n;
            ba.mask_on = c.isect_mask_off ? 0 : 1;
            ba.flip_cut = 1e-3f;
            ba.stats = stats;
            ba.ray_ok = ok_dev + r0;
            ba.amp_cut = HR_VERIFY_AMP_CUT;
            ba.phase = 0;                              // which rays are well conditioned ...
            hr_launch_band_probe(ba, Z, st);
            ba.phase = 1;                              // ... and the statistics over those
            hr_launch_band_probe(ba, Z, st);
        }
        unsigned hs[HR_BAND_WORDS];
        std::vector<unsigned char> ok((size_t)N);
        std::vector<float> rays_h((size_t)N * c.ray_dim);
        HR_HIP(hipMemcpyAsync(hs, stats, sizeof(hs), hipMemcpyDeviceToHost, st));
        HR_HIP(hipMemcpyAsync(ok.data(), ok_dev, (size_t)N, hipMemcpyDeviceToHost, st));
        HR_HIP(hipMemcpyAsync(rays_h.data(), s.calib->p, sizeof(float) * rays_h.size(), hipMemcpyDeviceToHost, st));
        HR_HIP(hipStreamSynchronize(st));
        auto f = [&](int i) { float v; memcpy(&v, &hs[i], sizeof(v)); return v; };
        vi.max_d_zc = f(HR_BAND_ZC);
        vi.max_d_dist_n = f(HR_BAND_DIST_N);
        vi.max_d_geo_n = f(HR_BAND_GEO_N);
        vi.max_d_off = f(HR_BAND_OFF);
        vi.max_d_dist = f(HR_BAND_DIST);
        for (int i = 0; i < 64; ++i) vi.max_d_head = fmaxf(vi.max_d_head, f(HR_BAND_HEAD0 + i));
        vi.n_rays = N;
        vi.n_samples = hs[HR_BAND_COUNTED];
        vi.n_flipped = hs[HR_BAND_FLIPPED];
        vi.n_shaky = hs[HR_BAND_SHAKY];
        s.band = hr_band_margins(vi.max_d_zc, vi.max_d_dist_n, vi.max_d_geo_n, vi.max_d_off);
        vi.band = s.band.band;
        vi.band_q = s.band.band_q;
        vi.band_off = s.band.band_off;
        // the well-conditioned rays, compacted on the host (<= 65 536 rays: not worth a kernel)
        int64_t nu = 0;
        for (int64_t i = 0; i < N; ++i)
            if (ok[(size_t)i]) {
                if (nu != i) memcpy(&rays_h[(size_t)nu * c.ray_dim], &rays_h[(size_t)i * c.ray_dim], sizeof(float) * c.ray_dim);
                ++nu;
            }
        vi.n_rays_used = nu;
        // (fewer than 64 well-conditioned rays -- a caller calibrating on a handful: the margins stand, there is no image to judge by)
        unsigned listed = 0;
        if (nu >= 64) {
            // through the verified path as a render call takes it, and through the f16x3 tiles throughout: what fraction the first pass lists with
            // these margins, and how far the two IMAGES are apart -- f16f8's continuous error (every pixel that is not listed keeps it) grows with
            // the weights like the margins do, and no margin repairs it
            HR_HIP(sel.alloc(sizeof(float) * nu * c.ray_dim));
            HR_HIP(rgb.alloc(sizeof(float) * nu * 3));
            HR_HIP(rgb2.alloc(sizeof(float) * nu * 3));
            HR_HIP(hipMemcpyAsync(sel, rays_h.data(), sizeof(float) * nu * c.ray_dim, hipMemcpyHostToDevice, st));
            HR_HIP(hipMemsetAsync(m->redo_count, 0, 4 * sizeof(unsigned), st));
            render_verified(m, s.band, sel, nu, rgb, hr_redo_list_cap(nu, m->redo_cap), st);
            HR_HIP(hipMemcpyAsync(&listed, m->redo_count + 1, sizeof(unsigned), hipMemcpyDeviceToHost, st));
            for (int64_t r0 = 0; r0 < nu; r0 += m->chunk) {
                const int64_t n = (nu - r0 < m->chunk) ? (nu - r0) : m->chunk;
                const float* rays = sel + r0 * c.ray_dim;
                launch_front(m, rays, n, st, 1);
                HrSampleArgs sa;
                fill_sample_args(m, sa, rays, n, rgb2 + r0 * 3);
                hr_launch_samples(m->kcfg, sa, st);
            }
            std::vector<float> ia((size_t)nu * 3), ib((size_t)nu * 3);
            HR_HIP(hipMemcpyAsync(ia.data(), rgb, sizeof(float) * ia.size(), hipMemcpyDeviceToHost, st));
            HR_HIP(hipMemcpyAsync(ib.data(), rgb2, sizeof(float) * ib.size(), hipMemcpyDeviceToHost, st));
            HR_HIP(hipStreamSynchronize(st));
            for (size_t i = 0; i < ia.size(); ++i) {
                const float d = fabsf(ia[i] - ib[i]);
                vi.max_d_rgb = (d > vi.max_d_rgb || d != d) ? d : vi.max_d_rgb;
            }
        }
        vi.listed_frac = hr_listed_frac(s.calibrated, N, nu, listed);
        HR_HIP(hipMemsetAsync(m->redo_count, 0, 4 * sizeof(unsigned), st));
        HR_HIP(hipMemsetAsync(m->flags, 0, sizeof(unsigned), st));        // range bits the calibration rays raised are not the caller's
        HR_HIP(hipStreamSynchronize(st));
    }
    const int fallback = m->cfg.mlp_precision == HR_MLP_AUTO ? hr_verify_fallback(vi.listed_frac, vi.max_d_rgb) : 0;
    if (fallback) {
        s.verified = vi.verified = 0;
        s.active_precision = HR_MLP_F16X3;
        vi.fallback = fallback;
        const int rc = pack_mlp(m, s);
        if (rc != HR_OK) return rc;
    }
    return install_mlp_state(m, s);
}

int hr_model_verify_info(hr_model* m, hr_verify_info* out)
{
    if (!m || !out) return fail(HR_E_INVALID, "null argument");
    if (!m->finalized) return fail(HR_E_STATE, "hr_model_finalize has not been called");
    *out = m->mlp.vinfo;
    out->verified = m->mlp.verified;
    return HR_OK;
}
