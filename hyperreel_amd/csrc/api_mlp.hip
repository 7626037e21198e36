// C ABI, the MLP's arithmetic: weight packing for the active precision, the activation-range calibration that resolves it, and the margins
// of the verified fast path (calibrate_band).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hr_model.h"

// fp8 image of hidden Linear l's output (f16 + fp8 split only): e4m3(x * 2^-Ea) with the calibration's largest |pre-activation| of that layer
// (act_max[l + 1]) times HR_F8_HEADROOM at or below 448 (hr_f8_exponent, hr_mlp_pack.h) -- beyond 448 * 2^Ea the image saturates and the
// kernels say so (HR_OPT_MLP_F8_SATURATED).  Depends on the calibration only, not on the packed weights: hr_model_calibrate refreshes it
// without re-packing.
static void f8_exponents(hr_model* m)
{
    for (int l = 0; l < HR_MAX_LAYERS; ++l) {
        const bool hidden_f8 = m->active_precision == HR_MLP_F16F8 && l + 1 < m->cfg.mlp_layers;
        m->xexp[l] = hidden_f8 ? hr_f8_exponent(m->act_max[l + 1]) : 0;
    }
}

// One packing of the MLP's weights in `precision` -> t (layout, roundings and scalings: hr_mlp_pack.h).  Called by hr_model_finalize
// and again by hr_model_calibrate when the calibration changes the active arithmetic.
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
        t.wpack[l].reset();
        t.wsplit[l].reset();
        t.bias[l].reset();
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

static const float HR_BAND_FLOOR = 1e-6f;
static const float HR_VERIFY_LISTED_LIMIT = 0.05f; // fraction of the calibration rays the first pass may list (a call's list holds a sixteenth of its rays)
static const float HR_VERIFY_RGB_LIMIT = 6e-5f;   // on <= 65 536 calibration rays; the shipped families measure 1.5e-5 - 5e-5 here and 2.3e-5 - 5.4e-5 on their 640 000-ray frames

// the primary tiles in the active arithmetic, and -- verified fast path -- the f16x3 and bf16x3 tiles of its later passes
int pack_mlp(hr_model* m)
{
    f8_exponents(m);
    const HrMlpLayer g = mlp_layer(m->cfg, m->p_live, m->col_map, 0, 16);
    m->k0p = g.k0p;
    m->n_out = g.n_out;
    int rc = pack_mlp_as(m, m->active_precision, m->tiles[0]);
    if (rc != HR_OK) return rc;
    m->tiles[1] = HrMlpTiles();
    m->tiles[2] = HrMlpTiles();
    if (m->verified) {
        rc = pack_mlp_as(m, HR_MLP_F16X3, m->tiles[1]);
        if (rc != HR_OK) return rc;
        rc = pack_mlp_as(m, HR_MLP_BF16X3, m->tiles[2]);
        if (rc != HR_OK) return rc;
        if (!m->redo_count) HR_HIP(m->redo_count.alloc(4 * sizeof(unsigned)));
        HR_HIP(hipMemset(m->redo_count, 0, 4 * sizeof(unsigned)));
        // the margins of the decisions at risk (HrRisk): here their floor -- four float32 ulps of the largest |zc|; the model's own are measured
        // by calibrate_band once the workspace exists
        m->redo_band = m->redo_band_q = HR_BAND_FLOOR;
        m->redo_band_off = 0.0f;
        m->band_stale = true;
    }
    m->mlp_bytes = m->tiles[0].bytes + m->tiles[1].bytes + m->tiles[2].bytes;
    return HR_OK;
}

// largest activation a model may show in calibration for the fp16 split arithmetic to be used: a factor 8 below the IEEE-half maximum,
// because calibration sees 4096 rays and a frame has 640 000
static const float HR_F16_CALIBRATION_LIMIT = 65504.0f / 8.0f;

// Activation range of the MLP on `rays_dev` (NULL: 4096 synthetic rays -- origins uniform in the scene box, unit directions,
// times in [0, 1)) -> m->act_max, then the arithmetic: HR_MLP_AUTO becomes f16x3 when every input feature and hidden activation
// stays below HR_F16_CALIBRATION_LIMIT and bf16x3 (fp32 exponent range) otherwise; a FORCED fp16 mode that fails the test is an error.
int resolve_precision(hr_model* m, const float* rays_dev, int64_t n, hipStream_t st)
{
    const hr_config& c = m->cfg;
    const int want = c.mlp_precision;
    for (int l = 0; l < HR_MAX_LAYERS; ++l) m->act_max[l] = 0.0f;
    m->calibrated = 0;
    m->verified = 0;
    if (c.mlp_layers == 0 || want == HR_MLP_FP32 || want == HR_MLP_BF16X3) {
        m->active_precision = (c.mlp_layers == 0 && want == HR_MLP_AUTO) ? HR_MLP_F16X3 : want;
        return HR_OK;
    }
    if (want == HR_MLP_AUTO && c.mlp_hidden != 256) {        // the split kernels are written for 256-wide layers
        m->active_precision = HR_MLP_FP32;
        return HR_OK;
    }
    if (!hr_mlp_range_supported(c))
        return fail(HR_E_INVALID, "activation-range calibration does not cover mlp_in %d / mlp_hidden %d", c.mlp_in, c.mlp_hidden);
    DevMem<float> synth, d_max;
    hipError_t e = hipSuccess;
    const int rd = m->coarse ? c.casc_row_dim : c.ray_dim;
    if (rays_dev) {
        // the caller's rays: a strided sample of at most 65 536 of them stays with the model (the band of the verified fast path is measured
        // on it, again after hr_model_update_config)
        const int64_t stride = (n + 65535) / 65536, keep = (n + stride - 1) / stride;
        m->calib_rays.reset();
        m->calib_n = 0;
        e = m->calib_rays.alloc(sizeof(float) * keep * rd);
        if (e == hipSuccess) e = hipMemcpy2DAsync(m->calib_rays, sizeof(float) * rd, rays_dev, sizeof(float) * rd * stride, sizeof(float) * rd, keep,
                                                  hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) m->calib_n = keep;
    }
    if (!rays_dev) {
        n = 4096;
        e = synth.alloc(sizeof(float) * n * rd);
        if (e == hipSuccess) {
            // where rays start: the model's own box, or (cascade rows, whose first columns are points) the same box.  Real cameras may stand
            // outside it, and a parameterisation such as the Pluecker moment o x d grows with |o|: a caller who has the real rays passes
            // them (hr_model_calibrate), and the host checks the kernels' sticky overflow bit on the first rendered batches and
            // falls back to bf16x3 (models.py, _overflow_guard).  (Origins in a box three times as large were tried for this default: with
            // uniformly random directions the two-plane families then show activations of 1.8e4 that no camera of theirs produces,
            // and AUTO would give up f16x3 -- and its zero flipped rays, DESIGN 3a -- on every one of them.)
            hr_launch_synthetic_rays(synth, n, rd, c.aabb, c.aabb + 3, 0x5eedu, st);
            rays_dev = synth;
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
        e = hipMemcpyAsync(m->act_max, d_max, sizeof(float) * HR_MAX_LAYERS, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    d_max.reset();
    const bool synthetic = synth;
    if (synth && e == hipSuccess) {            // kept (see above)
        m->calib_rays = std::move(synth);
        m->calib_n = n;
    } else synth.reset();
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(HR_E_HIP, "activation-range calibration: %s", hipGetErrorString(e)); }
    m->calibrated = synthetic ? 1 : 2;
    float mx = 0.0f;
    bool finite = true;
    for (int l = 0; l < c.mlp_layers; ++l) {
        if (!std::isfinite(m->act_max[l])) finite = false;
        mx = fmaxf(mx, m->act_max[l]);
    }
    const bool fits = finite && mx < HR_F16_CALIBRATION_LIMIT;
    // the verified fast path: f16f8 + a list-driven second pass in f16x3.  What it needs: a ray's samples inside one wavefront
    // (the list entry is written from a wave-level vote), no cascade (the point MLP's rows are internal).  (An occupancy volume adds a
    // head-dependent decision the band does not cover: hr_render then takes the f16x3 tiles throughout, see hr_render_fields.)
    // The per-sample margins (hr_math.h, HrRisk) are derived for: axis planes, sphere / cylinder with fixed origins, the euclidean distance;
    // the identity, affine and MIP-NeRF contractions.
    const bool isect_ok = c.isect_type == HR_ISECT_Z_PLANE || c.isect_type == HR_ISECT_VOXEL_GRID || c.isect_type == HR_ISECT_EUCLIDEAN_UNIFIED ||
                          ((c.isect_type == HR_ISECT_SPHERE || c.isect_type == HR_ISECT_CYLINDER) && c.origin_scale == 0.0f);
    const bool can_verify = !m->coarse && !m->is_coarse && c.z_channels <= 64 && c.mlp_layers >= 2 && c.mlp_hidden == 256 && isect_ok &&
                            c.contract_type != HR_CONTRACT_DONERF;
    m->verified = 0;
    if (want == HR_MLP_AUTO) {
        m->active_precision = fits ? (can_verify ? HR_MLP_F16F8 : HR_MLP_F16X3) : HR_MLP_BF16X3;
        m->verified = (fits && can_verify) ? 1 : 0;
        return HR_OK;
    }
    if (want == HR_MLP_F16F8V && !can_verify)
        return fail(HR_E_INVALID, "mlp_precision f16f8v (verified) needs a plain ray MLP of width 256, at most 64 samples per ray and an intersection "
                    "the margins are derived for (axis planes, sphere / cylinder with fixed origins, euclidean; not DoNeRFContract)");
    if (!fits)
        return fail(HR_E_RANGE, "mlp_precision %s was requested, but the MLP's activations reach %.4g on the calibration rays (limit %.4g = "
                    "65504 / 8): IEEE-half operands would overflow.  Use HR_MLP_AUTO (falls back to bf16x3) or HR_MLP_BF16X3",
                    want == HR_MLP_F16X3 ? "f16x3" : (want == HR_MLP_F16X2 ? "f16x2" : "f16f8"), (double)mx, (double)HR_F16_CALIBRATION_LIMIT);
    m->active_precision = (want == HR_MLP_F16F8V) ? HR_MLP_F16F8 : want;
    m->verified = (want == HR_MLP_F16F8V) ? 1 : 0;
    return HR_OK;
}

int hr_model_calibrate(hr_model* m, const float* rays_dev, int64_t n_rays, float* act_max, void* stream)
{
    if (!m) return fail(HR_E_INVALID, "null model");
    if (!m->finalized) return fail(HR_E_STATE, "hr_model_calibrate before hr_model_finalize");
    if (m->coarse || m->is_coarse) return fail(HR_E_INVALID, "hr_model_calibrate: cascades are calibrated by hr_model_finalize (the point MLP's rows are internal)");
    if (!rays_dev || n_rays <= 0) return fail(HR_E_INVALID, "hr_model_calibrate needs rays");
    const int before = m->active_precision, calibrated_before = m->calibrated, verified_before = m->verified;
    float act_before[HR_MAX_LAYERS];
    for (int l = 0; l < HR_MAX_LAYERS; ++l) act_before[l] = m->act_max[l];
    int rc = resolve_precision(m, rays_dev, n_rays, (hipStream_t)stream);
    if (rc != HR_OK) {                         // the model stays exactly as it was
        m->active_precision = before;
        m->verified = verified_before;
        m->calibrated = calibrated_before;
        for (int l = 0; l < HR_MAX_LAYERS; ++l) m->act_max[l] = act_before[l];
        return rc;
    }
    HR_HIP(hipMemset(m->flags, 0, sizeof(unsigned)));
    f8_exponents(m);
    if (m->active_precision != before || m->verified != verified_before) {
        m->packed_bytes -= m->mlp_bytes;
        rc = pack_mlp(m);
        if (rc != HR_OK) return rc;
        m->packed_bytes += m->mlp_bytes;
        HR_HIP(hipDeviceSynchronize());
    }
    if (act_max)
        for (int l = 0; l < m->cfg.mlp_layers; ++l) act_max[l] = m->act_max[l];
    m->band_stale = true;
    return calibrate_band(m, (hipStream_t)stream);
}

// The margins of the verified fast path for THIS model: both arithmetics' heads on the calibration rays, pushed through the
// model's own activations, anchors, contraction and intersection by the probe kernel (band_kernel.hip) in the normalisation the sample
// stage's per-sample margins use (hr_math.h, HrRisk); margin = 4 x the largest difference, never below HR_BAND_FLOOR.  Then the
// well-conditioned calibration rays once through the verified path and once through the f16x3 tiles: the fraction listed, and how far the
// two images are apart.  HR_MLP_AUTO gives the fast path up (f16x3 throughout) above 5 % / 6e-5.  Synchronises `st`.
int calibrate_band(hr_model* m, hipStream_t st)
{
    m->band_stale = false;
    hr_verify_info& vi = m->vinfo;
    const int fallback_before = vi.fallback;
    vi = hr_verify_info();
    vi.verified = m->verified;
    vi.band_floor = HR_BAND_FLOOR;
    vi.fallback = (fallback_before && !m->verified) ? fallback_before : 0;
    if (!m->verified || m->coarse || m->is_coarse) return HR_OK;
    if (!m->calib_rays || m->calib_n <= 0 || !m->head) return fail(HR_E_STATE, "verified fast path without calibration rays / workspace");
    bool too_many = false, too_far = false;
    {   // (the temporaries are freed before a fallback re-packs)
        const hr_config& c = m->cfg;
        const int Z = c.z_channels, P = c.preds_per_z;
        const int64_t N = m->calib_n, nc_max = N < m->chunk ? N : m->chunk;
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
            const float* rays = m->calib_rays + r0 * c.ray_dim;
            for (int tier = 0; tier < 2; ++tier) {
                HrMlpArgs ma;
                fill_mlp_args(m, ma, rays, n, tier);
                launch_mlp(m, m->kcfg, ma, st, tier);
                hr_launch_head_export(m->head, tier == 0 ? ha : hb, n, Z, P, m->p_live, (m->n_out + 3) / 4, rows_per_ray(c), m->col_map, st);
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
        HR_HIP(hipMemcpyAsync(rays_h.data(), m->calib_rays, sizeof(float) * rays_h.size(), hipMemcpyDeviceToHost, st));
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
        m->redo_band = fmaxf(HR_BAND_FLOOR, 4.0f * fmaxf(vi.max_d_zc, vi.max_d_dist_n));
        m->redo_band_q = fmaxf(HR_BAND_FLOOR, 4.0f * vi.max_d_geo_n);
        m->redo_band_off = 4.0f * vi.max_d_off;
        vi.band = m->redo_band;
        vi.band_q = m->redo_band_q;
        vi.band_off = m->redo_band_off;
        // the well-conditioned rays, compacted on the host (<= 65 536 rays: not worth a kernel)
        int64_t nu = 0;
        for (int64_t i = 0; i < N; ++i)
            if (ok[(size_t)i]) {
                if (nu != i) memcpy(&rays_h[(size_t)nu * c.ray_dim], &rays_h[(size_t)i * c.ray_dim], sizeof(float) * c.ray_dim);
                ++nu;
            }
        vi.n_rays_used = nu;
        // (fewer than 64 well-conditioned rays -- a caller calibrating on a handful: the margins stand, there is no image to judge by)
        if (nu >= 64) {
            // through the verified path as a render call takes it, and through the f16x3 tiles throughout: what fraction the first pass lists with
            // these margins, and how far the two IMAGES are apart -- f16f8's continuous error (every pixel that is not listed keeps it) grows with
            // the weights like the margins do, and no margin repairs it
            HR_HIP(sel.alloc(sizeof(float) * nu * c.ray_dim));
            HR_HIP(rgb.alloc(sizeof(float) * nu * 3));
            HR_HIP(rgb2.alloc(sizeof(float) * nu * 3));
            HR_HIP(hipMemcpyAsync(sel, rays_h.data(), sizeof(float) * nu * c.ray_dim, hipMemcpyHostToDevice, st));
            HR_HIP(hipMemsetAsync(m->redo_count, 0, 4 * sizeof(unsigned), st));
            render_verified(m, sel, nu, rgb, hr_redo_list_cap(nu, m->redo_cap), st);
            unsigned listed = 0;
            HR_HIP(hipMemcpyAsync(&listed, m->redo_count + 1, sizeof(unsigned), hipMemcpyDeviceToHost, st));
            for (int64_t r0 = 0; r0 < nu; r0 += m->chunk) {
                const int64_t n = (nu - r0 < m->chunk) ? (nu - r0) : m->chunk;
                const float* rays = sel + r0 * c.ray_dim;
                launch_front(m, rays, n, st, -1, 1);
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
            vi.listed_frac = (float)((double)listed / (double)nu);
            too_far = !(vi.max_d_rgb <= HR_VERIFY_RGB_LIMIT);
        }
        // the CALLER's rays are what will be rendered: the ill-conditioned ones among them are listed too (synthetic rays point anywhere;
        // half of them graze a z-plane net's planes, which says nothing about its cameras)
        if (m->calibrated == 2) vi.listed_frac = (float)(((double)(N - nu) + (double)vi.listed_frac * (double)nu) / (double)N);
        too_many = vi.listed_frac > HR_VERIFY_LISTED_LIMIT;
        HR_HIP(hipMemsetAsync(m->redo_count, 0, 4 * sizeof(unsigned), st));
        HR_HIP(hipMemsetAsync(m->flags, 0, sizeof(unsigned), st));        // range bits the calibration rays raised are not the caller's
        HR_HIP(hipStreamSynchronize(st));
    }
    if ((too_many || too_far) && m->cfg.mlp_precision == HR_MLP_AUTO) {
        // more than a twentieth of the rays would be rendered twice (a call's list holds a sixteenth), or the cheap arithmetic's own error is
        // too large a share of the 1e-4 budget on this model: plain f16x3 lists nothing and has neither problem
        m->verified = 0;
        m->active_precision = HR_MLP_F16X3;
        m->packed_bytes -= m->mlp_bytes;
        const int rc = pack_mlp(m);
        if (rc != HR_OK) return rc;
        m->packed_bytes += m->mlp_bytes;
        HR_HIP(hipDeviceSynchronize());
        m->band_stale = false;
        vi.verified = 0;
        vi.fallback = too_far ? 2 : 1;
    }
    return HR_OK;
}

int hr_model_verify_info(hr_model* m, hr_verify_info* out)
{
    if (!m || !out) return fail(HR_E_INVALID, "null argument");
    if (!m->finalized) return fail(HR_E_STATE, "hr_model_finalize has not been called");
    *out = m->vinfo;
    out->verified = m->verified;
    return HR_OK;
}
