// C ABI, training: the differentiable forward / backward of the render path, the fused MLP training forward, Linear layers, the plane
// regulariser and Adam.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "hr_model.h"

size_t hr_linear_workspace(int64_t rows, int32_t in, int32_t out)
{
    if (rows < 1 || in < 1 || out < 1) return 0;
    return hr_linear_workspace_bytes(rows, in, out);
}

int hr_linear_forward(const float* x_dev, int64_t ldx, int64_t rows, int32_t in, const float* w_dev, const float* b_dev, int32_t out,
                      float leaky_slope, float* y_dev, int64_t ldy, void* stream)
{
    if (rows < 0 || in < 1 || out < 1 || ldx < in || ldy < out) return fail(HR_E_INVALID, "bad Linear shape");
    if (rows > 0 && (!x_dev || !w_dev || !y_dev)) return fail(HR_E_INVALID, "null argument");
    if (rows > 0x7fffffff) return fail(HR_E_INVALID, "more than 2^31 rows");
    hr_launch_linear_forward(x_dev, ldx, rows, in, w_dev, b_dev, out, leaky_slope, y_dev, ldy, (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

int hr_linear_backward(const float* x_dev, int64_t ldx, const float* w_dev, const float* y_dev, int64_t ldy, const float* dy_dev, int64_t ld_dy,
                       int64_t rows, int32_t in, int32_t out, float leaky_slope, float* dx_dev, int64_t ld_dx, float* dw_dev, float* db_dev,
                       float* workspace_dev, void* stream)
{
    if (rows < 0 || in < 1 || out < 1 || ldx < in || ld_dy < out || (dx_dev && ld_dx < in) || (y_dev && ldy < out))
        return fail(HR_E_INVALID, "bad Linear shape");
    if (rows > 0 && (!x_dev || !w_dev || !dy_dev || !dw_dev || !db_dev || !workspace_dev)) return fail(HR_E_INVALID, "null argument");
    // (an empty batch has an empty output: no mask to ask for -- the weight and bias gradients are zero)
    if (rows > 0 && leaky_slope >= 0.0f && !y_dev) return fail(HR_E_INVALID, "an activated layer needs its output for the LeakyReLU mask");
    if (rows > 0x7fffffff) return fail(HR_E_INVALID, "more than 2^31 rows");
    if (rows == 0) {
        if (!dw_dev || !db_dev) return fail(HR_E_INVALID, "null argument");
        hr_launch_fill_zero(HrFillBatch{{dw_dev, db_dev}, {(size_t)out * in, (size_t)out}, 2}, (hipStream_t)stream);     // (a kernel: no memset node)
        HR_HIP(hipGetLastError());
        return HR_OK;
    }
    hr_launch_linear_backward(x_dev, ldx, w_dev, y_dev, ldy, dy_dev, ld_dy, rows, in, out, leaky_slope, dx_dev, ld_dx, dw_dev, db_dev, workspace_dev,
                              (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

int hr_plane_reg_forward(const float* plane_dev, int32_t channels, int32_t h, int32_t w, float* sums_dev, void* stream)
{
    if (channels < 0 || h < 1 || w < 1) return fail(HR_E_INVALID, "bad plane shape");
    if (!sums_dev || (channels > 0 && !plane_dev)) return fail(HR_E_INVALID, "null argument");
    hr_launch_plane_reg_forward(plane_dev, channels, h, w, sums_dev, (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

int hr_plane_reg_backward(const float* plane_dev, int32_t channels, int32_t h, int32_t w, const float* coef_dev, float* grad_dev, void* stream)
{
    if (channels < 0 || h < 1 || w < 1) return fail(HR_E_INVALID, "bad plane shape");
    if (channels > 0 && (!plane_dev || !coef_dev || !grad_dev)) return fail(HR_E_INVALID, "null argument");
    hr_launch_plane_reg_backward(plane_dev, channels, h, w, coef_dev, grad_dev, (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

int hr_adam_step(float* const* param_dev, const float* const* grad_dev, float* const* exp_avg_dev, float* const* exp_avg_sq_dev, const int64_t* n,
                 const double* hp, int32_t n_tensors, void* stream)
{
    if (n_tensors < 0 || (n_tensors > 0 && (!param_dev || !grad_dev || !exp_avg_dev || !exp_avg_sq_dev || !n || !hp))) return fail(HR_E_INVALID, "null argument");
    if (n_tensors == 0) return HR_OK;
    HrAdamBatch b;
    b.count = 0;
    b.first_block[0] = 0;
    auto flush = [&]() {
        hr_launch_adam(b, (hipStream_t)stream);
        b.count = 0;
        b.first_block[0] = 0;
    };
    for (int i = 0; i < n_tensors; ++i) {
        if (n[i] < 0) return fail(HR_E_INVALID, "hr_adam_step: tensor %d has a negative size", i);
        if (n[i] == 0) continue;
        if (!param_dev[i] || !grad_dev[i] || !exp_avg_dev[i] || !exp_avg_sq_dev[i]) return fail(HR_E_INVALID, "hr_adam_step: tensor %d has a null buffer", i);
        const double lr = hp[6 * i], b1 = hp[6 * i + 1], b2 = hp[6 * i + 2], eps = hp[6 * i + 3], wd = hp[6 * i + 4], step = hp[6 * i + 5];
        if (!(step >= 1.0) || !(b1 >= 0.0 && b1 < 1.0) || !(b2 >= 0.0 && b2 < 1.0)) return fail(HR_E_INVALID, "hr_adam_step: tensor %d: step >= 1 and betas in [0, 1) required", i);
        const int64_t blocks = (n[i] + 4095) / 4096;
        if (blocks > 0x3fffffff) return fail(HR_E_INVALID, "hr_adam_step: tensor %d is too large", i);
        if (b.count == HR_ADAM_MAX_TENSORS || (int64_t)b.first_block[b.count] + blocks > 0x7fffffff) flush();
        const int k = b.count++;
        b.p[k] = param_dev[i]; b.g[k] = grad_dev[i]; b.m[k] = exp_avg_dev[i]; b.v[k] = exp_avg_sq_dev[i]; b.n[k] = n[i];
        // bias corrections in double on the host (torch: python floats)
        const double bc1 = 1.0 - pow(b1, step), bc2 = 1.0 - pow(b2, step);
        b.step_size[k] = (float)(lr / bc1);
        b.inv_sqrt_bc2[k] = (float)(1.0 / sqrt(bc2));
        b.omb1[k] = (float)(1.0 - b1); b.beta2[k] = (float)b2; b.omb2[k] = (float)(1.0 - b2); b.eps[k] = (float)eps; b.weight_decay[k] = (float)wd;
        b.first_block[k + 1] = b.first_block[k] + (int)blocks;
    }
    if (b.count > 0) flush();
    HR_HIP(hipGetLastError());
    return HR_OK;
}

int hr_adam_step_dev(float* const* param_dev, const float* const* grad_dev, float* const* exp_avg_dev, float* const* exp_avg_sq_dev, const int64_t* n,
                     const double* hp, const int32_t* lr_index, int32_t n_lr, const float* lr_dev, int64_t* step_dev, int32_t n_tensors, void* stream)
{
    if (n_tensors < 0 || (n_tensors > 0 && (!param_dev || !grad_dev || !exp_avg_dev || !exp_avg_sq_dev || !n || !hp || !lr_index || !lr_dev || !step_dev)))
        return fail(HR_E_INVALID, "hr_adam_step_dev: null argument");
    // validate everything before the first launch: a refused call must leave no tensor stepped
    bool any = false;
    for (int i = 0; i < n_tensors; ++i) {
        if (n[i] < 0) return fail(HR_E_INVALID, "hr_adam_step_dev: tensor %d has a negative size", i);
        if (n[i] == 0) continue;
        if (!param_dev[i] || !grad_dev[i] || !exp_avg_dev[i] || !exp_avg_sq_dev[i]) return fail(HR_E_INVALID, "hr_adam_step_dev: tensor %d has a null buffer", i);
        const double b1 = hp[4 * i], b2 = hp[4 * i + 1];
        if (!(b1 >= 0.0 && b1 < 1.0) || !(b2 >= 0.0 && b2 < 1.0)) return fail(HR_E_INVALID, "hr_adam_step_dev: tensor %d: betas in [0, 1) required", i);
        if (lr_index[i] < 0 || lr_index[i] >= n_lr) return fail(HR_E_INVALID, "hr_adam_step_dev: tensor %d reads learning rate %d of %d", i, (int)lr_index[i], (int)n_lr);
        if ((n[i] + 4095) / 4096 > 0x3fffffff) return fail(HR_E_INVALID, "hr_adam_step_dev: tensor %d is too large", i);
        any = true;
    }
    if (!any) return HR_OK;
    HrAdamDevBatch b;
    b.count = 0;
    b.first_block[0] = 0;
    b.lr = lr_dev;
    b.step = step_dev;
    auto flush = [&]() {
        hr_launch_adam_dev(b, (hipStream_t)stream);
        b.count = 0;
        b.first_block[0] = 0;
    };
    for (int i = 0; i < n_tensors; ++i) {
        if (n[i] == 0) continue;
        const double b1 = hp[4 * i], b2 = hp[4 * i + 1], eps = hp[4 * i + 2], wd = hp[4 * i + 3];
        const int64_t blocks = (n[i] + 4095) / 4096;
        if (b.count == HR_ADAM_MAX_TENSORS || (int64_t)b.first_block[b.count] + blocks > 0x7fffffff) flush();
        const int k = b.count++;
        b.p[k] = param_dev[i]; b.g[k] = grad_dev[i]; b.m[k] = exp_avg_dev[i]; b.v[k] = exp_avg_sq_dev[i]; b.n[k] = n[i];
        b.beta1[k] = b1; b.beta2d[k] = b2;
        b.omb1[k] = (float)(1.0 - b1); b.beta2[k] = (float)b2; b.omb2[k] = (float)(1.0 - b2); b.eps[k] = (float)eps; b.weight_decay[k] = (float)wd;
        b.lr_index[k] = lr_index[i];
        b.first_block[k + 1] = b.first_block[k] + (int)blocks;
    }
    if (b.count > 0) flush();
    // the count advances in a launch of its own, behind every block of the step on the stream: none of them can read the new value
    hr_launch_adam_advance(step_dev, (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

// ---------------------------------------------------------------- training path
// the sample stage's training kernels of the model: the time-dependent colour modes have a build of their own (train_time_kernel.hip)
static void launch_train(const hr_model* m, const HrTrainArgs& a, hipStream_t st)
{
    if (hr_shading_is_time_family(m->cfg.shading)) hr_launch_train_time(m->cfg, &a, sizeof(a), st);
    else hr_launch_train(m->cfg, a, st);
}

static int check_train(hr_model* m, const float* rays, int64_t n)
{
    if (!m) return fail(HR_E_INVALID, "null model");
    if (m->is_coarse) return fail(HR_E_INVALID, "training path: pass the cascade's handle, not its coarse level");
    if (!m->finalized) return fail(HR_E_STATE, "hr_model_finalize has not been called (or tensors changed since)");
    if (const char* why = hr_train_unsupported(m->cfg)) return fail(HR_E_INVALID, "training path: %s not differentiated", why);
    if (hr_model_time_density(m)) return fail(HR_E_INVALID, "training path: densityMode DensityLinear / DensityFourier (inference only) not differentiated");
    if (m->ca_total > HR_TRAIN_MAX_CA) return fail(HR_E_INVALID, "training path: more than %d appearance components", HR_TRAIN_MAX_CA);
    if (n < 0 || (n > 0 && !rays)) return fail(HR_E_INVALID, "bad ray buffer");
    for (hr_model* lvl : {m, m->coarse.get()}) {
        if (!lvl || lvl->ucfg_dev) continue;
        HR_HIP(lvl->ucfg_dev.alloc(sizeof(hr_config)));
        HR_HIP(hipMemcpy(lvl->ucfg_dev, &lvl->cfg, sizeof(hr_config), hipMemcpyHostToDevice));
    }
    return HR_OK;
}

// per-sample workspace of the backward's phases (hr_tape_bind's HR_TAPE_WORDS per sample); grows on the first step and if the batch grows
static int ensure_tape(hr_model* m, int64_t ns, hipStream_t st)
{
    if (ns <= m->tape_samples) return HR_OK;
    HR_HIP(hipStreamSynchronize(st));
    m->tape.reset();
    m->tape_samples = 0;
    HR_HIP(m->tape.alloc(sizeof(float) * HR_TAPE_WORDS * (size_t)ns));
    m->tape_samples = ns;
    return HR_OK;
}

// the four reference-layout tensors of plane pair j: {density a, app a, density b, app b} with their channel counts
struct TrainPlaneIO {
    float* p[4];
    int ch[4];
};
static TrainPlaneIO train_plane_io(const hr_model* m, const hr_train_tensors* t, int j)
{
    const hr_config& c = m->cfg;
    int nd = c.n_den[j], na = c.n_app[j];
    if (c.video && nd == 0) na = 0;
    return TrainPlaneIO{{t->density_a[j], t->app_a[j], t->density_b[j], t->app_b[j]}, {nd, na, nd, na}};
}

int hr_train_features(hr_model* m, const float* rays_dev, int64_t n_rays, float* feats_dev, void* stream)
{
    int rc = check_train(m, rays_dev, n_rays);
    if (rc != HR_OK) return rc;
    if (n_rays > 0 && !feats_dev) return fail(HR_E_INVALID, "null feature buffer");
    // a cascade's ray MLP belongs to its coarse level
    hr_launch_features(m->coarse ? m->coarse->ucfg_dev : m->ucfg_dev, rays_dev, n_rays, feats_dev, (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

int hr_mlp_train_forward(hr_model* m, const float* const* weights_dev, const float* const* biases_dev, const float* rays_dev, int64_t n_rays,
                         float* const* acts_dev, const int64_t* act_ld, const int32_t* act_off, float* head_dev, void* stream)
{
    int rc = check_train(m, rays_dev, n_rays);
    if (rc != HR_OK) return rc;
    if (m->coarse || m->is_coarse) return fail(HR_E_INVALID, "hr_mlp_train_forward: point_prediction cascades run their MLPs layer by layer (hr_linear_forward)");
    const hr_config& c = m->cfg;
    const int L = c.mlp_layers;
    if (L < 2 || c.mlp_hidden != 256) return fail(HR_E_INVALID, "hr_mlp_train_forward needs hidden width 256 and at least two layers");
    if (!weights_dev || !biases_dev || !acts_dev || !act_ld || !act_off || (n_rays > 0 && !head_dev)) return fail(HR_E_INVALID, "null argument");
    hipStream_t st = (hipStream_t)stream;
    // ---- the current parameter values -> bf16 hi / lo tiles, on the device (what pack_mlp does on the host at finalize: hr_mlp_pack.h)
    const int P_user = c.preds_per_z, P_live = m->p_live;
    const int k0p = m->mlp.pack->k0p, n_out = m->mlp.pack->n_out;
    HrMlpTiles& t = m->train_tiles;
    for (int l = 0; l < L; ++l) {
        if (!weights_dev[l] || !biases_dev[l]) return fail(HR_E_INVALID, "hr_mlp_train_forward: layer %d has no weights", l);
        const HrMlpLayer g = mlp_layer(c, m->p_live, m->col_map, l, 32);
        if (!t.wsplit[l] || t.n_tiles[l] != g.nt) {
            t.wsplit[l].reset();
            t.bias[l].reset();
            HR_HIP(t.wsplit[l].alloc(sizeof(uint16_t) * (size_t)(g.Kp / 16) * g.nt * 2 * 64 * 8));
            HR_HIP(t.bias[l].alloc(sizeof(float) * (size_t)g.nt * 32));
            t.n_tiles[l] = g.nt;
        }
        hr_launch_pack_split_bf16(g, weights_dev[l], biases_dev[l], t.wsplit[l], t.bias[l], st);
    }
    HrMlpTaps taps = {};
    for (int l = 0; l + 1 < L; ++l) { taps.act[l] = acts_dev[l]; taps.ld[l] = act_ld[l]; taps.off[l] = act_off[l]; }
    const int nq = (n_out + 3) / 4;
    for (int64_t r0 = 0; r0 < n_rays; r0 += m->chunk) {
        const int64_t n = (n_rays - r0 < m->chunk) ? (n_rays - r0) : m->chunk;
        HrMlpArgs a = {};
        a.rays = rays_dev + r0 * c.ray_dim;
        a.n_rays = n;
        a.head = m->head;
        for (int l = 0; l < L; ++l) { a.wsplit[l] = t.wsplit[l]; a.bias[l] = t.bias[l]; a.winv[l] = 1.0f; a.n_tiles[l] = t.n_tiles[l]; }
        a.n_out = n_out; a.nq = nq; a.k0p = k0p;
        a.trace = nullptr; a.flags = nullptr;
        HrMlpTaps tc = taps;
        for (int l = 0; l + 1 < L; ++l)
            if (tc.act[l]) tc.act[l] += r0 * tc.ld[l];
        hr_launch_mlp_train_bf16x3(m->kcfg, a, tc, st);
        hr_launch_head_export(m->head, head_dev + r0 * (int64_t)c.z_channels * P_user, n, c.z_channels, P_user, P_live, nq, 1, m->col_map, st);
    }
    HR_HIP(hipGetLastError());
    return HR_OK;
}

static void fill_train_args(const hr_model* m, HrTrainArgs& a, const float* rays, const float* head, int64_t n, int white_bg)
{
    a = HrTrainArgs();
    a.cfg_dev = m->ucfg_dev;
    a.rays = rays;
    a.head = head;
    a.n_rays = n;
    for (int j = 0; j < 3; ++j) { a.planes[j] = m->planes[j]; a.g_a[j] = m->grad_a[j]; a.g_b[j] = m->grad_b[j]; }
    a.basis = m->basis;
    a.n_basis_cols = m->n_basis_cols;
    a.ca_total = m->ca_total;
    a.white_bg = white_bg ? 1 : 0;
    if (m->bg_source == 1) {          // hr_train_set_background: a white_bg configuration is white at every step, any other one flips the coin
        a.white_bg = m->cfg.white_bg ? 1 : 0;
        if (!m->cfg.white_bg) { a.bg_step = m->bg_step_dev; a.bg_seed = m->bg_seed; }
    }
    a.color_table = nullptr;
    if (m->cfg.color_table_views > 0) {
        auto it = m->raw.find("color_embedding");
        if (it != m->raw.end()) a.color_table = it->second.p;
    }
}

static int train_forward(hr_model* m, const hr_train_tensors* params, const float* rays_dev, const float* head_dev, int64_t n_rays,
                         int32_t white_bg, float* rgb_dev, const hr_fields* fields, void* stream);

int32_t hr_train_background_coin(uint64_t seed, uint64_t step) { return hr_background_coin(seed, step); }

int hr_train_set_background(hr_model* m, int32_t source, uint64_t seed, const int64_t* step_dev)
{
    if (!m) return fail(HR_E_INVALID, "hr_train_set_background: null model");
    if (source != 0 && source != 1) return fail(HR_E_INVALID, "hr_train_set_background: source %d (0: the white_bg argument, 1: the coin of the device step count)", (int)source);
    if (source == 1 && !step_dev) return fail(HR_E_INVALID, "hr_train_set_background: source 1 needs the device step count (step_dev)");
    m->bg_source = source;
    m->bg_seed = source == 1 ? seed : 0;
    m->bg_step_dev = source == 1 ? step_dev : nullptr;
    return HR_OK;
}

int hr_train_forward(hr_model* m, const hr_train_tensors* params, const float* rays_dev, const float* head_dev, int64_t n_rays,
                     int32_t white_bg, float* rgb_dev, void* stream)
{
    return train_forward(m, params, rays_dev, head_dev, n_rays, white_bg, rgb_dev, nullptr, stream);
}

int hr_train_forward_fields(hr_model* m, const hr_train_tensors* params, const float* rays_dev, const float* head_dev, int64_t n_rays,
                            int32_t white_bg, float* rgb_dev, const hr_fields* fields, void* stream)
{
    if (fields && (fields->sigma_dev || fields->head_dev)) return fail(HR_E_INVALID, "hr_train_forward_fields serves distances, points and weights");
    if (fields && m && m->cfg.z_channels > 64) return fail(HR_E_INVALID, "hr_train_forward_fields: rays of more than 64 samples take the one-thread-per-ray walk, which keeps no fields");
    return train_forward(m, params, rays_dev, head_dev, n_rays, white_bg, rgb_dev, fields, stream);
}

static int train_forward(hr_model* m, const hr_train_tensors* params, const float* rays_dev, const float* head_dev, int64_t n_rays,
                         int32_t white_bg, float* rgb_dev, const hr_fields* fields, void* stream)
{
    int rc = check_train(m, rays_dev, n_rays);
    if (rc != HR_OK) return rc;
    if (n_rays > 0 && (!head_dev || !rgb_dev)) return fail(HR_E_INVALID, "null head / rgb buffer");
    hipStream_t st = (hipStream_t)stream;
    if (params) {                     // this step's parameter values -> the kernels' texel layout (no allocation, no sync)
        HrLayoutBatch batch = {};                  // all twelve tensors in one launch
        for (int j = 0; j < 3; ++j) {
            const HrGridPlane& g = m->planes[j];
            if (g.tex == 0) continue;
            const TrainPlaneIO io = train_plane_io(m, params, j);
            for (int t = 0; t < 4; ++t) {
                if (io.ch[t] == 0) continue;
                if (!io.p[t]) return fail(HR_E_INVALID, "hr_train_forward: params tensor of plane pair %d is NULL", j);
                const bool is_a = t < 2;
                batch.job[batch.n++] = HrLayoutJob{io.p[t], is_a ? m->grid_a[j] : m->grid_b[j], io.ch[t], is_a ? g.ah : g.bh, is_a ? g.aw : g.bw, g.tex,
                                                   (t & 1) ? 4 * g.cd4 : 0};
            }
        }
        hr_launch_layout_batch(batch, true, st);
        const size_t bytes = m->raw["basis_mat.weight"].bytes;
        if (bytes > 0) {
            if (!params->basis) return fail(HR_E_INVALID, "hr_train_forward: params->basis is NULL");
            HR_HIP(hipMemcpyAsync(m->basis, params->basis, bytes, hipMemcpyDeviceToDevice, st));
            // the render kernels read the column-major copy: keep it in step, so that hr_render after a training step sees the
            // same basis_mat as the planes refreshed above
            hr_launch_basis_transpose(m->basis, m->basis_t, m->cfg.app_dim, m->n_basis_cols, m->basis_ld, st);
        }
        if (m->cfg.color_table_views > 0) {       // read in place from the uploaded copy: refresh it
            if (!params->color_table) return fail(HR_E_INVALID, "hr_train_forward: params->color_table is NULL");
            DevBuf& b = m->raw["color_embedding"];
            HR_HIP(hipMemcpyAsync(b.p, params->color_table, b.bytes, hipMemcpyDeviceToDevice, st));
        }
    }
    HrTrainArgs a;
    fill_train_args(m, a, rays_dev, head_dev, n_rays, white_bg);
    a.rgb = rgb_dev;
    if (fields) { a.f_dist = fields->distances_dev; a.f_points = fields->points_dev; a.f_weights = fields->weights_dev; }
    launch_train(m, a, st);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

int hr_train_backward(hr_model* m, const float* rays_dev, const float* head_dev, const float* d_rgb_dev, int64_t n_rays,
                      int32_t white_bg, float* d_head_dev, const hr_train_tensors* grads, void* stream)
{
    int rc = check_train(m, rays_dev, n_rays);
    if (rc != HR_OK) return rc;
    if (!grads) return fail(HR_E_INVALID, "null grads");
    if (n_rays > 0 && (!head_dev || !d_rgb_dev || !d_head_dev)) return fail(HR_E_INVALID, "null head / d_rgb / d_head buffer");
    hipStream_t st = (hipStream_t)stream;
    if (!m->grad_pool) {              // packed accumulators: one allocation, made on the first step
        const HrGradPool pool = hr_grad_pool(m->planes, sizeof(float), 256);
        if (pool.total > 0) {
            HR_HIP(m->grad_pool.alloc(sizeof(float) * pool.total));
            m->grad_pool_bytes = sizeof(float) * pool.total;
            float* base = reinterpret_cast<float*>(static_cast<char*>(m->grad_pool));
            for (int j = 0; j < 3; ++j) {
                if (m->planes[j].tex == 0) continue;
                m->grad_a[j] = base + pool.off_a[j];
                m->grad_b[j] = base + pool.off_b[j];
            }
        }
    }
    const size_t basis_bytes = m->raw["basis_mat.weight"].bytes;
    // basis_mat's gradient needs no re-layout: accumulate in the caller's buffer
    float* d_basis = grads->basis;
    if (!d_basis) return fail(HR_E_INVALID, "hr_train_backward: grads->basis is NULL");
    if (m->cfg.color_table_views > 0 && !grads->color_table) return fail(HR_E_INVALID, "hr_train_backward: grads->color_table is NULL");
    // The step's accumulators are cleared on the stream by ONE fill kernel (no memset node: the step is meant to be replayed from a graph,
    // DESIGN 10).  Default build: the packed texel gradients, basis_mat's and the colour table's.  Deterministic build: its fixed-point
    // scratch alone -- hr_launch_fixed_to_float overwrites every element of those three from it, so they need no clear.
    HrFillBatch clear = {};
    if (!m->opt_train_det) {
        if (m->grad_pool) { clear.p[clear.count] = reinterpret_cast<float*>(static_cast<char*>(m->grad_pool)); clear.n[clear.count++] = m->grad_pool_bytes / sizeof(float); }
        if (basis_bytes > 0) { clear.p[clear.count] = d_basis; clear.n[clear.count++] = basis_bytes / sizeof(float); }
        if (m->cfg.color_table_views > 0) { clear.p[clear.count] = grads->color_table; clear.n[clear.count++] = 12 * (size_t)m->cfg.color_table_views; }
        hr_launch_fill_zero(clear, st);
    }
    const int64_t ns = n_rays * m->cfg.z_channels;
    rc = ensure_tape(m, ns, st);
    if (rc != HR_OK) return rc;
    HrTrainArgs a;
    fill_train_args(m, a, rays_dev, head_dev, n_rays, white_bg);
    a.tape = hr_tape_bind(m->tape, ns);
    a.d_rgb = d_rgb_dev;
    a.d_head = d_head_dev;
    a.d_basis = d_basis;
    if (m->cfg.color_table_views > 0) a.d_color_table = grads->color_table;
    if (m->opt_train_det) {
        // deterministic mode: every accumulator of the step is a 64-bit fixed-point word of ONE scratch buffer (integer atomics: the
        // totals do not depend on the order of the adds); converted to the float buffers the rest of the step reads
        const HrGradPool pool = hr_grad_pool(m->planes, sizeof(long long), sizeof(long long));       // packed
        const size_t *off_a = pool.off_a, *off_b = pool.off_b, *n_a = pool.n_a, *n_b = pool.n_b;
        size_t need = pool.total;
        const size_t n_basis = basis_bytes / sizeof(float), off_basis = need;
        need += n_basis;
        const size_t n_ct = m->cfg.color_table_views > 0 ? 12 * (size_t)m->cfg.color_table_views : 0, off_ct = need;
        need += n_ct;
        if (need > m->grad_fx_elems) {
            HR_HIP(hipStreamSynchronize(st));
            m->grad_fx.reset(); m->grad_fx_elems = 0;
            HR_HIP(m->grad_fx.alloc(sizeof(long long) * need));
            m->grad_fx_elems = need;
        }
        clear.p[0] = reinterpret_cast<float*>(static_cast<long long*>(m->grad_fx)); clear.n[0] = need * (sizeof(long long) / sizeof(float)); clear.count = 1;
        hr_launch_fill_zero(clear, st);
        if (!m->fx_unit) HR_HIP(m->fx_unit.alloc(sizeof(HrFxUnit)));
        HrTrainArgs ad = a;
        ad.fx = m->fx_unit;
        for (int j = 0; j < 3; ++j) {
            ad.g_a[j] = n_a[j] ? reinterpret_cast<float*>(m->grad_fx + off_a[j]) : nullptr;
            ad.g_b[j] = n_b[j] ? reinterpret_cast<float*>(m->grad_fx + off_b[j]) : nullptr;
        }
        ad.d_basis = reinterpret_cast<float*>(m->grad_fx + off_basis);
        ad.d_color_table = n_ct ? reinterpret_cast<float*>(m->grad_fx + off_ct) : nullptr;
        if (hr_shading_is_time_family(m->cfg.shading)) hr_launch_train_time_det(m->cfg, &ad, sizeof(ad), st);
        else hr_launch_train_det(m->cfg, &ad, sizeof(ad), st);
        const float* fx_inv = &m->fx_unit->inv;
        const unsigned* fx_bad = &m->fx_unit->bad;
        for (int j = 0; j < 3; ++j) {
            if (n_a[j]) hr_launch_fixed_to_float(m->grad_fx + off_a[j], m->grad_a[j], (int64_t)n_a[j], fx_inv, fx_bad, st);
            if (n_b[j]) hr_launch_fixed_to_float(m->grad_fx + off_b[j], m->grad_b[j], (int64_t)n_b[j], fx_inv, fx_bad, st);
        }
        hr_launch_fixed_to_float(m->grad_fx + off_basis, d_basis, (int64_t)n_basis, fx_inv, fx_bad, st);
        if (n_ct) hr_launch_fixed_to_float(m->grad_fx + off_ct, grads->color_table, (int64_t)n_ct, fx_inv, fx_bad, st);
    } else {
        launch_train(m, a, st);
    }
    HrLayoutBatch batch = {};                      // packed texel gradients -> the reference's (C, H, W) tensors, one launch
    for (int j = 0; j < 3; ++j) {
        const HrGridPlane& g = m->planes[j];
        if (g.tex == 0) continue;
        const TrainPlaneIO io = train_plane_io(m, grads, j);
        for (int t = 0; t < 4; ++t) {
            if (io.ch[t] == 0 || !io.p[t]) continue;
            const bool is_a = t < 2;
            batch.job[batch.n++] = HrLayoutJob{is_a ? m->grad_a[j] : m->grad_b[j], io.p[t], io.ch[t], is_a ? g.ah : g.bh, is_a ? g.aw : g.bw, g.tex,
                                               (t & 1) ? 4 * g.cd4 : 0};
        }
    }
    hr_launch_layout_batch(batch, false, st);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

static int fill_rows_args(hr_model* m, HrRowsArgs& a, const float* rays, const float* head, int64_t n)
{
    if (!m->coarse) return fail(HR_E_INVALID, "hr_train_rows_*: the model is not a point_prediction cascade");
    a = HrRowsArgs();
    a.cfg_dev = m->coarse->ucfg_dev;
    a.rays = rays;
    a.head = head;
    a.n_rays = n;
    a.row_dim = m->cfg.casc_row_dim;
    a.n_inputs = m->cfg.casc_n_inputs;
    for (int i = 0; i < 4; ++i) { a.kind[i] = m->cfg.casc_input_kind[i]; a.len[i] = m->cfg.casc_input_dim[i]; }
    return HR_OK;
}

int hr_train_rows_forward(hr_model* m, const float* rays_dev, const float* head_dev, int64_t n_rays, float* rows_dev, void* stream)
{
    int rc = check_train(m, rays_dev, n_rays);
    if (rc != HR_OK) return rc;
    if (n_rays > 0 && (!head_dev || !rows_dev)) return fail(HR_E_INVALID, "null head / rows buffer");
    HrRowsArgs a;
    rc = fill_rows_args(m, a, rays_dev, head_dev, n_rays);
    if (rc != HR_OK) return rc;
    a.rows = rows_dev;
    hr_launch_rows(m->coarse->cfg, a, (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

int hr_train_rows_backward(hr_model* m, const float* rays_dev, const float* head_dev, const float* d_rows_dev, int64_t n_rays,
                           float* rows_scratch_dev, float* d_head_dev, void* stream)
{
    int rc = check_train(m, rays_dev, n_rays);
    if (rc != HR_OK) return rc;
    if (n_rays > 0 && (!head_dev || !d_rows_dev || !rows_scratch_dev || !d_head_dev)) return fail(HR_E_INVALID, "null buffer");
    HrRowsArgs a;
    rc = fill_rows_args(m, a, rays_dev, head_dev, n_rays);
    if (rc != HR_OK) return rc;
    const int64_t ns = n_rays * m->coarse->cfg.z_channels;
    rc = ensure_tape(m, ns, (hipStream_t)stream);
    if (rc != HR_OK) return rc;
    a.rows = rows_scratch_dev;
    a.d_rows = d_rows_dev;
    a.d_head = d_head_dev;
    a.tape = hr_tape_bind_rows(m->tape, ns);
    hr_launch_rows(m->coarse->cfg, a, (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}
