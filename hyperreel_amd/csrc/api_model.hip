// C ABI, the model's lifecycle: create, upload, finalize, update_config, reserve, options, occupancy, device_bytes, destroy.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hr_model.h"

namespace {

// z_vals channels read per sample: z (z_plane, euclidean_distance_unified, voxel_grid), origin xyz + radius
// (sphere/cylinder), origin xyz + resize xyz + raw offset + radius (sphere_new/cylinder_new)
int isect_z_channels(int t)
{
    if (t == HR_ISECT_SPHERE || t == HR_ISECT_CYLINDER || t == HR_ISECT_DEFORMABLE_VOXEL_GRID) return 4;
    if (t == HR_ISECT_SPHERE_NEW || t == HR_ISECT_CYLINDER_NEW) return 8;
    return 1;
}

int validate(const hr_config& c, bool coarse = false)
{
    if (c.ray_dim != 6 && c.ray_dim != 8) return fail(HR_E_INVALID, "ray_dim must be 6 or 8 (got %d)", c.ray_dim);
    if (c.n_groups < 1 || c.n_groups > HR_MAX_GROUPS) return fail(HR_E_INVALID, "n_groups out of range");
    for (int g = 0; g < c.n_groups; ++g)
        if (c.groups[g].pe_type == HR_PE_WINDOWED && c.groups[g].pe_n_freqs > HR_MAX_FREQS)
            return fail(HR_E_INVALID, "windowed positional encoding with more than %d frequencies", HR_MAX_FREQS);
    if (c.mlp_layers != 0) {   // 0: ZeroMLP (nlf/nets/mlp.py:14-33), the head is all zeros and samples sit on their anchors
        if (c.mlp_hidden != 64 && c.mlp_hidden != 128 && c.mlp_hidden != 256)
            return fail(HR_E_INVALID, "mlp_hidden must be 64, 128 or 256 (got %d)", c.mlp_hidden);
        // nn.LeakyReLU(0.01) (nlf/nets/mlp.py:149-154).  The split kernels evaluate it as max(v, slope v), which is the same function for a slope in [0, 1]
        if (!(c.leaky_slope >= 0.0f && c.leaky_slope <= 1.0f))
            return fail(HR_E_INVALID, "leaky_slope must be in [0, 1] (got %g)", (double)c.leaky_slope);
        if (c.mlp_layers < 2 || c.mlp_layers > HR_MAX_LAYERS) return fail(HR_E_INVALID, "mlp_layers must be 0 or in [2,%d]", HR_MAX_LAYERS);
        if (c.mlp_in < 1 || c.mlp_in > HR_MAX_MLP_IN) return fail(HR_E_INVALID, "mlp_in must be in [1,%d]", HR_MAX_MLP_IN);
        if (c.mlp_skip_mask & 1) return fail(HR_E_INVALID, "layer 0 cannot be a skip layer");
    }
    if (c.z_channels < 1 || c.z_channels > HR_KERNEL_MAX_Z) return fail(HR_E_INVALID, "z_channels must be in [1,%d]", HR_KERNEL_MAX_Z);
    if (c.preds_per_z < 1 || c.preds_per_z > 64) return fail(HR_E_INVALID, "preds_per_z out of range");
    const hr_head_field* fs[9] = {&c.f_z_vals, &c.f_isect_sigma, &c.f_offset_sigma, &c.f_point_offset, &c.f_color_scale,
                                  &c.f_color_shift, &c.f_spatial_flow, &c.f_color_scale_global, &c.f_color_shift_global};
    for (const hr_head_field* f : fs)
        if (f->offset >= 0 && f->offset + f->channels > c.preds_per_z) return fail(HR_E_INVALID, "head field exceeds preds_per_z");
    if (c.f_z_vals.offset < 0) return fail(HR_E_INVALID, "z_vals head is required");
    if (c.isect_type < HR_ISECT_Z_PLANE || c.isect_type > HR_ISECT_DEFORMABLE_VOXEL_GRID) return fail(HR_E_INVALID, "unknown isect_type %d", c.isect_type);
    if (c.f_z_vals.channels != isect_z_channels(c.isect_type))
        return fail(HR_E_INVALID, "z_vals needs %d channel(s) for intersect type %d (got %d)", isect_z_channels(c.isect_type),
                    c.isect_type, c.f_z_vals.channels);
    if (c.isect_type == HR_ISECT_VOXEL_GRID && c.z_channels % 3) return fail(HR_E_INVALID, "voxel_grid needs z_channels divisible by 3");
    if (c.isect_type == HR_ISECT_DEFORMABLE_VOXEL_GRID && (c.dvg_axes < 1 || c.dvg_axes > 3 || c.z_channels % c.dvg_axes))
        return fail(HR_E_INVALID, "deformable_voxel_grid needs 1..3 start normals dividing z_channels");
    if (c.contract_type < HR_CONTRACT_IDENTITY || c.contract_type > HR_CONTRACT_DONERF) return fail(HR_E_INVALID, "unknown contract_type");
    if (c.contract_type == HR_CONTRACT_DONERF && !(c.c_pow_fac > 0.0f && c.c_pow_power > 0.0f && c.c_pow_inv_power > 0.0f))
        return fail(HR_E_INVALID, "donerf contraction needs positive c_pow_fac / c_pow_power / c_pow_inv_power");
    if (c.contract_type == HR_CONTRACT_AFFINE)
        for (int i = 0; i < 3; ++i)
            if (c.c_aff_size[i] == 0.0f) return fail(HR_E_INVALID, "affine contraction with an empty box");
    if ((c.f_color_scale.offset >= 0) != (c.f_color_shift.offset >= 0)) return fail(HR_E_INVALID, "color_scale and color_shift come together");
    if ((c.f_color_scale_global.offset >= 0) != (c.f_color_shift_global.offset >= 0))
        return fail(HR_E_INVALID, "color_scale_global and color_shift_global come together");
    if (c.point_offset && (c.f_point_offset.offset < 0 || c.f_point_offset.channels != 3)) return fail(HR_E_INVALID, "point_offset head missing");
    if (c.advect && c.use_spatial_flow && (c.f_spatial_flow.offset < 0 || c.f_spatial_flow.channels != 3))
        return fail(HR_E_INVALID, "spatial_flow head missing");
    if (c.video && c.ray_dim != 8) return fail(HR_E_INVALID, "video net needs 8-column rays");
    if (c.video && !coarse && (!c.advect || c.num_keyframes < 1)) return fail(HR_E_INVALID, "video net needs the advect stage and num_keyframes >= 1");
    if (c.casc_in_z < 0 || (coarse && c.casc_in_z != 0)) return fail(HR_E_INVALID, "casc_in_z is set on the fine config of a cascade only");
    if (c.casc_in_z > 0) {
        if (c.z_channels % c.casc_in_z) return fail(HR_E_INVALID, "z_channels must be a multiple of casc_in_z");
        if (c.casc_n_inputs < 1 || c.casc_n_inputs > 4 || c.casc_row_dim < 1 || c.casc_row_dim > 8)
            return fail(HR_E_INVALID, "point_prediction rows: 1..4 inputs, 1..8 columns");
        int sum = 0;
        for (int i = 0; i < c.casc_n_inputs; ++i) {
            if (c.casc_input_kind[i] < HR_PIN_POINTS || c.casc_input_kind[i] > HR_PIN_TIMES || c.casc_input_dim[i] < 1 || c.casc_input_dim[i] > 3)
                return fail(HR_E_INVALID, "bad point_prediction input %d", i);
            sum += c.casc_input_dim[i];
        }
        if (sum != c.casc_row_dim) return fail(HR_E_INVALID, "casc_row_dim does not match the inputs");
        for (int g = 0; g < c.n_groups; ++g)
            if (c.groups[g].fn != HR_PARAM_IDENTITY || c.groups[g].end > c.casc_row_dim)
                return fail(HR_E_INVALID, "point_prediction params must be identity groups over the row's columns");
    }
    for (int i = 0; i < 3; ++i)
        if (c.grid[i] < 2) return fail(HR_E_INVALID, "grid size must be >= 2 on every axis");
    if (c.shading < HR_SHADING_RGB || c.shading > HR_SHADING_RGB_IDENTITY) return fail(HR_E_INVALID, "unknown shading %d", c.shading);
    if (hr_shading_is_time(c.shading)) {              // (the descriptor checks app_dim against 3 nb: hr_model_set_time_decode)
        if (!c.video) return fail(HR_E_INVALID, "shading RGBtLinear / RGBtFourier needs the keyframe net (a static net has no time basis)");
        if (c.app_dim < 6 || c.app_dim > 3 * HR_TIME_MAX_NB || c.app_dim % 3) return fail(HR_E_INVALID, "app_dim %d is not 3 nb of a time basis (frames_per_keyframe 1..%d)", c.app_dim, HR_TIME_MAX_FPK);
        if (c.casc_in_z > 0 || coarse) return fail(HR_E_INVALID, "shading RGBtLinear / RGBtFourier does not support point_prediction cascades");
    } else if (c.shading == HR_SHADING_RGB_IDENTITY) {
        if (c.video) return fail(HR_E_INVALID, "shading RGBIdentity on the keyframe net: the reference cannot build it");
        if (c.app_dim != 3) return fail(HR_E_INVALID, "app_dim must be 3 (RGBIdentity)");
        if (c.casc_in_z > 0 || coarse) return fail(HR_E_INVALID, "shading RGBIdentity does not support point_prediction cascades");
    } else if (c.shading == HR_SHADING_RGB ? c.app_dim != 3 : c.app_dim != 27) return fail(HR_E_INVALID, "app_dim must be 3 (RGB) or 27 (SH)");
    if (hr_shading_is_mlp(c.shading) && !coarse) {     // the colour network's kernels
        if (c.casc_in_z > 0) return fail(HR_E_INVALID, "MLP shading modes do not support point_prediction cascades");
        if (c.z_channels > HR_SHADE_MAX_Z) return fail(HR_E_INVALID, "MLP shading modes support at most %d samples per ray (got %d)", HR_SHADE_MAX_Z, c.z_channels);
    }
    if (c.mlp_precision < HR_MLP_FP32 || c.mlp_precision > HR_MLP_F16F8V) return fail(HR_E_INVALID, "unknown mlp_precision");
    if (c.mlp_layers != 0 && c.mlp_precision != HR_MLP_FP32 && c.mlp_precision != HR_MLP_AUTO && c.mlp_hidden != 256)      // (AUTO resolves to fp32 there)
        return fail(HR_E_INVALID, "the split (bf16x3 / f16x3) MLP needs mlp_hidden == 256");
    if (c.grid_dtype != HR_GRID_FP32 && c.grid_dtype != HR_GRID_FP16) return fail(HR_E_INVALID, "unknown grid_dtype");
    if (c.color_table_views < 0) return fail(HR_E_INVALID, "negative color_table_views");
    if (c.color_table_views > 0 && c.ray_dim != 8) return fail(HR_E_INVALID, "the colour table is indexed by rays[..., -2]: needs 8-column rays");
    return HR_OK;
}

// The live head columns of the model's configuration (hr_live_columns, hr_plan.h; HR_PRUNE=0 keeps every column) -> col_map, p_live, kcfg
void analyse_live_columns(hr_model* m)
{
    const char* e = getenv("HR_PRUNE");
    hr_live_columns(m->cfg, !(e && e[0] == '0'), m->col_map.col, &m->p_live, &m->kcfg);
}

}  // namespace

static int create_level(const hr_config* cfg, bool coarse, hr_model** out)
{
    if (!cfg || !out) return fail(HR_E_INVALID, "null argument");
    *out = nullptr;
    int rc = validate(*cfg, coarse);
    if (rc != HR_OK) return rc;
    int ndev = 0;
    HR_HIP(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail(HR_E_HIP, "no HIP device");
    hr_model* m = new hr_model();
    m->cfg = *cfg;
    m->is_coarse = coarse;
    {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) m->n_cus = prop.multiProcessorCount;
        if (m->n_cus < 1) m->n_cus = 256;
    }
    analyse_live_columns(m);
    {   // the kernels read the configuration from device memory
        if (m->kcfg_dev.alloc(sizeof(hr_config)) != hipSuccess) {
            delete m;
            return fail(HR_E_HIP, "hipMalloc of the device configuration failed");
        }
        (void)hipMemcpy(m->kcfg_dev, &m->kcfg, sizeof(hr_config), hipMemcpyHostToDevice);
    }
    const hr_config& c = m->cfg;
    size_t lds = 0;
    if (hr_sample_lds_refused(c, m->p_live, &lds)) {
        const int z = c.z_channels, pl = m->p_live;
        hr_model_destroy(m);                      // also releases the device configuration
        return fail(HR_E_INVALID, "z_channels %d x %d head columns need %zu bytes of LDS per workgroup (160 KiB available)", z, pl, lds);
    }
    char name[64];
    for (int l = 0; l < c.mlp_layers; ++l) {
        snprintf(name, sizeof(name), "mlp.%d.weight", l);
        m->expect[name] = sizeof(float) * (size_t)layer_out(c, l) * layer_in(c, l);
        snprintf(name, sizeof(name), "mlp.%d.bias", l);
        m->expect[name] = sizeof(float) * (size_t)layer_out(c, l);
    }
    if (coarse) {          // ray MLP + first intersect only: no grids
        *out = m;
        return HR_OK;
    }
    HrGridPlane pl[3];                     // the extents hr_model_finalize packs by; the uploads carry every channel of the configuration
    int ca_total = 0, n_app_sum = 0;
    (void)hr_plane_geometry(c, pl, &ca_total, &n_app_sum);
    for (int j = 0; j < 3; ++j) {
        const char* kinds[2] = {"density", "app"};
        const int nch[2] = {c.n_den[j], c.n_app[j]};
        for (int t = 0; t < 2; ++t) {
            snprintf(name, sizeof(name), c.video ? "%s_plane_space.%d" : "%s_plane.%d", kinds[t], j);
            m->expect[name] = sizeof(float) * (size_t)nch[t] * pl[j].ah * pl[j].aw;
            snprintf(name, sizeof(name), c.video ? "%s_plane_time.%d" : "%s_line.%d", kinds[t], j);
            m->expect[name] = sizeof(float) * (size_t)nch[t] * pl[j].bh * pl[j].bw;
        }
    }
    m->expect["basis_mat.weight"] = sizeof(float) * (size_t)c.app_dim * n_app_sum;
    if (c.color_table_views > 0) m->expect["color_embedding"] = sizeof(float) * (size_t)c.color_table_views * 12;
    *out = m;
    return HR_OK;
}

int hr_model_create(const hr_config* cfg, hr_model** out)
{
    if (cfg && cfg->casc_in_z != 0) return fail(HR_E_INVALID, "a cascade's fine config goes through hr_model_create_cascade");
    return create_level(cfg, false, out);
}

int hr_model_create_cascade(const hr_config* coarse, const hr_config* fine, hr_model** out)
{
    if (!coarse || !fine || !out) return fail(HR_E_INVALID, "null argument");
    *out = nullptr;
    if (fine->casc_in_z <= 0) return fail(HR_E_INVALID, "the fine config needs casc_in_z (samples of the coarse level)");
    if (fine->casc_in_z != coarse->z_channels) return fail(HR_E_INVALID, "casc_in_z %d != coarse z_channels %d", fine->casc_in_z, coarse->z_channels);
    if (fine->ray_dim != coarse->ray_dim) return fail(HR_E_INVALID, "both levels read the same rays: ray_dim must agree");
    hr_model* c = nullptr;
    int rc = create_level(coarse, true, &c);
    if (rc != HR_OK) return rc;
    hr_model* m = nullptr;
    rc = create_level(fine, false, &m);
    if (rc != HR_OK) {
        hr_model_destroy(c);
        return rc;
    }
    m->coarse.reset(c);
    *out = m;
    return HR_OK;
}

static const char* const DENSITY_BASIS = "basis_mat_density.weight";

int hr_model_set_time_decode(hr_model* m, const hr_time_decode* d)
{
    if (!m || !d) return fail(HR_E_INVALID, "null argument");
    const hr_config& c = m->cfg;
    if (m->is_coarse || m->coarse || !c.video) return fail(HR_E_INVALID, "hr_model_set_time_decode: the model is not a keyframe net (RGBt* / Density* modes on the static net)");
    if (d->density_mode < HR_DENSITY_PLAIN || d->density_mode > HR_DENSITY_FOURIER) return fail(HR_E_INVALID, "unknown density_mode %d", d->density_mode);
    if (!hr_shading_is_time(c.shading) && d->density_mode == HR_DENSITY_PLAIN)
        return fail(HR_E_INVALID, "hr_model_set_time_decode: the model has neither an RGBt* shading nor a Density* mode");
    if (hr_shading_is_mlp(c.shading) && d->density_mode != HR_DENSITY_PLAIN)
        return fail(HR_E_INVALID, "a Density* mode together with an MLP shading mode (MLP_Fea / MLP)");
    if (d->frames_per_keyframe < 1 || d->frames_per_keyframe > HR_TIME_MAX_FPK)
        return fail(HR_E_INVALID, "frames_per_keyframe must be in [1,%d] (got %d)", HR_TIME_MAX_FPK, d->frames_per_keyframe);
    if (d->num_frames < 1) return fail(HR_E_INVALID, "num_frames must be positive (got %d)", d->num_frames);
    if (hr_shading_is_time(c.shading) && c.app_dim != hr_time_app_dim(c.shading, d->frames_per_keyframe))
        return fail(HR_E_INVALID, "data_dim_color %d contradicts 3 nb = %d (frames_per_keyframe %d)", c.app_dim, hr_time_app_dim(c.shading, d->frames_per_keyframe),
                    d->frames_per_keyframe);
    if (m->finalized || !m->raw.empty()) return fail(HR_E_STATE, "hr_model_set_time_decode comes between hr_model_create and the first upload");
    m->expect.erase(DENSITY_BASIS);
    if (d->density_mode != HR_DENSITY_PLAIN) {
        size_t lds = 0;
        if (hr_sample_lds_refused(c, m->p_live, HR_SAMPLE_TIME_DENSITY, &lds))
            return fail(HR_E_INVALID, "z_channels %d x %d head columns with a density row need %zu bytes of LDS per workgroup (160 KiB available)", c.z_channels, m->p_live, lds);
        const int nb = hr_time_nb(d->density_mode == HR_DENSITY_FOURIER, d->frames_per_keyframe);
        m->expect[DENSITY_BASIS] = sizeof(float) * (size_t)nb * (c.n_den[0] + c.n_den[1] + c.n_den[2]);
    }
    m->time_desc = *d;
    m->time_set = true;
    return HR_OK;
}

// a density mode's basis_mat_density -> the column-major copy and the slot table of the density row (hr_plan.h: hr_time_density_slots), at finalize
static int pack_density_basis(hr_model* m)
{
    const hr_config& c = m->cfg;
    const int nb = hr_time_nb(m->time_desc.density_mode == HR_DENSITY_FOURIER, m->time_desc.frames_per_keyframe);
    const int n_cols = c.n_den[0] + c.n_den[1] + c.n_den[2], ld = (nb + 3) & ~3;
    std::vector<float> w((size_t)nb * n_cols), wt((size_t)(n_cols > 0 ? n_cols : 1) * ld, 0.0f);
    if (!w.empty()) HR_HIP(hipMemcpy(w.data(), m->raw[DENSITY_BASIS].p, w.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int col = 0; col < n_cols; ++col)
        for (int r = 0; r < nb; ++r) wt[(size_t)col * ld + r] = w[(size_t)r * n_cols + col];
    // the plan the launches will take (the class does not depend on the ray count or on hr_render_frame's line form)
    const HrSampleFormPlan T = hr_sample_form_plan(m->kcfg, m->planes, m->ca_total, hr_head_quads(c, m->p_live), rows_per_ray(c), 1, false, {HR_SAMPLE_TIME_DENSITY, true, false});
    std::vector<int> sc((size_t)T.d_slots, -1);
    int slot = 0, col0 = 0;
    for (int j = 0; j < 3; ++j) {       // density slot order: plane pair after plane pair, 4 cd4 each (the classes: row 0 of the matrix-shaped block)
        for (int i = 0; i < 4 * m->planes[j].cd4; ++i) sc[slot + i] = i < c.n_den[j] ? col0 + i : -1;
        slot += 4 * m->planes[j].cd4;
        col0 += c.n_den[j];
    }
    m->dbasis_t.reset();
    m->dslot_col.reset();
    HR_HIP(m->dbasis_t.alloc(wt.size() * sizeof(float)));
    HR_HIP(hipMemcpy(m->dbasis_t, wt.data(), wt.size() * sizeof(float), hipMemcpyHostToDevice));
    HR_HIP(m->dslot_col.alloc((sc.empty() ? 1 : sc.size()) * sizeof(int)));
    if (!sc.empty()) HR_HIP(hipMemcpy(m->dslot_col, sc.data(), sc.size() * sizeof(int), hipMemcpyHostToDevice));
    m->d_ld = ld;
    m->d_slots = T.d_slots;
    m->packed_bytes += (int64_t)(wt.size() * sizeof(float) + sc.size() * sizeof(int));
    return HR_OK;
}

static const char* const SHADE_TENSORS[6] = {"renderModule.mlp.0.weight", "renderModule.mlp.0.bias", "renderModule.mlp.2.weight",
                                             "renderModule.mlp.2.bias",   "renderModule.mlp.4.weight", "renderModule.mlp.4.bias"};

int hr_model_set_shading_mlp(hr_model* m, const hr_shading_mlp* d)
{
    if (!m || !d) return fail(HR_E_INVALID, "null argument");
    if (m->is_coarse || !hr_shading_is_mlp(m->cfg.shading))
        return fail(HR_E_INVALID, "hr_model_set_shading_mlp: the model's shading is not HR_SHADING_MLP_FEA / HR_SHADING_MLP");
    if (d->view_pe < 0 || d->view_pe > HR_SHADE_MAX_PE) return fail(HR_E_INVALID, "view_pe must be in [0,%d] (got %d)", HR_SHADE_MAX_PE, d->view_pe);
    if (m->cfg.shading == HR_SHADING_MLP_FEA && (d->fea_pe < 0 || d->fea_pe > HR_SHADE_MAX_PE))
        return fail(HR_E_INVALID, "fea_pe must be in [0,%d] (got %d)", HR_SHADE_MAX_PE, d->fea_pe);
    if (d->feature_c < 1 || d->feature_c > HR_SHADE_MAX_C) return fail(HR_E_INVALID, "feature_c must be in [1,%d] (got %d)", HR_SHADE_MAX_C, d->feature_c);
    for (const char* name : SHADE_TENSORS) { m->expect.erase(name); m->raw.erase(name); }
    m->shade_net = hr_shade_net(m->cfg.shading, *d);
    for (int l = 0; l < 3; ++l) {
        const HrShadeLayer L = hr_shade_layer(m->shade_net, l);
        m->expect[SHADE_TENSORS[2 * l]] = sizeof(float) * (size_t)L.N * L.K;
        m->expect[SHADE_TENSORS[2 * l + 1]] = sizeof(float) * (size_t)L.N;
    }
    m->shade_set = true;
    m->finalized = false;
    return HR_OK;
}

// the colour network's tensors -> the shading kernel's tiles (hr_shade.h), at finalize
static int pack_shading(hr_model* m)
{
    for (int l = 0; l < 3; ++l) {
        const HrShadeLayer L = hr_shade_layer(m->shade_net, l);
        std::vector<float> w((size_t)L.N * L.K), b((size_t)L.N), tiles, bias;
        HR_HIP(hipMemcpy(w.data(), m->raw[SHADE_TENSORS[2 * l]].p, w.size() * sizeof(float), hipMemcpyDeviceToHost));
        HR_HIP(hipMemcpy(b.data(), m->raw[SHADE_TENSORS[2 * l + 1]].p, b.size() * sizeof(float), hipMemcpyDeviceToHost));
        hr_shade_pack_layer(L, w.data(), b.data(), tiles, bias);
        HR_HIP(m->shade_w[l].alloc(tiles.size() * sizeof(float)));
        HR_HIP(hipMemcpy(m->shade_w[l], tiles.data(), tiles.size() * sizeof(float), hipMemcpyHostToDevice));
        HR_HIP(m->shade_b[l].alloc(bias.size() * sizeof(float)));
        HR_HIP(hipMemcpy(m->shade_b[l], bias.data(), bias.size() * sizeof(float), hipMemcpyHostToDevice));
        m->packed_bytes += (int64_t)((tiles.size() + bias.size()) * sizeof(float));
    }
    return HR_OK;
}

int hr_model_upload(hr_model* m, const char* name, const void* ptr, size_t bytes)
{
    if (!m || !name) return fail(HR_E_INVALID, "null argument");
    std::string key = name;
    if (m->coarse) {                      // cascade: mlp.* is the coarse ray MLP, mlp1.* the point MLP of this level
        if (key.compare(0, 4, "mlp.") == 0) {
            m->finalized = false;
            return hr_model_upload(m->coarse.get(), name, ptr, bytes);
        }
        if (key.compare(0, 5, "mlp1.") == 0) key = "mlp." + key.substr(5);
    }
    name = key.c_str();
    auto it = m->expect.find(name);
    if (it == m->expect.end()) return fail(HR_E_INVALID, "unknown tensor name '%s'", name);
    if (bytes != it->second) return fail(HR_E_INVALID, "tensor '%s': expected %zu bytes, got %zu", name, it->second, bytes);
    if (bytes > 0 && !ptr) return fail(HR_E_INVALID, "tensor '%s': null data", name);
    DevBuf& b = m->raw[name];
    if (b.bytes != bytes || (bytes > 0 && !b.p)) {
        b.p.reset();
        b.bytes = bytes;
        if (bytes > 0) HR_HIP(b.p.alloc(bytes));
    }
    if (bytes > 0) HR_HIP(hipMemcpy(b.p, ptr, bytes, hipMemcpyDefault));
    m->finalized = false;
    return HR_OK;
}

// The end of hr_model_finalize: the default workspace, then the MLP's new state into the model with its margins measured (set_mlp_state,
// which first synchronises the device -- the tiles are fresh --, so whatever finalize launched is done as well).  Finalized only if
// all of it succeeded.
static int finalize_end(hr_model* m, HrMlpState& mlp)
{
    HR_HIP(hipGetLastError());
    if (m->chunk == 0 && !m->is_coarse) {
        int64_t chunk = hr_default_chunk(hr_head_quads(m->cfg, m->p_live), rows_per_ray(m->cfg));
        if (hr_shading_is_mlp(m->cfg.shading))
            chunk = hr_shade_default_chunk(chunk, hr_shade_plan(m->cfg.shading, m->shade_net.view_pe, m->shade_net.fea_pe, m->shade_net.feature_c, m->cfg.z_channels));
        const int rc = hr_model_reserve(m, chunk);
        if (rc != HR_OK) return rc;
    }
    const int rc = set_mlp_state(m, mlp, nullptr);
    m->finalized = rc == HR_OK;
    return rc;
}

int hr_model_finalize(hr_model* m)
{
    if (!m) return fail(HR_E_INVALID, "null argument");
    m->finalized = false;              // until all of it has succeeded (finalize_end)
    if (m->coarse) {
        int rc = hr_model_finalize(m->coarse.get());
        if (rc != HR_OK) return rc;
    }
    const hr_config& c = m->cfg;
    if (hr_shading_is_mlp(c.shading) && !m->is_coarse) {
        if (!m->shade_set) return fail(HR_E_STATE, "MLP shading mode: hr_model_set_shading_mlp has not been called");
        for (const char* name : SHADE_TENSORS)
            if (m->raw.find(name) == m->raw.end()) return fail(HR_E_STATE, "MLP shading mode: tensor '%s' was never uploaded", name);
    }
    if (hr_shading_is_time(c.shading) && !m->time_set)
        return fail(HR_E_STATE, "shading RGBtLinear / RGBtFourier: hr_model_set_time_decode has not been called");
    for (auto& kv : m->expect)
        if (m->raw.find(kv.first) == m->raw.end())
            return fail(HR_E_MISSING, "tensor '%s%s' was never uploaded", (m->coarse && kv.first.compare(0, 4, "mlp.") == 0) ? "mlp1." : "",
                        (m->coarse && kv.first.compare(0, 4, "mlp.") == 0) ? kv.first.c_str() + 4 : kv.first.c_str());
    m->packed_bytes = 0;
    char name[64];

    // ---- MLP: which arithmetic (the fp16 split needs every activation below 65504), then MFMA operand tiles -- built aside; they reach the
    // model at the end, once the workspace their margins are measured with exists.  (A re-finalize: the tiles and rays made from the
    // weights before go first, as the grids do below)
    if (!m->flags) HR_HIP(m->flags.alloc(sizeof(unsigned)));
    HR_HIP(hipMemset(m->flags, 0, sizeof(unsigned)));
    m->mlp.pack.reset();
    m->mlp.calib.reset();
    HrMlpState mlp;
    {
        const int rc = build_mlp_state(m, nullptr, 0, nullptr, false, mlp);
        if (rc != HR_OK) return rc;
    }
    if (m->is_coarse) return finalize_end(m, mlp);      // coarse level of a cascade: no grids

    // ---- grids: channel-last texels, density | appearance interleaved per plane pair
    const bool cols_ok = hr_plane_geometry(c, m->planes, &m->ca_total, &m->n_basis_cols);
    for (int j = 0; j < 3; ++j) {
        HrGridPlane& g = m->planes[j];
        m->grid_a[j].reset();
        m->grid_b[j].reset();
        const int half = (c.grid_dtype == HR_GRID_FP16), tex = g.tex, nd = c.n_den[j], na = g.app_real;
        if (tex == 0) continue;
        const size_t esz = half ? 2 : sizeof(float);
        const size_t a_bytes = esz * (size_t)g.aw * g.ah * tex;
        const size_t b_bytes = esz * (size_t)g.bw * g.bh * tex;
        // the gathers address texels by 32-bit BYTE offsets (and the class-specialised one marks a masked sample by the offset 0xffffffff)
        if (a_bytes >= ((size_t)1 << 32) || b_bytes >= ((size_t)1 << 32))
            return fail(HR_E_INVALID, "plane pair %d: %zu / %zu bytes -- a feature plane must stay below 4 GiB (32-bit texel offsets)", j, a_bytes, b_bytes);
        HR_HIP(m->grid_a[j].alloc(a_bytes));
        HR_HIP(m->grid_b[j].alloc(b_bytes));
        HR_HIP(hipMemset(m->grid_a[j], 0, a_bytes));
        HR_HIP(hipMemset(m->grid_b[j], 0, b_bytes));
        const char* an = c.video ? "plane_space" : "plane";
        const char* bn = c.video ? "plane_time" : "line";
        snprintf(name, sizeof(name), "density_%s.%d", an, j);
        hr_launch_interleave(m->raw[name].p, m->grid_a[j], half, nd, g.ah, g.aw, tex, 0, nullptr);
        snprintf(name, sizeof(name), "app_%s.%d", an, j);
        hr_launch_interleave(m->raw[name].p, m->grid_a[j], half, na, g.ah, g.aw, tex, 4 * g.cd4, nullptr);
        snprintf(name, sizeof(name), "density_%s.%d", bn, j);
        hr_launch_interleave(m->raw[name].p, m->grid_b[j], half, nd, g.bh, g.bw, tex, 0, nullptr);
        snprintf(name, sizeof(name), "app_%s.%d", bn, j);
        hr_launch_interleave(m->raw[name].p, m->grid_b[j], half, na, g.bh, g.bw, tex, 4 * g.cd4, nullptr);
        g.a = m->grid_a[j];
        g.b = m->grid_b[j];
        m->packed_bytes += (int64_t)(a_bytes + b_bytes);
    }
    // basis_mat columns follow the reference's torch.cat over the sampled planes.  For the
    // video net a skipped plane pair contributes no columns; its n_app must then be 0 too
    // (otherwise the reference itself fails with a shape error in basis_mat).
    if (!cols_ok) return fail(HR_E_INVALID, "video net: n_lamb_sh must be 0 wherever n_lamb_sigma is 0");
    const int n_app_sum = m->n_basis_cols;
    m->basis.reset();
    {
        const size_t bytes = m->raw["basis_mat.weight"].bytes;
        HR_HIP(m->basis.alloc(bytes > 0 ? bytes : 16));
        if (bytes > 0) HR_HIP(hipMemcpy(m->basis, m->raw["basis_mat.weight"].p, bytes, hipMemcpyDeviceToDevice));
        m->packed_bytes += (int64_t)bytes;
        // column-major copy + the slot -> column map (what hr_fill_decode used to recompute per ray and slot)
        const int AD = c.app_dim, ld = (AD + 3) & ~3;
        std::vector<float> bm((size_t)AD * n_app_sum), bt((size_t)(n_app_sum > 0 ? n_app_sum : 1) * ld, 0.0f);
        if (bytes > 0) HR_HIP(hipMemcpy(bm.data(), m->raw["basis_mat.weight"].p, bytes, hipMemcpyDeviceToHost));
        for (int col = 0; col < n_app_sum; ++col)
            for (int r = 0; r < AD; ++r) bt[(size_t)col * ld + r] = bm[(size_t)r * n_app_sum + col];
        std::vector<int> sc(m->ca_total > 0 ? m->ca_total : 1, -1);
        for (int j = 0; j < 3; ++j)
            if (m->planes[j].ca4 > 0)
                for (int rel = 0; rel < m->planes[j].app_real; ++rel) sc[m->planes[j].app_off + rel] = m->planes[j].app_real_off + rel;
        m->basis_t.reset();
        m->slot_col.reset();
        HR_HIP(m->basis_t.alloc(bt.size() * sizeof(float)));
        HR_HIP(hipMemcpy(m->basis_t, bt.data(), bt.size() * sizeof(float), hipMemcpyHostToDevice));
        HR_HIP(m->slot_col.alloc(sc.size() * sizeof(int)));
        HR_HIP(hipMemcpy(m->slot_col, sc.data(), sc.size() * sizeof(int), hipMemcpyHostToDevice));
        m->basis_ld = ld;
    }
    if (hr_shading_is_mlp(c.shading)) {
        const int rc = pack_shading(m);
        if (rc != HR_OK) return rc;
    }
    if (hr_model_time_density(m)) {
        const int rc = pack_density_basis(m);
        if (rc != HR_OK) return rc;
    }
    // hr_render_frame: one line per time plane for the frame's blended keyframe rows (float32 texels)
    for (int j = 0; j < 3; ++j) {
        m->frame_line[j].reset();
        const HrGridPlane& p = m->planes[j];
        if (c.video && c.grid_dtype != HR_GRID_FP16 && p.bw > 1 && p.cd4 + p.ca4 > 0)
            HR_HIP(m->frame_line[j].alloc(sizeof(float) * (size_t)p.bw * p.tex));
    }
    return finalize_end(m, mlp);
}

// the configuration with every schedule-dependent constant blanked: what hr_model_update_config may not change
static hr_config structure_of(const hr_config& in)
{
    hr_config c = in;
    hr_act* acts[] = {&c.f_z_vals.act, &c.f_isect_sigma.act, &c.f_offset_sigma.act, &c.f_point_offset.act, &c.f_color_scale.act,
                      &c.f_color_shift.act, &c.f_spatial_flow.act, &c.f_color_scale_global.act, &c.f_color_shift_global.act,
                      &c.z_act, &c.flow_act, &c.offset_act, &c.color_table_t_act, &c.color_table_s_act};
    for (hr_act* a : acts) { a->outer = 0.0f; a->add = 0.0f; }
    c.isect_mask_off = 0;                          // the near/far mask is dropped after mask.stop_iters (intersect/base.py:104-108)
    for (int g = 0; g < HR_MAX_GROUPS; ++g)
        for (int j = 0; j < HR_MAX_FREQS; ++j) c.groups[g].pe_weight[j] = 0.0f;
    return c;
}

int hr_model_update_config(hr_model* m, const hr_config* cfg, void* stream)
{
    if (!m || !cfg) return fail(HR_E_INVALID, "null argument");
    if (!m->finalized) return fail(HR_E_STATE, "hr_model_update_config before hr_model_finalize");
    if (m->coarse || m->is_coarse) return fail(HR_E_INVALID, "hr_model_update_config: cascades are re-created instead");
    const hr_config a = structure_of(m->cfg), b = structure_of(*cfg);
    if (memcmp(&a, &b, sizeof(hr_config)) != 0)
        return fail(HR_E_INVALID, "hr_model_update_config: the configurations differ in more than activation / PE schedule constants");
    HR_HIP(hipStreamSynchronize((hipStream_t)stream));      // launches in flight still read the device copies
    m->cfg = *cfg;
    analyse_live_columns(m);                                  // same live columns (structure unchanged): rebuilds kcfg
    if (m->kcfg_dev) HR_HIP(hipMemcpy(m->kcfg_dev, &m->kcfg, sizeof(hr_config), hipMemcpyHostToDevice));
    if (m->ucfg_dev) HR_HIP(hipMemcpy(m->ucfg_dev, &m->cfg, sizeof(hr_config), hipMemcpyHostToDevice));
    m->mlp.band_stale = true;                                   // the activations' constants feed the distances: measured again before the next render
    return HR_OK;
}

int hr_model_reserve(hr_model* m, int64_t rays_per_chunk)
{
    if (!m) return fail(HR_E_INVALID, "null argument");
    if (rays_per_chunk < 64) rays_per_chunk = 64;
    rays_per_chunk = (rays_per_chunk + 63) & ~(int64_t)63;
    if (rays_per_chunk == m->chunk && m->head) return HR_OK;
    m->head.reset();
    m->rows.reset();
    m->chunk = 0;
    const size_t n_rows = (size_t)rays_per_chunk * rows_per_ray(m->cfg);      // a multiple of 64
    const size_t nq = (size_t)hr_head_quads(m->cfg, m->p_live);
    const size_t bytes = sizeof(float) * n_rows * nq * 4;                        // HQ layout over rows
    HR_HIP(m->head.alloc(bytes));
    if (m->cfg.mlp_layers == 0) HR_HIP(hipMemset(m->head, 0, bytes));   // ZeroMLP: written once, only ever read
    m->shade_rows.reset();
    m->shade_rgb.reset();
    if (hr_shading_is_mlp(m->cfg.shading) && !m->is_coarse) {           // hr_shade_plan's ws_bytes_per_ray
        const size_t samples = (size_t)rays_per_chunk * m->cfg.z_channels;
        HR_HIP(m->shade_rows.alloc(sizeof(float) * samples * HR_SHADE_ROW));
        HR_HIP(m->shade_rgb.alloc(sizeof(float) * samples * 3));
    }
    if (m->coarse) {
        int rc = hr_model_reserve(m->coarse.get(), rays_per_chunk);
        if (rc != HR_OK) return rc;
        HR_HIP(m->rows.alloc(sizeof(float) * n_rows * m->cfg.casc_row_dim));
    }
    m->chunk = rays_per_chunk;
    // verified fast path: the list of rays the second pass renders again.  The buffer holds 4 M entries (16 MB); a call uses
    // hr_redo_list_cap of them (max(32 768, n_rays / 16); measured: 0.01 - 2.5 % of a frame's rays are listed; the calibration gives the fast path up above 5 %)
    // and walks them in slices of the chunk's head workspace.  Beyond that the kernels raise bit 2 of the status word (HR_OPT_REDO_OVERFLOW)
    m->redo_list.reset();
    m->wide_list.reset();
    m->redo_cap = 1 << 22;
    m->wide_cap = hr_wide_cap(rays_per_chunk);
    HR_HIP(m->redo_list.alloc(sizeof(int) * (size_t)m->redo_cap));
    HR_HIP(m->wide_list.alloc(sizeof(int) * (size_t)m->wide_cap));
    if (!m->redo_count) {
        HR_HIP(m->redo_count.alloc(4 * sizeof(unsigned)));
        HR_HIP(hipMemset(m->redo_count, 0, 4 * sizeof(unsigned)));
    }
    return HR_OK;
}

int hr_model_set_occupancy(hr_model* m, const float* volume_dev, const int32_t n[3], const float aabb[6], void* stream)
{
    if (!m) return fail(HR_E_INVALID, "null model");
    if (m->is_coarse) return fail(HR_E_INVALID, "the coarse level of a cascade has no colour net");
    HR_HIP(hipStreamSynchronize((hipStream_t)stream));          // launches in flight may still read the old volume
    m->occ.reset();
    m->occ_cells.reset();
    if (!volume_dev) return HR_OK;
    if (!n || !aabb || n[0] < 1 || n[1] < 1 || n[2] < 1) return fail(HR_E_INVALID, "occupancy volume without a size / box");
    for (int i = 0; i < 3; ++i)
        if (!(aabb[3 + i] > aabb[i])) return fail(HR_E_INVALID, "empty occupancy box");
    const size_t bytes = sizeof(float) * (size_t)n[0] * n[1] * n[2];
    HR_HIP(m->occ.alloc(bytes));
    HR_HIP(hipMemcpy(m->occ, volume_dev, bytes, hipMemcpyDefault));
    for (int i = 0; i < 3; ++i) {
        m->occ_n[i] = n[i];
        m->occ_lo[i] = aabb[i];
        m->occ_inv[i] = (1.0f / (aabb[3 + i] - aabb[i])) * 2.0f;        // AlphaGridMask: invgridSize = 1.0 / aabbSize * 2
    }
    // cell table: a 0/1 volume (what updateAlphaMask stores) sampled strictly inside a lattice cell is > 0 exactly when one of
    // the cell's 8 corners is set
    if (n[0] > 1 && n[1] > 1 && n[2] > 1) {
        const size_t W = n[0], H = n[1], D = n[2];
        std::vector<float> v(W * H * D);
        HR_HIP(hipMemcpy(v.data(), m->occ, bytes, hipMemcpyDeviceToHost));
        bool binary = true;
        for (float x : v) if (x != 0.0f && x != 1.0f) { binary = false; break; }
        if (binary) {
            const size_t cells = (W - 1) * (H - 1) * (D - 1);
            std::vector<unsigned> bits((cells + 31) / 32, 0u);
            for (size_t z = 0; z + 1 < D; ++z)
                for (size_t y = 0; y + 1 < H; ++y)
                    for (size_t x = 0; x + 1 < W; ++x) {
                        bool any = false;
                        for (int c = 0; c < 8 && !any; ++c) any = v[((z + (c >> 2)) * H + y + ((c >> 1) & 1)) * W + x + (c & 1)] != 0.0f;
                        if (any) {
                            const size_t cell = (z * (H - 1) + y) * (W - 1) + x;
                            bits[cell >> 5] |= 1u << (cell & 31);
                        }
                    }
            HR_HIP(m->occ_cells.alloc(bits.size() * sizeof(unsigned)));
            HR_HIP(hipMemcpy(m->occ_cells, bits.data(), bits.size() * sizeof(unsigned), hipMemcpyHostToDevice));
        }
    }
    return HR_OK;
}

int hr_model_set_option(hr_model* m, int32_t option, int32_t value)
{
    if (!m) return fail(HR_E_INVALID, "null model");
    if (option == HR_OPT_FRAME_KERNEL) {
        if (value < 0 || value > 2) return fail(HR_E_INVALID, "HR_OPT_FRAME_KERNEL takes 0, 1 or 2");
        m->opt_frame_kernel = value;
    } else if (option == HR_OPT_TRAIN_DETERMINISTIC) {
        if (value != 0 && value != 1) return fail(HR_E_INVALID, "HR_OPT_TRAIN_DETERMINISTIC takes 0 or 1");
        m->opt_train_det = value;
    } else if (option == HR_OPT_SAMPLE_WAVES) {
        if (value != 0 && value != 4 && value != 8) return fail(HR_E_INVALID, "HR_OPT_SAMPLE_WAVES takes 0 (the plan's default), 4 or 8");
        m->opt_sample_waves = value;
    } else {
        return fail(HR_E_INVALID, "unknown or read-only option %d", option);
    }
    return HR_OK;
}

int hr_model_get_option(hr_model* m, int32_t option, int32_t* value)
{
    if (!m || !value) return fail(HR_E_INVALID, "null argument");
    if (option == HR_OPT_FRAME_KERNEL) *value = m->opt_frame_kernel;
    else if (option == HR_OPT_SAMPLE_WAVES) *value = m->opt_sample_waves;
    else if (option == HR_OPT_TRAIN_DETERMINISTIC) *value = m->opt_train_det;
    else if (option == HR_OPT_CHUNK_RAYS) *value = (int32_t)m->chunk;
    else if (option == HR_OPT_MLP_PRECISION_ACTIVE || option == HR_OPT_MLP_CALIBRATED || option == HR_OPT_MLP_OVERFLOW || option == HR_OPT_MLP_F8_SATURATED ||
             option == HR_OPT_MLP_VERIFIED || option == HR_OPT_REDO_OVERFLOW || option == HR_OPT_REDO_COUNT || option == HR_OPT_WIDE_COUNT) {
        if (!m->finalized) return fail(HR_E_STATE, "hr_model_finalize has not been called");
        if (option == HR_OPT_MLP_PRECISION_ACTIVE) *value = m->mlp.active_precision;
        else if (option == HR_OPT_MLP_CALIBRATED) *value = m->mlp.calibrated;
        else if (option == HR_OPT_MLP_VERIFIED) *value = m->mlp.verified;
        else if (option == HR_OPT_REDO_COUNT || option == HR_OPT_WIDE_COUNT) {
            unsigned n = 0;
            if (m->redo_count) HR_HIP(hipMemcpy(&n, m->redo_count + (option == HR_OPT_REDO_COUNT ? 1 : 3), sizeof(unsigned), hipMemcpyDeviceToHost));      // the pass's copy
            *value = (int32_t)n;
        } else if (option == HR_OPT_REDO_OVERFLOW) {
            unsigned f = 0;
            HR_HIP(hipMemcpy(&f, m->flags, sizeof(unsigned), hipMemcpyDeviceToHost));
            *value = (int32_t)((f >> 2) & 1u);
        } else {
            unsigned f = 0;
            HR_HIP(hipMemcpy(&f, m->flags, sizeof(unsigned), hipMemcpyDeviceToHost));
            if (m->coarse) {
                unsigned g = 0;
                HR_HIP(hipMemcpy(&g, m->coarse->flags, sizeof(unsigned), hipMemcpyDeviceToHost));
                f |= g;
            }
            *value = (int32_t)(option == HR_OPT_MLP_OVERFLOW ? (f & 1u) : ((f >> 1) & 1u));
        }
    } else if (option == HR_OPT_FRAME_KERNEL_ACTIVE) {
        if (!m->finalized) return fail(HR_E_STATE, "hr_model_finalize has not been called");
        *value = hr_render_route(render_route_facts(m, 64, false, false)).route == HR_ROUTE_FRAME ? 1 : 0;
    } else return fail(HR_E_INVALID, "unknown option %d", option);
    return HR_OK;
}

int64_t hr_model_device_bytes(const hr_model* m)
{
    if (!m) return 0;
    int64_t raw = 0;
    for (auto& kv : m->raw) raw += (int64_t)kv.second.bytes;
    return raw + m->packed_bytes + (m->mlp.pack ? m->mlp.pack->bytes : 0) + (int64_t)sizeof(float) * m->chunk * m->cfg.z_channels * m->p_live +
           (m->rows ? (int64_t)sizeof(float) * m->chunk * m->cfg.casc_in_z * m->cfg.casc_row_dim : 0) +
           (m->shade_rows ? (int64_t)sizeof(float) * m->chunk * m->cfg.z_channels * (HR_SHADE_ROW + 3) : 0) + hr_model_device_bytes(m->coarse.get());
}

void hr_model_destroy(hr_model* m)
{
    delete m;        // the members free their device memory, the coarse level of a cascade included
}
