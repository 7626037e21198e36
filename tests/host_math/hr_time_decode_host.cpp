// TEST-ONLY host build of hyperreel_amd/csrc/hr_time_decode.h (the time-dependent decode modes' basis, fold and activation) and of
// hr_plan.h's time-kernel plan, for tests/test_time_decode_host.py.  Nothing in the product links or loads this file.
#include "../../hyperreel_amd/csrc/hr_plan.h"

extern "C" {

int td_sizeof_config() { return (int)sizeof(hr_config); }
int td_sizeof_desc() { return (int)sizeof(hr_time_decode); }
int td_max_fpk() { return HR_TIME_MAX_FPK; }
int td_nb(int fourier, int fpk) { return hr_time_nb(fourier, fpk); }
int td_app_dim(int shading, int fpk) { return hr_time_app_dim(shading, fpk); }
float td_scale(int k, int f) { return hr_time_scale(k, f); }
// time_offset of a ray as the kernels form it: t - hr_base_time
float td_offset(const hr_config* c, float t) { return c->advect ? t - hr_base_time(*c, t) : 0.0f; }

// out (n, nb): the basis of n rays
void td_basis(int fourier, int fpk, float fac, const float* t, const float* off, long long n, float* out)
{
    const int nb = hr_time_nb(fourier, fpk);
    for (long long i = 0; i < n; ++i)
        for (int j = 0; j < nb; ++j) out[i * nb + j] = hr_time_basis(fourier, fpk, t[i], off[i], fac, j);
}
// out (n, groups, cols): weight (groups * nb, cols) row-major folded with each ray's basis, through a column-major copy as the kernels do
void td_fold(int fourier, int fpk, float fac, const float* t, const float* off, long long n, const float* weight, int groups, int cols, float* out)
{
    const int nb = hr_time_nb(fourier, fpk), rows = groups * nb;
    float* wt = new float[(size_t)rows * cols];
    for (int c = 0; c < cols; ++c)
        for (int r = 0; r < rows; ++r) wt[(size_t)c * rows + r] = weight[(size_t)r * cols + c];
    for (long long i = 0; i < n; ++i)
        for (int g = 0; g < groups; ++g)
            for (int c = 0; c < cols; ++c)
                out[(i * groups + g) * cols + c] = hr_time_fold(fourier, fpk, t[i], off[i], fac, wt + (size_t)c * rows + g * nb, 1);
    delete[] wt;
}
float td_color(int shading, float pre) { return hr_time_color(shading, pre); }
int td_family(int shading) { return (hr_shading_is_time(shading) ? 1 : 0) | (hr_shading_is_time_family(shading) ? 2 : 0) | (hr_shading_relu_half(shading) ? 4 : 0); }

// out = {zp, pclass, all_lines, big_lds, blocks, lds, d_slots, d_off, per_ray_M, refused (density), refused bytes}
void td_plan(const hr_config* c, int p_live, long long n_rays, int density, long long* out)
{
    HrGridPlane pl[3];
    int ca_total = 0, n_cols = 0;
    (void)hr_plane_geometry(*c, pl, &ca_total, &n_cols);
    const HrSampleForm form = {density ? HR_SAMPLE_TIME_DENSITY : HR_SAMPLE_TIME, true, false};
    const HrSampleFormPlan T = hr_sample_form_plan(*c, pl, ca_total, hr_head_quads(*c, p_live), rows_per_ray(*c), n_rays, false, form);
    size_t bytes = 0;
    const bool refused = hr_sample_lds_refused(*c, p_live, HR_SAMPLE_TIME_DENSITY, &bytes);
    const long long v[11] = {T.zp, T.pclass, T.all_lines, T.big_lds, T.blocks, (long long)T.lds,
                             T.d_slots, T.x_off, hr_time_per_ray_M(c->shading) ? 1 : 0, refused ? 1 : 0, (long long)bytes};
    for (int i = 0; i < 11; ++i) out[i] = v[i];
}
// hr_sample_lds_bytes of the same level: what the plan had before the density rows
long long td_sample_lds(const hr_config* c, int p_live)
{
    HrGridPlane pl[3];
    int ca_total = 0, n_cols = 0;
    (void)hr_plane_geometry(*c, pl, &ca_total, &n_cols);
    return (long long)hr_sample_lds_bytes(hr_head_quads(*c, p_live), ca_total, hr_round_zp(c->z_channels), rows_per_ray(*c));
}
// out = {active_precision, verified, status} with every activation small
void td_choice(const hr_config* c, int time_density, int* out)
{
    float act[HR_MAX_LAYERS];
    for (int l = 0; l < HR_MAX_LAYERS; ++l) act[l] = 1.0f;
    const HrMlpChoice ch = hr_mlp_choice(*c, hr_sample_kind(c->shading, time_density != 0), false, true, act);
    out[0] = ch.active_precision; out[1] = ch.verified; out[2] = ch.status;
}

}
