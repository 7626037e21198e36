// TEST-ONLY host build of hyperreel_amd/csrc/hr_train.h as train_time_kernel.hip compiles it (HR_TRAIN_TIME: the time-dependent colour
// modes' basis vector, activation and derivative), for tests/test_time_decode_host.py.  Nothing in the product links or loads this file.
#include <vector>

#include "../../hyperreel_amd/csrc/hr_mask.h"
#include "../../hyperreel_amd/csrc/hr_plan.h"
#define HR_TRAIN_TIME 1
#include "../../hyperreel_amd/csrc/hr_train.h"

extern "C" {

int htt_nbv(const hr_config* c) { return hr_train_nbv(*c); }
const char* htt_unsupported(const hr_config* c) { return hr_train_unsupported(*c); }

// tests/host_math/hr_train_host.cpp's ht_train with the ray's basis vector of this build: forward of every ray, then phase B and C per ray
int htt_train(const hr_config* c, const float* rays, const float* head, long long n, const float* d_rgb, float* rgb, float* d_head,
              const HrGridPlane* planes, float** g_a, float** g_b, const float* basis, float* d_basis, int n_basis_cols, int ca_total, int white_bg)
{
    if (c->z_channels > 256 || ca_total > HR_TRAIN_MAX_CA) return -1;
    HrTrainArgs a = {};
    a.cfg_dev = c;
    a.rays = rays; a.head = head; a.n_rays = n; a.rgb = rgb; a.d_rgb = d_rgb; a.d_head = d_head;
    for (int j = 0; j < 3; ++j) { a.planes[j] = planes[j]; a.g_a[j] = g_a[j]; a.g_b[j] = g_b[j]; }
    a.basis = basis; a.d_basis = d_basis; a.n_basis_cols = n_basis_cols; a.ca_total = ca_total; a.white_bg = white_bg;
    const size_t NS = (size_t)n * c->z_channels;
    std::vector<float> tape(HR_TAPE_WORDS * NS);
    a.tape = hr_tape_bind(tape.data(), (int64_t)NS);
    a.tape.taps = nullptr; a.tape.dp = nullptr; a.tape.perm = nullptr;
    hr_with_zp(hr_round_zp(c->z_channels), [&](auto zp) {
        for (long long i = 0; i < n; ++i) hr_ray_train<decltype(zp)::value>(*c, a, i);
    });
    if (!d_rgb) return 0;
    for (long long i = 0; i < n; ++i) {
        float sh[HR_TRAIN_NBV_MAX] = {};
        hr_train_ray_basis(*c, rays + (size_t)i * c->ray_dim, sh);
        float M[3 * HR_TRAIN_MAX_CA], dM[3 * HR_TRAIN_MAX_CA];
        for (int cc = 0; cc < 3; ++cc)
            for (int pos = 0; pos < ca_total; ++pos) { M[cc * ca_total + pos] = hr_train_decode_coef(*c, a, sh, cc, pos); dM[cc * ca_total + pos] = 0.0f; }
        for (int k = 0; k < c->z_channels; ++k) hr_sample_train_bwd(*c, a, i, k, M, dM);
        for (int cc = 0; cc < 3; ++cc)
            for (int pos = 0; pos < ca_total; ++pos) hr_train_fold_basis(*c, a, sh, cc, pos, dM[cc * ca_total + pos]);
    }
    for (long long i = 0; i < n; ++i)
        for (int k = 0; k < c->z_channels; ++k) hr_sample_train_dist_bwd(*c, a, i, k);
    return 0;
}

}
