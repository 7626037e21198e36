// TEST-ONLY host build of hyperreel_amd/csrc/hr_shade.h (the MLP shading modes' input layout, weight tiles and scalar function) and of
// hr_plan.h's shading plan, for tests/test_shade_host.py.  Nothing in the product links or loads this file.
#include "../../hyperreel_amd/csrc/hr_shade.h"

static HrShadeNet net_of(int shading, int view_pe, int fea_pe, int feature_c)
{
    hr_shading_mlp d = {view_pe, fea_pe, feature_c};
    return hr_shade_net(shading, d);
}

extern "C" {

// out = {k0, k0p, hp, nt_h, nt_wave, rows_per_tile, stride, lds, ws_bytes_per_ray, launches, default chunk of head_chunk}
void sh_plan(int shading, int view_pe, int fea_pe, int feature_c, int z, long long head_chunk, long long* out)
{
    const HrShadePlan P = hr_shade_plan(shading, view_pe, fea_pe, feature_c, z);
    const long long v[11] = {P.k0, P.k0p, P.hp, P.nt_h, P.nt_wave, P.rows_per_tile, P.stride, (long long)P.lds, (long long)P.ws_bytes_per_ray, P.launches,
                             (long long)hr_shade_default_chunk(head_chunk, P)};
    for (int i = 0; i < 11; ++i) out[i] = v[i];
}
long long sh_blocks(long long n_rows) { return hr_shade_blocks(n_rows); }
int sh_live(float weight, float thresh) { return hr_shade_live(weight, thresh) ? 1 : 0; }

// columns 0 .. k0p - 1 of the input row: out[3 c ..] = {kind, src, freq}
void sh_columns(int shading, int view_pe, int fea_pe, int feature_c, int* out)
{
    const HrShadeNet g = net_of(shading, view_pe, fea_pe, feature_c);
    for (int c = 0; c < g.k0p; ++c) {
        const HrShadeCol col = hr_shade_column(g, c);
        out[3 * c] = col.kind; out[3 * c + 1] = col.src; out[3 * c + 2] = col.freq;
    }
}
// the encoded input row (k0p floats) of a sample [f | v]
void sh_input(int shading, int view_pe, int fea_pe, int feature_c, const float* row30, float* out)
{
    const HrShadeNet g = net_of(shading, view_pe, fea_pe, feature_c);
    for (int c = 0; c < g.k0p; ++c) out[c] = hr_shade_input(g, c, row30);
}

// geometry of Linear l: out = {N, K, Kp, nt, tile floats}
void sh_layer(int shading, int view_pe, int fea_pe, int feature_c, int l, long long* out)
{
    const HrShadeLayer L = hr_shade_layer(net_of(shading, view_pe, fea_pe, feature_c), l);
    out[0] = L.N; out[1] = L.K; out[2] = L.Kp; out[3] = L.nt; out[4] = (long long)hr_shade_tile_floats(L);
}
// packs Linear l and applies the tiles as the kernel does: y[16 t + (lane & 15)] += x[16 kt + 4 (lane >> 4) + s] * tile[kt][t][lane][s]
// (x: Kp floats, y: nt * 16 floats, bias added last).  With one-hot weights and integer inputs every sum is exact
void sh_apply_tiles(int shading, int view_pe, int fea_pe, int feature_c, int l, const float* w, const float* b, const float* x, float* y)
{
    const HrShadeLayer L = hr_shade_layer(net_of(shading, view_pe, fea_pe, feature_c), l);
    std::vector<float> tiles, bias;
    hr_shade_pack_layer(L, w, b, tiles, bias);
    for (int n = 0; n < L.nt * 16; ++n) y[n] = 0.0f;
    for (int kt = 0; kt < L.Kp / 16; ++kt)
        for (int t = 0; t < L.nt; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int s = 0; s < 4; ++s)
                    y[hr_shade_tile_n(t, lane)] += x[hr_shade_tile_k(kt, lane, s)] * tiles[hr_shade_tile_index(L, kt, t, lane, s)];
    for (int n = 0; n < L.nt * 16; ++n) y[n] += bias[n];
}

// hr_shade_row over n rows: f (n, 27), v (n, 3) -> rgb (n, 3)
void sh_rows(int shading, int view_pe, int fea_pe, int feature_c, const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
             const float* b2, const float* f, const float* v, long long n, float* rgb)
{
    const HrShadeNet g = net_of(shading, view_pe, fea_pe, feature_c);
    const float* const w[3] = {w0, w1, w2};
    const float* const b[3] = {b0, b1, b2};
    std::vector<float> scratch(2 * (size_t)(g.k0 + g.feature_c));
    for (long long i = 0; i < n; ++i) hr_shade_row(g, w, b, f + i * HR_SHADE_FEAT, v + i * 3, rgb + i * 3, scratch.data());
}

}
