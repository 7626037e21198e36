// TEST-ONLY host build of hyperreel_amd/csrc/hr_mlp_pack.h (the MLP weight packer: geometry, source and tile indices, conversions,
// scalings, the host routine pack_mlp calls), for tests/test_mlp_pack_host.py.  Nothing in the product links or loads this file.
#include "../../hyperreel_amd/csrc/hr_mlp_pack.h"

extern "C" {

void pk_bf16(const float* x, long long n, uint16_t* out) { for (long long i = 0; i < n; ++i) out[i] = hr_bf16_rne(x[i]); }
void pk_f16(const float* x, long long n, uint16_t* out) { for (long long i = 0; i < n; ++i) out[i] = hr_f16_rne(x[i]); }
void pk_e4m3(const float* x, long long n, uint8_t* out) { for (long long i = 0; i < n; ++i) out[i] = hr_e4m3_rne(x[i]); }
void pk_f16_to_float(const uint16_t* h, long long n, float* out) { for (long long i = 0; i < n; ++i) out[i] = hr_f16_to_float(h[i]); }
void pk_bf16_to_float(const uint16_t* h, long long n, float* out) { for (long long i = 0; i < n; ++i) out[i] = hr_bf16_to_float(h[i]); }
int pk_weight_shift(float w_max) { return hr_weight_shift(w_max); }
int pk_f8_exponent(float act_max) { return hr_f8_exponent(act_max); }
float pk_f8_headroom() { return HR_F8_HEADROOM; }

// Linear l of an MLP (mlp_in -> hidden x (layers - 1) -> z * p_user, skip layers by mask) whose user head column i is live column col[i]
static HrMlpLayer layer_of(int mlp_in, int hidden, int layers, int skip_mask, int z, int p_user, const int* col, int p_live, int l, int precision)
{
    hr_config c = hr_config();
    c.mlp_in = mlp_in;
    c.mlp_hidden = hidden;
    c.mlp_layers = layers;
    c.mlp_skip_mask = skip_mask;
    c.z_channels = z;
    c.preds_per_z = p_user;
    HrColMap map;
    for (int i = 0; i < 64; ++i) map.col[i] = col[i];
    return mlp_layer(c, p_live, map, l, hr_pack_tile_n(precision));
}

// geometry of the layer: out = {N_user, Kt, N, Kp, nt, kseg, tile bytes, bias floats}
void pk_layer_geometry(int mlp_in, int hidden, int layers, int skip_mask, int z, int p_user, const int* col, int p_live, int l, int precision, long long* out)
{
    const HrMlpLayer g = layer_of(mlp_in, hidden, layers, skip_mask, z, p_user, col, p_live, l, precision);
    const long long per_tile = precision == HR_MLP_FP32 ? 64 * 4 * 4 : 2 * 64 * 8 * 2;
    const long long v[8] = {g.N_user, g.Kt, g.N, g.Kp, g.nt, hr_pack_kseg(g), (long long)(g.Kp / 16) * g.nt * per_tile, (long long)g.nt * hr_pack_tile_n(precision)};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
}

// hr_pack_mlp_layer on w (N_user, Kt), b (N_user) -> tiles / bias (sized by pk_layer_geometry), winv
void pk_pack_layer(int mlp_in, int hidden, int layers, int skip_mask, int z, int p_user, const int* col, int p_live, int l, int precision, const float* w,
                   const float* b, uint8_t* tiles, float* bias, float* winv)
{
    const HrMlpLayer g = layer_of(mlp_in, hidden, layers, skip_mask, z, p_user, col, p_live, l, precision);
    const std::vector<float> wv(w, w + (size_t)g.N_user * g.Kt), bv(b, b + g.N_user);
    HrPackedLayer pk;
    hr_pack_mlp_layer(g, precision, wv, bv, pk);
    memcpy(tiles, pk.tiles.data(), pk.tiles.size());
    memcpy(bias, pk.bias.data(), pk.bias.size() * sizeof(float));
    *winv = pk.winv;
}

}  // extern "C"
