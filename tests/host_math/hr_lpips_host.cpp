// Host build of hyperreel_amd/csrc/hr_lpips.h for tests/test_lpips_host.py: the layer tables, every layer's size, the minimum frame,
// the workspace and the weight packer's index map, asked directly.  Also hr_lpips_scores' layout as the C compiler of the public header sees it.
#include <stddef.h>
#include <stdint.h>

#include "../../hyperreel_amd/csrc/hr_lpips.h"
#include "../../include/hyperreel_hip.h"

extern "C" {

int hlp_n_layers(int net) { return hr_lp_n_layers(net); }
int hlp_n_convs(int net) { return hr_lp_n_convs(net); }
int hlp_min_size(int net) { return hr_lp_min_size(net); }

// out[7]: kind, cin, cout, k, stride, pad, tap
void hlp_layer(int net, int i, int32_t* out)
{
    const HrLpLayer l = hr_lp_layer(net, i);
    out[0] = l.kind; out[1] = l.cin; out[2] = l.cout; out[3] = l.k; out[4] = l.stride; out[5] = l.pad; out[6] = l.tap;
}

// hs, ws: n_layers each; slots: tap_slots[5] then tap_slot_at[5]; sizes: buf_elems, n_slots, bytes.  Returns hr_lp_plan's verdict.
int hlp_plan(int net, int h, int w, int32_t* hs, int32_t* ws, int64_t* slots, int64_t* sizes)
{
    HrLpPlan p;
    if (!hr_lp_plan(net, h, w, &p)) return 0;
    for (int i = 0; i < p.n_layers; ++i) { hs[i] = p.hs[i]; ws[i] = p.ws[i]; }
    for (int k = 0; k < HR_LP_TAPS; ++k) { slots[k] = p.tap_slots[k]; slots[HR_LP_TAPS + k] = p.tap_slot_at[k]; }
    sizes[0] = p.buf_elems; sizes[1] = p.n_slots; sizes[2] = (int64_t)p.bytes;
    return 1;
}

int64_t hlp_packed_elems(int net, int i) { return hr_lp_packed_elems(hr_lp_layer(net, i)); }

// src[n] for every packed index of layer i
void hlp_pack_src(int net, int i, int64_t* src)
{
    const HrLpLayer l = hr_lp_layer(net, i);
    const int64_t n = hr_lp_packed_elems(l);
    for (int64_t d = 0; d < n; ++d) src[d] = hr_lp_pack_src(l, d);
}

// dst[o] for every OIHW index of layer i
void hlp_pack_dst(int net, int i, int64_t* dst)
{
    const HrLpLayer l = hr_lp_layer(net, i);
    int64_t o = 0;
    for (int n = 0; n < l.cout; ++n)
        for (int c = 0; c < l.cin; ++c)
            for (int ky = 0; ky < l.k; ++ky)
                for (int kx = 0; kx < l.k; ++kx) dst[o++] = hr_lp_pack_dst(l, n, c, ky, kx);
}

int hlp_scores_sizeof(void) { return (int)sizeof(hr_lpips_scores); }
int hlp_scores_offset(int field) { return field == 0 ? (int)offsetof(hr_lpips_scores, layer) : (int)offsetof(hr_lpips_scores, total); }
int hlp_abi_version(void) { return HR_ABI_VERSION; }
int hlp_net_number(int which) { return which == 0 ? HR_LPIPS_ALEX : HR_LPIPS_VGG; }

}  // extern "C"
