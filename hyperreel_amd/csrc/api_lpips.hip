// C ABI, LPIPS: hr_lpips_create / hr_lpips_destroy / hr_lpips_workspace / hr_lpips (kernels: lpips_kernel.hip; the definition, the layer
// tables and every size: hr_lpips.h).  The object owns the packed weights; the call itself only enqueues kernels on `stream`.
#include <hip/hip_runtime.h>

#include <memory>

#include "hr_lpips.h"
#include "hr_model.h"

static_assert(sizeof(hr_lpips_scores) == sizeof(double) * (HR_LP_TAPS + 1), "the finish kernel writes the result as six doubles");
static_assert(HR_LPIPS_ALEX == HR_LP_ALEX && HR_LPIPS_VGG == HR_LP_VGG, "the public net numbers are hr_lpips.h's");

struct hr_lpips {
    int32_t net = 0;
    DevMem<float> packed[HR_LP_MAX_CONVS];      // hr_lpips.h's operand order
    DevMem<float> bias[HR_LP_MAX_CONVS];
    DevMem<float> lin[HR_LP_TAPS];
};

namespace {

// `src` is wherever the caller keeps it: a device pointer is copied on the device, anything else from the host
hipError_t copy_in(float* dst, const float* src, size_t bytes)
{
    hipPointerAttribute_t at = {};
    const bool dev = hipPointerGetAttributes(&at, src) == hipSuccess && (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged);
    (void)hipGetLastError();                    // an ordinary host pointer is "invalid" to the query: not an error of this call
    return hipMemcpy(dst, src, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
}

}  // namespace

int hr_lpips_create(int32_t net, const float* const* conv_w, const float* const* conv_b, const float* const* lin_w, struct hr_lpips** out)
{
    if (!out) return fail(HR_E_INVALID, "hr_lpips_create: null argument (out)");
    *out = nullptr;
    if (!hr_lp_net_known(net)) return fail(HR_E_INVALID, "hr_lpips_create: unknown net %d (HR_LPIPS_ALEX 0, HR_LPIPS_VGG 1)", (int)net);
    if (!conv_w || !conv_b || !lin_w) return fail(HR_E_INVALID, "hr_lpips_create: null argument");
    for (int i = 0; i < hr_lp_n_convs(net); ++i)
        if (!conv_w[i] || !conv_b[i]) return fail(HR_E_INVALID, "hr_lpips_create: null weight or bias of convolution %d", i);
    for (int k = 0; k < HR_LP_TAPS; ++k)
        if (!lin_w[k]) return fail(HR_E_INVALID, "hr_lpips_create: null lin weight of tap %d", k);
    std::unique_ptr<struct hr_lpips> p(new struct hr_lpips());
    p->net = net;
    int conv = 0;
    for (int i = 0; i < hr_lp_n_layers(net); ++i) {
        const HrLpLayer l = hr_lp_layer(net, i);
        if (l.kind != HR_LP_CONV) continue;
        const size_t w_bytes = sizeof(float) * (size_t)l.cout * l.cin * l.k * l.k;
        DevMem<float> raw;
        HR_HIP(raw.alloc(w_bytes));
        HR_HIP(copy_in(raw, conv_w[conv], w_bytes));
        HR_HIP(p->packed[conv].alloc(sizeof(float) * (size_t)hr_lp_packed_elems(l)));
        hr_launch_lpips_pack(raw, l, p->packed[conv], nullptr);
        HR_HIP(hipGetLastError());
        HR_HIP(hipDeviceSynchronize());         // `raw` goes at the end of this iteration
        HR_HIP(p->bias[conv].alloc(sizeof(float) * l.cout));
        HR_HIP(copy_in(p->bias[conv], conv_b[conv], sizeof(float) * l.cout));
        if (l.tap >= 0) {
            HR_HIP(p->lin[l.tap].alloc(sizeof(float) * l.cout));
            HR_HIP(copy_in(p->lin[l.tap], lin_w[l.tap], sizeof(float) * l.cout));
        }
        ++conv;
    }
    HR_HIP(hipDeviceSynchronize());
    *out = p.release();
    return HR_OK;
}

void hr_lpips_destroy(struct hr_lpips* p) { delete p; }

size_t hr_lpips_workspace(int32_t net, int32_t h, int32_t w)
{
    HrLpPlan plan;
    return hr_lp_plan(net, h, w, &plan) ? plan.bytes : 0;
}

int hr_lpips(const struct hr_lpips* p, const float* pred_dev, const float* gt_dev, int32_t h, int32_t w, hr_lpips_scores* out_dev, void* workspace_dev,
             void* stream)
{
    if (!p) return fail(HR_E_INVALID, "hr_lpips: null argument (the hr_lpips object)");
    if (!pred_dev || !gt_dev || !out_dev || !workspace_dev) return fail(HR_E_INVALID, "hr_lpips: null argument");
    const int min_size = hr_lp_min_size(p->net);
    if (h < min_size || w < min_size)
        return fail(HR_E_INVALID, "hr_lpips: %s needs at least %d x %d pixels (every tap at least 1 x 1), got %d x %d", p->net == HR_LP_ALEX ? "alex" : "vgg",
                    min_size, min_size, (int)h, (int)w);
    HrLpPlan plan;
    if (!hr_lp_plan(p->net, h, w, &plan))
        return fail(HR_E_INVALID, "hr_lpips: frame %d x %d too large: a layer's pixels of both images, and with them the workspace size, pass int32", (int)h, (int)w);
    if (reinterpret_cast<uintptr_t>(workspace_dev) & 15) return fail(HR_E_INVALID, "hr_lpips: workspace_dev must be 16-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    float* buf[2] = {reinterpret_cast<float*>(workspace_dev), reinterpret_cast<float*>(workspace_dev) + plan.buf_elems};
    double* slots = reinterpret_cast<double*>(buf[1] + plan.buf_elems);
    HrLpHeadTaps taps = {};
    int cur = 1;                                // the buffer the next layer writes
    const float* in = pred_dev;
    int ch = h, cw = w, conv = 0;
    for (int i = 0; i < plan.n_layers; ++i) {
        const HrLpLayer l = hr_lp_layer(p->net, i);
        float* dst = buf[cur];
        if (l.kind == HR_LP_CONV) {
            HrLpConvArgs a = {};
            a.in = in; a.in2 = gt_dev; a.wp = reinterpret_cast<const float4*>((const float*)p->packed[conv]); a.bias = p->bias[conv]; a.out = dst;
            a.H = ch; a.W = cw; a.cin = l.cin; a.Ho = plan.hs[i]; a.Wo = plan.ws[i]; a.cout = l.cout; a.k = l.k; a.stride = l.stride; a.pad = l.pad;
            hr_launch_lpips_conv(a, i == 0, s);
            ++conv;
        } else {
            hr_launch_lpips_pool(in, dst, ch, cw, l.cin, plan.hs[i], plan.ws[i], l.k, l.stride, s);
        }
        ch = plan.hs[i];
        cw = plan.ws[i];
        if (l.tap >= 0) {
            const int64_t pixels = (int64_t)ch * cw;
            double* at = slots + plan.tap_slot_at[l.tap];
            hr_launch_lpips_head(dst, p->lin[l.tap], pixels, l.cout, at, plan.tap_slots[l.tap], s);
            taps.slots[l.tap] = at;
            taps.n_slots[l.tap] = plan.tap_slots[l.tap];
            taps.pixels[l.tap] = (double)pixels;
        }
        in = dst;
        cur ^= 1;
    }
    hr_launch_lpips_finish(taps, reinterpret_cast<double*>(out_dev), s);
    HR_HIP(hipGetLastError());
    return HR_OK;
}
