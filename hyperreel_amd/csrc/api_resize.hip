// C ABI, image resize: hr_resize_plan_create / hr_resize_plan_create_rgba / hr_image_resize / hr_resize_plan_destroy (kernels: resize_kernel.hip; the rule and the
// choice of kernel: hr_resize.h).  The plan holds everything the host decides -- both axes' coefficient tables, checked, in device
// memory, and the 8-bit image between the passes -- so that the call itself only enqueues kernels on `stream`.
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "hr_model.h"
#include "hr_resize.h"

namespace {

constexpr int32_t MAX_SIZE = 1 << 20;       // per axis: a row's bytes and the tables' entries stay far inside int32

struct Axis {
    bool run = false;                       // the axis changes size
    int64_t ksize = 0;
    size_t bounds_at = 0, k_at = 0;         // words into the plan's tables
    hr_resize_axis_plan plan = {};
    int mad24 = 0;
};

// one axis: its tables appended to `host`, checked; its kernel chosen
int plan_axis(const char* name, int32_t in, int32_t out, int32_t filter, bool vertical, int32_t bpp, std::vector<int32_t>& host, Axis& a)
{
    a.run = in != out;
    if (!a.run) return HR_OK;
    a.ksize = hr_resize_ksize(in, out, filter);
    a.bounds_at = host.size();
    a.k_at = a.bounds_at + 2 * (size_t)out;
    host.resize(a.k_at + (size_t)out * (size_t)a.ksize);
    hr_resize_coeffs(in, out, filter, host.data() + a.bounds_at, host.data() + a.k_at);
    int64_t bad = -1;
    const int ok = hr_resize_check(host.data() + a.k_at, out, a.ksize, &bad);
    if (ok == HR_RESIZE_ROWS_OVERFLOW)
        return fail(HR_E_INVALID, "hr_resize_plan_create: accumulator check: %s coefficient row %lld (%d -> %d, filter %d) has 255 * sum|k| + 2^21 >= 2^31, "
                    "the int32 sum could overflow", name, (long long)bad, (int)in, (int)out, (int)filter);
    a.mad24 = ok == HR_RESIZE_ROWS_FIT_MAD24;
    a.plan = vertical ? hr_resize_plan_vertical(host.data() + a.bounds_at, out, a.ksize, bpp) : hr_resize_plan_horizontal(host.data() + a.bounds_at, out, a.ksize, bpp);
    return HR_OK;
}

}  // namespace

struct hr_resize_plan {
    int32_t w = 0, h = 0, w2 = 0, h2 = 0, filter = 0, max_images = 0;
    int32_t bpp = 3;                        // bytes of a pixel: 3 RGB, 4 RGBA (resampled premultiplied: hr_resize.h)
    Axis horizontal, vertical;
    DevMem<int32_t> tables;
    DevMem<uint8_t> between;                // (max_images, h, w2, bpp): the horizontal pass's bytes (RGBA: premultiplied) when a vertical pass follows
};

namespace {

HrResizePass make_pass(const hr_resize_plan* p, const Axis& a, bool vertical, const uint8_t* src, int64_t src_row, int64_t src_rows, uint8_t* dst,
                       int n_images)
{
    HrResizePass r = {};
    r.src = src;
    r.dst = dst;
    r.src_lo = src;
    r.src_hi = src + (int64_t)n_images * src_rows * src_row;
    r.src_pitch = src_row;
    r.src_image = src_rows * src_row;
    r.dst_pitch = (int64_t)p->w2 * p->bpp;
    r.dst_image = (vertical ? (int64_t)p->h2 : src_rows) * r.dst_pitch;
    r.bounds = p->tables + a.bounds_at;
    r.k = p->tables + a.k_at;
    r.ksize = (int)a.ksize;
    r.out = vertical ? p->h2 : p->w2;
    r.lines = vertical ? p->w2 * p->bpp : p->h;
    r.staged = a.plan.staged;
    r.tile = a.plan.tile;
    r.row_pitch = a.plan.row_pitch;
    r.lds_bytes = a.plan.lds_bytes;
    r.mad24 = a.mad24;
    r.channels = p->bpp;
    // RGBA: the first pass that runs premultiplies what it reads, the last un-premultiplies what it writes (a single pass does both)
    r.premultiply = p->bpp == 4 && (!vertical || !p->horizontal.run);
    r.unpremultiply = p->bpp == 4 && (vertical || !p->vertical.run);
    return r;
}

}  // namespace

static int plan_create(int32_t w, int32_t h, int32_t w2, int32_t h2, int32_t filter, int32_t max_images, int32_t bpp, hr_resize_plan** out)
{
    if (!out) return fail(HR_E_INVALID, "hr_resize_plan_create: null argument (out)");
    *out = nullptr;
    if (w < 1 || h < 1) return fail(HR_E_INVALID, "hr_resize_plan_create: source size %d x %d (w, h) must be at least 1 x 1", (int)w, (int)h);
    if (w2 < 1 || h2 < 1) return fail(HR_E_INVALID, "hr_resize_plan_create: destination size %d x %d (w2, h2) must be at least 1 x 1", (int)w2, (int)h2);
    if (w > MAX_SIZE || h > MAX_SIZE || w2 > MAX_SIZE || h2 > MAX_SIZE)
        return fail(HR_E_INVALID, "hr_resize_plan_create: sizes (w, h, w2, h2) = (%d, %d, %d, %d) beyond %d", (int)w, (int)h, (int)w2, (int)h2, (int)MAX_SIZE);
    if (!hr_resize_filter_known(filter))
        return fail(HR_E_INVALID, "hr_resize_plan_create: unknown filter %d (PIL's numbers: 1 LANCZOS, 2 BILINEAR, 3 BICUBIC, 4 BOX)", (int)filter);
    if (max_images < 1) return fail(HR_E_INVALID, "hr_resize_plan_create: max_images %d < 1", (int)max_images);
    std::unique_ptr<hr_resize_plan> p(new hr_resize_plan());
    p->w = w; p->h = h; p->w2 = w2; p->h2 = h2; p->filter = filter; p->max_images = max_images; p->bpp = bpp;
    std::vector<int32_t> host;
    if (int rc = plan_axis("horizontal", w, w2, filter, false, bpp, host, p->horizontal)) return rc;
    if (int rc = plan_axis("vertical", h, h2, filter, true, bpp, host, p->vertical)) return rc;
    const Axis &ah = p->horizontal, &av = p->vertical;
    const uint8_t* none = nullptr;
    if ((ah.run && hr_resize_pass_blocks(make_pass(p.get(), ah, false, none, (int64_t)w * bpp, h, nullptr, max_images), false, max_images) > 0x7fffffff)
        || (av.run && hr_resize_pass_blocks(make_pass(p.get(), av, true, none, (int64_t)w2 * bpp, h, nullptr, max_images), true, max_images) > 0x7fffffff))
        return fail(HR_E_INVALID, "hr_resize_plan_create: max_images %d images of this size are more than one launch covers: resize them in smaller batches",
                    (int)max_images);
    hipError_t e = hipSuccess;
    if (!host.empty()) {
        e = p->tables.alloc(sizeof(int32_t) * host.size());
        if (e == hipSuccess) e = hipMemcpy(p->tables, host.data(), sizeof(int32_t) * host.size(), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && ah.run && av.run) e = p->between.alloc((size_t)max_images * h * w2 * bpp);
    if (e != hipSuccess) return fail(HR_E_HIP, "hr_resize_plan_create: %s", hipGetErrorString(e));
    *out = p.release();
    return HR_OK;
}

// (messages name hr_resize_plan_create: the RGBA call is that one on four-byte pixels)
int hr_resize_plan_create(int32_t w, int32_t h, int32_t w2, int32_t h2, int32_t filter, int32_t max_images, hr_resize_plan** out)
{
    return plan_create(w, h, w2, h2, filter, max_images, 3, out);
}

int hr_resize_plan_create_rgba(int32_t w, int32_t h, int32_t w2, int32_t h2, int32_t filter, int32_t max_images, hr_resize_plan** out)
{
    return plan_create(w, h, w2, h2, filter, max_images, 4, out);
}

int hr_image_resize(const hr_resize_plan* p, const uint8_t* src_dev, int32_t n_images, uint8_t* dst_dev, void* stream)
{
    if (!p) return fail(HR_E_INVALID, "hr_image_resize: null argument (plan)");
    if (!src_dev) return fail(HR_E_INVALID, "hr_image_resize: null argument (src_dev)");
    if (!dst_dev) return fail(HR_E_INVALID, "hr_image_resize: null argument (dst_dev)");
    if (n_images < 1 || n_images > p->max_images)
        return fail(HR_E_INVALID, "hr_image_resize: n_images %d outside 1..%d (the plan's max_images)", (int)n_images, (int)p->max_images);
    if (p->bpp == 4 && ((((uintptr_t)src_dev) | ((uintptr_t)dst_dev)) & 3))
        return fail(HR_E_INVALID, "hr_image_resize: RGBA images (src_dev, dst_dev) must be 4-byte aligned: a pixel is read and written as one word");
    const hipStream_t s = (hipStream_t)stream;
    const Axis &ah = p->horizontal, &av = p->vertical;
    if (!ah.run && !av.run) {
        HR_HIP(hipMemcpyAsync(dst_dev, src_dev, (size_t)n_images * p->h * p->w * p->bpp, hipMemcpyDeviceToDevice, s));
        return HR_OK;
    }
    const uint8_t* v_src = src_dev;
    if (ah.run) {
        uint8_t* h_dst = av.run ? (uint8_t*)p->between : dst_dev;
        HR_HIP(hr_launch_resize_pass(make_pass(p, ah, false, src_dev, (int64_t)p->w * p->bpp, p->h, h_dst, n_images), false, n_images, s));
        v_src = h_dst;
    }
    if (av.run) HR_HIP(hr_launch_resize_pass(make_pass(p, av, true, v_src, (int64_t)p->w2 * p->bpp, p->h, dst_dev, n_images), true, n_images, s));
    return HR_OK;
}

void hr_resize_plan_destroy(hr_resize_plan* p) { delete p; }
