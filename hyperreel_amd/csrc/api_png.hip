// C ABI, PNG files: hr_png_bound / hr_png_encoder_create / hr_png_encode / hr_png_encoder_destroy (kernels: png_kernel.hip; the format's
// arithmetic and the plan: hr_png.h).  The encoder owns its workspace in device memory, so that the call itself only enqueues kernels on
// `stream`: no allocation, no synchronisation, no read-back, no memset.
#include <hip/hip_runtime.h>

#include <memory>

#include "hr_model.h"
#include "hr_png.h"

struct hr_png_encoder {
    hr_png_plan_t plan = {};
    DevMem<uint8_t> workspace;
};

namespace {

int check_shape(const char* who, int32_t w, int32_t h, int32_t channels)
{
    if (w < 1 || h < 1) return fail(HR_E_INVALID, "%s: size %d x %d (w, h) must be at least 1 x 1", who, (int)w, (int)h);
    if (channels != 1 && channels != 3 && channels != 4)
        return fail(HR_E_INVALID, "%s: channels %d is not 1 (grey), 3 (RGB) or 4 (RGBA)", who, (int)channels);
    if (!hr_png_shape_ok(w, h, channels))
        return fail(HR_E_INVALID, "%s: %d x %d x %d is more than %d bytes a row or %lld filtered bytes in all", who, (int)w, (int)h, (int)channels,
                    (int)HR_PNG_MAX_ROW_BYTES, (long long)HR_PNG_MAX_BYTES);
    return HR_OK;
}

}  // namespace

int hr_png_bound(int32_t w, int32_t h, int32_t channels, int64_t* bytes)
{
    if (!bytes) return fail(HR_E_INVALID, "hr_png_bound: null argument (bytes)");
    if (int rc = check_shape("hr_png_bound", w, h, channels)) return rc;
    *bytes = hr_png_plan(w, h, channels).bound;
    return HR_OK;
}

int hr_png_encoder_create(int32_t w, int32_t h, int32_t channels, hr_png_encoder** out)
{
    if (!out) return fail(HR_E_INVALID, "hr_png_encoder_create: null argument (out)");
    *out = nullptr;
    if (int rc = check_shape("hr_png_encoder_create", w, h, channels)) return rc;
    std::unique_ptr<hr_png_encoder> e(new hr_png_encoder());
    e->plan = hr_png_plan(w, h, channels);
    const hipError_t err = e->workspace.alloc((size_t)e->plan.workspace_bytes);
    if (err != hipSuccess) return fail(HR_E_HIP, "hr_png_encoder_create: %s", hipGetErrorString(err));
    *out = e.release();
    return HR_OK;
}

int hr_png_encode(hr_png_encoder* e, const void* pixels_dev, int32_t pixel_type, int32_t filter_mode, void* file_dev, int64_t capacity,
                  int64_t* file_bytes_dev, void* stream)
{
    if (!e) return fail(HR_E_INVALID, "hr_png_encode: null argument (encoder)");
    if (!pixels_dev) return fail(HR_E_INVALID, "hr_png_encode: null argument (pixels_dev)");
    if (!file_dev) return fail(HR_E_INVALID, "hr_png_encode: null argument (file_dev)");
    if (!file_bytes_dev) return fail(HR_E_INVALID, "hr_png_encode: null argument (file_bytes_dev)");
    if (pixel_type != HR_PNG_U8 && pixel_type != HR_PNG_F32_TO8B)
        return fail(HR_E_INVALID, "hr_png_encode: unknown pixel_type %d (HR_PNG_U8 0, HR_PNG_F32_TO8B 1)", (int)pixel_type);
    if (filter_mode < 0 || filter_mode > HR_PNG_FILTER_ADAPTIVE)
        return fail(HR_E_INVALID, "hr_png_encode: unknown filter_mode %d (a PNG filter 0..4, or HR_PNG_FILTER_ADAPTIVE %d)", (int)filter_mode,
                    (int)HR_PNG_FILTER_ADAPTIVE);
    if (capacity < e->plan.bound)
        return fail(HR_E_INVALID, "hr_png_encode: capacity %lld is below hr_png_bound's %lld bytes", (long long)capacity, (long long)e->plan.bound);
    if (pixel_type == HR_PNG_F32_TO8B && (((uintptr_t)pixels_dev) & 3))
        return fail(HR_E_INVALID, "hr_png_encode: a float frame (pixels_dev) must be 4-byte aligned");
    if (((uintptr_t)file_bytes_dev) & 7) return fail(HR_E_INVALID, "hr_png_encode: file_bytes_dev must be 8-byte aligned");
    HrPngArgs a = {};
    a.pixels = pixels_dev;
    a.pixel_type = pixel_type;
    a.filter_mode = filter_mode;
    a.plan = e->plan;
    a.workspace = e->workspace;
    a.file = (uint8_t*)file_dev;
    a.file_bytes = file_bytes_dev;
    HR_HIP(hr_launch_png_encode(a, (hipStream_t)stream));
    return HR_OK;
}

void hr_png_encoder_destroy(hr_png_encoder* e) { delete e; }
