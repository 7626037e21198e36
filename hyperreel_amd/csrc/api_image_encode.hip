// C ABI, PNG and JPEG files encoded on the device: hr_{png,jpeg}_bound / _encoder_create / _encode / _encoder_destroy (kernels:
// png_kernel.hip, jpeg_encode_kernel.hip; the formats' arithmetic and the plans: hr_png.h, hr_jpeg_encode.h).  An encoder owns its workspace
// in device memory -- the JPEG one with the quantisation and Huffman tables and the file's header, built on the host at create time, at
// its start -- so that the call itself only enqueues kernels on `stream`: no allocation, no synchronisation, no read-back, no memset.
#include <hip/hip_runtime.h>

#include <memory>

#include "hr_model.h"
#include "hr_jpeg_encode.h"
#include "hr_png.h"

struct hr_png_encoder {
    hr_png_plan_t plan = {};
    DevMem<uint8_t> workspace;
};

struct hr_jpeg_encoder {
    hr_jpeg_enc_plan_t plan = {};
    DevMem<uint8_t> workspace;
};

namespace {

// the sizes a PNG encoder takes (hr_png_shape_ok); JPEG has hr_jpeg_enc_refusal
int check_png_shape(const char* who, int32_t w, int32_t h, int32_t channels)
{
    if (w < 1 || h < 1) return fail(HR_E_INVALID, "%s: size %d x %d (w, h) must be at least 1 x 1", who, (int)w, (int)h);
    if (channels != 1 && channels != 3 && channels != 4)
        return fail(HR_E_INVALID, "%s: channels %d is not 1 (grey), 3 (RGB) or 4 (RGBA)", who, (int)channels);
    if (!hr_png_shape_ok(w, h, channels))
        return fail(HR_E_INVALID, "%s: %d x %d x %d is more than %d bytes a row or %lld filtered bytes in all", who, (int)w, (int)h, (int)channels,
                    (int)HR_PNG_MAX_ROW_BYTES, (long long)HR_PNG_MAX_BYTES);
    return HR_OK;
}

// the end of hr_*_encoder_create, `who` being the caller and e->plan filled in: the workspace of the plan's size
template <class E> int alloc_workspace(const char* who, E* e)
{
    const hipError_t err = e->workspace.alloc((size_t)e->plan.workspace_bytes);
    if (err != hipSuccess) return fail(HR_E_HIP, "%s: %s", who, hipGetErrorString(err));
    return HR_OK;
}

// the arguments hr_*_encode share, e being either encoder: `who` is the caller, `bound` the function that gives the capacity it asks
// for, length_name its name of length_dev
template <class E> int check_encode(const char* who, const E* e, const void* pixels_dev, int32_t pixel_type, const void* file_dev, int64_t capacity,
                                    const char* bound, const int64_t* length_dev, const char* length_name)
{
    if (!e) return fail(HR_E_INVALID, "%s: null argument (encoder)", who);
    if (!pixels_dev) return fail(HR_E_INVALID, "%s: null argument (pixels_dev)", who);
    if (!file_dev) return fail(HR_E_INVALID, "%s: null argument (file_dev)", who);
    if (!length_dev) return fail(HR_E_INVALID, "%s: null argument (%s)", who, length_name);
    if (pixel_type != HR_PNG_U8 && pixel_type != HR_PNG_F32_TO8B)
        return fail(HR_E_INVALID, "%s: unknown pixel_type %d (HR_PNG_U8 0, HR_PNG_F32_TO8B 1)", who, (int)pixel_type);
    if (capacity < e->plan.bound)
        return fail(HR_E_INVALID, "%s: capacity %lld is below %s's %lld bytes", who, (long long)capacity, bound, (long long)e->plan.bound);
    if (pixel_type == HR_PNG_F32_TO8B && (((uintptr_t)pixels_dev) & 3))
        return fail(HR_E_INVALID, "%s: a float frame (pixels_dev) must be 4-byte aligned", who);
    if (((uintptr_t)length_dev) & 7) return fail(HR_E_INVALID, "%s: %s must be 8-byte aligned", who, length_name);
    return HR_OK;
}

}  // namespace

int hr_png_bound(int32_t w, int32_t h, int32_t channels, int64_t* bytes)
{
    if (!bytes) return fail(HR_E_INVALID, "hr_png_bound: null argument (bytes)");
    if (int rc = check_png_shape("hr_png_bound", w, h, channels)) return rc;
    *bytes = hr_png_plan(w, h, channels).bound;
    return HR_OK;
}

int hr_png_encoder_create(int32_t w, int32_t h, int32_t channels, hr_png_encoder** out)
{
    if (!out) return fail(HR_E_INVALID, "hr_png_encoder_create: null argument (out)");
    *out = nullptr;
    if (int rc = check_png_shape("hr_png_encoder_create", w, h, channels)) return rc;
    std::unique_ptr<hr_png_encoder> e(new hr_png_encoder());
    e->plan = hr_png_plan(w, h, channels);
    if (int rc = alloc_workspace("hr_png_encoder_create", e.get())) return rc;
    *out = e.release();
    return HR_OK;
}

int hr_png_encode(hr_png_encoder* e, const void* pixels_dev, int32_t pixel_type, int32_t filter_mode, void* file_dev, int64_t capacity,
                  int64_t* file_bytes_dev, void* stream)
{
    if (int rc = check_encode("hr_png_encode", e, pixels_dev, pixel_type, file_dev, capacity, "hr_png_bound", file_bytes_dev, "file_bytes_dev"))
        return rc;
    if (filter_mode < 0 || filter_mode > HR_PNG_FILTER_ADAPTIVE)
        return fail(HR_E_INVALID, "hr_png_encode: unknown filter_mode %d (a PNG filter 0..4, or HR_PNG_FILTER_ADAPTIVE %d)", (int)filter_mode,
                    (int)HR_PNG_FILTER_ADAPTIVE);
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

int hr_jpeg_bound(int32_t w, int32_t h, int32_t channels, int32_t subsampling, int32_t restart_rows, int64_t* bytes)
{
    if (!bytes) return fail(HR_E_INVALID, "hr_jpeg_bound: null argument (bytes)");
    if (const char* why = hr_jpeg_enc_refusal(w, h, channels, 90, subsampling, restart_rows))
        return fail(HR_E_INVALID, "hr_jpeg_bound: %d x %d x %d, subsampling %d, restart_rows %d: %s", (int)w, (int)h, (int)channels, (int)subsampling,
                    (int)restart_rows, why);
    *bytes = hr_jpeg_enc_plan(w, h, channels, subsampling, restart_rows).bound;
    return HR_OK;
}

int hr_jpeg_encoder_create(int32_t w, int32_t h, int32_t channels, int32_t quality, int32_t subsampling, int32_t restart_rows, hr_jpeg_encoder** out)
{
    if (!out) return fail(HR_E_INVALID, "hr_jpeg_encoder_create: null argument (out)");
    *out = nullptr;
    if (const char* why = hr_jpeg_enc_refusal(w, h, channels, quality, subsampling, restart_rows))
        return fail(HR_E_INVALID, "hr_jpeg_encoder_create: %d x %d x %d, quality %d, subsampling %d, restart_rows %d: %s", (int)w, (int)h, (int)channels,
                    (int)quality, (int)subsampling, (int)restart_rows, why);
    std::unique_ptr<hr_jpeg_encoder> e(new hr_jpeg_encoder());
    e->plan = hr_jpeg_enc_plan(w, h, channels, subsampling, restart_rows);
    std::unique_ptr<hr_jpeg_enc_tables> t(new hr_jpeg_enc_tables());
    hr_jpeg_enc_tables_build(e->plan, quality, restart_rows, t.get());
    if (t->head_bytes != e->plan.head_bytes)
        return fail(HR_E_INVALID, "hr_jpeg_encoder_create: the header is %d bytes, the plan says %d", (int)t->head_bytes, (int)e->plan.head_bytes);
    if (int rc = alloc_workspace("hr_jpeg_encoder_create", e.get())) return rc;
    HR_HIP(hipMemcpy((uint8_t*)e->workspace + e->plan.off_tables, t.get(), sizeof(hr_jpeg_enc_tables), hipMemcpyHostToDevice));
    *out = e.release();
    return HR_OK;
}

int hr_jpeg_encode(hr_jpeg_encoder* e, const void* pixels_dev, int32_t pixel_type, void* file_dev, int64_t capacity, int64_t* length_dev, void* stream)
{
    if (int rc = check_encode("hr_jpeg_encode", e, pixels_dev, pixel_type, file_dev, capacity, "hr_jpeg_bound", length_dev, "length_dev")) return rc;
    HrJpegEncArgs a = {};
    a.pixels = pixels_dev;
    a.pixel_type = pixel_type;
    a.plan = e->plan;
    a.workspace = e->workspace;
    a.file = (uint8_t*)file_dev;
    a.file_bytes = length_dev;
    HR_HIP(hr_launch_jpeg_encode(a, (hipStream_t)stream));
    return HR_OK;
}

void hr_jpeg_encoder_destroy(hr_jpeg_encoder* e) { delete e; }
