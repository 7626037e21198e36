// C ABI, JPEG files written: hr_jpeg_bound / hr_jpeg_encoder_create / hr_jpeg_encode / hr_jpeg_encoder_destroy (kernels:
// jpeg_encode_kernel.hip; the format's arithmetic and the plan: hr_jpeg_encode.h).  The encoder owns its workspace in device memory, the
// quantisation and Huffman tables and the file's header -- built on the host at create time -- at its start, so that the call itself only
// enqueues kernels on `stream`: no allocation, no synchronisation, no read-back, no memset.
#include <hip/hip_runtime.h>

#include <memory>

#include "hr_model.h"
#include "hr_jpeg_encode.h"

struct hr_jpeg_encoder {
    hr_jpeg_enc_plan_t plan = {};
    DevMem<uint8_t> workspace;
};

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
    const hipError_t err = e->workspace.alloc((size_t)e->plan.workspace_bytes);
    if (err != hipSuccess) return fail(HR_E_HIP, "hr_jpeg_encoder_create: %s", hipGetErrorString(err));
    HR_HIP(hipMemcpy((uint8_t*)e->workspace + e->plan.off_tables, t.get(), sizeof(hr_jpeg_enc_tables), hipMemcpyHostToDevice));
    *out = e.release();
    return HR_OK;
}

int hr_jpeg_encode(hr_jpeg_encoder* e, const void* pixels_dev, int32_t pixel_type, void* file_dev, int64_t capacity, int64_t* length_dev, void* stream)
{
    if (!e) return fail(HR_E_INVALID, "hr_jpeg_encode: null argument (encoder)");
    if (!pixels_dev) return fail(HR_E_INVALID, "hr_jpeg_encode: null argument (pixels_dev)");
    if (!file_dev) return fail(HR_E_INVALID, "hr_jpeg_encode: null argument (file_dev)");
    if (!length_dev) return fail(HR_E_INVALID, "hr_jpeg_encode: null argument (length_dev)");
    if (pixel_type != HR_PNG_U8 && pixel_type != HR_PNG_F32_TO8B)
        return fail(HR_E_INVALID, "hr_jpeg_encode: unknown pixel_type %d (HR_PNG_U8 0, HR_PNG_F32_TO8B 1)", (int)pixel_type);
    if (capacity < e->plan.bound)
        return fail(HR_E_INVALID, "hr_jpeg_encode: capacity %lld is below hr_jpeg_bound's %lld bytes", (long long)capacity, (long long)e->plan.bound);
    if (pixel_type == HR_PNG_F32_TO8B && (((uintptr_t)pixels_dev) & 3))
        return fail(HR_E_INVALID, "hr_jpeg_encode: a float frame (pixels_dev) must be 4-byte aligned");
    if (((uintptr_t)length_dev) & 7) return fail(HR_E_INVALID, "hr_jpeg_encode: length_dev must be 8-byte aligned");
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
