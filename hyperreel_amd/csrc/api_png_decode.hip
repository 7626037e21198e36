// C ABI, PNG files decoded on the device: hr_png_probe / hr_png_decoder_create / hr_png_decode / hr_png_decoder_destroy (kernels:
// png_decode_kernel.hip; the format: hr_png_decode.h).  The decoder owns its workspace in device memory, so that the call itself only
// enqueues kernels on `stream`: no allocation, no synchronisation, no read-back, no memset.
#include <hip/hip_runtime.h>

#include <memory>

#include "hr_model.h"
#include "hr_png_decode.h"

struct hr_png_decoder {
    int32_t w = 0, h = 0, max_images = 0;
    int64_t max_file_bytes = 0, image_stride = 0, carry_offset = 0;
    DevMem<uint8_t> workspace;       // max_images * image_stride, then the images' meta words
};

int hr_png_probe(const void* file_host, int64_t n, hr_png_info* info)
{
    if (!file_host || !info) return fail(HR_E_INVALID, "hr_png_probe: null argument (%s)", !file_host ? "file_host" : "info");
    if (n < 0) return fail(HR_E_INVALID, "hr_png_probe: n %lld is negative", (long long)n);
    const int st = hr_png_read_head((const uint8_t*)file_host, n, info);
    if (st != HR_PNG_OK)
        return fail(HR_E_INVALID, "hr_png_probe: %s", st == HR_PNG_E_SIGNATURE ? "not a PNG signature" : st == HR_PNG_E_TRUNCATED
                    ? "fewer than the 33 bytes of a signature and IHDR" : "the first chunk is not a 13-byte IHDR with a size of 1 x 1 or more");
    return HR_OK;
}

int hr_png_decoder_create(int32_t w, int32_t h, int32_t max_images, int64_t max_file_bytes_total, hr_png_decoder** out)
{
    if (!out) return fail(HR_E_INVALID, "hr_png_decoder_create: null argument (out)");
    *out = nullptr;
    if (w < 1 || h < 1) return fail(HR_E_INVALID, "hr_png_decoder_create: size %d x %d (w, h) must be at least 1 x 1", (int)w, (int)h);
    if (max_images < 1) return fail(HR_E_INVALID, "hr_png_decoder_create: max_images %d must be at least 1", (int)max_images);
    if (max_file_bytes_total < 0) return fail(HR_E_INVALID, "hr_png_decoder_create: max_file_bytes_total %lld is negative", (long long)max_file_bytes_total);
    if (!hr_png_shape_ok(w, h, 4))
        return fail(HR_E_INVALID, "hr_png_decoder_create: %d x %d RGBA is more than %d bytes a row or %lld filtered bytes in all", (int)w, (int)h,
                    (int)HR_PNG_MAX_ROW_BYTES, (long long)HR_PNG_MAX_BYTES);
    std::unique_ptr<hr_png_decoder> d(new hr_png_decoder());
    d->w = w; d->h = h; d->max_images = max_images; d->max_file_bytes = max_file_bytes_total;
    d->carry_offset = (((int64_t)h * (1 + 4 * (int64_t)w) + 15) / 16) * 16;
    d->image_stride = d->carry_offset + ((4 * (int64_t)w + 15) / 16) * 16;
    const hipError_t err = d->workspace.alloc((size_t)(d->image_stride * max_images) + (size_t)max_images * HR_PNG_DEC_META_WORDS * sizeof(int32_t));
    if (err != hipSuccess) return fail(HR_E_HIP, "hr_png_decoder_create: %s", hipGetErrorString(err));
    *out = d.release();
    return HR_OK;
}

int hr_png_decode(hr_png_decoder* d, const void* files_dev, const int64_t* offsets_dev, int32_t n_images, int32_t out_channels, void* out_dev,
                  int32_t* status_dev, void* stream)
{
    if (!d) return fail(HR_E_INVALID, "hr_png_decode: null argument (decoder)");
    if (n_images < 0 || n_images > d->max_images)
        return fail(HR_E_INVALID, "hr_png_decode: n_images %d is outside [0, max_images %d]", (int)n_images, (int)d->max_images);
    if (out_channels != 1 && out_channels != 3 && out_channels != 4)
        return fail(HR_E_INVALID, "hr_png_decode: out_channels %d is not 1 (L), 3 (RGB) or 4 (RGBA)", (int)out_channels);
    if (n_images == 0) return HR_OK;
    if (!files_dev) return fail(HR_E_INVALID, "hr_png_decode: null argument (files_dev)");
    if (!offsets_dev) return fail(HR_E_INVALID, "hr_png_decode: null argument (offsets_dev)");
    if (!out_dev) return fail(HR_E_INVALID, "hr_png_decode: null argument (out_dev)");
    if (!status_dev) return fail(HR_E_INVALID, "hr_png_decode: null argument (status_dev)");
    if (((uintptr_t)offsets_dev) & 7) return fail(HR_E_INVALID, "hr_png_decode: offsets_dev must be 8-byte aligned");
    if (((uintptr_t)status_dev) & 3) return fail(HR_E_INVALID, "hr_png_decode: status_dev must be 4-byte aligned");
    HrPngDecodeArgs a = {};
    a.files = (const uint8_t*)files_dev;
    a.offsets = offsets_dev;
    a.max_file_bytes = d->max_file_bytes;
    a.w = d->w; a.h = d->h; a.n_images = n_images; a.out_channels = out_channels;
    a.filtered = d->workspace;
    a.image_stride = d->image_stride; a.carry_offset = d->carry_offset;
    a.meta = (int32_t*)((uint8_t*)d->workspace + d->image_stride * d->max_images);
    a.out = (uint8_t*)out_dev;
    a.status = status_dev;
    HR_HIP(hr_launch_png_decode(a, (hipStream_t)stream));
    return HR_OK;
}

void hr_png_decoder_destroy(hr_png_decoder* d) { delete d; }
