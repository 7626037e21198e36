// C ABI, PNG and JPEG files decoded on the device: hr_{png,jpeg}_probe / _decoder_create / _decode / _decoder_destroy (kernels:
// png_decode_kernel.hip, jpeg_decode_kernel.hip; the formats: hr_png_decode.h, hr_jpeg_decode.h).  A decoder owns its workspace in device
// memory, so that the call itself only enqueues kernels on `stream`: no allocation, no synchronisation, no read-back, no memset.
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "hr_model.h"
#include "hr_jpeg_decode.h"
#include "hr_png_decode.h"

struct hr_png_decoder {
    int32_t w = 0, h = 0, max_images = 0;
    int64_t max_file_bytes = 0, image_stride = 0, carry_offset = 0;
    DevMem<uint8_t> workspace;       // max_images * image_stride, then the images' meta words
};

struct hr_jpeg_decoder {
    int32_t w = 0, h = 0, max_images = 0, sub_bytes = 0;
    int64_t max_file_bytes = 0, max_units = 0, max_blocks = 0, total_slots = 0;
    size_t off_ustart = 0, off_ustat = 0, off_urounds = 0, off_slots = 0, off_coef = 0, off_planes = 0;
    DevMem<uint8_t> workspace;
};

namespace {

// the arguments hr_*_decoder_create share, `who` being the caller; *out is null from here on
template <class D> int check_create(const char* who, int32_t max_images, int64_t max_file_bytes_total, D** out)
{
    if (!out) return fail(HR_E_INVALID, "%s: null argument (out)", who);
    *out = nullptr;
    if (max_images < 1) return fail(HR_E_INVALID, "%s: max_images %d must be at least 1", who, (int)max_images);
    if (max_file_bytes_total < 0) return fail(HR_E_INVALID, "%s: max_file_bytes_total %lld is negative", who, (long long)max_file_bytes_total);
    return HR_OK;
}

// the batch of hr_*_decode, d being either decoder; rounds_dev (may be null) and its name are hr_jpeg_decode's; an empty batch is HR_OK
template <class D> int check_batch(const char* who, const D* d, const void* files_dev, const int64_t* offsets_dev, int32_t n_images,
                                   int32_t out_channels, const void* out_dev, const int32_t* status_dev, const int32_t* rounds_dev, const char* and_rounds)
{
    if (!d) return fail(HR_E_INVALID, "%s: null argument (decoder)", who);
    if (n_images < 0 || n_images > d->max_images)
        return fail(HR_E_INVALID, "%s: n_images %d is outside [0, max_images %d]", who, (int)n_images, (int)d->max_images);
    if (out_channels != 1 && out_channels != 3 && out_channels != 4)
        return fail(HR_E_INVALID, "%s: out_channels %d is not 1 (L), 3 (RGB) or 4 (RGBA)", who, (int)out_channels);
    if (n_images == 0) return HR_OK;
    if (!files_dev) return fail(HR_E_INVALID, "%s: null argument (files_dev)", who);
    if (!offsets_dev) return fail(HR_E_INVALID, "%s: null argument (offsets_dev)", who);
    if (!out_dev) return fail(HR_E_INVALID, "%s: null argument (out_dev)", who);
    if (!status_dev) return fail(HR_E_INVALID, "%s: null argument (status_dev)", who);
    if (((uintptr_t)offsets_dev) & 7) return fail(HR_E_INVALID, "%s: offsets_dev must be 8-byte aligned", who);
    if ((((uintptr_t)status_dev) | ((uintptr_t)rounds_dev)) & 3) return fail(HR_E_INVALID, "%s: status_dev%s must be 4-byte aligned", who, and_rounds);
    return HR_OK;
}

}  // namespace

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
    if (int rc = check_create("hr_png_decoder_create", max_images, max_file_bytes_total, out)) return rc;
    if (w < 1 || h < 1) return fail(HR_E_INVALID, "hr_png_decoder_create: size %d x %d (w, h) must be at least 1 x 1", (int)w, (int)h);
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
    const int rc = check_batch("hr_png_decode", d, files_dev, offsets_dev, n_images, out_channels, out_dev, status_dev, nullptr, "");
    if (rc != HR_OK || n_images == 0) return rc;
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

int hr_jpeg_probe(const void* file_host, int64_t n, hr_jpeg_info* info)
{
    if (!file_host || !info) return fail(HR_E_INVALID, "hr_jpeg_probe: null argument (%s)", !file_host ? "file_host" : "info");
    if (n < 0) return fail(HR_E_INVALID, "hr_jpeg_probe: n %lld is negative", (long long)n);
    std::vector<hr_jpeg_parse_mem> mem(1);
    std::vector<hr_jpeg_desc> desc(1);
    const int st = hr_jpeg_parse_head((const uint8_t*)file_host, n, mem.data(), desc.data());
    hr_jpeg_fill_info(desc.data(), st, info);
    if (st == HR_JPEG_E_SOI) return fail(HR_E_INVALID, "hr_jpeg_probe: no SOI marker at the start");
    if (info->width < 1 || info->height < 1) return fail(HR_E_INVALID, "hr_jpeg_probe: no frame header with a size (JPEG status %d)", st);
    return HR_OK;
}

int hr_jpeg_decoder_create(int32_t w, int32_t h, int32_t max_images, int64_t max_file_bytes_total, int32_t subseq_bits, hr_jpeg_decoder** out)
{
    if (int rc = check_create("hr_jpeg_decoder_create", max_images, max_file_bytes_total, out)) return rc;
    if (w < 1 || h < 1 || w > 65535 || h > 65535) return fail(HR_E_INVALID, "hr_jpeg_decoder_create: size %d x %d (w, h) must be 1 x 1 to 65535 x 65535", (int)w, (int)h);
    if ((int64_t)w * h * 4 > (1ll << 31)) return fail(HR_E_INVALID, "hr_jpeg_decoder_create: %d x %d RGBA is more than 2^31 bytes", (int)w, (int)h);
    if (subseq_bits != 0 && (subseq_bits < 128 || subseq_bits % 32 != 0))
        return fail(HR_E_INVALID, "hr_jpeg_decoder_create: subseq_bits %d must be 0 (default) or a multiple of 32 from 128 up", (int)subseq_bits);
    std::unique_ptr<hr_jpeg_decoder> d(new hr_jpeg_decoder());
    d->w = w; d->h = h; d->max_images = max_images; d->max_file_bytes = max_file_bytes_total;
    d->sub_bytes = (subseq_bits ? subseq_bits : HR_JPEG_DEFAULT_SUBSEQ_BITS) / 8;
    d->max_units = hr_jpeg_max_units(w, h);
    d->max_blocks = hr_jpeg_max_blocks(w, h);
    d->total_slots = max_file_bytes_total / d->sub_bytes + (int64_t)max_images * (d->max_units + 1) + 2;
    size_t at = 0;
    const auto take = [&at](size_t bytes) { const size_t here = at; at += (bytes + 255) / 256 * 256; return here; };
    take(sizeof(hr_jpeg_desc) * (size_t)max_images);
    d->off_ustart = take(sizeof(int32_t) * (size_t)max_images * (size_t)(d->max_units + 2));
    d->off_ustat = take(sizeof(int32_t) * (size_t)max_images * (size_t)(d->max_units + 1));
    d->off_urounds = take(sizeof(int32_t) * (size_t)max_images * (size_t)(d->max_units + 1));
    d->off_slots = take(sizeof(int32_t) * 5 * (size_t)d->total_slots);
    d->off_coef = take(sizeof(int16_t) * 64 * (size_t)max_images * (size_t)d->max_blocks);
    d->off_planes = take(64 * (size_t)max_images * (size_t)d->max_blocks);
    const hipError_t err = d->workspace.alloc(at);
    if (err != hipSuccess) return fail(HR_E_HIP, "hr_jpeg_decoder_create: %s", hipGetErrorString(err));
    *out = d.release();
    return HR_OK;
}

int hr_jpeg_decode(hr_jpeg_decoder* d, const void* files_dev, const int64_t* offsets_dev, int32_t n_images, int32_t out_channels, void* out_dev,
                   int32_t* status_dev, int32_t* rounds_dev, void* stream)
{
    const int rc = check_batch("hr_jpeg_decode", d, files_dev, offsets_dev, n_images, out_channels, out_dev, status_dev, rounds_dev, " and rounds_dev");
    if (rc != HR_OK || n_images == 0) return rc;
    uint8_t* ws = d->workspace;
    HrJpegDecodeArgs a = {};
    a.files = (const uint8_t*)files_dev;
    a.offsets = offsets_dev;
    a.max_file_bytes = d->max_file_bytes; a.max_units = d->max_units; a.max_blocks = d->max_blocks; a.total_slots = d->total_slots;
    a.w = d->w; a.h = d->h; a.n_images = n_images; a.out_channels = out_channels; a.sub_bytes = d->sub_bytes;
    a.desc = (hr_jpeg_desc*)ws;
    a.ustart = (int32_t*)(ws + d->off_ustart);
    a.ustat = (int32_t*)(ws + d->off_ustat);
    a.urounds = (int32_t*)(ws + d->off_urounds);
    a.slots = (int32_t*)(ws + d->off_slots);
    a.coef = (int16_t*)(ws + d->off_coef);
    a.planes = ws + d->off_planes;
    a.out = (uint8_t*)out_dev;
    a.status = status_dev;
    a.rounds = rounds_dev;
    HR_HIP(hr_launch_jpeg_decode(a, (hipStream_t)stream));
    return HR_OK;
}

void hr_jpeg_decoder_destroy(hr_jpeg_decoder* d) { delete d; }
