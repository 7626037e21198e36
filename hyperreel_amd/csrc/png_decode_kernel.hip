// PNG files in device memory -> pixels in device memory (hr_png_decode; every rule of the format: hr_png_decode.h, which the host decoder
// calls too, so both give the same bytes and the same status).  One image per workgroup of one wavefront in each of three kernels; the
// batch is the parallel axis -- a DEFLATE stream is serial:
//   png_walk_kernel      the chunk headers one after another; the lanes checksum slices of each chunk, merged by the x^(8 n) rule.
//                        Writes the status, the file's channels and the first IDAT chunk's offset to the image's meta words.
//   png_inflate_kernel   hr_png_inflate: all lanes follow the one symbol stream (the same reads, the same tables in LDS; the file comes
//                        through a 4 KB stage in LDS, so the bit buffer never waits for global memory), lanes split the
//                        table fills, the match copies inside the 32 KB window in LDS, its flush to the filtered bytes in pieces and
//                        the Adler-32 of each piece.  A back-reference never reads global memory.
//   png_unfilter_kernel  rows in bands of 64: lane r takes row r of the band and runs one pixel behind lane r - 1, whose last two results
//                        reach it by a lane shift as "up" and "upper left".  A band's last row goes to the image's carry row for the next
//                        band's lane 0.  The pixel is converted to the output channels at the store.  An image whose status is not OK
//                        -- or one of whose filter bytes is above 4 -- is written as zeros here, so every output byte is written.
// Integer arithmetic only, no atomics on global memory, no wait between workgroups, no memset.
#include "hr_png_decode.h"

namespace {

enum { META_STATUS = 0, META_CHANNELS = 1, META_IDAT_LO = 2, META_IDAT_HI = 3 };

// the image's file, or false when offsets_dev does not delimit one inside the files buffer
__device__ __forceinline__ bool image_file(const HrPngDecodeArgs& a, int img, const uint8_t** f, int64_t* n)
{
    const int64_t lo = a.offsets[img], hi = a.offsets[img + 1];
    if (lo < 0 || hi < lo || hi > a.max_file_bytes) return false;
    *f = a.files + lo;
    *n = hi - lo;
    return true;
}

__global__ __launch_bounds__(64) void png_walk_kernel(const HrPngDecodeArgs a)
{
    const int img = blockIdx.x, lane = threadIdx.x;
    const uint8_t* f;
    int64_t n, idat_at = 0;
    hr_png_info info;
    info.channels = 0;
    const int st = image_file(a, img, &f, &n) ? hr_png_walk(f, n, a.w, a.h, &info, &idat_at, lane, 64) : HR_PNG_E_OFFSETS;
    if (lane == 0) {
        int32_t* meta = a.meta + (size_t)img * HR_PNG_DEC_META_WORDS;
        meta[META_STATUS] = st;
        meta[META_CHANNELS] = info.channels;
        meta[META_IDAT_LO] = (int32_t)(uint32_t)idat_at;
        meta[META_IDAT_HI] = (int32_t)(idat_at >> 32);
    }
}

__global__ __launch_bounds__(64) void png_inflate_kernel(const HrPngDecodeArgs a)
{
    __shared__ hr_png_inflate_mem mem;
    const int img = blockIdx.x, lane = threadIdx.x & 63;     // & 63: the loops over whole multiples of 64 then need no lane mask

    int32_t* meta = a.meta + (size_t)img * HR_PNG_DEC_META_WORDS;
    if (HR_PNG_UNIFORM(meta[META_STATUS]) != HR_PNG_OK) return;
    const uint8_t* f;
    int64_t n;
    if (!image_file(a, img, &f, &n)) return;                  // the walk has said so already
    const int64_t idat_at = (int64_t)HR_PNG_UNIFORM(meta[META_IDAT_LO]) | ((int64_t)HR_PNG_UNIFORM(meta[META_IDAT_HI]) << 32);
    const int64_t total = (int64_t)a.h * (1 + (int64_t)a.w * (int64_t)HR_PNG_UNIFORM(meta[META_CHANNELS]));
    const int st = hr_png_inflate(f, (uint32_t)n, (uint32_t)idat_at, a.filtered + (size_t)img * a.image_stride, (uint32_t)total, &mem, lane, 64);
    if (lane == 0) meta[META_STATUS] = st;
}

__device__ __forceinline__ uint32_t load_pixel(const uint8_t* p, int bpp)
{
    uint32_t v = p[0];
    if (bpp > 1) v |= (uint32_t)p[1] << 8;
    if (bpp > 2) v |= (uint32_t)p[2] << 16;
    if (bpp > 3) v |= (uint32_t)p[3] << 24;
    return v;
}

__global__ __launch_bounds__(64) void png_unfilter_kernel(const HrPngDecodeArgs a)
{
    const int img = blockIdx.x, lane = threadIdx.x;
    const int32_t* meta = a.meta + (size_t)img * HR_PNG_DEC_META_WORDS;
    const int32_t w = a.w, h = a.h, oc = a.out_channels, c = meta[META_CHANNELS];
    const int64_t row_bytes = 1 + (int64_t)w * c, n_out = (int64_t)h * w * oc;
    const uint8_t* filt = a.filtered + (size_t)img * a.image_stride;
    uint32_t* carry = (uint32_t*)(a.filtered + (size_t)img * a.image_stride + a.carry_offset);
    uint8_t* __restrict__ out = a.out + (size_t)img * (size_t)n_out;
    int st = meta[META_STATUS];
    if (st == HR_PNG_OK) {
        uint32_t bad = 0;
        for (int32_t y = lane; y < h; y += 64) bad |= filt[(size_t)y * row_bytes] > 4 ? 1u : 0u;
        if (__any((int)bad)) st = HR_PNG_E_FILTER;
    }
    if (lane == 0) a.status[img] = st;
    if (st != HR_PNG_OK) {
        for (int64_t i = lane; i < n_out; i += 64) out[i] = 0;
        return;
    }
    for (int32_t y0 = 0; y0 < h; y0 += 64) {
        const int32_t y = y0 + lane;
        const bool row_on = y < h;
        const uint8_t* row = filt + (size_t)(row_on ? y : 0) * row_bytes;
        const int f = row_on ? row[0] : 0;
        uint8_t* o = out + (size_t)(row_on ? y : 0) * w * oc;
        uint32_t left = 0, last = 0, last2 = 0, carry_prev = 0;
        for (int32_t s = 0; s < w + 63; ++s) {
            const int32_t x = s - lane;
            uint32_t up = __shfl_up(last, 1), up_left = __shfl_up(last2, 1);
            const bool on = row_on && x >= 0 && x < w;
            if (lane == 0) {
                // the carry row was stored by lane 63 during the band before.  A plain load could be served from this CU's vector
                // cache, which a store does not update; the agent-scope load reads where the stores land.  It is a load, not a
                // read-modify-write: the kernel has no atomic operation on global memory.
                up_left = carry_prev;
                up = (on && y0 > 0) ? __hip_atomic_load(carry + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
                carry_prev = up;
            }
            if (on) {
                const uint32_t v = hr_png_unfilter_pixel(f, load_pixel(row + 1 + (size_t)x * c, c), left, up, up_left, c);
                left = v; last2 = last; last = v;
                const uint32_t px = hr_png_convert_pixel(v, c, oc);
                uint8_t* q = o + (size_t)x * oc;
                q[0] = (uint8_t)px;
                if (oc > 1) { q[1] = (uint8_t)(px >> 8); q[2] = (uint8_t)(px >> 16); }
                if (oc > 3) q[3] = (uint8_t)(px >> 24);
                if (lane == 63) carry[x] = v;
            }
        }
        __threadfence();                                      // the carry row's stores before the next band's loads
    }
}

}  // namespace

hipError_t hr_launch_png_decode(const HrPngDecodeArgs& a, hipStream_t stream)
{
    const unsigned n = (unsigned)a.n_images;
    hipLaunchKernelGGL(png_walk_kernel, dim3(n), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(png_inflate_kernel, dim3(n), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(png_unfilter_kernel, dim3(n), dim3(64), 0, stream, a);
    return hipGetLastError();
}
