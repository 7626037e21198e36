// PIL's 8-bit resize on the device (hr_image_resize; arithmetic and the choice of kernel: hr_resize.h).  One pass per axis, horizontal
// first, over interleaved RGB or RGBA bytes; integer arithmetic only -- the coefficients come from the host.
//   staged kernels   a workgroup copies the source bytes its tile reads into LDS with aligned 16-byte loads (rows of 3-byte pixels start
//                    at any address: the chunk that holds a row's first byte is loaded whole, and the bytes keep their address modulo
//                    16 in LDS), then every tap is an LDS byte read.  Only chunks that lie wholly inside the source buffer are loaded
//                    wide; the buffer's first and last chunk go byte by byte.
//                    horizontal: a tile is 64 output pixels x 4 rows, one thread each with three accumulators; the tile's coefficient
//                    rows are staged once (ksize is odd, so thread t's row t * ksize + x meets no bank conflict) and serve 16 rows.
//                    vertical: a tile is 256 bytes of a row x up to 8 output rows, one thread per byte column; a row's coefficients
//                    are uniform over the workgroup.
//   general kernel   one thread per output byte, taps and coefficients from global memory: any ksize.
// Every kernel sums with hr_resize_mad and ends with hr_resize_finish, the functions the host statement is made of.
// RGBA (CH = 4; HrResizePass::premultiply / unpremultiply): PIL resamples premultiplied bytes, and both conversions are fused into the
// passes.  hr_premultiply_pixel runs where the first pass that runs reads its source -- in the staging copy, once per staged pixel (a
// 4-byte aligned pixel never straddles a 16-byte chunk) -- and hr_unpremultiply where the last pass that runs writes its result: the
// horizontal thread holds the whole pixel and stores it as one word; the vertical thread owns one byte and fetches its pixel's alpha
// from lane (lane | 3) of its wavefront.  The general kernel recomputes the alpha sum per byte instead.
#include "hr_kernels.h"
#include "hr_resize.h"

namespace {

constexpr int THREADS = 256;

// Copies global bytes [g, g + nbytes) to row + (g & 15) and on: chunk c of the row holds the 16 bytes at (g & ~15) + 16 c.  [lo, hi) is the
// source buffer: nothing outside it is read.  Called by `nthreads` threads with t = 0 .. nthreads - 1.
// PREMUL: the bytes are 4-byte aligned RGBA pixels (g, lo and hi are multiples of 4), premultiplied on their way.
template <bool PREMUL>
__device__ __forceinline__ void stage_bytes(unsigned char* row, const uint8_t* g, int nbytes, const uint8_t* lo, const uint8_t* hi, int t, int nthreads)
{
    const int off = (int)((uintptr_t)g & 15);
    const uint8_t* a0 = g - off;                      // (derived from g, not from an integer: the loads stay global loads)
    const int chunks = (off + nbytes + 15) >> 4;
    for (int c = t; c < chunks; c += nthreads) {
        const uint8_t* a = a0 + 16 * c;
        if (a >= lo && a + 16 <= hi) {
            uint4 v = *reinterpret_cast<const uint4*>(a);
            if (PREMUL) {
                v.x = hr_premultiply_pixel(v.x); v.y = hr_premultiply_pixel(v.y);
                v.z = hr_premultiply_pixel(v.z); v.w = hr_premultiply_pixel(v.w);
            }
            *reinterpret_cast<uint4*>(row + 16 * c) = v;
        } else if (PREMUL) {
            for (int b = 0; b < 16; b += 4)
                if (a + b >= lo && a + b + 4 <= hi)
                    *reinterpret_cast<uint32_t*>(row + 16 * c + b) = hr_premultiply_pixel(*reinterpret_cast<const uint32_t*>(a + b));
        } else {
            for (int b = 0; b < 16; ++b)
                if (a + b >= lo && a + b < hi) row[16 * c + b] = a[b];
        }
    }
}

template <bool MAD24, int CH>
__global__ __launch_bounds__(THREADS) void resize_horizontal_kernel(const HrResizePass p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int32_t* sk = reinterpret_cast<int32_t*>(smem);
    unsigned char* rows = smem + (size_t)HR_RESIZE_H_TILE * p.ksize * 4;
    const int tiles_x = (p.out + HR_RESIZE_H_TILE - 1) / HR_RESIZE_H_TILE;
    const int groups_y = (p.lines + HR_RESIZE_H_ROWS_PER_GROUP - 1) / HR_RESIZE_H_ROWS_PER_GROUP;
    const int tx_i = blockIdx.x % tiles_x, gy = (blockIdx.x / tiles_x) % groups_y, img = blockIdx.x / (tiles_x * groups_y);
    const int x0 = tx_i * HR_RESIZE_H_TILE, nx = min(HR_RESIZE_H_TILE, p.out - x0);
    const int tx = threadIdx.x & 63, ry = threadIdx.x >> 6;

    for (int i = threadIdx.x; i < nx * p.ksize; i += THREADS) sk[i] = p.k[(int64_t)x0 * p.ksize + i];
    const int px_lo = p.bounds[2 * x0];
    const int px_hi = p.bounds[2 * (x0 + nx - 1)] + p.bounds[2 * (x0 + nx - 1) + 1];
    const int xmin = tx < nx ? p.bounds[2 * (x0 + tx)] : 0, n = tx < nx ? p.bounds[2 * (x0 + tx) + 1] : 0;
    const uint8_t* src = p.src + (int64_t)img * p.src_image;
    uint8_t* dst = p.dst + (int64_t)img * p.dst_image;
    const int y_end = min(p.lines, (gy + 1) * HR_RESIZE_H_ROWS_PER_GROUP);

    for (int yb = gy * HR_RESIZE_H_ROWS_PER_GROUP; yb < y_end; yb += HR_RESIZE_H_ROWS) {
        const int y = yb + ry;                        // wavefront ry stages and resamples row y
        const uint8_t* g = src + (int64_t)y * p.src_pitch + (int64_t)px_lo * CH;
        unsigned char* row = rows + ry * p.row_pitch;
        __syncthreads();                              // the coefficient rows are in place; the last round's reads are over
        if (y < y_end) {
            if (CH == 4 && p.premultiply) stage_bytes<true>(row, g, (px_hi - px_lo) * CH, p.src_lo, p.src_hi, tx, 64);
            else stage_bytes<false>(row, g, (px_hi - px_lo) * CH, p.src_lo, p.src_hi, tx, 64);
        }
        __syncthreads();
        if (y < y_end && tx < nx) {
            const unsigned char* px = row + ((uintptr_t)g & 15) + (xmin - px_lo) * CH;
            const int32_t* kr = sk + tx * p.ksize;
            if (CH == 4) {                            // a tap is one aligned LDS word; the pixel leaves as one word
                const uint32_t* pw = reinterpret_cast<const uint32_t*>(px);
                int32_t a0 = hr_resize_acc0(), a1 = a0, a2 = a0, a3 = a0;
                for (int x = 0; x < n; ++x) {
                    const int32_t kk = kr[x];
                    const uint32_t w = pw[x];
                    a0 = hr_resize_mad<MAD24>(a0, (uint8_t)w, kk);
                    a1 = hr_resize_mad<MAD24>(a1, (uint8_t)(w >> 8), kk);
                    a2 = hr_resize_mad<MAD24>(a2, (uint8_t)(w >> 16), kk);
                    a3 = hr_resize_mad<MAD24>(a3, (uint8_t)(w >> 24), kk);
                }
                uint8_t c0 = hr_resize_finish(a0), c1 = hr_resize_finish(a1), c2 = hr_resize_finish(a2);
                const uint8_t al = hr_resize_finish(a3);
                if (p.unpremultiply) { c0 = hr_unpremultiply(c0, al); c1 = hr_unpremultiply(c1, al); c2 = hr_unpremultiply(c2, al); }
                *reinterpret_cast<uint32_t*>(dst + (int64_t)y * p.dst_pitch + (int64_t)(x0 + tx) * 4) =
                    (uint32_t)c0 | (uint32_t)c1 << 8 | (uint32_t)c2 << 16 | (uint32_t)al << 24;
            } else {
                int32_t a0 = hr_resize_acc0(), a1 = a0, a2 = a0;
                for (int x = 0; x < n; ++x) {
                    const int32_t kk = kr[x];
                    a0 = hr_resize_mad<MAD24>(a0, px[3 * x], kk);
                    a1 = hr_resize_mad<MAD24>(a1, px[3 * x + 1], kk);
                    a2 = hr_resize_mad<MAD24>(a2, px[3 * x + 2], kk);
                }
                uint8_t* o = dst + (int64_t)y * p.dst_pitch + (int64_t)(x0 + tx) * 3;
                o[0] = hr_resize_finish(a0);
                o[1] = hr_resize_finish(a1);
                o[2] = hr_resize_finish(a2);
            }
        }
    }
}

template <bool MAD24, int CH>
__global__ __launch_bounds__(THREADS) void resize_vertical_kernel(const HrResizePass p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tiles_x = (p.lines + HR_RESIZE_V_BYTES - 1) / HR_RESIZE_V_BYTES;        // here `lines` counts the bytes of a row
    const int tiles_y = (p.out + p.tile - 1) / p.tile;
    const int tx_i = blockIdx.x % tiles_x, ty_i = (blockIdx.x / tiles_x) % tiles_y, img = blockIdx.x / (tiles_x * tiles_y);
    const int j0 = tx_i * HR_RESIZE_V_BYTES, nb = min(HR_RESIZE_V_BYTES, p.lines - j0);
    const int y0 = ty_i * p.tile, ny = min(p.tile, p.out - y0);
    const int r_lo = p.bounds[2 * y0];
    const int r_hi = p.bounds[2 * (y0 + ny - 1)] + p.bounds[2 * (y0 + ny - 1) + 1];
    const uint8_t* src = p.src + (int64_t)img * p.src_image + j0;
    uint8_t* dst = p.dst + (int64_t)img * p.dst_image + j0;

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int r = r_lo + wave; r < r_hi; r += THREADS / 64) {
        unsigned char* row = smem + (r - r_lo) * HR_RESIZE_V_PITCH;
        if (CH == 4 && p.premultiply) stage_bytes<true>(row, src + (int64_t)r * p.src_pitch, nb, p.src_lo, p.src_hi, lane, 64);
        else stage_bytes<false>(row, src + (int64_t)r * p.src_pitch, nb, p.src_lo, p.src_hi, lane, 64);
    }
    __syncthreads();
    if ((int)threadIdx.x >= nb) return;
    const int step = (int)(p.src_pitch & 15);
    for (int yy = 0; yy < ny; ++yy) {
        const int ymin = p.bounds[2 * (y0 + yy)], n = p.bounds[2 * (y0 + yy) + 1];
        const int32_t* kr = p.k + (int64_t)(y0 + yy) * p.ksize;
        const unsigned char* px = smem + (ymin - r_lo) * HR_RESIZE_V_PITCH + threadIdx.x;
        int off = (int)((uintptr_t)(src + (int64_t)ymin * p.src_pitch) & 15);         // where the row's bytes begin in its LDS row
        int32_t acc = hr_resize_acc0();
        for (int x = 0; x < n; ++x) {
            acc = hr_resize_mad<MAD24>(acc, px[off], kr[x]);
            px += HR_RESIZE_V_PITCH;
            off = (off + step) & 15;
        }
        uint8_t v = hr_resize_finish(acc);
        if (CH == 4 && p.unpremultiply) {
            // nb is a multiple of 4 and so is a tile's first byte: the lanes of a pixel are all here, its alpha in the last of them
            const uint8_t al = (uint8_t)__shfl((int)v, lane | 3, 64);
            if ((lane & 3) != 3) v = hr_unpremultiply(v, al);
        }
        dst[(int64_t)(y0 + yy) * p.dst_pitch + threadIdx.x] = v;
    }
}

// one thread per output byte.  vertical: `lines` counts the bytes of a row, a tap is a row apart; else the rows, a tap a pixel apart
template <bool MAD24, int CH>
__global__ __launch_bounds__(THREADS) void resize_general_kernel(const HrResizePass p, int vertical, int64_t total)
{
    const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (t >= total) return;
    const int64_t row_bytes = vertical ? p.lines : (int64_t)p.out * CH, rows = vertical ? p.out : p.lines;
    const int64_t j = t % row_bytes, y = (t / row_bytes) % rows, img = t / (row_bytes * rows);
    const int64_t o = vertical ? y : j / CH;                                           // the output's index along the axis
    const int32_t first = p.bounds[2 * o], n = p.bounds[2 * o + 1];
    const uint8_t* px = p.src + img * p.src_image + (vertical ? first * p.src_pitch + j : y * p.src_pitch + (int64_t)first * CH + j % CH);
    const int64_t stride = vertical ? p.src_pitch : CH;
    const int32_t* k = p.k + o * p.ksize;
    uint8_t* out = p.dst + img * p.dst_image + y * p.dst_pitch + j;
    const int to_alpha = 3 - (int)(j & 3);           // CH == 4: from a byte to its pixel's alpha (rows and pixels are 4-byte aligned)
    if (CH == 4 && to_alpha != 0 && (p.premultiply || p.unpremultiply)) {
        // a colour byte: its own sum over premultiplied taps, and the alpha's sum again where the result is un-premultiplied
        int32_t acc = hr_resize_acc0(), acc_a = acc;
        for (int32_t x = 0; x < n; ++x) {
            const uint8_t c = px[x * stride], a = px[x * stride + to_alpha];
            acc = hr_resize_mad<MAD24>(acc, p.premultiply ? hr_premultiply(c, a) : c, k[x]);
            acc_a = hr_resize_mad<MAD24>(acc_a, a, k[x]);
        }
        const uint8_t v = hr_resize_finish(acc);
        *out = p.unpremultiply ? hr_unpremultiply(v, hr_resize_finish(acc_a)) : v;
        return;
    }
    *out = hr_resize_dot<MAD24>(px, stride, k, n);
}

}  // namespace

int64_t hr_resize_pass_blocks(const HrResizePass& p, bool vertical, int n_images)
{
    if (!p.staged) return ((int64_t)n_images * (vertical ? (int64_t)p.out * p.lines : (int64_t)p.lines * p.out * p.channels) + THREADS - 1) / THREADS;
    if (vertical) return (int64_t)n_images * ((p.lines + HR_RESIZE_V_BYTES - 1) / HR_RESIZE_V_BYTES) * ((p.out + p.tile - 1) / p.tile);
    return (int64_t)n_images * ((p.out + HR_RESIZE_H_TILE - 1) / HR_RESIZE_H_TILE)
           * ((p.lines + HR_RESIZE_H_ROWS_PER_GROUP - 1) / HR_RESIZE_H_ROWS_PER_GROUP);
}

namespace {

template <bool MAD24, int CH>
hipError_t launch(const HrResizePass& p, bool vertical, int n_images, hipStream_t stream)
{
    const dim3 grid((unsigned)hr_resize_pass_blocks(p, vertical, n_images));
    if (!p.staged) {
        const int64_t total = (int64_t)n_images * (vertical ? (int64_t)p.out * p.lines : (int64_t)p.lines * p.out * CH);
        hipLaunchKernelGGL((resize_general_kernel<MAD24, CH>), grid, dim3(THREADS), 0, stream, p, (int)vertical, total);
    } else if (vertical) {
        hipLaunchKernelGGL((resize_vertical_kernel<MAD24, CH>), grid, dim3(THREADS), (size_t)p.lds_bytes, stream, p);
    } else {
        hipLaunchKernelGGL((resize_horizontal_kernel<MAD24, CH>), grid, dim3(THREADS), (size_t)p.lds_bytes, stream, p);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t hr_launch_resize_pass(const HrResizePass& p, bool vertical, int n_images, hipStream_t stream)
{
    if (p.channels == 4) return p.mad24 ? launch<true, 4>(p, vertical, n_images, stream) : launch<false, 4>(p, vertical, n_images, stream);
    return p.mad24 ? launch<true, 3>(p, vertical, n_images, stream) : launch<false, 3>(p, vertical, n_images, stream);
}
