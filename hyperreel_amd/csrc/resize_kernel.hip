// PIL's 8-bit resize on the device (hr_image_resize; arithmetic and the choice of kernel: hr_resize.h).  One pass per axis, horizontal
// first, over interleaved RGB bytes; integer arithmetic only -- the coefficients come from the host.
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
#include "hr_kernels.h"
#include "hr_resize.h"

namespace {

constexpr int THREADS = 256;

// Copies global bytes [g, g + nbytes) to row + (g & 15) and on: chunk c of the row holds the 16 bytes at (g & ~15) + 16 c.  [lo, hi) is the
// source buffer: nothing outside it is read.  Called by `nthreads` threads with t = 0 .. nthreads - 1.
__device__ __forceinline__ void stage_bytes(unsigned char* row, const uint8_t* g, int nbytes, const uint8_t* lo, const uint8_t* hi, int t, int nthreads)
{
    const int off = (int)((uintptr_t)g & 15);
    const uint8_t* a0 = g - off;                      // (derived from g, not from an integer: the loads stay global loads)
    const int chunks = (off + nbytes + 15) >> 4;
    for (int c = t; c < chunks; c += nthreads) {
        const uint8_t* a = a0 + 16 * c;
        if (a >= lo && a + 16 <= hi) {
            *reinterpret_cast<uint4*>(row + 16 * c) = *reinterpret_cast<const uint4*>(a);
        } else {
            for (int b = 0; b < 16; ++b)
                if (a + b >= lo && a + b < hi) row[16 * c + b] = a[b];
        }
    }
}

template <bool MAD24>
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
        const uint8_t* g = src + (int64_t)y * p.src_pitch + (int64_t)px_lo * 3;
        unsigned char* row = rows + ry * p.row_pitch;
        __syncthreads();                              // the coefficient rows are in place; the last round's reads are over
        if (y < y_end) stage_bytes(row, g, (px_hi - px_lo) * 3, p.src_lo, p.src_hi, tx, 64);
        __syncthreads();
        if (y < y_end && tx < nx) {
            const unsigned char* px = row + ((uintptr_t)g & 15) + (xmin - px_lo) * 3;
            const int32_t* kr = sk + tx * p.ksize;
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

template <bool MAD24>
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
    for (int r = r_lo + wave; r < r_hi; r += THREADS / 64)
        stage_bytes(smem + (r - r_lo) * HR_RESIZE_V_PITCH, src + (int64_t)r * p.src_pitch, nb, p.src_lo, p.src_hi, lane, 64);
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
        dst[(int64_t)(y0 + yy) * p.dst_pitch + threadIdx.x] = hr_resize_finish(acc);
    }
}

// one thread per output byte.  vertical: `lines` counts the bytes of a row, a tap is a row apart; else the rows, a tap a pixel apart
template <bool MAD24>
__global__ __launch_bounds__(THREADS) void resize_general_kernel(const HrResizePass p, int vertical, int64_t total)
{
    const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (t >= total) return;
    const int64_t row_bytes = vertical ? p.lines : (int64_t)p.out * 3, rows = vertical ? p.out : p.lines;
    const int64_t j = t % row_bytes, y = (t / row_bytes) % rows, img = t / (row_bytes * rows);
    const int64_t o = vertical ? y : j / 3;                                            // the output's index along the axis
    const int32_t first = p.bounds[2 * o], n = p.bounds[2 * o + 1];
    const uint8_t* px = p.src + img * p.src_image + (vertical ? first * p.src_pitch + j : y * p.src_pitch + (int64_t)first * 3 + j % 3);
    p.dst[img * p.dst_image + y * p.dst_pitch + j] = hr_resize_dot<MAD24>(px, vertical ? p.src_pitch : 3, p.k + o * p.ksize, n);
}

}  // namespace

int64_t hr_resize_pass_blocks(const HrResizePass& p, bool vertical, int n_images)
{
    if (!p.staged) return ((int64_t)n_images * (vertical ? (int64_t)p.out * p.lines : (int64_t)p.lines * p.out * 3) + THREADS - 1) / THREADS;
    if (vertical) return (int64_t)n_images * ((p.lines + HR_RESIZE_V_BYTES - 1) / HR_RESIZE_V_BYTES) * ((p.out + p.tile - 1) / p.tile);
    return (int64_t)n_images * ((p.out + HR_RESIZE_H_TILE - 1) / HR_RESIZE_H_TILE)
           * ((p.lines + HR_RESIZE_H_ROWS_PER_GROUP - 1) / HR_RESIZE_H_ROWS_PER_GROUP);
}

namespace {

template <bool MAD24>
hipError_t launch(const HrResizePass& p, bool vertical, int n_images, hipStream_t stream)
{
    const dim3 grid((unsigned)hr_resize_pass_blocks(p, vertical, n_images));
    if (!p.staged) {
        const int64_t total = (int64_t)n_images * (vertical ? (int64_t)p.out * p.lines : (int64_t)p.lines * p.out * 3);
        hipLaunchKernelGGL(resize_general_kernel<MAD24>, grid, dim3(THREADS), 0, stream, p, (int)vertical, total);
    } else if (vertical) {
        hipLaunchKernelGGL(resize_vertical_kernel<MAD24>, grid, dim3(THREADS), (size_t)p.lds_bytes, stream, p);
    } else {
        hipLaunchKernelGGL(resize_horizontal_kernel<MAD24>, grid, dim3(THREADS), (size_t)p.lds_bytes, stream, p);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t hr_launch_resize_pass(const HrResizePass& p, bool vertical, int n_images, hipStream_t stream)
{
    return p.mad24 ? launch<true>(p, vertical, n_images, stream) : launch<false>(p, vertical, n_images, stream);
}
