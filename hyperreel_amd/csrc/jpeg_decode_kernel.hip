// JPEG files in device memory -> pixels in device memory (hr_jpeg_decode; every rule of the format: hr_jpeg_decode.h, which the host
// decoder calls too, so both give the same bytes, the same status and the same rounds).  Six kernels, gfx950, wave64:
//   jpeg_parse_kernel    a workgroup of 256 per image.  Lane 0 reads the markers and builds the quantisation and Huffman tables into the
//                        image's descriptor; all lanes then search the entropy data for RSTn and the end of the scan and list the units.
//   jpeg_zero_kernel     zeroes the coefficients of the blocks the image has.
//   jpeg_entropy_kernel  a workgroup of 1024 per unit (restart interval, or the whole scan): hr_jpeg_entropy_unit -- a lane per
//                        subsequence, rounds until no subsequence's start changes, the prefix sum of completed data units, the write
//                        pass, DC differences into DC values.  All state of a round lives in the decoder's workspace; the barrier between
//                        the phases of a round is the workgroup's, there is no wait between workgroups.
//   jpeg_status_kernel   the image's status is that of its first failing unit, its rounds the most any unit took.
//   jpeg_idct_kernel     eight lanes per block: a column each, the column results through LDS, a row each; 8-bit component planes.
//   jpeg_output_kernel   a lane per output pixel: upsampling, colour conversion, PIL's convert; zeros for an image whose status is not OK.
// Integer arithmetic only, no memset node, no atomic read-modify-write on global memory except the one flag of jpeg_idct_kernel.
#include "hr_jpeg_decode.h"

namespace {

__device__ __forceinline__ bool image_file(const HrJpegDecodeArgs& a, int img, const uint8_t** f, int64_t* lo, int32_t* n)
{
    const int64_t b = a.offsets[img], e = a.offsets[img + 1];
    if (b < 0 || e < b || e > a.max_file_bytes || e - b > 0x7FFFFFF0ll) return false;
    *f = a.files + b;
    *lo = b;
    *n = (int32_t)(e - b);
    return true;
}

__global__ __launch_bounds__(HR_JPEG_PARSE_LANES) void jpeg_parse_kernel(const HrJpegDecodeArgs a)
{
    __shared__ hr_jpeg_parse_mem mem;
    __shared__ int head_status;
    const int img = blockIdx.x, lane = threadIdx.x;
    hr_jpeg_desc* d = a.desc + img;
    const uint8_t* f = nullptr;
    int64_t lo = 0;
    int32_t n = 0;
    const bool there = image_file(a, img, &f, &lo, &n);
    if (lane == 0) {
        int st;
        if (!there) { hr_jpeg_desc_clear(d); st = HR_JPEG_E_OFFSETS; }
        else st = hr_jpeg_parse_head(f, n, &mem, d);
        if (st == HR_JPEG_OK && (d->w != a.w || d->h != a.h)) st = HR_JPEG_E_SIZE;
        head_status = st;
        __threadfence();
    }
    __syncthreads();
    int st = head_status;
    if (st == HR_JPEG_OK) st = hr_jpeg_scan_units(f, n, d, a.ustart + (size_t)img * (size_t)(a.max_units + 2), &mem, lane, HR_JPEG_PARSE_LANES);
    if (lane == 0) d->status = st;
}

__global__ __launch_bounds__(256) void jpeg_zero_kernel(const HrJpegDecodeArgs a)
{
    const int img = blockIdx.y;
    const hr_jpeg_desc* d = a.desc + img;
    if (d->status != HR_JPEG_OK) return;
    const int64_t n16 = (int64_t)d->n_mcu * d->dpm * 8;               // 16-byte pieces: 128 bytes a block
    uint4* p = (uint4*)(a.coef + (size_t)img * (size_t)a.max_blocks * 64);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ __launch_bounds__(HR_JPEG_ENTROPY_LANES) void jpeg_entropy_kernel(const HrJpegDecodeArgs a)
{
    __shared__ int32_t red[3 * HR_JPEG_ENTROPY_LANES + 4];
    const int img = blockIdx.y, lane = threadIdx.x;
    const hr_jpeg_desc* d = a.desc + img;
    if (d->status != HR_JPEG_OK) return;
    const uint8_t* f;
    int64_t lo;
    int32_t n;
    if (!image_file(a, img, &f, &lo, &n)) return;                     // the parse has said so already
    const int32_t* ustart = a.ustart + (size_t)img * (size_t)(a.max_units + 2);
    const int64_t total_slots = a.total_slots;
    const int32_t n_units = d->n_units, ri = d->ri, n_mcu = d->n_mcu, dpm = d->dpm;
    for (int32_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        hr_jpeg_unit c;
        const int32_t at = ustart[u];
        c.d = f + at;
        c.n = ustart[u + 1] - 2 - at;
        c.desc = d;
        c.sub_bytes = a.sub_bytes;
        c.n_sub = c.n > 0 ? (int32_t)(((int64_t)c.n + a.sub_bytes - 1) / a.sub_bytes) : 1;
        const int64_t base = hr_jpeg_slot_base(lo, at, a.sub_bytes, img, a.max_units, u);
        if (base < 0 || base + c.n_sub > total_slots) return;         // cannot be (the slots are laid out for any valid offsets); never write outside
        c.start = a.slots + 2 * base;
        c.end = a.slots + 2 * total_slots + 2 * base;
        c.ndu = a.slots + 4 * total_slots + base;
        const int32_t mcu0 = ri ? u * ri : 0, mcu1 = ri && mcu0 + ri < n_mcu ? mcu0 + ri : n_mcu;
        c.coef = a.coef + ((size_t)img * (size_t)a.max_blocks + (size_t)mcu0 * dpm) * 64;
        c.expect_du = (mcu1 - mcu0) * dpm;
        const size_t k = (size_t)img * (size_t)(a.max_units + 1) + (size_t)u;
        hr_jpeg_entropy_unit(c, red, lane, HR_JPEG_ENTROPY_LANES, a.ustat + k, a.urounds + k);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void jpeg_status_kernel(const HrJpegDecodeArgs a)
{
    __shared__ int first_bad, most;
    const int img = blockIdx.x, lane = threadIdx.x;
    hr_jpeg_desc* d = a.desc + img;
    if (d->status != HR_JPEG_OK) return;
    if (lane == 0) { first_bad = 0x7FFFFFFF; most = 0; }
    __syncthreads();
    const size_t k = (size_t)img * (size_t)(a.max_units + 1);
    const int32_t n_units = d->n_units;
    int mine = 0x7FFFFFFF, rounds = 0;
    for (int32_t u = lane; u < n_units; u += 256) {
        if (a.ustat[k + u] != HR_JPEG_OK && u < mine) mine = u;
        rounds = max(rounds, a.urounds[k + u]);
    }
    if (mine != 0x7FFFFFFF) atomicMin(&first_bad, mine);
    atomicMax(&most, rounds);
    __syncthreads();
    if (lane == 0) {
        d->rounds = most;
        if (first_bad != 0x7FFFFFFF) d->status = a.ustat[k + first_bad];
    }
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const HrJpegDecodeArgs a)
{
    __shared__ int32_t ws[32][64 + 8];                                // a block's rows nine words apart: a column's stores spread over the banks
    const int img = blockIdx.y, blk = threadIdx.x >> 3, x = threadIdx.x & 7;
    hr_jpeg_desc* d = a.desc + img;
    if (d->status != HR_JPEG_OK) return;
    const hr_jpeg_planes pl = hr_jpeg_plane_layout(d);
    const int32_t n_du = d->n_mcu * d->dpm;
    const int16_t* coef = a.coef + (size_t)img * (size_t)a.max_blocks * 64;
    uint8_t* planes = a.planes + (size_t)img * (size_t)a.max_blocks * 64;
    int wide = 0;
    for (int32_t g0 = blockIdx.x * 32; g0 < n_du; g0 += gridDim.x * 32) {
        const int32_t g = g0 + blk;
        const bool on = g < n_du;
        int comp = 0, stride = 0;
        int64_t at = 0;
        if (on) {
            hr_jpeg_block_place(d, pl, g, &comp, &at, &stride);
            int32_t col[8];
            wide |= hr_jpeg_idct_column(coef + (size_t)g * 64, d->qt[comp], x, col);
            HR_UNROLL
            for (int y = 0; y < 8; ++y) ws[blk][9 * y + x] = col[y];
        }
        __syncthreads();
        if (on) {
            int32_t row[8];
            HR_UNROLL
            for (int k = 0; k < 8; ++k) row[k] = ws[blk][9 * x + k];
            int32_t px[8];
            wide |= hr_jpeg_idct_row(row, px);
            uint2 v;
            v.x = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16) | ((uint32_t)px[3] << 24);
            v.y = (uint32_t)px[4] | ((uint32_t)px[5] << 8) | ((uint32_t)px[6] << 16) | ((uint32_t)px[7] << 24);
            *(uint2*)(planes + at + (int64_t)x * stride) = v;
        }
        __syncthreads();
    }
    if (wide) atomicOr(&d->idct_flag, 1);
}

__global__ __launch_bounds__(256) void jpeg_output_kernel(const HrJpegDecodeArgs a)
{
    const int img = blockIdx.y;
    const hr_jpeg_desc* d = a.desc + img;
    int st = d->status;
    if (st == HR_JPEG_OK && d->idct_flag) st = HR_JPEG_E_COEF;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.status[img] = st;
        if (a.rounds) a.rounds[img] = st == HR_JPEG_E_OFFSETS ? 0 : d->rounds;
    }
    const int32_t w = a.w, oc = a.out_channels;
    const int64_t n_px = (int64_t)w * a.h;
    uint8_t* __restrict__ out = a.out + (size_t)img * (size_t)n_px * (size_t)oc;
    const uint8_t* planes = a.planes + (size_t)img * (size_t)a.max_blocks * 64;
    const hr_jpeg_planes pl = hr_jpeg_plane_layout(d);
    const int nc = d->ncomp;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_px; i += (int64_t)gridDim.x * 256) {
        uint32_t px = 0;
        if (st == HR_JPEG_OK) px = hr_png_convert_pixel(hr_jpeg_pixel(d, pl, planes, (int32_t)(i % w), (int32_t)(i / w)), nc, oc);
        uint8_t* q = out + (size_t)i * oc;
        q[0] = (uint8_t)px;
        if (oc > 1) { q[1] = (uint8_t)(px >> 8); q[2] = (uint8_t)(px >> 16); }
        if (oc > 3) q[3] = (uint8_t)(px >> 24);
    }
}

}  // namespace

hipError_t hr_launch_jpeg_decode(const HrJpegDecodeArgs& a, hipStream_t stream)
{
    const unsigned n = (unsigned)a.n_images;
    const auto grid = [](int64_t want, int64_t cap) { return (unsigned)(want < 1 ? 1 : want > cap ? cap : want); };
    hipLaunchKernelGGL(jpeg_parse_kernel, dim3(n), dim3(HR_JPEG_PARSE_LANES), 0, stream, a);
    hipLaunchKernelGGL(jpeg_zero_kernel, dim3(grid((a.max_blocks * 8 + 255) / 256, 2048), n), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(grid(a.max_units, 128), n), dim3(HR_JPEG_ENTROPY_LANES), 0, stream, a);
    hipLaunchKernelGGL(jpeg_status_kernel, dim3(n), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(grid((a.max_blocks + 31) / 32, 4096), n), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(jpeg_output_kernel, dim3(grid(((int64_t)a.w * a.h + 255) / 256, 4096), n), dim3(256), 0, stream, a);
    return hipGetLastError();
}
