// A frame in device memory -> a baseline JPEG file in device memory (hr_jpeg_encode; every rule of the format: hr_jpeg_encode.h, which the
// host encoder calls too, so both give the same bytes).  Eight kernels, each pass separated from the next by the kernel boundary:
//   1  jpeg_enc_blocks_kernel   eight lanes a block: colour conversion, edge replication and downsampling as the samples are read (to8b of a
//                               float frame fused in), the FDCT's row pass in registers, the column pass through LDS, quantisation; int16
//                               coefficients in zigzag order at the block's place in the scan.  Dummy blocks write nothing.
//   2  jpeg_enc_count_kernel    a lane a block: the DC difference (the predecessor is index arithmetic) and the block's bit count; an
//                               exclusive scan over the workgroup's 256 blocks and the workgroup's total
//   3  jpeg_enc_scan_kernel     one workgroup: exclusive scan of the workgroups' totals, then per restart interval its first bit and its
//                               bytes (padded), scanned into the intervals' byte offsets in the unstuffed scan
//   4  jpeg_enc_clear_kernel    zeroes the words of the unstuffed scan that will be written (a kernel, not a memset node)
//   5  jpeg_enc_write_kernel    a lane a block: its codes OR-ed into the unstuffed scan (integer atomics on 32-bit words), the
//                               interval's last block adds the padding ones
//   6  jpeg_enc_ffcount_kernel  FF bytes per chunk of 1024 unstuffed bytes
//   7  jpeg_enc_ffscan_kernel   one workgroup: exclusive scan of the chunks' counts; the header, EOI and the length word
//   8  jpeg_enc_scatter_kernel  every byte to its place: header + index + FF bytes before it + 2 per restart marker before it, a 00 after
//                               an FF, the marker after an interval's last byte
// Integer arithmetic and integer atomic OR only: the file is the same on every run.  Every word that is read has been written by the same call.
#include "hr_jpeg_encode.h"
#include "hr_scan.h"

namespace {

constexpr int THREADS = HR_JPEG_ENC_WG_BLOCKS;      // kernels 1, 2, 5, 6, 8
constexpr int SCAN_THREADS = 1024;                  // kernels 3, 7
constexpr int ROW = 9;                              // ints between two rows of a block in LDS: columns read without bank conflicts

static_assert(HR_JPEG_ENC_CHUNK == 4 * THREADS, "a lane of the stuffing passes owns one word of its chunk");

__device__ __forceinline__ const hr_jpeg_enc_tables* tables_of(const HrJpegEncArgs& a) { return (const hr_jpeg_enc_tables*)(a.workspace + a.plan.off_tables); }
__device__ __forceinline__ int16_t* coef_of(const HrJpegEncArgs& a) { return (int16_t*)(a.workspace + a.plan.off_coef); }
__device__ __forceinline__ uint32_t* words_at(const HrJpegEncArgs& a, int64_t off) { return (uint32_t*)(a.workspace + off); }

__global__ __launch_bounds__(THREADS) void jpeg_enc_blocks_kernel(const HrJpegEncArgs a)
{
    __shared__ int32_t ws[THREADS / 8][8 * ROW];
    const hr_jpeg_enc_plan_t& p = a.plan;
    const int t = threadIdx.x, g = t >> 3, r = t & 7;
    const int32_t b = (int32_t)blockIdx.x * (THREADS / 8) + g;
    const bool in = b < p.n_blocks;
    const hr_jpeg_enc_block k = hr_jpeg_enc_block_at(p, in ? b : 0);
    const bool work = in && !k.dummy;
    int32_t d[8];
    if (work) {
        HR_UNROLL
        for (int c = 0; c < 8; ++c) d[c] = hr_jpeg_enc_sample(a.pixels, a.pixel_type, p, k.comp, k.bx * 8 + c, k.by * 8 + r) - 128;
        hr_jpeg_fdct_pass(d, 0);
        HR_UNROLL
        for (int c = 0; c < 8; ++c) ws[g][r * ROW + c] = d[c];
    }
    __syncthreads();
    if (work) {
        HR_UNROLL
        for (int y = 0; y < 8; ++y) d[y] = ws[g][y * ROW + r];
        hr_jpeg_fdct_pass(d, 1);
    }
    __syncthreads();
    if (work) {
        HR_UNROLL
        for (int y = 0; y < 8; ++y) ws[g][y * ROW + r] = d[y];
    }
    __syncthreads();
    if (work) {
        const uint16_t* __restrict__ div = tables_of(a)->div[k.comp ? 1 : 0] + r * 8;
        uint32_t o[4];
        HR_UNROLL
        for (int i = 0; i < 4; ++i) {
            const int n0 = hr_jpeg_natural(r * 8 + 2 * i), n1 = hr_jpeg_natural(r * 8 + 2 * i + 1);
            const int32_t v0 = hr_jpeg_enc_quant(ws[g][(n0 >> 3) * ROW + (n0 & 7)], div[2 * i]);
            const int32_t v1 = hr_jpeg_enc_quant(ws[g][(n1 >> 3) * ROW + (n1 & 7)], div[2 * i + 1]);
            o[i] = ((uint32_t)v0 & 0xFFFFu) | ((uint32_t)v1 << 16);
        }
        *(uint4*)(coef_of(a) + (int64_t)b * 64 + r * 8) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// the two Huffman tables into LDS: dc[2][16] then ac[2][256]
__device__ __forceinline__ void load_codes(const HrJpegEncArgs& a, uint32_t* codes)
{
    const hr_jpeg_enc_tables* tb = tables_of(a);
    for (int i = threadIdx.x; i < 32 + 512; i += THREADS) codes[i] = i < 32 ? tb->dc[i >> 4][i & 15] : tb->ac[(i - 32) >> 8][(i - 32) & 255];
    __syncthreads();
}

__global__ __launch_bounds__(THREADS) void jpeg_enc_count_kernel(const HrJpegEncArgs a)
{
    __shared__ uint32_t codes[32 + 512];
    __shared__ uint32_t sc[THREADS];
    const hr_jpeg_enc_plan_t& p = a.plan;
    const int t = threadIdx.x;
    const int32_t b = (int32_t)blockIdx.x * THREADS + t;
    load_codes(a, codes);
    uint32_t bits = 0;
    if (b < p.n_blocks) {
        const hr_jpeg_enc_block k = hr_jpeg_enc_block_at(p, b);
        const int ti = k.comp ? 1 : 0;
        const int16_t* coef = coef_of(a);
        hr_jpeg_enc_block_code(codes + 16 * ti, codes + 32 + 256 * ti, coef + (int64_t)b * 64, hr_jpeg_enc_dc_diff(p, coef, b, k), k.dummy != 0,
                               [&](uint32_t, int len, int, bool) { bits += (uint32_t)len; });
    }
    const uint32_t incl = hr_block_scan_inclusive<THREADS>(bits, sc);
    if (b < p.n_blocks) words_at(a, p.off_local)[b] = incl - bits;
    if (t == THREADS - 1) words_at(a, p.off_wg)[blockIdx.x] = incl;
}

__global__ __launch_bounds__(SCAN_THREADS) void jpeg_enc_scan_kernel(const HrJpegEncArgs a)
{
    __shared__ uint32_t sc[SCAN_THREADS];
    const hr_jpeg_enc_plan_t& p = a.plan;
    const int t = threadIdx.x;
    uint32_t* wg = words_at(a, p.off_wg);
    const uint32_t* local = words_at(a, p.off_local);
    uint32_t carry = 0;
    for (int32_t base = 0; base < p.n_wg; base += SCAN_THREADS) {
        const int32_t i = base + t;
        const uint32_t v = i < p.n_wg ? wg[i] : 0u;
        const uint32_t incl = hr_block_scan_inclusive<SCAN_THREADS>(v, sc);
        if (i < p.n_wg) wg[i] = carry + incl - v;
        carry += sc[SCAN_THREADS - 1];
        __syncthreads();
    }
    const uint32_t total_bits = carry;
    __threadfence();
    __syncthreads();
    // bit offset of block b in the scan without padding; the prefixes were stored by other lanes of this workgroup
    auto start = [&](int64_t b) { return b < p.n_blocks ? HR_JPEG_LD(wg + (b / HR_JPEG_ENC_WG_BLOCKS)) + local[b] : total_bits; };
    uint32_t* ibyte = words_at(a, p.off_int_byte);
    uint32_t* ibit = words_at(a, p.off_int_bit);
    carry = 0;
    for (int32_t base = 0; base < p.n_int; base += SCAN_THREADS) {
        const int32_t i = base + t;
        uint32_t bytes = 0;
        if (i < p.n_int) {
            const int64_t m1 = (int64_t)(i + 1) * p.ri;
            const uint32_t s0 = start((int64_t)i * p.ri * p.bpm), s1 = start((m1 < p.n_mcu ? m1 : (int64_t)p.n_mcu) * p.bpm);
            bytes = (s1 - s0 + 7u) >> 3;
            ibit[i] = s0;
        }
        const uint32_t incl = hr_block_scan_inclusive<SCAN_THREADS>(bytes, sc);
        if (i < p.n_int) ibyte[i] = carry + incl - bytes;
        carry += sc[SCAN_THREADS - 1];
        __syncthreads();
    }
    if (t == 0) {
        ibyte[p.n_int] = carry;
        words_at(a, p.off_glob)[HR_JPEG_ENC_G_RAW_BYTES] = carry;
    }
}

__global__ __launch_bounds__(THREADS) void jpeg_enc_clear_kernel(const HrJpegEncArgs a)
{
    const hr_jpeg_enc_plan_t& p = a.plan;
    const uint32_t raw_bytes = words_at(a, p.off_glob)[HR_JPEG_ENC_G_RAW_BYTES];
    const int64_t i = ((int64_t)blockIdx.x * THREADS + threadIdx.x) * 16;      // the buffer holds whole chunks and 64 bytes more
    if (i < (int64_t)raw_bytes + 8) *(uint4*)(a.workspace + p.off_raw + i) = make_uint4(0u, 0u, 0u, 0u);
}

__global__ __launch_bounds__(THREADS) void jpeg_enc_write_kernel(const HrJpegEncArgs a)
{
    __shared__ uint32_t codes[32 + 512];
    const hr_jpeg_enc_plan_t& p = a.plan;
    const int32_t b = (int32_t)blockIdx.x * THREADS + (int32_t)threadIdx.x;
    load_codes(a, codes);
    if (b >= p.n_blocks) return;
    const hr_jpeg_enc_block k = hr_jpeg_enc_block_at(p, b);
    const int ti = k.comp ? 1 : 0;
    const int32_t i = k.mcu / p.ri;
    const uint32_t mine = words_at(a, p.off_wg)[b / HR_JPEG_ENC_WG_BLOCKS] + words_at(a, p.off_local)[b];
    const uint32_t at = words_at(a, p.off_int_byte)[i] * 8u + (mine - words_at(a, p.off_int_bit)[i]);
    const int16_t* coef = coef_of(a);
    hr_jpeg_enc_bitw bw;
    hr_jpeg_enc_bitw_init(&bw, words_at(a, p.off_raw), at);
    uint32_t bits = 0;
    hr_jpeg_enc_block_code(codes + 16 * ti, codes + 32 + 256 * ti, coef + (int64_t)b * 64, hr_jpeg_enc_dc_diff(p, coef, b, k), k.dummy != 0,
                           [&](uint32_t v, int len, int, bool) { hr_jpeg_enc_bitw_put(&bw, v, len); bits += (uint32_t)len; });
    const bool last = k.j == p.bpm - 1 && (k.mcu == p.n_mcu - 1 || (k.mcu + 1) % p.ri == 0);
    const int pad = (int)((8u - ((at + bits) & 7u)) & 7u);
    if (last && pad) hr_jpeg_enc_bitw_put(&bw, (1u << pad) - 1u, pad);
    hr_jpeg_enc_bitw_flush(&bw);
}

// the FF bytes among the valid bytes of word `word` of the unstuffed scan
__device__ __forceinline__ uint32_t ff_in_word(uint32_t v, int64_t first_byte, uint32_t raw_bytes)
{
    uint32_t n = 0;
    HR_UNROLL
    for (int j = 0; j < 4; ++j) n += (first_byte + j < (int64_t)raw_bytes && ((v >> (8 * j)) & 255u) == 255u) ? 1u : 0u;
    return n;
}

__global__ __launch_bounds__(THREADS) void jpeg_enc_ffcount_kernel(const HrJpegEncArgs a)
{
    __shared__ uint32_t sc[THREADS];
    const hr_jpeg_enc_plan_t& p = a.plan;
    const uint32_t raw_bytes = words_at(a, p.off_glob)[HR_JPEG_ENC_G_RAW_BYTES];
    const int64_t first = ((int64_t)blockIdx.x * THREADS + threadIdx.x) * 4;
    if ((int64_t)blockIdx.x * HR_JPEG_ENC_CHUNK >= (int64_t)raw_bytes) return;      // (the whole workgroup)
    const uint32_t v = first < (int64_t)raw_bytes ? words_at(a, p.off_raw)[first >> 2] : 0u;
    const uint32_t incl = hr_block_scan_inclusive<THREADS>(ff_in_word(v, first, raw_bytes), sc);
    if (threadIdx.x == THREADS - 1) words_at(a, p.off_ff)[blockIdx.x] = incl;
}

__global__ __launch_bounds__(SCAN_THREADS) void jpeg_enc_ffscan_kernel(const HrJpegEncArgs a)
{
    __shared__ uint32_t sc[SCAN_THREADS];
    const hr_jpeg_enc_plan_t& p = a.plan;
    const int t = threadIdx.x;
    const uint32_t raw_bytes = words_at(a, p.off_glob)[HR_JPEG_ENC_G_RAW_BYTES];
    const int64_t chunks = ((int64_t)raw_bytes + HR_JPEG_ENC_CHUNK - 1) / HR_JPEG_ENC_CHUNK;
    uint32_t* ff = words_at(a, p.off_ff);
    uint32_t carry = 0;
    for (int64_t base = 0; base < chunks; base += SCAN_THREADS) {
        const int64_t i = base + t;
        const uint32_t v = i < chunks ? ff[i] : 0u;
        const uint32_t incl = hr_block_scan_inclusive<SCAN_THREADS>(v, sc);
        if (i < chunks) ff[i] = carry + incl - v;
        carry += sc[SCAN_THREADS - 1];
        __syncthreads();
    }
    const hr_jpeg_enc_tables* tb = tables_of(a);
    for (int i = t; i < p.head_bytes; i += SCAN_THREADS) a.file[i] = tb->head[i];
    if (t == 0) {
        const int64_t eoi = (int64_t)p.head_bytes + raw_bytes + carry + 2 * (int64_t)(p.n_int - 1);
        a.file[eoi] = 0xFF;
        a.file[eoi + 1] = 0xD9;
        *a.file_bytes = eoi + 2;
    }
}

__global__ __launch_bounds__(THREADS) void jpeg_enc_scatter_kernel(const HrJpegEncArgs a)
{
    __shared__ uint32_t sc[THREADS];
    const hr_jpeg_enc_plan_t& p = a.plan;
    const uint32_t raw_bytes = words_at(a, p.off_glob)[HR_JPEG_ENC_G_RAW_BYTES];
    const int64_t first = ((int64_t)blockIdx.x * THREADS + threadIdx.x) * 4;
    if ((int64_t)blockIdx.x * HR_JPEG_ENC_CHUNK >= (int64_t)raw_bytes) return;      // (the whole workgroup)
    const uint32_t v = first < (int64_t)raw_bytes ? words_at(a, p.off_raw)[first >> 2] : 0u;
    const uint32_t mine = ff_in_word(v, first, raw_bytes);
    uint32_t ff = words_at(a, p.off_ff)[blockIdx.x] + hr_block_scan_inclusive<THREADS>(mine, sc) - mine;
    if (first >= (int64_t)raw_bytes) return;
    // the restart interval of the lane's first byte: the last one that starts at or before it
    const uint32_t* ibyte = words_at(a, p.off_int_byte);
    int32_t lo = 0, hi = p.n_int - 1;
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if ((int64_t)ibyte[mid] <= first) lo = mid; else hi = mid - 1;
    }
    int32_t k = lo;
    for (int j = 0; j < 4; ++j) {
        const int64_t i = first + j;
        if (i >= (int64_t)raw_bytes) break;
        while (k < p.n_int - 1 && (int64_t)ibyte[k + 1] <= i) ++k;
        const uint32_t byte = (v >> (8 * j)) & 255u;
        int64_t o = (int64_t)p.head_bytes + i + ff + 2 * (int64_t)k;
        a.file[o++] = (uint8_t)byte;
        if (byte == 255u) { a.file[o++] = 0; ++ff; }
        if (k < p.n_int - 1 && i + 1 == (int64_t)ibyte[k + 1]) {
            a.file[o] = 0xFF;
            a.file[o + 1] = (uint8_t)(0xD0 + (k & 7));
        }
    }
}

}  // namespace

hipError_t hr_launch_jpeg_encode(const HrJpegEncArgs& a, hipStream_t stream)
{
    const hr_jpeg_enc_plan_t& p = a.plan;
    const unsigned per_block = (unsigned)p.n_wg;
    hipLaunchKernelGGL(jpeg_enc_blocks_kernel, dim3((unsigned)((p.n_blocks + THREADS / 8 - 1) / (THREADS / 8))), dim3(THREADS), 0, stream, a);
    hipLaunchKernelGGL(jpeg_enc_count_kernel, dim3(per_block), dim3(THREADS), 0, stream, a);
    hipLaunchKernelGGL(jpeg_enc_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, a);
    hipLaunchKernelGGL(jpeg_enc_clear_kernel, dim3((unsigned)((p.n_chunks * HR_JPEG_ENC_CHUNK + 64) / (16 * THREADS) + 1)), dim3(THREADS), 0, stream, a);
    hipLaunchKernelGGL(jpeg_enc_write_kernel, dim3(per_block), dim3(THREADS), 0, stream, a);
    hipLaunchKernelGGL(jpeg_enc_ffcount_kernel, dim3((unsigned)p.n_chunks), dim3(THREADS), 0, stream, a);
    hipLaunchKernelGGL(jpeg_enc_ffscan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, a);
    hipLaunchKernelGGL(jpeg_enc_scatter_kernel, dim3((unsigned)p.n_chunks), dim3(THREADS), 0, stream, a);
    return hipGetLastError();
}
