// A frame in device memory -> a PNG file in device memory (hr_png_encode; every rule of the format: hr_png.h, which the host encoder of
// the test-suite calls too, so both give the same bytes).  One workgroup per strip of rows in each of three kernels:
//   A  png_filter_kernel   a wavefront per row: the five filters' costs (to8b fused into the read of a float frame), the choice, the
//                          filtered bytes to the workspace.  Then the strip's bytes are cut into one contiguous slice per thread: a
//                          summary of each slice (first / last byte, leading / trailing run, Adler partial), a scan of the summaries
//                          that tells every slice how long the run reaching it is and how far the run leaving it goes, and the tokens,
//                          each from hr_png_token.  The literal / length histogram is built in LDS by integer atomics.
//   B  png_codes_kernel    a wavefront per strip ranks the used symbols (hr_png_rank), lane 0 runs hr_png_strip_codes: code lengths,
//                          the code-length code, the block header's bits, the exact block size, stored or dynamic.
//      png_scan_kernel     one workgroup: exclusive scan of the chunk sizes in chunks of 256 with a carry, the Adler-32, the file length.
//   C  png_pack_kernel     token bit lengths per slice, a scan for the slices' bit offsets, the codes OR-ed into LDS words (integer
//                          atomics), flushed to the file with the slice CRCs merged by multiplication with x^(8 n); then the chunk's
//                          length, type, CRC and marker; strip 0 adds the signature and IHDR, the last strip the Adler-32 and IEND.
// Integer arithmetic and integer LDS atomics only: the file is the same on every run.  No global atomics, no memset: every word of the
// workspace that is read has been written by the same call.
#include "hr_png.h"
#include "hr_scan.h"

namespace {

constexpr int THREADS = 1024;                                 // kernels A and C: a strip's slices are walked serially, so the more the shorter
constexpr int SCAN_THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr uint32_t OUT_BYTES = HR_PNG_STRIP_BYTES + 1024;      // the chunk window in LDS: a whole ordinary strip's chunk data
constexpr uint32_t WIDE_SLICE = 8;                            // tokens per thread and window of a strip wider than the budget (21 bits at most each)

__device__ __forceinline__ uint32_t* strip_meta(const HrPngArgs& a, int s)
{
    return (uint32_t*)(a.workspace + a.plan.off_meta) + (size_t)s * HR_PNG_META_WORDS;
}

__global__ __launch_bounds__(THREADS) void png_filter_kernel(const HrPngArgs a)
{
    __shared__ uint32_t hist[HR_PNG_HIST_WORDS];
    __shared__ uint32_t seg_lead[THREADS], seg_run[THREADS];
    __shared__ uint8_t seg_first[THREADS], seg_last[THREADS], seg_any[THREADS];
    __shared__ uint32_t adler[2];
    const hr_png_plan_t& pl = a.plan;
    const int s = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int32_t rows = hr_png_strip_rows(pl, s), y0 = s * pl.rows_per_strip, row_len = pl.w * pl.channels;
    uint8_t* __restrict__ filt = a.workspace + pl.off_filtered + (size_t)s * pl.strip_stride;
    uint16_t* __restrict__ tok = (uint16_t*)(a.workspace + pl.off_tokens) + (size_t)s * pl.strip_stride;
    for (int i = t; i < HR_PNG_HIST_WORDS; i += THREADS) hist[i] = i == HR_PNG_EOB ? 1u : 0u;
    if (t < 2) adler[t] = 0;

    // ---- filters: a wavefront per row
    for (int32_t r = wave; r < rows; r += WAVES) {
        const int32_t y = y0 + r;
        int f = a.filter_mode;
        if (f == HR_PNG_FILTER_ADAPTIVE) {
            uint32_t sums[5] = {0, 0, 0, 0, 0};
            for (int32_t x = lane; x < row_len; x += 64) hr_png_filter_costs(a.pixels, a.pixel_type, y, x, row_len, pl.channels, sums);
            HR_UNROLL
            for (int k = 0; k < 5; ++k) sums[k] = hr_wave_sum(sums[k]);
            f = hr_png_choose_filter(sums);
        }
        uint8_t* o = filt + (size_t)r * pl.row_bytes;
        if (lane == 0) o[0] = (uint8_t)f;
        for (int32_t x = lane; x < row_len; x += 64) o[1 + x] = (uint8_t)hr_png_filtered(a.pixels, a.pixel_type, y, x, row_len, pl.channels, f);
    }
    __threadfence_block();
    __syncthreads();

    // ---- slices: thread t owns bytes [beg, end) of the strip
    const uint32_t n = (uint32_t)rows * (uint32_t)pl.row_bytes;
    const uint32_t per = (n + THREADS - 1) / THREADS;
    const uint32_t beg = min(n, (uint32_t)t * per), end = min(n, beg + per);
    const hr_png_segment seg = hr_png_segment_scan(filt + beg, end - beg);
    seg_first[t] = (uint8_t)seg.first;
    seg_last[t] = (uint8_t)seg.last;
    seg_lead[t] = seg.lead;
    seg_any[t] = seg.len ? 1 : 0;
    // the run ending at each slice's last byte, across slices: scan of (length << 1 | the run covers everything scanned so far)
    seg_run[t] = (seg.trail << 1) | (seg.len && seg.trail == seg.len ? 1u : 0u);
    __syncthreads();
    for (int off = 1; off < THREADS; off <<= 1) {
        uint32_t mine = seg_run[t];
        // the block [t - off + 1, t] meets the block before it between slices t - off and t - off + 1
        if (t >= off) mine = hr_png_run_join(mine, seg_run[t - off], seg_first[t - off + 1] == seg_last[t - off]);
        __syncthreads();
        seg_run[t] = mine;
        __syncthreads();
    }
    if (seg.len) {
        const uint32_t before = (t > 0 && seg_last[t - 1] == seg.first) ? seg_run[t - 1] >> 1 : 0u;
        // bytes equal to the slice's last one after it: exact, or at least 258
        uint32_t after = 0;
        for (int j = t + 1; j < THREADS && after < 258u && seg_any[j] && seg_first[j] == seg.last; ++j) {
            after += seg_lead[j];
            if (seg_lead[j] != min(n, (uint32_t)(j + 1) * per) - min(n, (uint32_t)j * per)) break;
        }
        hr_png_segment_tokens(filt + beg, end - beg, before, after, [&](uint32_t i, uint32_t token) {
            tok[beg + i] = (uint16_t)token;
            if (token != HR_PNG_TOK_COVERED) {
                atomicAdd(&hist[hr_png_token_symbol(token)], 1u);
                if (token >= HR_PNG_TOK_MATCH) atomicAdd(&hist[HR_PNG_LL], 1u);
            }
        });
        uint32_t pa, pb;
        hr_adler_place(seg.a, seg.b, (uint64_t)pl.total_bytes - ((uint64_t)y0 * (uint64_t)pl.row_bytes + end), &pa, &pb);
        atomicAdd(&adler[0], pa);
        atomicAdd(&adler[1], pb);
    }
    __syncthreads();
    uint32_t* __restrict__ hist_out = (uint32_t*)(a.workspace + pl.off_hist) + (size_t)s * HR_PNG_HIST_WORDS;
    for (int i = t; i < HR_PNG_HIST_WORDS; i += THREADS) hist_out[i] = hist[i];
    if (t == 0) {
        uint32_t* m = strip_meta(a, s);
        m[HR_PNG_M_ADLER_A] = adler[0] % HR_PNG_ADLER_MOD;      // THREADS terms below 65521 each
        m[HR_PNG_M_ADLER_B] = adler[1] % HR_PNG_ADLER_MOD;
    }
}

__global__ __launch_bounds__(64) void png_codes_kernel(const HrPngArgs a)
{
    __shared__ hr_png_huff_work wk;
    __shared__ uint32_t hist[HR_PNG_HIST_WORDS];
    __shared__ uint32_t used[64];
    const hr_png_plan_t& pl = a.plan;
    const int s = blockIdx.x, lane = threadIdx.x;
    const uint32_t* __restrict__ hist_in = (const uint32_t*)(a.workspace + pl.off_hist) + (size_t)s * HR_PNG_HIST_WORDS;
    for (int i = lane; i < HR_PNG_HIST_WORDS; i += 64) hist[i] = hist_in[i];
    __syncthreads();
    uint32_t m = 0;
    for (int i = lane; i < HR_PNG_LL; i += 64)
        if (hist[i]) { wk.sorted[hr_png_rank(hist, HR_PNG_LL, i)] = (uint16_t)i; ++m; }
    used[lane] = m;
    __syncthreads();
    if (lane == 0) {
        m = 0;
        for (int i = 0; i < 64; ++i) m += used[i];
        const uint32_t n = (uint32_t)hr_png_strip_rows(pl, s) * (uint32_t)pl.row_bytes;
        hr_png_strip_codes(hist, (int)m, n, s == 0, s == pl.n_strips - 1, &wk, (uint32_t*)(a.workspace + pl.off_codes) + (size_t)s * HR_PNG_HIST_WORDS,
                           a.workspace + pl.off_hdr + (size_t)s * HR_PNG_HDR_BYTES, strip_meta(a, s));
    }
}

// one workgroup: every strip's chunk offset in the file (exclusive scan in chunks of 256 with a carry), the Adler-32, the file's length
__global__ __launch_bounds__(SCAN_THREADS) void png_scan_kernel(const HrPngArgs a)
{
    __shared__ uint32_t sc[SCAN_THREADS];
    __shared__ uint32_t ad[2];
    const int t = threadIdx.x;
    const int n_strips = a.plan.n_strips;
    uint32_t carry = HR_PNG_FILE_HEAD, aa = 0, ab = 0;
    for (int base = 0; base < n_strips; base += SCAN_THREADS) {
        const int i = base + t;
        uint32_t* m = strip_meta(a, i < n_strips ? i : 0);
        const uint32_t c = i < n_strips ? 12u + m[HR_PNG_M_DATA_LEN] : 0u;
        if (t < 2) ad[t] = 0;
        const uint32_t incl = hr_block_scan_inclusive<SCAN_THREADS>(c, sc);
        if (i < n_strips) {
            m[HR_PNG_M_OFFSET] = carry + incl - c;
            atomicAdd(&ad[0], m[HR_PNG_M_ADLER_A]);
            atomicAdd(&ad[1], m[HR_PNG_M_ADLER_B]);
        }
        carry += sc[SCAN_THREADS - 1];
        __syncthreads();
        aa = (aa + ad[0]) % HR_PNG_ADLER_MOD;
        ab = (ab + ad[1]) % HR_PNG_ADLER_MOD;
        __syncthreads();
    }
    if (t == 0) {
        uint32_t* g = strip_meta(a, n_strips);
        g[HR_PNG_G_ADLER] = hr_adler_final(aa, ab, (uint64_t)a.plan.total_bytes);
        *a.file_bytes = (int64_t)carry + HR_PNG_IEND;
    }
}

__global__ __launch_bounds__(THREADS) void png_pack_kernel(const HrPngArgs a)
{
    __shared__ uint32_t out[OUT_BYTES / 4];
    __shared__ uint32_t codes[HR_PNG_HIST_WORDS];
    __shared__ uint32_t crc_table[256];
    __shared__ uint32_t sc[THREADS];
    __shared__ uint32_t crc_acc;
    const hr_png_plan_t& pl = a.plan;
    const int s = blockIdx.x, t = threadIdx.x;
    const bool first = s == 0, last = s == pl.n_strips - 1;
    const uint32_t* __restrict__ meta = strip_meta(a, s);
    const uint8_t* __restrict__ filt = a.workspace + pl.off_filtered + (size_t)s * pl.strip_stride;
    const uint16_t* __restrict__ tok = (const uint16_t*)(a.workspace + pl.off_tokens) + (size_t)s * pl.strip_stride;
    const uint32_t n = (uint32_t)hr_png_strip_rows(pl, s) * (uint32_t)pl.row_bytes;
    const uint32_t data_len = meta[HR_PNG_M_DATA_LEN], stream_len = 4u + data_len;      // the CRC's bytes: the type, then the data
    const bool dynamic = meta[HR_PNG_M_DYNAMIC] != 0;
    uint8_t* __restrict__ chunk = a.file + meta[HR_PNG_M_OFFSET];
    uint8_t* __restrict__ dst = chunk + 4;
    uint8_t* out8 = (uint8_t*)out;
    const uint32_t trailer = last ? strip_meta(a, pl.n_strips)[HR_PNG_G_ADLER] : 0x0000FFFFu;      // big-endian bytes after the body
    const uint32_t prefix = first ? 6u : 4u;

    if (t < 256) crc_table[t] = hr_crc_table_entry((uint32_t)t);
    if (t == 0) crc_acc = 0;
    for (uint32_t i = t; i < OUT_BYTES / 4; i += THREADS) out[i] = 0;
    if (dynamic)
        for (int i = t; i < HR_PNG_HIST_WORDS; i += THREADS) codes[i] = ((const uint32_t*)(a.workspace + pl.off_codes) + (size_t)s * HR_PNG_HIST_WORDS)[i];
    __syncthreads();

    // the window out8[0..cnt) holds the stream's bytes [pos, pos + cnt): CRC slices merged, bytes to the file
    auto flush = [&](uint32_t pos, uint32_t cnt) {
        if (pos + cnt > stream_len) cnt = stream_len > pos ? stream_len - pos : 0u;      // (never: the sizes come from the same arithmetic)
        const uint32_t per = (((cnt + THREADS - 1) / THREADS) + 3u) & ~3u;
        const uint32_t b0 = min(cnt, (uint32_t)t * per), b1 = min(cnt, b0 + per);
        uint32_t c = 0;
        for (uint32_t i = b0; i < b1; ++i) c = crc_table[(c ^ out8[i]) & 255u] ^ (c >> 8);
        if (b1 > b0) atomicXor(&crc_acc, hr_crc_shift(c, stream_len - (pos + b1)));
        for (uint32_t i = t; i < cnt; i += THREADS) dst[pos + i] = out8[i];
    };
    auto or_bits = [&](uint32_t bit, uint32_t value, uint32_t count) {      // count <= 21: two words at most
        if (!count) return;
        const uint32_t w = bit >> 5, sh = bit & 31u;
        atomicOr(&out[w], value << sh);
        if (sh + count > 32u) atomicOr(&out[w + 1], value >> (32u - sh));
    };

    if (!dynamic) {
        // every byte of the stream is a function of its position
        const uint32_t stored = (uint32_t)hr_png_stored_bytes(n);
        for (uint32_t pos = 0; pos < stream_len; pos += OUT_BYTES) {
            const uint32_t cnt = min(OUT_BYTES, stream_len - pos);
            for (uint32_t i = t; i < cnt; i += THREADS) {
                const uint32_t q = pos + i;
                int v;
                if (q < 4) v = "IDAT"[q];
                else if (q < prefix) v = q == 4 ? 0x78 : 0x01;
                else if (q < prefix + stored) v = hr_png_stored_byte(filt, n, q - prefix, last);
                else if (q >= stream_len - 4) v = (int)((trailer >> (8u * (stream_len - 1u - q))) & 255u);
                else v = 0;                                   // the marker's header bits and padding
                out8[i] = (uint8_t)v;
            }
            __syncthreads();
            flush(pos, cnt);
            __syncthreads();
        }
    } else {
        if (t < 4) out8[t] = (uint8_t)"IDAT"[t];
        if (first && t == 4) out8[4] = 0x78;
        if (first && t == 5) out8[5] = 0x01;
        const uint32_t hdr_bits = meta[HR_PNG_M_HDR_BITS];
        const uint8_t* __restrict__ hdr = a.workspace + pl.off_hdr + (size_t)s * HR_PNG_HDR_BYTES;
        for (uint32_t i = t; i < (hdr_bits + 7u) / 8u; i += THREADS) out8[prefix + i] = hdr[i];      // (its last byte's spare bits are zero)
        __syncthreads();
        uint32_t flushed = 0;                                 // stream bytes before out8[0]
        uint32_t bit = prefix * 8u + hdr_bits;                // stream bit of the next token
        const uint32_t per = n <= HR_PNG_STRIP_BYTES ? (n + THREADS - 1) / THREADS : WIDE_SLICE;
        for (uint32_t base = 0; base < n; base += per * THREADS) {
            const uint32_t beg = min(n, base + (uint32_t)t * per), end = min(n, beg + per);
            uint32_t bits = 0;
            for (uint32_t i = beg; i < end; ++i) {
                uint32_t value, count;
                hr_png_token_bits(codes, tok[i], &value, &count);
                bits += count;
            }
            const uint32_t incl = hr_block_scan_inclusive<THREADS>(bits, sc);
            uint32_t at = bit - flushed * 8u + (incl - bits);
            for (uint32_t i = beg; i < end; ++i) {
                uint32_t value, count;
                hr_png_token_bits(codes, tok[i], &value, &count);
                or_bits(at, value, count);
                at += count;
            }
            bit += sc[THREADS - 1];
            __syncthreads();
            if (base + per * THREADS < n) {
                // more windows follow: whole words go out, the word holding the next bit comes along
                const uint32_t words = (bit / 8u - flushed) / 4u;
                const uint32_t keep = out[words];
                __syncthreads();
                flush(flushed, words * 4u);
                __syncthreads();
                for (uint32_t i = t; i <= words; i += THREADS) out[i] = 0;
                __syncthreads();
                if (t == 0) out[0] = keep;
                flushed += words * 4u;
                __syncthreads();
            }
        }
        if (t == 0) {
            or_bits(bit - flushed * 8u, codes[HR_PNG_EOB] & 0xFFFFu, codes[HR_PNG_EOB] >> 16);
            const uint32_t end_bit = bit + (codes[HR_PNG_EOB] >> 16) + (last ? 0u : 3u);
            const uint32_t body_end = (end_bit + 7u) / 8u - flushed;      // padding and the marker's header bits are the zeros already there
            for (int k = 0; k < 4; ++k) out8[body_end + k] = (uint8_t)(trailer >> (8 * (3 - k)));
        }
        __syncthreads();
        flush(flushed, stream_len - flushed);
        __syncthreads();
    }

    if (t == 0) {
        hr_png_be32(chunk, data_len);
        hr_png_be32(dst + stream_len, hr_crc_final(crc_acc, stream_len));
        if (first) hr_png_file_head(a.file, pl.w, pl.h, pl.channels);
        if (last) hr_png_file_tail(dst + stream_len + 4);
    }
}

}  // namespace

hipError_t hr_launch_png_encode(const HrPngArgs& a, hipStream_t stream)
{
    const unsigned strips = (unsigned)a.plan.n_strips;
    hipLaunchKernelGGL(png_filter_kernel, dim3(strips), dim3(THREADS), 0, stream, a);
    hipLaunchKernelGGL(png_codes_kernel, dim3(strips), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(png_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, a);
    hipLaunchKernelGGL(png_pack_kernel, dim3(strips), dim3(THREADS), 0, stream, a);
    return hipGetLastError();
}
