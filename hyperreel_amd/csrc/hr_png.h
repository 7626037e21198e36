// The arithmetic of a PNG file, stated once: shared by the kernels of png_kernel.hip and, compiled by the host compiler, by
// hr_png_encode_host (tests/host_math/hr_png_host.cpp, hyperreel_amd/png.py's encode_host).  Both walk the same functions in the same
// order, everything is integer arithmetic with stated tie-breaks, so both produce the same bytes.
//
// The file:  signature, IHDR, one IDAT chunk per strip of rows, IEND.  8 bits a sample, colour type 0 / 2 / 6, no interlace.
//   plan     hr_png_plan: rows per strip (the strip's filtered bytes, rows * (1 + w * c), stay within HR_PNG_STRIP_BYTES unless one row
//            alone is wider: then one row a strip), strip count, the workspace's layout and hr_png_bound
//   filter   PNG filters 0..4 on raw pixels (a strip's first row reads the source row above it: strips stay independent); adaptive = the
//            smallest sum of min(v, 256 - v) over the row, lowest index on a tie
//   tokens   per strip over its filtered bytes: a byte is a literal; the L equal bytes after it, when L >= 3, are distance-1 matches cut
//            greedily into 258s, a remainder of 1 or 2 being literals (hr_png_token: a position's token from its distance to the run's
//            head and the run's length alone)
//   codes    one dynamic-Huffman block per strip (hr_png_strip_codes): optimal lengths by the two-queue merge over symbols sorted by
//            (count, index), limited to 15 / 7 bits by hr_png_code_lengths' repair, canonical codes, the 16/17/18 run coding of the
//            lengths, HCLEN trimmed; the distance code is absent or the single code 0 at one bit.  The block's exact size comes from the
//            histogram before any bit is written; a strip whose dynamic block is not smaller than its stored form is stored
//   stream   every strip but the last ends with an empty stored block (3 bits, padding, 00 00 FF FF), so strips start on byte boundaries
//            at offsets from a prefix sum; the first chunk carries the zlib header, the last the Adler-32
//   sums     Adler-32 and CRC-32 as partials with combine rules (hr_adler_*, hr_crc_*): lanes and strips checksum slices and merge them
#ifndef HR_PNG_H
#define HR_PNG_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "hr_math.h"      // hr_to8b, HR_FN, HR_HD

#define HR_PNG_STRIP_BYTES 32768      // budget of a strip's filtered bytes: beyond ~32 KB a strip buys nothing (its table costs ~100 B)
#define HR_PNG_MAX_ROWS 256           // ... and of its rows
#define HR_PNG_LL 286                 // literal / length alphabet
#define HR_PNG_EOB 256
#define HR_PNG_HIST_WORDS 288         // counts of the 286 symbols; [286] the number of matches (the distance code's one count); [287] unused
#define HR_PNG_HDR_BYTES 640          // a block header's bits: at most 3 + 14 + 19 * 3 + 287 * 14 = 4092
#define HR_PNG_META_WORDS 8
#define HR_PNG_TOK_COVERED 0xFFFFu    // a position inside a match: no token.  0..255: literal; 256 + (len - 3): match of distance 1
#define HR_PNG_TOK_MATCH 256u
#define HR_PNG_STORED_MAX 65535u
#define HR_PNG_ADLER_MOD 65521u
#define HR_PNG_MAX_BYTES (1ll << 30)  // filtered bytes of an image: offsets and the bound stay inside int32
#define HR_PNG_MAX_ROW_BYTES (1 << 27) // ... and of a row, which may be a strip of its own: 21 bits a token at most, so a strip's bit counts stay inside uint32
#define HR_PNG_FILE_HEAD 33           // signature + IHDR chunk
#define HR_PNG_IEND 12

// per-strip words the kernels hand on (workspace, HR_PNG_META_WORDS each)
enum { HR_PNG_M_ADLER_A = 0, HR_PNG_M_ADLER_B = 1, HR_PNG_M_DYNAMIC = 2, HR_PNG_M_HDR_BITS = 3, HR_PNG_M_BLOCK_BITS = 4, HR_PNG_M_DATA_LEN = 5,
       HR_PNG_M_OFFSET = 6 };
// words after the last strip's
enum { HR_PNG_G_ADLER = 0, HR_PNG_G_WORDS = 4 };

struct hr_png_plan_t {
    int32_t w, h, channels;
    int32_t row_bytes;          // 1 + w * channels
    int32_t rows_per_strip, n_strips;
    int64_t strip_stride;       // bytes between two strips' filtered bytes in the workspace (16-byte multiple)
    int64_t total_bytes;        // h * row_bytes: what the Adler-32 covers
    int64_t off_filtered, off_tokens, off_hist, off_codes, off_hdr, off_meta;      // byte offsets into the workspace
    int64_t workspace_bytes;
    int64_t bound;              // a capacity that always suffices: every strip stored
};

HR_HD int64_t hr_png_stored_bytes(int64_t n) { return n + 5 * ((n + HR_PNG_STORED_MAX - 1) / HR_PNG_STORED_MAX); }

HR_HD hr_png_plan_t hr_png_plan(int32_t w, int32_t h, int32_t channels)
{
    hr_png_plan_t p;
    p.w = w; p.h = h; p.channels = channels;
    p.row_bytes = 1 + w * channels;
    int32_t rows = HR_PNG_STRIP_BYTES / p.row_bytes;
    rows = rows < 1 ? 1 : rows > HR_PNG_MAX_ROWS ? HR_PNG_MAX_ROWS : rows;
    p.rows_per_strip = rows;
    p.n_strips = (h + rows - 1) / rows;
    p.strip_stride = (((int64_t)rows * p.row_bytes + 15) / 16) * 16;
    p.total_bytes = (int64_t)h * p.row_bytes;
    int64_t at = 0;
    p.off_filtered = at; at += p.n_strips * p.strip_stride;
    p.off_tokens = at;   at += p.n_strips * p.strip_stride * 2;
    p.off_hist = at;     at += (int64_t)p.n_strips * HR_PNG_HIST_WORDS * 4;
    p.off_codes = at;    at += (int64_t)p.n_strips * HR_PNG_HIST_WORDS * 4;
    p.off_hdr = at;      at += (int64_t)p.n_strips * HR_PNG_HDR_BYTES;
    p.off_meta = at;     at += ((int64_t)p.n_strips * HR_PNG_META_WORDS + HR_PNG_G_WORDS) * 4;
    p.workspace_bytes = at;
    const int64_t full = (int64_t)rows * p.row_bytes, last = p.total_bytes - (int64_t)(p.n_strips - 1) * full;
    // per strip: chunk length, type and CRC (12), the stored blocks, the alignment marker (5); once: zlib header (2), Adler-32 (4)
    p.bound = HR_PNG_FILE_HEAD + HR_PNG_IEND + 6 + (int64_t)(p.n_strips - 1) * (17 + hr_png_stored_bytes(full)) + 17 + hr_png_stored_bytes(last);
    return p;
}

HR_HD int32_t hr_png_strip_rows(const hr_png_plan_t& p, int32_t s)
{
    const int32_t r0 = s * p.rows_per_strip;
    return p.h - r0 < p.rows_per_strip ? p.h - r0 : p.rows_per_strip;
}

// what both encoders accept: 1 x 1 or more, 1 / 3 / 4 channels, within HR_PNG_MAX_ROW_BYTES a row and HR_PNG_MAX_BYTES in all
HR_HD bool hr_png_shape_ok(int32_t w, int32_t h, int32_t channels)
{
    if (w < 1 || h < 1 || (channels != 1 && channels != 3 && channels != 4)) return false;
    const int64_t row = 1 + (int64_t)w * channels;
    return row <= HR_PNG_MAX_ROW_BYTES && row * h <= HR_PNG_MAX_BYTES;
}

HR_HD int hr_png_color_type(int channels) { return channels == 1 ? 0 : channels == 3 ? 2 : 6; }

// ---------------------------------------------------------------- pixels and filters
// sample i of the frame as 8 bits.  HR_PNG_F32_TO8B: hr_to8b as it stands (NaN gives 0: fmaxf returns its other operand)
HR_FN int hr_png_sample(const void* pixels, int pixel_type, int64_t i)
{
    return pixel_type == HR_PNG_U8 ? (int)((const uint8_t*)pixels)[i] : (int)hr_to8b(((const float*)pixels)[i]);
}

// filter f of a byte: raw, a left, b up, c upper left (zeros outside the image)
HR_HD int hr_png_filter_byte(int f, int raw, int a, int b, int c)
{
    int pred = 0;
    if (f == 1) pred = a;
    else if (f == 2) pred = b;
    else if (f == 3) pred = (a + b) >> 1;
    else if (f == 4) {
        const int p = a + b - c;
        const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
        pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    }
    return (raw - pred) & 255;
}

HR_HD uint32_t hr_png_filter_cost(int v) { return (uint32_t)(v < 128 ? v : 256 - v); }

// the five filters' costs of byte x of row y, added to sums[5]; returns nothing.  row_len = w * channels
HR_FN void hr_png_filter_costs(const void* pixels, int pixel_type, int32_t y, int32_t x, int32_t row_len, int32_t channels, uint32_t sums[5])
{
    const int64_t at = (int64_t)y * row_len + x;
    const int raw = hr_png_sample(pixels, pixel_type, at);
    const int a = x >= channels ? hr_png_sample(pixels, pixel_type, at - channels) : 0;
    const int b = y > 0 ? hr_png_sample(pixels, pixel_type, at - row_len) : 0;
    const int c = (y > 0 && x >= channels) ? hr_png_sample(pixels, pixel_type, at - row_len - channels) : 0;
    HR_UNROLL
    for (int f = 0; f < 5; ++f) sums[f] += hr_png_filter_cost(hr_png_filter_byte(f, raw, a, b, c));
}

HR_FN int hr_png_filtered(const void* pixels, int pixel_type, int32_t y, int32_t x, int32_t row_len, int32_t channels, int f)
{
    const int64_t at = (int64_t)y * row_len + x;
    const int raw = hr_png_sample(pixels, pixel_type, at);
    if (f == 0) return raw;
    const int a = x >= channels ? hr_png_sample(pixels, pixel_type, at - channels) : 0;
    const int b = y > 0 ? hr_png_sample(pixels, pixel_type, at - row_len) : 0;
    const int c = (y > 0 && x >= channels) ? hr_png_sample(pixels, pixel_type, at - row_len - channels) : 0;
    return hr_png_filter_byte(f, raw, a, b, c);
}

// adaptive choice: the smallest sum, the lowest index on a tie
HR_HD int hr_png_choose_filter(const uint32_t sums[5])
{
    int best = 0;
    for (int f = 1; f < 5; ++f)
        if (sums[f] < sums[best]) best = f;
    return best;
}

// ---------------------------------------------------------------- tokens
// The run rule, position by position.  k: the position's distance to the head of its run of equal bytes (0: the head); follow: the
// number of bytes of the run after its head (L).  Exact whenever `follow` is exact up to 258 bytes past the position's chunk.
HR_HD uint32_t hr_png_token(int byte, uint32_t k, uint32_t follow)
{
    if (k == 0 || follow < 3) return (uint32_t)byte;
    const uint32_t j = k - 1, m = j % 258u;
    const uint32_t left = follow - (j - m);                  // bytes of the run from this chunk's first position on
    const uint32_t len = left < 258u ? left : 258u;
    if (len < 3) return (uint32_t)byte;
    return m == 0 ? HR_PNG_TOK_MATCH + (len - 3) : HR_PNG_TOK_COVERED;
}

// length 3..258 -> its symbol, the number of extra bits and their value (RFC 1951 3.2.5)
HR_HD void hr_png_length_code(uint32_t len, uint32_t* sym, uint32_t* ebits, uint32_t* eval)
{
    const uint32_t l = len - 3;
    if (l < 8) { *sym = 257 + l; *ebits = 0; *eval = 0; return; }
    if (l == 255) { *sym = 285; *ebits = 0; *eval = 0; return; }
    uint32_t e = 0;
    while ((l >> (e + 3)) > 1) ++e;
    e += 1;                                                  // floor(log2 l) - 2: l in [2^(e + 2), 2^(e + 3)), four symbols of 2^e lengths each
    *sym = 261 + 4 * e + ((l - (1u << (e + 2))) >> e);
    *ebits = e;
    *eval = l & ((1u << e) - 1u);
}

HR_HD uint32_t hr_png_length_ebits(uint32_t sym) { return (sym < 265 || sym == 285) ? 0u : (sym - 261) >> 2; }

// the symbol a token counts under
HR_HD uint32_t hr_png_token_symbol(uint32_t tok)
{
    if (tok < HR_PNG_TOK_MATCH) return tok;
    uint32_t sym, eb, ev;
    hr_png_length_code(tok - HR_PNG_TOK_MATCH + 3, &sym, &eb, &ev);
    return sym;
}

// A slice of a strip's bytes, as the one who tokenises it sees it from outside
struct hr_png_segment {
    uint32_t len, lead, trail;       // bytes; leading bytes equal to the first; trailing bytes equal to the last
    int first, last;
    uint32_t a, b;                   // Adler partial of the slice (hr_adler_part)
};

// ---------------------------------------------------------------- Adler-32
// Partial of a slice from a zero state: a = sum x_i, b = sum (len - i) x_i, both mod 65521.  The modulo is deferred over 5552 bytes.
HR_HD void hr_adler_part(const uint8_t* p, uint32_t len, uint32_t* a_out, uint32_t* b_out)
{
    uint32_t a = 0, b = 0;
    while (len) {
        const uint32_t n = len < 5552u ? len : 5552u;
        for (uint32_t i = 0; i < n; ++i) { a += p[i]; b += a; }
        a %= HR_PNG_ADLER_MOD; b %= HR_PNG_ADLER_MOD;
        p += n; len -= n;
    }
    *a_out = a; *b_out = b;
}

// the partial of A || B from the partials of A and B and B's length
HR_HD void hr_adler_combine(uint32_t a1, uint32_t b1, uint32_t a2, uint32_t b2, uint64_t len2, uint32_t* a, uint32_t* b)
{
    *a = (a1 + a2) % HR_PNG_ADLER_MOD;
    *b = (uint32_t)((b1 + (uint64_t)(len2 % HR_PNG_ADLER_MOD) * a1 + b2) % HR_PNG_ADLER_MOD);
}

// what a slice adds to the partial of a whole of which `after` bytes follow the slice
HR_HD void hr_adler_place(uint32_t a, uint32_t b, uint64_t after, uint32_t* a_out, uint32_t* b_out)
{
    *a_out = a;
    *b_out = (uint32_t)((b + (uint64_t)(after % HR_PNG_ADLER_MOD) * a) % HR_PNG_ADLER_MOD);
}

// Adler-32 of `len` bytes whose partial is (a, b): the initial s1 = 1 adds 1 to s1 and len to s2
HR_HD uint32_t hr_adler_final(uint32_t a, uint32_t b, uint64_t len)
{
    const uint32_t s1 = (1u + a) % HR_PNG_ADLER_MOD, s2 = (uint32_t)((len % HR_PNG_ADLER_MOD + b) % HR_PNG_ADLER_MOD);
    return (s2 << 16) | s1;
}

// ---------------------------------------------------------------- CRC-32 (reflected 0xEDB88320)
HR_HD uint32_t hr_crc_table_entry(uint32_t i)
{
    for (int k = 0; k < 8; ++k) i = (i & 1u) ? (i >> 1) ^ 0xEDB88320u : i >> 1;
    return i;
}

// the register after one more byte, from a zero state and without the final complement: linear over GF(2)
HR_HD uint32_t hr_crc0_byte(uint32_t crc, int byte) { return hr_crc_table_entry((crc ^ (uint32_t)byte) & 255u) ^ (crc >> 8); }

HR_HD uint32_t hr_crc0(const uint8_t* p, uint64_t len)
{
    uint32_t c = 0;
    for (uint64_t i = 0; i < len; ++i) c = hr_crc0_byte(c, p[i]);
    return c;
}

// a * b mod P, polynomials with bit 31 the coefficient of x^0
HR_HD uint32_t hr_crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}

// x^(8 n) mod P
HR_HD uint32_t hr_crc_xpow8(uint64_t n)
{
    uint32_t r = 0x80000000u, base = 0x00800000u;      // x^0, x^8
    while (n) {
        if (n & 1u) r = hr_crc_mul(r, base);
        base = hr_crc_mul(base, base);
        n >>= 1;
    }
    return r;
}

// the register `crc` after `n` further zero-state bytes: the combine rule is  crc0(A || B) = hr_crc_shift(crc0(A), |B|) ^ crc0(B)
HR_HD uint32_t hr_crc_shift(uint32_t crc, uint64_t n) { return hr_crc_mul(crc, hr_crc_xpow8(n)); }

// CRC-32 of `len` bytes whose zero-state register is crc0: the initial all-ones state, shifted through, and the final complement
HR_HD uint32_t hr_crc_final(uint32_t crc0, uint64_t len) { return hr_crc_shift(0xFFFFFFFFu, len) ^ crc0 ^ 0xFFFFFFFFu; }

// ---------------------------------------------------------------- code lengths
struct hr_png_huff_work {
    uint16_t sorted[HR_PNG_LL];      // used symbols, ascending (count, index)
    uint16_t leaf_parent[HR_PNG_LL], node_parent[HR_PNG_LL], depth[HR_PNG_LL];
    uint32_t node_weight[HR_PNG_LL];
    uint32_t bl[16];
    uint8_t ll_len[HR_PNG_HIST_WORDS];          // 286 literal / length code lengths, then the distance alphabet's one
    uint32_t cl_count[19], cl_code[19];
    uint8_t cl_len[19];
};

// how many used symbols sort before used symbol i: ascending count, then index.  sorted[hr_png_rank(i)] = i
HR_HD int hr_png_rank(const uint32_t* count, int n, int i)
{
    const uint32_t c = count[i];
    int r = 0;
    for (int j = 0; j < n; ++j) {
        const uint32_t d = count[j];
        r += (d != 0 && (d < c || (d == c && j < i))) ? 1 : 0;
    }
    return r;
}

// Length-limited prefix code lengths of the m used symbols wk->sorted[0..m) of count[0..n): the optimal (Huffman) depths by the two-queue
// merge -- a leaf before a node of equal weight -- then, when a depth exceeds `limit`, the deep leaves are cut to it and the Kraft sum
// is repaired one unit of 2^-limit at a time (the deepest leaf above the limit goes one down and takes a cut leaf as its sibling).  The
// lengths are handed out along the sorted order, longest to the rarest: within the limit that is the optimum's cost, and ties are the
// sort's.  Unused symbols get 0; a lone symbol gets 1.
HR_HD void hr_png_code_lengths(const uint32_t* count, int n, int m, int limit, uint8_t* len, hr_png_huff_work* wk)
{
    for (int i = 0; i < n; ++i) len[i] = 0;
    if (m == 0) return;
    if (m == 1) { len[wk->sorted[0]] = 1; return; }
    int li = 0, ni = 0;
    for (int k = 0; k < m - 1; ++k) {
        uint32_t w = 0;
        for (int pick = 0; pick < 2; ++pick) {
            if (li < m && (ni >= k || count[wk->sorted[li]] <= wk->node_weight[ni])) {
                w += count[wk->sorted[li]];
                wk->leaf_parent[li++] = (uint16_t)k;
            } else {
                w += wk->node_weight[ni];
                wk->node_parent[ni++] = (uint16_t)k;
            }
        }
        wk->node_weight[k] = w;
    }
    wk->depth[m - 2] = 0;
    for (int k = m - 3; k >= 0; --k) wk->depth[k] = (uint16_t)(wk->depth[wk->node_parent[k]] + 1);
    for (int b = 0; b <= limit; ++b) wk->bl[b] = 0;
    uint64_t kraft = 0;                                       // in units of 2^-limit
    for (int r = 0; r < m; ++r) {
        int d = wk->depth[wk->leaf_parent[r]] + 1;
        if (d > limit) d = limit;
        wk->bl[d] += 1;
        kraft += 1ull << (limit - d);
    }
    for (uint64_t excess = kraft - (1ull << limit); excess > 0; --excess) {
        int bits = limit - 1;
        while (wk->bl[bits] == 0) --bits;
        wk->bl[bits] -= 1;
        wk->bl[bits + 1] += 2;
        wk->bl[limit] -= 1;
    }
    int r = 0;
    for (int bits = limit; bits >= 1; --bits)
        for (uint32_t j = 0; j < wk->bl[bits]; ++j) len[wk->sorted[r++]] = (uint8_t)bits;
}

HR_HD uint32_t hr_png_bit_reverse(uint32_t v, int bits)
{
    uint32_t r = 0;
    for (int i = 0; i < bits; ++i) { r = (r << 1) | (v & 1u); v >>= 1; }
    return r;
}

// canonical codes (RFC 1951 3.2.2), bit-reversed for the LSB-first stream: out[i] = code | len << 16
HR_HD void hr_png_canonical(const uint8_t* len, int n, int limit, uint32_t* out)
{
    uint32_t count[16], next[16];
    for (int b = 0; b <= limit; ++b) count[b] = 0;
    for (int i = 0; i < n; ++i) count[len[i]] += 1;
    count[0] = 0;
    uint32_t code = 0;
    for (int b = 1; b <= limit; ++b) { code = (code + count[b - 1]) << 1; next[b] = code; }
    for (int i = 0; i < n; ++i) {
        const int l = len[i];
        out[i] = l ? (hr_png_bit_reverse(next[l]++, l) | ((uint32_t)l << 16)) : 0u;
    }
}

// The code-length alphabet's next symbol for seq[*pos..n): 18 / 17 for 11..138 / 3..10 zeros, 16 for 3..6 repeats of the length just
// before, else the length itself.  Advances *pos.
HR_HD int hr_png_cl_next(const uint8_t* seq, int n, int* pos, int* ebits, int* eval)
{
    const int at = *pos, v = seq[at];
    int run = 1;
    while (at + run < n && seq[at + run] == v && run < 138) ++run;
    *ebits = 0; *eval = 0;
    if (v == 0 && run >= 11) { *pos = at + run; *ebits = 7; *eval = run - 11; return 18; }
    if (v == 0 && run >= 3) { *pos = at + run; *ebits = 3; *eval = run - 3; return 17; }
    if (v != 0 && at > 0 && seq[at - 1] == v && run >= 3) {
        const int r = run < 6 ? run : 6;
        *pos = at + r; *ebits = 2; *eval = r - 3;
        return 16;
    }
    *pos = at + 1;
    return v;
}

// LSB-first bit writer over bytes it alone writes (nothing needs clearing beforehand)
struct hr_png_bits {
    uint8_t* p;
    uint64_t acc;
    uint32_t fill, total;
};
HR_HD void hr_png_put(hr_png_bits* w, uint32_t value, uint32_t bits)
{
    w->acc |= (uint64_t)value << w->fill;
    w->fill += bits; w->total += bits;
    while (w->fill >= 8) { *w->p++ = (uint8_t)w->acc; w->acc >>= 8; w->fill -= 8; }
}
HR_HD void hr_png_flush(hr_png_bits* w)
{
    if (w->fill) { *w->p++ = (uint8_t)w->acc; w->acc = 0; w->fill = 0; }
}

// bytes of a strip's chunk data: [zlib header] body [00 00 FF FF | Adler-32]; the body of every strip but the last takes the marker's 3
// header bits and its padding
HR_HD uint32_t hr_png_data_len(int dynamic, uint32_t block_bits, uint32_t n, int first, int last)
{
    const uint32_t body = dynamic ? (block_bits + (last ? 0u : 3u) + 7u) / 8u : (uint32_t)hr_png_stored_bytes(n) + (last ? 0u : 1u);
    return (first ? 2u : 0u) + body + 4u;
}

// One strip's block, from its histogram (hist[256] counts the end-of-block once) and wk->sorted[0..m) (hr_png_rank): the code table
// (codes[0..286), codes[286] the distance code), the header's bits (hdr, HR_PNG_HDR_BYTES) and the strip's meta words DYNAMIC,
// HDR_BITS, BLOCK_BITS and DATA_LEN.  n: the strip's filtered bytes.
HR_HD void hr_png_strip_codes(const uint32_t* hist, int m, uint32_t n, int first, int last, hr_png_huff_work* wk, uint32_t* codes, uint8_t* hdr,
                              uint32_t* meta)
{
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    hr_png_code_lengths(hist, HR_PNG_LL, m, 15, wk->ll_len, wk);
    int hlit = HR_PNG_LL;
    while (hlit > 257 && wk->ll_len[hlit - 1] == 0) --hlit;
    const int n_seq = hlit + 1;
    const uint8_t keep = wk->ll_len[hlit];                   // the distance alphabet's single length follows the hlit lengths
    wk->ll_len[hlit] = hist[HR_PNG_LL] ? 1 : 0;
    for (int i = 0; i < 19; ++i) wk->cl_count[i] = 0;
    int eb, ev;
    for (int pos = 0; pos < n_seq;) wk->cl_count[hr_png_cl_next(wk->ll_len, n_seq, &pos, &eb, &ev)] += 1;
    int cm = 0;
    for (int i = 0; i < 19; ++i)
        if (wk->cl_count[i]) { wk->sorted[hr_png_rank(wk->cl_count, 19, i)] = (uint16_t)i; ++cm; }
    hr_png_code_lengths(wk->cl_count, 19, cm, 7, wk->cl_len, wk);
    hr_png_canonical(wk->cl_len, 19, 7, wk->cl_code);
    int hclen = 19;
    while (hclen > 4 && wk->cl_len[order[hclen - 1]] == 0) --hclen;

    hr_png_bits w = {hdr, 0, 0, 0};
    hr_png_put(&w, last ? 1u : 0u, 1);
    hr_png_put(&w, 2u, 2);
    hr_png_put(&w, (uint32_t)(hlit - 257), 5);
    hr_png_put(&w, 0u, 5);
    hr_png_put(&w, (uint32_t)(hclen - 4), 4);
    for (int i = 0; i < hclen; ++i) hr_png_put(&w, wk->cl_len[order[i]], 3);
    for (int pos = 0; pos < n_seq;) {
        const int s = hr_png_cl_next(wk->ll_len, n_seq, &pos, &eb, &ev);
        hr_png_put(&w, wk->cl_code[s] & 0xFFFFu, wk->cl_code[s] >> 16);
        if (eb) hr_png_put(&w, (uint32_t)ev, (uint32_t)eb);
    }
    hr_png_flush(&w);
    const uint32_t dist_len = wk->ll_len[hlit];
    wk->ll_len[hlit] = keep;

    hr_png_canonical(wk->ll_len, HR_PNG_LL, 15, codes);
    codes[HR_PNG_LL] = dist_len << 16;                       // code 0, one bit -- or no code
    codes[HR_PNG_LL + 1] = 0;
    uint32_t bits = w.total;
    for (int s = 0; s < HR_PNG_LL; ++s) bits += hist[s] * (wk->ll_len[s] + (s > 256 ? hr_png_length_ebits((uint32_t)s) : 0u));
    bits += hist[HR_PNG_LL];
    const int dynamic = (bits + 7u) / 8u < (uint32_t)hr_png_stored_bytes(n) ? 1 : 0;
    meta[HR_PNG_M_DYNAMIC] = (uint32_t)dynamic;
    meta[HR_PNG_M_HDR_BITS] = w.total;
    meta[HR_PNG_M_BLOCK_BITS] = bits;
    meta[HR_PNG_M_DATA_LEN] = hr_png_data_len(dynamic, bits, n, first, last);
}

// a token's bits (value, count) under a strip's code table
HR_HD void hr_png_token_bits(const uint32_t* codes, uint32_t tok, uint32_t* value, uint32_t* count)
{
    if (tok == HR_PNG_TOK_COVERED) { *value = 0; *count = 0; return; }
    if (tok < HR_PNG_TOK_MATCH) { *value = codes[tok] & 0xFFFFu; *count = codes[tok] >> 16; return; }
    uint32_t sym, eb, ev;
    hr_png_length_code(tok - HR_PNG_TOK_MATCH + 3, &sym, &eb, &ev);
    const uint32_t l = codes[sym] >> 16;
    *value = (codes[sym] & 0xFFFFu) | (ev << l);              // then the distance code 0: one zero bit
    *count = l + eb + 1;
}

// Byte q of a stored strip's blocks (of hr_png_stored_bytes(n) bytes): header, LEN, NLEN, then up to 65535 filtered bytes a block
HR_HD int hr_png_stored_byte(const uint8_t* filtered, uint32_t n, uint32_t q, int last)
{
    const uint32_t blk = q / (HR_PNG_STORED_MAX + 5u), r = q % (HR_PNG_STORED_MAX + 5u);
    const uint32_t left = n - blk * HR_PNG_STORED_MAX, len = left < HR_PNG_STORED_MAX ? left : HR_PNG_STORED_MAX;
    switch (r) {
    case 0: return (last && left <= HR_PNG_STORED_MAX) ? 1 : 0;
    case 1: return (int)(len & 255u);
    case 2: return (int)(len >> 8);
    case 3: return (int)(~len & 255u);
    case 4: return (int)((~len >> 8) & 255u);
    default: return filtered[blk * HR_PNG_STORED_MAX + (r - 5u)];
    }
}

HR_HD void hr_png_be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

// signature and IHDR (HR_PNG_FILE_HEAD bytes)
HR_HD void hr_png_file_head(uint8_t* p, int32_t w, int32_t h, int32_t channels)
{
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    for (int i = 0; i < 8; ++i) p[i] = sig[i];
    hr_png_be32(p + 8, 13);
    p[12] = 'I'; p[13] = 'H'; p[14] = 'D'; p[15] = 'R';
    hr_png_be32(p + 16, (uint32_t)w);
    hr_png_be32(p + 20, (uint32_t)h);
    p[24] = 8; p[25] = (uint8_t)hr_png_color_type(channels); p[26] = 0; p[27] = 0; p[28] = 0;
    uint32_t c = 0;
    for (int i = 12; i < 29; ++i) c = hr_crc0_byte(c, p[i]);
    hr_png_be32(p + 29, hr_crc_final(c, 17));
}

HR_HD void hr_png_file_tail(uint8_t* p)
{
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    for (int i = 0; i < 12; ++i) p[i] = iend[i];
}

// ---------------------------------------------------------------- slices of a strip
HR_HD hr_png_segment hr_png_segment_scan(const uint8_t* p, uint32_t len)
{
    hr_png_segment s;
    s.len = len; s.lead = 0; s.trail = 0; s.first = 0; s.last = 0; s.a = 0; s.b = 0;
    if (!len) return s;
    s.first = p[0]; s.last = p[len - 1];
    uint32_t run = 0;
    int prev = -1;
    bool leading = true;
    for (uint32_t i = 0; i < len; ++i) {
        const int v = p[i];
        run = v == prev ? run + 1 : 1;
        if (leading && v == s.first) s.lead = i + 1; else leading = false;
        prev = v;
    }
    s.trail = run;
    hr_adler_part(p, len, &s.a, &s.b);
    return s;
}

// The scan operator of runs across slices.  A state is (length of the run ending at the block's last byte) << 1 | (the block is one run).
// `right` is the later block, `left` the block before it, joint_equal whether the bytes on both sides of their joint are equal.
HR_HD uint32_t hr_png_run_join(uint32_t right, uint32_t left, bool joint_equal)
{
    if (!(right & 1u)) return right;
    if (!joint_equal) return right & ~1u;
    return (((right >> 1) + (left >> 1)) << 1) | (left & 1u);
}

// Tokens of the slice p[0..len): `before` bytes equal to p[0] end just before it and belong to its run (the run's head among them);
// `after` bytes equal to p[len - 1] follow it (exact, or any count >= 258).  emit(i, token) once per position, in order.
template <class Emit>
HR_HD void hr_png_segment_tokens(const uint8_t* p, uint32_t len, uint32_t before, uint32_t after, Emit&& emit)
{
    uint32_t i = 0, k = before;                              // k: distance of position i to its run's head
    while (i < len) {
        const int v = p[i];
        uint32_t j = i + 1;
        while (j < len && p[j] == v) ++j;
        const uint32_t follow = k + (j - i) - 1 + (j == len ? after : 0u);
        for (uint32_t q = i; q < j; ++q) emit(q, hr_png_token(v, k + (q - i), follow));
        i = j; k = 0;
    }
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------- the launch (png_kernel.hip)
struct HrPngArgs {
    const void* pixels;          // (h, w, channels): bytes or floats
    int32_t pixel_type, filter_mode;
    hr_png_plan_t plan;
    uint8_t* workspace;          // plan.workspace_bytes, 16-byte aligned
    uint8_t* file;               // plan.bound bytes or more
    int64_t* file_bytes;
};
hipError_t hr_launch_png_encode(const HrPngArgs& a, hipStream_t stream);
#endif

#if !defined(__HIPCC__)
// ---------------------------------------------------------------- the whole file on the host
// What the three kernels do, strip by strip.  filtered_out (h * (1 + w * c) bytes) and tokens_out (as many uint16) may be NULL.
// Returns the file's length, or -1 when the shape is not hr_png_shape_ok or `capacity` is below hr_png_bound.
#include <vector>
static inline int64_t hr_png_encode_host(const void* pixels, int pixel_type, int filter_mode, int32_t w, int32_t h, int32_t channels, uint8_t* file,
                                         int64_t capacity, uint8_t* filtered_out, uint16_t* tokens_out, uint8_t* row_filters_out)
{
    if (!hr_png_shape_ok(w, h, channels)) return -1;
    const hr_png_plan_t pl = hr_png_plan(w, h, channels);
    if (capacity < pl.bound) return -1;
    const int32_t row_len = w * channels;
    std::vector<uint8_t> filt((size_t)pl.rows_per_strip * pl.row_bytes);
    std::vector<uint16_t> tok(filt.size());
    std::vector<uint8_t> hdr(HR_PNG_HDR_BYTES), body;
    hr_png_huff_work wk;
    uint32_t hist[HR_PNG_HIST_WORDS], codes[HR_PNG_HIST_WORDS], meta[HR_PNG_META_WORDS];
    uint32_t adler_a = 0, adler_b = 0;
    hr_png_file_head(file, w, h, channels);
    int64_t at = HR_PNG_FILE_HEAD;
    for (int32_t s = 0; s < pl.n_strips; ++s) {
        const int32_t rows = hr_png_strip_rows(pl, s), y0 = s * pl.rows_per_strip;
        const uint32_t n = (uint32_t)rows * (uint32_t)pl.row_bytes;
        const int first = s == 0, last = s == pl.n_strips - 1;
        // kernel A: filters, tokens, histogram, Adler partial
        for (int32_t r = 0; r < rows; ++r) {
            int f = filter_mode;
            if (filter_mode == HR_PNG_FILTER_ADAPTIVE) {
                uint32_t sums[5] = {0, 0, 0, 0, 0};
                for (int32_t x = 0; x < row_len; ++x) hr_png_filter_costs(pixels, pixel_type, y0 + r, x, row_len, channels, sums);
                f = hr_png_choose_filter(sums);
            }
            uint8_t* o = filt.data() + (size_t)r * pl.row_bytes;
            o[0] = (uint8_t)f;
            if (row_filters_out) row_filters_out[y0 + r] = (uint8_t)f;
            for (int32_t x = 0; x < row_len; ++x) o[1 + x] = (uint8_t)hr_png_filtered(pixels, pixel_type, y0 + r, x, row_len, channels, f);
        }
        for (int i = 0; i < HR_PNG_HIST_WORDS; ++i) hist[i] = i == HR_PNG_EOB ? 1u : 0u;
        const hr_png_segment seg = hr_png_segment_scan(filt.data(), n);
        hr_png_segment_tokens(filt.data(), n, 0u, 0u, [&](uint32_t i, uint32_t t) {
            tok[i] = (uint16_t)t;
            if (t != HR_PNG_TOK_COVERED) hist[hr_png_token_symbol(t)] += 1;
            if (t != HR_PNG_TOK_COVERED && t >= HR_PNG_TOK_MATCH) hist[HR_PNG_LL] += 1;
        });
        const uint64_t off = (uint64_t)y0 * (uint64_t)pl.row_bytes;
        uint32_t pa, pb;
        hr_adler_place(seg.a, seg.b, (uint64_t)pl.total_bytes - off - n, &pa, &pb);
        adler_a = (adler_a + pa) % HR_PNG_ADLER_MOD;
        adler_b = (adler_b + pb) % HR_PNG_ADLER_MOD;
        if (filtered_out) memcpy(filtered_out + off, filt.data(), n);
        if (tokens_out) memcpy(tokens_out + off, tok.data(), 2 * (size_t)n);
        // kernel B: the strip's code
        int m = 0;
        for (int i = 0; i < HR_PNG_LL; ++i)
            if (hist[i]) { wk.sorted[hr_png_rank(hist, HR_PNG_LL, i)] = (uint16_t)i; ++m; }
        hr_png_strip_codes(hist, m, n, first, last, &wk, codes, hdr.data(), meta);
        // kernel C: the chunk
        const uint32_t data_len = meta[HR_PNG_M_DATA_LEN];
        uint8_t* chunk = file + at;
        hr_png_be32(chunk, data_len);
        chunk[4] = 'I'; chunk[5] = 'D'; chunk[6] = 'A'; chunk[7] = 'T';
        uint8_t* d = chunk + 8;
        memset(d, 0, data_len);
        uint32_t pos = 0;
        if (first) { d[0] = 0x78; d[1] = 0x01; pos = 2; }
        if (meta[HR_PNG_M_DYNAMIC]) {
            const uint32_t hb = meta[HR_PNG_M_HDR_BITS];
            memcpy(d + pos, hdr.data(), (hb + 7) / 8);
            uint64_t bit = (uint64_t)pos * 8 + hb;
            auto put = [&](uint32_t value, uint32_t count) {
                for (uint32_t b = 0; b < count; ++b, ++bit)
                    if ((value >> b) & 1u) d[bit >> 3] |= (uint8_t)(1u << (bit & 7));
            };
            for (uint32_t i = 0; i < n; ++i) {
                uint32_t value, count;
                hr_png_token_bits(codes, tok[i], &value, &count);
                put(value, count);
            }
            put(codes[HR_PNG_EOB] & 0xFFFFu, codes[HR_PNG_EOB] >> 16);
            if (!last) bit += 3;
            pos = (uint32_t)((bit + 7) / 8);
        } else {
            const uint32_t sb = (uint32_t)hr_png_stored_bytes(n);
            for (uint32_t q = 0; q < sb; ++q) d[pos + q] = (uint8_t)hr_png_stored_byte(filt.data(), n, q, last);
            pos += sb + (last ? 0u : 1u);
        }
        if (last) hr_png_be32(d + pos, hr_adler_final(adler_a, adler_b, (uint64_t)pl.total_bytes));
        else { d[pos] = 0; d[pos + 1] = 0; d[pos + 2] = 0xFF; d[pos + 3] = 0xFF; }
        hr_png_be32(d + data_len, hr_crc_final(hr_crc0(chunk + 4, 4 + (uint64_t)data_len), 4 + (uint64_t)data_len));
        at += 12 + (int64_t)data_len;
    }
    hr_png_file_tail(file + at);
    return at + HR_PNG_IEND;
}
#endif

#endif  // HR_PNG_H
