// The other half of hr_png.h: a PNG file back into pixels, stated once for the kernels of png_decode_kernel.hip and, compiled by the host
// compiler, for hr_png_decode_host (hyperreel_amd/csrc/png_decode_host.cpp, tests/host_math/hr_png_decode_host.cpp).  Integer arithmetic
// only; the canonical codes, the bit reversal, the filter predictors and the CRC-32 / Adler-32 partials with their combine rules are
// hr_png.h's, not restated.
//
// Every function takes (lane, lanes): the host calls it with (0, 1), a kernel with one wavefront's (lane, 64).  All lanes walk the same
// control flow over the same values -- the file's bytes and the tables are read by every lane alike -- and split only the work that
// has a parallel axis: checksums of slices, table fills, match copies, the flush of the window.  HR_PNG_SYNC orders one lane's LDS
// writes before the others' reads; it is nothing on the host.  HR_PNG_UNIFORM tells the compiler which loaded values all lanes share.
//
//   container  hr_png_walk: signature, IHDR first (length 13), the CRC-32 of every chunk, IDAT chunks consecutive, IEND present; other
//              chunks are skipped by length.  Accepted: 8 bits a sample, colour type 0 / 2 / 4 / 6, no interlace; the rest is
//              HR_PNG_E_UNSUPPORTED, never guessed at.  Every step consumes a whole chunk (12 bytes or more), so the walk ends.
//   reader     hr_png_reader: the zlib stream's bytes across IDAT boundaries -- at the end of a chunk it skips the CRC, reads the next
//              length and requires the type IDAT -- checked against the end of the file and of the chunk, feeding a 64-bit LSB-first
//              bit buffer.  A boundary may fall anywhere: inside a code, inside extra bits, between LEN and NLEN.  hr_png_refill, once
//              per turn of every loop, brings the buffer to 48 bits (six bytes in two steps inside a chunk, else byte by byte);
//              hr_png_take only hands bits out.  A kernel reads the file through an aligned 4 KB block of it in LDS that all lanes fill.
//   inflate    hr_png_inflate: the zlib header (check bits, CM 8, window up to 32 KB, no preset dictionary), stored (LEN / ~LEN), fixed
//              and dynamic blocks.  A set of code lengths is taken or refused as zlib's inflate does: over-subscribed sets are refused,
//              incomplete ones too except a single code of one bit (never for the code-length code), an empty distance set is fine
//              until a length symbol occurs; symbol 16 needs a length before it, a run may not pass the end, the end-of-block code must
//              exist.  In a block: length symbols 286 / 287, distance symbols 30 / 31 and unassigned codes are refused, and so is a
//              distance beyond the bytes produced so far.  Two-level tables (hr_png_build_table): root bits, then one sub-table of
//              (longest - root) bits per root prefix that long codes share; in a complete canonical code those prefixes are the last
//              2^root - p0 ones in code order, p0 the root entries the short codes cover, so a sub-table's index is prefix - p0.
//              Every symbol consumes one bit or more, or ends the decode.
//   window     the last 32 KB of output live in hr_png_inflate_mem.win (LDS on the device); a match is  win[pos + i] = win[pos - dist
//              + i % dist]  for i < len, lanes taking i (hr_png_put_match says why that holds at the window's edge); hr_png_drain, once
//              per turn of a loop, flushes a full piece of HR_PNG_PIECE bytes to the filtered-bytes buffer and adds it to the Adler-32
//              by slices (hr_adler_part / place / combine).  Output beyond h * (1 + w * c) bytes is refused
//              before it is written, fewer is refused at the end, then the Adler-32 is compared.
//   unfilter   hr_png_unfilter_pixel: filters 0..4 over packed pixels (a left, b up, c upper left) through hr_png_filter_byte;
//   convert    hr_png_convert_pixel: PIL's convert('L' | 'RGB' | 'RGBA') of the four colour types at 8 bits -- grey replicates, an
//              absent alpha is 255, alpha is dropped without compositing, colour to L is (19595 R + 38470 G + 7471 B + 32768) >> 16.
// A damaged file ends in a status after a bounded number of steps and its image is all zeros.
#ifndef HR_PNG_DECODE_H
#define HR_PNG_DECODE_H

#include "hr_png.h"

#define HR_PNG_WINDOW 32768u
#define HR_PNG_PIECE 4096u             // the window is flushed, and the Adler-32 accumulated, in pieces of this size
#define HR_PNG_LIT_ROOT 10
#define HR_PNG_DIST_ROOT 8
#define HR_PNG_CL_ROOT 7
// root entries + sub-tables: a prefix shared by long codes holds two of them or more, so 286 / 2 and 30 / 2 sub-tables at most
#define HR_PNG_LIT_TABLE ((1 << HR_PNG_LIT_ROOT) + 144 * (1 << (15 - HR_PNG_LIT_ROOT)))
#define HR_PNG_DIST_TABLE ((1 << HR_PNG_DIST_ROOT) + 16 * (1 << (15 - HR_PNG_DIST_ROOT)))
#define HR_PNG_CL_TABLE (1 << HR_PNG_CL_ROOT)
#define HR_PNG_DEC_META_WORDS 4        // per image, between the kernels: status, the file's channels, the first IDAT chunk's offset
#define HR_PNG_ENTRY_LINK 0x8000u      // a table entry: symbol | bits << 9; or LINK | sub-table; 0: no such code

// HR_PNG_UNIFORM(x): x is the same in every lane -- a byte of the file, a table entry -- and the compiler is told so (it cannot see it
// through a vector load).  The serial state and the branches on it then live in scalar registers and scalar branches: without it
// every `if` of the decoder is compiled as a divergent region with a saved execution mask, and the state as vector registers.
// HR_PNG_STAGED: a kernel reads the file, which lies in global memory, through a block of it copied to LDS; the host reads the file itself
#if defined(__HIP_DEVICE_COMPILE__)
#define HR_PNG_STAGED 1
#define HR_PNG_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#define HR_PNG_SYNC() __syncthreads()
HR_FN uint32_t hr_png_lanes_add(uint32_t v) { for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off); return v; }
HR_FN uint32_t hr_png_lanes_xor(uint32_t v) { for (int off = 32; off; off >>= 1) v ^= __shfl_xor(v, off); return v; }
#else
#define HR_PNG_STAGED 0
#define HR_PNG_UNIFORM(x) ((uint32_t)(x))
#define HR_PNG_SYNC() ((void)0)
HR_HD uint32_t hr_png_lanes_add(uint32_t v) { return v; }
HR_HD uint32_t hr_png_lanes_xor(uint32_t v) { return v; }
#endif

HR_HD uint32_t hr_png_rd32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]; }
HR_HD bool hr_png_is_type(const uint8_t* p, char a, char b, char c, char d) { return p[0] == (uint8_t)a && p[1] == (uint8_t)b && p[2] == (uint8_t)c && p[3] == (uint8_t)d; }

// channels of a colour type at 8 bits (0 for a type PNG does not define); palette indices count as one
HR_HD int hr_png_type_channels(int color_type) { return color_type == 0 || color_type == 3 ? 1 : color_type == 2 ? 3 : color_type == 4 ? 2 : color_type == 6 ? 4 : 0; }

// signature and IHDR into info, no checksum: HR_PNG_OK, HR_PNG_E_SIGNATURE, HR_PNG_E_TRUNCATED or HR_PNG_E_CHUNK
HR_HD int hr_png_read_head(const uint8_t* f, int64_t n, hr_png_info* info)
{
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    info->width = 0; info->height = 0; info->bit_depth = 0; info->color_type = 0; info->channels = 0; info->interlace = 0; info->supported = 0;
    info->reserved = 0;
    for (int i = 0; i < 8 && i < n; ++i)
        if (f[i] != sig[i]) return HR_PNG_E_SIGNATURE;
    if (n < HR_PNG_FILE_HEAD) return HR_PNG_E_TRUNCATED;
    if (hr_png_rd32(f + 8) != 13u || !hr_png_is_type(f + 12, 'I', 'H', 'D', 'R')) return HR_PNG_E_CHUNK;
    const uint32_t w = hr_png_rd32(f + 16), h = hr_png_rd32(f + 20);
    if (w == 0 || h == 0 || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu) return HR_PNG_E_CHUNK;
    info->width = (int32_t)w; info->height = (int32_t)h;
    info->bit_depth = f[24]; info->color_type = f[25]; info->interlace = f[28];
    info->channels = hr_png_type_channels(f[25]);
    info->supported = (f[24] == 8 && (f[25] == 0 || f[25] == 2 || f[25] == 4 || f[25] == 6) && f[26] == 0 && f[27] == 0 && f[28] == 0) ? 1 : 0;
    return HR_PNG_OK;
}

// CRC-32 of len bytes, the lanes taking slices merged by the x^(8 n) rule
HR_HD uint32_t hr_png_crc_lanes(const uint8_t* p, uint64_t len, int lane, int lanes)
{
    const uint64_t per = (len + (uint64_t)lanes - 1) / (uint64_t)lanes;
    const uint64_t beg = (uint64_t)lane * per < len ? (uint64_t)lane * per : len, end = beg + per < len ? beg + per : len;
    uint32_t c = hr_crc0(p + beg, end - beg);
    if (lanes > 1) c = hr_png_lanes_xor(end > beg ? hr_crc_shift(c, len - end) : 0u);
    return hr_crc_final(c, len);
}

// The container.  expect_w / expect_h: the decoder's size, or -1 for the file's own.  *idat_at: offset of the first IDAT chunk.
HR_HD int hr_png_walk(const uint8_t* f, int64_t n, int32_t expect_w, int32_t expect_h, hr_png_info* info, int64_t* idat_at, int lane, int lanes)
{
    *idat_at = 0;
    if (int st = hr_png_read_head(f, n, info)) return st;
    if (n > 0x7FFFFFFFll) return HR_PNG_E_UNSUPPORTED;        // the reader's offsets are 32 bits
    if (hr_png_crc_lanes(f + 12, 17, lane, lanes) != hr_png_rd32(f + 29)) return HR_PNG_E_CRC;
    if (!info->supported) return HR_PNG_E_UNSUPPORTED;
    if (expect_w >= 0 && (info->width != expect_w || info->height != expect_h)) return HR_PNG_E_SIZE;
    int64_t at = HR_PNG_FILE_HEAD;
    bool seen = false, closed = false;
    for (;;) {                                                // a chunk per turn: at grows by 12 or more
        if (n - at < 12) return HR_PNG_E_TRUNCATED;
        const uint32_t len = hr_png_rd32(f + at);
        if (len > 0x7FFFFFFFu) return HR_PNG_E_CHUNK;
        if ((int64_t)len > n - at - 12) return HR_PNG_E_TRUNCATED;
        const uint8_t* type = f + at + 4;
        if (hr_png_crc_lanes(type, 4 + (uint64_t)len, lane, lanes) != hr_png_rd32(type + 4 + len)) return HR_PNG_E_CRC;
        if (hr_png_is_type(type, 'I', 'H', 'D', 'R')) return HR_PNG_E_CHUNK;
        if (hr_png_is_type(type, 'I', 'D', 'A', 'T')) {
            if (closed) return HR_PNG_E_CHUNK;
            if (!seen) { seen = true; *idat_at = at; }
        } else {
            if (seen) closed = true;
            if (hr_png_is_type(type, 'I', 'E', 'N', 'D')) return seen ? HR_PNG_OK : HR_PNG_E_CHUNK;
        }
        at += 12 + (int64_t)len;
    }
}

// ---------------------------------------------------------------- the zlib stream's bytes and bits
#define HR_PNG_STAGE 4096              // bytes of the file a kernel keeps in LDS in front of the reader

// What the decoder looks at once per 4 KB or less often -- the file, its end, the output -- kept in memory (LDS in a kernel), not in
// registers that would be carried through the symbol loop.  Read through these; every lane reads the same values.
struct hr_png_cold {
    const uint8_t* file;
    uint8_t* out;
    uint32_t end;
};

// Offsets into the file are 32 bits: hr_png_walk refuses a file of 2^31 bytes or more, so the serial state stays small.
struct hr_png_reader {
    const hr_png_cold* cold;
    uint8_t* stage_mem;          // staged: the file's block of HR_PNG_STAGE bytes that starts at stage_at, a copy in LDS; else the file itself is read
    uint32_t pos;                // next byte
    uint32_t left;               // bytes left in the current IDAT chunk; at 0, pos stands on the chunk's CRC
    uint32_t stage_at;           // a multiple of HR_PNG_STAGE, or all ones before the first block is staged
    uint32_t fill;
    uint64_t acc;
    int lane, lanes;
};

// idat_at: the first IDAT chunk's offset (33 or more).  The reader starts as if at the end of a chunk before it.  stage_mem: HR_PNG_STAGE
// bytes (used where HR_PNG_STAGED).
HR_HD void hr_png_reader_init(hr_png_reader* r, const hr_png_cold* cold, uint32_t idat_at, uint8_t* stage_mem, int lane, int lanes)
{
    r->cold = cold; r->pos = idat_at - 4u; r->left = 0; r->acc = 0; r->fill = 0; r->lane = lane; r->lanes = lanes;
    r->stage_mem = stage_mem;
    r->stage_at = 0xFFFFFFFFu;
}

// the block of HR_PNG_STAGE bytes of the file that holds pos, copied by all lanes
HR_HD void hr_png_reader_stage(hr_png_reader* r)
{
    HR_PNG_SYNC();
    const uint32_t at = r->pos & ~(HR_PNG_STAGE - 1u), rest = HR_PNG_UNIFORM(r->cold->end) - at, n = rest < HR_PNG_STAGE ? rest : HR_PNG_STAGE;
    for (uint32_t i = (uint32_t)r->lane; i < n; i += (uint32_t)r->lanes) r->stage_mem[i] = r->cold->file[at + i];
    r->stage_at = at;
    HR_PNG_SYNC();
}

// steps to the next IDAT chunk when the current one is used up: false when there is none
HR_HD bool hr_png_reader_chunk(hr_png_reader* r)
{
    while (r->left == 0) {                                    // 12 bytes a turn
        const uint32_t rest = HR_PNG_UNIFORM(r->cold->end) - r->pos;
        if (rest < 12u) return false;
        const uint8_t* p = r->cold->file + r->pos + 4;
        if (HR_PNG_UNIFORM(hr_png_rd32(p + 4)) != 0x49444154u) return false;      // "IDAT"
        const uint32_t len = HR_PNG_UNIFORM(hr_png_rd32(p));
        if (rest < 16u || len > rest - 16u) return false;      // its data and its CRC lie inside the file
        r->pos += 12u;
        r->left = len;
    }
    return true;
}

HR_HD bool hr_png_reader_byte(hr_png_reader* r, uint32_t* b)
{
    if (!hr_png_reader_chunk(r)) return false;
    if (HR_PNG_STAGED && (r->pos & ~(HR_PNG_STAGE - 1u)) != r->stage_at) hr_png_reader_stage(r);
    *b = HR_PNG_UNIFORM(HR_PNG_STAGED ? r->stage_mem[r->pos & (HR_PNG_STAGE - 1u)] : r->cold->file[r->pos]);
    r->pos += 1u; r->left -= 1u;
    return true;
}

// Fills the bit buffer to 48 bits or more while the stream lasts -- what the longest turn of any loop below consumes (a length and
// a distance code with their extra bits) --, four and two bytes in a step where the chunk and the stage hold them, else byte by byte.
// hr_png_take itself never reads input: the loops call this once a turn.
HR_HD void hr_png_refill(hr_png_reader* r)
{
    if (r->fill >= 48u) return;
    const uint32_t in_stage = r->pos & (HR_PNG_STAGE - 1u);
    if (r->left >= 6u && (!HR_PNG_STAGED || (r->pos - in_stage == r->stage_at && in_stage + 6u <= HR_PNG_STAGE))) {
        const uint8_t* p = HR_PNG_STAGED ? r->stage_mem + in_stage : r->cold->file + r->pos;
        uint32_t take = 2u, word = (uint32_t)p[0] | ((uint32_t)p[1] << 8);
        if (r->fill <= 32u) { word |= ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); take = 4u; }
        r->acc |= (uint64_t)HR_PNG_UNIFORM(word) << r->fill;
        r->fill += 8u * take; r->pos += take; r->left -= take;
        if (r->fill >= 48u) return;
        const uint32_t more = HR_PNG_UNIFORM((uint32_t)p[4] | ((uint32_t)p[5] << 8));
        r->acc |= (uint64_t)more << r->fill;
        r->fill += 16u; r->pos += 2u; r->left -= 2u;
        return;
    }
    uint32_t b;
    while (r->fill <= 56u && hr_png_reader_byte(r, &b)) { r->acc |= (uint64_t)b << r->fill; r->fill += 8u; }
}

// n <= 32 bits of what hr_png_refill has fetched; false when the stream ended first
HR_HD bool hr_png_take(hr_png_reader* r, uint32_t n, uint32_t* v)
{
    if (r->fill < n) return false;
    *v = (uint32_t)(r->acc & ((1ull << n) - 1ull));
    r->acc >>= n; r->fill -= n;
    return true;
}

// ---------------------------------------------------------------- tables
struct hr_png_inflate_mem {
    uint8_t win[HR_PNG_WINDOW];
    uint16_t lit[HR_PNG_LIT_TABLE], dist[HR_PNG_DIST_TABLE], cl[HR_PNG_CL_TABLE];
    uint32_t codes[320];
    uint16_t count[16];          // codes per length of the table being built
    uint16_t sub_bits[4];        // index bits of the sub-tables of lit, dist, cl (read only when a long code comes up)
    uint8_t lens[320];           // literal / length code lengths, the distance code's after them
    uint8_t stage[HR_PNG_STAGE];  // the reader's piece of the file (kernels only)
    hr_png_cold cold;
};

// The lookup table of the n code lengths `lens` (limit: 15, or 7 for the code-length code).  *sub_bits: index bits of every sub-table.
// HR_PNG_OK, or HR_PNG_E_CODE for a set zlib refuses.
HR_HD int hr_png_build_table(hr_png_inflate_mem* m, const uint8_t* lens, int n, int limit, int root, bool code_length_code, uint16_t* table,
                             int table_len, uint16_t* sub_bits_at, int lane, int lanes)
{
    HR_PNG_SYNC();                                            // lens and the table's last readers
    for (int k = lane; k < (lanes > 16 ? lanes : 16); k += lanes) {      // how many codes of b bits: a lane per length (lanes beyond 16 repeat)
        const int b = k & 15;
        uint32_t c = 0;
        for (int i = 0; i < n; ++i) c += lens[i] == b ? 1u : 0u;
        m->count[b] = (uint16_t)c;
    }
    for (int i = lane; i < table_len; i += lanes) table[i] = 0;
    HR_PNG_SYNC();
    int max = 0, left = 1;
    uint32_t p0 = 0;                                          // root entries that codes of root bits or fewer cover
    bool over = false;
    for (int b = 1; b <= limit; ++b) {
        const uint32_t c = HR_PNG_UNIFORM(m->count[b]);
        if (c) max = b;
        left = (left << 1) - (int)c;
        if (left < 0) { over = true; left = 0; }
        if (b <= root) p0 += c << (root - b);
    }
    const int sub_bits = max > root ? max - root : 0;
    *sub_bits_at = (uint16_t)sub_bits;                        // every lane the same value: no lane mask to keep
    if (max == 0) return HR_PNG_OK;                           // no code at all: any symbol read from it is refused
    if (over) return HR_PNG_E_CODE;                           // over-subscribed
    if (left > 0 && (code_length_code || max != 1)) return HR_PNG_E_CODE;      // incomplete, and not the single code of one bit
    hr_png_canonical(lens, n, limit, m->codes);               // every lane walks it and stores the same codes: serial either way, and no lane mask
    HR_PNG_SYNC();
    const uint32_t root_size = 1u << root, sub_size = 1u << sub_bits;
    for (int s = lane; s < n; s += lanes) {
        const uint32_t e = m->codes[s], l = e >> 16, r = e & 0xFFFFu;
        if (!l) continue;
        const uint16_t entry = (uint16_t)((uint32_t)s | (l << 9));
        if (l <= (uint32_t)root) {
            for (uint32_t k = r; k < root_size; k += 1u << l) table[k] = entry;
        } else {
            const uint32_t low = r & (root_size - 1u), sub = hr_png_bit_reverse(low, root) - p0, base = root_size + sub * sub_size;
            if (base + sub_size > (uint32_t)table_len) continue;     // cannot happen in a complete code; a write stays inside the table
            table[low] = (uint16_t)(HR_PNG_ENTRY_LINK | sub);
            for (uint32_t k = r >> root; k < sub_size; k += 1u << (l - (uint32_t)root)) table[base + k] = entry;
        }
    }
    HR_PNG_SYNC();
    return HR_PNG_OK;
}

// One symbol; the caller has refilled the bit buffer.  hr_png_refill leaves fewer than 48 bits only when the stream has ended -- no
// byte left in this IDAT chunk and no IDAT chunk after it -- and a turn of a loop uses at most 33 bits before its last code, so fewer
// than 15 bits here means exactly that: the missing bits are the stream's, and the status is TRUNCATED.  With 15 bits or more the
// table has seen every bit a code can have, and an unassigned entry is a bad code wherever in the stream it stands.
HR_HD int hr_png_symbol(hr_png_reader* r, const uint16_t* table, int root, const uint16_t* sub_bits_at, uint32_t* sym)
{
    const uint32_t bits = (uint32_t)r->acc;
    uint32_t e = HR_PNG_UNIFORM(table[bits & ((1u << root) - 1u)]);
    if (e & HR_PNG_ENTRY_LINK) {
        const uint32_t sub_bits = HR_PNG_UNIFORM(*sub_bits_at);
        e = HR_PNG_UNIFORM(table[(1u << root) + ((e & 0x7FFFu) << sub_bits) + ((bits >> root) & ((1u << sub_bits) - 1u))]);
    }
    const uint32_t l = e >> 9;
    if (l == 0 || l > r->fill) return (r->fill < 15u) ? HR_PNG_E_TRUNCATED : HR_PNG_E_CODE;
    r->acc >>= l; r->fill -= l;
    *sym = e & 511u;
    return HR_PNG_OK;
}

// ---------------------------------------------------------------- output: window, flush, Adler-32
// Positions are 32 bits (hr_png_shape_ok: 2^30 filtered bytes at most).  `done` bytes, a multiple of the piece, have been flushed; what
// lies between done and pos is still only in the window: less than a piece and a match, far from the 32 KB that may be overwritten.
struct hr_png_sink {
    uint8_t* win;                // HR_PNG_WINDOW bytes
    const hr_png_cold* cold;     // out: `total` filtered bytes, 4-byte aligned
    uint32_t total, pos, done;
    uint32_t a, b;               // Adler partial of the pieces flushed so far
    int lane, lanes;
};

// the n bytes from s->done on: a piece, or at the end what there is of one
HR_HD void hr_png_flush_piece(hr_png_sink* s, uint32_t n)
{
    HR_PNG_SYNC();
    const uint8_t* src = s->win + (s->done & (HR_PNG_WINDOW - 1u));
    uint8_t* dst = s->cold->out + s->done;
#if defined(__HIP_DEVICE_COMPILE__)
    for (uint32_t i = 4u * (uint32_t)s->lane; i < n; i += 4u * (uint32_t)s->lanes) {
        if (i + 4u <= n) *(uint32_t*)(dst + i) = *(const uint32_t*)(src + i);         // done is a multiple of the piece, out is aligned
        else for (uint32_t k = i; k < n; ++k) dst[k] = src[k];
    }
#else
    for (uint32_t i = (uint32_t)s->lane; i < n; i += (uint32_t)s->lanes) dst[i] = src[i];
#endif
    const uint32_t per = (n + (uint32_t)s->lanes - 1u) / (uint32_t)s->lanes;
    const uint32_t beg = (uint32_t)s->lane * per < n ? (uint32_t)s->lane * per : n, end = beg + per < n ? beg + per : n;
    uint32_t a, b, pa, pb;
    hr_adler_part(src + beg, end - beg, &a, &b);
    hr_adler_place(a, b, n - end, &pa, &pb);
    pa = hr_png_lanes_add(pa) % HR_PNG_ADLER_MOD;
    pb = hr_png_lanes_add(pb) % HR_PNG_ADLER_MOD;
    hr_adler_combine(s->a, s->b, pa, pb, n, &s->a, &s->b);
    s->done += n;
    HR_PNG_SYNC();
}

// Once per turn of a block's loop, the one place a piece is flushed: a turn adds 258 bytes at most, so one piece at most is due.
// at_end: what is left, too.
HR_HD void hr_png_drain(hr_png_sink* s, bool at_end)
{
    while (s->pos - s->done >= HR_PNG_PIECE || (at_end && s->pos > s->done)) {
        const uint32_t due = s->pos - s->done;
        hr_png_flush_piece(s, due < HR_PNG_PIECE ? due : HR_PNG_PIECE);
    }
}

HR_HD int hr_png_put_byte(hr_png_sink* s, uint32_t v)
{
    if (s->pos == s->total) return HR_PNG_E_TOO_LONG;
    s->win[s->pos & (HR_PNG_WINDOW - 1u)] = (uint8_t)v;      // every lane stores the same value to the same slot: no lane mask in the loop
    s->pos += 1u;
    return HR_PNG_OK;
}

// len 3..258 bytes from `dist` back:  byte pos + i = byte pos - dist + i % dist,  lanes taking i, so an overlapping match (dist <
// len) is one step: every source byte was there before the copy.  In the window the slots are taken modulo 32768, and for dist >
// 32768 - len a lane's source slot is the destination slot of another: index i reads slot pos - dist + i, which index i + (32768 -
// dist) writes.  The writer's index is the higher one, and the lanes of a wavefront do a step's loads before its stores and its
// steps of 64 indices in order, as the host's loop does index by index: every source is read before it is overwritten.
HR_HD int hr_png_put_match(hr_png_sink* s, uint32_t len, uint32_t dist)
{
    if (dist > s->pos) return HR_PNG_E_DISTANCE;
    if (len > s->total - s->pos) return HR_PNG_E_TOO_LONG;
    const uint32_t to = s->pos, from = to - dist;
    // i % dist for an overlapping match without a division per byte: with magic = ceil(2^17 / dist), (i * magic) >> 17 is i / dist
    // exactly while i * dist < 2^17, and here both are below 258
    const uint32_t magic = dist < len ? (131072u + dist - 1u) / dist : 0u;
    HR_PNG_SYNC();
    for (uint32_t i = (uint32_t)s->lane; i < len; i += (uint32_t)s->lanes)
        s->win[(to + i) & (HR_PNG_WINDOW - 1u)] = s->win[(from + i - ((i * magic) >> 17) * dist) & (HR_PNG_WINDOW - 1u)];
    s->pos += len;
    return HR_PNG_OK;
}

// length symbol 257..285 -> base length, via hr_png_length_ebits; distance symbol 0..29 -> base and extra bits (RFC 1951 3.2.5)
HR_HD uint32_t hr_png_length_base(uint32_t sym)
{
    if (sym < 265u) return sym - 254u;
    if (sym == 285u) return 258u;
    const uint32_t e = hr_png_length_ebits(sym);
    return 3u + (1u << (e + 2u)) + (((sym - 261u) & 3u) << e);
}
HR_HD uint32_t hr_png_dist_ebits(uint32_t sym) { return sym < 4u ? 0u : (sym >> 1) - 1u; }
HR_HD uint32_t hr_png_dist_base(uint32_t sym) { return sym < 4u ? sym + 1u : 1u + ((2u + (sym & 1u)) << hr_png_dist_ebits(sym)); }

// ---------------------------------------------------------------- inflate
// f[0..n): the file; idat_at: its first IDAT chunk; out: `total` = h * (1 + w * c) filtered bytes.
HR_HD int hr_png_inflate(const uint8_t* f, uint32_t n, uint32_t idat_at, uint8_t* out, uint32_t total, hr_png_inflate_mem* m, int lane, int lanes)
{
    static constexpr uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    m->cold.file = f; m->cold.out = out; m->cold.end = n;     // every lane stores the same values
    HR_PNG_SYNC();
    hr_png_reader r;
    hr_png_reader_init(&r, &m->cold, idat_at, m->stage, lane, lanes);
    hr_png_sink s;
    s.win = m->win; s.cold = &m->cold; s.total = total; s.pos = 0; s.done = 0; s.a = 0; s.b = 0; s.lane = lane; s.lanes = lanes;
    uint32_t v;
    hr_png_refill(&r);
    if (!hr_png_take(&r, 16, &v)) return HR_PNG_E_TRUNCATED;
    const uint32_t cmf = v & 255u, flg = v >> 8;
    if (((cmf << 8) | flg) % 31u || (cmf & 15u) != 8u || (cmf >> 4) > 7u || (flg & 0x20u)) return HR_PNG_E_ZLIB_HEADER;
    uint32_t final_block = 0;
    while (!final_block) {                                    // a block per turn: 3 bits or more
        hr_png_refill(&r);                                    // the block's header: 3 + 7 + 32 bits stored, 3 + 14 dynamic
        if (!hr_png_take(&r, 3, &v)) return HR_PNG_E_TRUNCATED;
        final_block = v & 1u;
        const uint32_t type = v >> 1;
        if (type == 3u) return HR_PNG_E_BLOCK;
        if (type == 0u) {
            hr_png_take(&r, r.fill & 7u, &v);                 // to the byte boundary: those bits are there
            if (!hr_png_take(&r, 32, &v)) return HR_PNG_E_TRUNCATED;
            const uint32_t len = v & 0xFFFFu;
            if ((len ^ (v >> 16)) != 0xFFFFu) return HR_PNG_E_BLOCK;
            for (uint32_t i = 0; i < len; ++i) {
                hr_png_drain(&s, false);
                hr_png_refill(&r);
                if (!hr_png_take(&r, 8, &v)) return HR_PNG_E_TRUNCATED;
                if (int st = hr_png_put_byte(&s, v)) return st;
            }
            continue;
        }
        int n_lit, n_dist;
        HR_PNG_SYNC();
        if (type == 1u) {
            n_lit = 288; n_dist = 32;
            for (int i = lane; i < 320; i += lanes) m->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
        } else {
            if (!hr_png_take(&r, 14, &v)) return HR_PNG_E_TRUNCATED;
            const uint32_t hclen = v >> 10;
            n_lit = (int)(v & 31u) + 257; n_dist = (int)((v >> 5) & 31u) + 1;
            if (n_lit > 286 || n_dist > 30) return HR_PNG_E_BLOCK;
            for (int i = lane; i < 64; i += lanes) m->lens[i] = 0;      // the code-length code's 19 lengths as a table of 64, 45 of them unused: whole wavefronts
            HR_PNG_SYNC();
            for (uint32_t i = 0; i < hclen + 4u; ++i) {
                hr_png_refill(&r);
                if (!hr_png_take(&r, 3, &v)) return HR_PNG_E_TRUNCATED;
                m->lens[order[i]] = (uint8_t)v;               // every lane stores the same value
            }
            if (int st = hr_png_build_table(m, m->lens, 64, 7, HR_PNG_CL_ROOT, true, m->cl, HR_PNG_CL_TABLE, m->sub_bits + 2, lane, lanes)) return st;
            int have = 0;
            uint32_t prev = 0, end_of_block_len = 0;
            while (have < n_lit + n_dist) {                   // a code-length symbol per turn: one bit or more
                uint32_t sym, rep = 1, val;
                hr_png_refill(&r);
                if (int st = hr_png_symbol(&r, m->cl, HR_PNG_CL_ROOT, m->sub_bits + 2, &sym)) return st;
                if (sym < 16u) val = sym;
                else {
                    const uint32_t eb = sym == 16u ? 2u : sym == 17u ? 3u : 7u;
                    if (!hr_png_take(&r, eb, &v)) return HR_PNG_E_TRUNCATED;
                    if (sym == 16u && have == 0) return HR_PNG_E_CODE;
                    val = sym == 16u ? prev : 0u;
                    rep = v + (sym == 18u ? 11u : 3u);
                    if (have + (int)rep > n_lit + n_dist) return HR_PNG_E_CODE;
                }
                for (uint32_t k = 0; k < rep; ++k) {
                    if (have == HR_PNG_EOB) end_of_block_len = val;
                    m->lens[have] = (uint8_t)val;
                    ++have;
                }
                prev = val;
            }
            if (end_of_block_len == 0) return HR_PNG_E_CODE;
        }
        if (int st = hr_png_build_table(m, m->lens, n_lit, 15, HR_PNG_LIT_ROOT, false, m->lit, HR_PNG_LIT_TABLE, m->sub_bits + 0, lane, lanes)) return st;
        if (int st = hr_png_build_table(m, m->lens + n_lit, n_dist, 15, HR_PNG_DIST_ROOT, false, m->dist, HR_PNG_DIST_TABLE, m->sub_bits + 1, lane, lanes)) return st;
        for (;;) {                                            // a symbol per turn: one bit or more
            uint32_t sym;
            hr_png_drain(&s, false);
            hr_png_refill(&r);
            if (int st = hr_png_symbol(&r, m->lit, HR_PNG_LIT_ROOT, m->sub_bits + 0, &sym)) return st;
            if (sym < 256u) {
                if (int st = hr_png_put_byte(&s, sym)) return st;
                continue;
            }
            if (sym == HR_PNG_EOB) break;
            if (sym >= (uint32_t)HR_PNG_LL) return HR_PNG_E_CODE;
            uint32_t len = hr_png_length_base(sym), dsym;
            if (!hr_png_take(&r, hr_png_length_ebits(sym), &v)) return HR_PNG_E_TRUNCATED;
            len += v;
            if (int st = hr_png_symbol(&r, m->dist, HR_PNG_DIST_ROOT, m->sub_bits + 1, &dsym)) return st;
            if (dsym >= 30u) return HR_PNG_E_CODE;
            if (!hr_png_take(&r, hr_png_dist_ebits(dsym), &v)) return HR_PNG_E_TRUNCATED;
            if (int st = hr_png_put_match(&s, len, hr_png_dist_base(dsym) + v)) return st;
        }
    }
    if (s.pos < total) return HR_PNG_E_TOO_SHORT;
    hr_png_drain(&s, true);
    hr_png_refill(&r);
    hr_png_take(&r, r.fill & 7u, &v);
    if (!hr_png_take(&r, 32, &v)) return HR_PNG_E_TRUNCATED;
    const uint32_t stored = (v << 24) | ((v & 0xFF00u) << 8) | ((v >> 8) & 0xFF00u) | (v >> 24);
    return stored == hr_adler_final(s.a, s.b, (uint64_t)total) ? HR_PNG_OK : HR_PNG_E_ADLER;
}

// ---------------------------------------------------------------- pixels
// One pixel of `bpp` bytes packed low byte first: filter f, x the filtered bytes, a left, b up, c upper left (zeros outside the image).
// hr_png_filter_byte(f, 0, ...) is minus the predictor.
HR_HD uint32_t hr_png_unfilter_pixel(int f, uint32_t x, uint32_t a, uint32_t b, uint32_t c, int bpp)
{
    uint32_t out = 0;
    HR_UNROLL
    for (int k = 0; k < 4; ++k) {
        if (k < bpp) {
            const int sh = 8 * k;
            const int v = ((int)((x >> sh) & 255u) - hr_png_filter_byte(f, 0, (int)((a >> sh) & 255u), (int)((b >> sh) & 255u), (int)((c >> sh) & 255u))) & 255;
            out |= (uint32_t)v << sh;
        }
    }
    return out;
}

// A pixel of `channels` (1 grey, 2 grey + alpha, 3 RGB, 4 RGBA) as out_channels (1 L, 3 RGB, 4 RGBA), packed the same way
HR_HD uint32_t hr_png_convert_pixel(uint32_t px, int channels, int out_channels)
{
    const bool grey = channels <= 2;
    const uint32_t r = px & 255u, g = grey ? r : (px >> 8) & 255u, b = grey ? r : (px >> 16) & 255u;
    const uint32_t alpha = channels == 2 ? (px >> 8) & 255u : channels == 4 ? px >> 24 : 255u;
    if (out_channels == 1) return grey ? r : (r * 19595u + g * 38470u + b * 7471u + 0x8000u) >> 16;
    return r | (g << 8) | (b << 16) | (out_channels == 4 ? alpha << 24 : 0u);
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------- the launch (png_decode_kernel.hip)
struct HrPngDecodeArgs {
    const uint8_t* files;        // the files, concatenated
    const int64_t* offsets;      // n_images + 1
    int64_t max_file_bytes;      // offsets lie in [0, max_file_bytes] and do not decrease, or the image is HR_PNG_E_OFFSETS
    int32_t w, h, n_images, out_channels;
    uint8_t* filtered;           // per image image_stride bytes: h * (1 + 4 w) at most, then a row of packed pixels (4 w)
    int64_t image_stride, carry_offset;
    int32_t* meta;               // per image HR_PNG_DEC_META_WORDS
    uint8_t* out;                // (n_images, h, w, out_channels)
    int32_t* status;
};
hipError_t hr_launch_png_decode(const HrPngDecodeArgs& a, hipStream_t stream);
#endif

#if !defined(__HIPCC__)
// ---------------------------------------------------------------- the whole file on the host
// What the three kernels do.  out: h * w * out_channels bytes for the expected size (expect_w, expect_h; -1, -1: the file's own, which
// hr_png_read_head gives beforehand).  Returns the status; when it is not HR_PNG_OK and the size is known, out is all zeros.
#include <vector>
static inline int32_t hr_png_decode_host_sized(const uint8_t* file, int64_t n, int32_t expect_w, int32_t expect_h, int32_t out_channels, uint8_t* out,
                                               hr_png_info* info)
{
    int64_t idat_at = 0;
    int st = hr_png_walk(file, n, expect_w, expect_h, info, &idat_at, 0, 1);
    const int64_t w = expect_w >= 0 ? expect_w : info->width, h = expect_w >= 0 ? expect_h : info->height;
    // a size the device decoder would not be created for (a hostile header asks for up to 2^62 bytes): refused, nothing is written
    if (w > 0 && h > 0 && (w > 0x7FFFFFFF || h > 0x7FFFFFFF || !hr_png_shape_ok((int32_t)w, (int32_t)h, 4))) return st != HR_PNG_OK ? st : HR_PNG_E_UNSUPPORTED;
    const size_t n_out = (size_t)w * (size_t)h * (size_t)out_channels;
    std::vector<uint8_t> filtered;
    if (st == HR_PNG_OK) {
        const int c = info->channels;
        const int64_t row_bytes = 1 + w * c;
        filtered.resize((size_t)(h * row_bytes));
        std::vector<hr_png_inflate_mem> mem(1);
        st = hr_png_inflate(file, (uint32_t)n, (uint32_t)idat_at, filtered.data(), (uint32_t)(h * row_bytes), mem.data(), 0, 1);
        for (int64_t y = 0; y < h && st == HR_PNG_OK; ++y)
            if (filtered[(size_t)(y * row_bytes)] > 4) st = HR_PNG_E_FILTER;
        if (st == HR_PNG_OK) {
            std::vector<uint32_t> above((size_t)w, 0u);
            for (int64_t y = 0; y < h; ++y) {
                const uint8_t* row = filtered.data() + y * row_bytes;
                uint32_t left = 0, up_left = 0;
                for (int64_t x = 0; x < w; ++x) {
                    uint32_t px = 0;
                    for (int k = 0; k < c; ++k) px |= (uint32_t)row[1 + x * c + k] << (8 * k);
                    const uint32_t up = above[(size_t)x], v = hr_png_unfilter_pixel(row[0], px, left, up, up_left, c);
                    up_left = up; left = v; above[(size_t)x] = v;
                    const uint32_t o = hr_png_convert_pixel(v, c, out_channels);
                    for (int k = 0; k < out_channels; ++k) out[((size_t)(y * w + x)) * (size_t)out_channels + k] = (uint8_t)(o >> (8 * k));
                }
            }
        }
    }
    if (st != HR_PNG_OK && w > 0 && h > 0) memset(out, 0, n_out);
    return st;
}

static inline int32_t hr_png_decode_host(const uint8_t* file, int64_t n, int32_t out_channels, uint8_t* out, hr_png_info* info)
{
    return hr_png_decode_host_sized(file, n, -1, -1, out_channels, out, info);
}
#endif

#endif  // HR_PNG_DECODE_H
