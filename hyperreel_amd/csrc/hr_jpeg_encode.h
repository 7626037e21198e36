// Pixels into a baseline JPEG file, byte for byte as PIL (libjpeg-turbo) writes it with optimize=False: stated once for the kernels of
// jpeg_encode_kernel.hip and, compiled by the host compiler, for hr_jpeg_encode_host (hyperreel_amd/csrc/jpeg_encode_host.cpp,
// tests/host_math/hr_jpeg_encode_host.cpp).  Integer arithmetic only, so both give the same bytes.  The zigzag order is
// hr_jpeg_decode.h's hr_jpeg_natural, the pixel read hr_png.h's hr_png_sample (to8b of a float frame, NaN giving 0), not restated.
//
//   file       SOI, APP0 JFIF 1.01 (units 0, density 1 x 1), one DQT per table, SOF0 (ids 1 2 3; luma 1x1 / 2x1 / 2x2, chroma 1x1; tables
//              0 1 1), DHT DC0 AC0 DC1 AC1 (grey: DC0 AC0), DRI with restart markers only, SOS (0..63, Ah/Al 0), the scan, EOI
//   tables     the standard Huffman tables of the JPEG standard's annex K; the quantisation tables are jpeg_set_quality's with forced
//              baseline: scale = 5000 / q below 50, else 200 - 2 q; entry = clamp((base * scale + 50) / 100, 1, 255)
//   colour     libjpeg's 16-bit fixed point RGB -> YCbCr (hr_jpeg_enc_ycc)
//   samples    hr_jpeg_enc_sample: a component's sample at (x, y) of its padded block grid.  Columns replicate the last input column; rows
//              replicate the last input row up to a multiple of vmax before downsampling and the last DOWNSAMPLED row after it; h2v1
//              (a + b + bias) >> 1 with bias 0 1 0 1 along the output row, h2v2 (a + b + c + d + bias) >> 2 with bias 1 2 1 2
//   blocks     hr_jpeg_fdct_pass: jpeg_fdct_islow on samples minus 128 (rows: even outputs << 2, the rest descaled by 11; columns: 2 and
//              15), then hr_jpeg_enc_quant: d = 8 q, (|c| + d / 2) / d with the sign put back.  Coefficients are kept in zigzag order
//   scan       grey: blocks in raster order; colour: interleaved MCUs of hs x vs luma blocks (rows first), Cb, Cr (hr_jpeg_enc_block_at).
//              A luma block of an MCU right of or below the component's blocks is a dummy: no AC, the DC of the block coded before it,
//              so its difference is 0 and the prediction chain passes over it (hr_jpeg_enc_pred)
//   entropy    hr_jpeg_enc_block_code: the DC difference's category code and magnitude bits (a negative value as v - 1), AC (run << 4 |
//              size) codes, F0 per 16 zeros, 00 when the block ends in zeros; most significant bit first (hr_jpeg_enc_bitw)
//   restarts   an interval is restart_rows MCU rows: its bits are padded to a byte with ones, FF D0+(k & 7) follows every interval but
//              the last, and every DC prediction starts from 0 again
//   stuffing   a 00 after every FF of the scan (the padded bytes too), never after a marker
//   bound      hr_jpeg_enc_plan's bound: per block the longest DC code and 63 times the longest AC code with their magnitude bits plus
//              an EOB, doubled for stuffing, plus the header, the markers and a pad byte per interval
#ifndef HR_JPEG_ENCODE_H
#define HR_JPEG_ENCODE_H

#include "hr_jpeg_decode.h"      // hr_jpeg_natural, HR_JPEG_LD; through it hr_png.h's hr_png_sample and HR_PNG_U8 / HR_PNG_F32_TO8B

#define HR_JPEG_ENC_HEAD_MAX 640      // SOI .. SOS of a colour file with DRI is 629 bytes
#define HR_JPEG_ENC_WG_BLOCKS 256     // blocks whose bit counts one workgroup scans
#define HR_JPEG_ENC_CHUNK 1024        // unstuffed bytes per workgroup of the stuffing passes
#define HR_JPEG_ENC_MAX_DIM 65535

struct hr_jpeg_enc_tables {
    uint16_t div[2][64];         // 8 * the quantisation table, zigzag order
    uint32_t dc[2][16];          // by category: length << 16 | code
    uint32_t ac[2][256];         // by (run << 4 | size)
    int32_t head_bytes;
    uint8_t head[HR_JPEG_ENC_HEAD_MAX];
};

struct hr_jpeg_enc_plan_t {
    int32_t w, h, channels, ncomp, hs, vs;
    int32_t mcux, mcuy, bpm, n_mcu, n_blocks;      // bpm: blocks per MCU, dummies included
    int32_t wb0, hb0;            // the luma (or grey) component's blocks
    int32_t rows_c;              // chroma rows after downsampling, before the replication to whole blocks
    int32_t ri, n_int;           // MCUs per restart interval (n_mcu without markers), intervals
    int32_t n_wg;                // workgroups of HR_JPEG_ENC_WG_BLOCKS blocks
    int32_t head_bytes;
    uint32_t max_block_bits;
    int64_t raw_max;             // most unstuffed scan bytes, the intervals' padding included
    int64_t n_chunks;            // of HR_JPEG_ENC_CHUNK bytes in raw_max
    int64_t off_tables, off_coef, off_local, off_wg, off_int_byte, off_int_bit, off_glob, off_raw, off_ff;      // byte offsets into the workspace
    int64_t workspace_bytes;
    int64_t bound;
};

// words of the workspace's globals
enum { HR_JPEG_ENC_G_RAW_BYTES = 0, HR_JPEG_ENC_G_WORDS = 4 };      // the unstuffed scan's bytes

// ---------------------------------------------------------------- the standard tables (counts per code length, symbols in code order)
HR_HD const uint8_t* hr_jpeg_enc_std_counts(int ac, int t)
{
    static const uint8_t c[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                     {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
    return c[ac * 2 + t];
}

HR_HD const uint8_t* hr_jpeg_enc_std_vals(int ac, int t, int* n)
{
    static const uint8_t dc[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    static const uint8_t ac0[162] = {
        1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,   35,  66,  177,
        193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,  41,  42,  52,  53,  54,  55,
        56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106,
        115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
        164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211,
        212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250};
    static const uint8_t ac1[162] = {
        0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145, 161, 177, 193,
        9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,  39,  40,  41,  42,  53,  54,
        55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105,
        106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
        162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
        210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250};
    *n = ac ? 162 : 12;
    return ac ? (t ? ac1 : ac0) : dc;
}

// libjpeg's base tables (quality 50) in zigzag order, as a DQT segment holds them
HR_HD const uint8_t* hr_jpeg_enc_base_table(int t)
{
    static const uint8_t q[2][64] = {
        {16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24,  40, 26, 24, 22, 22, 24, 49,  35,  37,  29,  40,  58,  51,  61,  60, 57,  51,
         56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99},
        {17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
    return q[t];
}

HR_HD int hr_jpeg_enc_quant_entry(int base, int quality)
{
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int v = (base * scale + 50) / 100;
    return v < 1 ? 1 : v > 255 ? 255 : v;
}

// by symbol: length << 16 | code, 0 for a symbol the table does not have
HR_HD void hr_jpeg_enc_codes(int ac, int t, uint32_t* out, int n_out)
{
    int n = 0;
    const uint8_t* counts = hr_jpeg_enc_std_counts(ac, t);
    const uint8_t* vals = hr_jpeg_enc_std_vals(ac, t, &n);
    for (int i = 0; i < n_out; ++i) out[i] = 0;
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < counts[l - 1]; ++i, ++k, ++code)
            if (vals[k] < n_out) out[vals[k]] = ((uint32_t)l << 16) | code;
        code <<= 1;
    }
}

// the most bits a block can take: the longest DC code with its magnitude bits, 63 times the longest AC code with its, and an EOB
HR_HD uint32_t hr_jpeg_enc_max_block_bits()
{
    uint32_t tab[256], dc = 0, ac = 0, eob = 0;
    for (int t = 0; t < 2; ++t) {
        hr_jpeg_enc_codes(0, t, tab, 16);
        for (uint32_t s = 0; s < 12; ++s)
            if (tab[s] && (tab[s] >> 16) + s > dc) dc = (tab[s] >> 16) + s;
        hr_jpeg_enc_codes(1, t, tab, 256);
        for (uint32_t s = 0; s < 256; ++s)
            if (tab[s] && (tab[s] >> 16) + (s & 15u) > ac) ac = (tab[s] >> 16) + (s & 15u);
        if ((tab[0] >> 16) > eob) eob = tab[0] >> 16;
    }
    return dc + 63u * ac + eob;
}

// ---------------------------------------------------------------- the plan
// NULL when the encoders take the shape, else why not.  subsampling: 0 4:4:4, 1 4:2:2, 2 4:2:0 (PIL's numbers)
HR_HD const char* hr_jpeg_enc_refusal(int32_t w, int32_t h, int32_t channels, int32_t quality, int32_t subsampling, int32_t restart_rows)
{
    if (w < 1 || h < 1 || w > HR_JPEG_ENC_MAX_DIM || h > HR_JPEG_ENC_MAX_DIM) return "the size must be 1 x 1 to 65535 x 65535";
    if (channels != 1 && channels != 3 && channels != 4) return "channels is not 1 (grey), 3 (RGB) or 4 (RGBA, alpha ignored)";
    if (quality < 1 || quality > 100) return "quality is outside 1..100";
    if (subsampling < 0 || subsampling > 2) return "unknown subsampling (0: 4:4:4, 1: 4:2:2, 2: 4:2:0)";
    if (channels == 1 && subsampling != 0) return "a grey image has no subsampling other than 4:4:4 (0)";
    if (restart_rows < 0) return "restart_rows is negative";
    const int hs = subsampling ? 2 : 1, vs = subsampling == 2 ? 2 : 1;
    const int64_t mcux = (w + 8 * hs - 1) / (8 * hs), mcuy = (h + 8 * vs - 1) / (8 * vs);
    if ((int64_t)restart_rows * mcux > 65535) return "restart_rows MCU rows are more than the 65535 MCUs a DRI segment can hold";
    const int64_t blocks = mcux * mcuy * (channels == 1 ? 1 : hs * vs + 2);
    if (blocks * hr_jpeg_enc_max_block_bits() >= (1ll << 32)) return "the image has more blocks than 32-bit bit offsets can address";
    return nullptr;
}

// of a shape hr_jpeg_enc_refusal passes
HR_HD hr_jpeg_enc_plan_t hr_jpeg_enc_plan(int32_t w, int32_t h, int32_t channels, int32_t subsampling, int32_t restart_rows)
{
    hr_jpeg_enc_plan_t p;
    p.w = w; p.h = h; p.channels = channels;
    p.ncomp = channels == 1 ? 1 : 3;
    p.hs = subsampling ? 2 : 1;
    p.vs = subsampling == 2 ? 2 : 1;
    p.mcux = (w + 8 * p.hs - 1) / (8 * p.hs);
    p.mcuy = (h + 8 * p.vs - 1) / (8 * p.vs);
    p.bpm = p.ncomp == 1 ? 1 : p.hs * p.vs + 2;
    p.n_mcu = p.mcux * p.mcuy;
    p.n_blocks = p.n_mcu * p.bpm;
    p.wb0 = (w + 7) / 8;
    p.hb0 = (h + 7) / 8;
    p.rows_c = (h + p.vs - 1) / p.vs;
    p.ri = restart_rows > 0 ? restart_rows * p.mcux : p.n_mcu;
    p.n_int = (p.n_mcu + p.ri - 1) / p.ri;
    p.n_wg = (p.n_blocks + HR_JPEG_ENC_WG_BLOCKS - 1) / HR_JPEG_ENC_WG_BLOCKS;
    const int nc = p.ncomp;
    p.head_bytes = 2 + 18 + 69 * (nc == 1 ? 1 : 2) + (10 + 3 * nc) + (33 + 183) * (nc == 1 ? 1 : 2) + (restart_rows > 0 ? 6 : 0) + (8 + 2 * nc);
    p.max_block_bits = hr_jpeg_enc_max_block_bits();
    p.raw_max = ((int64_t)p.n_blocks * p.max_block_bits + 7) / 8 + p.n_int;
    p.n_chunks = (p.raw_max + HR_JPEG_ENC_CHUNK - 1) / HR_JPEG_ENC_CHUNK;
    int64_t at = 0;
    auto take = [&](int64_t bytes) { const int64_t o = at; at += (bytes + 15) / 16 * 16; return o; };
    p.off_tables = take((int64_t)sizeof(hr_jpeg_enc_tables));
    p.off_coef = take((int64_t)p.n_blocks * 128);
    p.off_local = take((int64_t)p.n_blocks * 4);
    p.off_wg = take((int64_t)p.n_wg * 4);
    p.off_int_byte = take(((int64_t)p.n_int + 1) * 4);
    p.off_int_bit = take(((int64_t)p.n_int + 1) * 4);
    p.off_glob = take(HR_JPEG_ENC_G_WORDS * 4);
    p.off_raw = take(p.n_chunks * HR_JPEG_ENC_CHUNK + 64);
    p.off_ff = take(p.n_chunks * 4);
    p.workspace_bytes = at;
    p.bound = p.head_bytes + 2 * p.raw_max + 2 * (int64_t)(p.n_int - 1) + 2;
    return p;
}

// ---------------------------------------------------------------- the scan's order
struct hr_jpeg_enc_block {
    int32_t mcu, j, comp, bx, by, dummy;
};

HR_HD hr_jpeg_enc_block hr_jpeg_enc_block_at(const hr_jpeg_enc_plan_t& p, int32_t b)
{
    hr_jpeg_enc_block k;
    k.mcu = b / p.bpm;
    k.j = b - k.mcu * p.bpm;
    const int32_t my = k.mcu / p.mcux, mx = k.mcu - my * p.mcux, nl = p.hs * p.vs;
    if (p.ncomp == 1 || k.j < nl) {
        k.comp = 0;
        k.bx = p.ncomp == 1 ? mx : mx * p.hs + k.j % p.hs;
        k.by = p.ncomp == 1 ? my : my * p.vs + k.j / p.hs;
        k.dummy = k.bx >= p.wb0 || k.by >= p.hb0;
    } else {
        k.comp = 1 + k.j - nl;
        k.bx = mx; k.by = my; k.dummy = 0;
    }
    return k;
}

// the block whose DC predicts block b's (b not a dummy), -1 where the prediction is 0: the component's block coded before it that is no
// dummy, within the restart interval.  An MCU's first luma block is never a dummy, so the walk back ends inside one MCU.
HR_HD int32_t hr_jpeg_enc_pred(const hr_jpeg_enc_plan_t& p, int32_t b, const hr_jpeg_enc_block& k)
{
    const bool first = k.mcu % p.ri == 0;
    if (k.comp > 0) return first ? -1 : b - p.bpm;
    int32_t q = b - 1;
    if (k.j == 0) {
        if (first) return -1;
        q = b - p.bpm + p.hs * p.vs - 1;
    }
    while (hr_jpeg_enc_block_at(p, q).dummy) --q;
    return q;
}

// ---------------------------------------------------------------- pixels to samples
HR_HD int hr_jpeg_enc_ycc(int comp, int r, int g, int b)
{
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// component `comp` of the input pixel (x, y), both inside the image
HR_FN int hr_jpeg_enc_pixel(const void* px, int pixel_type, const hr_jpeg_enc_plan_t& p, int comp, int x, int y)
{
    const int64_t at = ((int64_t)y * p.w + x) * p.channels;
    if (p.ncomp == 1) return hr_png_sample(px, pixel_type, at);
    return hr_jpeg_enc_ycc(comp, hr_png_sample(px, pixel_type, at), hr_png_sample(px, pixel_type, at + 1), hr_png_sample(px, pixel_type, at + 2));
}

// the sample (x, y) of component `comp` on its grid of whole blocks
HR_FN int hr_jpeg_enc_sample(const void* px, int pixel_type, const hr_jpeg_enc_plan_t& p, int comp, int x, int y)
{
    const int fx = comp ? p.hs : 1, fy = comp ? p.vs : 1;
    if (fx == 1 && fy == 1) return hr_jpeg_enc_pixel(px, pixel_type, p, comp, x < p.w ? x : p.w - 1, y < p.h ? y : p.h - 1);
    if (y >= p.rows_c) y = p.rows_c - 1;
    int sum = 0;
    for (int dy = 0; dy < fy; ++dy)
        for (int dx = 0; dx < 2; ++dx) {
            const int xx = 2 * x + dx, yy = fy * y + dy;
            sum += hr_jpeg_enc_pixel(px, pixel_type, p, comp, xx < p.w ? xx : p.w - 1, yy < p.h ? yy : p.h - 1);
        }
    return fy == 1 ? (sum + (x & 1)) >> 1 : (sum + 1 + (x & 1)) >> 2;
}

// ---------------------------------------------------------------- blocks
HR_HD int32_t hr_jpeg_enc_descale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of jpeg_fdct_islow over eight values in place: pass 0 the rows (of samples minus 128), pass 1 the columns
HR_HD void hr_jpeg_fdct_pass(int32_t* d, int pass)
{
    const int32_t t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int32_t t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int n = pass ? 15 : 11;
    if (pass) {
        d[0] = hr_jpeg_enc_descale(t10 + t11, 2);
        d[4] = hr_jpeg_enc_descale(t10 - t11, 2);
    } else {
        d[0] = (t10 + t11) * 4;
        d[4] = (t10 - t11) * 4;
    }
    int32_t z1 = (t12 + t13) * 4433;
    d[2] = hr_jpeg_enc_descale(z1 + t13 * 6270, n);
    d[6] = hr_jpeg_enc_descale(z1 - t12 * 15137, n);
    z1 = t4 + t7;
    int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int32_t z5 = (z3 + z4) * 9633;
    const int32_t a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    d[7] = hr_jpeg_enc_descale(a4 + z1 + z3, n);
    d[5] = hr_jpeg_enc_descale(a5 + z2 + z4, n);
    d[3] = hr_jpeg_enc_descale(a6 + z2 + z3, n);
    d[1] = hr_jpeg_enc_descale(a7 + z1 + z4, n);
}

// div = 8 * the table's entry
HR_HD int32_t hr_jpeg_enc_quant(int32_t c, int32_t div)
{
    const int32_t a = c < 0 ? -c : c, v = (a + (div >> 1)) / div;
    return c < 0 ? -v : v;
}

// ---------------------------------------------------------------- bits
HR_HD int hr_jpeg_enc_nbits(uint32_t a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return 32 - __clz((int)a);
#else
    return a ? 32 - __builtin_clz(a) : 0;
#endif
}

HR_HD uint32_t hr_jpeg_enc_bswap(uint32_t v) { return __builtin_bswap32(v); }

// Bits, most significant first, OR-ed into 32-bit words that were cleared beforehand: blocks that share a word add to it in any order.
struct hr_jpeg_enc_bitw {
    uint32_t* words;
    uint32_t word;
    uint64_t acc;
    int n;
};

HR_FN void hr_jpeg_enc_or(uint32_t* w, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (v) atomicOr(w, v);
#else
    *w |= v;
#endif
}

HR_FN void hr_jpeg_enc_bitw_init(hr_jpeg_enc_bitw* s, uint32_t* words, uint32_t bit)
{
    s->words = words; s->word = bit >> 5; s->n = (int)(bit & 31u); s->acc = 0;
}

// len 1..27
HR_FN void hr_jpeg_enc_bitw_put(hr_jpeg_enc_bitw* s, uint32_t v, int len)
{
    s->acc |= (uint64_t)v << (64 - s->n - len);
    s->n += len;
    if (s->n >= 32) {
        hr_jpeg_enc_or(s->words + s->word, hr_jpeg_enc_bswap((uint32_t)(s->acc >> 32)));
        s->acc <<= 32; s->n -= 32; ++s->word;
    }
}

HR_FN void hr_jpeg_enc_bitw_flush(hr_jpeg_enc_bitw* s)
{
    if (s->n) hr_jpeg_enc_or(s->words + s->word, hr_jpeg_enc_bswap((uint32_t)(s->acc >> 32)));
}

// A block's codes, each handed to sink(value, length, symbol, is_dc): c the 64 coefficients in zigzag order (not read for a dummy), diff
// the DC difference.  dc / ac: the component's tables.
template <class Sink>
HR_FN void hr_jpeg_enc_block_code(const uint32_t* dc, const uint32_t* ac, const int16_t* c, int32_t diff, bool dummy, Sink&& sink)
{
    {
        const int32_t a = diff < 0 ? -diff : diff, low = diff < 0 ? diff - 1 : diff;
        const int nb = hr_jpeg_enc_nbits((uint32_t)a);
        const uint32_t e = dc[nb];
        sink(((e & 0xFFFFu) << nb) | ((uint32_t)low & ((1u << nb) - 1u)), (int)(e >> 16) + nb, nb, true);
    }
    int run = 0;
    if (dummy) run = 63;
    else
        for (int k = 1; k < 64; ++k) {
            const int32_t v = c[k];
            if (v == 0) { ++run; continue; }
            while (run > 15) { sink(ac[0xF0] & 0xFFFFu, (int)(ac[0xF0] >> 16), 0xF0, false); run -= 16; }
            const int32_t a = v < 0 ? -v : v, low = v < 0 ? v - 1 : v;
            const int nb = hr_jpeg_enc_nbits((uint32_t)a), sym = (run << 4) | nb;
            const uint32_t e = ac[sym & 255];
            sink(((e & 0xFFFFu) << nb) | ((uint32_t)low & ((1u << nb) - 1u)), (int)(e >> 16) + nb, sym, false);
            run = 0;
        }
    if (run > 0) sink(ac[0] & 0xFFFFu, (int)(ac[0] >> 16), 0, false);
}

// the DC difference of block b: coef holds every real block's coefficients
HR_FN int32_t hr_jpeg_enc_dc_diff(const hr_jpeg_enc_plan_t& p, const int16_t* coef, int32_t b, const hr_jpeg_enc_block& k)
{
    if (k.dummy) return 0;
    const int32_t q = hr_jpeg_enc_pred(p, b, k);
    return (int32_t)coef[(int64_t)b * 64] - (q < 0 ? 0 : (int32_t)coef[(int64_t)q * 64]);
}

// ---------------------------------------------------------------- host only: the tables and the header of a file
static inline uint8_t* hr_jpeg_enc_segment(uint8_t* o, int marker, int payload)
{
    o[0] = 0xFF; o[1] = (uint8_t)marker; o[2] = (uint8_t)((payload + 2) >> 8); o[3] = (uint8_t)((payload + 2) & 255);
    return o + 4;
}

static inline void hr_jpeg_enc_tables_build(const hr_jpeg_enc_plan_t& p, int quality, int restart_rows, hr_jpeg_enc_tables* t)
{
    const int nt = p.ncomp == 1 ? 1 : 2;
    uint8_t qt[2][64];
    for (int i = 0; i < 2; ++i) {
        for (int k = 0; k < 64; ++k) {
            qt[i][k] = (uint8_t)hr_jpeg_enc_quant_entry(hr_jpeg_enc_base_table(i)[k], quality);
            t->div[i][k] = (uint16_t)(8 * qt[i][k]);
        }
        hr_jpeg_enc_codes(0, i, t->dc[i], 16);
        hr_jpeg_enc_codes(1, i, t->ac[i], 256);
    }
    for (int i = 0; i < HR_JPEG_ENC_HEAD_MAX; ++i) t->head[i] = 0;
    uint8_t* o = t->head;
    *o++ = 0xFF; *o++ = 0xD8;
    o = hr_jpeg_enc_segment(o, 0xE0, 14);
    const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (int i = 0; i < 14; ++i) *o++ = jfif[i];
    for (int i = 0; i < nt; ++i) {
        o = hr_jpeg_enc_segment(o, 0xDB, 65);
        *o++ = (uint8_t)i;
        for (int k = 0; k < 64; ++k) *o++ = qt[i][k];
    }
    o = hr_jpeg_enc_segment(o, 0xC0, 6 + 3 * p.ncomp);
    *o++ = 8; *o++ = (uint8_t)(p.h >> 8); *o++ = (uint8_t)(p.h & 255); *o++ = (uint8_t)(p.w >> 8); *o++ = (uint8_t)(p.w & 255); *o++ = (uint8_t)p.ncomp;
    for (int i = 0; i < p.ncomp; ++i) {
        *o++ = (uint8_t)(i + 1);
        *o++ = (uint8_t)(i == 0 && p.ncomp == 3 ? (p.hs << 4) | p.vs : 0x11);
        *o++ = (uint8_t)(i ? 1 : 0);
    }
    for (int i = 0; i < nt; ++i)
        for (int ac = 0; ac < 2; ++ac) {
            int n = 0;
            const uint8_t* vals = hr_jpeg_enc_std_vals(ac, i, &n);
            o = hr_jpeg_enc_segment(o, 0xC4, 17 + n);
            *o++ = (uint8_t)((ac << 4) | i);
            for (int k = 0; k < 16; ++k) *o++ = hr_jpeg_enc_std_counts(ac, i)[k];
            for (int k = 0; k < n; ++k) *o++ = vals[k];
        }
    if (restart_rows > 0) {
        o = hr_jpeg_enc_segment(o, 0xDD, 2);
        *o++ = (uint8_t)(p.ri >> 8); *o++ = (uint8_t)(p.ri & 255);
    }
    o = hr_jpeg_enc_segment(o, 0xDA, 4 + 2 * p.ncomp);
    *o++ = (uint8_t)p.ncomp;
    for (int i = 0; i < p.ncomp; ++i) { *o++ = (uint8_t)(i + 1); *o++ = (uint8_t)(i ? 0x11 : 0x00); }
    *o++ = 0; *o++ = 63; *o++ = 0;
    t->head_bytes = (int32_t)(o - t->head);      // == p.head_bytes
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------- the launch (jpeg_encode_kernel.hip)
struct HrJpegEncArgs {
    const void* pixels;          // (h, w, channels): bytes or floats
    int32_t pixel_type;
    hr_jpeg_enc_plan_t plan;
    uint8_t* workspace;          // plan.workspace_bytes, 16-byte aligned, the tables at plan.off_tables
    uint8_t* file;               // plan.bound bytes or more
    int64_t* file_bytes;
};
hipError_t hr_launch_jpeg_encode(const HrJpegEncArgs& a, hipStream_t stream);
#endif

#if !defined(__HIPCC__)
// ---------------------------------------------------------------- the whole file on the host
#include <vector>
// what the fixtures are chosen by: stuffed bytes, F0 codes, the largest DC and AC category of the scan
struct hr_jpeg_enc_stats {
    int64_t stuffed, zrl;
    int32_t max_dc_cat, max_ac_cat;
};

// a block's 64 coefficients in zigzag order: what the block kernel's eight lanes do together
static inline void hr_jpeg_enc_block_coefs(const void* px, int pixel_type, const hr_jpeg_enc_plan_t& p, const uint16_t* div, const hr_jpeg_enc_block& k,
                                           int16_t* out)
{
    int32_t ws[64], col[8];
    for (int r = 0; r < 8; ++r) {
        for (int c = 0; c < 8; ++c) ws[r * 8 + c] = hr_jpeg_enc_sample(px, pixel_type, p, k.comp, k.bx * 8 + c, k.by * 8 + r) - 128;
        hr_jpeg_fdct_pass(ws + r * 8, 0);
    }
    for (int c = 0; c < 8; ++c) {
        for (int r = 0; r < 8; ++r) col[r] = ws[r * 8 + c];
        hr_jpeg_fdct_pass(col, 1);
        for (int r = 0; r < 8; ++r) ws[r * 8 + c] = col[r];
    }
    for (int z = 0; z < 64; ++z) out[z] = (int16_t)hr_jpeg_enc_quant(ws[hr_jpeg_natural(z)], div[z]);
}

// Returns the file's length, or -1 for arguments hr_jpeg_enc_refusal names or a capacity below the bound.  coef_out (n_blocks * 64
// int16, dummies zero) and stats may be NULL.
static inline int64_t hr_jpeg_encode_host(const void* pixels, int pixel_type, int32_t w, int32_t h, int32_t channels, int32_t quality, int32_t subsampling,
                                          int32_t restart_rows, uint8_t* file, int64_t capacity, int16_t* coef_out, hr_jpeg_enc_stats* stats)
{
    if (hr_jpeg_enc_refusal(w, h, channels, quality, subsampling, restart_rows)) return -1;
    if (pixel_type != HR_PNG_U8 && pixel_type != HR_PNG_F32_TO8B) return -1;
    const hr_jpeg_enc_plan_t p = hr_jpeg_enc_plan(w, h, channels, subsampling, restart_rows);
    if (capacity < p.bound) return -1;
    std::vector<hr_jpeg_enc_tables> tv(1);
    hr_jpeg_enc_tables& t = tv[0];
    hr_jpeg_enc_tables_build(p, quality, restart_rows, &t);
    if (t.head_bytes != p.head_bytes) return -1;
    std::vector<int16_t> coef((size_t)p.n_blocks * 64, 0);
    std::vector<uint32_t> start((size_t)p.n_blocks + 1, 0);
    // kernel 1: coefficients
    for (int32_t b = 0; b < p.n_blocks; ++b) {
        const hr_jpeg_enc_block k = hr_jpeg_enc_block_at(p, b);
        if (!k.dummy) hr_jpeg_enc_block_coefs(pixels, pixel_type, p, t.div[k.comp ? 1 : 0], k, coef.data() + (size_t)b * 64);
    }
    if (coef_out) memcpy(coef_out, coef.data(), coef.size() * 2);
    hr_jpeg_enc_stats st = {0, 0, 0, 0};
    // kernels 2 and 3: bit counts, their prefix sums, the intervals' byte offsets
    for (int32_t b = 0; b < p.n_blocks; ++b) {
        const hr_jpeg_enc_block k = hr_jpeg_enc_block_at(p, b);
        const int ti = k.comp ? 1 : 0;
        uint32_t bits = 0;
        hr_jpeg_enc_block_code(t.dc[ti], t.ac[ti], coef.data() + (size_t)b * 64, hr_jpeg_enc_dc_diff(p, coef.data(), b, k), k.dummy != 0,
                               [&](uint32_t, int len, int sym, bool dc) {
                                   bits += (uint32_t)len;
                                   if (dc && sym > st.max_dc_cat) st.max_dc_cat = sym;
                                   if (!dc && (sym & 15) > st.max_ac_cat) st.max_ac_cat = sym & 15;
                                   if (!dc && sym == 0xF0) ++st.zrl;
                               });
        start[b + 1] = start[b] + bits;
    }
    std::vector<uint32_t> ibyte((size_t)p.n_int + 1, 0);
    for (int32_t i = 0; i < p.n_int; ++i) {
        const int64_t b0 = (int64_t)i * p.ri * p.bpm, m1 = (int64_t)(i + 1) * p.ri;
        const int64_t b1 = (m1 < p.n_mcu ? m1 : p.n_mcu) * p.bpm;
        ibyte[i + 1] = ibyte[i] + (start[b1] - start[b0] + 7) / 8;
    }
    // kernels 4 and 5: the unstuffed scan
    const uint32_t raw_bytes = ibyte[p.n_int];
    std::vector<uint32_t> raw(raw_bytes / 4 + 2, 0);
    for (int32_t b = 0; b < p.n_blocks; ++b) {
        const hr_jpeg_enc_block k = hr_jpeg_enc_block_at(p, b);
        const int ti = k.comp ? 1 : 0;
        const int32_t i = k.mcu / p.ri;
        const uint32_t at = ibyte[i] * 8u + (start[b] - start[(int64_t)i * p.ri * p.bpm]);
        hr_jpeg_enc_bitw bw;
        hr_jpeg_enc_bitw_init(&bw, raw.data(), at);
        uint32_t bits = 0;
        hr_jpeg_enc_block_code(t.dc[ti], t.ac[ti], coef.data() + (size_t)b * 64, hr_jpeg_enc_dc_diff(p, coef.data(), b, k), k.dummy != 0,
                               [&](uint32_t v, int len, int, bool) { hr_jpeg_enc_bitw_put(&bw, v, len); bits += (uint32_t)len; });
        const bool last = k.j == p.bpm - 1 && (k.mcu == p.n_mcu - 1 || (k.mcu + 1) % p.ri == 0);
        const int pad = (int)((8u - ((at + bits) & 7u)) & 7u);
        if (last && pad) hr_jpeg_enc_bitw_put(&bw, (1u << pad) - 1u, pad);
        hr_jpeg_enc_bitw_flush(&bw);
    }
    // kernels 6 to 8: the header, the stuffed scan with its markers, EOI
    memcpy(file, t.head, (size_t)t.head_bytes);
    int64_t o = t.head_bytes;
    const uint8_t* rb = (const uint8_t*)raw.data();
    for (int32_t i = 0; i < p.n_int; ++i) {
        for (uint32_t q = ibyte[i]; q < ibyte[i + 1]; ++q) {
            file[o++] = rb[q];
            if (rb[q] == 0xFF) { file[o++] = 0; ++st.stuffed; }
        }
        if (i < p.n_int - 1) { file[o++] = 0xFF; file[o++] = (uint8_t)(0xD0 + (i & 7)); }
    }
    file[o++] = 0xFF; file[o++] = 0xD9;
    if (stats) *stats = st;
    return o;
}
#endif

#endif
