// TEST-ONLY probes into hyperreel_amd/csrc/hr_png.h (the arithmetic of a PNG file): the plan, the checksums' partials, the code lengths,
// to8b, the token rule and its slicing, so that the CPU suite can check them against zlib and numpy.  Whole files come from the product's
// host build of the same header (hyperreel_amd/csrc/png_host.cpp, hyperreel_amd/png.py), which the GPU suite compares the kernels with.
// With -DHR_PNG_STANDALONE the file is a program of its own: it encodes a list of shapes into buffers of exactly hr_png_bound bytes,
// for a sanitizer build (tests/test_png_host.py).
#include "../../hyperreel_amd/csrc/hr_png.h"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

extern "C" {

// out (8): rows_per_strip, n_strips, workspace_bytes, bound, row_bytes, strip_stride, the strip budget in bytes, 0
void hp_plan(int32_t w, int32_t h, int32_t channels, int64_t* out)
{
    const hr_png_plan_t p = hr_png_plan(w, h, channels);
    out[0] = p.rows_per_strip; out[1] = p.n_strips; out[2] = p.workspace_bytes; out[3] = p.bound; out[4] = p.row_bytes; out[5] = p.strip_stride;
    out[6] = HR_PNG_STRIP_BYTES; out[7] = 0;
}

uint32_t hp_crc0(const uint8_t* p, uint64_t len) { return hr_crc0(p, len); }
uint32_t hp_crc_shift(uint32_t crc, uint64_t n) { return hr_crc_shift(crc, n); }
uint32_t hp_crc_final(uint32_t crc0, uint64_t len) { return hr_crc_final(crc0, len); }

void hp_adler_part(const uint8_t* p, uint32_t len, uint32_t* a, uint32_t* b) { hr_adler_part(p, len, a, b); }
void hp_adler_combine(uint32_t a1, uint32_t b1, uint32_t a2, uint32_t b2, uint64_t len2, uint32_t* a, uint32_t* b)
{
    hr_adler_combine(a1, b1, a2, b2, len2, a, b);
}
uint32_t hp_adler_final(uint32_t a, uint32_t b, uint64_t len) { return hr_adler_final(a, b, len); }

// count[n] (n <= 286) -> len[n]: the sort by (count, index), then the length-limited construction
void hp_code_lengths(const uint32_t* count, int32_t n, int32_t limit, uint8_t* len)
{
    hr_png_huff_work wk;
    int m = 0;
    for (int i = 0; i < n; ++i)
        if (count[i]) { wk.sorted[hr_png_rank(count, n, i)] = (uint16_t)i; ++m; }
    hr_png_code_lengths(count, n, m, limit, len, &wk);
}

void hp_to8b(const float* x, int64_t n, uint8_t* out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = hr_to8b(x[i]);
}

// the tokens of n bytes cut into `slices` contiguous slices, joined as png_filter_kernel joins its threads' slices: a summary per slice,
// a Hillis-Steele scan of hr_png_run_join for the run reaching each slice, a walk forward for the run leaving it
void hp_tokens_sliced(const uint8_t* p, uint32_t n, int32_t slices, uint16_t* tok)
{
    std::vector<hr_png_segment> seg(slices);
    std::vector<uint32_t> run(slices), next(slices);
    const uint32_t per = (n + slices - 1) / slices;
    auto lo = [&](int t) { return (uint32_t)t * per < n ? (uint32_t)t * per : n; };
    for (int t = 0; t < slices; ++t) {
        seg[t] = hr_png_segment_scan(p + lo(t), lo(t + 1) - lo(t));
        run[t] = (seg[t].trail << 1) | (seg[t].len && seg[t].trail == seg[t].len ? 1u : 0u);
    }
    for (int off = 1; off < slices; off <<= 1) {
        for (int t = 0; t < slices; ++t) next[t] = t >= off ? hr_png_run_join(run[t], run[t - off], seg[t - off + 1].first == seg[t - off].last) : run[t];
        run = next;
    }
    for (int t = 0; t < slices; ++t) {
        if (!seg[t].len) continue;
        const uint32_t before = (t > 0 && seg[t - 1].last == seg[t].first) ? run[t - 1] >> 1 : 0u;
        uint32_t after = 0;
        for (int j = t + 1; j < slices && after < 258u && seg[j].len && seg[j].first == seg[t].last; ++j) {
            after += seg[j].lead;
            if (seg[j].lead != seg[j].len) break;
        }
        hr_png_segment_tokens(p + lo(t), seg[t].len, before, after, [&](uint32_t i, uint32_t token) { tok[lo(t) + i] = (uint16_t)token; });
    }
}

uint32_t hp_token(int32_t byte, uint32_t k, uint32_t follow) { return hr_png_token(byte, k, follow); }

}

#ifdef HR_PNG_STANDALONE
static uint32_t mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// one image: its file goes into a heap block of exactly hr_png_bound bytes, so that a byte too many is the sanitizer's to report
static int one(int32_t w, int32_t h, int32_t c, int content, int pixel_type, int filter_mode)
{
    const size_t n = (size_t)w * h * c;
    uint8_t* px8 = (uint8_t*)malloc(n);
    float* pxf = (float*)malloc(n * sizeof(float));
    for (size_t i = 0; i < n; ++i) {
        const size_t x = (i / c) % w, y = i / ((size_t)c * w);
        uint32_t v;
        if (content == 0) v = mix((uint32_t)i + 77u * (uint32_t)w) >> 24;              // noise: the stored fallback
        else if (content == 1) v = (uint32_t)((x * 3 + y * 2 + i % c) & 255);           // a ramp
        else if (content == 2) v = 255;                                                 // constant: long runs across rows
        else v = ((x - w / 2) * (x - w / 2) + (y - h / 2) * (y - h / 2) < (size_t)(w * h / 8 + 1)) ? mix((uint32_t)i) >> 26 : 255;
        px8[i] = (uint8_t)v;
        pxf[i] = (float)v / 255.0f;
    }
    const hr_png_plan_t p = hr_png_plan(w, h, c);
    uint8_t* file = (uint8_t*)malloc((size_t)p.bound);
    const int64_t len = hr_png_encode_host(pixel_type == HR_PNG_U8 ? (const void*)px8 : (const void*)pxf, pixel_type, filter_mode, w, h, c, file,
                                           p.bound, nullptr, nullptr, nullptr);
    const int bad = len < 57 || len > p.bound || file[len - 12 + 4] != 'I';
    if (bad) fprintf(stderr, "w %d h %d c %d content %d: length %lld, bound %lld\n", w, h, c, content, (long long)len, (long long)p.bound);
    free(file); free(pxf); free(px8);
    return bad;
}

int main()
{
    int bad = 0, count = 0;
    const int32_t chans[3] = {1, 3, 4};
    for (int ci = 0; ci < 3; ++ci) {
        const int32_t c = chans[ci];
        const int32_t rps = hr_png_plan(300, 1, c).rows_per_strip, wide = HR_PNG_STRIP_BYTES / c + 5;
        const int32_t shapes[][2] = {{1, 1}, {1, 7}, {7, 1}, {61, 47}, {64, 64}, {300, rps - 1}, {300, rps}, {300, rps + 1}, {300, 2 * rps + 1}, {wide, 2}};
        for (size_t s = 0; s < sizeof(shapes) / sizeof(shapes[0]); ++s)
            for (int content = 0; content < 4; ++content) {
                bad += one(shapes[s][0], shapes[s][1], c, content, (int)((s + content) & 1), content == 1 ? (int)(s % 5) : HR_PNG_FILTER_ADAPTIVE);
                ++count;
            }
    }
    printf("%d images, %d bad\n", count, bad);
    return bad ? 1 : 0;
}
#endif
