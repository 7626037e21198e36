// Host build of hyperreel_amd/csrc/hr_jpeg_encode.h for the test-suite: probes into the header's parts (the FDCT, the quantiser, the plan)
// for tests/test_jpeg_encode_host.py, and a main of its own for the stand-alone sanitizer run: it encodes generated images of every mode
// from heap blocks of exactly the image's size into heap blocks of exactly the bound, so that a read or a write outside either is seen.
#include "../../hyperreel_amd/csrc/hr_jpeg_encode.h"

#include <stdio.h>
#include <stdlib.h>

extern "C" {

// jpeg_fdct_islow as the block kernel runs it: 64 samples 0..255 in, 64 coefficients (natural order, scaled by 8) out
void hje_fdct(const int32_t* samples, int32_t* out)
{
    int32_t ws[64], col[8];
    for (int r = 0; r < 8; ++r) {
        for (int c = 0; c < 8; ++c) ws[r * 8 + c] = samples[r * 8 + c] - 128;
        hr_jpeg_fdct_pass(ws + r * 8, 0);
    }
    for (int c = 0; c < 8; ++c) {
        for (int r = 0; r < 8; ++r) col[r] = ws[r * 8 + c];
        hr_jpeg_fdct_pass(col, 1);
        for (int r = 0; r < 8; ++r) out[r * 8 + c] = col[r];
    }
}

void hje_quant_many(const int32_t* c, int32_t n, int32_t div, int32_t* out)
{
    for (int32_t i = 0; i < n; ++i) out[i] = hr_jpeg_enc_quant(c[i], div);
}

int32_t hje_quant_entry(int32_t base, int32_t quality) { return hr_jpeg_enc_quant_entry(base, quality); }

uint32_t hje_max_block_bits(void) { return hr_jpeg_enc_max_block_bits(); }

// n_blocks, n_int, n_wg, head_bytes, raw_max, bound of a shape the encoders take
void hje_plan(int32_t w, int32_t h, int32_t channels, int32_t subsampling, int32_t restart_rows, int64_t* out)
{
    const hr_jpeg_enc_plan_t p = hr_jpeg_enc_plan(w, h, channels, subsampling, restart_rows);
    out[0] = p.n_blocks; out[1] = p.n_int; out[2] = p.n_wg; out[3] = p.head_bytes; out[4] = p.raw_max; out[5] = p.bound;
}

}

static uint32_t lcg(uint32_t* s) { *s = *s * 1664525u + 1013904223u; return *s >> 8; }

int main(int argc, char** argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 1;
    const int sizes[][2] = {{1, 1}, {3, 3}, {8, 8}, {9, 7}, {7, 9}, {16, 16}, {17, 17}, {33, 15}, {15, 33}, {40, 24}, {2, 70}, {70, 2}, {136, 40}};
    const int qualities[] = {1, 50, 90, 100};
    uint32_t seed = 2026;
    long images = 0, bad = 0;
    for (int round = 0; round < rounds; ++round)
        for (const auto& wh : sizes)
            for (int mode = 0; mode < 5; ++mode)      // grey, RGB 4:4:4 / 4:2:2 / 4:2:0, RGBA 4:2:0
                for (int q : qualities)
                    for (int type = 0; type < 2; ++type) {
                        const int w = wh[0], h = wh[1], c = mode == 0 ? 1 : mode == 4 ? 4 : 3, sub = mode == 0 ? 0 : mode == 4 ? 2 : mode - 1;
                        const int rr = (int)(lcg(&seed) % 3u), kind = (int)(lcg(&seed) % 3u);
                        const size_t n = (size_t)w * h * c;
                        void* px = malloc(n * (type ? 4 : 1));
                        for (size_t i = 0; i < n; ++i) {
                            const uint32_t r = lcg(&seed);
                            const int v = kind == 0 ? (int)(r & 255u) : kind == 1 ? ((r & 1u) ? 255 : 0) : (int)(i % 251);
                            if (type) ((float*)px)[i] = (r & 0xFF00u) == 0 ? NAN : (float)v / 170.0f - 0.25f;
                            else ((uint8_t*)px)[i] = (uint8_t)v;
                        }
                        const int64_t cap = hr_jpeg_enc_plan(w, h, c, sub, rr).bound;
                        uint8_t* f1 = (uint8_t*)malloc((size_t)cap);
                        uint8_t* f2 = (uint8_t*)malloc((size_t)cap);
                        hr_jpeg_enc_stats st;
                        const int64_t n1 = hr_jpeg_encode_host(px, type, w, h, c, q, sub, rr, f1, cap, nullptr, &st);
                        const int64_t n2 = hr_jpeg_encode_host(px, type, w, h, c, q, sub, rr, f2, cap, nullptr, nullptr);
                        ++images;
                        if (n1 < 4 || n1 > cap || n1 != n2 || memcmp(f1, f2, (size_t)n1) || f1[0] != 0xFF || f1[1] != 0xD8 || f1[n1 - 2] != 0xFF || f1[n1 - 1] != 0xD9 ||
                            hr_jpeg_encode_host(px, type, w, h, c, q, sub, rr, f2, cap - 1, nullptr, nullptr) != -1)
                            ++bad;
                        free(px); free(f1); free(f2);
                    }
    printf("%ld images, %ld bad\n", images, bad);
    return bad ? 1 : 0;
}
