// TEST-ONLY stand-alone program over hyperreel_amd/csrc/hr_jpeg_decode.h (a JPEG file back into pixels) for a sanitizer build
// (tests/test_jpeg_decode_host.py): it decodes the files of a pack into heap blocks of exactly the image's size, at the default
// subsequence length and at 128 bits, then copies of them damaged by a seeded generator.  Whole files otherwise go through the product's
// host build of the same header (hyperreel_amd/csrc/jpeg_decode_host.cpp, hyperreel_amd/jpeg.py's decode_host).
#include "../../hyperreel_amd/csrc/hr_jpeg_decode.h"

#include <stdio.h>
#include <stdlib.h>

// The pack: int32 count; per file int32 w, h, int64 n, the n bytes of the file, the h * w * 4 bytes its RGBA decode must give.
static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s pack mutations-per-file\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const long per_file = atol(argv[2]);
    int32_t count = 0;
    if (!read_exact(f, &count, 4)) return 2;
    long good = 0, bad_bytes = 0, refused_good = 0, mutated = 0, accepted = 0, dirty = 0;
    uint32_t lcg = 12345u;
    for (int32_t i = 0; i < count; ++i) {
        int32_t w, h, rounds;
        int64_t n;
        if (!read_exact(f, &w, 4) || !read_exact(f, &h, 4) || !read_exact(f, &n, 8)) return 2;
        const size_t px = (size_t)w * (size_t)h;
        uint8_t* file = (uint8_t*)malloc((size_t)n);           // exact sizes: a byte too many is the sanitizer's to report
        uint8_t* want = (uint8_t*)malloc(px * 4);
        if (!read_exact(f, file, (size_t)n) || !read_exact(f, want, px * 4)) return 2;
        hr_jpeg_info info;
        const int32_t modes[3] = {4, 3, 1};
        for (int m = 0; m < 6; ++m) {
            uint8_t* out = (uint8_t*)malloc(px * (size_t)modes[m % 3]);
            const int32_t st = hr_jpeg_decode_host_sized(file, n, w, h, modes[m % 3], m < 3 ? 0 : 128, out, &info, &rounds);
            if (st != HR_JPEG_OK) { ++refused_good; fprintf(stderr, "file %d: status %d\n", (int)i, (int)st); }
            if (m % 3 == 0)
                for (size_t k = 0; k < px * 4; ++k) bad_bytes += out[k] != want[k];
            free(out);
        }
        ++good;
        uint8_t* copy = (uint8_t*)malloc((size_t)n);
        uint8_t* out = (uint8_t*)malloc(px * 4);
        for (long k = 0; k < per_file; ++k) {
            memcpy(copy, file, (size_t)n);
            lcg = lcg * 1664525u + 1013904223u;
            const int hits = 1 + (int)((lcg >> 28) & 3u);
            for (int q = 0; q < hits; ++q) {
                lcg = lcg * 1664525u + 1013904223u;
                const size_t at = (size_t)((lcg >> 8) % (uint32_t)n);
                lcg = lcg * 1664525u + 1013904223u;
                copy[at] ^= (uint8_t)(1u + ((lcg >> 16) % 255u));
            }
            lcg = lcg * 1664525u + 1013904223u;
            const int64_t len = ((lcg >> 20) & 7u) == 0 ? (int64_t)((lcg >> 4) % (uint32_t)(n + 1)) : n;       // one in eight is cut short too
            uint8_t* cut = (uint8_t*)malloc((size_t)len + 1);  // a block of its own length (+ 1: malloc(0) may be NULL)
            memcpy(cut, copy, (size_t)len);
            const int32_t st = hr_jpeg_decode_host_sized(cut, len, w, h, 4, (k & 1) ? 128 : 0, out, &info, &rounds);
            free(cut);
            ++mutated;
            if (st == HR_JPEG_OK) ++accepted;
            else
                for (size_t b = 0; b < px * 4; ++b)
                    if (out[b]) { ++dirty; break; }
        }
        free(out); free(copy); free(want); free(file);
    }
    fclose(f);
    printf("%ld good files, %ld refused, %ld bad bytes; %ld damaged, %ld accepted, %ld refused with a non-zero image\n", good, refused_good, bad_bytes, mutated,
           accepted, dirty);
    return (refused_good || bad_bytes || dirty) ? 1 : 0;
}
