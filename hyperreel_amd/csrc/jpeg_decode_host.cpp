// Host build of hr_jpeg_decode.h for hyperreel_amd/jpeg.py's decode_host: the same functions the kernels of jpeg_decode_kernel.hip call,
// compiled by the host compiler into a small library of its own.  Pixels, status and rounds equal the device's.
#include "hr_jpeg_decode.h"

extern "C" {

// the markers up to the scan: the status of hr_jpeg_parse_head (info is filled as far as the file was read)
int32_t hr_jpeg_host_probe(const uint8_t* file, int64_t n, hr_jpeg_info* info) { return hr_jpeg_probe_host(file, n, info); }

// out: expect_h * expect_w * out_channels bytes; (-1, -1): the size hr_jpeg_host_probe reports.  Returns the image's status.
int32_t hr_jpeg_host_decode(const uint8_t* file, int64_t n, int32_t expect_w, int32_t expect_h, int32_t out_channels, int32_t subseq_bits,
                            uint8_t* out, hr_jpeg_info* info, int32_t* rounds)
{
    return hr_jpeg_decode_host_sized(file, n, expect_w, expect_h, out_channels, subseq_bits, out, info, rounds);
}

// one block: 64 quantised coefficients and a quantisation table, both in natural order, to 64 samples; returns 1 for HR_JPEG_E_COEF's ranges
int32_t hr_jpeg_host_idct(const int16_t* coef, const uint8_t* qt, uint8_t* out)
{
    int32_t ws[8][8], row[8], col[8];
    int wide = 0;
    for (int x = 0; x < 8; ++x) {
        wide |= hr_jpeg_idct_column(coef, qt, x, col);
        for (int y = 0; y < 8; ++y) ws[y][x] = col[y];
    }
    for (int y = 0; y < 8; ++y) {
        for (int x = 0; x < 8; ++x) row[x] = ws[y][x];
        int32_t px[8];
        wide |= hr_jpeg_idct_row(row, px);
        for (int x = 0; x < 8; ++x) out[8 * y + x] = (uint8_t)px[x];
    }
    return wide;
}

}
