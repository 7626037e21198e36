// TEST-ONLY host build of the RGBA part of hyperreel_amd/csrc/hr_resize.h (PIL's resize of an 8-bit RGBA image: premultiply, the 8-bit
// resize on four channels, un-premultiply; the axis plans with 4 bytes per pixel), so that the CPU suite can compare it with PIL's
// conversions on every (colour, alpha) pair and with the fixtures PIL wrote.  Nothing in the product links or loads this file.
#include <stdlib.h>

#include "../../hyperreel_amd/csrc/hr_resize.h"

extern "C" {

// out (256, 256): out[c][a]
void hrz4_premultiply_table(uint8_t* out)
{
    for (int c = 0; c < 256; ++c)
        for (int a = 0; a < 256; ++a) out[c * 256 + a] = hr_premultiply((uint8_t)c, (uint8_t)a);
}

void hrz4_unpremultiply_table(uint8_t* out)
{
    for (int c = 0; c < 256; ++c)
        for (int a = 0; a < 256; ++a) out[c * 256 + a] = hr_unpremultiply((uint8_t)c, (uint8_t)a);
}

// n little-endian RGBA words in place
void hrz4_premultiply_pixels(uint32_t* px, int64_t n)
{
    for (int64_t i = 0; i < n; ++i) px[i] = hr_premultiply_pixel(px[i]);
}

// out5 = staged, tile, span, row_pitch, lds_bytes
void hrz4_axis_plan(int32_t vertical, const int32_t* bounds, int32_t out, int64_t ksize, int32_t bpp, int32_t* out5)
{
    const hr_resize_axis_plan p = vertical ? hr_resize_plan_vertical(bounds, out, ksize, bpp) : hr_resize_plan_horizontal(bounds, out, ksize, bpp);
    out5[0] = p.staged; out5[1] = p.tile; out5[2] = p.span; out5[3] = p.row_pitch; out5[4] = p.lds_bytes;
}

// one axis of one dense premultiplied image: vertical 0: (lines, in, 4) -> (lines, out, 4); vertical 1: (in, lines) -> (out, lines), `lines` the
// bytes of a row
static int axis(const uint8_t* s, uint8_t* d, int32_t in, int32_t out, int32_t lines, int32_t filter, int vertical)
{
    const int64_t ksize = hr_resize_ksize(in, out, filter);
    int32_t* bounds = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)out);
    int32_t* k = (int32_t*)malloc(sizeof(int32_t) * (size_t)out * (size_t)ksize);
    hr_resize_coeffs(in, out, filter, bounds, k);
    const int ok = hr_resize_check(k, out, ksize, nullptr);
    if (ok != HR_RESIZE_ROWS_OVERFLOW) {
        if (vertical) {
            for (int32_t y = 0; y < out; ++y)
                for (int32_t j = 0; j < lines; ++j)
                    d[(int64_t)y * lines + j] = hr_resize_dot<false>(s + (int64_t)bounds[2 * y] * lines + j, lines, k + y * ksize, bounds[2 * y + 1]);
        } else {
            for (int32_t y = 0; y < lines; ++y)
                for (int32_t j = 0; j < out * 4; ++j)
                    d[((int64_t)y * out) * 4 + j] = hr_resize_dot<false>(s + ((int64_t)y * in + bounds[2 * (j / 4)]) * 4 + j % 4, 4, k + (j / 4) * ksize,
                                                                         bounds[2 * (j / 4) + 1]);
        }
    }
    free(bounds);
    free(k);
    return ok == HR_RESIZE_ROWS_OVERFLOW ? -1 : 0;
}

// src (n, h, w, 4) RGBA -> dst (n, h2, w2, 4) RGBA as Image.resize computes it: equal sizes copy; else premultiply, the horizontal pass into
// 8 bits, the vertical pass (a pass whose axis keeps its size is skipped), un-premultiply.  premultiplied_or_null (n, h2, w2, 4): the
// resampled bytes before the last conversion
int32_t hrz4_resize(const uint8_t* src, int32_t n_images, int32_t w, int32_t h, int32_t w2, int32_t h2, int32_t filter, uint8_t* dst,
                    uint8_t* premultiplied_or_null)
{
    if (w == w2 && h == h2) {
        for (int64_t i = 0; i < (int64_t)n_images * h * w * 4; ++i) dst[i] = src[i];
        if (premultiplied_or_null)
            for (int64_t i = 0; i < (int64_t)n_images * h * w * 4; ++i) premultiplied_or_null[i] = src[i];
        return 0;
    }
    int rc = 0;
    uint8_t* pre = (uint8_t*)malloc((size_t)h * w * 4);
    uint8_t* mid = (uint8_t*)malloc((size_t)h * w2 * 4);
    for (int64_t img = 0; img < n_images && !rc; ++img) {
        const uint8_t* s = src + img * h * w * 4;
        uint8_t* d = dst + img * h2 * w2 * 4;
        for (int64_t i = 0; i < (int64_t)h * w; ++i) {
            const uint8_t a = s[4 * i + 3];
            for (int c = 0; c < 3; ++c) pre[4 * i + c] = hr_premultiply(s[4 * i + c], a);
            pre[4 * i + 3] = a;
        }
        if (h == h2) rc = axis(pre, d, w, w2, h, filter, 0);
        else if (w == w2) rc = axis(pre, d, h, h2, w * 4, filter, 1);
        else {
            rc = axis(pre, mid, w, w2, h, filter, 0);
            if (!rc) rc = axis(mid, d, h, h2, w2 * 4, filter, 1);
        }
        if (rc) break;
        if (premultiplied_or_null)
            for (int64_t i = 0; i < (int64_t)h2 * w2 * 4; ++i) premultiplied_or_null[img * h2 * w2 * 4 + i] = d[i];
        for (int64_t i = 0; i < (int64_t)h2 * w2; ++i) {
            const uint8_t a = d[4 * i + 3];
            for (int c = 0; c < 3; ++c) d[4 * i + c] = hr_unpremultiply(d[4 * i + c], a);
        }
    }
    free(pre);
    free(mid);
    return rc;
}

}
