// TEST-ONLY host build of hyperreel_amd/csrc/hr_resize.h (PIL's 8-bit resize: coefficients, the accumulator check, the choice of
// kernel, the sum and its clamp), so that the CPU suite can compare it with a numpy statement of the rule, with the fixtures PIL wrote
// and with PIL itself.  Nothing in the product links or loads this file.
#include <stdlib.h>

#include "../../hyperreel_amd/csrc/hr_resize.h"

extern "C" {

int64_t hrz_ksize(int32_t in, int32_t out, int32_t filter) { return hr_resize_ksize(in, out, filter); }

// bounds (out, 2), k (out, hrz_ksize)
void hrz_coeffs(int32_t in, int32_t out, int32_t filter, int32_t* bounds, int32_t* k) { hr_resize_coeffs(in, out, filter, bounds, k); }

int32_t hrz_check(const int32_t* k, int64_t rows, int64_t ksize, int64_t* bad_row) { return hr_resize_check(k, rows, ksize, bad_row); }

// out5 = staged, tile, span, row_pitch, lds_bytes
void hrz_axis_plan(int32_t vertical, const int32_t* bounds, int32_t out, int64_t ksize, int32_t* out5)
{
    const hr_resize_axis_plan p = vertical ? hr_resize_plan_vertical(bounds, out, ksize) : hr_resize_plan_horizontal(bounds, out, ksize);
    out5[0] = p.staged; out5[1] = p.tile; out5[2] = p.span; out5[3] = p.row_pitch; out5[4] = p.lds_bytes;
}

// one axis of n_images dense images: vertical 0: (lines, in, 3) -> (lines, out, 3); vertical 1: (in, lines / 3, 3) -> (out, lines / 3, 3), `lines`
// the bytes of a row
static int axis(const uint8_t* src, uint8_t* dst, int32_t n_images, int32_t in, int32_t out, int32_t lines, int32_t filter, int vertical)
{
    const int64_t ksize = hr_resize_ksize(in, out, filter);
    int32_t* bounds = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)out);
    int32_t* k = (int32_t*)malloc(sizeof(int32_t) * (size_t)out * (size_t)ksize);
    hr_resize_coeffs(in, out, filter, bounds, k);
    const int ok = hr_resize_check(k, out, ksize, nullptr);
    if (ok != HR_RESIZE_ROWS_OVERFLOW) {
        for (int64_t img = 0; img < n_images; ++img) {
            if (vertical) {
                const uint8_t* s = src + img * in * lines;
                uint8_t* d = dst + img * out * lines;
                for (int32_t y = 0; y < out; ++y)
                    for (int32_t j = 0; j < lines; ++j)
                        d[(int64_t)y * lines + j] = hr_resize_dot<false>(s + (int64_t)bounds[2 * y] * lines + j, lines, k + y * ksize, bounds[2 * y + 1]);
            } else {
                const uint8_t* s = src + img * lines * in * 3;
                uint8_t* d = dst + img * lines * out * 3;
                for (int32_t y = 0; y < lines; ++y)
                    for (int32_t j = 0; j < out * 3; ++j)
                        d[((int64_t)y * out) * 3 + j] = hr_resize_dot<false>(s + ((int64_t)y * in + bounds[2 * (j / 3)]) * 3 + j % 3, 3, k + (j / 3) * ksize,
                                                                             bounds[2 * (j / 3) + 1]);
            }
        }
    }
    free(bounds);
    free(k);
    return ok == HR_RESIZE_ROWS_OVERFLOW ? -1 : 0;
}

// src (n, h, w, 3) -> dst (n, h2, w2, 3): the horizontal pass into 8 bits, then the vertical; a pass whose axis keeps its size is skipped
int32_t hrz_resize(const uint8_t* src, int32_t n_images, int32_t w, int32_t h, int32_t w2, int32_t h2, int32_t filter, uint8_t* dst)
{
    if (w == w2 && h == h2) {
        for (int64_t i = 0; i < (int64_t)n_images * h * w * 3; ++i) dst[i] = src[i];
        return 0;
    }
    if (h == h2) return axis(src, dst, n_images, w, w2, h, filter, 0);
    if (w == w2) return axis(src, dst, n_images, h, h2, w * 3, filter, 1);
    uint8_t* mid = (uint8_t*)malloc((size_t)n_images * h * w2 * 3);
    int rc = axis(src, mid, n_images, w, w2, h, filter, 0);
    if (!rc) rc = axis(mid, dst, n_images, h, h2, w2 * 3, filter, 1);
    free(mid);
    return rc;
}

}
