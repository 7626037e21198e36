// Arithmetic of PIL's 8-bit image resize (Image.resize of an RGB image: libImaging/Resample.c), the rule behind every PIL-based
// dataset's get_rgb (datasets/llff.py:145-163: LANCZOS to _img_wh, then BOX to img_wh).  Shared by the kernels of resize_kernel.hip,
// the plan of api_resize.hip and, compiled by the host compiler, by the CPU suite (tests/host_math/hr_resize_host.cpp).  PIL's output is
// the authority; this is its arithmetic, for one axis of `in` pixels resampled to `out`:
//   scale = in / out, fs = max(scale, 1), sup = support * fs, ksize = (int)ceil(sup) * 2 + 1                       (all double)
//   output xx: c = (xx + 0.5) * scale, xmin = max((int)(c - sup + 0.5), 0), n = min((int)(c + sup + 0.5), in) - xmin,
//              w[x] = f((x + xmin - c + 0.5) * (1 / fs)), ww = their sum in index order, w[x] /= ww when ww != 0
//   k[x] = (int)(w[x] * 2^22 + 0.5) for w[x] >= 0, (int)(w[x] * 2^22 - 0.5) below               (the cast truncates toward zero)
//   byte = clamp((2^21 + sum_x pixel[xmin + x] * k[x]) >> 22, 0, 255) in int32, the shift arithmetic
// Two axes: the horizontal pass first, into an 8-bit image (its clamp is part of the result), then the vertical pass; a pass whose axis
// keeps its size is skipped.  Coefficients are computed on the host only: no device code evaluates a filter.
#ifndef HR_RESIZE_H
#define HR_RESIZE_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HR_RSZ_FN __host__ __device__ __forceinline__
#else
#define HR_RSZ_FN static inline
#endif

// the values of PIL's Image.Resampling; NEAREST (0) and HAMMING (5) are not provided
enum { HR_RESIZE_LANCZOS = 1, HR_RESIZE_BILINEAR = 2, HR_RESIZE_BICUBIC = 3, HR_RESIZE_BOX = 4 };

constexpr int HR_RESIZE_BITS = 22;                // fractional bits of a coefficient: 32 - 8 - 2

// what hr_resize_check says of a coefficient table
enum { HR_RESIZE_ROWS_OK = 0, HR_RESIZE_ROWS_FIT_MAD24 = 1, HR_RESIZE_ROWS_OVERFLOW = -1 };

static inline bool hr_resize_filter_known(int filter)
{
    return filter == HR_RESIZE_LANCZOS || filter == HR_RESIZE_BILINEAR || filter == HR_RESIZE_BICUBIC || filter == HR_RESIZE_BOX;
}

static inline double hr_resize_support(int filter)
{
    return filter == HR_RESIZE_BOX ? 0.5 : filter == HR_RESIZE_BILINEAR ? 1.0 : filter == HR_RESIZE_BICUBIC ? 2.0 : 3.0;
}

static inline double hr_resize_sinc(double x)
{
    if (x == 0.0) return 1.0;
    x = x * 3.14159265358979323846;
    return sin(x) / x;
}

// one IEEE double operation per operator, in this order, whatever the translation unit's flags say
static inline double hr_resize_filter(int filter, double x)
{
#pragma clang fp contract(off)
#pragma clang fp reassociate(off)
    switch (filter) {
    case HR_RESIZE_BOX:
        return x > -0.5 && x <= 0.5 ? 1.0 : 0.0;
    case HR_RESIZE_BILINEAR:
        if (x < 0.0) x = -x;
        return x < 1.0 ? 1.0 - x : 0.0;
    case HR_RESIZE_BICUBIC: {
        const double a = -0.5;
        if (x < 0.0) x = -x;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
        if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
        return 0.0;
    }
    default:
        return -3.0 <= x && x < 3.0 ? hr_resize_sinc(x) * hr_resize_sinc(x / 3) : 0.0;
    }
}

// taps a coefficient row holds (the rows of one axis are all this long, zero-filled past their n); 0 for arguments no axis has
static inline int64_t hr_resize_ksize(int32_t in, int32_t out, int filter)
{
    if (in < 1 || out < 1 || !hr_resize_filter_known(filter)) return 0;
    const double scale = (double)in / (double)out;
    const double sup = hr_resize_support(filter) * (scale < 1.0 ? 1.0 : scale);
    return (int64_t)ceil(sup) * 2 + 1;
}

// bounds: (out, 2) = (xmin, n) per output; k: (out, ksize) fixed-point coefficients.  Nothing is allocated: a row's weights are evaluated
// twice, once for their sum and once for the quotients (the same operations give the same doubles).
static inline void hr_resize_coeffs(int32_t in, int32_t out, int filter, int32_t* bounds, int32_t* k)
{
#pragma clang fp contract(off)
#pragma clang fp reassociate(off)
#pragma clang fp reciprocal(off)
    const int64_t ksize = hr_resize_ksize(in, out, filter);
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double sup = hr_resize_support(filter) * fs;
    const double ss = 1.0 / fs;
    for (int32_t xx = 0; xx < out; ++xx) {
        const double c = (xx + 0.5) * scale;
        int32_t xmin = (int32_t)(c - sup + 0.5);
        if (xmin < 0) xmin = 0;
        int32_t xmax = (int32_t)(c + sup + 0.5);
        if (xmax > in) xmax = in;
        const int32_t n = xmax - xmin;
        double ww = 0.0;
        for (int32_t x = 0; x < n; ++x) ww += hr_resize_filter(filter, (x + xmin - c + 0.5) * ss);
        int32_t* row = k + (int64_t)xx * ksize;
        for (int32_t x = 0; x < n; ++x) {
            double w = hr_resize_filter(filter, (x + xmin - c + 0.5) * ss);
            if (ww != 0.0) w /= ww;
            row[x] = w < 0 ? (int32_t)(-0.5 + w * (double)(1 << HR_RESIZE_BITS)) : (int32_t)(0.5 + w * (double)(1 << HR_RESIZE_BITS));
        }
        for (int64_t x = n; x < ksize; ++x) row[x] = 0;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = n;
    }
}

// What makes int32 a derived fact: every row must have 255 * sum|k| + 2^21 < 2^31, else HR_RESIZE_ROWS_OVERFLOW and *bad_row (may be NULL)
// names the first that has not.  HR_RESIZE_ROWS_FIT_MAD24 when besides every |k| < 2^23, so that the 24-bit multiply-add is exact.
static inline int hr_resize_check(const int32_t* k, int64_t rows, int64_t ksize, int64_t* bad_row)
{
    bool fit24 = true;
    for (int64_t r = 0; r < rows; ++r) {
        int64_t sum = 0;
        for (int64_t x = 0; x < ksize; ++x) {
            const int64_t v = k[r * ksize + x], a = v < 0 ? -v : v;
            sum += a;
            if (a >= (1 << 23)) fit24 = false;
        }
        if (255 * sum + (1 << (HR_RESIZE_BITS - 1)) >= ((int64_t)1 << 31)) {
            if (bad_row) *bad_row = r;
            return HR_RESIZE_ROWS_OVERFLOW;
        }
    }
    return fit24 ? HR_RESIZE_ROWS_FIT_MAD24 : HR_RESIZE_ROWS_OK;
}

// acc + pixel * k.  MAD24: the 24-bit multiply-add, exact when |k| < 2^23 (pixel <= 255 always)
template <bool MAD24>
HR_RSZ_FN int32_t hr_resize_mad(int32_t acc, uint8_t pixel, int32_t k)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (MAD24) return __mul24((int)pixel, k) + acc;
#endif
    return acc + (int32_t)pixel * k;
}

HR_RSZ_FN int32_t hr_resize_acc0() { return 1 << (HR_RESIZE_BITS - 1); }

// the sum's byte: an arithmetic shift (negative sums occur, and clamp to 0)
HR_RSZ_FN uint8_t hr_resize_finish(int32_t acc)
{
    const int32_t v = acc >> HR_RESIZE_BITS;
    return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// one output byte: n taps, pixel bytes `stride` apart (3 or 4: along a row of RGB or RGBA pixels; the row pitch: down a column)
template <bool MAD24>
HR_RSZ_FN uint8_t hr_resize_dot(const uint8_t* px, int64_t stride, const int32_t* k, int32_t n)
{
    int32_t acc = hr_resize_acc0();
    for (int32_t x = 0; x < n; ++x) acc = hr_resize_mad<MAD24>(acc, px[x * stride], k[x]);
    return hr_resize_finish(acc);
}

// ---- RGBA: PIL resamples premultiplied bytes (Image.resize of an RGBA image: RGBA -> RGBa, the resize above on all four channels,
// RGBa -> RGBA; libImaging/Convert.c).  Both conversions are integer rules of their own; alpha passes through both unchanged.
// colour byte c under alpha a -> premultiplied: PIL's MULDIV255, the rounded c * a / 255 without a division
HR_RSZ_FN uint8_t hr_premultiply(uint8_t c, uint8_t a)
{
    const uint32_t t = (uint32_t)c * a + 128;
    return (uint8_t)(((t >> 8) + t) >> 8);
}

// premultiplied byte c under alpha a -> colour: copied at a == 0 and a == 255, else min(255, 255 * c / a), the division truncating
// (after a Lanczos or bicubic pass c > a occurs: the clamp is live)
HR_RSZ_FN uint8_t hr_unpremultiply(uint8_t c, uint8_t a)
{
    if (a == 0 || a == 255) return c;
    const uint32_t q = (255u * c) / a;                // exact: an integer division of 16-bit by 8-bit values
    return (uint8_t)(q > 255 ? 255 : q);
}

// a whole pixel, alpha in the top byte (little-endian R, G, B, A)
HR_RSZ_FN uint32_t hr_premultiply_pixel(uint32_t px)
{
    const uint8_t a = (uint8_t)(px >> 24);
    return (uint32_t)hr_premultiply((uint8_t)px, a) | (uint32_t)hr_premultiply((uint8_t)(px >> 8), a) << 8
           | (uint32_t)hr_premultiply((uint8_t)(px >> 16), a) << 16 | (px & 0xff000000u);
}

// ---- which kernel serves an axis (resize_kernel.hip) ------------------------------------------------------------------------------
// The staged kernels keep a tile's source bytes in LDS, and the horizontal one its coefficient rows as well.  They are chosen while that
// fits HR_RESIZE_LDS_BUDGET, the LDS of a workgroup when 8 workgroups of 256 threads fill a compute unit's 32 wavefronts (160 KiB / 8);
// an axis whose taps need more (ksize is unbounded: in / out is the caller's) is served by the general kernel, one thread per output
// byte reading global memory.  Both compute hr_resize_dot's sum.
constexpr int HR_RESIZE_LDS_BUDGET = 20 * 1024;
constexpr int HR_RESIZE_H_TILE = 64;              // horizontal: output pixels of a workgroup's tile ...
constexpr int HR_RESIZE_H_ROWS = 4;               // ... and image rows it holds at a time
constexpr int HR_RESIZE_H_ROWS_PER_GROUP = 16;    // rows a workgroup walks with one staging of its coefficient rows
constexpr int HR_RESIZE_V_BYTES = 256;            // vertical: bytes of an image row a workgroup's tile spans (one per thread)
constexpr int HR_RESIZE_V_PITCH = HR_RESIZE_V_BYTES + 16;   // LDS bytes per staged row: the bytes keep their address modulo 16

struct hr_resize_axis_plan {
    int32_t staged;       // 1: the staged kernel; 0: the general kernel
    int32_t tile;         // outputs of a workgroup along the axis (vertical: 8, 4, 2 or 1 output rows)
    int32_t span;         // the most source pixels (horizontal) or rows (vertical) any tile reads
    int32_t row_pitch;    // horizontal: LDS bytes per staged row (a multiple of 16)
    int32_t lds_bytes;    // dynamic LDS of the staged kernel
};

// the most source positions that `tile` consecutive outputs read: xmin and xmin + n never decrease along the axis
static inline int32_t hr_resize_span(const int32_t* bounds, int32_t out, int32_t tile)
{
    int32_t span = 0;
    for (int32_t i0 = 0; i0 < out; i0 += tile) {
        const int32_t i1 = (i0 + tile < out ? i0 + tile : out) - 1;
        const int32_t s = bounds[2 * i1] + bounds[2 * i1 + 1] - bounds[2 * i0];
        if (s > span) span = s;
    }
    return span;
}

// bpp: the bytes of a pixel, 3 (RGB) or 4 (RGBA)
static inline hr_resize_axis_plan hr_resize_plan_horizontal(const int32_t* bounds, int32_t out, int64_t ksize, int32_t bpp = 3)
{
    hr_resize_axis_plan p = {0, HR_RESIZE_H_TILE, hr_resize_span(bounds, out, HR_RESIZE_H_TILE), 0, 0};
    const int64_t pitch = ((int64_t)p.span * bpp + 15 + 15) / 16 * 16;               // the span, wherever its first byte falls in a 16-byte chunk
    const int64_t lds = (int64_t)HR_RESIZE_H_TILE * ksize * 4 + HR_RESIZE_H_ROWS * pitch;
    if (lds <= HR_RESIZE_LDS_BUDGET) {
        p.staged = 1;
        p.row_pitch = (int32_t)pitch;
        p.lds_bytes = (int32_t)lds;
    }
    return p;
}

// (a vertical tile spans bytes, whatever pixel they belong to: bpp changes nothing here)
static inline hr_resize_axis_plan hr_resize_plan_vertical(const int32_t* bounds, int32_t out, int64_t ksize, int32_t bpp = 3)
{
    (void)ksize;
    (void)bpp;
    hr_resize_axis_plan p = {0, 1, 0, HR_RESIZE_V_PITCH, 0};
    for (int32_t tile = 8; tile >= 1; tile >>= 1) {
        p.tile = tile;
        p.span = hr_resize_span(bounds, out, tile);
        if ((int64_t)p.span * HR_RESIZE_V_PITCH <= HR_RESIZE_LDS_BUDGET) {
            p.staged = 1;
            p.lds_bytes = p.span * HR_RESIZE_V_PITCH;
            break;
        }
    }
    return p;
}

#endif  // HR_RESIZE_H
