// Camera rays with NDC (hr_generate_rays_ndc), fisheye cameras' rays (hr_generate_rays_fisheye), two-plane light-field rays (hr_generate_rays_lightfield, hr_generate_rays_epi) and the
// training feed (hr_rayset_batch / hr_rayset_order / hr_rayset_sample).  One lane per ray; the arithmetic is hr_camera.h's, hr_lightfield.h's and hr_sample_rng.h's, which
// the CPU suite compiles for the host.  Launch-bound at a training batch (16 384 rays: 64
// workgroups); nothing to tune beyond the stores: a lane owns a whole output row and writes it in 16- or 8-byte pieces when the
// buffer is aligned for that, so a wavefront's stores cover a contiguous 64 * row bytes.
#include "hr_camera.h"
#include "hr_lightfield.h"
#include "hr_sample_rng.h"
#include "hr_kernels.h"

namespace {

// VEC: rows start on 8-byte (6 columns) / 16-byte (8 columns) boundaries
template <bool VEC>
__device__ __forceinline__ void store_ray(float* __restrict__ r, const float* v, int ray_dim)
{
    if (VEC && ray_dim == 8) {
        reinterpret_cast<float4*>(r)[0] = make_float4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<float4*>(r)[1] = make_float4(v[4], v[5], v[6], v[7]);
    } else if (VEC) {
        reinterpret_cast<float2*>(r)[0] = make_float2(v[0], v[1]);
        reinterpret_cast<float2*>(r)[1] = make_float2(v[2], v[3]);
        reinterpret_cast<float2*>(r)[2] = make_float2(v[4], v[5]);
    } else {
#pragma unroll
        for (int c = 0; c < 8; ++c)                    // (fixed trip count: v stays in registers)
            if (c < ray_dim) r[c] = v[c];
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void hr_generate_rays_ndc_kernel(const hr_camera cam, const hr_ndc ndc, int has_ndc, int ray_dim,
                                                                   int64_t first_pixel, int64_t n_pixels, float* __restrict__ rays)
{
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n_pixels; t += (int64_t)gridDim.x * 256) {
        const int64_t p = first_pixel + t;
        float v[8];
        hr_pixel_ray(cam, has_ndc ? &ndc : nullptr, (int)(p % cam.width), (int)(p / cam.width), v);
        v[6] = cam.cam_id; v[7] = cam.time;
        store_ray<VEC>(rays + t * ray_dim, v, ray_dim);
    }
}

// hr_generate_rays_ndc_kernel's shape with hr_pixel_ray_lens per pixel (a NULL hr_fisheye never gets here: the pinhole kernels serve it)
template <bool VEC>
__global__ __launch_bounds__(256) void hr_generate_rays_fisheye_kernel(const hr_camera cam, const hr_fisheye fe, const hr_ndc ndc, int has_ndc, int ray_dim,
                                                                       int64_t first_pixel, int64_t n_pixels, float* __restrict__ rays)
{
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n_pixels; t += (int64_t)gridDim.x * 256) {
        const int64_t p = first_pixel + t;
        float v[8];
        // two calls, not has_ndc ? &ndc : nullptr: with the select the by-value ndc was copied to scratch (24 bytes a lane)
        if (has_ndc) hr_pixel_ray_lens(cam, fe, &ndc, (int)(p % cam.width), (int)(p / cam.width), v);
        else hr_pixel_ray_lens(cam, fe, nullptr, (int)(p % cam.width), (int)(p / cam.width), v);
        v[6] = cam.cam_id; v[7] = cam.time;
        store_ray<VEC>(rays + t * ray_dim, v, ray_dim);
    }
}

// a view at (a, b) = (s, t), or with EPI the slice at (a, b) = (v, t): row p = y * width + x of the list
template <bool VEC, bool EPI>
__global__ __launch_bounds__(256) void hr_generate_rays_lightfield_kernel(const hr_lightfield lf, float a, float b, int64_t first, int64_t n,
                                                                          float* __restrict__ rays)
{
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
        const int64_t p = first + t;
        float v[8];
        if (EPI) hr_epi_ray(lf, a, b, (int)(p % lf.width), (int)(p / lf.width), v);
        else hr_lightfield_ray(lf, a, b, (int)(p % lf.width), (int)(p / lf.width), v);
        store_ray<VEC>(rays + t * 6, v, 6);
    }
}

// set element -> image (binary search in the prefix sums) -> pixel (closed form) -> ray, colour, weight: output row t of a call.  Shared by
// hr_rayset_batch (the epoch's order, or the caller's indices) and hr_rayset_sample (draws with replacement): the same bits for the same element
template <bool VEC, bool LF>
__device__ __forceinline__ void rayset_write_row(const HrRaySetArgs& a, int64_t t, int64_t e)
{
    if (a.elements) a.elements[t] = e;
    if (!a.coords && !a.rgb && !a.weight) return;
    const bool inside = e >= 0 && e < a.size;           // only a caller's own index can be outside
    float v[8], c[3], wgt = 0.0f;
    if (inside) {
        int lo = 0, hi = a.n_images - 1;                 // the image with prefix[i] <= e < prefix[i + 1]
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (a.prefix[mid + 1] > e) hi = mid; else lo = mid + 1;
        }
        const HrRayImage& im = a.images[lo];
        int x, y;
        hr_subsample_pixel(a.width, a.height, im.every, im.offset, e - a.prefix[lo], &x, &y);
        if (LF) {
            hr_lightfield_ray(a.lf, im.s, im.t, x, y, v);
        } else {
            hr_pixel_ray_fisheye(im.cam, im.has_fe ? &im.fe : nullptr, a.has_ndc ? &a.ndc : nullptr, x, y, v);
            v[6] = im.cam.cam_id; v[7] = im.cam.time;
        }
        if (a.rgb) {
            const uint8_t* px = a.pixels + (((int64_t)lo * a.height + y) * a.width + x) * 3;
            c[0] = (float)px[0] / 255.0f; c[1] = (float)px[1] / 255.0f; c[2] = (float)px[2] / 255.0f;   // ToTensor
        }
        wgt = 1.0f;
    } else {
        for (int k = 0; k < 8; ++k) v[k] = __builtin_nanf("");
        c[0] = c[1] = c[2] = __builtin_nanf("");
    }
    if (a.coords) store_ray<VEC>(a.coords + t * a.ray_dim, v, a.ray_dim);
    if (a.rgb) { float* o = a.rgb + t * 3; o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; }
    if (a.weight) a.weight[t] = wgt;
}

template <bool VEC, bool LF>
__global__ __launch_bounds__(256) void hr_rayset_batch_kernel(const HrRaySetArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n) return;
    const int64_t e = a.indices ? a.indices[t] : (int64_t)hr_perm((uint64_t)a.size, a.key, (uint64_t)(a.first + t));
    rayset_write_row<VEC, LF>(a, t, e);
}

// row t = element hr_sample_element(size, seed, s, t), s = *step_dev when given (read by every lane: one cached word), else `step`.
// An empty set (size 0) has no element to draw: -1, which rayset_write_row turns into a NaN row of weight 0.
template <bool VEC, bool LF>
__global__ __launch_bounds__(256) void hr_rayset_sample_kernel(const HrRaySetArgs a, uint64_t seed, uint64_t step, const uint64_t* __restrict__ step_dev)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n) return;
    const uint64_t s = step_dev ? *step_dev : step;
    const int64_t e = a.size > 0 ? (int64_t)hr_sample_element((uint64_t)a.size, seed, s, (uint64_t)t) : -1;
    rayset_write_row<VEC, LF>(a, t, e);
}

bool rows_aligned(const float* p, int ray_dim)
{
    return p && (reinterpret_cast<uintptr_t>(p) & (ray_dim == 8 ? 15 : 7)) == 0;
}

}  // namespace

void hr_launch_generate_rays_ndc(const hr_camera& cam, const hr_ndc* ndc, int ray_dim, int64_t first_pixel, int64_t n_pixels, float* rays,
                                 hipStream_t stream)
{
    if (n_pixels <= 0) return;
    int64_t blocks = (n_pixels + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    const hr_ndc nd = ndc ? *ndc : hr_ndc();
    if (rows_aligned(rays, ray_dim))
        hipLaunchKernelGGL(hr_generate_rays_ndc_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, cam, nd, ndc ? 1 : 0, ray_dim,
                           first_pixel, n_pixels, rays);
    else
        hipLaunchKernelGGL(hr_generate_rays_ndc_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, cam, nd, ndc ? 1 : 0, ray_dim,
                           first_pixel, n_pixels, rays);
}

void hr_launch_generate_rays_fisheye(const hr_camera& cam, const hr_fisheye& fe, const hr_ndc* ndc, int ray_dim, int64_t first_pixel,
                                     int64_t n_pixels, float* rays, hipStream_t stream)
{
    if (n_pixels <= 0) return;
    int64_t blocks = (n_pixels + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    const hr_ndc nd = ndc ? *ndc : hr_ndc();
    if (rows_aligned(rays, ray_dim))
        hipLaunchKernelGGL(hr_generate_rays_fisheye_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, cam, fe, nd, ndc ? 1 : 0, ray_dim,
                           first_pixel, n_pixels, rays);
    else
        hipLaunchKernelGGL(hr_generate_rays_fisheye_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, cam, fe, nd, ndc ? 1 : 0, ray_dim,
                           first_pixel, n_pixels, rays);
}

template <bool EPI>
static void launch_lightfield(const hr_lightfield& lf, float a, float b, int64_t first, int64_t n, float* rays, hipStream_t stream)
{
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (rows_aligned(rays, 6))
        hipLaunchKernelGGL((hr_generate_rays_lightfield_kernel<true, EPI>), dim3((unsigned)blocks), dim3(256), 0, stream, lf, a, b, first, n, rays);
    else
        hipLaunchKernelGGL((hr_generate_rays_lightfield_kernel<false, EPI>), dim3((unsigned)blocks), dim3(256), 0, stream, lf, a, b, first, n, rays);
}

void hr_launch_generate_rays_lightfield(const hr_lightfield& lf, bool epi, float a, float b, int64_t first, int64_t n, float* rays, hipStream_t stream)
{
    if (n <= 0) return;
    if (epi) launch_lightfield<true>(lf, a, b, first, n, rays, stream);
    else launch_lightfield<false>(lf, a, b, first, n, rays, stream);
}

void hr_launch_rayset_batch(const HrRaySetArgs& a, hipStream_t stream)
{
    if (a.n <= 0) return;
    const dim3 grid((unsigned)((a.n + 255) / 256));
    const bool vec = !a.coords || rows_aligned(a.coords, a.ray_dim);
    if (a.lightfield) {
        if (vec) hipLaunchKernelGGL((hr_rayset_batch_kernel<true, true>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((hr_rayset_batch_kernel<false, true>), grid, dim3(256), 0, stream, a);
    } else {
        if (vec) hipLaunchKernelGGL((hr_rayset_batch_kernel<true, false>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((hr_rayset_batch_kernel<false, false>), grid, dim3(256), 0, stream, a);
    }
}

void hr_launch_rayset_sample(const HrRaySetArgs& a, uint64_t seed, uint64_t step, const uint64_t* step_dev, hipStream_t stream)
{
    if (a.n <= 0) return;
    const dim3 grid((unsigned)((a.n + 255) / 256));
    const bool vec = !a.coords || rows_aligned(a.coords, a.ray_dim);
    if (a.lightfield) {
        if (vec) hipLaunchKernelGGL((hr_rayset_sample_kernel<true, true>), grid, dim3(256), 0, stream, a, seed, step, step_dev);
        else hipLaunchKernelGGL((hr_rayset_sample_kernel<false, true>), grid, dim3(256), 0, stream, a, seed, step, step_dev);
    } else {
        if (vec) hipLaunchKernelGGL((hr_rayset_sample_kernel<true, false>), grid, dim3(256), 0, stream, a, seed, step, step_dev);
        else hipLaunchKernelGGL((hr_rayset_sample_kernel<false, false>), grid, dim3(256), 0, stream, a, seed, step, step_dev);
    }
}
