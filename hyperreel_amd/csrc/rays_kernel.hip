// Every ray kernel.  One pixel-list kernel, hr_generate_rays_kernel<Gen>, with one launcher serves a camera's rays (CameraRays<LENS, NDC>: hr_generate_rays,
// hr_generate_rays_ndc, hr_generate_rays_fisheye -- pinhole or lens, world or NDC) and the two-plane light-field rays (LightfieldRays:
// hr_generate_rays_lightfield, hr_generate_rays_epi); the training feed (hr_rayset_batch / hr_rayset_order / hr_rayset_sample) has its two kernels over
// rayset_write_row.  One lane per ray; the arithmetic is hr_camera.h's, hr_lightfield.h's and hr_sample_rng.h's, which the CPU suite compiles for the
// host.  Launch-bound at a training batch (16 384 rays: 64 workgroups); nothing to tune beyond the stores: a lane owns a whole output row and writes
// it in one 16-byte and one or two 8-byte pieces (store_ray), so a wavefront's stores cover a contiguous 64 * row bytes.
#include "hr_camera.h"
#include "hr_lightfield.h"
#include "hr_sample_rng.h"
#include "hr_kernels.h"

namespace {

// Plain column stores: the compiler joins them into one 16-byte and one or two 8-byte stores, which global memory takes at any 4-byte
// address, so no form of the kernels depends on the buffer's alignment.  (float4 / float2 stores written out by hand for aligned rows came
// apart, between their 6- and 8-column branches, into five narrower ones.)
__device__ __forceinline__ void store_ray(float* __restrict__ r, const float* v, int ray_dim)
{
#pragma unroll
    for (int c = 0; c < 6; ++c) r[c] = v[c];
    if (ray_dim == 8) { r[6] = v[6]; r[7] = v[7]; }
}

// Row p of a camera's pixel list: the one camera pipeline of hr_camera.h -- pinhole, or the lens with LENS; then NDC with NDC.  Template
// flags, not launch-uniform fields: the pinhole instantiation then holds no more than the plain call's kernel did, and an 800 x 800 frame
// is not launch-bound -- with runtime flags it was measurably slower than that kernel.
template <bool LENS, bool NDC>
struct CameraRays {
    hr_camera cam;
    hr_fisheye fe;                              // read with LENS
    hr_ndc ndc;                                 // read with NDC
    int ray_dim;                                // 6, or 8 with (cam_id, time)
    __device__ __forceinline__ void operator()(int64_t p, float* v) const
    {
        const int x = (int)(p % cam.width), y = (int)(p / cam.width);
        // the world ray, then NDC as the stage of its own that it is in hr_pixel_ray: a has_ndc ? &ndc : nullptr handed down instead had
        // the by-value ndc copied to scratch (24 bytes a lane)
        if (LENS) hr_pixel_ray_lens(cam, fe, nullptr, x, y, v);
        else hr_pixel_ray(cam, nullptr, x, y, v);
        if (NDC) hr_world_to_ndc(&ndc, v);
        v[6] = cam.cam_id; v[7] = cam.time;
    }
};

// Row p = y * width + x of a light-field list: a view at (a, b) = (s, t), or with EPI the slice at (a, b) = (v, t)
template <bool EPI>
struct LightfieldRays {
    hr_lightfield lf;
    float a, b;
    static constexpr int ray_dim = 6;           // known to the compiler: the 8-column stores are not built
    __device__ __forceinline__ void operator()(int64_t p, float* v) const
    {
        const int x = (int)(p % lf.width), y = (int)(p / lf.width);
        if (EPI) hr_epi_ray(lf, a, b, x, y, v);
        else hr_lightfield_ray(lf, a, b, x, y, v);
    }
};

// The pixel-list kernel: rows [first, first + n) of `gen`'s list -> rays (n, gen.ray_dim)
template <class Gen>
__global__ __launch_bounds__(256) void hr_generate_rays_kernel(const Gen gen, int64_t first, int64_t n, float* __restrict__ rays)
{
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
        float v[8];
        gen(first + t, v);
        store_ray(rays + t * gen.ray_dim, v, gen.ray_dim);
    }
}

// set element -> image (binary search in the prefix sums) -> pixel (closed form, or the image's list) -> ray, colour, weight: output row t of a call.  Shared by
// hr_rayset_batch (the epoch's order, or the caller's indices) and hr_rayset_sample (draws with replacement): the same bits for the same element
template <bool LF>
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
        if (im.list) {                                   // the importance rule's list (importance_kernel.hip)
            const uint32_t p = im.list[e - a.prefix[lo]];
            x = (int)(p % (uint32_t)a.width); y = (int)(p / (uint32_t)a.width);
        } else {
            hr_subsample_pixel(a.width, a.height, im.every, im.offset, e - a.prefix[lo], &x, &y);
        }
        if (LF) {
            hr_lightfield_ray(a.lf, im.s, im.t, x, y, v);
        } else {
            hr_pixel_ray_fisheye(im.cam, im.has_fe ? &im.fe : nullptr, a.has_ndc ? &a.ndc : nullptr, x, y, v);
            v[6] = im.cam.cam_id; v[7] = im.cam.time;
        }
        if (a.rgb && a.rgba) {
            // RGBA over white (datasets/blender.py:61-70): ToTensor, then rgb * alpha + (1 - alpha), one float32 rounding per
            // operation as torch computes it -- no multiply-add is contracted out of these
            const uint32_t px = reinterpret_cast<const uint32_t*>(a.pixels)[((int64_t)lo * a.height + y) * a.width + x];
            const float al = (float)(px >> 24) / 255.0f, rest = __fsub_rn(1.0f, al);
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = __fadd_rn(__fmul_rn((float)((px >> (8 * k)) & 255u) / 255.0f, al), rest);
        } else if (a.rgb) {
            const uint8_t* px = a.pixels + (((int64_t)lo * a.height + y) * a.width + x) * 3;
            c[0] = (float)px[0] / 255.0f; c[1] = (float)px[1] / 255.0f; c[2] = (float)px[2] / 255.0f;   // ToTensor
        }
        wgt = 1.0f;
    } else {
        for (int k = 0; k < 8; ++k) v[k] = __builtin_nanf("");
        c[0] = c[1] = c[2] = __builtin_nanf("");
    }
    if (a.coords) store_ray(a.coords + t * a.ray_dim, v, a.ray_dim);
    if (a.rgb) { float* o = a.rgb + t * 3; o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; }
    if (a.weight) a.weight[t] = wgt;
}

template <bool LF>
__global__ __launch_bounds__(256) void hr_rayset_batch_kernel(const HrRaySetArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n) return;
    const int64_t e = a.indices ? a.indices[t] : (int64_t)hr_perm((uint64_t)a.size, a.key, (uint64_t)(a.first + t));
    rayset_write_row<LF>(a, t, e);
}

// row t = element hr_sample_element(size, seed, s, t), s = *step_dev when given (read by every lane: one cached word), else `step`.
// An empty set (size 0) has no element to draw: -1, which rayset_write_row turns into a NaN row of weight 0.
template <bool LF>
__global__ __launch_bounds__(256) void hr_rayset_sample_kernel(const HrRaySetArgs a, uint64_t seed, uint64_t step, const uint64_t* __restrict__ step_dev)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n) return;
    const uint64_t s = step_dev ? *step_dev : step;
    const int64_t e = a.size > 0 ? (int64_t)hr_sample_element((uint64_t)a.size, seed, s, (uint64_t)t) : -1;
    rayset_write_row<LF>(a, t, e);
}

template <class Gen>
void launch_pixel_list(const Gen& gen, int64_t first, int64_t n, float* rays, hipStream_t stream)
{
    if (n <= 0) return;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(hr_generate_rays_kernel<Gen>, dim3((unsigned)blocks), dim3(256), 0, stream, gen, first, n, rays);
}

// one lane per row of the call with k[LF], the set's kind
template <class... P, class... A>
void launch_rayset(void (*const (&k)[2])(P...), const HrRaySetArgs& a, hipStream_t stream, const A&... args)
{
    if (a.n <= 0) return;
    hipLaunchKernelGGL(k[a.lightfield != 0], dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, stream, args...);
}

}  // namespace

void hr_launch_generate_rays(const hr_camera& cam, const hr_fisheye* fe, const hr_ndc* ndc, int ray_dim, int64_t first_pixel, int64_t n_pixels,
                             float* rays, hipStream_t stream)
{
    const hr_fisheye f = fe ? *fe : hr_fisheye();
    const hr_ndc nd = ndc ? *ndc : hr_ndc();
    if (fe && ndc) launch_pixel_list(CameraRays<true, true>{cam, f, nd, ray_dim}, first_pixel, n_pixels, rays, stream);
    else if (fe) launch_pixel_list(CameraRays<true, false>{cam, f, nd, ray_dim}, first_pixel, n_pixels, rays, stream);
    else if (ndc) launch_pixel_list(CameraRays<false, true>{cam, f, nd, ray_dim}, first_pixel, n_pixels, rays, stream);
    else launch_pixel_list(CameraRays<false, false>{cam, f, nd, ray_dim}, first_pixel, n_pixels, rays, stream);
}

void hr_launch_generate_rays_lightfield(const hr_lightfield& lf, bool epi, float a, float b, int64_t first, int64_t n, float* rays, hipStream_t stream)
{
    if (epi) launch_pixel_list(LightfieldRays<true>{lf, a, b}, first, n, rays, stream);
    else launch_pixel_list(LightfieldRays<false>{lf, a, b}, first, n, rays, stream);
}

void hr_launch_rayset_batch(const HrRaySetArgs& a, hipStream_t stream)
{
    static void (*const k[2])(HrRaySetArgs) = {hr_rayset_batch_kernel<false>, hr_rayset_batch_kernel<true>};
    launch_rayset(k, a, stream, a);
}

void hr_launch_rayset_sample(const HrRaySetArgs& a, uint64_t seed, uint64_t step, const uint64_t* step_dev, hipStream_t stream)
{
    static void (*const k[2])(HrRaySetArgs, uint64_t, uint64_t, const uint64_t*) = {hr_rayset_sample_kernel<false>, hr_rayset_sample_kernel<true>};
    launch_rayset(k, a, stream, a, seed, step, step_dev);
}
