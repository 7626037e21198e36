// Two-plane light-field arithmetic shared by the ray kernels (rays_kernel.hip: hr_generate_rays_lightfield, hr_generate_rays_epi,
// hr_rayset_batch on a light-field set) and, compiled by the host compiler, by the CPU suite (tests/host_math/hr_lightfield_host.cpp):
//   hr_linspace          element i of torch.linspace(start, end, steps, dtype=float32) as the CPU kernel forms it
//   hr_lightfield_ray    pixel (x, y) of the view at camera-plane position (s, t)        (get_lightfield_rays, utils/ray_utils.py:14-45)
//   hr_epi_ray           pixel (x, j) of the epipolar slice (u, s) at a fixed (v, t)      (get_epi_rays, utils/ray_utils.py:47-78)
// Every operation is the reference's float32 operation, in its order; IEEE division and square root.  The library is built with
// -ffp-contract=off, the host restatement too: the only fused multiply-adds are the two written out in hr_linspace.
#ifndef HR_LIGHTFIELD_H
#define HR_LIGHTFIELD_H

#include <math.h>
#include <stdint.h>

#include "../../include/hyperreel_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HR_LF_FN __host__ __device__ __forceinline__
#else
#define HR_LF_FN static inline
#endif

// torch.linspace on the CPU (ATen/native/cpu/RangeFactoriesKernel.cpp): step = (end - start) / (steps - 1) in float32; the first half
// steps from the start, start + step * i, the second half from the end, end - step * (steps - 1 - i), so that both ends are exact and
// the list is symmetric.  Each is ONE rounding: the shipped CPU kernels contract the multiply and the add (measured: with an explicit
// fma every element of every size tried is reproduced bit for bit; with two roundings about 40 % of the elements are 1/2 ulp off).
// steps == 1: [start].
HR_LF_FN float hr_linspace(float start, float end, int steps, int i)
{
    if (steps == 1) return start;
    const float step = (end - start) / (float)(steps - 1);
    return i < steps / 2 ? fmaf(step, (float)i, start) : fmaf(-step, (float)(steps - 1 - i), end);
}

// origin (os, ot, near) on the camera plane, through (u, v, far) on the image plane: stack, then F.normalize(p=2, eps=1e-12) of the
// direction.  far - near is a Python number in the reference (double arithmetic, rounded once when it meets the float32 tensor).
HR_LF_FN void hr_two_plane_ray(const hr_lightfield& lf, float os, float ot, float u, float v, float* out)
{
    const float dx = u - os, dy = v - ot;
    const float dz = (float)((double)lf.far - (double)lf.near);
    const float nrm = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-12f);
    out[0] = os; out[1] = ot; out[2] = lf.near;
    out[3] = dx / nrm; out[4] = dy / nrm; out[5] = dz / nrm;
}

// u = linspace(-1, 1, U)[x] * uv_scale, v = linspace(1, -1, V)[y] / aspect * uv_scale, origin (s * st_scale, t * st_scale, near)
HR_LF_FN void hr_lightfield_ray(const hr_lightfield& lf, float s, float t, int x, int y, float* out)
{
    const float u = hr_linspace(-1.0f, 1.0f, lf.width, x) * lf.uv_scale;
    const float v = hr_linspace(1.0f, -1.0f, lf.height, y) / lf.aspect * lf.uv_scale;
    hr_two_plane_ray(lf, s * lf.st_scale, t * lf.st_scale, u, v, out);
}

// width = U, height = S: u as above, s = linspace(-1, 1, S)[j] / aspect * st_scale; v * uv_scale and t * st_scale are the call's constants
HR_LF_FN void hr_epi_ray(const hr_lightfield& lf, float v, float t, int x, int j, float* out)
{
    const float u = hr_linspace(-1.0f, 1.0f, lf.width, x) * lf.uv_scale;
    const float s = hr_linspace(-1.0f, 1.0f, lf.height, j) / lf.aspect * lf.st_scale;
    hr_two_plane_ray(lf, s, t * lf.st_scale, u, v * lf.uv_scale, out);
}

#endif  // HR_LIGHTFIELD_H
