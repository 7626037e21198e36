// Camera arithmetic shared by the ray kernels (rays_kernel.hip: the pixel-list kernel behind hr_generate_rays, hr_generate_rays_ndc and
// hr_generate_rays_fisheye, and hr_rayset_batch / hr_rayset_sample) and, compiled by the host compiler, by the CPU suite
// (tests/host_math/hr_camera_host.cpp, hr_fisheye_host.cpp; tests/test_camera_pin.py pins the bits):
//   hr_pixel_plane, hr_camera_to_world, hr_world_to_ndc   the one camera pipeline's stages
//   hr_pixel_ray        pixel + camera -> the ray the reference's dataset stores (pinhole, optionally NDC)
//   hr_pixel_ray_fisheye  the same for a fisheye camera's own pixel: hr_fisheye_undistort first (Immersive's training rays)
//   hr_subsample_*      the k-th pixel of the checkerboard rule (x + y + offset) % every == 0, in closed form
//   hr_perm             a keyed bijection of [0, n): the epoch's order
// IEEE division and square root throughout: these values feed the intersections, whose comparisons must fall as the reference's.
// The library is built with -ffp-contract=off, the host restatement too: no multiply is fused with an add.
#ifndef HR_CAMERA_H
#define HR_CAMERA_H

#include <math.h>
#include <stdint.h>

#include "../../include/hyperreel_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HR_CAM_FN __host__ __device__ __forceinline__
#else
#define HR_CAM_FN static inline
#endif

// Camera -> ray in the stages it has, each written once; hr_pixel_ray and hr_pixel_ray_lens below only chain them.
// Stage 1, pixel -> camera plane (utils/ray_utils.py:98-135, datasets/base.py:485-518): pixel centres +0.5, directions (x, -y, -1) / focal.
HR_CAM_FN void hr_pixel_plane(const hr_camera& cam, int x, int y, float* dx, float* dy)
{
    const float i = (float)x, j = (float)y;
    *dx = (i - cam.cx + 0.5f) / cam.fx;
    *dy = -(j - cam.cy + 0.5f) / cam.fy;
}

// Stage 2, camera-space direction -> world ray (get_rays, utils/ray_utils.py:117-135): rotated by the pose, normalised; origin = pose
// translation.  out[0..2] origin, out[3..5] direction.
HR_CAM_FN void hr_camera_to_world(const hr_camera& cam, float dx, float dy, float dz, float* out)
{
    float wx = dx * cam.c2w[0] + dy * cam.c2w[1] + dz * cam.c2w[2];
    float wy = dx * cam.c2w[4] + dy * cam.c2w[5] + dz * cam.c2w[6];
    float wz = dx * cam.c2w[8] + dy * cam.c2w[9] + dz * cam.c2w[10];
    const float nrm = fmaxf(sqrtf(wx * wx + wy * wy + wz * wz), 1e-12f);   // F.normalize(p=2, eps=1e-12)
    wx = wx / nrm; wy = wy / nrm; wz = wz / nrm;
    out[0] = cam.c2w[3]; out[1] = cam.c2w[7]; out[2] = cam.c2w[11];
    out[3] = wx; out[4] = wy; out[5] = wz;
}

// Stage 3, world ray -> NDC ray, in place: get_ndc_rays_fx_fy (utils/ray_utils.py:137-164) in its operation order, with the DATASET's
// W, H, fx, fy, near (datasets/technicolor.py:355-358), which need not be the frame's.  The two scalar factors -1 / (W / (2 fx)) are
// Python floats in the reference (double arithmetic, rounded once when they meet the float32 tensor), so they are formed in double here.
HR_CAM_FN void hr_world_to_ndc(const hr_ndc* ndc, float* ray)
{
    const float wx = ray[3], wy = ray[4], wz = ray[5];
    const float sx = (float)(-1.0 / ((double)ndc->width / (2.0 * (double)ndc->fx)));
    const float sy = (float)(-1.0 / ((double)ndc->height / (2.0 * (double)ndc->fy)));
    const float t = -(ndc->near + ray[2]) / wz;               // shift the origin to the near plane
    const float ox = ray[0] + t * wx, oy = ray[1] + t * wy, oz = ray[2] + t * wz;
    const float ox_oz = ox / oz, oy_oz = oy / oz;
    const float o2 = 1.0f + (2.0f * ndc->near) / oz;
    ray[0] = sx * ox_oz;
    ray[1] = sy * oy_oz;
    ray[2] = o2;
    ray[3] = sx * (wx / wz - ox_oz);
    ray[4] = sy * (wy / wz - oy_oz);
    ray[5] = 1.0f - o2;
}

// The pinhole camera: plane -> world (dx, dy, -1) -> NDC when `ndc` is given.
HR_CAM_FN void hr_pixel_ray(const hr_camera& cam, const hr_ndc* ndc, int x, int y, float* out)
{
    float dx, dy;
    hr_pixel_plane(cam, x, y, &dx, &dy);
    hr_camera_to_world(cam, dx, dy, -1.0f, out);
    if (ndc) hr_world_to_ndc(ndc, out);
}

// ---- fisheye cameras (datasets/immersive.py:43-48, 514-564): the equidistant model theta_d = theta (1 + k1 theta^2 + k2 theta^4),
// inverted per pixel as cv2.fisheye.undistortPoints(K = I, D = (k1, k2, 0, 0)) does for the reference.  The contract is the inverse
// itself, so the solver is ours: Newton from theta = theta_d, a fixed count, every lane the same instructions.

// The model has an inverse on [0, pi / 2] when theta_d(theta) increases there: 1 + 3 k1 u + 5 k2 u^2 > 0 for u = theta^2 in
// [0, (pi / 2)^2].  A quadratic in u that is 1 at u = 0: its minimum is at the far end or, when it opens upwards, at its vertex.
HR_CAM_FN bool hr_fisheye_invertible(float k1, float k2)
{
    if (!isfinite(k1) || !isfinite(k2)) return false;
    const double a = 5.0 * (double)k2, b = 3.0 * (double)k1, U = 1.5707963267948966 * 1.5707963267948966;
    if (1.0 + b * U + a * U * U <= 0.0) return false;
    if (a > 0.0) {
        const double u = -b / (2.0 * a);
        if (u > 0.0 && u < U && 1.0 + b * u + a * u * u <= 0.0) return false;
    }
    return true;
}

// Float32 Newton steps on theta (1 + k1 theta^2 + k2 theta^4) - theta_d from theta = theta_d.  The float32 iterate never comes to
// rest -- the residual is a difference of two nearly equal numbers, so every further step keeps moving some iterates by up to 3 ulp --
// but its largest distance to the root stops shrinking: over theta_d in [0, 1.3] and the pairs the tests use that happens after 3
// steps (2.2e-1, 1.0e-2, 2.7e-5, 1.66e-7, 1.57e-7, 1.52e-7, 1.57e-7, ... for (0.2, -0.02), the slowest; single iterates still gain
// fractions of an ulp until the 5th).  6 steps: the margin is for invertible pairs stronger than those, and costs nothing in a
// launch-bound kernel (tests/test_fisheye_host.py prints the table).
#define HR_FISHEYE_NEWTON_STEPS 6

HR_CAM_FN float hr_fisheye_theta(float k1, float k2, float theta_d, int steps)
{
    float th = theta_d;
    for (int i = 0; i < steps; ++i) {
        const float t2 = th * th, t4 = t2 * t2;
        const float f = th * (1.0f + k1 * t2 + k2 * t4) - theta_d;
        const float fp = 1.0f + 3.0f * k1 * t2 + 5.0f * k2 * t4;
        th = th - f / fp;
    }
    return th;
}

// tan on [0, pi / 2) out of IEEE operations alone.  tanf would be libm's on the host and the device library's in a kernel: two
// functions that round differently, where the CPU suite's build of this header has to give the kernels' bits.  On [0, pi / 4]
// tan x = x + x^3 P(x^2), P a degree-6 minimax fit of (tan x - x) / x^3 (relative error of tan 1.3e-9 before rounding); above,
// 1 / tan(pi / 2 - x) with pi / 2 in two pieces (the subtraction of the first is exact there).  Within 3 ulp of tan on [0, 1.55].
HR_CAM_FN float hr_tan_quadrant(float x)
{
    const bool flip = x > 0.785398163f;
    const float a = flip ? (1.5707963705062866f - x) + -4.371138828673793e-08f : x;
    const float z = a * a;
    float p = 0.004376267548650503f;
    p = p * z + 8.95429911906831e-05f;
    p = p * z + 0.010835813358426094f;
    p = p * z + 0.02128218486905098f;
    p = p * z + 0.054059918969869614f;
    p = p * z + 0.13332663476467133f;
    p = p * z + 0.33333349227905273f;
    const float t = a + (a * z) * p;
    return flip ? 1.0f / t : t;
}

// (dx, dy) on the distorted image plane -> (dx', dy') on the pinhole one.  A point within 1e-8 of the axis is returned unchanged, as
// OpenCV returns it (a factor of exactly 1: the same bits, and no branch).
HR_CAM_FN void hr_fisheye_undistort(float k1, float k2, float dx, float dy, float* ox, float* oy)
{
    const float theta_d = sqrtf(dx * dx + dy * dy);
    const float theta = hr_fisheye_theta(k1, k2, theta_d, HR_FISHEYE_NEWTON_STEPS);
    const bool on_axis = theta_d <= 1e-8f;
    const float s = on_axis ? 1.0f : hr_tan_quadrant(theta) / theta_d;
    *ox = s * dx;
    *oy = s * dy;
}

// hr_pixel_ray for a fisheye camera's own pixel: plane -> hr_fisheye_undistort -> normalise -> world -> NDC when `ndc` is given.  The
// undistorted direction (dx', dy', -1) is normalised before get_rays rotates and normalises it again (immersive.py:550-558), which the
// pinhole path never does.  hr_pixel_ray_lens always undistorts; hr_pixel_ray_fisheye adds the interface's convention that a NULL or
// all-zero hr_fisheye means "no distortion given": the pinhole camera, hr_pixel_ray's bits (include/hyperreel_hip.h; the model itself
// would make (0, 0) the lens theta_d = theta).
HR_CAM_FN void hr_pixel_ray_lens(const hr_camera& cam, const hr_fisheye& fe, const hr_ndc* ndc, int x, int y, float* out)
{
    float dx, dy, dz = -1.0f;
    hr_pixel_plane(cam, x, y, &dx, &dy);
    hr_fisheye_undistort(fe.k1, fe.k2, dx, dy, &dx, &dy);
    const float n0 = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-12f);     // F.normalize of the camera-space direction
    dx = dx / n0; dy = dy / n0; dz = dz / n0;
    hr_camera_to_world(cam, dx, dy, dz, out);
    if (ndc) hr_world_to_ndc(ndc, out);
}

HR_CAM_FN void hr_pixel_ray_fisheye(const hr_camera& cam, const hr_fisheye* fe, const hr_ndc* ndc, int x, int y, float* out)
{
    if (fe && (fe->k1 != 0.0f || fe->k2 != 0.0f)) hr_pixel_ray_lens(cam, *fe, ndc, x, y, out);
    else hr_pixel_ray(cam, ndc, x, y, out);
}

// ---- checkerboard subsampling (datasets/technicolor.py:211-236, datasets/neural_3d.py:168-185): pixel (x, y) is kept when
// (x + y + offset) % every == 0.  For a fixed x exactly one of `every` consecutive rows keeps it, so every block of `every` rows
// holds exactly w kept pixels.  Within a block that starts at a row whose first kept column is c = (-(y0 + offset)) mod every, row r
// keeps the columns (c - r) mod every, + every, ...: w / every of them, one more when (c - r) mod every < w % every.

// kept pixels in rows [0, r) of such a block, r <= every
HR_CAM_FN int64_t hr_subsample_block_rows(int w, int every, int c, int r)
{
    const int q = w / every, rem = w % every;
    const int lo = c - rem + 1 > 0 ? c - rem + 1 : 0;               // rows 0 .. c: first column c - s, below rem from s = c - rem + 1 on
    const int hi = r < c + 1 ? r : c + 1;
    const int a = hi > lo ? hi - lo : 0;
    const int b = r - (every + c - rem + 1);                        // rows c + 1 .. : first column every + c - s
    return (int64_t)r * q + a + (b > 0 ? b : 0);
}

HR_CAM_FN int hr_subsample_first_col(int y, int every, int offset)
{
    return (every - (int)(((int64_t)y + offset) % every)) % every;
}

HR_CAM_FN int64_t hr_subsample_count(int w, int h, int every, int offset)
{
    const int full = h / every, y0 = full * every;
    return (int64_t)full * w + hr_subsample_block_rows(w, every, hr_subsample_first_col(y0, every, offset), h - y0);
}

// the k-th kept pixel in row-major order, k < hr_subsample_count
HR_CAM_FN void hr_subsample_pixel(int w, int h, int every, int offset, int64_t k, int* x, int* y)
{
    (void)h;
    const int64_t blk = k / w;
    const int64_t kk = k - blk * w;
    const int y0 = (int)blk * every;
    const int c = hr_subsample_first_col(y0, every, offset);
    int lo = 0, hi = every - 1;                                      // the last row r of the block with block_rows(r) <= kk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (hr_subsample_block_rows(w, every, c, mid) <= kk) lo = mid; else hi = mid - 1;
    }
    *y = y0 + lo;
    *x = (c - lo + every) % every + (int)(kk - hr_subsample_block_rows(w, every, c, lo)) * every;
}

// ---- the epoch's order: a keyed bijection of [0, n), n < 2^63.  A 4-round Feistel network over the next even number of bits
// (a bijection of [0, 2^2b) whatever the round function is), cycle-walked into [0, n): 2^2b < 4 n, so a walk takes fewer than
// four steps on average.  It replaces np.random.permutation(len(self)) per epoch (datasets/base.py:202-227); it does not
// reproduce numpy's stream -- the contract is "every element exactly once per epoch, order set by (seed, epoch)".
HR_CAM_FN uint64_t hr_mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

HR_CAM_FN uint64_t hr_perm_key(uint64_t seed, uint64_t epoch)
{
    return hr_mix64(hr_mix64(seed + 0x9e3779b97f4a7c15ull) ^ (epoch + 0x7f4a7c159e3779b9ull));
}

HR_CAM_FN uint64_t hr_perm(uint64_t n, uint64_t key, uint64_t i)
{
    if (n <= 1) return 0;
    const int bits = 64 - __builtin_clzll(n - 1);
    const int hb = (bits + 1) >> 1;                                   // bits of one half, 1 .. 32
    const uint64_t mask = (1ull << hb) - 1;
    uint64_t x = i;
    do {
        uint64_t l = x >> hb, r = x & mask;
        for (int round = 0; round < 4; ++round) {
            const uint64_t f = hr_mix64(r + key * (uint64_t)(2 * round + 1) + (uint64_t)round) >> 32;
            const uint64_t t = l ^ (f & mask);
            l = r;
            r = t;
        }
        x = (l << hb) | r;
    } while (x >= n);
    return x;
}

#endif  // HR_CAMERA_H
