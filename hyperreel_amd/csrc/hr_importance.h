// Arithmetic of the importance subsample rule (datasets/immersive.py:295-310, datasets/neural_3d.py:191-204), shared by the kernels of
// importance_kernel.hip and, compiled by the host compiler, by the CPU suite (tests/host_math/hr_importance_host.cpp):
//   hr_importance_diff   torch.abs(rgb - last_rgb).mean(-1) of one pixel, from the two images' bytes, bit for bit
//   hr_importance_key    the diff's bit pattern: diffs are non-negative and finite, so unsigned order is float order
//   hr_importance_rank   the ascending rank whose value is the rule's threshold, diff_sorted[-num_take]
// The rule keeps a pixel when its diff is strictly greater than the threshold (and, for Immersive, when its ray's d_z lies below a
// limit: that test needs the camera and is the kernels').
#ifndef HR_IMPORTANCE_H
#define HR_IMPORTANCE_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HR_IMP_FN __host__ __device__ __forceinline__
#else
#define HR_IMP_FN static inline
#endif

// The reference evaluates the rule on the CPU on ToTensor's floats: x / 255 per channel, the difference, its absolute value, the
// mean over the last axis as ((a0 + a1) + a2) / 3.  Every operation is one float32 IEEE operation in this order; the last is a true
// division.  No contraction, no reassociation, whatever the translation unit's flags say.
HR_IMP_FN float hr_importance_diff(const uint8_t cur[3], const uint8_t prev[3])
{
#pragma clang fp contract(off)
#pragma clang fp reassociate(off)
#pragma clang fp reciprocal(off)
    const float a0 = fabsf((float)cur[0] / 255.0f - (float)prev[0] / 255.0f);
    const float a1 = fabsf((float)cur[1] / 255.0f - (float)prev[1] / 255.0f);
    const float a2 = fabsf((float)cur[2] / 255.0f - (float)prev[2] / 255.0f);
    return ((a0 + a1) + a2) / 3.0f;
}

HR_IMP_FN uint32_t hr_importance_key(const uint8_t cur[3], const uint8_t prev[3])
{
    const float d = hr_importance_diff(cur, prev);
    uint32_t k;
    memcpy(&k, &d, 4);
    return k;
}

HR_IMP_FN float hr_importance_key_value(uint32_t key)
{
    float d;
    memcpy(&d, &key, 4);
    return d;
}

// 1 <= num_take <= n_pixels.  (num_take == 0 is not a rank: in the reference diff_sorted[-0] is diff_sorted[0], the minimum, and the
// rule silently keeps nearly every pixel; every caller refuses it.)
HR_IMP_FN int64_t hr_importance_rank(int64_t n_pixels, int64_t num_take) { return n_pixels - num_take; }

#endif  // HR_IMPORTANCE_H
