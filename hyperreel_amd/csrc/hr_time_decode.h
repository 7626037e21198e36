// The keyframe net's time-dependent decode modes: `shadingMode: RGBtLinear | RGBtFourier | RGBIdentity`
// (utils/tensorf_utils.py:346-400) and `densityMode: DensityLinear | DensityFourier` (:407-456, tensorf_dynamic.py:327-330, 373-392).
// The definitions, once: the sample kernel of these models (sample_time_kernel.hip), hr_model_set_time_decode (api_model.hip) and the
// CPU suite (tests/host_math/hr_time_decode_host.cpp) compile this file as it is.
//
// The features after basis_mat (colour: 3 nb of them, row c * nb + j; density: nb of basis_mat_density) are COEFFICIENTS of a basis of
// nb functions of the ray's time t (rays[..., -1]) and of its offset from the keyframe before it (AdvectPointsEmbedding,
// nlf/embedding/point.py:797-825: both are per ray, repeated over the samples):
//   Linear   [1, t]                                                     nb = 2
//   Fourier  [t, cos(2 pi f s) f = 0 .. fpk - 1, sin(2 pi f s) ...]     nb = 2 fpk + 1,   s = time_offset * K (F - 1) / F
// (K keyframes, F frames; fpk = net.frames_per_keyframe, else F // K: tensorf_dynamic.py:51-55).  The frequency-0 terms are a constant
// 1 and a constant 0: kept, the checkpoint carries their weights.
//   colour c = relu(sum_j basis_j * feature[c nb + j] + 0.5)           RGBIdentity: |feature[c] + 0.5|, no basis
//   density feature = sum_j basis_j * (basis_mat_density . comps)_j
// Both are linear in the features, so the basis folds into what the ray multiplies its gathered components with: the decode matrix
// M[c][ch] = sum_j basis_j * basis_mat[c nb + j][ch] (SH's form with another per-ray vector) and a density row
// m_d[ch] = sum_j basis_j * basis_mat_density[j][ch] in the place of the row of ones.
#ifndef HR_TIME_DECODE_H
#define HR_TIME_DECODE_H

#include "hr_math.h"

// HR_TIME_MAX_FPK (the public header): frames_per_keyframe the kernels accept, 1 .. 8 -- the shipped video datasets have 50 // 12 = 4
// (technicolor) and 4 (neural_3d, immersive at their keyframe counts); 8 doubles that.  Stated again in plan.py (TIME_MAX_FPK).
#define HR_TIME_MAX_NB (2 * HR_TIME_MAX_FPK + 1)

HR_HD bool hr_shading_is_time(int shading) { return shading == HR_SHADING_RGBT_LINEAR || shading == HR_SHADING_RGBT_FOURIER; }
// a shading the stand-alone sample kernel and the frame kernel do not know: the time kernel's
HR_HD bool hr_shading_is_time_family(int shading) { return hr_shading_is_time(shading) || shading == HR_SHADING_RGB_IDENTITY; }
// the colour modes whose activation is relu(x + 0.5)
HR_HD bool hr_shading_relu_half(int shading) { return shading == HR_SHADING_SH || hr_shading_is_time(shading); }

// basis functions: fourier 0 = Linear, 1 = Fourier
HR_HD int hr_time_nb(int fourier, int fpk) { return fourier ? 2 * fpk + 1 : 2; }
// rows of basis_mat: 3 nb for the RGBt modes (features.view(-1, 3, nb)), -1 for a shading without a time basis
HR_HD int hr_time_app_dim(int shading, int fpk)
{
    if (shading == HR_SHADING_RGBT_LINEAR) return 6;
    if (shading == HR_SHADING_RGBT_FOURIER) return 3 * (2 * fpk + 1);
    return -1;
}
// time_scale_factor of RGBtFourierRender / DensityFourierRender (tensorf_utils.py:376, 432): formed in double by Python, then a float32
// factor of a float32 tensor
HR_HD float hr_time_scale(int num_keyframes, int num_frames)
{
    return num_frames > 0 ? (float)((double)num_keyframes * (double)(num_frames - 1) / (double)num_frames) : 0.0f;
}

// basis function j of a ray (t, time_offset); fac = hr_time_scale.  The argument follows the reference's float32 products in its order,
// ((s f) 2) pi with pi rounded to float32 (`time_offset * freqs * 2 * np.pi`).  |s| <= 0.5 between keyframes (get_base_time rounds
// to the nearest one, utils/flow_utils.py:10-35) and at most K (F - 1) / F - (K - 1) < 1 behind the last one (t = 1), so
// |argument| < 2 pi (fpk - 1) <= 44 rad at the cap: sinf / cosf in their IEEE forms (libm on the host, OCML on the device: <= 2 ulp
// over that range, a full argument reduction) -- the hardware's v_sin_f32 / v_cos_f32 lose ~1e-6 absolute, a tenth of what the
// colours may differ by, and are evaluated once per ray and slot: nothing to gain.
HR_HD float hr_time_basis(int fourier, int fpk, float t, float time_offset, float fac, int j)
{
    if (!fourier) return j == 0 ? 1.0f : t;
    if (j == 0) return t;
    const bool is_cos = j <= fpk;
    const float f = (float)(is_cos ? j - 1 : j - 1 - fpk);
    const float x = ((time_offset * fac) * f) * 2.0f * 3.14159265358979323846f;
    return is_cos ? cosf(x) : sinf(x);
}

// sum_j basis_j * b[j * stride]: one folded entry (b: column `ch` of a (rows, cols) matrix, or nb contiguous rows of its transpose)
HR_HD float hr_time_fold(int fourier, int fpk, float t, float time_offset, float fac, const float* b, int stride)
{
    if (!fourier) return __builtin_fmaf(t, b[stride], b[0]);
    float v = t * b[0];
    const float s2 = (time_offset * fac);
    for (int f = 0; f < fpk; ++f) {
        const float x = (s2 * (float)f) * 2.0f * 3.14159265358979323846f;
        v = __builtin_fmaf(cosf(x), b[(1 + f) * stride], v);
        v = __builtin_fmaf(sinf(x), b[(1 + fpk + f) * stride], v);
    }
    return v;
}

// the colour of a sample from the decode sums of a time-family or plain shading
HR_HD float hr_time_color(int shading, float pre)
{
    if (shading == HR_SHADING_RGB_IDENTITY) return fabsf(pre + 0.5f);      // RGBIdentityRender, tensorf_utils.py:346-348
    return fmaxf(pre + 0.5f, 0.0f);                                         // RGBtLinearRender / RGBtFourierRender, :367, 398
}

#endif  // HR_TIME_DECODE_H
