// The draw of hr_rayset_sample (rays_kernel.hip): which set element row j of training step s is.  Plain C++ that also compiles for the
// host: the CPU suite builds it (tests/host_math/hr_sample_rng_host.cpp) and compares it with a numpy restatement of the definition.
//
// Counter-based, so that a row needs no state and no neighbour: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as
// easy as 1, 2, 3", SC'11) with key = (seed low word, seed high word) and counter = (j low, j high, s low, s high).  Words 0 and 1 of the
// output form a 64-bit draw u (word 1 the high half); the element is floor(u * size / 2^64), the high 64 bits of the 128-bit product.
// That map sends floor(2^64 / size) or one more values of u to each element: the probabilities differ from 1 / size by less than
// 2^-64, a relative bias below size / 2^64 (5e-11 for a set of 2^30 rays).
//
// It replaces RandomSampler(replacement=True) (nlf/__init__.py:222-230) and does not reproduce torch's stream: the contract is
// "uniform and independent over [0, size), fixed by (seed, step, row)".
#ifndef HR_SAMPLE_RNG_H
#define HR_SAMPLE_RNG_H

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HR_RNG_FN __host__ __device__ __forceinline__
#else
#define HR_RNG_FN static inline
#endif

struct HrPhilox {
    uint32_t w[4];
};

HR_RNG_FN HrPhilox hr_philox4x32_10(uint64_t key, uint64_t ctr_lo, uint64_t ctr_hi)
{
    uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    uint32_t c0 = (uint32_t)ctr_lo, c1 = (uint32_t)(ctr_lo >> 32), c2 = (uint32_t)ctr_hi, c3 = (uint32_t)(ctr_hi >> 32);
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0;
        c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;              // (the bump after the last round is never read)
    }
    HrPhilox out;
    out.w[0] = c0; out.w[1] = c1; out.w[2] = c2; out.w[3] = c3;
    return out;
}

// high 64 bits of a * b
HR_RNG_FN uint64_t hr_mulhi64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// the 64-bit draw of (seed, step, row)
HR_RNG_FN uint64_t hr_sample_draw(uint64_t seed, uint64_t step, uint64_t row)
{
    const HrPhilox r = hr_philox4x32_10(seed, row, step);
    return ((uint64_t)r.w[1] << 32) | r.w[0];
}

// element of [0, size) that row `row` of step `step` reads; size >= 1
HR_RNG_FN uint64_t hr_sample_element(uint64_t size, uint64_t seed, uint64_t step, uint64_t row)
{
    return hr_mulhi64(hr_sample_draw(seed, step, row), size);
}

// The background coin of training step `step` (the reference composites a training step over white with probability 1/2,
// tensorf_no_sample.py:236: `white_bg or (training and rand() < 0.5)`): one Philox word of (seed, step), white iff its top bit is set.
// The sampler's rows of the same (seed, step) use counters (row, step) with row < 2^63; the coin's counter carries a constant no row
// reaches in that place, so the coin is independent of every ray the step draws.
#define HR_BG_COIN_DOMAIN 0xB6C01DC01DB6C01Dull

HR_RNG_FN int hr_background_coin(uint64_t seed, uint64_t step)
{
    return (int)(hr_philox4x32_10(seed, HR_BG_COIN_DOMAIN, step).w[0] >> 31);
}

#endif  // HR_SAMPLE_RNG_H
