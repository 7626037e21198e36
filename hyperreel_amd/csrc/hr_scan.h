// Sums over a wavefront and over a workgroup, for the kernels that lay out a file or a list by prefix sums (png_kernel.hip,
// jpeg_encode_kernel.hip, importance_kernel.hip).  Device code only.
#ifndef HR_SCAN_H
#define HR_SCAN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint32_t hr_wave_sum(uint32_t v)
{
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// inclusive sum over the workgroup's N threads (Hillis-Steele in LDS); s[N - 1] holds the total on return
template <int N>
__device__ __forceinline__ uint32_t hr_block_scan_inclusive(uint32_t v, uint32_t* s)
{
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int off = 1; off < N; off <<= 1) {
        const uint32_t add = t >= off ? s[t - off] : 0u;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    return s[t];
}

#endif
