// The importance subsample rule on the device (hr_rayset_set_image_importance; arithmetic: hr_importance.h, hr_camera.h): for one image
// of a training set and the image before it in its video, both in the set's pixel store,
//   1. threshold: an exact radix select of the key (the diff's bit pattern) at ascending rank n_pixels - num_take -- four 8-bit digit
//      passes from the top, each a per-workgroup LDS histogram merged into a 256-bin global one by integer atomics, each followed by a
//      one-workgroup step that picks the digit holding the rank and narrows (prefix, remaining rank).  No sort, no host round trip.
//      The keys are recomputed from the bytes in every pass (6 bytes a pixel): no W x H word buffer exists.
//   2. mask: key > threshold (strict), and with a direction limit the pixel's ray -- hr_pixel_ray_fisheye with the image's camera, lens
//      and the set's NDC, the function rayset_write_row emits -- has v[5] < dir_z_below.  The ray is evaluated only where the key passes.
//   3. stable compaction: per-workgroup counts, an exclusive scan of the counts (one workgroup, chunks of 256 with a carry: any number of
//      workgroups), and a scatter.  A workgroup owns HR_IMP_TILE consecutive pixels; inside it the order comes from the 64-bit __ballot
//      and the popcount of the lower lanes, the wavefronts' counts and the running count of the earlier rounds: no cursor, no atomics.
// Integer atomics only: the list is the same on every run.  Bandwidth is not at stake (1280 x 960: 7.4 MB a pass, L2-resident after the
// first); the call is a handful of short launches beside the image's host-to-device copy.
#include "hr_camera.h"
#include "hr_importance.h"
#include "hr_kernels.h"
#include "hr_scan.h"

namespace {

constexpr int THREADS = 256;
constexpr int ITEMS = HR_IMP_TILE / THREADS;      // rounds of a workgroup over its tile

__device__ __forceinline__ uint32_t pixel_key(const HrImportanceArgs& a, uint32_t p)
{
    return hr_importance_key(a.cur + (size_t)p * 3, a.prev + (size_t)p * 3);
}

// digit pass PASS (0: bits 31..24): histogram of the digit over the keys whose higher digits equal the prefix found so far
template <int PASS>
__global__ __launch_bounds__(THREADS) void importance_hist_kernel(const HrImportanceArgs a)
{
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    constexpr int shift = 24 - 8 * PASS;
    const uint32_t n = (uint32_t)a.width * (uint32_t)a.height;
    const uint32_t prefix = PASS ? a.workspace[HR_IMP_WS_PREFIX] : 0u;
    for (uint32_t p = blockIdx.x * THREADS + threadIdx.x; p < n; p += gridDim.x * THREADS) {
        const uint32_t key = pixel_key(a, p);
        if (PASS == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&h[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    const uint32_t c = h[threadIdx.x];
    if (c) atomicAdd(&a.workspace[HR_IMP_WS_HIST + PASS * 256 + threadIdx.x], c);
}

// one workgroup: the digit d with  #(digits < d) <= rank < #(digits <= d)  joins the prefix; the rank becomes the rank among its keys
__global__ __launch_bounds__(THREADS) void importance_narrow_kernel(uint32_t* __restrict__ ws, int pass, uint32_t rank0)
{
    __shared__ uint32_t s[THREADS];
    const uint32_t c = ws[HR_IMP_WS_HIST + pass * 256 + threadIdx.x];
    const uint32_t rank = pass ? ws[HR_IMP_WS_RANK] : rank0;
    const uint32_t prefix = pass ? ws[HR_IMP_WS_PREFIX] : 0u;
    const uint32_t incl = hr_block_scan_inclusive<THREADS>(c, s);
    if (incl - c <= rank && rank < incl) {               // exactly one thread: the counts sum to more than the rank
        ws[HR_IMP_WS_RANK] = rank - (incl - c);
        ws[HR_IMP_WS_PREFIX] = (prefix << 8) | threadIdx.x;
        if (pass == 3) ws[HR_IMP_WS_THRESHOLD] = (prefix << 8) | threadIdx.x;
    }
}

// SCATTER false: counts[workgroup] = kept pixels of its tile.  SCATTER true: counts[] holds the exclusive scan; the kept pixels' indices
// go to list[] in ascending order
template <bool SCATTER>
__global__ __launch_bounds__(THREADS) void importance_compact_kernel(const HrImportanceArgs a)
{
    __shared__ uint32_t wave_count[THREADS / 64];
    uint32_t* __restrict__ counts = a.workspace + HR_IMP_WS_COUNTS;
    const uint32_t n = (uint32_t)a.width * (uint32_t)a.height;
    const uint32_t threshold = a.workspace[HR_IMP_WS_THRESHOLD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t running = SCATTER ? counts[blockIdx.x] : 0u;
    for (int j = 0; j < ITEMS; ++j) {
        const uint32_t p = blockIdx.x * (uint32_t)HR_IMP_TILE + (uint32_t)(j * THREADS) + threadIdx.x;
        bool keep = p < n && pixel_key(a, p) > threshold;
        if (keep && a.has_dir) {
            float v[8];
            hr_pixel_ray_fisheye(a.image.cam, a.image.has_fe ? &a.image.fe : nullptr, a.has_ndc ? &a.ndc : nullptr, (int)(p % (uint32_t)a.width),
                                 (int)(p / (uint32_t)a.width), v);
            keep = v[5] < a.dir_z_below;
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_count[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) {
            const uint32_t c = wave_count[w];
            total += c;
            if (w < wave) before += c;
        }
        if (SCATTER && keep) {
            const uint32_t pos = running + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (pos < a.list_cap) a.list[pos] = p;         // (never beyond: strictly above the num_take-th largest leaves num_take - 1 at most)
        }
        running += total;
        __syncthreads();
    }
    if (!SCATTER && threadIdx.x == 0) counts[blockIdx.x] = running;
}

// one workgroup: counts[] -> its exclusive scan in place, in chunks of 256 with a carry; the total -> the 64-bit word at HR_IMP_WS_TOTAL
__global__ __launch_bounds__(THREADS) void importance_scan_kernel(uint32_t* __restrict__ ws, uint32_t n_counts)
{
    __shared__ uint32_t s[THREADS];
    uint32_t* __restrict__ counts = ws + HR_IMP_WS_COUNTS;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_counts; base += THREADS) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t c = i < n_counts ? counts[i] : 0u;
        const uint32_t incl = hr_block_scan_inclusive<THREADS>(c, s);
        if (i < n_counts) counts[i] = carry + incl - c;
        carry += s[THREADS - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) { ws[HR_IMP_WS_TOTAL] = carry; ws[HR_IMP_WS_TOTAL + 1] = 0u; }
}

// kept pixels [first, first + n) of an image as row-major indices: its list, or the checkerboard rule's closed form
__global__ __launch_bounds__(THREADS) void image_pixels_kernel(const uint32_t* __restrict__ list, int width, int height, int every, int offset,
                                                               int64_t first, int64_t n, int32_t* __restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (t >= n) return;
    if (list) {
        out[t] = (int32_t)list[first + t];
    } else {
        int x, y;
        hr_subsample_pixel(width, height, every, offset, first + t, &x, &y);
        out[t] = y * width + x;
    }
}

}  // namespace

size_t hr_importance_workspace_words(int64_t n_pixels) { return (size_t)HR_IMP_WS_COUNTS + (size_t)((n_pixels + HR_IMP_TILE - 1) / HR_IMP_TILE); }

hipError_t hr_launch_importance_select(const HrImportanceArgs& a, hipStream_t stream)
{
    const int64_t n = (int64_t)a.width * a.height;
    const unsigned tiles = (unsigned)((n + HR_IMP_TILE - 1) / HR_IMP_TILE);
    const unsigned hist_blocks = tiles < 2048u ? tiles : 2048u;       // a lane sees 4 pixels or more
    const hipError_t e = hipMemsetAsync(a.workspace, 0, sizeof(uint32_t) * HR_IMP_WS_COUNTS, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(importance_hist_kernel<0>, dim3(hist_blocks), dim3(THREADS), 0, stream, a);
    hipLaunchKernelGGL(importance_narrow_kernel, dim3(1), dim3(THREADS), 0, stream, a.workspace, 0, a.rank);
    hipLaunchKernelGGL(importance_hist_kernel<1>, dim3(hist_blocks), dim3(THREADS), 0, stream, a);
    hipLaunchKernelGGL(importance_narrow_kernel, dim3(1), dim3(THREADS), 0, stream, a.workspace, 1, a.rank);
    hipLaunchKernelGGL(importance_hist_kernel<2>, dim3(hist_blocks), dim3(THREADS), 0, stream, a);
    hipLaunchKernelGGL(importance_narrow_kernel, dim3(1), dim3(THREADS), 0, stream, a.workspace, 2, a.rank);
    hipLaunchKernelGGL(importance_hist_kernel<3>, dim3(hist_blocks), dim3(THREADS), 0, stream, a);
    hipLaunchKernelGGL(importance_narrow_kernel, dim3(1), dim3(THREADS), 0, stream, a.workspace, 3, a.rank);
    hipLaunchKernelGGL(importance_compact_kernel<false>, dim3(tiles), dim3(THREADS), 0, stream, a);
    hipLaunchKernelGGL(importance_scan_kernel, dim3(1), dim3(THREADS), 0, stream, a.workspace, tiles);
    hipLaunchKernelGGL(importance_compact_kernel<true>, dim3(tiles), dim3(THREADS), 0, stream, a);
    return hipGetLastError();
}

void hr_launch_image_pixels(const uint32_t* list, int width, int height, int every, int offset, int64_t first, int64_t n, int32_t* out,
                            hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(image_pixels_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, list, width, height, every,
                       offset, first, n, out);
}
