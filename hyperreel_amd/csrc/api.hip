// C ABI of libhyperreel_hip.so (declared in include/hyperreel_hip.h): error state, version, and the entry points that keep no model
// state.  The model's own entry points: api_model.hip (lifecycle), api_mlp.hip (packing, calibration), api_render.hip, api_train.hip.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <dlfcn.h>

#include "hr_mask.h"
#include "hr_model.h"

namespace {

thread_local char g_err[512] = "";

}  // namespace

int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hr_abi_version(void) { return HR_ABI_VERSION; }

int hr_sizeof_config(void) { return (int)sizeof(hr_config); }

const char* hr_last_error(void) { return g_err; }

int hr_shard_range(int64_t n_pixels, int32_t rank, int32_t world, int64_t* first, int64_t* count)
{
    if (!first || !count || world < 1 || rank < 0 || rank >= world || n_pixels < 0) return fail(HR_E_INVALID, "hr_shard_range: bad arguments");
    const int64_t base = n_pixels / world, extra = n_pixels % world;
    *first = (int64_t)rank * base + (rank < extra ? rank : extra);
    *count = base + (rank < extra ? 1 : 0);
    return HR_OK;
}

int hr_allgather_tiles(void* nccl_comm, const float* tile_dev, float* full_dev, int64_t floats_per_rank, void* stream)
{
    if (!nccl_comm || !tile_dev || !full_dev || floats_per_rank <= 0) return fail(HR_E_INVALID, "hr_allgather_tiles: null communicator / buffer or empty tile");
    // ncclResult_t ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t datatype, ncclComm_t comm, hipStream_t stream)
    typedef int (*allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
    static allgather_fn fn = nullptr;
    static bool looked = false;
    if (!looked) {
        looked = true;
        void* sym = dlsym(RTLD_DEFAULT, "ncclAllGather");        // the RCCL the process already uses (torch.distributed's, the integrator's)
        if (!sym) {
            for (const char* name : {"librccl.so.1", "librccl.so"}) {
                void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
                if (h && (sym = dlsym(h, "ncclAllGather"))) break;
            }
        }
        fn = reinterpret_cast<allgather_fn>(sym);
    }
    if (!fn) return fail(HR_E_HIP, "hr_allgather_tiles: no RCCL (ncclAllGather) in this process and librccl.so cannot be loaded");
    const int rc = fn(tile_dev, full_dev, (size_t)floats_per_rank, /* ncclFloat32 */ 7, nccl_comm, (hipStream_t)stream);
    if (rc != 0) return fail(HR_E_HIP, "ncclAllGather failed with ncclResult_t %d", rc);
    return HR_OK;
}

int hr_upsample_plane(const float* src_dev, int32_t channels, int32_t h, int32_t w, float* dst_dev, int32_t h2, int32_t w2, void* stream)
{
    if (channels < 0 || h < 1 || w < 1 || h2 < 1 || w2 < 1) return fail(HR_E_INVALID, "bad plane shape");
    if (channels > 0 && (!src_dev || !dst_dev)) return fail(HR_E_INVALID, "null plane");
    hr_launch_upsample_plane(src_dev, channels, h, w, dst_dev, h2, w2, (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

int hr_dense_alpha(hr_model* m, const int32_t n[3], float length, int32_t num_frames, const float* prev_volume_dev, const int32_t prev_n[3],
                   const float prev_aabb[6], float* alpha_dev, void* stream)
{
    if (!m || !n || !alpha_dev) return fail(HR_E_INVALID, "null argument");
    if (m->is_coarse) return fail(HR_E_INVALID, "the coarse level of a cascade has no grids");
    if (!m->finalized) return fail(HR_E_STATE, "hr_model_finalize has not been called (or tensors changed since)");
    if (m->cfg.grid_dtype != HR_GRID_FP32) return fail(HR_E_INVALID, "hr_dense_alpha reads float32 grids");
    if (hr_model_time_density(m)) return fail(HR_E_INVALID, "hr_dense_alpha: densityMode DensityLinear / DensityFourier is inference only (the mask update does not evaluate the density row)");
    if (n[0] < 1 || n[1] < 1 || n[2] < 1) return fail(HR_E_INVALID, "bad lattice size");
    if (m->cfg.video && num_frames < 1) return fail(HR_E_INVALID, "keyframe nets need num_frames");
    if (prev_volume_dev && (!prev_n || !prev_aabb || prev_n[0] < 1 || prev_n[1] < 1 || prev_n[2] < 1))
        return fail(HR_E_INVALID, "previous mask without its size / box");
    if (!m->ucfg_dev) {
        HR_HIP(m->ucfg_dev.alloc(sizeof(hr_config)));
        HR_HIP(hipMemcpy(m->ucfg_dev, &m->cfg, sizeof(hr_config), hipMemcpyHostToDevice));
    }
    HrMaskArgs a = HrMaskArgs();
    a.cfg_dev = m->ucfg_dev;
    for (int j = 0; j < 3; ++j) { a.planes[j] = m->planes[j]; a.n[j] = n[j]; a.pn[j] = prev_volume_dev ? prev_n[j] : 0; }
    for (int j = 0; j < 6; ++j) a.prev_aabb[j] = prev_volume_dev ? prev_aabb[j] : 0.0f;
    a.length = length;
    a.num_frames = num_frames;
    a.prev_volume = prev_volume_dev;
    a.alpha = alpha_dev;
    hr_launch_dense_alpha(a, (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

int hr_pack_display(const float* rgb_dev, int32_t h, int32_t w, int32_t transpose, int32_t flip, int32_t rgba8, void* out_dev, void* stream)
{
    if (h < 1 || w < 1) return fail(HR_E_INVALID, "bad image shape");
    if (!rgb_dev || !out_dev) return fail(HR_E_INVALID, "null argument");
    hr_launch_pack_display(rgb_dev, h, w, transpose ? 1 : 0, flip ? 1 : 0, rgba8 ? 1 : 0, out_dev, (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}
