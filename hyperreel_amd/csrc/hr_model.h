// Private to the C-ABI layer (api*.hip): the model behind an hr_model handle, its device memory, and the helpers the
// api files share.  Not part of the public interface (include/hyperreel_hip.h), whose declarations give the hr_* entry points
// that the api files define their C linkage.
#ifndef HR_MODEL_H
#define HR_MODEL_H

#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <string>

#include "hr_kernels.h"
#include "hr_train.h"

// functions and types shared between the api files: the library exports none of them
#define HR_HIDDEN __attribute__((visibility("hidden")))

// sample wavefronts per workgroup of the frame kernel when the caller does not say (measured: DESIGN.md section 3)
#ifndef HR_DEFAULT_SAMPLE_WAVES
#define HR_DEFAULT_SAMPLE_WAVES 0      // the plan's own choice (8)
#endif

// the error message of the calling thread (hr_last_error); returns `code`
HR_HIDDEN int fail(int code, const char* fmt, ...);

#define HR_HIP(call)                                                                                   \
    do {                                                                                               \
        hipError_t e__ = (call);                                                                       \
        if (e__ != hipSuccess) return fail(HR_E_HIP, "%s failed: %s", #call, hipGetErrorString(e__));  \
    } while (0)

// One device allocation, freed when its owner goes (move-only)
template <typename T>
class HR_HIDDEN DevMem {
public:
    DevMem() = default;
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    DevMem(DevMem&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevMem& operator=(DevMem&& o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
        return *this;
    }
    ~DevMem() { reset(); }
    hipError_t alloc(size_t bytes) { reset(); return hipMalloc((void**)&p_, bytes); }   // (frees what it held first)
    void reset()
    {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
    }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }

private:
    T* p_ = nullptr;
};

struct HR_HIDDEN DevBuf {
    DevMem<float> p;
    size_t bytes = 0;
};

// One packing of the MLP: MFMA A-operand tiles per Linear (layout: hr_mlp_pack.h)
struct HR_HIDDEN HrMlpTiles {
    DevMem<float4> wpack[HR_MAX_LAYERS];     // HR_MLP_FP32: fp32 tiles
    DevMem<uint16_t> wsplit[HR_MAX_LAYERS];  // the split arithmetics: hi / lo tiles
    DevMem<float> bias[HR_MAX_LAYERS];
    float winv[HR_MAX_LAYERS] = {};          // 2^-s of the packed split weights (HrMlpArgs::winv)
    int n_tiles[HR_MAX_LAYERS] = {};
    int64_t bytes = 0;
};

// The packed MLP, by tier: 0 = the active arithmetic.  Verified fast path: the MLP runs f16f8, rays with a comparison at risk
// (or a range bit) are listed on the device and rendered again by a second, list-driven pass at the end of hr_render with tier 1, the
// f16x3 tiles; tier 2: bf16x3 tiles (fp32 exponent range) for the third pass -- the tiles of the second pass in which an activation left
// the IEEE-half range (what the reference's fp32 BaseMLP, nlf/nets/mlp.py:159-172, cannot do)
struct HR_HIDDEN HrMlpPack {
    HrMlpTiles tiles[3];
    int k0p = 0;
    int n_out = 0;
    int64_t bytes = 0;
};

struct HR_HIDDEN HrCalibRays {
    DevMem<float> p;
    int64_t n = 0;
};

// Everything the choice of the MLP's arithmetic decides.  A value: api_mlp.hip builds a new one aside -- sharing the tiles or
// the rays of the old one where they stay -- and set_mlp_state puts it in the model's place once it is complete; nothing else writes it
// but hr_model_update_config, which marks the band stale, and hr_model_finalize, which lets go of the tiles and rays made from the
// weights before (the model is not finalized again until the new state is in).
struct HR_HIDDEN HrMlpState {
    int active_precision = HR_MLP_FP32;   // the arithmetic the MLP kernels run: cfg.mlp_precision, with HR_MLP_AUTO resolved (hr_mlp_choice)
    int verified = 0;                     // the verified fast path is on (tiles[1], tiles[2])
    int calibrated = 0;                   // 0: not calibrated (cascade rows / unsupported width), 1: synthetic rays (finalize), 2: the caller's rays
    float act_max[HR_MAX_LAYERS] = {};    // calibration: max |input feature|, max |pre-activation| of hidden Linear l - 1
    int xexp[HR_MAX_LAYERS] = {};         // f16 + fp8 split: exponent of the fp8 images of hidden Linear l's output (HrMlpArgs::xexp), from act_max
    std::shared_ptr<const HrMlpPack> pack;
    std::shared_ptr<const HrCalibRays> calib;   // the rays the arithmetic was decided on (synthetic, or a strided sample of the caller's): kept for the band
    HrBand band = {};                     // the margins of THIS model (calibrate_band; hr_math.h HrRisk)
    bool band_stale = false;              // the margins are the floor, or hr_model_update_config changed the activations' constants: measured before the next render
    hr_verify_info vinfo = {};
};

struct HR_HIDDEN hr_model {
    hr_config cfg;        // as handed over by the caller
    hr_config kcfg;       // what the kernels see: dead head columns removed (preds_per_z, field offsets)
    HrColMap col_map;     // user column -> live column (-1: never read by the path, not computed)
    int p_live = 0;
    bool finalized = false;
    std::map<std::string, DevBuf> raw;     // uploaded tensors, reference layout, device memory
    std::map<std::string, size_t> expect;  // name -> expected byte size
    HrMlpState mlp;                       // which arithmetic the MLP runs, its tiles, the verified fast path's margins: replaced whole (set_mlp_state)
    DevMem<unsigned> flags;               // sticky device status word (HrMlpArgs::flags)
    DevMem<int> redo_list;                // the second pass's rays
    DevMem<int> wide_list;                // the third pass's rays
    DevMem<unsigned> redo_count;          // [0] second-pass counter, [1] its copy, [2] third-pass counter, [3] its copy
    int redo_cap = 0;                    // entries the list holds (hr_model_reserve); a call uses hr_redo_list_cap of them
    int wide_cap = 0;
    // packed grids
    DevMem<float> grid_a[3];   // texel storage (floats, or halfs when cfg.grid_dtype == HR_GRID_FP16)
    DevMem<float> grid_b[3];
    HrGridPlane planes[3] = {};
    DevMem<float> basis;
    DevMem<float> basis_t;               // column-major copy for the decode-matrix fold (HrSampleArgs::basis_t)
    DevMem<int> slot_col;
    int basis_ld = 0;
    int n_basis_cols = 0;
    int ca_total = 0;
    // workspace
    DevMem<float> head;
    int64_t chunk = 0;
    int64_t packed_bytes = 0;            // grids and basis (the MLP's tiles: mlp.pack->bytes)
    // point_prediction cascade (hr_model_create_cascade): `this` is the fine level (point MLP, second intersect,
    // colour); `coarse` holds the ray MLP and the first intersect and owns no grids
    DevMem<hr_config> kcfg_dev;          // device copy of kcfg for the sample kernel (the MLP kernels take it by value)
    std::unique_ptr<hr_model> coarse;
    bool is_coarse = false;
    DevMem<float> rows;      // input rows of the point MLP for one chunk: (chunk * casc_in_z, casc_row_dim)
    // training path (hr_train_*): the caller's configuration on the device and packed gradient accumulators
    DevMem<hr_config> ucfg_dev;
    float* grad_a[3] = {};               // training: packed texel-gradient accumulators of the plane pairs -- slices of grad_pool
    float* grad_b[3] = {};
    DevMem<char> grad_pool;              // ONE allocation (cleared by one fill kernel per step)
    size_t grad_pool_bytes = 0;
    HrMlpTiles train_tiles;              // training forward (hr_mlp_train_forward): bf16 split tiles of the CURRENT parameter values, re-packed on the device every step
    DevMem<long long> grad_fx;           // deterministic training (HR_OPT_TRAIN_DETERMINISTIC): ONE 64-bit fixed-point buffer for every accumulator of a step
    size_t grad_fx_elems = 0;
    DevMem<HrFxUnit> fx_unit;            // ... and THIS model's fixed-point unit of the step (hr_train.h)
    int opt_train_det = 0;
    // hr_train_set_background: 0 the white_bg argument of the training calls decides; 1 the coin of (bg_seed, *bg_step_dev) does
    int bg_source = 0;
    uint64_t bg_seed = 0;
    const int64_t* bg_step_dev = nullptr;
    DevMem<float> tape;                  // per-sample values between the backward's phases: HR_TAPE_WORDS x tape_samples (hr_tape_bind)
    int64_t tape_samples = 0;
    // occupancy early-reject (hr_model_set_occupancy)
    DevMem<float> occ;
    DevMem<unsigned> occ_cells;           // one bit per lattice cell, built from a 0/1 volume (HrSampleArgs::occ_cells)
    int occ_n[3] = {};
    float occ_lo[3] = {}, occ_inv[3] = {};
    // execution plan of hr_render (hr_model_set_option)
    int frame_row = -1;                  // hr_render_frame: >= 0 while a call renders from frame_line[] (-1: general path)
    DevMem<float> frame_line[3];         // the frame's blended keyframe rows, one line per time plane (float32 texels)
    int opt_frame_kernel = 0;              // two kernels per chunk: level with the frame kernel since K1 took buffer loads (1.96 vs 1.99 ms per DoNeRF frame, interleaved
                                           // events, profiles/r05_headline_diag_*.json) and with the tighter tail (hardware block dispatch instead of a static tile deal)
    int opt_sample_waves = HR_DEFAULT_SAMPLE_WAVES;
    int n_cus = 0;
    // MLP shading modes (hr_model_set_shading_mlp): the colour network's descriptor, its tiles (hr_shade.h) and the chunk's workspace
    bool shade_set = false;
    HrShadeNet shade_net = {};
    DevMem<float4> shade_w[3];
    DevMem<float> shade_b[3];
    DevMem<float> shade_rows;            // (chunk * Z, HR_SHADE_ROW): the export form's rows
    DevMem<float> shade_rgb;             // (chunk * Z, 3): the shading kernel's colours
    // time-dependent decode modes (hr_model_set_time_decode)
    bool time_set = false;
    hr_time_decode time_desc = {};
    DevMem<float> dbasis_t;              // a density mode: column-major copy of basis_mat_density (HrTimeIO::dbasis_t)
    DevMem<int> dslot_col;               //   density-row slot -> column (HrTimeIO::dslot_col)
    int d_ld = 0, d_slots = 0;
};

// the model's sample stage (hr_plan.h); time kernel: sample_time_kernel.hip's -- a time-dependent colour mode, RGBIdentity, or a density mode
inline HrSampleKind hr_model_sample_kind(const hr_model* m) { return hr_sample_kind(m->cfg.shading, m->time_set && m->time_desc.density_mode != HR_DENSITY_PLAIN); }
inline bool hr_model_time_density(const hr_model* m) { return hr_model_sample_kind(m) == HR_SAMPLE_TIME_DENSITY; }
inline bool hr_model_time_kernel(const hr_model* m) { return hr_model_sample_kind(m) == HR_SAMPLE_TIME || hr_model_time_density(m); }

// a ray with a live sample beyond it (60 degrees off a plane's normal; a sphere nearly tangent) is not what the margins of the verified fast
// path are measured on -- its errors are the geometry's, the MLP's two-plane / Pluecker inputs included -- and is always listed
constexpr float HR_VERIFY_AMP_CUT = 2.0f;

// ---- api_mlp.hip
HR_HIDDEN int build_mlp_state(hr_model* m, const float* rays_dev, int64_t n, hipStream_t st, bool keep_tiles, HrMlpState& s);
HR_HIDDEN int set_mlp_state(hr_model* m, HrMlpState& s, hipStream_t st);
HR_HIDDEN int calibrate_band(hr_model* m, hipStream_t st);

// ---- api_render.hip (tier: 0 = the model's primary arithmetic; the verified fast path's later passes: 1 = its f16x3 tiles, 2 = its bf16x3 tiles)
HR_HIDDEN void launch_mlp(const hr_model* m, const hr_config& c, const HrMlpArgs& a, hipStream_t st, int tier = 0);
HR_HIDDEN void fill_mlp_args(const hr_model* m, HrMlpArgs& a, const float* rays, int64_t n, int tier = 0);
HR_HIDDEN void fill_sample_args(const hr_model* m, HrSampleArgs& a, const float* rays, int64_t n, float* rgb);
HR_HIDDEN void launch_front(hr_model* m, const float* rays, int64_t n, hipStream_t st, int tier = 0);
HR_HIDDEN HrRouteIn render_route_facts(const hr_model* m, int64_t n, bool fields, bool maps, HrFramePlan* frame = nullptr);
HR_HIDDEN void render_verified(hr_model* m, const HrBand& band, const float* rays_dev, int64_t n_rays, float* rgb_dev, int list_cap, hipStream_t st,
                               const hr_maps* maps = nullptr);

#endif  // HR_MODEL_H
