// The statements of the stand-alone sample kernel, included as the body of hr_sample_kernel (sample_kernel.hip) and of
// hr_sample_maps_kernel (sample_maps_kernel.hip) -- textually, not as a function, so that hr_sample_kernel compiles to the
// instructions it always had.  In scope: ZP, HALF, PC, NB, `cfg` (the configuration in device memory) and the argument block `a`;
// HR_SAMPLE_MAPS (false | true) and HR_SAMPLE_MAPS_PTR (nullptr | the kernel's hr_maps) select hr_sample_body's per-ray maps.
// HR_SAMPLE_SHADE (0 unless defined; 1 export | 2 import) and HR_SAMPLE_SHADE_PTR (the kernel's HrShadeIO) select hr_sample_body's
// forms for the MLP shading modes (sample_shade_kernel.hip).
// HR_SAMPLE_TIME (0 unless defined; hr_sample_body's TD, a constant expression: 1 = a time-dependent colour mode or RGBIdentity, 3 = with a
// density mode) and HR_SAMPLE_TIME_PTR (the kernel's HrTimeIO; defined by that kernel only: what the preprocessor tests) select the forms
// of sample_time_kernel.inc (DESIGN 3m).
#ifndef HR_SAMPLE_SHADE
#define HR_SAMPLE_SHADE 0
#define HR_SAMPLE_SHADE_PTR nullptr
#endif
#ifndef HR_SAMPLE_TIME
#define HR_SAMPLE_TIME 0
#endif
    constexpr int RPB = 256 / ZP;   // rays per block
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int CA = a.ca_total;                   // padded appearance slots (multiple of 4)
    const int HS = a.nq * 4 + 4;                   // LDS row stride of a head row (+4: conflict-free float4 fills)
    const int RPR = a.rows_per_ray;                // head rows per ray (1 unless the head comes from a point MLP)
    float* s_head = lds;                           // [RPB * RPR][HS]
    float* s_M = lds + RPB * RPR * HS;             // [RPB][3][CA]
    float* s_x = s_M + RPB * 3 * CA;               // [256] cross-wave scratch, ZP > 64 only

    const int tid = threadIdx.x;
    const int rib = tid / ZP;
    const int k = tid % ZP;
    // XCD-aware block order: the dispatcher places block b on XCD b % 8, so consecutive
    // blocks (neighbouring rays, overlapping texel footprints) would land on 8 different L2s.
    // Give each XCD a contiguous range of the ray list instead (bijective for any grid size).
    unsigned bid = blockIdx.x;
    {
        const unsigned nwg = gridDim.x, q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
    }
    const int64_t ray_base = (int64_t)bid * RPB;
    const int64_t lrow = ray_base + rib;           // position in this launch = row of the head
    // second pass of the verified fast path: the launch is sized for the list's capacity, *n_rays_dev rays are there.  (Workgroups that walk
    // the list from a fixed grid would save the ~14 us of dispatching empty workgroups -- and cost every launch of this kernel 44 registers and
    // 52 bytes of scratch: the loop makes the compiler hoist the body's invariants.)
    int64_t n_rays = a.n_rays;
    if (a.zero_word && blockIdx.x == 0 && threadIdx.x == 0) *a.zero_word = 0u;
    if (a.n_rays_dev) {
        const int64_t nd_raw = (int64_t)*a.n_rays_dev;
        const int64_t nd = nd_raw > a.list_off ? nd_raw - a.list_off : 0;
        n_rays = nd < n_rays ? nd : n_rays;
    }
    if (ray_base >= n_rays) return;                // (block-uniform, before any barrier)
    const bool ray_ok = lrow < n_rays;
    const int64_t ray = (a.ray_index && ray_ok) ? (int64_t)a.ray_index[lrow] : lrow;     // the caller's ray

    // ---- stage this block's head into LDS: per feature quad the block's RPB rays are RPB x 16
    //      contiguous bytes in the HQ layout (RPB divides 64, so a block never straddles a 64-ray group)
    if (RPR == 1) {
        const float4* src4 = reinterpret_cast<const float4*>(a.head) + ((size_t)(ray_base >> 6) * a.nq << 6) + (ray_base & 63);
        const int total = a.nq * RPB;
        for (int i = tid; i < total; i += 256) {
            const int q = i / RPB, r = i - q * RPB;
            *reinterpret_cast<float4*>(s_head + r * HS + 4 * q) = src4[((size_t)q << 6) + r];
        }
    } else {                                       // cascade: RPB * RPR rows of the point MLP's head, any alignment
        const float4* src4 = reinterpret_cast<const float4*>(a.head);
        const int NR = RPB * RPR;
        const int64_t row0 = ray_base * RPR, n_rows = n_rays * RPR;
        for (int i = tid; i < a.nq * NR; i += 256) {
            const int q = i / NR, r = i - q * NR;
            const int64_t row = row0 + r;
            if (row < n_rows) *reinterpret_cast<float4*>(s_head + r * HS + 4 * q) = src4[hr_head_index(row, 4 * q, a.nq) >> 2];
        }
    }

    // ---- per-ray quantities (computed redundantly by the ray's lanes) and the ray's decode matrix
    // RGB shading: the decode matrix is basis_mat itself, the same for every ray -- the block keeps ONE copy, filled by its
    // first ray's lanes (SH: one per ray, folded with that ray's view direction)
    // The ray record (origin, direction, time, contracted origin, keyframe time, the quadratic's ray terms: sample_core.inc, HrRayLane) is
    // computed by ONE lane per ray -- the first RPB lanes of the workgroup, a ray each -- and read back from LDS by the ray's lanes after the
    // barrier: in the lane-per-sample mapping every lane of the ray would otherwise repeat it.
    __shared__ __attribute__((aligned(16))) float s_ray[RPB * HR_RAY_RECORD];
    if (tid < RPB) {
        const int64_t lrow_r = ray_base + tid;
        const bool ok_r = lrow_r < n_rays;
        const int64_t ray_r = (a.ray_index && ok_r) ? (int64_t)a.ray_index[lrow_r] : lrow_r;
        HrRayLane R = hr_load_ray(cfg, a, ray_r, ok_r);
        hr_ray_constants(cfg, R);
        hr_store_ray_record(R, s_ray + tid * HR_RAY_RECORD);
    }
#ifdef HR_SAMPLE_TIME_PTR
    const bool per_ray_M = hr_shading_relu_half(cfg.shading);      // SH, and the RGBt modes: folded with the ray's time basis
#else
    const bool per_ray_M = (cfg.shading == HR_SHADING_SH);
#endif
    float* M = s_M + (per_ray_M ? rib * 3 * CA : 0);
#ifdef HR_SAMPLE_TIME_PTR
    const float t_lane = ray_ok ? a.rays[ray * cfg.ray_dim + cfg.ray_dim - 1] : 0.0f;      // (the record is not published yet)
    const float off_lane = cfg.advect ? t_lane - hr_base_time(cfg, t_lane) : 0.0f;         // hr_ray_constants' time_off
    if (hr_shading_is_time(cfg.shading)) hr_fill_decode_time<ZP>(a, HR_SAMPLE_TIME_PTR, t_lane, off_lane, k, M);
    else
#endif
    if (per_ray_M) {                          // SH: folded with the ray's view direction, which its lanes read themselves (the record is not published yet)
        HrRayLane V = hr_load_ray(cfg, a, 0, false);
        if (ray_ok) {
            const float* r = a.rays + ray * cfg.ray_dim;
            V.vd[0] = r[3]; V.vd[1] = r[4]; V.vd[2] = r[5];
        }
        hr_fill_decode<ZP>(cfg, a, V, k, M);
    } else if (rib == 0) {
        hr_fill_decode<ZP>(cfg, a, hr_load_ray(cfg, a, 0, false), k, M);
    }
#if HR_SAMPLE_SHADE == 1                          // export form (sample_shade_kernel.hip): all 27 rows of basis_mat, one copy per workgroup, behind the plan's LDS
    M = lds + HR_SAMPLE_SHADE_PTR->m_off;
    for (int pos = tid; pos < CA; pos += 256) {
        const int col = a.slot_col[pos];
        for (int c = 0; c < HR_SHADE_FEAT; ++c) M[c * CA + pos] = col >= 0 ? a.basis_t[(size_t)col * a.basis_ld + c] : 0.0f;
    }
#endif
    __shared__ __attribute__((aligned(16))) float s_ones[HR_GATHER_ONES];
    hr_gather_ones_init(s_ones);
#ifdef HR_SAMPLE_TIME_PTR                        // a density mode: the ray's density row, behind the plan's LDS, in the place of the ones
    const float* s_row = s_ones;
    if constexpr ((HR_SAMPLE_TIME & 2) != 0) {
        float* const s_D = lds + HR_SAMPLE_TIME_PTR.d_off + rib * HR_SAMPLE_TIME_PTR.d_slots;
        hr_fill_density_row<ZP>(HR_SAMPLE_TIME_PTR, t_lane, off_lane, k, s_D);
        s_row = s_D;
    }
#define HR_SAMPLE_ONES s_row
#else
#define HR_SAMPLE_ONES s_ones
#endif
    __syncthreads();
    const HrRayLane L = hr_read_ray_record(s_ray + rib * HR_RAY_RECORD);

    hr_sample_body<ZP, HALF, 1, NB, PC, HR_SAMPLE_MAPS, HR_SAMPLE_SHADE, HR_SAMPLE_TIME>(cfg, a, L, ray, ray_ok, k, s_head + rib * RPR * HS, HS, M, HR_SAMPLE_ONES, s_x,
                                                                                         HR_SAMPLE_MAPS_PTR, HR_SAMPLE_SHADE_PTR);
#undef HR_SAMPLE_ONES
