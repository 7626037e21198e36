/*
 * hyperreel_hip.h -- C ABI of libhyperreel_hip.so, the MI355X (gfx950) forward renderer
 * for HyperReel scenes.
 *
 * This is the drop-in boundary for ONE path of the reference: what
 * `render_fn(rays)` computes, i.e. RenderLightfield.forward
 * (nlf/rendering.py:72-77) -> LightfieldModel.forward (nlf/models/models.py:135-138)
 * -> RayPointEmbedding (nlf/embedding/embedding.py:100-117) -> TensorVMNoSample /
 * TensorVMKeyframeTime .forward (nlf/nets/tensorf_no_sample.py:128-280,
 * nlf/nets/tensorf_dynamic.py:645-839).  The reference has no FFI of its own (it is
 * pure PyTorch); the binding a maintainer adds is the ctypes stub shown in
 * INTEGRATION.md, selected with `experiment.model.render.type: lightfield_hip`
 * through the reference's own registry (nlf/rendering.py:95-97).
 *
 * Beside that path the header declares what surrounds it on the device: camera, fisheye and
 * light-field rays, the training step, its loss and optimizer, image scores, and the
 * training feed (hr_rayset_*): a device-resident training set under the datasets' subsample
 * rules -- the checkerboard in closed form, and Immersive's data-dependent
 * importance_subsample (datasets/immersive.py:295-310) as a per-image pixel list that
 * hr_rayset_set_image_importance selects and compacts on the device.
 *
 * Conventions: plain C types only; every pointer named *_dev is a device pointer
 * owned by the caller (e.g. torch tensor .data_ptr()); the library never frees
 * caller memory; `stream` is a hipStream_t passed as void*; all calls return 0 on
 * success and a negative HR_E_* code otherwise (hr_last_error() has the text; the
 * Python wrapper raises RuntimeError, the reference's only error channel).  Render
 * calls only enqueue work on `stream`: no allocation, no synchronisation, so they
 * can be captured in a hipGraph.
 */
#ifndef HYPERREEL_HIP_H
#define HYPERREEL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped when an existing struct, enum value or signature changes.  Purely additive entry points (new functions and the structs only
 * they use, such as the image scores below) do not bump it: every binding of version 27 keeps working against a library that has them. */
#define HR_ABI_VERSION 27

#define HR_MAX_Z 256         /* samples per ray (z_channels) supported by the sample kernel */
#define HR_MAX_P 64          /* per-sample head columns (preds_per_z) */
#define HR_MAX_GROUPS 4      /* ray-parameterisation groups feeding the MLP (`params:` in the YAML) */
#define HR_MAX_LAYERS 8      /* Linear layers of the sample-prediction MLP */
#define HR_MAX_FREQS 8       /* frequencies of a windowed positional encoding */
#define HR_MAX_MLP_IN 64     /* MLP input features after positional encoding */

/* error codes */
#define HR_OK 0
#define HR_E_INVALID (-1)    /* bad argument / unsupported configuration */
#define HR_E_STATE (-2)      /* call order: upload after finalize, render before finalize ... */
#define HR_E_HIP (-3)        /* a HIP runtime call failed */
#define HR_E_MISSING (-4)    /* finalize: a required tensor was never uploaded */
#define HR_E_RANGE (-5)      /* finalize / calibrate: a forced fp16 MLP arithmetic would overflow on this model's activations */

/* nlf/activations.py: Identity (:163-178), Sigmoid (:53-69), Tanh (:121-137).  y = act(x*inner+shift)*outer + add.
 * EaseValue (:462-496), w * act(x) + (1 - w) * start_value with the iteration-dependent weight w, is folded by the host
 * into outer (times w) and add ((1 - w) * start_value); once its window has passed w == 1 and add == 0. */
enum { HR_ACT_IDENTITY = 0, HR_ACT_SIGMOID = 1, HR_ACT_TANH = 2 };
typedef struct hr_act {
    int32_t type;
    float inner, shift, outer, add;
} hr_act;

/* nlf/param.py: identity (:20-24), PlueckerParam (:223-256), TwoPlaneParam (:63-118) */
enum { HR_PARAM_IDENTITY = 0, HR_PARAM_PLUECKER = 1, HR_PARAM_TWO_PLANE = 2 };
/* nlf/pe.py: IdentityPE, WindowedPE (:130-224, per-frequency weights in pe_weight), BasicPE (:32-71) */
enum { HR_PE_NONE = 0, HR_PE_WINDOWED = 1, HR_PE_BASIC = 2 };
typedef struct hr_param_group {
    int32_t start, end;          /* ray columns [start, end) (nlf/embedding/ray.py:319-321) */
    int32_t fn;                  /* HR_PARAM_* */
    float origin[3];
    float a, b;                  /* pluecker: direction/moment multiplier; two_plane: near/far plane z */
    int32_t pe_type;             /* HR_PE_* */
    int32_t pe_n_freqs;
    int32_t pe_exclude_identity;
    float pe_freq_mult, pe_base_mult;
    float pe_weight[HR_MAX_FREQS]; /* windowed: WindowedPE.weight(j) of frequency j (nlf/pe.py:186-208), 1 once its window has passed */
} hr_param_group;

/* One per-sample output of the MLP head (nlf/embedding/ray.py:333-337): `channels`
 * consecutive columns starting at `offset` inside the P = preds_per_z columns of a
 * sample; offset < 0: the field does not exist in this model. */
typedef struct hr_head_field {
    int32_t offset, channels;
    hr_act act;
} hr_head_field;

/* nlf/intersect: z.py:15-97 (z_plane), primitive.py:366-438 (sphere), :181-253 (cylinder), :441-545
 * (sphere_new), :256-363 (cylinder_new), :131-176 (euclidean_distance_unified), voxel.py:19-112
 * (voxel_grid), :115-215 (deformable_voxel_grid).  `plane` and `euclidean_distance` cannot run in the reference itself (their scalar
 * z_scale breaks Intersect.process_z_vals, base.py:129), so there is nothing to be compatible with. */
enum {
    HR_ISECT_Z_PLANE = 0, HR_ISECT_SPHERE = 1, HR_ISECT_CYLINDER = 2, HR_ISECT_SPHERE_NEW = 3,
    HR_ISECT_CYLINDER_NEW = 4, HR_ISECT_EUCLIDEAN_UNIFIED = 5, HR_ISECT_VOXEL_GRID = 6,
    HR_ISECT_DEFORMABLE_VOXEL_GRID = 7
};
/* nlf/contract.py: IdentityContract (:53-62), MIPNeRFContract (:113-192); BBoxContract (:65-87) and
 * ZDepthContract (:90-111) are both the affine map p -> (p - c_aff_min) / c_aff_size, d -> d / c_aff_fac */
enum { HR_CONTRACT_IDENTITY = 0, HR_CONTRACT_MIPNERF = 1, HR_CONTRACT_AFFINE = 2,
       /* DoNeRFContract (contract.py:195-240): p -> p / |p| * (|p| fac + 1e-8)^(1/power), d -> sign(d) (|d| + 1e-8)^power / fac */
       HR_CONTRACT_DONERF = 3 };
enum { HR_DENSITY_RELU = 0, HR_DENSITY_SOFTPLUS = 1, HR_DENSITY_RELU_ABS = 2 };
enum { HR_SHADING_RGB = 0, HR_SHADING_SH = 1,
       /* TensoRF's per-sample colour networks (nlf/nets/tensorf_base.py:38-69 MLPRender_Fea, :106-135 MLPRender): inference only; the
        * network is described by hr_model_set_shading_mlp (below), app_dim is 27 */
       HR_SHADING_MLP_FEA = 2, HR_SHADING_MLP = 3,
       /* the keyframe net's time-dependent colour (utils/tensorf_utils.py:346-400): the appearance features are coefficients of a
        * per-ray time basis, described by hr_model_set_time_decode (below); app_dim is 3 nb (RGBT_*) or 3 (RGB_IDENTITY: |x + 0.5|) */
       HR_SHADING_RGBT_LINEAR = 4, HR_SHADING_RGBT_FOURIER = 5, HR_SHADING_RGB_IDENTITY = 6 };
/* arithmetic of the MLP GEMMs: exact fp32 MFMA, or three 16-bit MFMA products of the hi/lo split operands with fp32
 * accumulation (needs mlp_hidden 256): bf16 halves (~2^-17 relative per product, fp32 range) or fp16 halves (~2^-22,
 * i.e. fp32-grade, but activations must stay below 65504); F16X2 additionally takes the weights as single halfs (two
 * products, 2^-12 relative weight rounding) */
enum { HR_MLP_FP32 = 0, HR_MLP_BF16X3 = 1, HR_MLP_F16X3 = 2, HR_MLP_F16X2 = 3,
       /* the library chooses: f16x3 when an activation-range calibration of the uploaded weights (hr_model_finalize: 4096 synthetic
        * rays; hr_model_calibrate: the caller's rays) keeps every input feature and hidden activation below 65504 / 8, bf16x3
        * otherwise (fp32 when mlp_hidden != 256).  The same test makes a FORCED f16x3 / f16x2 fail with HR_E_RANGE instead of
        * rendering infinities (the reference's BaseMLP is fp32, nlf/nets/mlp.py:127-172: any finite activation is legal there) */
       HR_MLP_AUTO = 4,
       /* fp16 halves like F16X3, but only the leading product x_hi*w_hi is an f16 MFMA: the two correction products (2^-11 of it) are ONE
        * fp8 (OCP e4m3) K=64 MFMA per 32 k with power-of-two block scales -- two thirds of F16X3's matrix-pipe time at ~2^-16 relative
        * per product (F16X3 2^-22, F16X2 2^-12).  Same range rule as F16X3, plus a per-layer exponent for the fp8 images taken from the
        * calibration (16x headroom); an activation beyond either range sets HR_OPT_MLP_OVERFLOW.  gfx950 (v_mfma_scale_f32_32x32x64_f8f6f4).
        * Its kernels evaluate the windowed positional encoding with v_sin / v_cos, which holds up to pe_base_mult * pe_freq_mult^pe_n_freqs
        * = 16 per windowed group: beyond that F16F8, F16F8V and HR_MLP_AUTO all resolve to F16X3 (HR_OPT_MLP_PRECISION_ACTIVE says so). */
       HR_MLP_F16F8 = 5,
       /* F16F8 with its discrete decisions VERIFIED (what HR_MLP_AUTO resolves to where it applies: a plain ray MLP of width 256, at most 64
        * samples per ray, activations inside the fp16 range).  The per-sample stage is continuous in the MLP's head except at a few
        * comparisons -- `dist <= near` / `>= far` (nlf/intersect/base.py:194), the quadratic's discriminant and root choice
        * (utils/intersect_utils.py:45-125), the bounding box (nlf/nets/tensorf_base.py:349-353), a positive weight threshold -- and F16F8's head
        * error (2e-5 of the head's range; distances move by < 1e-6 of the scene's extent) only shows when one of them falls the other way.  The
        * sample kernel therefore lists, on the device, every ray with a comparison inside a BAND of flipping (and the MLP kernel every tile that
        * raised a range bit), and hr_render / hr_render_frame end with a second, list-driven pass that renders exactly those rays (0.05 - 3 %
        * of a frame) again with F16X3's tiles.  The band is PER MODEL and PER SAMPLE: hr_model_finalize / hr_model_calibrate run the MLP in both
        * arithmetics on the calibration rays and measure how far the length fed to the intersection moves; the sample kernel pushes 4x that through
        * the derivatives of the inverse contraction and of the intersection of each sample (hr_verify_info below; csrc/hr_math.h, HrRisk).
        * Under HR_MLP_AUTO a model whose margins would list more than 5 % of the calibration rays, or whose calibration image differs from
        * F16X3's by more than 6e-5 anywhere, is rendered with F16X3 throughout instead; so are intersections the margins are not derived for
        * (the `_new` primitives, the deformable grid, learned sphere origins, DoNeRFContract).  Both passes are ordinary launches on the caller's stream: capturable.  hr_render_fields with diagnostics,
        * and models with an occupancy volume set (its cell test is a head-dependent decision the band does not cover), render everything with the
        * F16X3 tiles.  HR_OPT_MLP_PRECISION_ACTIVE reports HR_MLP_F16F8, HR_OPT_MLP_VERIFIED 1. */
       HR_MLP_F16F8V = 6 };
/* storage of the feature grids on the device: the reference's float32, or float16 texels (viewer
 * path, BASELINE config 5: half the gather bytes; values are rounded once at finalize, all arithmetic
 * stays fp32 -- results equal the fp32 path run on the rounded grids) */
enum { HR_GRID_FP32 = 0, HR_GRID_FP16 = 1 };
/* inputs of a point_prediction row: x['points'] of the coarse intersect, rays[..., 3:6], rays[..., 0:3], rays[..., -1:] */
enum { HR_PIN_POINTS = 0, HR_PIN_VIEWDIRS = 1, HR_PIN_ORIGINS = 2, HR_PIN_TIMES = 3 };

/* Everything the kernels need that the reference derives from the model YAML and the
 * five dataset scalars (near, far, depth_range, num_keyframes, num_frames).  Derived
 * floats are computed by the host in the reference's own precision and order
 * (hyperreel_amd/plan.py cites the lines). */
typedef struct hr_config {
    /* ---- rays + MLP (nlf/embedding/ray.py:213-347, nlf/nets/mlp.py:60-172) */
    int32_t ray_dim;                     /* 6 static [o,d]; 8 video [o,d,cam_id,t] */
    int32_t n_groups;
    hr_param_group groups[HR_MAX_GROUPS];
    int32_t mlp_in;                      /* input features (sum over groups after PE) */
    int32_t mlp_layers;                  /* number of Linear layers (D+2); 0 = ZeroMLP (nlf/nets/mlp.py:14-33) */
    int32_t mlp_hidden;                  /* W */
    int32_t mlp_skip_mask;               /* bit i set: layer i takes cat([input, x]) */
    float leaky_slope;                   /* 0.01 */
    int32_t z_channels;                  /* Z */
    int32_t preds_per_z;                 /* P */
    hr_head_field f_z_vals;
    hr_head_field f_isect_sigma;         /* x[intersect.in_density_field], intersect/base.py:152-158 */
    hr_head_field f_offset_sigma;        /* x[point_offset.in_density_field], embedding/point.py:378-381 */
    hr_head_field f_point_offset;
    hr_head_field f_color_scale;
    hr_head_field f_color_shift;
    hr_head_field f_spatial_flow;
    hr_head_field f_color_scale_global;  /* scale_shift_color_one, utils/tensorf_utils.py:275-281 (sample 0's values); with 9 channels: the head
                                          * `color_transform_global`, a row-major 3x3 for transform_color_one (:308-320) */
    hr_head_field f_color_shift_global;
    /* ---- intersect (nlf/intersect/base.py:142-259, z.py, primitive.py) */
    int32_t isect_type;                  /* HR_ISECT_* */
    float isect_origin[3];
    float near, far;                     /* mask: dist <= near | dist >= far */
    hr_act z_act;
    int32_t sort;
    float samples[HR_MAX_Z];             /* anchor samples (contracted space when contract_samples) */
    float z_scale;
    float origin_scale;                  /* sphere/cylinder: origins = z[:3]*origin_scale + origin_initial */
    float origin_initial[3];             /*   (*_new: origins = z[:3]*origin_scale, primitive.py:490-492) */
    float resize_scale;                  /* *_new: resize = z[3:6]*resize_scale + resize_initial (:494-496) */
    float resize_initial[3];
    float voxel_scale[3];                /* voxel_grid: per-axis z_scale; samples[] is (Z/3, 3) row-major */
    int32_t isect_outward;               /* voxel_grid: outward_facing (planes mirrored by sign(d)) */
    int32_t dvg_axes;                    /* deformable_voxel_grid: number of start normals (sample k uses normal k % axes) */
    float dvg_normals[9];                /*   start_normal rows */
    float dvg_normal_scale;              /*   normal = z[:3]*normal_scale_factor + start_normal, then normalised */
    int32_t isect_mask_off;              /* mask.stop_iters passed: no near/far masking (base.py:197-198) */
    /* ---- contraction (nlf/contract.py:113-192) */
    int32_t contract_type;               /* HR_CONTRACT_* */
    int32_t contract_samples;
    float c_r0, c_r_inv_end, c_r_scale;  /* points:   start radius,   r0/r1, 1/(1-r0/r1) */
    float c_d0, c_d_inv_end, c_d_scale;  /* distance: start distance, d0/d1, 1/(1-d0/d1) */
    float c_aff_min[3], c_aff_size[3];   /* affine: bbox_min, bbox_max - bbox_min (z_depth: 0, fac) */
    float c_aff_fac;                     /* affine: inverse_contract_distance(d) = d * fac */
    float c_pow_fac, c_pow_power, c_pow_inv_power;   /* donerf: fac, power, 1/power as the reference holds them (float32 of its python floats) */
    /* ---- advect (nlf/embedding/point.py:780-831, utils/flow_utils.py:10-35) */
    int32_t advect;
    int32_t use_spatial_flow;
    float flow_fac, flow_inv_fac;        /* K*(F-1)/F and its reciprocal */
    float flow_kmax;                     /* K-1 */
    hr_act flow_act;
    /* ---- point offset (nlf/embedding/point.py:371-396) */
    int32_t point_offset;
    hr_act offset_act;
    /* ---- colour net (nlf/nets/tensorf_no_sample.py, tensorf_dynamic.py, tensorf_base.py) */
    int32_t video;                       /* 0: tensor_vm_split_no_sample, 1: tensor_vm_split_time */
    float aabb[6];                       /* [min xyz, max xyz] */
    float inv_size[3];                   /* 2/(max-min) */
    int32_t grid[3];                     /* gridSize [Nx,Ny,Nz] */
    int32_t num_keyframes;               /* K (video) */
    int32_t n_den[3], n_app[3];          /* n_lamb_sigma, n_lamb_sh */
    int32_t app_dim;                     /* 3 (RGB, RGB_IDENTITY), 27 (SH degree 2, MLP_*) or 3 nb (RGBT_*) */
    int32_t shading;                     /* HR_SHADING_* */
    float distance_scale;
    float weight_thresh;                 /* rm_weight_mask_thre */
    int32_t density_act;                 /* HR_DENSITY_* */
    float density_shift;
    float time_scale, time_offset;       /* (F-1)/F and 0.5/K, tensorf_dynamic.py:58-59 */
    int32_t white_bg;
    int32_t mlp_precision;               /* HR_MLP_* */
    int32_t grid_dtype;                  /* HR_GRID_* */
    /* ---- per-camera colour correction (ColorTransformEmbedding, nlf/embedding/point.py:558-602):
     *      table row round(rays[..., -2]) = [3x3 transform | shift]; applied to the composited colour
     *      (transform_color_one, utils/tensorf_utils.py:308-320).  0 views: stage absent, or
     *      dataset.val_all false, in which case the reference's stage returns x unchanged. */
    int32_t color_table_views;
    hr_act color_table_t_act, color_table_s_act;
    /* ---- point_prediction cascade (PointPredictionEmbedding, nlf/embedding/point.py:39-218), set only in the
     *      FINE config of hr_model_create_cascade: the MLP of this config runs once per COARSE sample on the row
     *      [inputs...] (groups[] index the row's columns) and emits z_channels / casc_in_z samples per row. */
    int32_t casc_in_z;                   /* coarse samples per ray (in_z_channels); 0: not a cascade */
    int32_t casc_row_dim;                /* columns of an input row = sum of casc_input_dim */
    int32_t casc_n_inputs;
    int32_t casc_input_kind[4];          /* HR_PIN_* in `inputs` order (point.py:142-156) */
    int32_t casc_input_dim[4];           /* columns taken from each */
} hr_config;

/* Optional per-sample diagnostics of hr_render_fields (all device pointers, any may be
 * NULL).  They mirror what the reference exposes through render_kwargs `fields`
 * (tensorf_no_sample.py:254-278) and LightfieldModel.embed. */
typedef struct hr_fields {
    float* distances_dev;       /* (n, Z)    x['distances'] after sort + contraction */
    float* points_dev;          /* (n, Z, 3) x['points'] fed to the colour net */
    float* sigma_dev;           /* (n, Z)    density after feature2density */
    float* weights_dev;         /* (n, Z)    'render_weights' */
    float* head_dev;            /* (n, Z*P)  raw MLP output */
} hr_fields;

/* Per-ray maps of hr_render_maps / hr_render_frame_maps (device pointers, any may be NULL): the ray's weighted sums over its
 * samples, sum_k w_k x[key]_k, which the reference returns for render_kwargs fields=['distances', 'points']
 * (tensorf_no_sample.py:254-278), and its acc_map sum_k w_k (tensorf_no_sample.py:232).  w_k are the compositing weights
 * ('render_weights'); distances and points are hr_fields' per-sample values. */
typedef struct hr_maps {
    float* distances_dev;       /* (n)    sum_k w_k x['distances'][k]: the depth map */
    float* points_dev;          /* (n, 3) sum_k w_k x['points'][k]: the expected point */
    float* acc_dev;             /* (n)    sum_k w_k: the opacity (acc_map; before the white background) */
} hr_maps;

/* Pinhole camera of the viewer / offline-render path: what get_coords_from_camera
 * (datasets/base.py:485-518) consumes -- a 3x4 camera-to-world pose and intrinsics K. */
typedef struct hr_camera {
    float c2w[12];              /* row-major 3x4 [R | t], -z forward (utils/ray_utils.py:121-135) */
    float fx, fy, cx, cy;       /* K[0,0], K[1,1], K[0,2], K[1,2] */
    int32_t width, height;
    float cam_id, time;         /* columns 6 and 7 of 8-column rays (datasets/base.py:511-515) */
} hr_camera;

/* Normalised device coordinates of the forward-facing datasets (use_ndc: True in conf/experiment/dataset/{technicolor,neural_3d,
 * llff}.yaml): the arguments of get_ndc_rays_fx_fy (utils/ray_utils.py:137-164) as the dataset's to_ndc passes them
 * (datasets/technicolor.py:355-358: self.img_wh, self.K, self.near) -- the DATASET's size and focal lengths, which stay the same
 * when a frame is generated at another size with a scaled K (utils/gui_utils.py:151-158). */
typedef struct hr_ndc {
    float fx, fy, near;
    int32_t width, height;
} hr_ndc;

/* Radial distortion of a fisheye camera (the Immersive dataset: datasets/immersive.py:43-48, 514-523): the first two coefficients of
 * the equidistant model, theta_d = theta (1 + k1 theta^2 + k2 theta^4), which the reference hands to cv2.fisheye.undistortPoints as
 * D = (k1, k2, 0, 0) with K = I.  An all-zero hr_fisheye means "no distortion given" and is the pinhole camera, exactly like a NULL one.
 * (This is a convention of this interface, not of the model: OpenCV treats k1 = k2 = 0 as the plain equidistant lens theta_d = theta,
 * whose pixels still move by tan(theta_d) / theta_d.  A caller who means that lens passes a coefficient too small to matter, such as
 * k1 = 1e-30f.) */
typedef struct hr_fisheye {
    float k1, k2;
} hr_fisheye;

/* Two-plane light field (the Stanford configs: datasets/lightfield.py, datasets/stanford.py): what get_lightfield_rays and
 * get_epi_rays (utils/ray_utils.py:14-78) take besides the position on the camera plane.  A ray starts at (s, t) * st_scale on the
 * plane z = near and passes through (u, v) * uv_scale on the plane z = far.  The reference's use_inf, center_u and center_v are
 * accepted there and never read; they are not part of this interface. */
typedef struct hr_lightfield {
    int32_t width, height;      /* U x V of a view; U x S of an epipolar slice */
    float aspect;               /* v (and an EPI's s) is divided by it: W / H of the images (datasets/stanford.py:66) */
    float st_scale, uv_scale;
    float near, far;            /* z of the camera plane and of the image plane (-1 and 0 by default) */
} hr_lightfield;

typedef struct hr_rayset hr_rayset;

typedef struct hr_model hr_model;

int hr_abi_version(void);
int hr_sizeof_config(void);      /* sizeof(hr_config) as compiled, for binding self-checks */
const char* hr_last_error(void);

/* Builds a model for `cfg` on the current HIP device.  Replaces the constructors
 * LightfieldModel.__init__ (nlf/models/models.py:104-129) + RenderLightfield.__init__
 * (nlf/rendering.py:59-70). */
int hr_model_create(const hr_config* cfg, hr_model** out);

/* Two-level model for the reference's point_prediction cascades (the shipped ..._cascaded.yaml and
 * ..._feedback.yaml model groups): `coarse` describes ray_prediction + the first ray_intersect (its colour-net fields are
 * ignored), `fine` the point_prediction MLP (casc_* set), the second ray_intersect and everything after it.
 * Tensors of the coarse MLP are uploaded as mlp.<i>.*, those of the point MLP as mlp1.<i>.*. */
int hr_model_create_cascade(const hr_config* coarse, const hr_config* fine, hr_model** out);

/* Hands over one tensor of the reference state_dict, float32, in the reference's own
 * layout (nlf/__init__.py:433-479 are the reference's loader).  `name` is the key with
 * the module prefix removed:
 *   mlp.<i>.weight (out,in)  mlp.<i>.bias (out)                      i < mlp_layers
 *   density_plane.<j> (1,C,H,W)  density_line.<j> (1,C,N,1)
 *   app_plane.<j>  app_line.<j>                                      static net, j < 3
 *   density_plane_space.<j> density_plane_time.<j> (1,C,K,N)
 *   app_plane_space.<j> app_plane_time.<j>                           video net
 *   basis_mat.weight (app_dim, sum n_app)
 *   color_embedding (color_table_views, 12)                           when color_table_views > 0
 * `ptr` may be host or device memory; the data is copied before the call returns. */
int hr_model_upload(hr_model* m, const char* name, const void* ptr, size_t bytes);

/* Re-lays the uploaded tensors out for the kernels (channel-last interleaved planes,
 * MFMA-tiled MLP weights).  May be called again after further uploads.  For mlp_precision AUTO / F16X3 / F16X2 it first measures
 * the MLP's activation range on 4096 synthetic rays (origins uniform in the model's aabb, unit directions) and resolves / checks
 * the arithmetic (see HR_MLP_AUTO); HR_E_RANGE when a forced fp16 mode does not fit. */
int hr_model_finalize(hr_model* m);

/* The same decision on the caller's own rays (device memory, n_rays x ray_dim): measures the activation range of the MLP
 * (BaseMLP.forward, nlf/nets/mlp.py:159-172, evaluated in plain fp32) on them, re-resolves HR_MLP_AUTO and re-packs the MLP
 * weights if the choice changes.  Synchronises `stream`.  `act_max` (may be NULL) receives mlp_layers floats: the largest
 * |input feature|, then the largest |pre-activation| of each hidden Linear.  HR_E_RANGE as for hr_model_finalize.
 * All or nothing: a return other than HR_OK leaves everything the choice rests on as it was before the call -- the active arithmetic,
 * HR_OPT_MLP_VERIFIED, HR_OPT_MLP_CALIBRATED, the activation maxima and fp8 exponents, the packed weights, the calibration rays the
 * model keeps, the margins of the verified fast path and hr_verify_info -- and the model renders the same pixels.  The same holds for
 * the measurement of the margins wherever it runs, the one hr_render makes after hr_model_update_config included: an error leaves the
 * previous margins and hr_verify_info in place, and the measurement is due again at the next render (only one that completed clears that). */
int hr_model_calibrate(hr_model* m, const float* rays_dev, int64_t n_rays, float* act_max, void* stream);

/* Replaces the model's configuration by one that differs only in schedule-dependent constants -- the `outer` / `add`
 * of the activations (EaseValue), `pe_weight` (WindowedPE) and `isect_mask_off` (mask.stop_iters) -- as INRSystem.set_train_iter does for the reference
 * modules every training step (nlf/__init__.py:608-614).  No weights are re-packed.  Any other difference is refused
 * with HR_E_INVALID.  Waits for `stream` before the device copies are replaced. */
int hr_model_update_config(hr_model* m, const hr_config* cfg, void* stream);

/* Sizes the per-launch workspace (rays processed per internal chunk).  Optional. */
int hr_model_reserve(hr_model* m, int64_t rays_per_chunk);

/* Execution plan of hr_render.  The arithmetic is the same under every setting (bit-identical images); the options choose
 * how it is laid out on the device.
 *   HR_OPT_FRAME_KERNEL   0 (default): two kernels per chunk of rays -- the MLP writes the head to an HBM workspace, the sample kernel
 *                         reads it back.  Level in time with the frame kernel (round 5, interleaved per-frame events: 1.96 vs 1.99 ms
 *                         on the DoNeRF frame) and with the tighter tail: the hardware dispatches its blocks, nothing is dealt statically.
 *                         1: models whose head tile fits the CU's LDS are rendered by ONE persistent kernel in which
 *                         MLP wavefronts hand the (B, Z*P) head that the reference materialises between RayPredictionEmbedding and
 *                         Intersect (nlf/embedding/ray.py:332-337 -> nlf/intersect/base.py:142-259) to sample wavefronts of the
 *                         same workgroup through LDS -- no workspace traffic (static nets, 64-ray tiles).  Models that do not
 *                         fit (wider heads, cascades, the exact-fp32 MLP, other plane decompositions), every hr_render_fields
 *                         call with a non-NULL `fields` and every hr_render_maps / hr_render_frame_maps call with a map requested
 *                         take the two-kernel path (same images).
 *                         2: additionally the keyframe families (480-column heads, 960 at 64 samples per ray;
 *                         nlf/nets/tensorf_dynamic.py:645-839) on 32-ray tiles, two head buffers where they fit: same images, no
 *                         head workspace traffic, measured as fast as or slower than two kernels (hence not part of 1).
 *   HR_OPT_SAMPLE_WAVES   sample wavefronts per workgroup of the frame kernel: 4 or 8 (0: the plan's default, 8).
 *   HR_OPT_TRAIN_DETERMINISTIC  1: hr_train_backward accumulates every gradient that many samples add to -- texel gradients, basis_mat's,
 *                         the colour table's -- as 64-bit fixed point with integer atomics instead of fp32 atomics (the unit is a power of two
 *                         chosen per step: the step's largest |dL/d rgb| = 2^32 units; a non-finite contribution, or one beyond 2^62 units,
 *                         turns the step's totals into NaN, as the fp32 path would hold inf / NaN there): the
 *                         result does not depend on the order of the adds, so two runs of the same step agree bit for bit (the
 *                         reference's loop, nlf/__init__.py:634-709, is deterministic for a given thread count).  The values agree
 *                         with the default mode's to fp32 rounding of the sums; slower (no LDS staging of the contended lines).
 *                         0 (default): fp32 atomics.  The MLP's GEMM gradients are reduced in a fixed order in both modes.
 * Read-only: HR_OPT_FRAME_KERNEL_ACTIVE whether hr_render currently takes the frame kernel; HR_OPT_MLP_PRECISION_ACTIVE the HR_MLP_*
 * arithmetic the MLP kernels run (HR_MLP_AUTO resolved); HR_OPT_MLP_CALIBRATED 0 / 1 (finalize's synthetic rays) / 2 (hr_model_calibrate);
 * HR_OPT_MLP_OVERFLOW the sticky bit the fp16-split kernels set when an input feature or hidden activation of a RENDERED ray reached
 * the IEEE-half range (reading it synchronises the device; cleared by hr_model_finalize / hr_model_calibrate); HR_OPT_MLP_F8_SATURATED the
 * sticky bit HR_MLP_F16F8's kernels set when a hidden activation of a rendered ray was beyond the range of its fp8 image (16x the calibration's
 * largest activation of that layer): the image saturates, the ray's correction products lose accuracy (towards HR_MLP_F16X2's), nothing
 * overflows -- hr_model_calibrate on such rays moves the exponents and clears the bit.
 * HR_OPT_MLP_VERIFIED 1 when hr_render runs the verified fast path (HR_MLP_F16F8V); HR_OPT_REDO_COUNT the number of rays the last hr_render listed
 * for its second pass (reading it synchronises the device); HR_OPT_REDO_OVERFLOW the sticky bit raised when a call listed more rays than the
 * list holds -- max(32 768, n_rays / 16) per call, i.e. more than 6.25 % of a large call's rays at risk, which the calibration's 5 % rule
 * makes a property of rays unlike the calibration's: the excess rays keep their first-pass pixels.  A caller that renders without
 * hyperreel_amd's host guard polls this bit (hr_model_calibrate on such rays re-decides; HR_MLP_F16X3 never lists).
 * HR_OPT_WIDE_COUNT: rays the last hr_render passed on to the THIRD pass (bf16x3 tiles: halves with the fp32 exponent range) because an activation of
 * theirs left the IEEE-half range in the second -- the device-side form of the overflow fallback, inside a captured graph too.  In the verified
 * mode HR_OPT_MLP_OVERFLOW / HR_OPT_MLP_F8_SATURATED are raised only for rays that could not be listed (a full list).
 * HR_OPT_CHUNK_RAYS: rays per launch of the head workspace (hr_model_reserve's, or hr_model_finalize's default): what hr_stage_* accept. */
enum { HR_OPT_FRAME_KERNEL = 0, HR_OPT_SAMPLE_WAVES = 1, HR_OPT_FRAME_KERNEL_ACTIVE = 2, HR_OPT_MLP_PRECISION_ACTIVE = 3,
       HR_OPT_MLP_OVERFLOW = 4, HR_OPT_MLP_CALIBRATED = 5, HR_OPT_TRAIN_DETERMINISTIC = 6, HR_OPT_MLP_F8_SATURATED = 7,
       HR_OPT_MLP_VERIFIED = 8, HR_OPT_REDO_COUNT = 9, HR_OPT_REDO_OVERFLOW = 10, HR_OPT_WIDE_COUNT = 11, HR_OPT_CHUNK_RAYS = 12 };
int hr_model_set_option(hr_model* m, int32_t option, int32_t value);
int hr_model_get_option(hr_model* m, int32_t option, int32_t* value);

/* What the verified fast path (HR_MLP_F16F8V) rests on for THIS model: the margins inside which a comparison counts as "at risk" and the
 * measurement they were derived from (hr_model_finalize on 4096 synthetic rays, hr_model_calibrate on the caller's, again after
 * hr_model_update_config).  The reference needs none of this: its MLP is fp32 (nlf/nets/mlp.py:159-172) and its decisions are exact
 * comparisons (nlf/intersect/base.py:194, utils/intersect_utils.py:45-150).
 * The margins are per SAMPLE (csrc/hr_math.h, HrRisk): with zc = z * scale + anchor (process_z_vals, nlf/intersect/base.py:128-140, before
 * the inverse contraction), dlen = |d length / d zc| of the inverse contraction and amp = |d distance / d length| of the intersection
 * (1 / |d_axis| for a plane, 2 |r| / sqrt(discriminant) for sphere and cylinder), a length is at risk within band * dlen, a distance within
 * band * dlen * amp, a point coordinate within band_q * (largest amp of the ray) + band_off. */
typedef struct hr_verify_info {
    int32_t verified;            /* 1: hr_render runs the verified fast path */
    int32_t fallback;            /* HR_MLP_AUTO gave the fast path up for this model (it renders F16X3): 1 = `listed_frac` exceeded 0.05,
                                  * 2 = `max_d_rgb` exceeded 6e-5 (the cheap arithmetic's own error is too large on these weights) */
    float band;                  /* margin of zc: max(band_floor, 4 * max(max_d_zc, max_d_dist_n)) */
    float band_q;                /* margin of a point coordinate per unit of amplification: max(band_floor, 4 * max_d_geo_n) */
    float band_off;              /* margin of the point-offset / flow heads: 4 * max_d_off */
    float band_floor;            /* 1e-6: four float32 ulps of the largest |zc| (2) */
    float max_d_zc;              /* largest |zc(f16f8) - zc(f16x3)| over all calibration samples */
    float max_d_dist_n;          /* largest |distance(f16f8) - distance(f16x3)| / (dlen * amp) over the samples alive under both: the margins' model, checked */
    float max_d_geo_n;           /* largest point difference caused by the distance difference, / amp */
    float max_d_off;             /* largest point difference caused by the offset / flow heads */
    float max_d_dist;            /* largest |distance difference| as it is (scene units; reported) */
    float max_d_head;            /* largest difference of a raw head column (reported) */
    float listed_frac;           /* fraction of the well-conditioned calibration rays the first pass lists with these margins (hr_model_calibrate: of
                                  * all the caller's rays, the ill-conditioned ones -- always listed -- included) */
    float max_d_rgb;             /* largest |rgb(verified path) - rgb(F16X3)| over the well-conditioned calibration rays: f16f8's continuous error on THIS model */
    int64_t n_rays;              /* calibration rays */
    int64_t n_rays_used;         /* ... of which well-conditioned (no live sample with amp > 2): every figure above is taken over these; at render time a ray
                                  * with a live sample beyond that is listed by that alone.  Fewer than 64: listed_frac and max_d_rgb are not measured */
    int64_t n_samples;           /* samples alive under both arithmetics */
    int64_t n_flipped;           /* samples left out because their normalised distance moved by more than 1e-3 (a decision fell the other way) */
    int64_t n_shaky;             /* samples left out because a radius, root or discriminant was exactly 0 */
} hr_verify_info;
int hr_model_verify_info(hr_model* m, hr_verify_info* out);

/* Opt-in occupancy early-reject of the render path.  The reference builds an AlphaGridMask while training
 * (TensorBase.updateAlphaMask) and carries the test in its forward -- `alphas = self.alphaMask.sample_alpha(xyz_sampled[ray_valid]);
 * ray_valid &= alphas > 0` (nlf/nets/tensorf_no_sample.py:171-177, utils/tensorf_utils.py:459-484) -- but ships it disabled
 * (`... and False`).  With a volume set, hr_render / hr_render_fields apply exactly that test to every valid sample before the
 * feature gather: rejected samples are not fetched and composite with sigma = 0, i.e. the image is the reference's with its
 * `and False` removed (pinned by a fixture rendered that way).  volume_dev: (n[2], n[1], n[0]) floats as AlphaGridMask.alpha_volume
 * holds them (x fastest), copied; aabb: its box [min xyz, max xyz].  NULL volume: back to the shipped behaviour.  Waits for `stream`. */
int hr_model_set_occupancy(hr_model* m, const float* volume_dev, const int32_t n[3], const float aabb[6], void* stream);

/* rgb_dev[n,3] = render_fn(rays_dev[n,ray_dim])['rgb']  (eval mode: clamped to [0,1]). */
int hr_render(hr_model* m, const float* rays_dev, int64_t n_rays, float* rgb_dev, void* stream);
/* hr_render for ONE FRAME of a keyframe net: the caller states that the last column of every ray is `time` (what
 * get_coords_from_camera builds for a frame, datasets/base.py:485-518; the viewer and validation_video render frame by frame,
 * nlf/__init__.py:754-893).  Every sample of the frame then blends the SAME two keyframe rows of each time plane with the same
 * weights (TensorVMKeyframeTime's grid_sample over (position, time), nlf/nets/tensorf_dynamic.py:287-371): the library folds them
 * into one line per time plane on `stream` first and the gather reads lines, as it does for a static net (2 taps instead of 4 per
 * plane pair and sample).  The blend is re-associated -- (b00 wt0 + b10 wt1) wx0 + ... instead of b00 (wx0 wt0) + ... -- so images
 * agree with hr_render's to ~1e-6, not bit for bit.  Static nets, cascades and float16 texels take hr_render's path unchanged.
 * Rays whose time differs from `time` are rendered with `time`'s rows (undefined with respect to the reference).  The lines are
 * per-model scratch: frames of one model at different times must not be in flight on different streams at once. */
int hr_render_frame(hr_model* m, const float* rays_dev, int64_t n_rays, float time, float* rgb_dev, void* stream);
int hr_render_fields(hr_model* m, const float* rays_dev, int64_t n_rays, float* rgb_dev,
                     const hr_fields* fields, void* stream);
/* hr_render / hr_render_frame that also write the per-ray maps of `maps` (hr_maps) in the same launches: rgb_dev is bit for bit
 * hr_render's / hr_render_frame's, on the same plan -- the verified fast path included (its later passes rewrite the listed rays'
 * maps with the pixels), no safe tier as hr_render_fields' diagnostics force -- except that HR_OPT_FRAME_KERNEL does not apply: a
 * maps call takes the two-kernel path.  O(n) memory, no allocation, no synchronisation (capturable).  maps == NULL, or all three
 * pointers NULL: exactly hr_render / hr_render_frame. */
int hr_render_maps(hr_model* m, const float* rays_dev, int64_t n_rays, float* rgb_dev, const hr_maps* maps, void* stream);
int hr_render_frame_maps(hr_model* m, const float* rays_dev, int64_t n_rays, float time, float* rgb_dev, const hr_maps* maps,
                         void* stream);

/* Image-parallel frames: every rank renders a contiguous pixel range of the frame into `tile_dev` and the tiles are
 * assembled on every rank by ONE all-gather over RCCL / xGMI: full_dev[r * floats_per_rank ..] = rank r's tile_dev[0 .. floats_per_rank).
 * `nccl_comm` is the caller's ncclComm_t (one process per GPU; the communicator is the integrator's: torch.distributed's, MPI's, ...),
 * passed as void* so that this header stays free of RCCL types; the collective is enqueued on `stream` (hipGraph-capturable like
 * hr_render; no host synchronisation).  The library resolves ncclAllGather from the RCCL already loaded into the process (or
 * librccl.so) on first use -- it has no link-time dependency on it; HR_E_HIP when no RCCL can be found.  The reference has no
 * counterpart: it shards whole validation images over DDP ranks and never gathers pixels (nlf/__init__.py:896). */
int hr_allgather_tiles(void* nccl_comm, const float* tile_dev, float* full_dev, int64_t floats_per_rank, void* stream);
/* pixel range [first, first + count) of rank `rank` of `world` for an image of n_pixels (even contiguous split, the first
 * n_pixels % world ranks take one pixel more); floats_per_rank for hr_allgather_tiles is 3 * the count of rank 0 (the largest). */
int hr_shard_range(int64_t n_pixels, int32_t rank, int32_t world, int64_t* first, int64_t* count);

/* rays_dev[n_pixels, ray_dim] for pixels [first_pixel, first_pixel + n_pixels) of the image in
 * row-major order: get_ray_directions_K(centered_pixels=True) + get_rays(normalize=True)
 * (utils/ray_utils.py:98-135) [+ cam_id, time when ray_dim == 8].  Generating the rays on the
 * device from 80 bytes of camera replaces the 15-20 MB host->device copy of a frame's ray list;
 * with image-parallel rendering every rank generates only its own pixel range. */
int hr_generate_rays(const hr_camera* cam, int32_t ray_dim, int64_t first_pixel, int64_t n_pixels, float* rays_dev, void* stream);
/* hr_generate_rays followed by get_ndc_rays_fx_fy (utils/ray_utils.py:137-164) on every ray, as get_coords / get_coords_from_camera
 * do for use_ndc datasets (datasets/base.py:507-509, datasets/technicolor.py:384-385, datasets/neural_3d.py:383,400): origin shifted
 * to the near plane and projected, direction = projected difference, d_z = 1 - o_z; IEEE divisions in the reference's order.
 * ndc == NULL: exactly hr_generate_rays (the same bits). */
int hr_generate_rays_ndc(const hr_camera* cam, const hr_ndc* ndc, int32_t ray_dim, int64_t first_pixel, int64_t n_pixels, float* rays_dev,
                         void* stream);
/* The rays of a fisheye camera's own pixels, as ImmersiveDataset.get_coords builds them for training and validation
 * (datasets/immersive.py:514-564).  Pixel (x, y):
 *   (dx, dy) = ((x - cx + 0.5) / fx, -(y - cy + 0.5) / fy)                          the pinhole direction's first two components
 *   theta_d = |(dx, dy)|;  theta solves theta (1 + k1 theta^2 + k2 theta^4) = theta_d;  (dx', dy') = (dx, dy) tan(theta) / theta_d
 *                                                                                    (unchanged when theta_d <= 1e-8)
 *   direction = normalize(dx', dy', -1), rotated by the pose and normalised again; origin = the pose's translation;
 *   then get_ndc_rays_fx_fy when ndc is given.
 * The contract is this inverse of the equidistant model, solved by a fixed number of Newton steps from theta = theta_d
 * (csrc/hr_camera.h), not OpenCV's iteration count or its non-convergence sentinel.  fisheye == NULL or
 * k1 == k2 == 0: exactly hr_generate_rays_ndc (the same kernel, the same bits) -- the reference's render split (distortion = None, line 507).  Ranges, ray_dim, ndc and the launch contract as for
 * hr_generate_rays_ndc: one kernel on `stream`, no allocation, no synchronisation, no memset, every output element written;
 * capturable in a hipGraph.  HR_E_INVALID before any launch, besides that call's reasons: a non-finite coefficient, or a pair for
 * which 1 + 3 k1 t^2 + 5 k2 t^4 <= 0 somewhere on [0, pi / 2] -- theta_d(theta) is then not increasing and has no inverse. */
int hr_generate_rays_fisheye(const hr_camera* cam, const hr_fisheye* fisheye, const hr_ndc* ndc, int32_t ray_dim, int64_t first_pixel,
                             int64_t n_pixels, float* rays_dev, void* stream);

/* rays_dev[n_pixels, 6] for pixels [first_pixel, first_pixel + n_pixels) of the row-major U x V view at camera-plane position
 * (s, t): get_lightfield_rays (utils/ray_utils.py:14-45) in its order of float32 operations.  Pixel (x, y):
 *   u = linspace(-1, 1, U)[x] * uv_scale,  v = linspace(1, -1, V)[y] / aspect * uv_scale  (torch.linspace's float32 elements on the
 *   CPU: stepped from the start in the first half, from the end in the second; U or V == 1: the start),
 *   origin = (s * st_scale, t * st_scale, near),  direction = (u - o_x, v - o_y, far - near) / max(|.|, 1e-12).
 * A range holds the same bits as the same rows of the whole view, so every image-parallel rank generates its own hr_shard_range.
 * One kernel on `stream`: no allocation, no synchronisation, no memset, every output element written; capturable in a hipGraph.
 * HR_E_INVALID before any launch: width or height < 1, aspect == 0, a non-finite scalar, a negative range, first_pixel + n_pixels
 * beyond U * V, rays_dev NULL with n_pixels > 0. */
int hr_generate_rays_lightfield(const hr_lightfield* lf, float s, float t, int64_t first_pixel, int64_t n_pixels, float* rays_dev,
                                void* stream);
/* The epipolar slice (u, s) at a fixed (v, t): get_epi_rays (utils/ray_utils.py:47-78).  lf->width = U, lf->height = S; row
 * p = j * U + x:  u as above,  s = linspace(-1, 1, S)[j] / aspect * st_scale,  origin = (s, t * st_scale, near),
 * direction = (u - s, v * uv_scale - t * st_scale, far - near), normalised.  Rows [first, first + n); otherwise as above. */
int hr_generate_rays_epi(const hr_lightfield* lf, float v, float t, int64_t first, int64_t n, float* rays_dev, void* stream);

/* ---- training feed --------------------------------------------------------------------------------
 * A device-resident training set.  The reference keeps `all_inputs`, a host float tensor of ray_dim + 4 floats per training ray
 * (prepare_train_data / update_all_data, datasets/base.py:130-143, datasets/technicolor.py:238-282), shuffles it on the host every
 * epoch (base.py:202-227) and slices batches out of it (format_batch, base.py:278-284).  Here the 8-bit images live in device memory
 * (3 bytes per pixel) with one camera and one subsample rule per image, and a batch's rays are computed when they are drawn.
 * The set element e (0 <= e < hr_rayset_size) is the e-th row of the reference's all_inputs: images in index order, within an image
 * the pixels with (x + y + offset) % every == 0 in row-major order (subsample, technicolor.py:211-236; every == 1: all of them).
 *
 * hr_rayset_create: n_images images of width x height on the current device, ray_dim 6 or 8, ndc as for hr_generate_rays_ndc (copied;
 * NULL: world-space rays).  The library owns the pixel store (n_images * height * width * 3 bytes) and the per-image table. */
int hr_rayset_create(int32_t n_images, int32_t width, int32_t height, int32_t ray_dim, const hr_ndc* ndc, hr_rayset** out);
void hr_rayset_destroy(hr_rayset* set);
/* What the set's pixels are: a set is one format as a whole, HR_PIXELS_RGB8 when this is never called.
 *   HR_PIXELS_RGBA8_WHITE  every hr_rayset_set_image* / hr_rayset_set_view then takes height * width * 4 bytes of RGBA, what
 *     Image.convert("RGBA") holds, and a row's colour is the pixel over white as the reference's RGBA datasets compute it
 *     (datasets/blender.py:61-70, donerf.py:240-249): C = byte / 255, rgb = C * A + (1 - A) in float32, one rounding per operation --
 *     bit for bit torch's.  Coordinates, weights, elements and the order are those of the RGB set of the same cameras.
 * Valid on a set of either kind (hr_rayset_create, hr_rayset_create_lightfield) before its first image is stored: afterwards
 * HR_E_STATE and nothing changes.  Replaces the pixel store (n_images * height * width * 4 bytes).  HR_E_INVALID: a NULL set, an unknown
 * format.  hr_rayset_set_image_importance on an RGBA set is HR_E_INVALID: the reference's importance datasets are RGB.
 * Additive: no existing struct or signature moved (HR_ABI_VERSION stays). */
enum { HR_PIXELS_RGB8 = 0, HR_PIXELS_RGBA8_WHITE = 1 };
int hr_rayset_set_pixel_format(hr_rayset* set, int32_t format);
/* Image i: pose, intrinsics, cam_id and time in `cam` (its width / height must be the set's), the subsample rule (every >= 1,
 * offset >= 0) and height * width * 3 bytes of RGB, row-major, host or device memory -- what Image.convert("RGB") holds before ToTensor
 * (get_rgb, technicolor.py:398-417).  Synchronous (set-up, not the training loop).  Images not yet set hold no rays. */
int hr_rayset_set_image(hr_rayset* set, int32_t i, const hr_camera* cam, int32_t every, int32_t offset, const uint8_t* rgb_host_or_dev);
/* The same for an image of a fisheye camera: the image's rays are hr_generate_rays_fisheye's, bit for bit; everything else --
 * elements, order, colours, weights, hr_rayset_batch / _order / _sample -- is unchanged, and images with and without distortion mix
 * in one set.  fisheye == NULL or both coefficients zero: exactly hr_rayset_set_image.  HR_E_INVALID for the pairs
 * hr_generate_rays_fisheye refuses and on a light-field set. */
int hr_rayset_set_image_fisheye(hr_rayset* set, int32_t i, const hr_camera* cam, const hr_fisheye* fisheye, int32_t every, int32_t offset,
                                const uint8_t* rgb_host_or_dev);
/* A set whose images are views of one two-plane light field (datasets/lightfield.py, datasets/stanford.py): n_views images of
 * lf->width x lf->height, ray_dim 6, *lf copied.  Element e is views in index order, row-major within a view (after the view's
 * checkerboard rule) -- the order prepare_train_data concatenates in when the caller lists the views as its loops do, t outer and s
 * inner (datasets/lightfield.py:106-141).  That method holds a leftover debugging exit() at line 120 and cannot run as shipped, so
 * this contract is defined by the ray function (get_lightfield_rays, as hr_generate_rays_lightfield computes it, bit for bit) and
 * that loop order, not by a run of the method.  hr_rayset_size / _batch / _order / _destroy work on it unchanged: the same
 * permutation, colours, weights and NaN rows.  hr_rayset_set_image on such a set, and hr_rayset_set_view on a set made by
 * hr_rayset_create, are HR_E_INVALID. */
int hr_rayset_create_lightfield(int32_t n_views, const hr_lightfield* lf, hr_rayset** out);
/* View i: its position (s, t) on the camera plane (before st_scale: LightfieldDataset.get_coord, lightfield.py:185-191, or
 * StanfordLightfieldDataset.normalize_coord, stanford.py:95-106), the subsample rule and height * width * 3 bytes of RGB as for
 * hr_rayset_set_image.  Synchronous. */
int hr_rayset_set_view(hr_rayset* set, int32_t i, float s, float t, int32_t every, int32_t offset, const uint8_t* rgb_host_or_dev);
/* rays in the set after subsampling: the reference's len(all_coords); negative on a null set */
int64_t hr_rayset_size(const hr_rayset* set);
/* Rows [first, first + n) of the order of epoch `epoch`: row r is set element perm(r), a bijection of [0, size) keyed by
 * (seed, epoch) -- every ray exactly once per epoch, replacing np.random.permutation (base.py:202-227), not reproducing its stream.
 * With indices_dev (n int64, device memory) output row j is element indices_dev[j] instead: the caller's own sampler; an element
 * outside [0, size) yields a row of NaN with weight 0.  coords_dev (n, ray_dim): the ray of the element's pixel as
 * hr_generate_rays_ndc computes it [+ cam_id, time]; rgb_dev (n, 3) = (float)u8 / 255.0f (ToTensor: exact); weight_dev (n, 1) = 1
 * (get_weights, base.py:191-194).  Outputs may be NULL.  first + n > size is HR_E_INVALID, not a wrap.  One kernel on `stream`: no
 * allocation, no synchronisation, no memset, every output element written; capturable in a hipGraph. */
int hr_rayset_batch(const hr_rayset* set, int64_t first, int64_t n, uint64_t seed, uint64_t epoch, const int64_t* indices_dev,
                    float* coords_dev, float* rgb_dev, float* weight_dev, void* stream);
/* elements_dev[j] (n int64) = the set element of row first + j of that order: which ray each row of hr_rayset_batch is. */
int hr_rayset_order(const hr_rayset* set, int64_t first, int64_t n, uint64_t seed, uint64_t epoch, int64_t* elements_dev, void* stream);
/* n rows drawn WITH replacement -- the sampler every shipped training config asks for (sample_with_replacement: True ->
 * RandomSampler(replacement=True, num_samples=num_iters * batch_size), nlf/__init__.py:222-230).  Output row j is set element
 * e(seed, s, j), uniform and independent over [0, size): a counter-based generator (Philox4x32-10, key = seed, counter = (j, s)) whose
 * 64-bit draw is mapped by multiply-high with size (csrc/hr_sample_rng.h; bias below size / 2^64).  It replaces that sampler and does
 * not reproduce torch's stream.  s = step when step_dev is NULL, else the 64-bit word at step_dev (DEVICE memory, read when the
 * kernel runs: a captured launch draws a new batch on every replay once the word has changed -- hr_adam_step_dev's counter serves).
 * Row j depends on (seed, s, j) alone, not on n.  The rows hold exactly what hr_rayset_batch(indices_dev = those elements) writes;
 * elements_dev_or_null (n int64) receives the elements.  Any output may be NULL, not all four (HR_E_INVALID when n > 0); n < 0, a
 * null set and a set without rays are HR_E_INVALID; n == 0 succeeds and launches nothing.  One kernel on `stream`: no allocation, no
 * synchronisation, no memset, every output element written; capturable in a hipGraph.  Additive: no existing struct or signature moved
 * (HR_ABI_VERSION stays). */
int hr_rayset_sample(const hr_rayset* set, int64_t n, uint64_t seed, uint64_t step, const uint64_t* step_dev, float* coords_dev, float* rgb_dev,
                     float* weight_dev, int64_t* elements_dev_or_null, void* stream);

/* ---- the importance subsample rule -- Immersive's, and Neural 3D's variant without the direction test
 * (importance_subsample, datasets/immersive.py:295-310, datasets/neural_3d.py:191-204).  Image i keeps the pixels whose mean absolute
 * difference to image `prev` (the frame before it in its video) is STRICTLY greater than the num_take-th largest such difference of the
 * image, and, when dir_z_below is not NaN, whose ray -- the one hr_rayset_batch returns for the pixel -- has column 5 < dir_z_below
 * (-0.05 in the reference).  The difference is torch.abs(rgb - last_rgb).mean(-1) on ToTensor's floats, bit for bit
 * (csrc/hr_importance.h); which pixels are kept is therefore the reference's choice exactly, ties at the threshold included, and set
 * element e stays row e of all_inputs: the kept pixels of an image follow in row-major order.  The rule depends on the pixels, so the
 * set keeps a list per such image: a radix select of the threshold, the mask and a stable compaction run on the device
 * (csrc/importance_kernel.hip), into at most (num_take - 1) * 4 bytes.  Images under either rule mix in one set.
 * Stores the image like hr_rayset_set_image_fisheye (fisheye_or_null as there), runs the rule against image `prev` and commits.
 * Synchronous.  HR_E_INVALID, naming the cause, before anything changes: a light-field set; prev == i, prev outside the set or not
 * set yet; num_take < 1 (in the reference diff_sorted[-0] is the MINIMUM and the rule silently keeps nearly every pixel: refused, not
 * reproduced) or num_take > width * height; a camera or distortion hr_rayset_set_image_fisheye refuses; width * height >= 2^31.
 * Any hr_rayset_set_image* of an image that a listed image names as its `prev` is refused as well -- that list would be stale: set
 * images in load order.  Additive: no existing struct or signature moved (HR_ABI_VERSION stays). */
int hr_rayset_set_image_importance(hr_rayset* set, int32_t i, const hr_camera* cam, const hr_fisheye* fisheye_or_null, int32_t prev,
                                   int64_t num_take, float dir_z_below, const uint8_t* rgb_host_or_dev);
/* out_dev[k] (n int32, device memory) = the row-major pixel index y * width + x of kept pixel first + k of image i, under either rule
 * (and for a light-field view).  [first, first + n) outside the image's kept pixels is HR_E_INVALID.  One kernel on `stream`. */
int hr_rayset_image_pixels(const hr_rayset* set, int32_t i, int64_t first, int64_t n, int32_t* out_dev, void* stream);
/* (a struct tag, not a typedef: the call below bears the same name) */
struct hr_rayset_image_info {
    int64_t count;            /* kept pixels: the image's rays in the set (0: not set yet, or nothing kept) */
    int64_t num_take;         /* importance rule: its num_take, else 0 */
    int32_t every, offset;    /* checkerboard rule (every == 0: not set yet); 1, 0 for a listed image */
    int32_t is_list;          /* 1: the importance rule's list */
    int32_t prev;             /* importance rule: the image the difference was taken to, else -1 */
    float threshold;          /* importance rule: the num_take-th largest difference, else 0 */
    float dir_z_below;        /* importance rule: the direction limit, NaN for none; else NaN */
};
int hr_rayset_image_info(const hr_rayset* set, int32_t i, struct hr_rayset_image_info* out);

/* The resize in front of the training feed: what every PIL-based dataset of the reference does to a decoded image in get_rgb
 * (datasets/llff.py:145-163: img.resize(_img_wh, Image.LANCZOS), then img.resize(img_wh, Image.BOX) when they differ), on the device and
 * byte for byte as PIL computes it for an 8-bit RGB image (csrc/hr_resize.h states the arithmetic; PIL's output is the authority).
 * Images are (h, w, 3) bytes, rows dense.  filter: PIL's Image.Resampling number -- 1 LANCZOS, 2 BILINEAR, 3 BICUBIC, 4 BOX.
 * A plan serves one (w, h) -> (w2, h2) and filter, for up to max_images images a call: it owns both axes' coefficient tables, computed
 * on the host and checked there (every row: 255 * sum|k| + 2^21 < 2^31, so that the int32 sums cannot overflow), and the 8-bit image
 * between the horizontal and the vertical pass, in the memory of the device that is current at creation.  Create, resize and destroy
 * on that device.  HR_E_INVALID, naming the argument: a size below 1 or beyond 2^20, an unknown filter, max_images < 1, a NULL `out`,
 * a coefficient row that fails the accumulator check. */
typedef struct hr_resize_plan hr_resize_plan;
int hr_resize_plan_create(int32_t w, int32_t h, int32_t w2, int32_t h2, int32_t filter, int32_t max_images, hr_resize_plan** out);
/* The same for 8-bit RGBA images, (h, w, 4) bytes: Image.resize of an RGBA image, which is not the RGB resize on four channels -- PIL
 * converts to premultiplied RGBa (c * a / 255, rounded), resamples the four channels by the rule above and converts back (copied at
 * alpha 0 and 255, else min(255, 255 * c / a), truncated); csrc/hr_resize.h states both.  Same size on both axes: a copy, nothing is
 * converted (a pixel of alpha 0 keeps its colour bytes).  hr_image_resize on such a plan reads and writes 4 bytes per pixel and wants
 * src_dev and dst_dev 4-byte aligned (HR_E_INVALID otherwise).  Refusals as hr_resize_plan_create, under its name.
 * Additive: no existing struct or signature moved (HR_ABI_VERSION stays). */
int hr_resize_plan_create_rgba(int32_t w, int32_t h, int32_t w2, int32_t h2, int32_t filter, int32_t max_images, hr_resize_plan** out);
/* src_dev: n_images images (h, w, 3) -> dst_dev: n_images images (h2, w2, 3), both dense in device memory and not overlapping; exactly
 * n_images * h2 * w2 * 3 bytes are written.  Only kernels (same size on both axes: one device-to-device copy) on `stream`: no
 * host-to-device copy, no allocation, no synchronisation; capturable in a hipGraph.  Calls on one plan share its intermediate image:
 * order them on one stream.  HR_E_INVALID: a NULL plan, src_dev or dst_dev; n_images outside 1..max_images.
 * Additive: no existing struct or signature moved (HR_ABI_VERSION stays). */
int hr_image_resize(const hr_resize_plan* p, const uint8_t* src_dev, int32_t n_images, uint8_t* dst_dev, void* stream);
void hr_resize_plan_destroy(hr_resize_plan* p);

/* ---- PNG files on the device (csrc/hr_png.h states the format arithmetic once) ----
 * A frame that is already in device memory becomes a complete, standard PNG file in device memory: signature, IHDR, one IDAT chunk
 * per strip of rows, IEND; 8 bits a sample, non-interlaced, `channels` 1 (grey), 3 (RGB) or 4 (RGBA).  The host copies `*file_bytes_dev`
 * bytes and writes them.  pixels_dev is row-major (h, w, channels), contiguous: HR_PNG_U8 bytes, or HR_PNG_F32_TO8B floats that go
 * through the display pack's to8b as they are read -- (uint8)(255 * clip(x, 0, 1)), NaN giving 0 (numpy's own cast of NaN is
 * undefined).  filter_mode: HR_PNG_FILTER_ADAPTIVE (per row, the filter with the smallest sum of min(v, 256 - v); lowest index on a
 * tie) or a fixed PNG filter 0..4.  Integer arithmetic and integer LDS atomics only: the same frame gives the same file on every run,
 * and the host build of hr_png.h (hr_png_encode_host) gives the same bytes.
 * hr_png_bound: a capacity that always suffices (every strip falls back to stored blocks when its Huffman block is not smaller).
 * hr_png_encoder_create: the encoder owns its workspace in device memory (current device).  hr_png_encode: three kernels and a
 * one-workgroup scan on `stream`; no allocation, no synchronisation, no host read-back, no memset; capturable in a hipGraph.  Nothing
 * beyond *file_bytes_dev bytes of file_dev is written.  One encode at a time per encoder (the workspace is its own).
 * HR_E_INVALID before anything is launched or written: w or h below 1 (or a row beyond 2^27 bytes, an image beyond 2^30 filtered bytes), channels not in
 * {1, 3, 4}, capacity below hr_png_bound, a NULL pointer, an unknown pixel_type or filter_mode.
 * Additive: no existing struct or signature moved (HR_ABI_VERSION stays). */
#define HR_PNG_U8 0
#define HR_PNG_F32_TO8B 1
#define HR_PNG_FILTER_ADAPTIVE 5
typedef struct hr_png_encoder hr_png_encoder;
int hr_png_bound(int32_t w, int32_t h, int32_t channels, int64_t* bytes);
int hr_png_encoder_create(int32_t w, int32_t h, int32_t channels, hr_png_encoder** out);
int hr_png_encode(hr_png_encoder* e, const void* pixels_dev, int32_t pixel_type, int32_t filter_mode, void* file_dev, int64_t capacity,
                  int64_t* file_bytes_dev, void* stream);
void hr_png_encoder_destroy(hr_png_encoder* e);

/* ---- JPEG files written on the device (csrc/hr_jpeg_encode.h states the encoder once for host and device) ----
 * A frame that is already in device memory becomes a complete baseline JPEG file in device memory, byte for byte the file PIL 12.2 /
 * libjpeg-turbo writes for Image.save(f, 'JPEG', quality=q, subsampling=s[, restart_marker_rows=r]) with the standard Huffman tables:
 * JFIF header, jpeg_set_quality's tables, libjpeg's fixed-point colour conversion, edge replication and h2v1 / h2v2 downsampling,
 * jpeg_fdct_islow, quantisation, interleaved MCUs, Huffman coding with byte stuffing, optional restart markers every restart_rows MCU rows.
 * pixels_dev is row-major (h, w, channels), contiguous, with hr_png_encode's pixel types: HR_PNG_U8 bytes, or HR_PNG_F32_TO8B floats that
 * go through to8b as they are read (NaN gives 0).  channels 1: grey; 3: RGB; 4: RGBA with the alpha byte ignored (hr_pack_display's).
 * subsampling: HR_JPEG_444 / HR_JPEG_422 / HR_JPEG_420 (PIL's numbers); a grey image takes HR_JPEG_444 only.
 * hr_jpeg_bound: a capacity that always holds the file.  hr_jpeg_encoder_create: the encoder owns its workspace in device memory (current
 * device), with the tables and the header built on the host.  hr_jpeg_encode: eight kernels on `stream` (a hipStream_t passed as void*),
 * no allocation, no synchronisation, capturable; file_dev[0 .. *length_dev) is the file, nothing is written past it; one encode at a time
 * per encoder.  Integer arithmetic and integer atomic OR only: the same frame gives the same file on every run, and the host build of
 * hr_jpeg_encode.h (hr_jpeg_encode_host) gives the same bytes.
 * HR_E_INVALID: a size below 1 or above 65535, channels outside {1, 3, 4}, quality outside 1..100, an unknown subsampling, grey with a
 * subsampling other than 4:4:4, negative restart_rows or more than 65535 MCUs per interval, an image of more blocks than 32-bit bit
 * offsets address (about 2.5 million), capacity below hr_jpeg_bound, a NULL pointer, an unknown pixel_type.
 * Additive: no existing struct or signature moved (HR_ABI_VERSION stays). */
#define HR_JPEG_444 0
#define HR_JPEG_422 1
#define HR_JPEG_420 2
typedef struct hr_jpeg_encoder hr_jpeg_encoder;
int hr_jpeg_bound(int32_t w, int32_t h, int32_t channels, int32_t subsampling, int32_t restart_rows, int64_t* bytes);
int hr_jpeg_encoder_create(int32_t w, int32_t h, int32_t channels, int32_t quality, int32_t subsampling, int32_t restart_rows, hr_jpeg_encoder** out);
int hr_jpeg_encode(hr_jpeg_encoder* e, const void* pixels_dev, int32_t pixel_type, void* file_dev, int64_t capacity, int64_t* length_dev,
                   void* stream);
void hr_jpeg_encoder_destroy(hr_jpeg_encoder* e);

/* ---- PNG files decoded on the device (csrc/hr_png_decode.h states the decoder once for host and device) ----
 * A batch of PNG files in device memory becomes (n, h, w, out_channels) bytes in device memory: the container with every chunk's CRC-32,
 * the zlib stream across IDAT boundaries (stored, fixed and dynamic blocks; code-length sets taken and refused as zlib's inflate does),
 * the Adler-32, PNG filters 0..4, and PIL's convert('L' | 'RGB' | 'RGBA').  Accepted: 8 bits a sample, colour type 0 / 2 / 4 / 6, no
 * interlace; everything else is HR_PNG_E_UNSUPPORTED (hr_png_probe says so beforehand, a caller keeps its own decoder for those).
 * status_dev holds one int32 per image: HR_PNG_OK or one of the codes below; an image whose status is not HR_PNG_OK is all zeros.
 * hr_png_probe: host only, reads the signature and IHDR of file_host[0..n) (no checksum); HR_E_INVALID when they are not there.
 * hr_png_decoder_create: every image of a call is w x h; the decoder owns its workspace in device memory (current device): the filtered
 * bytes of max_images images and one row of pixels each, nothing that grows with a file's chunk count.  max_file_bytes_total bounds
 * offsets_dev's values: files_dev holds at least that many bytes, and an image whose offsets leave [0, max_file_bytes_total] or decrease
 * is HR_PNG_E_OFFSETS and not read.
 * hr_png_decode: files_dev the files one after another, offsets_dev[n_images + 1] their bounds, out_dev (n_images, h, w, out_channels)
 * with out_channels 1, 3 or 4.  Three kernels on `stream`, one workgroup per image; no allocation, no synchronisation, no read-back,
 * no memset; capturable in a hipGraph.  One decode at a time per decoder.  n_images == 0 launches nothing.
 * HR_E_INVALID before anything is launched: a NULL pointer, n_images outside [0, max_images], out_channels not 1, 3 or 4.
 * Additive: no existing struct or signature moved (HR_ABI_VERSION stays). */
#define HR_PNG_OK 0
#define HR_PNG_E_SIGNATURE 1     /* not a PNG signature */
#define HR_PNG_E_CHUNK 2         /* IHDR not first or not 13 bytes, zero size, IDAT chunks apart, none at all, a length beyond 2^31 - 1 */
#define HR_PNG_E_CRC 3
#define HR_PNG_E_UNSUPPORTED 4   /* palette, 1 / 2 / 4 / 16 bits, Adam7, unknown compression or filter method */
#define HR_PNG_E_SIZE 5          /* not the decoder's w x h */
#define HR_PNG_E_ZLIB_HEADER 6
#define HR_PNG_E_BLOCK 7         /* block type 3, LEN / NLEN, more than 286 / 30 symbols */
#define HR_PNG_E_CODE 8          /* a refused set of code lengths, an unassigned code, length symbol 286 / 287, distance symbol 30 / 31 */
#define HR_PNG_E_DISTANCE 9      /* a distance reaching before the first byte produced */
#define HR_PNG_E_TRUNCATED 10    /* the file, or the zlib stream inside its IDAT chunks, ends early; no IEND */
#define HR_PNG_E_TOO_LONG 11     /* more than h * (1 + w * channels) bytes */
#define HR_PNG_E_TOO_SHORT 12
#define HR_PNG_E_ADLER 13
#define HR_PNG_E_FILTER 14       /* a row's filter byte above 4 */
#define HR_PNG_E_OFFSETS 15
typedef struct hr_png_info {
    int32_t width, height, bit_depth, color_type;
    int32_t channels;            /* samples a pixel in the file: 1, 2 (grey + alpha), 3 or 4; 1 for a palette */
    int32_t interlace;
    int32_t supported;           /* 1: hr_png_decode takes it */
    int32_t reserved;
} hr_png_info;
typedef struct hr_png_decoder hr_png_decoder;
int hr_png_probe(const void* file_host, int64_t n, hr_png_info* info);
int hr_png_decoder_create(int32_t w, int32_t h, int32_t max_images, int64_t max_file_bytes_total, hr_png_decoder** out);
int hr_png_decode(hr_png_decoder* dec, const void* files_dev, const int64_t* offsets_dev, int32_t n_images, int32_t out_channels, void* out_dev,
                  int32_t* status_dev, void* stream);
void hr_png_decoder_destroy(hr_png_decoder* dec);

/* ---- JPEG files decoded on the device (csrc/hr_jpeg_decode.h states the decoder once for host and device) ----
 * A batch of baseline JPEG files in device memory becomes (n, h, w, out_channels) bytes in device memory, byte for byte what PIL's
 * Image.open(f).convert('L' | 'RGB' | 'RGBA') gives: Huffman decoding parallel inside a stream (subsequences of subseq_bits bits that
 * synchronise themselves over rounds), libjpeg's jpeg_idct_islow, fancy upsampling and fixed-point YCbCr -> RGB.  Accepted: SOF0 / SOF1 at
 * 8 bits, one component or three as YCbCr with luma 1x1 / 2x1 / 2x2 and chroma 1x1, one scan, restart markers; everything else is
 * HR_JPEG_E_UNSUPPORTED (hr_jpeg_probe says so beforehand).  The decoder is strict: a damaged file gets a status below and an all-zero
 * image, libjpeg's recovery is not reproduced.
 * hr_jpeg_probe: host only, reads the markers of file_host[0..n) up to the scan; HR_E_INVALID when there is no SOI or no frame header.
 * hr_jpeg_decoder_create: every image of a call is w x h; subseq_bits 0 for the default, else a multiple of 32 from 128 up.  The decoder
 * owns its workspace in device memory (current device).
 * hr_jpeg_decode: as hr_png_decode; rounds_dev (may be NULL) gets per image the most rounds a restart interval took.  Only enqueues
 * kernels on `stream`: no allocation, no synchronisation, no read-back; capturable in a graph.  One decode at a time per decoder. */
#define HR_JPEG_OK 0
#define HR_JPEG_E_SOI 1          /* no SOI at the start of the file */
#define HR_JPEG_E_MARKER 2       /* bad or overlong segment, truncated header, no SOF / SOS, an unknown marker */
#define HR_JPEG_E_UNSUPPORTED 3
#define HR_JPEG_E_SIZE 4         /* not the decoder's w x h */
#define HR_JPEG_E_TABLE 5        /* missing or invalid DQT / DHT */
#define HR_JPEG_E_CODE 6         /* a bit pattern that is no code, a size above 11 (DC) or 10 (AC), a run symbol baseline does not have */
#define HR_JPEG_E_COEF 7         /* a run past coefficient 63; values beyond what libjpeg's 16-bit arithmetic holds */
#define HR_JPEG_E_RESTART 8      /* missing, surplus or out-of-order RSTn */
#define HR_JPEG_E_TRUNCATED 9    /* the entropy data or the file ends early; no EOI */
#define HR_JPEG_E_TOO_LONG 10    /* a byte or more of entropy data left over after a restart interval's last MCU */
#define HR_JPEG_E_OFFSETS 11
typedef struct hr_jpeg_info {
    int32_t width, height;
    int32_t components;          /* 1 or 3 (4 in a file that is not taken) */
    int32_t h_samp, v_samp;      /* luma sampling; 0 when the file is not taken */
    int32_t restart_interval;
    int32_t supported;           /* 1: hr_jpeg_decode takes it */
    int32_t status;              /* the HR_JPEG_* code the head of the file gives */
} hr_jpeg_info;
typedef struct hr_jpeg_decoder hr_jpeg_decoder;
int hr_jpeg_probe(const void* file_host, int64_t n, hr_jpeg_info* info);
int hr_jpeg_decoder_create(int32_t w, int32_t h, int32_t max_images, int64_t max_file_bytes_total, int32_t subseq_bits, hr_jpeg_decoder** out);
int hr_jpeg_decode(hr_jpeg_decoder* dec, const void* files_dev, const int64_t* offsets_dev, int32_t n_images, int32_t out_channels, void* out_dev,
                   int32_t* status_dev, int32_t* rounds_dev, void* stream);
void hr_jpeg_decoder_destroy(hr_jpeg_decoder* dec);

/* Grid management: F.interpolate(plane, size=(h2, w2), mode='bilinear', align_corners=True) of one
 * (1, C, H, W) float32 plane or line, as TensorVMSplit.up_sampling_VM / TensorVMKeyframeTime.up_sampling_VM apply it
 * when the reference grows its grids (nlf/nets/tensorf_base.py:1152-1176, tensorf_dynamic.py:395-427).  Both buffers
 * are device memory in the reference layout; no model is involved. */
int hr_upsample_plane(const float* src_dev, int32_t channels, int32_t h, int32_t w, float* dst_dev, int32_t h2, int32_t w2, void* stream);

/* ---- training path --------------------------------------------------------------------------
 * What torch.autograd does for the reference in INRSystem.training_step (nlf/__init__.py:634-709), for the stage
 * after the MLP: forward without the eval-mode clamp (nlf/nets/tensorf_no_sample.py:246) and the reverse-mode
 * derivative of Intersect.forward (nlf/intersect/base.py:142-259), the point embeddings (nlf/embedding/point.py:371-396,
 * 780-831), TensorVMNoSample / TensorVMKeyframeTime.forward (tensorf_no_sample.py:128-280, tensorf_dynamic.py:645-839)
 * and raw2alpha (utils/tensorf_utils.py:242-253).  The MLP itself (plain GEMMs) stays with the caller's autograd:
 * hr_train_features gives its input, `head_dev` is its raw output (n_rays, z_channels * preds_per_z) row-major in the
 * caller's column order, and hr_train_backward returns dL/d head for it.
 * All tensors are device memory, float32, in the reference's parameter layouts (same shapes as the hr_model_upload
 * names): a[j] = density_plane.j | density_plane_space.j, b[j] = density_line.j | density_plane_time.j, likewise app_*.
 * Supported: every model hr_model_create / hr_model_create_cascade accepts, with float32 grids (float16 grids return
 * HR_E_INVALID naming the feature).
 * Activation / encoding / mask schedules are those of the model's current configuration (hr_model_update_config). */
typedef struct hr_train_tensors {
    float* density_a[3];
    float* density_b[3];
    float* app_a[3];
    float* app_b[3];
    float* basis;                        /* basis_mat.weight (app_dim, sum n_app) */
    float* color_table;                  /* color_embedding (color_table_views, 12); NULL / ignored when the model has none */
} hr_train_tensors;

/* point_prediction cascades (nlf/embedding/point.py:137-203): the same three calls serve their fine level -- head_dev is then
 * the point MLP's raw output, one row of z_channels / casc_in_z samples per coarse point, which is (n_rays, z_channels *
 * preds_per_z) in memory -- and hr_train_features gives the input of the cascade's RAY MLP.  Between the two MLPs:
 *   hr_train_rows_forward   ray MLP head (n, Zc * Pc) -> rows_dev (n * Zc, casc_row_dim): per coarse sample the point after
 *                           the first intersect next to the ray constants the YAML lists, i.e. the point MLP's input row
 *                           (before its own positional encoding, which stays with the caller's autograd);
 *   hr_train_rows_backward  d_rows_dev -> d_head_dev (n, Zc * Pc); rows_scratch_dev: (n * Zc, casc_row_dim) workspace. */
int hr_train_rows_forward(hr_model* m, const float* rays_dev, const float* head_dev, int64_t n_rays, float* rows_dev, void* stream);
int hr_train_rows_backward(hr_model* m, const float* rays_dev, const float* head_dev, const float* d_rows_dev, int64_t n_rays,
                           float* rows_scratch_dev, float* d_head_dev, void* stream);

/* rays (n, ray_dim) -> feats_dev (n, mlp_in): ray parameterisation + positional encoding (nlf/param.py, nlf/pe.py) */
int hr_train_features(hr_model* m, const float* rays_dev, int64_t n_rays, float* feats_dev, void* stream);

/* rgb_dev (n, 3), not clamped.  `params`: current parameter values, re-packed into the model's texel layout on `stream`
 * before the launch (NULL: keep what the model holds).  white_bg: this step's background decision
 * (`white_bg or (training and rand() < 0.5)`, tensorf_no_sample.py:236). */
int hr_train_forward(hr_model* m, const hr_train_tensors* params, const float* rays_dev, const float* head_dev, int64_t n_rays,
                     int32_t white_bg, float* rgb_dev, void* stream);
/* hr_train_forward that also writes per-sample values of ITS OWN forward -- fields->distances_dev (n, Z), points_dev (n, Z, 3),
 * weights_dev (n, Z), by sorted rank, the definitions of hr_render_fields; NULL members are skipped, sigma_dev / head_dev must be NULL --
 * so that a training step whose regularisers read such fields (INRSystem.training_step passes their names on the main forward,
 * nlf/__init__.py:658-690) needs no second, inference pass over re-uploaded weights.  Up to 64 samples per ray. */
int hr_train_forward_fields(hr_model* m, const hr_train_tensors* params, const float* rays_dev, const float* head_dev, int64_t n_rays,
                            int32_t white_bg, float* rgb_dev, const hr_fields* fields, void* stream);

/* Given d_rgb_dev (n, 3) writes d_head_dev (n, z_channels * preds_per_z) and every non-NULL tensor of `grads` (overwritten,
 * not accumulated), for the parameter values of the last hr_train_forward / hr_model_finalize. */
int hr_train_backward(hr_model* m, const float* rays_dev, const float* head_dev, const float* d_rgb_dev, int64_t n_rays,
                      int32_t white_bg, float* d_head_dev, const hr_train_tensors* grads, void* stream);

/* The Linear layers of the sample-prediction MLP in training (BaseMLP.forward under autograd, nlf/nets/mlp.py:159-172;
 * INRSystem.training_step, nlf/__init__.py:634-709), no model involved; all tensors device memory, float32, row-major with
 * the given leading dimensions (so that the `cat([input, x])` of a skip layer can be a view into a wider buffer).  Every
 * fp32 GEMM runs on the matrix cores as bf16 MFMA products of split operands with fp32 accumulation (bf16 parts because
 * gradients span the fp32 exponent range): the backward GEMMs as three products of hi/lo halves (the bf16x3 arithmetic of
 * the render path), the forward as six products of a three-way split (24 mantissa bits: its output feeds the sample stage's
 * threshold decisions, which must fall as in the fp32 reference).
 *   forward:   y (rows, out) = act(x (rows, in) W^T + b),  W (out, in) as torch stores nn.Linear.weight;
 *              act = LeakyReLU(leaky_slope) when leaky_slope >= 0, none when < 0 (the last Linear)
 *   backward:  with dy (rows, out) the gradient of y and, for an activated layer, y itself (its sign is LeakyReLU's mask):
 *              dy' = dy * (y > 0 ? 1 : slope);  dx (rows, in) = dy' W (skipped when dx_dev is NULL);  dw (out, in) = dy'^T x;
 *              db (out) = column sums of dy'.  The batch dimension of dw / db is reduced in a fixed order (no atomics).
 *              workspace_dev: hr_linear_workspace(rows, in, out) bytes. */
size_t hr_linear_workspace(int64_t rows, int32_t in, int32_t out);
/* The ray MLP's FORWARD of a training step in ONE launch (BaseMLP.forward, nlf/nets/mlp.py:159-172, as INRSystem.training_step runs it,
 * nlf/__init__.py:658-690): weights_dev[l] / biases_dev[l] are the CURRENT values of the reference's parameters (torch layout (out, in) /
 * (out), device memory) -- the library splits them into bf16 hi / lo tiles on the device first (three v_mfma_f32_32x32x16_bf16 products
 * per fp32 GEMM, fp32 accumulation: head within 7e-6 of max |head| of the fp32 chain; bf16 halves keep the fp32 exponent range
 * whatever the weights become).  rays_dev (n, ray_dim) -> head_dev (n, Z * P) in the caller's column order (columns no stage reads: 0),
 * and the output of hidden Linear l after its LeakyReLU -> acts_dev[l] + ray * act_ld[l] + act_off[l] + feature, fp32 (l < layers - 1;
 * NULL: not kept): what hr_linear_backward needs as `x` of layer l + 1 and `y` of layer l (a skip layer's input starts at column mlp_in
 * of a wider row).  Hidden width 256, no cascades; the activation / encoding schedules are those of the last hr_model_update_config. */
int hr_mlp_train_forward(hr_model* m, const float* const* weights_dev, const float* const* biases_dev, const float* rays_dev, int64_t n_rays,
                         float* const* acts_dev, const int64_t* act_ld, const int32_t* act_off, float* head_dev, void* stream);

int hr_linear_forward(const float* x_dev, int64_t ldx, int64_t rows, int32_t in, const float* w_dev, const float* b_dev, int32_t out,
                      float leaky_slope, float* y_dev, int64_t ldy, void* stream);
int hr_linear_backward(const float* x_dev, int64_t ldx, const float* w_dev, const float* y_dev, int64_t ldy, const float* dy_dev, int64_t ld_dy,
                       int64_t rows, int32_t in, int32_t out, float leaky_slope, float* dx_dev, int64_t ld_dx, float* dw_dev, float* db_dev,
                       float* workspace_dev, void* stream);

/* Occupancy of the feature grids: TensorBase.getDenseAlpha (nlf/nets/tensorf_base.py:381-401) and its keyframe
 * override (nlf/nets/tensorf_dynamic.py:499-536) -- alpha = 1 - exp(-sigma * length) at the n[0] x n[1] x n[2] lattice points
 * aabb0 * (1 - s) + aabb1 * s, s = linspace(0, 1, n) of the model's box, written to alpha_dev (n[0], n[1], n[2]) (x slowest);
 * keyframe nets take the maximum over the `num_frames` frames of the sequence.  prev_volume_dev (D = prev_n[2], H = prev_n[1],
 * W = prev_n[0]; may be NULL) is the previous mask with its box prev_aabb[6]: points where its trilinear sample
 * (AlphaGridMask.sample_alpha, utils/tensorf_utils.py:459-484) is not positive get alpha 0, as in compute_alpha
 * (tensorf_base.py:489-507).  The max-pool / threshold / crop that follow are host-side tensor ops. */
int hr_dense_alpha(hr_model* m, const int32_t n[3], float length, int32_t num_frames, const float* prev_volume_dev, const int32_t prev_n[3],
                   const float prev_aabb[6], float* alpha_dev, void* stream);

/* Viewer hand-over: rgb_dev (h * w, 3) float32 as hr_render wrote it -> out_dev, the buffer NeRFGUI.test_step
 * builds on the host (utils/gui_utils.py:174-205): transposed to (w, h) if `transpose`, then flipped vertically if `flip`;
 * rgba8 != 0: 4 bytes per pixel, to8b(x) = (uint8)(255 * clip(x, 0, 1)) (utils/__init__.py:47) and alpha 255;
 * rgba8 == 0: 3 floats per pixel, values unchanged. */
int hr_pack_display(const float* rgb_dev, int32_t h, int32_t w, int32_t transpose, int32_t flip, int32_t rgba8, void* out_dev, void* stream);

/* Image scores: what the reference computes on the host for every validation image (nlf/__init__.py:976-980:
 * val/psnr and val/ssim from metrics.py:25-35, scikit-image's peak_signal_noise_ratio(data_range=1.0) and
 * structural_similarity(win_size=11, gaussian_weights=True, multichannel=True, data_range=1.0), after results['rgb'].cpu().numpy())
 * and, as psnr_gpu (metrics.py:37-45), for every training step (nlf/__init__.py:668).  Written on the device as SUMS: the
 * divisions and the logarithm are host arithmetic on four doubles (mse = sse / (3 h w), psnr = -10 log10(mse),
 * ssim = (ssim_sum[0] + ssim_sum[1] + ssim_sum[2]) / (3 (h - 10) (w - 10))), and the sums of the tiles of image-parallel ranks add. */
typedef struct hr_image_scores {
    double sse;                 /* sum over all 3*h*w values of (pred - gt)^2: fp32 differences and squares, added in double */
    double ssim_sum[3];         /* per channel: sum of the SSIM map S over the (h-10)*(w-10) pixels at least 5 away from every border
                                 * (the crop scikit-image applies); S from the 11-tap Gaussian window (sigma 1.5), population
                                 * covariances, C1 = 0.01^2, C2 = 0.03^2 */
} hr_image_scores;

/* bytes of workspace_dev that a call on an h x w frame needs (either value of want_ssim); 0 for h < 1 or w < 1 */
size_t hr_image_metrics_workspace(int32_t h, int32_t w);

/* pred_dev, gt_dev: (h * w, 3) float32, as hr_render writes a frame -> *out_dev (device memory).  One read of each image serves both
 * scores.  want_ssim == 0 (the per-step train/psnr, metrics.py:37-45): the squared-error sum alone, any h, w >= 1, ssim_sum left at 0;
 * otherwise h, w >= 11 (HR_E_INVALID below that: the window does not fit).  The sums are added in a fixed order without atomics:
 * calls on the same inputs give the same bits.  Every byte of *out_dev and of the workspace that is read is written first by the same
 * call (nothing to clear between calls); no allocation, no synchronisation, capturable in a hipGraph.  No model is involved. */
int hr_image_metrics(const float* pred_dev, const float* gt_dev, int32_t h, int32_t w, int32_t want_ssim, hr_image_scores* out_dev,
                     void* workspace_dev, void* stream);

/* LPIPS: the third score of the reference's results tables, which it computes on the host after a copy of the frame
 * (metrics.py:54-58 compute_lpips; utils/tensorf_utils.py:76-88 rgb_lpips with the nets 'alex' and 'vgg', version '0.1',
 * normalize=True).  LPIPS v0.1 in eval mode; the definition is stated once in csrc/hr_lpips.h: images * 2 - 1, the scaling layer,
 * the backbone on both images, five taps, channel-unit-normalised squared differences weighted by the non-negative `lin` layers,
 * spatial means, summed.  The pretrained weights are the CALLER's (torchvision's backbone, the lpips package's lin layers): nothing
 * is shipped, and agreement with published numbers rests on them.  Additive: no existing struct or signature moved
 * (HR_ABI_VERSION stays). */
enum { HR_LPIPS_ALEX = 0, HR_LPIPS_VGG = 1 };
struct hr_lpips;                /* (no typedef: the call below has the name; say `struct hr_lpips`) */
typedef struct hr_lpips_scores {
    double layer[5];            /* per tap: mean over its pixels of sum_c lin[c] (n_pred[c] - n_gt[c])^2 */
    double total;               /* layer[0] + ... + layer[4] in that order: the LPIPS distance */
} hr_lpips_scores;

/* conv_w[i], conv_b[i]: the i-th convolution's weight (cout, cin, k, k) and bias (cout) as torch holds them (OIHW, float32,
 * contiguous), 5 of them for HR_LPIPS_ALEX and 13 for HR_LPIPS_VGG; lin_w[k]: the C_k weights of tap k's 1x1 convolution (C_k = 64,
 * 192, 384, 256, 256 for alex, 64, 128, 256, 512, 512 for vgg).  Each pointer may be host or device memory.  The object owns its
 * copies: the weights packed into the matrix instructions' operand order, on the current device.  Synchronises the device once.
 * HR_E_INVALID for a NULL pointer or an unknown net. */
int hr_lpips_create(int32_t net, const float* const* conv_w, const float* const* conv_b, const float* const* lin_w,
                    struct hr_lpips** out);
void hr_lpips_destroy(struct hr_lpips* p);

/* bytes of workspace_dev that a call on an h x w frame needs; 0 for an unknown net, a frame below the minimum (31 x 31 for alex,
 * 16 x 16 for vgg: every tap is at least 1 x 1) or one whose layers pass 2^31 pixels */
size_t hr_lpips_workspace(int32_t net, int32_t h, int32_t w);

/* pred_dev, gt_dev: (h * w, 3) float32 in [0, 1], as hr_render writes a frame -> *out_dev (device memory).  workspace_dev: at least
 * hr_lpips_workspace(net, h, w) bytes, 16-byte aligned.  Only kernels on `stream`: no allocation, no synchronisation, no memset;
 * every byte of *out_dev and of the workspace that is read is written first by the same call; capturable in a hipGraph.  The sums
 * are added in a fixed order without atomics: calls on the same inputs give the same bits, (pred, gt) and (gt, pred) too.
 * HR_E_INVALID, before anything is launched, for a NULL pointer, a frame below the minimum or too large, a misaligned workspace.
 * The distance of a frame is not the sum of its tiles' (receptive fields cross the cut): score whole frames. */
int hr_lpips(const struct hr_lpips* p, const float* pred_dev, const float* gt_dev, int32_t h, int32_t w, hr_lpips_scores* out_dev,
             void* workspace_dev, void* stream);

/* Training image loss: INRSystem.training_step's
 *     image_loss = self.loss(results['rgb'] * weight, rgb * weight, **batch)            (nlf/__init__.py:665)
 * for the modules of losses.py's loss_dict that accept that call, with the squared error train/psnr needs (psnr_gpu, :668) from the
 * same read.  `type` is one of the five values below, optionally | HR_LOSS_PREMULTIPLIED.  Per element, with prediction p, target g and
 * the ray's weight w (1 where weight_dev is NULL):
 *     d = p*w - g*w  (two fp32 products, one fp32 subtraction), dd/dp = w;
 *     with HR_LOSS_PREMULTIPLIED (p and g already carry the weight, the reference's own call form): d = p - g, dd/dp = 1;
 *   type                  term                                            d term / d d
 *   HR_LOSS_MSE           d*d                                             2*d
 *   HR_LOSS_WEIGHTED_MSE  w*d*d                                           2*w*d
 *   HR_LOSS_MAE           |d|                                             sign(d), sign(0) = 0
 *   HR_LOSS_WEIGHTED_MAE  w*|d|                                           w*sign(d)
 *   HR_LOSS_HUBER         |d| < delta ? d*d/2 : delta*(|d| - delta/2)     |d| < delta ? d : delta*sign(d)       (nn.HuberLoss)
 * The loss is the mean of the terms over all 3 * n_rays elements. */
#define HR_LOSS_MSE 0
#define HR_LOSS_WEIGHTED_MSE 1
#define HR_LOSS_MAE 2
#define HR_LOSS_WEIGHTED_MAE 3
#define HR_LOSS_HUBER 4
#define HR_LOSS_PREMULTIPLIED 0x100

typedef struct hr_loss_out {
    double loss_sum;            /* sum of the 3 * n_rays terms: fp32 terms, added in double */
    double sse;                 /* sum of (pred - gt)^2 over the values as passed, without the weight: hr_image_scores.sse of the batch */
    float loss;                 /* loss_sum / (3 * n_rays), formed in double and rounded once */
    float pad;                  /* written as 0 */
} hr_loss_out;

/* bytes of workspace_dev that a call on n_rays rays needs; 0 for n_rays < 1 */
size_t hr_image_loss_workspace(int64_t n_rays);

/* pred_dev, gt_dev: (n_rays, 3) float32; weight_dev: (n_rays, 1) float32 or NULL (every weight 1) -> *out_dev (device memory) and, when
 * d_pred_dev is not NULL, d_pred_dev (n_rays, 3) = d loss / d pred, times *upstream_dev (one float in device memory, read by the
 * kernel: no host read of an upstream gradient; NULL: 1).  delta is read by HR_LOSS_HUBER only and must be > 0 there.  One pass over the
 * three inputs.  The sums are added in a fixed order without atomics: calls on the same inputs give the same bits.  Every byte of
 * *out_dev and of the workspace that is read is written first by the same call (nothing to clear between calls); no allocation, no
 * synchronisation, capturable in a hipGraph.  n_rays < 1, an unknown type and a NULL pred / gt / out / workspace are HR_E_INVALID. */
int hr_image_loss(const float* pred_dev, const float* gt_dev, const float* weight_dev, int64_t n_rays, int32_t type, float delta,
                  const float* upstream_dev, hr_loss_out* out_dev, float* d_pred_dev, void* workspace_dev, void* stream);

/* The reference's per-step background coin (`white_bg or (training and rand() < 0.5)`, tensorf_no_sample.py:236) where a replayed
 * graph can flip it: on the device.  hr_train_background_coin (host): 1 when training step `step` of `seed` composites over white --
 * one Philox4x32-10 word of (seed, step), its top bit, drawn with a counter no sampled row of that step uses (csrc/hr_sample_rng.h:
 * hr_background_coin, the same function the kernels call).  It does not reproduce torch's stream: the contract is "a fair coin, fixed by
 * (seed, step), independent of the step's rays".
 * hr_train_set_background: source 0 (the default) -- the white_bg argument of hr_train_forward* / hr_train_backward decides, as before;
 * source 1 -- those calls ignore their white_bg argument: a model whose configuration has white_bg set is white at every step, any other
 * one takes hr_train_background_coin(seed, *step_dev), with *step_dev (int64, device memory, e.g. hr_adam_step_dev's count) read when
 * the kernels run.  The forward and the backward of one step see the same count when it advances after the backward, as
 * hr_adam_step_dev does.  (hr_config.white_bg is already `white_bg and not black_bg`; a black_bg configuration is not bound to the
 * coin by the Python layer.)  step_dev must stay valid while source is 1.  Additive: no existing struct or signature moved
 * (HR_ABI_VERSION stays). */
int32_t hr_train_background_coin(uint64_t seed, uint64_t step);
int hr_train_set_background(hr_model* m, int32_t source, uint64_t seed, const int64_t* step_dev);

/* TensoRF regularisers of one (1, C, H, W) float32 plane (TVLoss, nlf/regularizers/tensorf.py:14-34; density_L1,
 * nlf/nets/tensorf_base.py:1024-1035), no model involved.  Forward ADDS to sums_dev[3] =
 *   { sum (x[:, 1:, :] - x[:, :-1, :])^2,  sum (x[:, :, 1:] - x[:, :, :-1])^2,  sum |x| };
 * backward writes grad_dev = coef_dev[0] * d sums[0]/dx + coef_dev[1] * d sums[1]/dx + coef_dev[2] * sign(x), with the
 * three upstream coefficients read from device memory (no host synchronisation inside a training step). */
int hr_plane_reg_forward(const float* plane_dev, int32_t channels, int32_t h, int32_t w, float* sums_dev, void* stream);
int hr_plane_reg_backward(const float* plane_dev, int32_t channels, int32_t h, int32_t w, const float* coef_dev, float* grad_dev, void* stream);

/* The reference's whole TensoRF regulariser (nlf/regularizers/tensorf.py:57-89: density_L1, TV_loss_density, TV_loss_app) over up to
 * HR_REG_MAX_TENSORS planes and lines in ONE pass: the value, and the gradient ADDED into the parameters' gradient buffers.  The gradient of
 * these terms is linear in the step's weights and independent of the sums, so each plane is read once and its gradient read-modify-written
 * once.  Per tensor t with sums Sh = sum (x[:, 1:, :] - x[:, :-1, :])^2, Sw = sum (x[:, :, 1:] - x[:, :, :-1])^2, Sl = sum |x|:
 *   value_t = w[slot_h] * kh * Sh + w[slot_w] * kw * Sw + w[slot_l] * kl * Sl
 *   grad   += w[slot_h] * kh * dSh/dx + w[slot_w] * kw * dSw/dx + w[slot_l] * kl * sign(x)
 * with w = weights_dev (HR_REG_SLOTS floats in DEVICE memory, read when the kernel runs: a replayed graph sees what the host last wrote)
 * and kh, kw, kl the static factors the reference's expressions put in front of the sums (TVLoss: 1e-2 * 2 / (C (H - 1) W) and
 * 1e-2 * 2 / (C H (W - 1)); density_L1: 1 / (C H W)), formed in double by the caller.  A slot of -1 leaves its term out. */
#define HR_REG_MAX_TENSORS 12
#define HR_REG_SLOTS 3          /* by convention of the Python layer: 0 L1, 1 density TV, 2 appearance TV */
typedef struct hr_reg_tensor {
    const float* plane_dev;     /* (1, channels, h, w) float32, contiguous */
    float* grad_dev;            /* same shape: added to */
    int32_t channels, h, w;
    float kh, kw, kl;
    int32_t slot_h, slot_w, slot_l;    /* 0 .. HR_REG_SLOTS - 1, or -1: the term is absent */
    int32_t reserved;
} hr_reg_tensor;
typedef struct hr_reg_plan hr_reg_plan;
/* Checks the table and allocates the per-workgroup partial sums the call reduces through.  HR_E_INVALID, naming the tensor, before
 * anything is allocated or launched: more than HR_REG_MAX_TENSORS tensors, channels < 0, h < 1 or w < 1, a NULL plane or gradient of
 * a tensor that has elements, a slot outside -1 .. HR_REG_SLOTS - 1, a tensor with a TV term (slot_h or slot_w >= 0) and h < 2 or
 * w < 2 (the reference divides by a zero count there).  Tensors with channels == 0 are skipped, as the reference skips its
 * n_comp == 0 planes.  The plan holds the pointers: build a new one when a tensor or its gradient buffer is replaced. */
int hr_reg_plan_create(const hr_reg_tensor* tensors, int32_t n_tensors, hr_reg_plan** out);
/* The same table with other pointers (autograd hands out a new gradient buffer after zero_grad(set_to_none=True)): checked as above, and
 * every tensor must keep its shape.  Host work only -- no allocation; launches already enqueued or recorded keep the pointers they had. */
int hr_reg_plan_update(hr_reg_plan* plan, const hr_reg_tensor* tensors, int32_t n_tensors);
/* One launch over every tensor (a workgroup owns 4096 consecutive elements of one tensor; 16-byte loads and stores where w % 4 == 0
 * and both buffers are 16-byte aligned), then a one-workgroup finishing launch that adds the partial sums in a fixed order:
 *   loss_dev[0] = sum over slots of w[s] * loss_dev[1 + s];   loss_dev[1 + s] = sum over the terms of slot s of k * S   (unweighted)
 * No float atomics, no memset, no allocation, no synchronisation: calls on the same inputs give the same bits, and the call is capturable
 * in a hipGraph.  add_grad == 0 computes the value only (the reference's warm-up: the term is logged, not trained on).
 * Additive: no existing struct or signature moved (HR_ABI_VERSION stays). */
int hr_tensorf_reg(const hr_reg_plan* plan, const float* weights_dev, float* loss_dev, int32_t add_grad, void* stream);
void hr_reg_plan_destroy(hr_reg_plan* plan);

/* The optimizer of the training loop (utils/__init__.py:49-76: torch.optim.Adam(params, lr, eps=1e-8, weight_decay, betas=(0.9, 0.99)); stepped by
 * Lightning after INRSystem.training_step, nlf/__init__.py:634-709): one Adam step over any number of parameter tensors in ONE pass over memory
 * (28 bytes per parameter).  Tensor i is n[i] contiguous floats at param_dev[i] with its gradient, first and second moment (torch's state names
 * exp_avg / exp_avg_sq) in grad_dev[i], exp_avg_dev[i], exp_avg_sq_dev[i]; the pointer arrays and hp are HOST memory.  hp holds six doubles per
 * tensor: lr, beta1, beta2, eps, weight_decay, step (the 1-based step count this call performs -- bias corrections are 1 - beta^step; doubles
 * because torch derives 1 - beta and the corrections from Python floats).  The arithmetic is torch/optim/adam.py's single-tensor form
 * (amsgrad / maximize off), evaluated in fp32. */
int hr_adam_step(float* const* param_dev, const float* const* grad_dev, float* const* exp_avg_dev, float* const* exp_avg_sq_dev, const int64_t* n,
                 const double* hp, int32_t n_tensors, void* stream);
/* hr_adam_step with the step count and the learning rates in DEVICE memory, so that one captured launch performs a new step on every
 * replay.  The pointer arrays, n and n_tensors as above.  hp holds FOUR doubles per tensor: beta1, beta2, eps, weight_decay (host).
 * *step_dev (int64) is the 0-based count of steps already done: the call performs step t = *step_dev + 1 with hr_adam_step's arithmetic,
 * the bias corrections 1 - beta^t evaluated in double on the device (pow), the step size (double)lr / (1 - beta1^t) rounded to float as
 * there.  Tensor i's learning rate is lr_dev[lr_index[i]] (floats in device memory, one per parameter group; lr_index is host memory,
 * every entry in [0, n_lr)).  After every tensor has been stepped a stream-ordered single-thread launch stores t into *step_dev: no
 * workgroup of this call can see the advanced count, and the next call on the stream sees it.  Only kernels on `stream`: no allocation,
 * no synchronisation, no memset; capturable in a hipGraph.  A call with nothing to step (n_tensors == 0, or every n[i] == 0) leaves
 * the counter alone.  Additive: no existing struct or signature moved (HR_ABI_VERSION stays). */
int hr_adam_step_dev(float* const* param_dev, const float* const* grad_dev, float* const* exp_avg_dev, float* const* exp_avg_sq_dev, const int64_t* n,
                     const double* hp, const int32_t* lr_index, int32_t n_lr, const float* lr_dev, int64_t* step_dev, int32_t n_tensors, void* stream);

/* The two stages of hr_render on their own, for profiling: the sample-prediction MLP
 * (rays -> raw head in the workspace) and the per-sample stage (head -> rgb).  n_rays
 * must not exceed the reserved chunk size. */
int hr_stage_mlp(hr_model* m, const float* rays_dev, int64_t n_rays, void* stream);
int hr_stage_samples(hr_model* m, const float* rays_dev, int64_t n_rays, float* rgb_dev, void* stream);

/* The per-sample colour network of an HR_SHADING_MLP_FEA / HR_SHADING_MLP model (`renderModule`, nlf/nets/tensorf_base.py:38-69, 106-135;
 * called at nlf/nets/tensorf_no_sample.py:208-219): three Linears of hidden width feature_c over
 *   MLP_FEA: [f, v, PE(f, fea_pe), PE(v, view_pe)]      MLP: [f, v, PE(v, view_pe)]        (fea_pe is not read)
 * with f the 27 appearance features after basis_mat, v the sample's view direction and PE utils/tensorf_utils.py:232-239's
 * cat[sin(p_i 2^j), cos(p_i 2^j)] (index i * F + j; a PE of 0 frequencies is left out), ReLU between the Linears, sigmoid after the last.
 * view_pe, fea_pe in 0..6, feature_c in 1..256.
 * hr_model_set_shading_mlp: between hr_model_create and hr_model_finalize of a model with such a shading (HR_E_INVALID for another model,
 * a cascade, more than 64 samples per ray or a value out of range).  hr_model_upload then takes `renderModule.mlp.{0,2,4}.weight|bias` in
 * the reference's (out, in) layout; hr_model_finalize returns HR_E_STATE, naming it, while the descriptor or one of the six tensors is
 * missing.  Such a model renders through every hr_render* entry point (its own three-launch sample stage: DESIGN 3l; never the frame
 * kernel or the verified fast path); the hr_train_* entry points return HR_E_INVALID for it.
 * hr_stage_shade: the network alone on n rows -- feat_dev (n, 27), viewdirs_dev (n, 3) -> rgb_dev (n, 3), one launch on `stream`, no
 * allocation, no synchronisation.  Additive: no existing struct or signature moved (HR_ABI_VERSION stays). */
typedef struct hr_shading_mlp {
    int32_t view_pe, fea_pe, feature_c;
} hr_shading_mlp;
int hr_model_set_shading_mlp(hr_model* m, const hr_shading_mlp* desc);
int hr_stage_shade(hr_model* m, const float* feat_dev, const float* viewdirs_dev, int64_t n, float* rgb_dev, void* stream);

/* Time-dependent colour of a keyframe net (`shadingMode: RGBtLinear | RGBtFourier`, utils/tensorf_utils.py:351-400) and `RGBIdentity`
 * (:346-348) of a static net.  The appearance features after basis_mat are the coefficients of a per-ray basis of nb functions,
 *   RGBT_LINEAR   [1, t]                                              nb = 2
 *   RGBT_FOURIER  [t, cos(2 pi f s) f = 0 .. fpk-1, sin(2 pi f s) ..]   nb = 2 fpk + 1,  s = time_offset * num_keyframes * (num_frames - 1) / num_frames
 * with t the ray's time (its last column) and time_offset its distance to the keyframe before it; colour c = relu(sum_j basis_j *
 * feature[c * nb + j] + 0.5), app_dim = 3 nb.  RGB_IDENTITY: colour c = |feature[c] + 0.5|, app_dim = 3, no descriptor.
 * `densityMode: DensityLinear | DensityFourier` (:407-456): the density before its activation is sum_j basis_j * feature_d[j], with
 * feature_d = basis_mat_density . (the density components) and the same bases; any of HR_SHADING_RGB / SH / RGBT_* beside it.
 * hr_model_set_time_decode: between hr_model_create and the first upload (HR_E_STATE later) of a keyframe model with an
 * HR_SHADING_RGBT_* shading or a density mode.  HR_E_INVALID, naming it: a static net or a cascade, neither an RGBT shading nor a
 * density mode, frames_per_keyframe outside 1..HR_TIME_MAX_FPK, an app_dim that is not 3 nb, a density mode beside an MLP shading
 * mode, or a density row that does not fit the workgroup's LDS.  With a density mode hr_model_upload then takes
 * `basis_mat_density.weight` (nb, sum n_den).  hr_model_finalize returns HR_E_STATE, naming the call, for an RGBT model without it.
 * Such a model renders through every hr_render* entry point (its own sample kernel; never the frame kernel or the
 * verified fast path: HR_MLP_AUTO / F16F8 / F16F8V run f16x3).  The hr_train_* entry points differentiate the three colour modes
 * (their own build of the training kernels, the deterministic one included); with a density mode they, and hr_dense_alpha, return
 * HR_E_INVALID naming it.  Additive: no existing struct or signature moved. */
#define HR_TIME_MAX_FPK 8
enum { HR_DENSITY_PLAIN = 0, HR_DENSITY_LINEAR = 1, HR_DENSITY_FOURIER = 2 };
typedef struct hr_time_decode {
    int32_t density_mode;                /* HR_DENSITY_* */
    int32_t frames_per_keyframe;         /* net.frames_per_keyframe, else num_frames // num_keyframes (tensorf_dynamic.py:51-55) */
    int32_t num_frames;                  /* dataset.num_frames */
} hr_time_decode;
int hr_model_set_time_decode(hr_model* m, const hr_time_decode* desc);

/* Profiling aid: runs the MLP stage with a per-wave phase timeline.  trace_dev receives 64
 * s_memtime stamps per wave (4 waves per workgroup, workgroups of 64 or 128 rays); only the
 * split-precision kernel records stamps. */
int hr_debug_trace_mlp(hr_model* m, const float* rays_dev, int64_t n_rays, unsigned long long* trace_dev, void* stream);

/* bytes of device memory held by the model (packed grids + weights + workspace) */
int64_t hr_model_device_bytes(const hr_model* m);

void hr_model_destroy(hr_model* m);

#ifdef __cplusplus
}
#endif
#endif /* HYPERREEL_HIP_H */
