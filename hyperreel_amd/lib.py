"""ctypes binding of libhyperreel_hip.so (include/hyperreel_hip.h).

There is deliberately no fallback: if the library is missing or a call fails this module
raises.  The product never routes through PyTorch ops or the CPU oracle.
"""
import ctypes as C
import os

from .plan import hr_camera, hr_config, hr_fields, hr_fisheye, hr_lightfield, hr_maps, hr_ndc, hr_shading_mlp, hr_time_decode

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, '_build', 'libhyperreel_hip.so')

ABI_VERSION = 27



HR_OPT_FRAME_KERNEL, HR_OPT_SAMPLE_WAVES, HR_OPT_FRAME_KERNEL_ACTIVE, HR_OPT_MLP_PRECISION_ACTIVE, HR_OPT_MLP_OVERFLOW, HR_OPT_MLP_CALIBRATED = 0, 1, 2, 3, 4, 5
HR_OPT_TRAIN_DETERMINISTIC = 6
HR_OPT_MLP_F8_SATURATED = 7
HR_OPT_MLP_VERIFIED, HR_OPT_REDO_COUNT, HR_OPT_REDO_OVERFLOW, HR_OPT_WIDE_COUNT, HR_OPT_CHUNK_RAYS = 8, 9, 10, 11, 12
HR_E_RANGE = -5


class hr_train_tensors(C.Structure):
    """Device pointers of the trainable tensors (or of their gradients), reference layouts (include/hyperreel_hip.h)."""
    _fields_ = [('density_a', C.c_void_p * 3), ('density_b', C.c_void_p * 3), ('app_a', C.c_void_p * 3), ('app_b', C.c_void_p * 3),
                ('basis', C.c_void_p), ('color_table', C.c_void_p)]


class hr_image_scores(C.Structure):
    """Result of hr_image_metrics, written on the device (include/hyperreel_hip.h)."""
    _fields_ = [('sse', C.c_double), ('ssim_sum', C.c_double * 3)]


class hr_lpips_scores(C.Structure):
    """Result of hr_lpips, written on the device (include/hyperreel_hip.h)."""
    _fields_ = [('layer', C.c_double * 5), ('total', C.c_double)]


HR_LPIPS_ALEX, HR_LPIPS_VGG = 0, 1


class hr_loss_out(C.Structure):
    """Result of hr_image_loss, written on the device (include/hyperreel_hip.h)."""
    _fields_ = [('loss_sum', C.c_double), ('sse', C.c_double), ('loss', C.c_float), ('pad', C.c_float)]


class hr_reg_tensor(C.Structure):
    """One plane or line of hr_tensorf_reg's descriptor table (include/hyperreel_hip.h)."""
    _fields_ = [('plane_dev', C.c_void_p), ('grad_dev', C.c_void_p), ('channels', C.c_int32), ('h', C.c_int32), ('w', C.c_int32),
                ('kh', C.c_float), ('kw', C.c_float), ('kl', C.c_float), ('slot_h', C.c_int32), ('slot_w', C.c_int32), ('slot_l', C.c_int32),
                ('reserved', C.c_int32)]


HR_REG_MAX_TENSORS, HR_REG_SLOTS = 12, 3
HR_E_INVALID = -1
HR_LOSS_MSE, HR_LOSS_WEIGHTED_MSE, HR_LOSS_MAE, HR_LOSS_WEIGHTED_MAE, HR_LOSS_HUBER = 0, 1, 2, 3, 4
HR_LOSS_PREMULTIPLIED = 0x100


class hr_verify_info(C.Structure):
    """What the verified fast path rests on for one model (include/hyperreel_hip.h)."""
    _fields_ = [('verified', C.c_int32), ('fallback', C.c_int32), ('band', C.c_float), ('band_q', C.c_float), ('band_off', C.c_float),
                ('band_floor', C.c_float), ('max_d_zc', C.c_float), ('max_d_dist_n', C.c_float), ('max_d_geo_n', C.c_float), ('max_d_off', C.c_float),
                ('max_d_dist', C.c_float), ('max_d_head', C.c_float), ('listed_frac', C.c_float), ('max_d_rgb', C.c_float),
                ('n_rays', C.c_int64), ('n_rays_used', C.c_int64), ('n_samples', C.c_int64), ('n_flipped', C.c_int64), ('n_shaky', C.c_int64)]


# hr_rayset_set_pixel_format's formats (include/hyperreel_hip.h)
HR_PIXELS_RGB8, HR_PIXELS_RGBA8_WHITE = 0, 1
# hr_png_encode's pixel types and its adaptive filter mode (the fixed ones are the PNG filter numbers 0..4)
HR_PNG_U8, HR_PNG_F32_TO8B = 0, 1
HR_PNG_FILTER_ADAPTIVE = 5
# hr_jpeg_encoder_create's subsampling (PIL's numbers)
HR_JPEG_444, HR_JPEG_422, HR_JPEG_420 = 0, 1, 2
# hr_png_decode's per-image status codes, by value
PNG_STATUS_NAMES = ('OK', 'BAD_SIGNATURE', 'BAD_CHUNK', 'BAD_CRC', 'UNSUPPORTED', 'SIZE_MISMATCH', 'BAD_ZLIB_HEADER', 'BAD_BLOCK', 'BAD_CODE',
                    'BAD_DISTANCE', 'TRUNCATED', 'TOO_LONG', 'TOO_SHORT', 'BAD_ADLER', 'BAD_FILTER', 'BAD_OFFSETS')


# hr_jpeg_decode's per-image status codes, by value
JPEG_STATUS_NAMES = ('OK', 'NO_SOI', 'BAD_MARKER', 'UNSUPPORTED', 'SIZE_MISMATCH', 'BAD_TABLE', 'BAD_CODE', 'BAD_COEF', 'BAD_RESTART', 'TRUNCATED',
                     'TOO_LONG', 'BAD_OFFSETS')


class hr_jpeg_info(C.Structure):
    """Result of hr_jpeg_probe (include/hyperreel_hip.h)."""
    _fields_ = [('width', C.c_int32), ('height', C.c_int32), ('components', C.c_int32), ('h_samp', C.c_int32), ('v_samp', C.c_int32),
                ('restart_interval', C.c_int32), ('supported', C.c_int32), ('status', C.c_int32)]


class hr_png_info(C.Structure):
    """Result of hr_png_probe (include/hyperreel_hip.h)."""
    _fields_ = [('width', C.c_int32), ('height', C.c_int32), ('bit_depth', C.c_int32), ('color_type', C.c_int32), ('channels', C.c_int32),
                ('interlace', C.c_int32), ('supported', C.c_int32), ('reserved', C.c_int32)]


class hr_rayset_image_info(C.Structure):
    """Result of hr_rayset_image_info (include/hyperreel_hip.h)."""
    _fields_ = [('count', C.c_int64), ('num_take', C.c_int64), ('every', C.c_int32), ('offset', C.c_int32), ('is_list', C.c_int32),
                ('prev', C.c_int32), ('threshold', C.c_float), ('dir_z_below', C.c_float)]


# every symbol include/hyperreel_hip.h declares: (name, restype, argtypes)
SYMBOLS = [
    ('hr_abi_version', C.c_int, []),
    ('hr_sizeof_config', C.c_int, []),
    ('hr_last_error', C.c_char_p, []),
    ('hr_model_create', C.c_int, [C.POINTER(hr_config), C.POINTER(C.c_void_p)]),
    ('hr_model_create_cascade', C.c_int, [C.POINTER(hr_config), C.POINTER(hr_config), C.POINTER(C.c_void_p)]),
    ('hr_model_upload', C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]),
    ('hr_model_finalize', C.c_int, [C.c_void_p]),
    ('hr_model_calibrate', C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_float), C.c_void_p]),
    ('hr_model_update_config', C.c_int, [C.c_void_p, C.POINTER(hr_config), C.c_void_p]),
    ('hr_model_reserve', C.c_int, [C.c_void_p, C.c_int64]),
    ('hr_model_set_option', C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    ('hr_model_get_option', C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    ('hr_model_verify_info', C.c_int, [C.c_void_p, C.POINTER(hr_verify_info)]),
    ('hr_model_set_occupancy', C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_void_p]),
    ('hr_render', C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ('hr_render_frame', C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]),
    ('hr_render_fields', C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(hr_fields), C.c_void_p]),
    ('hr_render_maps', C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(hr_maps), C.c_void_p]),
    ('hr_render_frame_maps', C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.POINTER(hr_maps), C.c_void_p]),
    ('hr_allgather_tiles', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    ('hr_shard_range', C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ('hr_generate_rays', C.c_int, [C.POINTER(hr_camera), C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    ('hr_generate_rays_ndc', C.c_int, [C.POINTER(hr_camera), C.POINTER(hr_ndc), C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    ('hr_generate_rays_fisheye', C.c_int, [C.POINTER(hr_camera), C.POINTER(hr_fisheye), C.POINTER(hr_ndc), C.c_int32, C.c_int64, C.c_int64, C.c_void_p,
                                           C.c_void_p]),
    ('hr_generate_rays_lightfield', C.c_int, [C.POINTER(hr_lightfield), C.c_float, C.c_float, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    ('hr_generate_rays_epi', C.c_int, [C.POINTER(hr_lightfield), C.c_float, C.c_float, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    ('hr_rayset_create', C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(hr_ndc), C.POINTER(C.c_void_p)]),
    ('hr_rayset_destroy', None, [C.c_void_p]),
    ('hr_rayset_set_image', C.c_int, [C.c_void_p, C.c_int32, C.POINTER(hr_camera), C.c_int32, C.c_int32, C.c_void_p]),
    ('hr_rayset_set_image_fisheye', C.c_int, [C.c_void_p, C.c_int32, C.POINTER(hr_camera), C.POINTER(hr_fisheye), C.c_int32, C.c_int32, C.c_void_p]),
    ('hr_rayset_create_lightfield', C.c_int, [C.c_int32, C.POINTER(hr_lightfield), C.POINTER(C.c_void_p)]),
    ('hr_rayset_set_view', C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_void_p]),
    ('hr_rayset_size', C.c_int64, [C.c_void_p]),
    ('hr_rayset_batch', C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    ('hr_rayset_order', C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    ('hr_rayset_sample', C.c_int, [C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    ('hr_rayset_set_image_importance', C.c_int, [C.c_void_p, C.c_int32, C.POINTER(hr_camera), C.POINTER(hr_fisheye), C.c_int32, C.c_int64, C.c_float,
                                                 C.c_void_p]),
    ('hr_rayset_image_pixels', C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    ('hr_rayset_image_info', C.c_int, [C.c_void_p, C.c_int32, C.POINTER(hr_rayset_image_info)]),
    ('hr_resize_plan_create', C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    ('hr_image_resize', C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    ('hr_resize_plan_destroy', None, [C.c_void_p]),
    ('hr_resize_plan_create_rgba', C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    ('hr_png_bound', C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    ('hr_png_encoder_create', C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    ('hr_png_encode', C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ('hr_png_encoder_destroy', None, [C.c_void_p]),
    ('hr_jpeg_bound', C.c_int, [C.c_int32] * 5 + [C.POINTER(C.c_int64)]),
    ('hr_jpeg_encoder_create', C.c_int, [C.c_int32] * 6 + [C.POINTER(C.c_void_p)]),
    ('hr_jpeg_encode', C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ('hr_jpeg_encoder_destroy', None, [C.c_void_p]),
    ('hr_png_probe', C.c_int, [C.c_void_p, C.c_int64, C.POINTER(hr_png_info)]),
    ('hr_png_decoder_create', C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_void_p)]),
    ('hr_png_decode', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('hr_png_decoder_destroy', None, [C.c_void_p]),
    ('hr_jpeg_probe', C.c_int, [C.c_void_p, C.c_int64, C.POINTER(hr_jpeg_info)]),
    ('hr_jpeg_decoder_create', C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]),
    ('hr_jpeg_decode', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('hr_jpeg_decoder_destroy', None, [C.c_void_p]),
    ('hr_rayset_set_pixel_format', C.c_int, [C.c_void_p, C.c_int32]),
    ('hr_upsample_plane', C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    ('hr_train_features', C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ('hr_train_rows_forward', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ('hr_train_rows_backward', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('hr_train_forward', C.c_int, [C.c_void_p, C.POINTER(hr_train_tensors), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                   C.c_void_p]),
    ('hr_train_forward_fields', C.c_int, [C.c_void_p, C.POINTER(hr_train_tensors), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                          C.POINTER(hr_fields), C.c_void_p]),
    ('hr_train_backward', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                    C.POINTER(hr_train_tensors), C.c_void_p]),
    ('hr_dense_alpha', C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_float, C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                 C.c_void_p, C.c_void_p]),
    ('hr_pack_display', C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    ('hr_image_metrics_workspace', C.c_size_t, [C.c_int32, C.c_int32]),
    ('hr_image_metrics', C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('hr_lpips_create', C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    ('hr_lpips_destroy', None, [C.c_void_p]),
    ('hr_lpips_workspace', C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    ('hr_lpips', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('hr_image_loss_workspace', C.c_size_t, [C.c_int64]),
    ('hr_image_loss', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p]),
    ('hr_plane_reg_forward', C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    ('hr_plane_reg_backward', C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('hr_train_background_coin', C.c_int32, [C.c_uint64, C.c_uint64]),
    ('hr_train_set_background', C.c_int, [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p]),
    ('hr_reg_plan_create', C.c_int, [C.POINTER(hr_reg_tensor), C.c_int32, C.POINTER(C.c_void_p)]),
    ('hr_reg_plan_update', C.c_int, [C.c_void_p, C.POINTER(hr_reg_tensor), C.c_int32]),
    ('hr_tensorf_reg', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    ('hr_reg_plan_destroy', None, [C.c_void_p]),
    ('hr_adam_step', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    ('hr_adam_step_dev', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_int32, C.c_void_p]),
    ('hr_mlp_train_forward', C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p, C.c_int64, C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]),
    ('hr_linear_workspace', C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    ('hr_linear_forward', C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p,
                                    C.c_int64, C.c_void_p]),
    ('hr_linear_backward', C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int32,
                                     C.c_int32, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('hr_stage_mlp', C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    ('hr_stage_samples', C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ('hr_model_set_shading_mlp', C.c_int, [C.c_void_p, C.POINTER(hr_shading_mlp)]),
    ('hr_model_set_time_decode', C.c_int, [C.c_void_p, C.POINTER(hr_time_decode)]),
    ('hr_stage_shade', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ('hr_debug_trace_mlp', C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ('hr_model_device_bytes', C.c_int64, [C.c_void_p]),
    ('hr_model_destroy', None, [C.c_void_p]),
]

_lib = None


class HipLibraryError(RuntimeError):
    pass


def load():
    """Loads (once) and returns the ctypes handle.  Raises HipLibraryError when the
    in-tree library has not been built (`python -m hyperreel_amd.build`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f'{LIB_PATH} is missing: build it with `python -m hyperreel_amd.build` '
            '(hipcc --offload-arch=gfx950).  hyperreel_amd has no CPU or PyTorch fallback.')
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:
        raise HipLibraryError(f'cannot load {LIB_PATH}: {e}') from e
    for name, res, args in SYMBOLS:
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipLibraryError(f'{LIB_PATH} does not export {name}') from e
        fn.restype = res
        fn.argtypes = args
    v = lib.hr_abi_version()
    if v != ABI_VERSION:
        raise HipLibraryError(f'ABI version mismatch: library {v}, binding {ABI_VERSION}')
    if lib.hr_sizeof_config() != C.sizeof(hr_config):
        raise HipLibraryError('hr_config layout differs between the library and plan.py')
    _lib = lib
    return lib


class HipRangeError(RuntimeError):
    """HR_E_RANGE: a forced fp16 MLP arithmetic does not fit the model's activation range."""


def check(rc, what):
    if rc != 0:
        msg = load().hr_last_error()
        cls = HipRangeError if rc == HR_E_RANGE else RuntimeError
        raise cls(f'{what} failed (code {rc}): {msg.decode() if msg else "?"}')


# symbols whose C int is the answer, not a status (c_int32 IS c_int here, so restype alone cannot tell hr_train_background_coin's 1 from an error)
VALUE_RETURNS = frozenset(('hr_abi_version', 'hr_sizeof_config', 'hr_train_background_coin'))


def stream(device):
    """The stream argument of the C ABI's calls: torch's current stream on `device`."""
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def call(name, *args, device=None):
    """The one way the package calls the library: symbol `name` of load() with `args`, under torch.cuda.device(device) when one is given.
    An argument with a data_ptr (a tensor) travels as that pointer -- NULL for None and for an empty tensor; it is neither copied, cast
    nor checked for strides (row-strided views and outputs pass through here), so callers hand in what the ABI documents.  A status
    return is checked as check() does and nothing is returned; a symbol that returns a value returns it."""
    fn = getattr(_lib or load(), name)
    args = [(a.data_ptr() if a.numel() else None) if hasattr(a, 'data_ptr') else a for a in args]
    if device is None:
        rc = fn(*args)
    else:
        import torch
        with torch.cuda.device(device):
            rc = fn(*args)
    if fn.restype is not C.c_int or name in VALUE_RETURNS:
        return rc
    if rc != 0:
        check(rc, name)
