"""Shared by tests/test_importance_host.py and tests/test_gpu_importance.py: the importance fixtures (tests/golden/importance/*.npz,
written by tools/make_importance_golden.py from the reference's own importance_subsample methods), the host build of
hyperreel_amd/csrc/hr_importance.h, a numpy statement of the rule (select + mask + compaction) and the float64 rays the coordinates
are held to.

A fixture holds images in Immersive's load order (video-major), one camera per video, and what the reference made of them: per
image `diff`, `threshold`, `num_take` and the kept pixels (`kept`, rows `kept_rows[i]:kept_rows[i + 1]`), and `all_inputs`.  The
float32 coords the method was handed are `video_coords[video_of[i]]` with the image's time appended."""
import ctypes as C
import os

import numpy as np

import camera_common
import fisheye_common
from helpers import build_host_lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'importance')
SRC = os.path.join(HERE, 'host_math', 'hr_importance_host.cpp')
OUT = os.path.join(HERE, 'host_math', '_build', 'libhr_importance_host.so')
CASES = ['immersive_small', 'static_background', 'neural3d_variant']

_cache = {}


def load(name):
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, f'{name}.npz')) as z:
            _cache[name] = {k: z[k] for k in z.files}
        for v in _cache[name].values():
            v.setflags(write=False)
    return _cache[name]


def host_lib():
    if 'lib' not in _cache:
        build_host_lib(OUT, SRC, [SRC, os.path.join(HERE, '..', 'hyperreel_amd', 'csrc', 'hr_importance.h')])
        lib = C.CDLL(OUT)
        lib.hi_diff.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        lib.hi_diff.restype = None
        lib.hi_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        lib.hi_keys.restype = None
        lib.hi_rank.argtypes = [C.c_int64, C.c_int64]
        lib.hi_rank.restype = C.c_int64
        _cache['lib'] = lib
    return _cache['lib']


def host_diff(cur, prev):
    """hr_importance_diff compiled for the host: cur, prev (..., 3) uint8 -> (n) float32"""
    cur, prev = np.ascontiguousarray(cur, np.uint8).reshape(-1, 3), np.ascontiguousarray(prev, np.uint8).reshape(-1, 3)
    assert cur.shape == prev.shape
    out = np.empty(cur.shape[0], np.float32)
    host_lib().hi_diff(cur.ctypes.data_as(C.c_void_p), prev.ctypes.data_as(C.c_void_p), cur.shape[0], out.ctypes.data_as(C.c_void_p))
    return out


def host_keys(cur, prev):
    cur, prev = np.ascontiguousarray(cur, np.uint8).reshape(-1, 3), np.ascontiguousarray(prev, np.uint8).reshape(-1, 3)
    out = np.empty(cur.shape[0], np.uint32)
    host_lib().hi_keys(cur.ctypes.data_as(C.c_void_p), prev.ctypes.data_as(C.c_void_p), cur.shape[0], out.ctypes.data_as(C.c_void_p))
    return out


def select(diff, num_take, d_z=None, dir_z_below=None):
    """The rule in numpy on float32 diffs: the threshold is the value at ascending rank hi_rank(n, num_take) (diff_sorted[-num_take]); a
    pixel is kept when its diff is strictly greater and, with a limit, its float32 d_z lies below float32(limit); the kept pixels'
    row-major indices ascend.  Returns (threshold float32, kept int32)."""
    diff = np.asarray(diff, np.float32)
    rank = int(host_lib().hi_rank(diff.size, int(num_take)))
    threshold = np.partition(diff, rank)[rank]
    mask = diff > threshold
    if dir_z_below is not None:
        mask &= np.asarray(d_z, np.float32) < np.float32(dir_z_below)
    return np.float32(threshold), np.nonzero(mask)[0].astype(np.int32)


def dir_limit(f):
    v = float(f['dir_z_below'])
    return None if np.isnan(v) else v


def is_fisheye(f):
    return 'distortions' in f


def ndc_of(f):
    return camera_common.ndc_of(f)


def rays64(W, H, K, pose, pair, ndc):
    """fisheye_common's float64 oracle (pair None: the pinhole camera) for a camera of this module: every pixel, (W * H, 6)"""
    key = ('importance_common', id(pose))
    fisheye_common.CASES[key] = (W, H, np.asarray(K, np.float32), np.asarray(pose, np.float32))
    try:
        return fisheye_common.rays(key, pair, ndc, np.float64)
    finally:
        del fisheye_common.CASES[key]


def image_rays64(f, i):
    W, H = int(f['img_wh'][0]), int(f['img_wh'][1])
    key = ('rays64', id(f), int(f['video_of'][i]))
    if key not in _cache:
        pair = tuple(float(v) for v in f['distortions'][i]) if is_fisheye(f) else None
        _cache[key] = rays64(W, H, f['intrinsics'][i], f['poses'][i], pair, ndc_of(f))
    return _cache[key]


def coord_bars(f):
    """the bars of the suite the camera model belongs to: fisheye_common's for a lens, camera_common's for the pinhole camera"""
    return fisheye_common.bars() if is_fisheye(f) else camera_common.bars()


def check_coords(f, got, ref, what):
    b = coord_bars(f)
    d_o = float(np.abs(got[:, :3] - ref[:, :3]).max()) if len(got) else 0.0
    d_d = float(np.abs(got[:, 3:6] - ref[:, 3:6]).max()) if len(got) else 0.0
    print(f'{what}: origins {d_o:.3e} (bar {b["origins"]:.3e}) directions {d_d:.3e} (bar {b["directions"]:.3e})', flush=True)
    assert d_o <= b['origins'] and d_d <= b['directions'], what


def rule_of(f):
    """the fixture's per-image rule through DeviceRaySet.importance_rule"""
    from hyperreel_amd.data import DeviceRaySet
    W, H = int(f['img_wh'][0]), int(f['img_wh'][1])
    full, key, kfrac, frac = int(f['rule'][0]), int(f['rule'][1]), float(f['rule'][2]), float(f['rule'][3])
    return DeviceRaySet.importance_rule(f['frames'], W * H, full, key, kfrac, frac, f['first_of_video'], dir_z_below=dir_limit(f))


def set_of(f):
    from hyperreel_amd.data import DeviceRaySet
    W, H = int(f['img_wh'][0]), int(f['img_wh'][1])
    return DeviceRaySet(np.array(f['images']), f['poses'], f['intrinsics'], f['times'], f['cam_ids'], (W, H), ndc=ndc_of(f), subsample=rule_of(f),
                        distortions=f['distortions'] if is_fisheye(f) else None)


def kept_of(f, i):
    return f['kept'][int(f['kept_rows'][i]):int(f['kept_rows'][i + 1])]
