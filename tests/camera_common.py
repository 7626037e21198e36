"""Shared by tests/test_camera_host.py and tests/test_gpu_rays.py: the camera fixtures (tests/golden/camera/*.npz, written by
tools/make_camera_golden.py from the reference's own ray functions), the host build of hyperreel_amd/csrc/hr_camera.h, and the
tolerance both suites hold the NDC rays to.

The tolerance is not a constant of these files.  NDC divides by d_z and o_z; how far one correct float32 evaluation lands from
another is a property of the formulas, so it is measured on the reference: per column group (origins, directions), the bar is
4 x the largest distance between the reference's float32 all_inputs and the float64 evaluation stored beside it, over all
fixtures -- the factor covers a different but equally valid operation order -- and never looser than 1e-5 absolute (NDC
coordinates are O(1); the intersections downstream are held to 1e-4 in RGB)."""
import ctypes as C
import glob
import os

import numpy as np

from helpers import build_host_lib
from hyperreel_amd.plan import hr_camera, hr_ndc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'camera')
SRC = os.path.join(HERE, 'host_math', 'hr_camera_host.cpp')
OUT = os.path.join(HERE, 'host_math', '_build', 'libhr_camera_host.so')
CAP = 1e-5
CASES = ['video_ndc', 'static_pinhole', 'ndc_other_size']


def fixture_names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN, '*.npz')))


def load(name):
    with np.load(os.path.join(GOLDEN, f'{name}.npz')) as z:
        return {k: z[k] for k in z.files}


def reference_distances():
    """{'origins': d, 'directions': d}: the largest |reference float32 - float64| over all fixtures."""
    d = {'origins': 0.0, 'directions': 0.0}
    for name in fixture_names():
        f = load(name)
        diff = np.abs(f['all_inputs'][:, :6].astype(np.float64) - f['coords64'])
        d['origins'] = max(d['origins'], float(diff[:, :3].max()))
        d['directions'] = max(d['directions'], float(diff[:, 3:].max()))
    return d


def bars():
    return {k: min(4.0 * v, CAP) for k, v in reference_distances().items()}


def ray_dim(f):
    return 8 if bool(f['video']) else 6


def ndc_of(f):
    if 'ndc' not in f:
        return None
    fx, fy, near, w, h = [float(v) for v in f['ndc']]
    return dict(fx=fx, fy=fy, near=near, width=int(w), height=int(h))


def ndc_struct(f):
    from hyperreel_amd.data import make_ndc
    return make_ndc(ndc_of(f))


def camera_of(f, i):
    from hyperreel_amd.data import make_camera
    W, H = int(f['img_wh'][0]), int(f['img_wh'][1])
    return make_camera(f['poses'][i], f['intrinsics'][i], W, H, float(f['cam_ids'][i]), float(f['times'][i]))


def image_rows(f):
    """[first row, end row) of every image in all_inputs (counted from the stored rules the brute-force way)"""
    W, H = int(f['img_wh'][0]), int(f['img_wh'][1])
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    counts = [int((((x + y + int(o)) % int(e)) == 0).sum()) for e, o in f['rules']]
    ends = np.cumsum(counts)
    return [(int(e - c), int(e)) for c, e in zip(counts, ends)]


def host_lib():
    deps = [SRC, os.path.join(HERE, '..', 'hyperreel_amd', 'csrc', 'hr_camera.h'), os.path.join(HERE, '..', 'include', 'hyperreel_hip.h')]
    build_host_lib(OUT, SRC, deps)
    lib = C.CDLL(OUT)
    lib.hc_pixel_rays.argtypes = [C.POINTER(hr_camera), C.POINTER(hr_ndc), C.c_int64, C.c_int64, C.c_void_p]
    lib.hc_pixel_rays.restype = None
    lib.hc_subsampled_rays.argtypes = [C.POINTER(hr_camera), C.POINTER(hr_ndc), C.c_int, C.c_int, C.c_void_p]
    lib.hc_subsampled_rays.restype = C.c_int64
    lib.hc_subsample_count.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.hc_subsample_count.restype = C.c_int64
    lib.hc_subsample_pixels.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p]
    lib.hc_subsample_pixels.restype = None
    lib.hc_perm_key.argtypes = [C.c_uint64, C.c_uint64]
    lib.hc_perm_key.restype = C.c_uint64
    lib.hc_perm.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.hc_perm.restype = None
    lib.hc_perm_not_bijective.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
    lib.hc_perm_not_bijective.restype = C.c_int64
    return lib


def host_rays(lib, f):
    """hr_camera.h compiled for the host over a whole fixture: (rays, 6) float32 in all_inputs' order."""
    nd = ndc_struct(f)
    W, H = int(f['img_wh'][0]), int(f['img_wh'][1])
    out = []
    for i, (e, o) in enumerate(f['rules']):
        cam = camera_of(f, i)
        buf = np.empty((W * H, 6), np.float32)
        n = lib.hc_subsampled_rays(C.byref(cam), C.byref(nd) if nd is not None else None, int(e), int(o), buf.ctypes.data_as(C.c_void_p))
        out.append(buf[:n].copy())
    return np.concatenate(out, 0)
