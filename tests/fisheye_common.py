"""Shared by tests/test_fisheye_host.py and tests/test_gpu_fisheye.py: the fisheye cases, the float64 oracle of what
ImmersiveDataset.get_coords computes for a distorted camera (datasets/immersive.py:514-564), the host build of the fisheye part of
hyperreel_amd/csrc/hr_camera.h, and the tolerance both suites hold ray coordinates to.

No fixture comes from OpenCV (cv2 is not a dependency of this repository; tools/make_fisheye_golden.py writes the same cases from
cv2.fisheye.undistortPoints where it is installed).  The contract is the mathematical inverse of the equidistant model
theta_d = theta (1 + k1 theta^2 + k2 theta^4), so the oracle is `rays(case, pair, ndc, np.float64)`: Newton run until theta, pushed back
through the polynomial, returns theta_d to 1e-15 relative -- asserted here, on every call.  The oracle restates the library's contract, which includes its
convention that an all-zero pair means "no distortion given": step 2 is skipped for (0, 0) exactly as for None, so that case holds the
library to the float64 pinhole rays (include/hyperreel_hip.h; OpenCV would treat zeros as the lens theta_d = theta).

The tolerance is not a constant of these files.  As for the NDC rays (tests/camera_common.py): per column group (origins,
directions), the bar is 4 x the largest distance between `rays(..., np.float32)` -- the same steps in numpy float32, np.tan and all --
and the float64 oracle over all cases, and never looser than 1e-5 absolute.  Nothing of the code under test enters it."""
import ctypes as C
import os

import numpy as np

from helpers import build_host_lib
from hyperreel_amd.plan import hr_camera, hr_fisheye, hr_ndc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'host_math', 'hr_fisheye_host.cpp')
OUT = os.path.join(HERE, 'host_math', '_build', 'libhr_fisheye_host.so')
CAP = 1e-5

PAIRS = [(0.0, 0.0), (0.03, 0.004), (-0.05, 0.01), (0.2, -0.02)]
# pairs whose model turns back before pi / 2: the library refuses them
NOT_INVERTIBLE = [(-0.2, 0.0), (-0.5, 0.1), (0.0, -0.04), (-0.14, 0.0), (float('nan'), 0.0), (0.0, float('inf'))]
NDC = dict(fx=20.0, fy=19.0, near=0.5, width=24, height=14)


def _pose(ry, rx, t):
    cy, sy, cx, sx = np.cos(ry), np.sin(ry), np.cos(rx), np.sin(rx)
    R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return np.concatenate([R, np.asarray(t, np.float64)[:, None]], 1).astype(np.float32)


def _K(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


# name -> (W, H, K, pose).  centred: 24 x 14, more than one wavefront, no multiple of it.  one_pixel: 1 x 1 with the pixel's centre
# exactly on the principal point (theta_d = 0: the unchanged branch).  off_centre: 33 x 7, the principal point far from the middle and
# exactly on pixel (10, 2)'s centre.  short_focal: the corner's theta_d is 1.2.
CASES = {
    'centred': (24, 14, _K(20.0, 19.0, 12.0, 7.0), _pose(0.1, -0.05, (0.2, -0.1, 0.3))),
    'one_pixel': (1, 1, _K(1.5, 1.5, 0.5, 0.5), _pose(-0.3, 0.2, (0.0, 0.5, -0.25))),
    'off_centre': (33, 7, _K(25.0, 22.0, 10.5, 2.5), _pose(-0.07, 0.12, (-0.4, 0.05, 0.1))),
    'short_focal': (24, 14, _K(11.0, 11.0, 12.0, 7.0), _pose(0.04, 0.03, (0.1, 0.2, 0.15))),
}


def corner_theta_d(name):
    W, H, K, _ = CASES[name]
    x = np.array([0, W - 1], np.float64)[:, None]
    y = np.array([0, H - 1], np.float64)[None, :]
    return float(np.sqrt(((x - K[0, 2] + 0.5) / K[0, 0]) ** 2 + ((y - K[1, 2] + 0.5) / K[1, 1]) ** 2).max())


def invertible(k1, k2):
    """1 + 3 k1 t^2 + 5 k2 t^4 > 0 on [0, pi / 2], on a fine grid (the library decides it in closed form)."""
    if not (np.isfinite(k1) and np.isfinite(k2)):
        return False
    t = np.linspace(0.0, np.pi / 2, 200001)
    return bool((1 + 3 * k1 * t ** 2 + 5 * k2 * t ** 4).min() > 0)


def solve_theta(k1, k2, theta_d, dtype):
    """Newton on theta (1 + k1 theta^2 + k2 theta^4) = theta_d from theta = theta_d, in `dtype`.  float64: to convergence, checked by
    pushing theta back through the polynomial; float32: 20 steps, well past where the iterate only walks its rounding cycle."""
    k1, k2 = dtype(k1), dtype(k2)
    th = theta_d.astype(dtype)
    for _ in range(60 if dtype is np.float64 else 20):
        t2 = th * th
        th = th - (th * (1 + k1 * t2 + k2 * t2 * t2) - theta_d) / (1 + 3 * k1 * t2 + 5 * k2 * t2 * t2)
    if dtype is np.float64:
        back = th * (1 + k1 * th ** 2 + k2 * th ** 4)
        assert (np.abs(back - theta_d) <= 1e-15 * theta_d).all(), float(np.abs(back / np.maximum(theta_d, 1e-300) - 1).max())
    return th


def undistort(k1, k2, dx, dy, dtype):
    theta_d = np.sqrt(dx * dx + dy * dy)
    theta = solve_theta(k1, k2, theta_d, dtype)
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.where(theta_d <= 1e-8, dtype(1), np.tan(theta) / theta_d).astype(dtype)
    return s * dx, s * dy


def _normalize(v):
    return v / np.maximum(np.sqrt((v * v).sum(-1, keepdims=True)), 1e-12).astype(v.dtype)


def rays(name, pair, ndc, dtype, pixels=None):
    """Steps 1-5 for every pixel of the case's image in row-major order (or the (n, 2) integer `pixels`), in `dtype`: (n, 6).  The
    pixel direction is formed in float32 either way, as the reference forms it before it calls OpenCV; pair None or (0, 0): no
    distortion given, no undistortion (the pinhole rays)."""
    W, H, K, pose = CASES[name]
    if pixels is None:
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        x, y = x.reshape(-1), y.reshape(-1)
    else:
        x, y = np.asarray(pixels)[:, 0], np.asarray(pixels)[:, 1]
    i, j = x.astype(np.float32), y.astype(np.float32)
    dx = ((i - K[0, 2] + np.float32(0.5)) / K[0, 0]).astype(dtype)
    dy = (-(j - K[1, 2] + np.float32(0.5)) / K[1, 1]).astype(dtype)
    if pair is not None and tuple(pair) != (0.0, 0.0):
        dx, dy = undistort(pair[0], pair[1], dx, dy, dtype)
        d = _normalize(np.stack([dx, dy, -np.ones_like(dx)], -1))
    else:
        d = np.stack([dx, dy, -np.ones_like(dx)], -1)
    P = pose.astype(dtype)
    d = _normalize(d @ P[:, :3].T)
    o = np.broadcast_to(P[:, 3], d.shape)
    if ndc is None:
        return np.concatenate([o, d], -1).astype(dtype)
    near = dtype(ndc['near'])
    sx, sy = dtype(-1.0 / (ndc['width'] / (2.0 * ndc['fx']))), dtype(-1.0 / (ndc['height'] / (2.0 * ndc['fy'])))
    t = -(near + o[:, 2]) / d[:, 2]
    o = o + t[:, None] * d
    ox_oz, oy_oz = o[:, 0] / o[:, 2], o[:, 1] / o[:, 2]
    o2 = 1 + 2 * near / o[:, 2]
    out = np.stack([sx * ox_oz, sy * oy_oz, o2, sx * (d[:, 0] / d[:, 2] - ox_oz), sy * (d[:, 1] / d[:, 2] - oy_oz), 1 - o2], -1)
    return out.astype(dtype)


_cache = {}


def oracle(name, pair, ndc):
    """rays(..., np.float64) of a whole image, computed once per case and left unchanged."""
    key = (name, pair, ndc is not None)
    if key not in _cache:
        _cache[key] = rays(name, pair, ndc, np.float64)
        _cache[key].setflags(write=False)
    return _cache[key]


def all_cases():
    return [(name, pair, ndc) for name in CASES for pair in PAIRS for ndc in (None, NDC)]


def reference_distances():
    """{'origins': d, 'directions': d}: the largest |numpy float32 evaluation - float64 oracle| over all cases."""
    if 'dist' not in _cache:
        d = {'origins': 0.0, 'directions': 0.0}
        for name, pair, ndc in all_cases():
            diff = np.abs(rays(name, pair, ndc, np.float32).astype(np.float64) - oracle(name, pair, ndc))
            d['origins'] = max(d['origins'], float(diff[:, :3].max()))
            d['directions'] = max(d['directions'], float(diff[:, 3:].max()))
        _cache['dist'] = d
    return dict(_cache['dist'])


def bars():
    return {k: min(4.0 * v, CAP) for k, v in reference_distances().items()}


def check_coords(got, ref, what):
    """got (n, >= 6) float32, ref (n, 6) float64: prints the distances beside the bars, then asserts."""
    b = bars()
    d_o, d_d = float(np.abs(got[:, :3] - ref[:, :3]).max()), float(np.abs(got[:, 3:6] - ref[:, 3:6]).max())
    print(f'{what}: origins {d_o:.3e} (bar {b["origins"]:.3e}) directions {d_d:.3e} (bar {b["directions"]:.3e})', flush=True)
    assert d_o <= b['origins'] and d_d <= b['directions'], what


def camera_of(name, cam_id=0.0, time=0.0):
    from hyperreel_amd.data import make_camera
    W, H, K, pose = CASES[name]
    return make_camera(pose, K, W, H, cam_id, time)


def host_lib():
    deps = [SRC, os.path.join(HERE, '..', 'hyperreel_amd', 'csrc', 'hr_camera.h'), os.path.join(HERE, '..', 'include', 'hyperreel_hip.h')]
    build_host_lib(OUT, SRC, deps)
    lib = C.CDLL(OUT)
    lib.hf_invertible.argtypes = [C.c_float, C.c_float]
    lib.hf_theta.argtypes = [C.c_float, C.c_float, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    lib.hf_theta.restype = None
    lib.hf_tan.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    lib.hf_tan.restype = None
    lib.hf_undistort.argtypes = [C.c_float, C.c_float, C.c_void_p, C.c_int64, C.c_void_p]
    lib.hf_undistort.restype = None
    lib.hf_pixel_rays.argtypes = [C.POINTER(hr_camera), C.POINTER(hr_fisheye), C.POINTER(hr_ndc), C.c_int64, C.c_int64, C.c_void_p]
    lib.hf_pixel_rays.restype = None
    lib.hf_pinhole_rays.argtypes = [C.POINTER(hr_camera), C.POINTER(hr_ndc), C.c_int64, C.c_int64, C.c_void_p]
    lib.hf_pinhole_rays.restype = None
    lib.hf_subsampled_rays.argtypes = [C.POINTER(hr_camera), C.POINTER(hr_fisheye), C.POINTER(hr_ndc), C.c_int, C.c_int, C.c_void_p]
    lib.hf_subsampled_rays.restype = C.c_int64
    return lib


def host_rays(lib, name, pair, ndc, first=0, n=None):
    """hr_pixel_ray_fisheye compiled for the host: rows [first, first + n) of the case's image, (n, 6) float32; pair None: a NULL
    hr_fisheye."""
    from hyperreel_amd.data import make_fisheye, make_ndc
    W, H = CASES[name][:2]
    n = W * H - first if n is None else n
    cam, fe, nd = camera_of(name), make_fisheye(pair), make_ndc(ndc)
    out = np.full((n, 6), np.nan, np.float32)
    lib.hf_pixel_rays(C.byref(cam), C.byref(fe) if fe is not None else None, C.byref(nd) if nd is not None else None, first, n,
                      out.ctypes.data_as(C.c_void_p))
    return out


# ---- a small training set: 3 images of 24 x 14 from different fisheye cameras under the checkerboard rule
SET_NAMES = ['centred', 'short_focal', 'centred']
SET_PAIRS = [(0.03, 0.004), (0.2, -0.02), (-0.05, 0.01)]
SET_RULES = [(1, 0), (3, 1), (4, 2)]
SET_TIMES = [0.0, 0.5, 1.0]
SET_CAM_IDS = [0.0, 1.0, 2.0]


def set_images():
    return np.random.default_rng(5).integers(0, 256, (3, 14, 24, 3), dtype=np.uint8)


def set_kept(i):
    """(n, 2) the (x, y) of image i's kept pixels, row-major"""
    e, o = SET_RULES[i]
    y, x = np.meshgrid(np.arange(14), np.arange(24), indexing='ij')
    keep = ((x + y + o) % e) == 0
    return np.stack([x[keep], y[keep]], -1)


def set_oracle(ndc):
    """The set's elements in order: coords (n, 6) float64, rgb (n, 3) float32, per-image [lo, hi)"""
    coords, rgb, rows, lo = [], [], [], 0
    img = set_images()
    for i in range(3):
        px = set_kept(i)
        coords.append(rays(SET_NAMES[i], SET_PAIRS[i], ndc, np.float64, pixels=px))
        rgb.append(img[i][px[:, 1], px[:, 0]].astype(np.float32) / np.float32(255.0))
        rows.append((lo, lo + len(px)))
        lo += len(px)
    return np.concatenate(coords, 0), np.concatenate(rgb, 0), rows
