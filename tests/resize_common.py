"""Shared by tests/test_resize_host.py and tests/test_gpu_resize.py: the resize fixtures (tests/golden/resize/*.npz, written by
tools/make_resize_golden.py from PIL), the host build of hyperreel_amd/csrc/hr_resize.h and a numpy statement of PIL's 8-bit resize.

A fixture is one shape and one filter: `expected` (3, h2, w2, 3) is what PIL's Image.resize made of the three inputs of `inputs(...)` --
random bytes, random 0 / 255 (ringing clamps at both ends) and a checkerboard -- whose crc32 the fixture keeps (`src_crc32`), with
`src_wh`, `dst_wh`, `filter`, `seed` and `pil_version`.  The inputs are a fixed integer hash of (seed, kind, byte index): the files hold
PIL's bytes, not noise that anyone can restate.  `twostep_*` fixtures went through get_rgb's two calls: `filter` to `mid_wh`, BOX to `dst_wh`."""
import ctypes as C
import math
import os
import zlib

import numpy as np

from helpers import build_host_lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'resize')
SRC = os.path.join(HERE, 'host_math', 'hr_resize_host.cpp')
OUT = os.path.join(HERE, 'host_math', '_build', 'libhr_resize_host.so')
HEADER = os.path.join(HERE, '..', 'hyperreel_amd', 'csrc', 'hr_resize.h')

FILTERS = ['lanczos', 'bilinear', 'bicubic', 'box']
FILTER_NUMBER = {'lanczos': 1, 'bilinear': 2, 'bicubic': 3, 'box': 4}          # PIL's Image.Resampling
KINDS = ['random', 'binary', 'checkerboard']

# (w, h) -> (w2, h2): the smallest shapes at which a kernel can still go wrong
SHAPES = [
    ((37, 29), (16, 11)),        # non-integer reduction
    ((16, 11), (37, 29)),        # enlargement: the filter keeps its own scale
    ((65, 47), (32, 23)),
    ((40, 30), (40, 13)),        # the horizontal pass is skipped
    ((40, 30), (17, 30)),        # the vertical pass is skipped
    ((9, 7), (1, 1)),
    ((1, 1), (4, 4)),
    ((5, 5), (64, 3)),
    ((3, 200), (2, 50)),
    ((264, 200), (33, 25)),      # ksize 49 under LANCZOS: the LLFF ratio
    ((100, 3), (7, 3)),          # ksize 87: the horizontal general kernel
    ((3, 100), (3, 7)),          # ... and the vertical one
    ((1030, 40), (515, 20)),     # more than one workgroup along a row
    ((40, 1030), (20, 515)),     # more than one workgroup along a column
    ((257, 9), (256, 9)),
    ((12, 10), (12, 10)),        # same size: a copy
]
TWOSTEP = [((264, 200), (66, 50), (33, 25), 'lanczos')]          # LANCZOS to _img_wh, then BOX to img_wh
# further axes (in, out) whose coefficient tables the host suite compares: LLFF's two, Technicolor's, and one pixel more or less
AXES = [(4032, 504), (3024, 378), (2704, 1352), (1000, 999), (999, 1000)]

_cache = {}


def case_name(src_wh, dst_wh, filt):
    return f'w{src_wh[0]}h{src_wh[1]}_w{dst_wh[0]}h{dst_wh[1]}_{filt}'


def twostep_name(src_wh, mid_wh, dst_wh, filt):
    return f'twostep_w{src_wh[0]}h{src_wh[1]}_w{mid_wh[0]}h{mid_wh[1]}_w{dst_wh[0]}h{dst_wh[1]}_{filt}'


def seed_of(src_wh, dst_wh):
    return (src_wh[0] * 1000003 + src_wh[1] * 10007 + dst_wh[0] * 101 + dst_wh[1]) & 0xFFFFFFFF


def _mix(z):
    """splitmix64's finaliser on uint64 arrays (wrapping arithmetic)"""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def inputs(src_wh, seed):
    """(3, h, w, 3) uint8: KINDS in order"""
    key = ('inputs', tuple(src_wh), seed)
    if key not in _cache:
        w, h = src_wh
        idx = np.arange(h * w * 3, dtype=np.uint64)
        out = np.empty((3, h, w, 3), np.uint8)
        for kind in range(2):
            z = _mix(idx + np.uint64(((seed * 2 + kind + 1) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF))
            v = (z >> np.uint64(56)).astype(np.uint8) if kind == 0 else ((z >> np.uint64(63)).astype(np.uint8) * np.uint8(255))
            out[kind] = v.reshape(h, w, 3)
        yy, xx = np.mgrid[0:h, 0:w]
        out[2] = ((((xx + yy) & 1) * 255).astype(np.uint8))[..., None]
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def crc(images):
    return np.array([zlib.crc32(np.ascontiguousarray(im).tobytes()) for im in images], np.uint32)


def load(name):
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, f'{name}.npz')) as z:
            f = {k: z[k] for k in z.files}
        for v in f.values():
            v.setflags(write=False)
        f['src'] = inputs(tuple(int(v) for v in f['src_wh']), int(f['seed']))
        assert np.array_equal(crc(f['src']), f['src_crc32']), f'{name}: the inputs are not the ones the fixture was made from'
        _cache[name] = f
    return _cache[name]


def wh(f, key):
    return int(f[key][0]), int(f[key][1])


# ---- the header, compiled for the host ------------------------------------------------------------------------------------------------
def host_lib():
    if 'lib' not in _cache:
        build_host_lib(OUT, SRC, [SRC, HEADER])
        lib = C.CDLL(OUT)
        lib.hrz_ksize.argtypes = [C.c_int32, C.c_int32, C.c_int32]
        lib.hrz_ksize.restype = C.c_int64
        lib.hrz_coeffs.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        lib.hrz_coeffs.restype = None
        lib.hrz_check.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
        lib.hrz_check.restype = C.c_int32
        lib.hrz_axis_plan.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]
        lib.hrz_axis_plan.restype = None
        lib.hrz_resize.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        lib.hrz_resize.restype = C.c_int32
        _cache['lib'] = lib
    return _cache['lib']


def host_coeffs(n_in, n_out, filt):
    """hr_resize_coeffs: bounds (out, 2), k (out, ksize), int32"""
    lib = host_lib()
    ksize = int(lib.hrz_ksize(n_in, n_out, FILTER_NUMBER[filt]))
    bounds, k = np.empty((n_out, 2), np.int32), np.empty((n_out, ksize), np.int32)
    lib.hrz_coeffs(n_in, n_out, FILTER_NUMBER[filt], bounds.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p))
    return bounds, k


OVERFLOW, ROWS_OK, FIT_MAD24 = -1, 0, 1


def host_check(k):
    """hr_resize_check of a (rows, ksize) table: (verdict, the first row that fails or -1)"""
    k = np.ascontiguousarray(k, np.int32)
    bad = C.c_int64(-1)
    return int(host_lib().hrz_check(k.ctypes.data_as(C.c_void_p), k.shape[0], k.shape[1], C.byref(bad))), int(bad.value)


def host_axis_plan(vertical, bounds, ksize):
    bounds = np.ascontiguousarray(bounds, np.int32)
    out = np.zeros(5, np.int32)
    host_lib().hrz_axis_plan(int(vertical), bounds.ctypes.data_as(C.c_void_p), bounds.shape[0], ksize, out.ctypes.data_as(C.c_void_p))
    return dict(zip(('staged', 'tile', 'span', 'row_pitch', 'lds_bytes'), (int(v) for v in out)))


def host_resize(images, dst_wh, filt):
    """the header's two passes on the host: (n, h, w, 3) uint8 -> (n, h2, w2, 3)"""
    images = np.ascontiguousarray(images, np.uint8)
    n, h, w, _ = images.shape
    out = np.empty((n, dst_wh[1], dst_wh[0], 3), np.uint8)
    rc = host_lib().hrz_resize(images.ctypes.data_as(C.c_void_p), n, w, h, dst_wh[0], dst_wh[1], FILTER_NUMBER[filt], out.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return out


# ---- PIL's arithmetic in numpy (libImaging/Resample.c), python floats being IEEE doubles ----------------------------------------------
def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


NP_FILTERS = {'box': (_box, 0.5), 'bilinear': (_bilinear, 1.0), 'bicubic': (_bicubic, 2.0), 'lanczos': (_lanczos, 3.0)}


def np_coeffs(n_in, n_out, filt):
    key = ('np_coeffs', n_in, n_out, filt)
    if key in _cache:
        return _cache[key]
    f, support = NP_FILTERS[filt]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    sup = support * fs
    ksize = int(math.ceil(sup)) * 2 + 1
    ss = 1.0 / fs
    bounds, k = np.zeros((n_out, 2), np.int32), np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        c = (xx + 0.5) * scale
        xmin = max(int(c - sup + 0.5), 0)
        n = min(int(c + sup + 0.5), n_in) - xmin
        w = [f((x + xmin - c + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, n)
        k[xx, :n] = [int(v * (1 << 22) + 0.5) if v >= 0 else int(v * (1 << 22) - 0.5) for v in w]
    _cache[key] = (bounds, k)
    return bounds, k


def _np_axis(img, axis, n_out, filt):
    n_in = img.shape[axis]
    if n_in == n_out:
        return img
    bounds, k = np_coeffs(n_in, n_out, filt)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.uint8)
    for xx in range(n_out):
        xmin, n = bounds[xx]
        acc = np.tensordot(k[xx, :n].astype(np.int64), src[xmin:xmin + n], axes=(0, 0)) + (1 << 21)
        assert np.abs(acc).max() < (1 << 31)
        out[xx] = np.clip(acc >> 22, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def np_resize(images, dst_wh, filt):
    """(..., h, w, 3) uint8 -> (..., h2, w2, 3): the horizontal pass into 8 bits, then the vertical"""
    return np.ascontiguousarray(_np_axis(_np_axis(np.asarray(images), -2, dst_wh[0], filt), -3, dst_wh[1], filt))


def pil_resize(images, dst_wh, filt):
    """live PIL on each image of (n, h, w, 3)"""
    from PIL import Image
    number = {'lanczos': Image.LANCZOS, 'bilinear': Image.BILINEAR, 'bicubic': Image.BICUBIC, 'box': Image.BOX}[filt]
    return np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(im), 'RGB').resize(tuple(dst_wh), number)) for im in images])
