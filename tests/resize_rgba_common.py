"""Shared by tests/test_resize_rgba_host.py, tests/test_gpu_resize_rgba.py and tests/test_gpu_rayset_rgba.py: the RGBA resize fixtures
(tests/golden/resize_rgba/*.npz, written by tools/make_resize_rgba_golden.py from PIL's own Image.resize on RGBA images), the host build
of the RGBA part of hyperreel_amd/csrc/hr_resize.h, numpy statements of PIL's two conversions and the all-pairs image.

A fixture is one shape and one filter: `expected` (3, h2, w2, 4) is what PIL made of the three inputs of `inputs(...)` -- random bytes,
random 0 / 255 in all four channels, random colours under a 0 / 255 alpha checkerboard -- whose crc32 it keeps (`src_crc32`), with
`src_wh`, `dst_wh`, `filter`, `seed`, `pil_version` and `reach` = how many resampled premultiplied values took each branch of the
un-premultiply that is not the plain quotient: [0 < a' < 255 and c' > a' (the clamp), a' == 0 and c' > 0 (copied, not zeroed)].
`twostep_*` fixtures went through get_rgb's two calls, each a full RGBA resize: `filter` to `mid_wh`, BOX to `dst_wh`."""
import ctypes as C
import os

import numpy as np

import resize_common as RC
from helpers import build_host_lib

HERE = RC.HERE
GOLDEN = os.path.join(HERE, 'golden', 'resize_rgba')
SRC = os.path.join(HERE, 'host_math', 'hr_resize_rgba_host.cpp')
OUT = os.path.join(HERE, 'host_math', '_build', 'libhr_resize_rgba_host.so')

FILTERS = RC.FILTERS
KINDS = ['random', 'binary', 'alpha_checkerboard']

# resize_common's shapes (what each is for is said there), and: the enlargement whose 0 / 255 content reaches both rare branches of the
# un-premultiply most often; one axis alone, where both conversions run around a single pass; a single pixel kept a single pixel
SHAPES = RC.SHAPES + [
    ((17, 9), (40, 21)),
    ((37, 23), (16, 23)),        # the horizontal pass alone: premultiplied in its staging, un-premultiplied in its store
    ((37, 23), (37, 9)),         # the vertical pass alone: the alpha comes from a neighbouring lane
    ((1, 1), (1, 1)),
]
TWOSTEP = [((264, 200), (66, 50), (33, 25), 'lanczos'), ((65, 47), (32, 23), (16, 12), 'bicubic')]
CASES = [(s, d, f) for s, d in SHAPES for f in FILTERS]

_cache = {}

case_name = RC.case_name
twostep_name = RC.twostep_name
wh = RC.wh
crc = RC.crc


def seed_of(src_wh, dst_wh):
    return RC.seed_of(src_wh, dst_wh) ^ 0x52474241            # 'RGBA': not the RGB fixtures' bytes with a channel more


def inputs(src_wh, seed):
    """(3, h, w, 4) uint8: KINDS in order, a fixed integer hash of (seed, kind, byte index)"""
    key = ('inputs', tuple(src_wh), seed)
    if key not in _cache:
        w, h = src_wh
        idx = np.arange(h * w * 4, dtype=np.uint64)
        out = np.empty((3, h, w, 4), np.uint8)
        for kind in range(3):
            z = RC._mix(idx + np.uint64(((seed * 3 + kind + 1) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF))
            v = ((z >> np.uint64(63)).astype(np.uint8) * np.uint8(255)) if kind == 1 else (z >> np.uint64(56)).astype(np.uint8)
            out[kind] = v.reshape(h, w, 4)
        yy, xx = np.mgrid[0:h, 0:w]
        out[2, :, :, 3] = (((xx + yy) & 1) * 255).astype(np.uint8)
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


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


def all_pairs():
    """(256, 256, 4): pixel (y, x) = (y, 255 - y, 7 y mod 256, x) -- every (colour byte, alpha) pair in each colour channel"""
    y, x = np.mgrid[0:256, 0:256]
    return np.ascontiguousarray(np.stack([y, 255 - y, (7 * y) % 256, x], -1).astype(np.uint8))


# ---- PIL's conversions in numpy (libImaging/Convert.c: rgbA2rgba, rgba2rgbA) ----------------------------------------------------------
def np_premultiply(rgba):
    x = np.asarray(rgba).astype(np.uint32)
    t = x[..., :3] * x[..., 3:] + 128
    out = np.array(rgba, np.uint8)
    out[..., :3] = (((t >> 8) + t) >> 8).astype(np.uint8)
    return out


def np_unpremultiply(rgba):
    x = np.asarray(rgba).astype(np.uint32)
    c, a = x[..., :3], x[..., 3:]
    q = np.minimum(255, (255 * c) // np.maximum(a, 1))
    out = np.array(rgba, np.uint8)
    out[..., :3] = np.where((a == 0) | (a == 255), c, q).astype(np.uint8)
    return out


def np_resize(images, dst_wh, filt):
    """(..., h, w, 4) RGBA -> (..., h2, w2, 4): resize_common's numpy statement of the 8-bit resize between the two conversions"""
    images = np.asarray(images)
    if (images.shape[-2], images.shape[-3]) == tuple(dst_wh):
        return np.array(images)
    return np_unpremultiply(RC.np_resize(np_premultiply(images), dst_wh, filt))


def reach(premultiplied):
    """[values with 0 < a' < 255 and c' > a', values with a' == 0 and c' > 0] of resampled premultiplied pixels (..., 4)"""
    p = np.asarray(premultiplied).astype(np.int32)
    c, a = p[..., :3], p[..., 3:]
    return np.array([int(((a > 0) & (a < 255) & (c > a)).sum()), int(((a == 0) & (c > 0)).sum())], np.int64)


def pil_resize(images, dst_wh, filt):
    """live PIL on each image of (n, h, w, 4)"""
    from PIL import Image
    number = {'lanczos': Image.LANCZOS, 'bilinear': Image.BILINEAR, 'bicubic': Image.BICUBIC, 'box': Image.BOX}[filt]
    return np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(im), 'RGBA').resize(tuple(dst_wh), number)) for im in images])


# ---- the header, compiled for the host ------------------------------------------------------------------------------------------------
def host_lib():
    if 'lib' not in _cache:
        build_host_lib(OUT, SRC, [SRC, RC.HEADER])
        lib = C.CDLL(OUT)
        lib.hrz4_premultiply_table.argtypes = lib.hrz4_unpremultiply_table.argtypes = [C.c_void_p]
        lib.hrz4_premultiply_table.restype = lib.hrz4_unpremultiply_table.restype = None
        lib.hrz4_premultiply_pixels.argtypes = [C.c_void_p, C.c_int64]
        lib.hrz4_premultiply_pixels.restype = None
        lib.hrz4_axis_plan.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p]
        lib.hrz4_axis_plan.restype = None
        lib.hrz4_resize.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        lib.hrz4_resize.restype = C.c_int32
        _cache['lib'] = lib
    return _cache['lib']


def host_tables():
    """hr_premultiply and hr_unpremultiply on every pair: two (256, 256) uint8 tables [c][a]"""
    pre, un = np.empty((256, 256), np.uint8), np.empty((256, 256), np.uint8)
    host_lib().hrz4_premultiply_table(pre.ctypes.data_as(C.c_void_p))
    host_lib().hrz4_unpremultiply_table(un.ctypes.data_as(C.c_void_p))
    return pre, un


def host_axis_plan(vertical, bounds, ksize, bpp):
    bounds = np.ascontiguousarray(bounds, np.int32)
    out = np.zeros(5, np.int32)
    host_lib().hrz4_axis_plan(int(vertical), bounds.ctypes.data_as(C.c_void_p), bounds.shape[0], ksize, bpp, out.ctypes.data_as(C.c_void_p))
    return dict(zip(('staged', 'tile', 'span', 'row_pitch', 'lds_bytes'), (int(v) for v in out)))


def host_resize(images, dst_wh, filt, want_premultiplied=False):
    """the header's RGBA resize on the host: (n, h, w, 4) uint8 -> (n, h2, w2, 4) [, the resampled bytes before the un-premultiply]"""
    images = np.ascontiguousarray(images, np.uint8)
    n, h, w, ch = images.shape
    assert ch == 4
    out = np.empty((n, dst_wh[1], dst_wh[0], 4), np.uint8)
    pre = np.empty_like(out) if want_premultiplied else None
    rc = host_lib().hrz4_resize(images.ctypes.data_as(C.c_void_p), n, w, h, dst_wh[0], dst_wh[1], RC.FILTER_NUMBER[filt], out.ctypes.data_as(C.c_void_p),
                                pre.ctypes.data_as(C.c_void_p) if want_premultiplied else None)
    assert rc == 0
    return (out, pre) if want_premultiplied else out
