"""Shared by tests/test_png_host.py and tests/test_gpu_png.py: the host encoder of hyperreel_amd/csrc/hr_png.h (the product's build,
hyperreel_amd.png.host_lib), probes into the header's parts (tests/host_math/hr_png_host.cpp), seeded test images, the shapes at which
the encoder can go wrong, and a PNG chunk reader."""
import ctypes as C
import os
import struct
import zlib

import numpy as np

from helpers import build_host_lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'host_math', 'hr_png_host.cpp')
OUT = os.path.join(HERE, 'host_math', '_build', 'libhr_png_host.so')
CSRC = os.path.join(HERE, '..', 'hyperreel_amd', 'csrc')
DEPS = [SRC, os.path.join(CSRC, 'hr_png.h'), os.path.join(CSRC, 'hr_math.h'), os.path.join(HERE, '..', 'include', 'hyperreel_hip.h')]

U8, F32 = 0, 1
ADAPTIVE = 5
FILTER_MODES = [ADAPTIVE, 0, 1, 2, 3, 4]
CHANNELS = [1, 3, 4]
CONTENTS = ['noise', 'ramp', 'white', 'black', 'disc']
TOK_COVERED, TOK_MATCH = 0xFFFF, 256

_cache = {}


def host_lib():
    if 'lib' not in _cache:
        build_host_lib(OUT, SRC, DEPS)
        lib = C.CDLL(OUT)
        lib.hp_plan.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        lib.hp_plan.restype = None
        lib.hp_crc0.argtypes = [C.c_void_p, C.c_uint64]
        lib.hp_crc0.restype = C.c_uint32
        lib.hp_crc_shift.argtypes = [C.c_uint32, C.c_uint64]
        lib.hp_crc_shift.restype = C.c_uint32
        lib.hp_crc_final.argtypes = [C.c_uint32, C.c_uint64]
        lib.hp_crc_final.restype = C.c_uint32
        lib.hp_adler_part.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.hp_adler_part.restype = None
        lib.hp_adler_combine.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.hp_adler_combine.restype = None
        lib.hp_adler_final.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
        lib.hp_adler_final.restype = C.c_uint32
        lib.hp_code_lengths.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        lib.hp_code_lengths.restype = None
        lib.hp_to8b.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        lib.hp_to8b.restype = None
        lib.hp_tokens_sliced.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p]
        lib.hp_tokens_sliced.restype = None
        lib.hp_token.argtypes = [C.c_int32, C.c_uint32, C.c_uint32]
        lib.hp_token.restype = C.c_uint32
        _cache['lib'] = lib
    return _cache['lib']


def plan(w, h, c):
    """hr_png_plan: the strip edges and the bound come from here, nowhere else"""
    out = np.zeros(8, np.int64)
    host_lib().hp_plan(w, h, c, out.ctypes.data_as(C.c_void_p))
    return dict(zip(('rows_per_strip', 'n_strips', 'workspace_bytes', 'bound', 'row_bytes', 'strip_stride', 'strip_budget'), (int(v) for v in out)))


def bound(w, h, c):
    return plan(w, h, c)['bound']


def encode_host(frame, channels, filter_mode=ADAPTIVE, details=False):
    """hr_png_encode_host (the product's host build: hyperreel_amd.png.host_lib) of an (h, w, c) uint8 or float32 array (or (h, w) with channels 1): the file's bytes, and with `details` the
    filtered bytes (h, 1 + w c), the tokens (as many uint16) and the rows' filter types"""
    frame = np.ascontiguousarray(frame)
    assert frame.dtype in (np.uint8, np.float32)
    h, w = frame.shape[:2]
    assert frame.size == h * w * channels
    p = plan(w, h, channels)
    file = np.full(p['bound'], 0xA5, np.uint8)
    filt = np.zeros((h, p['row_bytes']), np.uint8)
    tok = np.zeros(h * p['row_bytes'], np.uint16)
    rows = np.zeros(h, np.uint8)
    from hyperreel_amd import png
    n = png.host_lib().hr_png_host_encode(frame.ctypes.data_as(C.c_void_p), U8 if frame.dtype == np.uint8 else F32, filter_mode, w, h, channels,
                             file.ctypes.data_as(C.c_void_p), file.size, filt.ctypes.data_as(C.c_void_p), tok.ctypes.data_as(C.c_void_p),
                             rows.ctypes.data_as(C.c_void_p))
    assert 0 < n <= file.size
    assert (file[n:] == 0xA5).all(), 'the host encoder wrote past the length it reports'
    data = file[:n].tobytes()
    return (data, filt, tok, rows) if details else data


def to8b_host(x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty(x.shape, np.uint8)
    host_lib().hp_to8b(x.ctypes.data_as(C.c_void_p), x.size, out.ctypes.data_as(C.c_void_p))
    return out


def to8b_reference(x):
    """utils/__init__.py's to8b: (255 * np.clip(x, 0, 1)).astype(np.uint8), on float32"""
    return (np.float32(255) * np.clip(np.asarray(x, np.float32), np.float32(0), np.float32(1))).astype(np.uint8)


# ---- images ---------------------------------------------------------------------------------------------------------------------------
def image(content, w, h, c, seed=0):
    """(h, w, c) uint8, read-only"""
    key = ('image', content, w, h, c, seed)
    if key not in _cache:
        rng = np.random.default_rng(1000 * seed + 7 * w + 13 * h + c)
        yy, xx = np.mgrid[0:h, 0:w]
        if content == 'noise':
            im = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        elif content == 'ramp':
            im = ((xx[..., None] * 2 + yy[..., None] * 3 + np.arange(c) * 40) & 255).astype(np.uint8)
        elif content == 'white':
            im = np.full((h, w, c), 255, np.uint8)
        elif content == 'black':
            im = np.zeros((h, w, c), np.uint8)
        elif content == 'disc':        # white background around a textured disc
            inside = ((xx - w / 2) ** 2 + (yy - h / 2) ** 2) < (min(w, h) * 0.35) ** 2
            tex = (128 + 60 * np.sin(xx[..., None] * 0.31 + np.arange(c)) + 50 * np.cos(yy[..., None] * 0.17)
                   + rng.integers(-6, 7, (h, w, c))).clip(0, 255).astype(np.uint8)
            im = np.where(inside[..., None], tex, np.uint8(255)).astype(np.uint8)
        else:
            raise ValueError(content)
        im = np.ascontiguousarray(im)
        im.setflags(write=False)
        _cache[key] = im
    return _cache[key]


def as_float(im):
    """floats whose to8b is `im` exactly: k / 255 rounds so that 255 * (k / 255) >= k for some k and < k for others, so use the midpoint"""
    return ((im.astype(np.float32) + np.float32(0.5)) / np.float32(255)).astype(np.float32)


def strip_width(c):
    """width of the strip-edge shapes: rows of 301 / 901 / 1201 bytes -- odd, no multiple of the slices the kernels cut, and long enough
    that a constant colour image's file follows from the run rule to be below 1 % of the raw bytes (tests/test_png_host.py)"""
    return 300


def shapes(c):
    """(w, h): the small shapes, every strip edge of a 300-wide image (from hr_png_plan), and one row wider than the strip budget"""
    rps = plan(strip_width(c), 1, c)['rows_per_strip']
    wide = plan(1, 1, c)['strip_budget'] // c + 5          # 1 + wide * c bytes: beyond the budget, so one row a strip, tokenised in slices
    w = strip_width(c)
    return [(1, 1), (1, 7), (7, 1), (61, 47), (64, 64), (w, rps - 1), (w, rps), (w, rps + 1), (w, 2 * rps + 1), (wide, 2)]


# ---- reading a PNG back ---------------------------------------------------------------------------------------------------------------
def chunks(data):
    """[(type, payload)] of a PNG file; asserts the signature, every length and every CRC, and that nothing follows IEND"""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    out, at = [], 8
    while at < len(data):
        n, = struct.unpack('>I', data[at:at + 4])
        typ = data[at + 4:at + 8]
        payload = data[at + 8:at + 8 + n]
        assert len(payload) == n
        crc, = struct.unpack('>I', data[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(typ + payload), f'CRC of chunk {typ} at {at}'
        out.append((typ, payload))
        at += 12 + n
        if typ == b'IEND':
            break
    assert at == len(data), 'bytes after IEND'
    assert out[0][0] == b'IHDR' and out[-1][0] == b'IEND'
    return out


def idat(data):
    return b''.join(p for t, p in chunks(data) if t == b'IDAT')


def decode(data):
    """PIL's pixels as (h, w, c) uint8 and its mode"""
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    a = np.asarray(im)
    return (a[..., None] if a.ndim == 2 else a), im.mode


def np_tokens(b):
    """The run rule restated: a byte is a literal; the L equal bytes after it, when L >= 3, become distance-1 matches cut greedily into
    258s; a remainder of 1 or 2 is literals"""
    out, i, n = [], 0, len(b)
    while i < n:
        j = i + 1
        while j < n and b[j] == b[i]:
            j += 1
        out.append(int(b[i]))
        left = j - i - 1
        if left < 3:
            out += [int(b[i])] * left
        while left >= 3:
            take = min(left, 258)
            out += [TOK_MATCH + take - 3] + [TOK_COVERED] * (take - 1)
            left -= take
            if left < 3:
                out += [int(b[i])] * left
        i = j
    return np.array(out, np.uint16)


def np_filters(im):
    """(5, h, 1 + w c): every PNG filter of an (h, w, c) uint8 image, in int arithmetic"""
    h, w, c = im.shape
    raw = im.reshape(h, w * c).astype(np.int32)
    a = np.zeros_like(raw); a[:, c:] = raw[:, :-c] if w > 1 else 0
    b = np.zeros_like(raw); b[1:] = raw[:-1]
    cc = np.zeros_like(raw); cc[1:, c:] = raw[:-1, :-c] if w > 1 else 0
    p = a + b - cc
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - cc)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, cc))
    preds = [np.zeros_like(raw), a, b, (a + b) >> 1, paeth]
    out = np.zeros((5, h, 1 + w * c), np.uint8)
    for f, pr in enumerate(preds):
        out[f, :, 0] = f
        out[f, :, 1:] = ((raw - pr) & 255).astype(np.uint8)
    return out


def np_choose(filters):
    """adaptive choice per row: the smallest sum of min(v, 256 - v) over the row's bytes (the type byte apart), the lowest index on a tie"""
    v = filters[:, :, 1:].astype(np.int64)
    cost = np.minimum(v, 256 - v).sum(-1)          # (5, h)
    return np.argmin(cost, axis=0).astype(np.uint8)
