"""Shared by tests/test_jpeg_encode_host.py and tests/test_gpu_jpeg_encode.py: the fixtures of tests/golden/jpeg_encode
(tools/make_jpeg_encode_golden.py: seeded inputs and PIL's complete files), seeded images outside them, PIL's file for an array, an int64
numpy statement of the forward DCT, and probes into the header's parts (tests/host_math/hr_jpeg_encode_host.cpp)."""
import ctypes as C
import importlib.util
import os

import numpy as np

from helpers import build_host_lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'jpeg_encode')
SRC = os.path.join(HERE, 'host_math', 'hr_jpeg_encode_host.cpp')
OUT = os.path.join(HERE, 'host_math', '_build', 'libhr_jpeg_encode_host.so')
CSRC = os.path.join(HERE, '..', 'hyperreel_amd', 'csrc')
DEPS = [SRC] + [os.path.join(CSRC, h) for h in ('hr_jpeg_encode.h', 'hr_jpeg_decode.h', 'hr_png_decode.h', 'hr_png.h', 'hr_math.h')] + \
       [os.path.join(HERE, '..', 'include', 'hyperreel_hip.h')]
SUBS = {0: '4:4:4', 1: '4:2:2', 2: '4:2:0'}
_cache = {}


def tool():
    """tools/make_jpeg_encode_golden.py as a module: its shapes, contents and PIL call"""
    if 'tool' not in _cache:
        spec = importlib.util.spec_from_file_location('make_jpeg_encode_golden', os.path.join(HERE, '..', 'tools', 'make_jpeg_encode_golden.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _cache['tool'] = mod
    return _cache['tool']


def host_lib():
    if 'lib' not in _cache:
        build_host_lib(OUT, SRC, DEPS)
        lib = C.CDLL(OUT)
        lib.hje_fdct.argtypes, lib.hje_fdct.restype = [C.c_void_p, C.c_void_p], None
        lib.hje_quant_many.argtypes, lib.hje_quant_many.restype = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p], None
        lib.hje_quant_entry.argtypes, lib.hje_quant_entry.restype = [C.c_int32, C.c_int32], C.c_int32
        lib.hje_max_block_bits.argtypes, lib.hje_max_block_bits.restype = [], C.c_uint32
        lib.hje_plan.argtypes, lib.hje_plan.restype = [C.c_int32] * 5 + [C.c_void_p], None
        _cache['lib'] = lib
    return _cache['lib']


def plan(w, h, channels, subsampling, restart_rows=0):
    """{'n_blocks', 'n_int', 'n_wg', 'head_bytes', 'raw_max', 'bound'} of hr_jpeg_enc_plan"""
    out = np.zeros(6, np.int64)
    host_lib().hje_plan(w, h, channels, subsampling, restart_rows, out.ctypes.data_as(C.c_void_p))
    return dict(zip(('n_blocks', 'n_int', 'n_wg', 'head_bytes', 'raw_max', 'bound'), (int(v) for v in out)))


def golden():
    """[(name, array (h, w, c) uint8 or float32, {'quality', 'subsampling', 'restart_rows'}, PIL's file)] of every archive; loaded once"""
    if 'golden' not in _cache:
        out = []
        t = tool()
        for w, h in t.SMALL + [t.LARGE]:
            z = np.load(os.path.join(GOLDEN, f'w{w}_h{h}.npz'))
            files, off, inputs, ioff = z['files'], z['offsets'], z['inputs'], z['in_offsets']
            for i, name in enumerate(z['names']):
                _, _, c, q, sub, rr, is_float = (int(v) for v in z['meta'][i])
                a = np.frombuffer(inputs[ioff[i]:ioff[i + 1]].tobytes(), np.float32 if is_float else np.uint8).reshape(h, w, c).copy()
                out.append((f'w{w}_h{h}_{name}', a, {'quality': q, 'subsampling': SUBS[sub], 'restart_rows': rr}, files[off[i]:off[i + 1]].tobytes()))
        _cache['golden'] = out
    return _cache['golden']


def frame_of(a):
    """the array as the encoders take it: (h, w) for one channel"""
    return np.ascontiguousarray(a[..., 0] if a.shape[2] == 1 else a)


def pil_file(a, quality, subsampling, restart_rows=0):
    """PIL's file for a (h, w, c) array, uint8 or float32 (to8b first)"""
    t = tool()
    sub = {v: k for k, v in SUBS.items()}[subsampling]
    return t.pil_file(t.to8b(a) if a.dtype == np.float32 else a, quality, sub, restart_rows)


# shapes outside the fixtures: odd, one sample wide, an even height with an odd block count (24 x 40), several workgroups
LIVE_SHAPES = [(5, 3), (24, 40), (31, 18), (1, 20), (20, 1), (65, 33), (96, 80)]


def live_cases(seed=11):
    """[(name, array, options)]: seeded images of LIVE_SHAPES in every mode, the quality, content, restart rows and pixel type rotating"""
    t = tool()
    out = []
    i = 0
    for w, h in LIVE_SHAPES:
        for mode, c, sub in t.MODES + [('rgba420', 4, 2)]:
            q = (1, 25, 50, 75, 90, 95, 100)[i % 7]
            kind = ('noise', 'binary', 'ramp', 'checker', 'steps')[i % 5]
            rr = (0, 0, 1, 2)[i % 4]
            a = t.content(kind, w, h, c, seed + i)
            if i % 3 == 2:
                a = t.as_float(a, seed + i)
            out.append((f'w{w}_h{h}_{mode}_{kind}_q{q}_rst{rr}_{a.dtype}', a, {'quality': q, 'subsampling': SUBS[sub], 'restart_rows': rr}))
            i += 1
    return out


def fdct_int64(samples):
    """jpeg_fdct_islow in int64 numpy: samples (n, 8, 8) 0..255 -> coefficients (n, 8, 8), scaled by 8"""
    def descale(x, n):
        return (x + (1 << (n - 1))) >> n

    def one_pass(d, first):
        n = 11 if first else 15
        t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
        t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        o = np.empty_like(d)
        o[..., 0] = (t10 + t11) * 4 if first else descale(t10 + t11, 2)
        o[..., 4] = (t10 - t11) * 4 if first else descale(t10 - t11, 2)
        z1 = (t12 + t13) * 4433
        o[..., 2] = descale(z1 + t13 * 6270, n)
        o[..., 6] = descale(z1 - t12 * 15137, n)
        z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
        z5 = (z3 + z4) * 9633
        a4, a5, a6, a7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
        z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
        o[..., 7], o[..., 5], o[..., 3], o[..., 1] = descale(a4 + z1 + z3, n), descale(a5 + z2 + z4, n), descale(a6 + z2 + z3, n), descale(a7 + z1 + z4, n)
        return o

    d = samples.astype(np.int64) - 128
    d = one_pass(d, True)                                             # rows
    return one_pass(d.swapaxes(-1, -2), False).swapaxes(-1, -2)      # columns


def scan_of(data):
    """the entropy-coded bytes of a file written by the encoders or PIL: from after SOS to the EOI"""
    p = 2
    while True:
        assert data[p] == 0xFF
        mk, ln = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        p += 2 + ln
        if mk == 0xDA:
            return data[p:-2]
