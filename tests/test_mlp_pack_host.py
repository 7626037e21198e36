"""hyperreel_amd/csrc/hr_mlp_pack.h without a GPU: the header the host packer (pack_mlp, api_mlp.hip) and the device packer
(hr_pack_split_bf16_kernel) share, compiled by the plain host compiler (tests/host_math/hr_mlp_pack_host.cpp).

  conversions   float -> bf16 / IEEE half / OCP e4m3 against torch's CPU casts, zero differing codes
  layout        every byte of the tiles, the padded bias, winv and the tile count against a numpy restatement of the documented
                formulas (the header's opening comment) with torch's casts for the roundings
  pin           SHA-256 digests of the same outputs recorded from the code the header replaced (tests/golden/mlp_pack/tile_digests.json)
  scalings      the fp16 modes' weight shift and the fp8 exponent at their boundaries"""
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR, build_host_lib

HERE = os.path.dirname(os.path.abspath(__file__))
DIGESTS = os.path.join(GOLDEN_DIR, 'mlp_pack', 'tile_digests.json')
PRECISIONS = {'fp32': 0, 'bf16x3': 1, 'f16x3': 2, 'f16x2': 3, 'f16f8': 5}        # HR_MLP_* (include/hyperreel_hip.h)


def _bind(lib):
    vp, ll, i, f = C.c_void_p, C.c_longlong, C.c_int, C.c_float
    for name in ('pk_bf16', 'pk_f16', 'pk_e4m3'):
        getattr(lib, name).argtypes = [vp, ll, vp]
    if hasattr(lib, 'pk_weight_shift'):
        lib.pk_weight_shift.argtypes = lib.pk_f8_exponent.argtypes = [f]
        lib.pk_f8_headroom.restype = f
        lib.pk_f16_to_float.argtypes = lib.pk_bf16_to_float.argtypes = [vp, ll, vp]
        lib.pk_layer_geometry.argtypes = [i] * 6 + [vp] + [i] * 3 + [vp]
    lib.pk_pack_layer.argtypes = [i] * 6 + [vp] + [i] * 3 + [vp] * 5
    return lib


@functools.lru_cache(maxsize=None)
def host_lib():
    src = os.path.join(HERE, 'host_math', 'hr_mlp_pack_host.cpp')
    deps = [src, os.path.join(HERE, '..', 'include', 'hyperreel_hip.h')] + [os.path.join(HERE, '..', 'hyperreel_amd', 'csrc', f) for f in ('hr_mlp_pack.h', 'hr_plan.h', 'hr_grid.h', 'hr_math.h')]
    return _bind(C.CDLL(build_host_lib(os.path.join(HERE, 'host_math', '_build', 'libhr_mlp_pack_host.so'), src, deps)))


def _convert(fn, x, dtype):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty(x.shape, dtype)
    fn(x.ctypes.data, x.size, out.ctypes.data)
    return out


def _torch_codes(x, dtype):
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dtype)
    return t.view(torch.uint8 if t.element_size() == 1 else torch.int16).numpy().view(np.uint8 if t.element_size() == 1 else np.uint16)


# ---------------------------------------------------------------- conversions
def _with_midpoints(values):
    """the values (float32, one sign, ascending), every midpoint of two neighbours, and the floats just below and above each midpoint"""
    v = np.asarray(values, np.float64)
    mid = ((v[:-1] + v[1:]) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (v[:-1] + v[1:]) / 2)           # (one more bit than the format: exact in float32)
    return np.concatenate([v.astype(np.float32), mid, np.nextafter(mid, np.float32(-np.inf)), np.nextafter(mid, np.float32(np.inf))])


def _log_sweep(lo_exp, hi_exp, n):
    """n log-uniform magnitudes in [2^lo_exp, 2^hi_exp] (a closed form: no RNG), both signs"""
    m = np.exp2(np.linspace(lo_exp, hi_exp, n)).astype(np.float32)
    return np.concatenate([m, -m])


def half_inputs():
    halves = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)     # every finite half of one sign, ascending
    one = _with_midpoints(halves)
    return np.concatenate([one, -one, _log_sweep(-40, 20, 100000)])


def e4m3_inputs():
    codes = torch.arange(0, 0x7F, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy()  # the 127 finite codes of one sign
    one = _with_midpoints(codes)
    x = np.concatenate([one, -one, _log_sweep(-14, np.log2(448.0), 200000)])
    return x[np.abs(x) <= 448.0]                      # torch turns 480 into NaN where the packer saturates (checked below)


def test_bf16_and_half_codes_equal_torchs_casts():
    lib, x = host_lib(), half_inputs()
    assert x.size == 2 * (0x7C00 + 3 * (0x7C00 - 1)) + 200000 and np.isfinite(x).all()
    for fn, dtype in ((lib.pk_bf16, torch.bfloat16), (lib.pk_f16, torch.float16)):
        differ = int((_convert(fn, x, np.uint16) != _torch_codes(x, dtype)).sum())
        print(f'{dtype}: {x.size} inputs, {differ} codes differ', flush=True)
        assert differ == 0
    # and back: exact
    h = np.arange(0, 0x10000, dtype=np.uint16)
    back = np.empty(h.size, np.float32)
    lib.pk_f16_to_float(h.ctypes.data, h.size, back.ctypes.data)
    assert np.array_equal(back.view(np.uint32), h.view(np.float16).astype(np.float32).view(np.uint32))
    lib.pk_bf16_to_float(h.ctypes.data, h.size, back.ctypes.data)
    assert np.array_equal(back.view(np.uint32), h.astype(np.uint32) << 16)


def test_e4m3_codes_equal_torchs_cast():
    lib, x = host_lib(), e4m3_inputs()
    assert x.size == 254 + 3 * 252 + 400000 and np.abs(x).max() == 448.0
    differ = int((_convert(lib.pk_e4m3, x, np.uint8) != _torch_codes(x, torch.float8_e4m3fn)).sum())
    print(f'e4m3: {x.size} inputs, {differ} codes differ', flush=True)
    assert differ == 0


def test_saturation_infinity_and_nan():
    lib = host_lib()
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    # infinity stays infinity in bf16 and half; half overflows to infinity from 65520 (the tie above 65504) on; e4m3 saturates at +-448
    x = np.array([inf, -inf, 65519.996, 65520.0, -65520.0, 1e30, 3.4e38, -3.4e38], np.float32)
    assert list(_convert(lib.pk_f16, x, np.uint16)) == [0x7C00, 0xFC00, 0x7BFF, 0x7C00, 0xFC00, 0x7C00, 0x7C00, 0xFC00]
    assert list(_convert(lib.pk_bf16, x, np.uint16)[[0, 1, 6, 7]]) == [0x7F80, 0xFF80, 0x7F80, 0xFF80]           # (3.4e38 is above the largest bf16's tie)
    x = np.array([448.0, np.nextafter(np.float32(448), inf), 464.0, 480.0, 1e9, inf, -448.0, -480.0, -inf], np.float32)
    assert list(_convert(lib.pk_e4m3, x, np.uint8)) == [0x7E] * 6 + [0xFE] * 3
    # NaN stays a NaN in every format, whatever its sign and payload (a full mantissa used to round into -0 in bf16)
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F800001, 0xFF800001, 0x7F80FFFF], np.uint32).view(np.float32)
    assert np.isnan(nans).all()
    b = _convert(lib.pk_bf16, nans, np.uint16)
    assert ((b & 0x7F80) == 0x7F80).all() and ((b & 0x007F) != 0).all()
    h = _convert(lib.pk_f16, nans, np.uint16)
    assert ((h & 0x7C00) == 0x7C00).all() and ((h & 0x03FF) != 0).all()
    assert (_convert(lib.pk_e4m3, nans, np.uint8) == 0x7F).all()
    del nan
    # signed zeros and the smallest magnitudes
    z = np.array([0.0, -0.0, 2.0 ** -25, 2.0 ** -24, -2.0 ** -24, 2.0 ** -10, np.nextafter(np.float32(2.0 ** -10), inf), 2.0 ** -9], np.float32)
    assert list(_convert(lib.pk_f16, z[:5], np.uint16)) == [0, 0x8000, 0, 1, 0x8001]
    assert list(_convert(lib.pk_e4m3, z, np.uint8)) == [0, 0x80, 0, 0, 0x80, 0, 1, 1]


# ---------------------------------------------------------------- scalings
def test_weight_shift_boundaries():
    """14 - e with max |w| = f * 2^e, f in [0.5, 1): the largest weight lands in [2^13, 2^14); clamped to [-14, 40]; 0 without a finite
    positive maximum"""
    lib = host_lib()
    up = np.float32(np.inf)
    cases = [np.float32(2.0) ** e for e in range(-126, 128)]
    cases += [np.nextafter(v, np.float32(0)) for v in cases] + [np.nextafter(v, up) for v in cases[:-1]]
    cases += [np.float32(1e-45), np.float32(1e-40), np.float32(3.4028235e38)]
    for v in cases:
        e = int(np.frexp(np.float64(v))[1])
        want = min(40, max(-14, 14 - e))
        assert lib.pk_weight_shift(float(v)) == want, (v, want)
        if -14 < want < 40:
            assert 2.0 ** 13 <= float(v) * 2.0 ** want < 2.0 ** 14
    assert lib.pk_weight_shift(2.0 ** -28) == 40 and lib.pk_weight_shift(2.0 ** -27) == 40 and lib.pk_weight_shift(2.0 ** -26) == 39
    assert lib.pk_weight_shift(2.0 ** 27) == -14 and lib.pk_weight_shift(2.0 ** 28) == -14 and lib.pk_weight_shift(2.0 ** 26) == -13
    for v in (0.0, -0.0, float('inf'), float('nan'), -1.0):
        assert lib.pk_weight_shift(v) == 0, v


def test_f8_exponent_boundaries():
    """Ea with act_max * HR_F8_HEADROOM = f * 448 * 2^Ea, f in [0.5, 1) (the quotient formed in float32): the scaled maximum is at or
    below 448 * 2^Ea; clamped to +-30; 0 without a finite positive maximum"""
    lib = host_lib()
    room = np.float32(lib.pk_f8_headroom())
    assert room == 16.0
    up = np.float32(np.inf)
    cases = []
    for e in range(-40, 41):
        edge = np.float32(448.0 * 2.0 ** e) / room                     # act_max * headroom = 448 * 2^e exactly
        cases += [np.float32(2.0) ** e, edge, np.nextafter(edge, up), np.nextafter(edge, np.float32(0))]
    for a in cases:
        mx = np.float32(a * room)
        want = int(np.frexp(np.float32(mx / np.float32(448.0)))[1])
        want = min(30, max(-30, want))
        assert lib.pk_f8_exponent(float(a)) == want, (a, want)
        if -30 < want < 30:
            assert float(mx) <= 448.0 * 2.0 ** want and float(mx) >= 448.0 * 2.0 ** (want - 1)
    # an exact 448 * 2^e is f = 0.5 of the next octave; one float below it is the octave's top
    assert lib.pk_f8_exponent(448.0 / 16.0) == 1 and lib.pk_f8_exponent(float(np.nextafter(np.float32(28.0), np.float32(0)))) == 0
    assert lib.pk_f8_exponent(448.0 * 2.0 ** 29 / 16.0) == 30 and lib.pk_f8_exponent(448.0 * 2.0 ** 35 / 16.0) == 30
    assert lib.pk_f8_exponent(448.0 * 2.0 ** -32 / 16.0) == -30 and lib.pk_f8_exponent(448.0 * 2.0 ** -31 / 16.0) == -30
    assert lib.pk_f8_exponent(448.0 * 2.0 ** -29.5 / 16.0) == -29
    for v in (0.0, -0.0, float('inf'), float('nan'), -3.0, 3.0e38):      # (3e38 * 16 overflows)
        assert lib.pk_f8_exponent(v) == 0, v


# ---------------------------------------------------------------- layout
MLP_IN, HIDDEN, P_USER = 42, 256, 5
LIVE = [0, 2, 4]                                       # live head columns: not contiguous
COL = [LIVE.index(i) if i in LIVE else -1 for i in range(64)]
# name: (layers, skip mask, Z).  K0P = 48: the first layer's input is no multiple of 16
MLPS = {'four': (4, 1 << 1, 7), 'wide_head': (4, 1 << 1, 13), 'two': (2, 0, 7)}
# (MLP, layer, power of two on the weights; None: all zero).  first / skip / plain hidden / last with one tile (N = 21) / last with two
# (N = 39) / last AND fed by hidden activations in a two-layer MLP.  2^-60: the shift clamps at 40; zero: shift 0, winv 1.  2^30 on
# weights of 1 / sqrt(fan_in): the largest is 2^27.3 on the 42-wide first layer (14 - 28: the shift is -14 without being clamped) and 2^26
# on a 256-wide one (-12), so the layer on which the clamp at -14 BINDS is scaled by 2^34 (14 - 31)
LAYERS = [('four', 0, 0), ('four', 1, -60), ('four', 2, 34), ('four', 3, 0), ('wide_head', 3, None), ('two', 1, 0), ('two', 0, 30)]


def _hash_unit(n, seed):
    """n values in (-1, 1) with 24 significant bits from a closed-form integer hash of (index, seed)"""
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over='ignore'):
        h = (i + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)) * np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(31)
        h *= np.uint64(0x94D049BB133111EB)
        h ^= h >> np.uint64(29)
    return ((h >> np.uint64(40)).astype(np.float64) / 2.0 ** 23 - 1.0 + 2.0 ** -24).astype(np.float32)


def layer_shape(mlp, l):
    layers, skip_mask, z = MLPS[mlp]
    fan_in = MLP_IN if l == 0 else HIDDEN + (MLP_IN if (skip_mask >> l) & 1 else 0)
    fan_out = z * P_USER if l == layers - 1 else HIDDEN
    return fan_out, fan_in


@functools.lru_cache(maxsize=None)
def layer_tensors(mlp, l, power):
    """torch-layout weight (out, in) and bias (out) of the layer"""
    n, k = layer_shape(mlp, l)
    seed = 1 + 16 * sorted(MLPS).index(mlp) + l
    if power is None:
        return np.zeros((n, k), np.float32), _hash_unit(n, 1000 + seed)
    scale = np.float32(2.0 ** power / np.sqrt(k))
    return (_hash_unit(n * k, seed) * scale).reshape(n, k), _hash_unit(n, 1000 + seed) * np.float32(2.0 ** power)


def pack(lib, mlp, l, power, precision):
    """the library's packing of the layer: (tile bytes, padded bias, winv, n_tiles)"""
    layers, skip_mask, z = MLPS[mlp]
    w, b = layer_tensors(mlp, l, power)
    col = (C.c_int * 64)(*COL)
    args = (MLP_IN, HIDDEN, layers, skip_mask, z, P_USER, C.addressof(col), len(LIVE), l, PRECISIONS[precision])
    n, k = layer_shape(mlp, l)
    last = l == layers - 1
    kp = 48 if l == 0 else HIDDEN + (48 if (skip_mask >> l) & 1 else 0)
    tile_n = 16 if precision == 'fp32' else 32
    nt = -(-(z * len(LIVE) if last else n) // tile_n)
    if hasattr(lib, 'pk_layer_geometry'):
        geo = (C.c_longlong * 8)()
        lib.pk_layer_geometry(*args, C.addressof(geo))
        assert list(geo)[:2] == [n, k] and geo[3] == kp and geo[4] == nt and geo[6] == (kp // 16) * nt * 64 * 32 // (2 if precision == 'fp32' else 1) and geo[7] == nt * tile_n
    tiles = np.full((kp // 16) * nt * 64 * (16 if precision == 'fp32' else 32), 0xAB, np.uint8)
    bias = np.full(nt * tile_n, np.nan, np.float32)
    winv = C.c_float(np.nan)
    wc, bc = np.ascontiguousarray(w), np.ascontiguousarray(b)
    lib.pk_pack_layer(*args, wc.ctypes.data, bc.ctypes.data, tiles.ctypes.data, bias.ctypes.data, C.addressof(winv))
    return tiles, bias, np.float32(winv.value), nt


def expected(mlp, l, power, precision):
    """The same from the documented formulas alone.  Kernel matrix W'[n][kk]: K order (first layer: the input padded to 48; skip layer:
    [input padded to 48 | hidden]; else the hidden index), row map (last layer: kernel row k * P_live + c' = user row k * P_user +
    live[c']), zero elsewhere.  Split tiles [Kp/16][nt][hi, lo][64 lanes][8] 16-bit, lane l holding W'[32 t + (l & 31)][16 kt +
    8 (l >> 5) + 0..7]; fp32 tiles [Kp/16][nt][64][4], W[16 t + (l & 15)][16 kt + 4 (l >> 4) + 0..3]."""
    layers, skip_mask, z = MLPS[mlp]
    w, b = layer_tensors(mlp, l, power)
    first, skip, last = l == 0, bool((skip_mask >> l) & 1), l == layers - 1
    tile_n = 16 if precision == 'fp32' else 32
    rows = [k * P_USER + c for k in range(z) for c in LIVE] if last else list(range(HIDDEN))
    nt = -(-len(rows) // tile_n)
    if first:
        cols = list(range(MLP_IN)) + [-1] * 6
    elif skip:
        cols = list(range(MLP_IN)) + [-1] * 6 + list(range(MLP_IN, MLP_IN + HIDDEN))
    else:
        cols = list(range(HIDDEN))
    kp = len(cols)
    assert kp % 16 == 0 and max(cols) == w.shape[1] - 1 and (not skip or cols[48] == 42)
    wk = np.zeros((nt * tile_n, kp), np.float32)
    live_k = [i for i, cc in enumerate(cols) if cc >= 0]
    wk[np.ix_(range(len(rows)), live_k)] = w[np.ix_(rows, [cols[i] for i in live_k])]
    bk = np.zeros(nt * tile_n, np.float32)
    bk[:len(rows)] = b[rows]
    half = precision in ('f16x3', 'f16x2', 'f16f8')
    shift = 0
    mx = float(np.abs(w).max())
    if half and mx > 0 and np.isfinite(mx):
        shift = min(40, max(-14, 14 - int(np.frexp(mx)[1])))
    wmul = np.float32(2.0 ** shift)
    kt, t, lane = np.meshgrid(np.arange(kp // 16), np.arange(nt), np.arange(64), indexing='ij')
    if precision == 'fp32':
        s = np.arange(4)
        tiles = wk[(16 * t + (lane & 15))[..., None], (16 * kt + 4 * (lane >> 4))[..., None] + s]
    else:
        j = np.arange(8)
        v = torch.from_numpy(np.ascontiguousarray((wk * wmul)[(32 * t + (lane & 31))[..., None], (16 * kt + 8 * (lane >> 5))[..., None] + j]))   # [kt][t][lane][8]
        dt = torch.float16 if half else torch.bfloat16
        hi = v.to(dt)
        res = v - hi.float()
        lo = res.to(dt)
        tiles = torch.stack([hi, lo], 2).view(torch.int16).numpy().view(np.uint16).copy()       # [kt][t][part][lane][8]
        if precision == 'f16f8':
            kseg = kp // 16 if first else (3 if skip else 0)
            # (beyond 448 the packer saturates where torch's cast gives NaN: only the layer whose shift is clamped gets there)
            e4m3 = lambda x: torch.clamp(x, -448.0, 448.0).to(torch.float8_e4m3fn)
            images = torch.cat([e4m3(res * 64.0), e4m3(v * (1.0 / 64.0))], -1).view(torch.uint8).numpy()   # [kt][t][lane][16]
            tiles[kseg:, :, 1] = images[kseg:].view(np.uint16)
    return np.ascontiguousarray(tiles).view(np.uint8).ravel(), bk * wmul, np.float32(2.0 ** -shift), nt, shift


@pytest.mark.parametrize('precision', sorted(PRECISIONS))
@pytest.mark.parametrize('mlp,l,power', LAYERS)
def test_every_byte_is_where_the_documented_layout_puts_it(mlp, l, power, precision):
    tiles, bias, winv, nt = pack(host_lib(), mlp, l, power, precision)
    want_tiles, want_bias, want_winv, want_nt, shift = expected(mlp, l, power, precision)
    assert nt == want_nt and winv == want_winv
    assert np.array_equal(bias.view(np.uint32), want_bias.view(np.uint32))
    assert tiles.size == want_tiles.size
    differ = int((tiles != want_tiles).sum())
    assert differ == 0, f'{differ} of {tiles.size} bytes differ'
    # the cases reach what they are there for
    layers, skip_mask, z = MLPS[mlp]
    if precision in ('f16x3', 'f16x2', 'f16f8'):
        assert shift == {-60: 40, 34: -14, 30: -14, None: 0}.get(power, shift)
        if power is None:
            assert winv == 1.0
    else:
        assert winv == 1.0
    if l == layers - 1:
        n = z * len(LIVE)
        assert n % 32 != 0 and (bias[n:] == 0).all() and nt == {('fp32', 7): 2, ('fp32', 13): 3}.get((precision, z), 1 if z == 7 else 2)
    if l == 0 and precision != 'fp32':             # feature columns 42..47 of the padded input: zero in both halves
        t16 = tiles.view(np.uint16).reshape(3, nt, 2, 64, 8)
        assert (t16[2, :, :, 32:, 2:] == 0).all() and (t16[2, :, :, 32:, :2] != 0).any()


def test_f16f8_differs_from_f16x3_exactly_over_the_hidden_k_steps():
    """before kseg the lo part is the f16 low half, from kseg on the two fp8 images"""
    lib = host_lib()
    for mlp, l, power in LAYERS:
        layers, skip_mask, z = MLPS[mlp]
        a, b = pack(lib, mlp, l, power, 'f16x3'), pack(lib, mlp, l, power, 'f16f8')
        nt = a[3]
        ta, tb = a[0].reshape(-1, nt, 2, 64 * 16), b[0].reshape(-1, nt, 2, 64 * 16)
        kseg = ta.shape[0] if l == 0 else (3 if (skip_mask >> l) & 1 else 0)
        assert np.array_equal(ta[:, :, 0], tb[:, :, 0]) and np.array_equal(ta[:kseg], tb[:kseg])
        if power is not None:
            assert all((ta[k, :, 1] != tb[k, :, 1]).any() for k in range(kseg, ta.shape[0]))
        assert np.array_equal(a[1], b[1]) and a[2] == b[2]


# ---------------------------------------------------------------- the parent's bytes
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digests(lib):
    """{'<mlp>/layer<l>/<precision>': {'tiles', 'bias', 'winv'}}: SHA-256 of the tile bytes, of the padded bias' bytes and of winv's"""
    out = {}
    for mlp, l, power in LAYERS:
        for precision in sorted(PRECISIONS):
            tiles, bias, winv, _ = pack(lib, mlp, l, power, precision)
            out[f'{mlp}/layer{l}/{precision}'] = {'tiles': _sha(tiles), 'bias': _sha(bias), 'winv': _sha(np.float32(winv))}
    return out


def test_the_header_gives_the_bytes_of_the_code_it_replaced():
    """tests/golden/mlp_pack/tile_digests.json: `digests()` above, run ONCE on the packer this header replaced and never on the header
    under test.  That packer's loops sat between hipMemcpy calls inside pack_mlp_as (csrc/api_mlp.hip of the commit before
    hr_mlp_pack.h existed), so they were lifted verbatim -- its anonymous-namespace conversions (lines 14-68) and the body of its layer
    loop (lines 139-228: the K-order lambda, the shift, the three nested loops, the fp8 pass, the bias) -- into a throw-away
    translation unit behind a function with pk_pack_layer's signature that takes host vectors (hipMemcpy replaced by memcpy), compiled
    host-only with ROCm's clang++ (which has _Float16) at -O1 -ffp-contract=off, and loaded here in host_lib()'s place.  The inputs are
    LAYERS x PRECISIONS as above: all finite, so the one deliberate change of bits (NaN) is not among them."""
    with open(DIGESTS) as fh:
        want = json.load(fh)
    got = digests(host_lib())
    assert sorted(got) == sorted(want) and len(got) == len(LAYERS) * len(PRECISIONS)
    differ = [k for k in want if got[k] != want[k]]
    print(f'{len(want)} recorded packings, {len(differ)} differ', flush=True)
    assert not differ, differ
    # the recorded cases tell the branches apart
    t = lambda key: want[key]['tiles']
    assert t('four/layer2/f16x3') != t('four/layer2/f16f8') and t('four/layer1/f16x3') != t('four/layer1/f16f8')      # hidden k-steps: fp8 images
    assert t('four/layer0/f16x3') == t('four/layer0/f16f8')                                                            # a first layer has none (kseg = Kp / 16)
    assert t('four/layer0/f16x3') == t('four/layer0/f16x2') and t('four/layer0/f16x3') != t('four/layer0/bf16x3') != t('four/layer0/fp32')
    assert t('four/layer3/f16x3') != t('two/layer1/f16x3') and t('four/layer3/bf16x3') != t('wide_head/layer3/bf16x3')
    assert want['four/layer1/f16x3']['winv'] != want['four/layer2/f16x3']['winv'] != want['wide_head/layer3/f16x3']['winv']   # 2^-40, 2^14, 1
    assert want['wide_head/layer3/f16x3']['winv'] == want['four/layer0/bf16x3']['winv'] == _sha(np.float32(1.0))
