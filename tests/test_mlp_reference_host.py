"""tests/mlp_reference.py checked without a GPU: the float64 reference against the oracle, its restated weight roundings against the
packer's own bytes (pk_pack_layer of the host build), and the tolerances of tests/test_gpu_mlp_structure.py on the reference alone --
on every case of the structure grid a lost activation-side correction product is far above the fp32 chain's own error, a numpy model
of each arithmetic passes half the tolerance, and dropped(a) fails it.  The exact cases meet their precondition."""
import ctypes as C

import numpy as np
import pytest
import torch

import mlp_reference as R
from helpers import Golden
from test_mlp_pack_host import PRECISIONS, host_lib

F32, F64 = np.float32, np.float64


def test_exact_rounded_to_fp32_agrees_with_the_oracles_head():
    """the shipped DoNeRF net with fixture weights: `exact` against the oracle's _head_raw (its fp32 chain) to E_ref32, which is that very
    difference measured through the module's own chain32 -- and of the size fp32 summation gives (a few 1e-7 of the largest head value)"""
    from hyperreel_oracle import HyperReelOracle
    g = Golden('donerf_sphere_small')
    case = R.Case('golden', g.cfg, g.dataset, g.rays, sd=g.state_dict)
    head = HyperReelOracle(g.cfg, g.dataset, g.state_dict).embed(g.rays)['_head_raw']
    assert head.dtype == F32 and head.shape == case.exact().shape == (g.rays.shape[0], 32 * 15)
    assert np.array_equal(head, case.chain32())
    e = R.err(case.exact().astype(F32), head)
    e_ref32 = R.err(case.chain32(), case.exact())
    print(f'exact vs _head_raw {e:.3e}, E_ref32 {e_ref32:.3e}', flush=True)
    assert e <= e_ref32 + 2.0 ** -24 and 1e-8 < e_ref32 < 2e-6
    assert case.live_mask().sum() == 32 * 11 and case.live_mask(prune=False).all()


# ---------------------------------------------------------------- stored(a) against the packer's bytes
def _unpack(lib, case, l, a, prune=True):
    """What pk_pack_layer packed of layer l, read back through the documented tile layout: (kernel matrix W'[n][kk] as hi + lo in the
    packed unit, winv, row map, K map)"""
    hc = case.hc()
    col, p_live, _ = R.live_columns(hc, prune)
    layers, z, p_user, k_in, hidden = hc.mlp_layers, hc.z_channels, hc.preds_per_z, hc.mlp_in, hc.mlp_hidden
    w, b = case.layers[l]
    first, skip, last = l == 0, bool((hc.mlp_skip_mask >> l) & 1), l == layers - 1
    k0p = (k_in + 15) & ~15
    kp = k0p if first else (k0p + hidden if skip else hidden)
    tile_n = 16 if a == 'fp32' else 32
    live = [i for i in range(p_user) if col[i] >= 0]
    rows = [k * p_user + c for k in range(z) for c in live] if last else list(range(hidden))
    nt = -(-len(rows) // tile_n)
    colc = (C.c_int * 64)(*col)
    tiles = np.zeros((kp // 16) * nt * 64 * (16 if a == 'fp32' else 32), np.uint8)
    bias = np.zeros(nt * tile_n, F32)
    winv = C.c_float(0)
    wc, bc = np.ascontiguousarray(w, F32), np.ascontiguousarray(b, F32)
    lib.pk_pack_layer(k_in, hidden, layers, hc.mlp_skip_mask, z, p_user, C.addressof(colc), p_live, l, PRECISIONS[a],
                      wc.ctypes.data, bc.ctypes.data, tiles.ctypes.data, bias.ctypes.data, C.addressof(winv))
    kt, t, lane = np.meshgrid(np.arange(kp // 16), np.arange(nt), np.arange(64), indexing='ij')
    got = np.zeros((nt * tile_n, kp), F64)
    if a == 'fp32':
        s = np.arange(4)
        got[(16 * t + (lane & 15))[..., None], (16 * kt + 4 * (lane >> 4))[..., None] + s] = tiles.view(F32).reshape(kp // 16, nt, 64, 4)
    else:
        j = np.arange(8)
        n_idx, k_idx = (32 * t + (lane & 31))[..., None], (16 * kt + 8 * (lane >> 5))[..., None] + j
        words = tiles.view(np.uint16).reshape(kp // 16, nt, 2, 64, 8)
        dt = torch.bfloat16 if a == 'bf16x3' else torch.float16
        as_float = lambda u16: torch.from_numpy(np.ascontiguousarray(u16).view(np.int16)).view(dt).double().numpy()
        hi, lo = as_float(words[:, :, 0]), as_float(words[:, :, 1])
        if a == 'f16x2':
            lo = lo * 0.0                      # (packed like f16x3; the two-product kernel does not read the low half)
        if a == 'f16f8':
            kseg = kp // 16 if first else (k0p // 16 if skip else 0)
            img = torch.from_numpy(np.ascontiguousarray(words[:, :, 1]).view(np.uint8).reshape(kp // 16, nt, 64, 16)[..., :8].copy())
            lo[kseg:] = (img.view(torch.float8_e4m3fn).double().numpy() / 64.0)[kseg:]
        got[n_idx, k_idx] = hi + lo
    if first:
        kmap = list(range(k_in)) + [-1] * (k0p - k_in)
    elif skip:
        kmap = list(range(k_in)) + [-1] * (k0p - k_in) + list(range(k_in, k_in + hidden))
    else:
        kmap = list(range(hidden))
    return got, np.float64(winv.value), rows, kmap, bias


@pytest.mark.parametrize('a', R.ARITHMETICS)
def test_stored_weights_equal_what_the_packer_packed(a):
    """one skip layer (layer 3 of the base net: input k-steps padded from 18 to 32, then the hidden ones) and one last layer (352 live
    rows of 480) in every arithmetic, element for element; every padding element of the tiles is zero"""
    lib, case = host_lib(), R.get_case('base', 'hostile')
    for l in (3, 5):
        got, winv, rows, kmap, bias = _unpack(lib, case, l, a)
        w, b = case.layers[l]
        n_in = 18 if l == 3 else 0
        want = R.stored_weights(w, a, n_in)
        s = R.weight_shift(w) if a in ('f16x3', 'f16x2', 'f16f8') else 0
        assert winv == 2.0 ** -s
        live_k = [i for i, c in enumerate(kmap) if c >= 0]
        sub = got[np.ix_(range(len(rows)), live_k)] * winv
        assert np.array_equal(sub, want[np.ix_(rows, [kmap[i] for i in live_k])]), f'layer {l}: {int((sub != want[np.ix_(rows, [kmap[i] for i in live_k])]).sum())} elements differ'
        pad = got.copy()
        pad[np.ix_(range(len(rows)), live_k)] = 0.0
        assert not pad.any()
        assert np.array_equal(bias[:len(rows)].astype(F64) * winv, b[rows].astype(F64)) and not bias[len(rows):].any()
        if a in ('bf16x3', 'f16x2', 'f16f8'):                  # (f16x3's two halves hold most fp32 weights whole)
            assert (want != w.astype(F64)).any()
    assert len(rows) == 352 and len(kmap) == 256


# ---------------------------------------------------------------- the tolerances, on the reference alone
def _grid():
    out = [(n, i, True) for n in R.GRID for i in R.INITS] + [(n, i, False) for n in R.N_OUT for i in R.INITS]
    out += [(n, i, True) for n in R.WIDTHS + ['pe_limit_16', 'pe_beyond_256'] for i in R.INITS]
    return out


@pytest.mark.parametrize('name,init,prune', _grid())
def test_tolerances_hold_on_the_reference_alone(name, init, prune):
    """E_drop(a) >= 64 E_ref32; the numpy model of the arithmetic passes T(a) / 2; dropped(a) fails T(a)."""
    case = R.get_case(name, init)
    mask = case.live_mask(prune)
    e32 = case.e_ref32(prune)
    assert 0 < e32 < 4e-6, e32
    for a in case.arithmetics:
        T = case.tolerance(a, prune)
        m = R.err(case.model(a), case.stored(a), mask)
        line = f'{case.name} prune={int(prune)} {a}: E_ref32 {e32:.2e} T {T:.2e} model {m:.2e}'
        if a != 'fp32':
            d = case.e_drop(a, prune)
            line += f' E_drop {d:.2e}'
        print(line, flush=True)
        assert m <= T / 2, line
        if a != 'fp32':
            assert d >= 64 * e32, line
            assert d > T, line


def test_the_grid_reaches_the_shapes_it_is_there_for():
    """k0p, the last Linear's tiles, the skip masks and the depths the issue names, read off the compiled configs"""
    def shape(name, prune=True):
        case = R.get_case(name)
        hc = case.hc()
        n_out = int(case.live_mask(prune).sum())
        return hc.mlp_in, hc.mlp_layers, hc.mlp_skip_mask, hc.mlp_hidden, n_out
    assert shape('base') == (18, 6, 1 << 3, 256, 352) and 352 == 11 * 32
    assert [shape(n)[1] for n in ('depth2', 'depth3', 'depth8')] == [2, 3, 8] and R.plan.HR_MAX_LAYERS == 8
    assert [shape(n)[2] for n in ('depth2', 'depth3', 'skips_none', 'skip_1', 'skip_last', 'skips_all_depth8')] == [0, 2, 0, 2, 32, 254]
    assert [shape(n)[0] for n in ('in4', 'in12', 'in16', 'in20', 'in64', 'basic_pe', 'out_960_time_group')] == [4, 12, 16, 20, 64, 30, 23]
    assert [shape(n)[4] for n in R.N_OUT] == [22, 352, 374, 385, 960] and 374 <= 12 * 32 and 385 == 12 * 32 + 1
    assert [shape(n, False)[4] for n in R.N_OUT] == [30, 480, 510, 525, 960]
    assert [shape(n)[3] for n in R.WIDTHS] == [64, 128]
    for name, ok in (('in64', True), ('pe_limit_16', True), ('pe_beyond_256', False)):
        assert R.plan.fast_sincos_ok(R.get_case(name).hc()) == ok
    # the far rays: arguments of the order the issue names
    f = R.get_case('pe_beyond_256')
    y = f.oracle._param_pe_cfg({'ray': dict(f.cfg.embedding.embeddings.ray_prediction_0.params.ray, pe=None)}, f.rays)
    assert 256 * np.abs(y).max() > 700 and 256 * np.median(np.abs(y)) > 256


# ---------------------------------------------------------------- the exact cases
@pytest.mark.parametrize('skips', R.EXACT_SKIPS)
@pytest.mark.parametrize('depth', R.EXACT_DEPTHS)
def test_exact_cases_meet_their_precondition(depth, skips):
    """every intermediate a non-negative integer <= 2048 that one f16 (two bf16 halves) holds; every stored weight the weight itself,
    every low half and fp8 image 0; so exact == stored(a) == dropped-free model(a) bit for bit in every arithmetic, and the head's
    columns tell indices apart"""
    case = R.get_exact_case(depth, skips)
    ok, largest = R.exact_precondition(case)
    assert ok and largest <= 2048 and largest == float(case.exact().max())
    for a in R.ARITHMETICS:
        for l, (w, b) in enumerate(case.layers):
            k_in = w.shape[1] if l == 0 else (6 if l in case.skips else 0)
            s, hi, lo = R.stored_parts(w, a, k_in)
            assert np.array_equal(hi * 2.0 ** -s, w.astype(F64)) and not lo.any()
        assert np.array_equal(case.stored(a), case.exact())
        assert np.array_equal(case.model(a), case.exact()), a
    x = case.exact()
    hi, lo = R.two_halves(x.astype(F32), torch.bfloat16)
    assert np.array_equal(hi + lo, x) and np.array_equal(R.round_to(x, torch.float16), x)
    live = x[:, case.live_mask()]
    assert len({c.tobytes() for c in live.T}) >= live.shape[1] / 2
