"""The training image loss without a GPU: hr_loss_out (include/hyperreel_hip.h) against its ctypes mirror, the bound entry points, the
shared arithmetic of hyperreel_amd/csrc/hr_loss.h compiled by the host compiler against the reference's own loss modules
(tests/golden/loss, tools/make_loss_golden.py), the float64 oracle (tests/loss_oracle.py) against the same fixtures, and what
hyperreel_amd.losses refuses.  The bars are derived in tests/loss_common.py.

Measured on the fixtures (36 variant x batch cases): hr_loss.h's gradient equals the reference's float32 autograd gradient bit for bit
in every case; its loss (terms added in double, one rounding) is within 0.32 of its bar; the oracle is within 4e-16 relative of the
reference's float64 results."""
import ctypes as C

import numpy as np
import pytest

import loss_common as LC
import loss_oracle as LO
from hyperreel_amd import lib

CASES = [(v, B) for v in LC.VARIANTS for B in LC.BATCHES]


@pytest.fixture(scope='module')
def hl():
    return LC.host_lib()


def test_hr_loss_out_layout_matches_c(hl):
    assert hl.hl_sizeof_out() == C.sizeof(lib.hr_loss_out) == 24
    assert [n for n, _ in lib.hr_loss_out._fields_] == ['loss_sum', 'sse', 'loss', 'pad']
    for i, (name, want) in enumerate((('loss_sum', 0), ('sse', 8), ('loss', 16), ('pad', 20))):
        assert hl.hl_offsetof_out(i) == getattr(lib.hr_loss_out, name).offset == want, name
    codes = [hl.hl_type_code(i) for i in range(6)]
    assert codes == [lib.HR_LOSS_MSE, lib.HR_LOSS_WEIGHTED_MSE, lib.HR_LOSS_MAE, lib.HR_LOSS_WEIGHTED_MAE, lib.HR_LOSS_HUBER, lib.HR_LOSS_PREMULTIPLIED]
    from hyperreel_amd import losses
    assert losses.OUT_DOUBLES == 3 and {k: v for k, v in losses.TYPES.items()} == {t: c for t, c, _ in LC.VARIANTS.values()}


def test_loss_entry_points_are_bound_at_abi_27(hl):
    assert lib.ABI_VERSION == 27 == hl.hl_abi_version()
    bound = {name: (res, args) for name, res, args in lib.SYMBOLS}
    assert bound['hr_image_loss_workspace'] == (C.c_size_t, [C.c_int64])
    assert bound['hr_image_loss'] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p])


def test_library_exports_the_loss_and_sizes_its_workspace(hl):
    """No GPU: the workspace size is host arithmetic, and the argument checks come before any launch."""
    L = lib.load()
    assert L.hr_image_loss_workspace(0) == 0 and L.hr_image_loss_workspace(-3) == 0
    last = 0
    for n in (1, 2, 63, 64, 65, 257, 1023, 1024, 1025, 4099, 16384, 16385, 1 << 20, (1 << 31) + 7, 1 << 36):
        got = L.hr_image_loss_workspace(n)
        assert got == 16 * hl.hl_blocks(n) == 16 * -(-n // 1024), n        # one slot of two doubles per workgroup of 1024 rays
        assert got > 0 and got >= last, n
        last = got
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    call = lambda pred, n, type, delta=1.0, out=p, ws=p: L.hr_image_loss(pred, p, None, n, type, delta, None, out, None, ws, None)
    assert call(p, 0, lib.HR_LOSS_MSE) == -1 and b'batch size' in L.hr_last_error()
    assert call(p, -5, lib.HR_LOSS_MSE) == -1
    for bad in (5, 17, -1, 0x200, 0x105, 0x1000 | lib.HR_LOSS_MAE):
        assert call(p, 8, bad) == -1 and b'unknown loss type' in L.hr_last_error(), bad
        assert not hl.hl_type_valid(bad)
    for ok in range(5):
        assert hl.hl_type_valid(ok) and hl.hl_type_valid(ok | lib.HR_LOSS_PREMULTIPLIED)
    assert call(None, 8, lib.HR_LOSS_MSE) == -1 and b'null' in L.hr_last_error()
    assert call(p, 8, lib.HR_LOSS_MSE, out=None) == -1 and call(p, 8, lib.HR_LOSS_MSE, ws=None) == -1
    assert call(p, 8, lib.HR_LOSS_HUBER, delta=0.0) == -1 and b'delta' in L.hr_last_error()
    assert call(p, 8, lib.HR_LOSS_HUBER, delta=float('nan')) == -1


def test_fixture_inputs_hold_the_cases_every_branch_needs():
    assert sorted(LC.VARIANTS) == sorted(['mse', 'weighted_mse', 'mae', 'weighted_mae', 'huber_delta1', 'huber_delta0p1'])
    seen = dict(equal=0, zero_w=0, other_w=0, outside=0)
    for B in LC.BATCHES:
        p, g, w = LC.inputs(B)
        assert p.shape == g.shape == (B, 3) and w.shape == (B, 1) and p.dtype == g.dtype == w.dtype == np.float32
        seen['equal'] += int((p == g).all(1).sum())
        seen['zero_w'] += int((w == 0).sum())
        seen['other_w'] += int(((w != 0) & (w != 1)).sum())
        seen['outside'] += int(((p < 0) | (p > 1)).sum())
        d = np.abs(p * w - g * w)
        for delta in (np.float32(1.0), np.float32(0.1)):              # exactly delta, and on both sides of it, in every batch
            assert (d == delta).any(), (B, delta)
            if B > 1:
                assert (d == np.nextafter(delta, np.float32(0))).any() and (d == np.nextafter(delta, np.float32(4))).any(), (B, delta)
                assert ((d < delta) & (d > 0)).any() and (d > delta).any()
    assert min(seen.values()) > 0, seen


@pytest.mark.parametrize('variant', list(LC.VARIANTS))
def test_meta_records_the_measured_deviations_and_bars(variant):
    m = LC.meta(variant)
    dev = LC.deviations_of(LC.load_file(variant))
    for k, v in {**dev, **LC.bars_of(dev)}.items():
        assert m[k] == v, k
    assert m['batches'] == LC.BATCHES and m['cfg']['type'] == LC.VARIANTS[variant][0]
    assert 0 < dev['loss_deviation'] < 1e-6 and 0 < dev['grad_deviation'] < 1e-5         # float32 evaluations, and really not float64 ones
    print(f"{variant}: reference |f32 - f64| loss {dev['loss_deviation']:.3e} grad {dev['grad_deviation']:.3e} (relative to the array's largest)")


@pytest.mark.parametrize('variant,B', CASES)
def test_shared_arithmetic_reproduces_the_reference(hl, variant, B):
    """hr_loss.h on the host: step_loss's form (the multiplies inside) and the reference's call form (premultiplied tensors) both give
    the reference's loss and its gradient with respect to the un-multiplied prediction."""
    _, code, delta = LC.VARIANTS[variant]
    p, g, w = LC.inputs(B)
    e = LC.expected(variant, B)
    got = LC.host_loss(hl, code, delta, p, g, w)
    lbar, gbar = LC.loss_bar(variant, e['loss64']), LC.grad_bar(variant, e['grad64'])
    lerr = abs(float(got['loss']) - float(e['loss32']))
    gerr = float(np.abs(got['grad'].astype(np.float64) - e['grad32'].astype(np.float64)).max())
    print(f'{variant} B={B}: loss err {lerr:.3e} (bar {lbar:.3e})  grad err {gerr:.3e} (bar {gbar:.3e})')
    assert lerr <= lbar and gerr <= gbar
    assert got['pad'] == 0.0 and got['loss'] == np.float32(got['loss_sum'] / (3 * B))
    sse = float(((p.astype(np.float64) - g) ** 2).sum())
    assert abs(got['sse'] - sse) <= 1e-6 * sse
    # the reference's call form: the same loss; its gradient is with respect to pred * weight, the multiply's backward brings the weight
    pre = LC.host_loss(hl, code | lib.HR_LOSS_PREMULTIPLIED, delta, p * w, g * w, w)
    assert pre['loss'] == got['loss'] and pre['loss_sum'] == got['loss_sum']
    assert np.abs((pre['grad'] * w).astype(np.float64) - e['grad32']).max() <= gbar
    # an upstream factor multiplies the finished gradient: exactly, element by element
    up = LC.host_loss(hl, code, delta, p, g, w, upstream=3.0)
    assert np.array_equal(up['grad'], got['grad'] * np.float32(3.0)) and up['loss'] == got['loss']
    # no weight: every weight 1
    ones = LC.host_loss(hl, code, delta, p, g, np.ones_like(w))
    none = LC.host_loss(hl, code, delta, p, g, None)
    assert none['loss_sum'] == ones['loss_sum'] and np.array_equal(none['grad'], ones['grad'])


@pytest.mark.parametrize('variant,B', CASES)
def test_oracle_agrees_with_the_reference_in_float64(variant, B):
    name, _, delta = LC.VARIANTS[variant]
    p, g, w = LC.inputs(B)
    e = LC.expected(variant, B)
    o = LO.loss(name, p, g, w, delta)
    assert abs(o['loss'] - float(e['loss64'])) <= 1e-12 * abs(float(e['loss64']))
    assert np.abs(o['grad'] - e['grad64']).max() <= 1e-12 * np.abs(e['grad64']).max()
    pre = LO.loss(name, p.astype(np.float64) * w, g.astype(np.float64) * w, w, delta, premultiplied=True)
    assert abs(pre['loss'] - o['loss']) <= 1e-15 * o['loss'] and np.abs(pre['grad'] * w - o['grad']).max() <= 1e-15 * np.abs(o['grad']).max()


def test_refused_types_raise_naming_themselves():
    from hyperreel_amd import losses
    for t in ('tv', 'complex_mse', 'complex_mae', 'mse_top_n', 'mae_top_n'):
        with pytest.raises(NotImplementedError, match=f"'{t}'"):
            losses.get_loss({'type': t, 'frac': 0.5})
    with pytest.raises(KeyError, match='no_such_loss'):
        losses.get_loss({'type': 'no_such_loss'})
    for t in LO.TYPES:
        m = losses.get_loss({'type': t})
        assert m.type == t and m.kind == losses.TYPES[t] and m.delta == 1.0
    assert losses.get_loss({'type': 'huber', 'delta': 0.1}).delta == 0.1
    assert losses.get_loss('mse').type == 'mse'

    class Node:                                  # attribute access, as a configuration node gives
        type, delta = 'huber', 0.25
    assert losses.get_loss(Node()).delta == 0.25


def test_python_surface_refuses_cpu_and_malformed_tensors():
    import torch
    from hyperreel_amd import losses
    m = losses.get_loss({'type': 'mse'})
    x, w = torch.zeros((16, 3)), torch.ones((16, 1))
    with pytest.raises(RuntimeError, match='no CPU path'):
        m(x, x, weight=w)
    with pytest.raises(RuntimeError, match='no CPU path'):
        m.step_loss(x, x, w)
    with pytest.raises(ValueError, match=r'\(B, 3\)'):
        m.step_loss(torch.zeros((16, 4)), x, w)


@pytest.mark.reference
def test_fixtures_regenerate_bit_for_bit():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(LC.HERE), 'tools'))
    import make_loss_golden as G
    made = G.make_all()
    assert sorted(made) == sorted(['inputs', *LC.VARIANTS])
    for stem, arrays in made.items():
        stored = LC.load_file(stem)
        assert sorted(arrays) == sorted(stored), stem
        for k, a in arrays.items():
            if k == 'meta':                      # the torch version that wrote the file is recorded, not compared
                import json
                new, old = json.loads(bytes(a).decode()), json.loads(bytes(stored[k]).decode())
                new.pop('torch'), old.pop('torch')
                assert new == old, stem
            else:
                assert a.dtype == stored[k].dtype and a.shape == stored[k].shape and a.tobytes() == stored[k].tobytes(), (stem, k)
