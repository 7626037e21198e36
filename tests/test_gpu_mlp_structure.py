"""`-m gpu`: the sample-prediction MLP (K1; csrc/mlp_split_core.inc, mlp_*_kernel.hip, mlp_kernel.hip) held, per (structure, arithmetic), to
the float64 chain of tests/mlp_reference.py -- every live column of every ray of the raw head against stored(a), the chain whose weights
are what arithmetic `a` keeps of them, on structures no shipped net has: 2, 3 and HR_MAX_LAYERS layers; no skip, a skip into layer 1, into
the last Linear, into every layer; mlp_in 4 ... 64 (k0p padded to 16); heads under one 32-column tile, of exactly 11 tiles, of 12, of 12
and one column, of 960 columns; both column maps (HR_PRUNE); widths 64 and 128 of the exact-fp32 kernel; ragged ray counts; and exact
integer cases that must come out bit for bit.  The tolerance is computed per case from the reference alone (mlp_reference.Case.tolerance:
T(fp32) = 8 E_ref32, T(f16x3 / bf16x3 / f16x2) = E_drop / 64 + 8 E_ref32, T(f16f8) = E_drop / 4 + 8 E_ref32), never read off the
device; tests/test_mlp_reference_host.py shows on the CPU that a kernel without its activation-side correction product fails each one.
The head is exported by the two-kernel plan only (the frame kernel keeps it in LDS): where the frame kernel fits, its image must equal the
two-kernel plan's bit for bit, and where it must step aside (fp32, a skip into the last Linear, more than 12 tiles, a keyframe net on
64-ray tiles) it must be inactive.

Measured on an MI355X, error / T, worst case over the grid (structures x initialisers x column maps; 255 heads):
  fp32 0.18 (in4, hostile)   bf16x3 0.14 (in4)   f16x3 0.14 (skip_1)   f16x2 0.12 (depth8)   f16f8 0.64 (in4, hostile)
f16f8 against its first bound, E_drop / 8 + 8 E_ref32, measured 1.25 (in4 hostile), 1.17 (in4), 1.04 (in12) and 0.99 (in12 hostile) -- the
fp8 exponents of a model calibrated on synthetic rays that graze the two planes, not the kernels (mlp_reference's docstring); calibrated
on the rendered rays the same cases measure 0.29 - 0.33 of that bound, which test_f16f8_calibrated_on_its_rays_holds_the_tight_bound
keeps.  Every other f16f8 case: 0.25 - 0.34 of the first bound.
"""
import numpy as np
import pytest
import torch

import mlp_reference as R

pytestmark = pytest.mark.gpu
F64 = np.float64


def _model(case, a):
    from gpu_common import make_render_fn
    return make_render_fn(case.cfg, case.dataset, case.sd, mlp_precision=a).model


def _head(m, rays):
    return m.render(rays, want=('head',))['head']


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check_plans(m, rays, case, a, prune, expect_fit):
    """after the head: the frame kernel where it fits -- same bits in the image -- and inactive where it must not fit"""
    video = case.cfg.color.net.type == 'tensor_vm_split_time'
    tiles = -(-int(case.live_mask(prune).sum()) // 32)
    must_not_fit = a == 'fp32' or case.hidden != 256 or (case.depth - 1) in case.skips or tiles > 12 or video
    m.set_execution(frame_kernel=True)
    active = m.frame_kernel_active()
    assert not (must_not_fit and active)
    if expect_fit:
        assert active
    if active:
        one = m.render(rays)['rgb'].clone()
        m.set_execution(frame_kernel=False)
        assert not m.frame_kernel_active()
        two = m.render(rays)['rgb']
        assert _bits_equal(one, two), f'{int((one.view(torch.int32) != two.view(torch.int32)).any(-1).sum())} rays differ between the plans'


def _check_tolerance(name, init, a, prune, monkeypatch, expect_fit=False):
    case = R.get_case(name, init)
    if not prune:
        monkeypatch.setenv('HR_PRUNE', '0')
    m = _model(case, a)
    assert m.mlp_precision_active() == a
    assert not m.frame_kernel_active()
    rays = torch.from_numpy(case.rays).cuda()
    head = _head(m, rays).cpu().numpy()
    mask = case.live_mask(prune)
    assert head.shape == (R.N_RAYS, mask.size) and np.isfinite(head).all()
    assert not head[:, ~mask].any()
    e, T = R.err(head, case.stored(a), mask), case.tolerance(a, prune)
    print(f'K1 {case.name} prune={int(prune)} {a}: error {e:.3e} T {T:.3e} ratio {e / T:.3f}', flush=True)
    assert e <= T, f'{case.name} {a}: {e:.3e} > T = {T:.3e} (x {e / T:.2f}); worst column {int(np.abs(head - case.stored(a))[:, mask].max(0).argmax())}'
    assert not m.mlp_overflowed() and not m.mlp_f8_saturated()
    _check_plans(m, rays, case, a, prune, expect_fit)


# the static 32-sample nets with 11 live columns: hr_frame_plan's 64-ray tiles hold them (tests/test_render_plan_host.py has the rule)
FITS = [n for n in R.GRID if n not in ('skip_last', 'skips_all_depth8', 'out_22', 'out_374', 'out_385', 'out_960_time_group')]


@pytest.mark.parametrize('a', R.ARITHMETICS)
@pytest.mark.parametrize('init', R.INITS)
@pytest.mark.parametrize('name', R.GRID)
def test_head_matches_the_stored_chain(name, init, a, monkeypatch):
    _check_tolerance(name, init, a, True, monkeypatch, expect_fit=name in FITS and a != 'fp32')


@pytest.mark.parametrize('a', R.ARITHMETICS)
@pytest.mark.parametrize('init', R.INITS)
@pytest.mark.parametrize('name', R.N_OUT)
def test_head_matches_the_stored_chain_with_every_column_kept(name, init, a, monkeypatch):
    """HR_PRUNE=0: the other column map -- 15 columns per sample, 30 / 480 / 510 / 525 / 960 head columns (a 480-column static head is
    15 tiles: the frame kernel steps aside)"""
    _check_tolerance(name, init, a, False, monkeypatch)


@pytest.mark.parametrize('init', R.INITS)
@pytest.mark.parametrize('name', R.WIDTHS)
def test_exact_fp32_kernel_at_widths_64_and_128(name, init, monkeypatch):
    case = R.get_case(name, init)
    for a in R.SPLIT:
        with pytest.raises(NotImplementedError):
            case.hc(a)
    _check_tolerance(name, init, 'fp32', True, monkeypatch)


@pytest.mark.parametrize('a', R.ARITHMETICS)
def test_ragged_ray_counts_give_the_first_rows_of_the_full_head(a):
    """1, 63, 64, 65 and 129 rays: a tile's idle rows change nothing in the rows that are there"""
    case = R.get_case('base', 'default')
    m = _model(case, a)
    rays = torch.from_numpy(case.rays).cuda()
    full = _head(m, rays).clone()
    for n in (1, 63, 64, 65, 129):
        assert _bits_equal(_head(m, rays[:n].contiguous()), full[:n]), n


@pytest.mark.parametrize('init', R.INITS)
@pytest.mark.parametrize('name', ['in4', 'in12', 'in20', 'base'])
def test_f16f8_calibrated_on_its_rays_holds_the_tight_bound(name, init):
    """Why T(f16f8) is E_drop / 4 and not / 8 (mlp_reference's docstring): the fp8 exponents come from the calibration rays.  After
    hr_model_calibrate on the rays that are rendered the head holds E_drop / 8 + 8 E_ref32 on the cases that need the wider bound
    (two-plane coordinates as identity columns) as on the base net"""
    case = R.get_case(name, init)
    m = _model(case, 'f16f8')
    rays = torch.from_numpy(case.rays).cuda()
    m.calibrate(rays)
    assert m.mlp_precision_active() == 'f16f8'
    e, T = R.err(_head(m, rays).cpu().numpy(), case.stored('f16f8'), case.live_mask()), case.tight_f16f8()
    print(f'K1cal {case.name} f16f8 calibrated: error {e:.3e} T {T:.3e} ratio {e / T:.3f}', flush=True)
    assert e <= T and not m.mlp_overflowed() and not m.mlp_f8_saturated()


# ---------------------------------------------------------------- exact cases
@pytest.mark.parametrize('a', R.ARITHMETICS)
@pytest.mark.parametrize('skips', R.EXACT_SKIPS)
@pytest.mark.parametrize('depth', R.EXACT_DEPTHS)
def test_integer_nets_come_out_bit_for_bit(depth, skips, a):
    """Inputs no arithmetic rounds (mlp_reference.get_exact_case; the precondition is checked per case on the CPU): every live head value
    equals the float64 chain's, in all five arithmetics.  Values are integers of at most 1023, so scalars repeat: what tells a wrong index
    apart is that at least half of the head's columns differ from every other column as functions of the ray.  The frame kernel does
    not export its head: where it fits, its image has the two-kernel plan's bits."""
    case = R.get_exact_case(depth, skips)
    m = _model(case, a)
    assert m.mlp_precision_active() == a
    rays = torch.from_numpy(case.rays).cuda()
    head = _head(m, rays).cpu().numpy()
    mask = case.live_mask()
    want = case.exact()
    assert not head[:, ~mask].any()
    differ = head[:, mask].astype(F64) != want[:, mask]
    assert not differ.any(), f'{int(differ.sum())} of {differ.size} head values differ, first in column {int(differ.any(0).argmax())}'
    assert len({c.tobytes() for c in head[:, mask].T}) >= int(mask.sum()) / 2
    assert not m.mlp_overflowed()
    _check_plans(m, rays, case, a, True, expect_fit=a != 'fp32' and skips != 'all')


# ---------------------------------------------------------------- the f16f8 kernels' v_sin / v_cos
@pytest.mark.parametrize('a', R.ARITHMETICS)
@pytest.mark.parametrize('init', R.INITS)
def test_windowed_encoding_at_the_fast_sincos_limit(init, a, monkeypatch):
    """four frequencies on Pluecker moments of order 3 (arguments of ~48 rad): 2^4 = 16 is the largest pe_base_mult * freq_mult^n_freqs the
    f16f8 kernels are offered (hr_mlp_fast_sincos_ok), and they hold T(f16f8) there like the IEEE sincosf of the others holds theirs"""
    _check_tolerance('pe_limit_16', init, a, True, monkeypatch, expect_fit=a != 'fp32')


@pytest.mark.parametrize('want', ['auto', 'f16f8', 'f16f8v'])
@pytest.mark.parametrize('init', R.INITS)
def test_f16f8_falls_back_to_f16x3_beyond_the_fast_sincos_limit(init, want):
    """eight frequencies (2^8 = 256, arguments of ~768 rad): `auto` and a forced f16f8 / f16f8v run f16x3 -- IEEE sincosf, no verified
    f16f8 first pass -- and the head holds T(f16x3); the forced modes say so by name when the model is built"""
    import warnings
    case = R.get_case('pe_beyond_256', init)
    if want == 'auto':
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            m = _model(case, want)
    else:
        with pytest.warns(UserWarning, match='runs f16x3'):
            m = _model(case, want)
    assert m.mlp_precision_active() == 'f16x3' and not m.mlp_verified()
    head = _head(m, torch.from_numpy(case.rays).cuda()).cpu().numpy()
    mask = case.live_mask()
    assert not head[:, ~mask].any()
    e, T = R.err(head, case.stored('f16x3'), mask), case.tolerance('f16x3')
    print(f'K1 {case.name} {want} -> f16x3: error {e:.3e} T {T:.3e} ratio {e / T:.3f}', flush=True)
    assert e <= T and not m.mlp_overflowed()


@pytest.mark.parametrize('a', ['fp32', 'bf16x3', 'f16x3'])
@pytest.mark.parametrize('init', R.INITS)
def test_beyond_the_limit_the_ieee_sincos_arithmetics_hold_their_tolerance(init, a, monkeypatch):
    """the same case under the arithmetics whose kernels call sincosf"""
    _check_tolerance('pe_beyond_256', init, a, True, monkeypatch, expect_fit=a != 'fp32')
