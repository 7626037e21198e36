"""hyperreel_amd.train.HipTensoRFRegularizer's host side -- the reference's schedule (nlf/regularizers/base.py:146-168,
nlf/regularizers/tensorf.py:57-96) -- against tests/golden/reg: the reference's own regulariser on the reference's own nets
(tools/make_reg_golden.py).  No device: the model is built on the CPU and only set_iter(), the three weights and terms() are read."""
import numpy as np
import pytest
import torch

import reg_common as R


def _regularizer(f):
    from hyperreel_amd.render import build_render_fn
    from hyperreel_amd.train import HipTensoRFRegularizer
    fn = build_render_fn(f.cfg, dataset=f.dataset, grid_size=f.recipe['grid'], device='cpu')
    missing, unexpected = fn.model.load_state_dict({k: torch.from_numpy(v) for k, v in f.state_dict.items()}, strict=False)
    assert not [m for m in missing if 'dummy_layer' not in m] and not unexpected
    return fn.model, HipTensoRFRegularizer(fn.model, f.recipe['reg'], f.recipe['steps_per_epoch'])


def _bar(f):
    """4 x the largest relative distance, over the case's iterations, between the reference's float32 value and the same module's value
    on a float64 copy of the net: how far one correct float32 evaluation order lies from the exact value."""
    dev = [abs(float(f.arrays[f'it{i}/loss32']) - float(f.arrays[f'it{i}/loss64'])) / abs(float(f.arrays[f'it{i}/loss64']))
           for i in f.iterations if float(f.arrays[f'it{i}/loss64']) != 0.0]
    assert dev and max(dev) > 0.0
    return 4.0 * max(dev), max(dev)


@pytest.mark.parametrize('name', R.CASES)
def test_the_three_weights_reproduce_the_reference_value_at_every_recorded_iteration(name):
    """value(i) = sum over terms() of weights[slot] * k * S, with S the unweighted sums of squared differences / of |x| taken with torch
    in float64 on the CPU from the fixture's scene, weights = set_iter(i)'s three Python floats (loss_weight() and the double count of
    the density TV folded in) and k the static factors of terms() as the host forms them (doubles; the device receives their float32
    roundings).  Held to the reference's float32 value within 4 x the reference's own float32-vs-float64 distance.

    Measured (torch 2.x CPU, one thread), max over iterations of |loss32 - loss64| / |loss64|: static_decay 9.80e-8, video_no_app
    9.61e-8, static_n_lamb_800 1.81e-7, video_wait_stop 8.88e-8 -- bars of 3.6e-7 ... 7.3e-7; the values formed here lie within 3e-16
    (relative) of loss64, so their distance from loss32 is the reference's own."""
    f = R.fixture(name)
    model, reg = _regularizer(f)
    bar, measured = _bar(f)
    for i in f.iterations:
        reg.set_iter(i)
        total = 0.0
        for p, kh, kw, kl, sh, sw, sl in reg.terms():
            x = p.detach().double()
            if x.shape[1] == 0:
                continue
            if sh >= 0:
                total += reg.weights[sh] * kh * float(torch.pow(x[:, :, 1:, :] - x[:, :, :-1, :], 2).sum())
            if sw >= 0:
                total += reg.weights[sw] * kw * float(torch.pow(x[:, :, :, 1:] - x[:, :, :, :-1], 2).sum())
            if sl >= 0:
                total += reg.weights[sl] * kl * float(x.abs().sum())
        l32, l64 = float(f.arrays[f'it{i}/loss32']), float(f.arrays[f'it{i}/loss64'])
        print(f'{name} iteration {i}: weights {reg.weights}, value {total:.9e}, reference float32 {l32:.9e} float64 {l64:.9e}, '
              f'|value - float32| / |float64| {abs(total - l32) / abs(l64) if l64 else 0.0:.3e} (bar {bar:.3e}, measured {measured:.3e})')
        assert abs(total - l32) <= bar * abs(l64), (name, i)
        assert reg.warming_up() == bool(f.arrays[f'it{i}/warming_up']), (name, i)


@pytest.mark.parametrize('name', R.CASES)
def test_the_terms_are_the_nets_own_three_methods(name):
    """terms() lists the tensors density_L1 / TV_loss_density / TV_loss_app read, with their skip rules and static factors: with unit
    weights it reproduces the three methods written as the reference writes them (reg_common.reference_terms), in float64."""
    f = R.fixture(name)
    model, reg = _regularizer(f)
    net = model.color_model.net
    want = [float(v) for v in R.reference_terms([[p.detach().double() for p in grp] for grp in net._reg_planes()], net.video)]
    got = [0.0, 0.0, 0.0]
    for p, kh, kw, kl, sh, sw, sl in reg.terms():
        x = p.detach().double()
        if x.shape[1] == 0:
            continue
        if sh >= 0:
            got[sh] += kh * float(torch.pow(x[:, :, 1:, :] - x[:, :, :-1, :], 2).sum())
        if sw >= 0:
            got[sw] += kw * float(torch.pow(x[:, :, :, 1:] - x[:, :, :, :-1], 2).sum())
        if sl >= 0:
            got[sl] += kl * float(x.abs().sum())
    assert len(reg.terms()) <= 12
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0.0)


def test_app_tv_without_density_tv_is_refused_where_the_reference_raises_name_error():
    from hyperreel_amd.train import HipTensoRFRegularizer
    f = R.fixture(R.CASES[0])
    for tvd in (0.0, -1.0):
        with pytest.raises(ValueError, match='NameError'):
            HipTensoRFRegularizer(None, dict(f.recipe['reg'], TV_weight_density=tvd, TV_weight_app=0.0125), 50)
    HipTensoRFRegularizer(None, dict(f.recipe['reg'], TV_weight_density=0.0, TV_weight_app=0.0), 50)      # no TV at all is the reference's L1-only run


def test_the_schedule_is_the_references():
    """The pieces of set_iter on their own, against the reference's expressions evaluated here."""
    from hyperreel_amd.train import HipTensoRFRegularizer
    cfg = dict(R.fixture('static_decay').recipe['reg'], wait_iters=3, stop_iters=100, warmup_iters=2)
    reg = HipTensoRFRegularizer(None, cfg, 50)
    reg.set_iter(2)
    assert reg.cur_iter == -1 and reg.weights == (0.0, 0.0, 0.0) and reg.warming_up()
    reg.set_iter(13)
    lw = 1.0 * np.power(0.5, 10 / (1 * 50))
    assert reg.loss_weight() == lw and not reg.warming_up()
    assert reg.weights == (8e-5 * lw, (0.0125 + 0.0125) * lw, 0.0125 * lw)
    reg.set_iter(43)                                         # cur_iter == update_AlphaMask_list[0]: the switch, which stays
    assert reg.weights[0] == 4e-5 * (1.0 * np.power(0.5, 40 / 50))
    reg.set_iter(63)
    assert reg.weights[1] > 0
    reg.set_iter(64)                                         # cur_iter 61 > total_num_tv_iters 60
    assert reg.weights[0] == 4e-5 * (1.0 * np.power(0.5, 61 / 50)) and reg.weights[1:] == (0.0, 0.0)
    reg.set_iter(103)                                        # cur_iter == stop_iters
    assert reg.weights == (0.0, 0.0, 0.0)
    derived = HipTensoRFRegularizer(None, {k: v for k, v in dict(cfg, n_iters=30).items() if k != 'total_num_tv_iters'}, 50)
    assert derived.total_num_tv_iters == 120
