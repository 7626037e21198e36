"""hr_stage_shade -- the per-sample colour network of shadingMode MLP_Fea / MLP alone (csrc/shade_kernel.hip) -- against the
reference's own modules on seeded rows (tests/golden/shading/unit_*.npz, tools/make_shading_golden.py).  `-m gpu` only.

Bar: 4 x the fixture's own max |rgb32 - rgb64| (how far the reference's float32 evaluation lies from the exact value), floor 1e-6: the
kernel sums up to 390 exact fp32 products per output in another order than torch's GEMM."""
import numpy as np
import pytest
import torch

import shading_oracle as SO
from test_shade_host import UNITS, load_unit, unit_weights

pytestmark = pytest.mark.gpu

GRID = [12, 10, 8]


def make_model(mode, view_pe, fea_pe, c, weights=None):
    """A donerf_sphere model with the given colour network (its other tensors: a seeded scene) -> (render fn, native handle)."""
    from gpu_common import make_render_fn
    from hyperreel_amd import config as CFG
    from hyperreel_amd import scenes
    cfg, ds = CFG.model_config('donerf_sphere'), CFG.dataset_scalars('donerf_sphere')
    net = cfg.color.net
    net.shadingMode, net.data_dim_color, net.view_pe, net.fea_pe, net.featureC = mode, 27, view_pe, fea_pe, c
    sd = scenes.make_state_dict(cfg, ds, GRID, seed=3)
    for k, v in (weights or {}).items():
        sd['model.color_model.net.renderModule.' + k] = np.ascontiguousarray(v, np.float32)
    fn = make_render_fn(cfg, ds, sd)
    return fn, fn.model.native()


def stage_shade(fn, handle, f, v):
    from hyperreel_amd import lib as L
    f = torch.from_numpy(np.ascontiguousarray(f, np.float32)).cuda()
    v = torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()
    rgb = torch.full((f.shape[0], 3), float('nan'), device='cuda')
    L.call('hr_stage_shade', handle, f, v, f.shape[0], rgb, L.stream(f.device), device=f.device)
    torch.cuda.synchronize()
    return rgb.cpu().numpy()


@pytest.fixture(scope='module')
def models():
    cache = {}

    def get(name):
        if name not in cache:
            a, recipe = load_unit(name)
            cache[name] = (a, make_model(*SO.unit_descriptor(recipe), unit_weights(a)))
        return cache[name]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


MEASURED = {}


@pytest.mark.parametrize('name', UNITS)
def test_unit_fixture_within_the_bar(models, name):
    a, (fn, h) = models(name)
    got = stage_shade(fn, h, a['f'], a['v'])
    err = float(np.abs(got - a['rgb64']).max())
    own = float(np.abs(a['rgb'].astype(np.float64) - a['rgb64']).max())
    MEASURED[name] = err
    print(f'{name}: max |rgb - rgb64| {err:.3e} (the reference\'s float32: {own:.3e})')
    assert np.isfinite(got).all()
    assert err <= max(1e-6, 4 * own), f'{name}: {err:.3e} against {max(1e-6, 4 * own):.3e}'


@pytest.mark.parametrize('n', [1, 63, 64, 65, 300])
@pytest.mark.parametrize('name', ['unit_fea_default', 'unit_fea_c40', 'unit_mlp_pe0'])
def test_partial_and_multiple_tiles(models, name, n):
    """A row's colour depends on nothing but the row: every size gives the bits of the 300-row launch, and writes nothing past n."""
    a, (fn, h) = models(name)
    full = stage_shade(fn, h, a['f'], a['v'])
    got = stage_shade(fn, h, a['f'][:n], a['v'][:n])
    assert np.array_equal(got, full[:n])
    from hyperreel_amd import lib as L
    f, v = (torch.from_numpy(np.ascontiguousarray(a[k][:n], np.float32)).cuda() for k in ('f', 'v'))
    out = torch.full((n + 64, 3), 7.0, device='cuda')
    L.call('hr_stage_shade', h, f, v, n, out, L.stream(f.device), device=f.device)
    torch.cuda.synchronize()
    assert torch.all(out[n:] == 7.0) and np.array_equal(out[:n].cpu().numpy(), full[:n])


def test_two_runs_same_bits(models):
    a, (fn, h) = models('unit_fea_default')
    assert np.array_equal(stage_shade(fn, h, a['f'], a['v']), stage_shade(fn, h, a['f'], a['v']))


def test_integer_network_is_exact():
    """The device packer and the three GEMMs on integers (no positional encoding: MLP, view_pe 0): every product and sum is exact in
    fp32, so the value before the sigmoid is THE integer the weights define times 2^-s -- a weight or an input column in the wrong
    place changes it."""
    rng = np.random.default_rng(11)
    c, n = 64, 130
    f = rng.integers(-4, 5, (n, 27)).astype(np.float32)
    v = rng.integers(-1, 2, (n, 3)).astype(np.float32)
    w0, b0 = rng.integers(-1, 2, (c, 30)), rng.integers(-3, 4, c)
    w1, b1 = rng.integers(-1, 2, (c, c)) * (rng.random((c, c)) < 0.25), rng.integers(-3, 4, c)
    w2 = rng.integers(-2, 3, (3, c))
    x = np.concatenate([f, v], 1).astype(np.int64)
    h = np.maximum(x @ w0.T + b0, 0)
    h = np.maximum(h @ w1.T + b1, 0)
    o = h @ w2.T
    assert np.abs(o).max() < 2 ** 24
    s = int(np.ceil(np.log2(np.abs(o).max() / 8.0)))              # |o| 2^-s <= 8: the sigmoid stays informative
    weights = {'mlp.0.weight': w0, 'mlp.0.bias': b0, 'mlp.2.weight': w1, 'mlp.2.bias': b1, 'mlp.4.weight': w2 * 2.0 ** -s, 'mlp.4.bias': np.zeros(3)}
    fn, hdl = make_model('MLP', 0, 0, c, weights)
    got = stage_shade(fn, hdl, f, v)
    want = 1.0 / (1.0 + np.exp(-(o * 2.0 ** -s)))
    assert ((want > 0.05) & (want < 0.95)).mean() > 0.3
    assert np.abs(got - want).max() <= 2e-7                       # one float32 rounding of exp and of the quotient; a unit of o is 2^-s >> that


def test_one_hot_routes_every_encoded_column():
    """MLP_Fea with fea_pe = view_pe = 1 (90 columns) and 256 hidden units: hidden units 2 j and 2 j + 1 carry +x_j and -x_j through
    both ReLUs (identity second Linear), the last Linear returns x_j = h[2 j] - h[2 j + 1] for three columns at a time."""
    rng = np.random.default_rng(12)
    n, k0, c = 65, 90, 256
    f = (rng.integers(-16, 17, (n, 27)) / 4.0).astype(np.float32)
    v = (rng.integers(-4, 5, (n, 3)) / 4.0).astype(np.float32)
    x = SO.encode('MLP_Fea', 1, 1, torch.from_numpy(f).double(), torch.from_numpy(v).double()).numpy()
    w0 = np.zeros((c, k0), np.float32)
    w0[2 * np.arange(k0), np.arange(k0)] = 1.0
    w0[2 * np.arange(k0) + 1, np.arange(k0)] = -1.0
    weights = {'mlp.0.weight': w0, 'mlp.0.bias': np.zeros(c), 'mlp.2.weight': np.eye(c), 'mlp.2.bias': np.zeros(c),
               'mlp.4.weight': np.zeros((3, c)), 'mlp.4.bias': np.zeros(3)}
    fn, hdl = make_model('MLP_Fea', 1, 1, c, weights)
    last = fn.model.color_model.net.renderModule.mlp[4].weight
    worst = 0.0
    for j0 in range(0, k0, 3):
        w2 = torch.zeros(3, c)
        for ch in range(3):
            w2[ch, 2 * (j0 + ch)], w2[ch, 2 * (j0 + ch) + 1] = 1.0, -1.0
        with torch.no_grad():
            last.copy_(w2.to(last.device))
        got = stage_shade(fn, fn.model.native(), f, v)
        want = 1.0 / (1.0 + np.exp(-x[:, j0:j0 + 3]))
        worst = max(worst, float(np.abs(got - want).max()))
    # raw columns are exact, sin / cos within a float32 rounding or two of the float64 values; neighbouring columns differ by far more
    assert worst <= 4e-7, worst
