"""The keyframe net's time-dependent decode modes without a GPU: csrc/hr_time_decode.h compiled by the host compiler against
a float64 restatement written from the definition (tests/time_decode_oracle.py), hr_plan.h's plan of the time kernel, what
plan.compile_config accepts and refuses, the descriptor's ctypes mirror, the fixtures' conditions, and that scenes.make_state_dict
still draws the scenes it drew for every other mode."""
import ctypes as C
import functools
import glob
import hashlib
import os

import numpy as np
import pytest

import time_decode_oracle as TO
from helpers import GOLDEN_DIR, Golden, build_host_lib
from hyperreel_amd import config as CFG
from hyperreel_amd import plan, scenes

HERE = os.path.dirname(os.path.abspath(__file__))
WHOLE = sorted('time_decode/' + os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, 'time_decode', '*.npz')))      # (gradient fixtures: the grad/ folder below it)
GRID = [28, 24, 20]


@functools.lru_cache(maxsize=None)
def host_lib():
    src = os.path.join(HERE, 'host_math', 'hr_time_decode_host.cpp')
    deps = [src, os.path.join(HERE, '..', 'include', 'hyperreel_hip.h')] + [os.path.join(HERE, '..', 'hyperreel_amd', 'csrc', f)
                                                                           for f in ('hr_time_decode.h', 'hr_plan.h', 'hr_grid.h', 'hr_math.h')]
    lib = C.CDLL(build_host_lib(os.path.join(HERE, 'host_math', '_build', 'libhr_time_decode_host.so'), src, deps))
    i, vp, ll, f = C.c_int, C.c_void_p, C.c_longlong, C.c_float
    lib.td_scale.argtypes, lib.td_scale.restype = [i, i], f
    lib.td_offset.argtypes, lib.td_offset.restype = [vp, f], f
    lib.td_basis.argtypes = [i, i, f, vp, vp, ll, vp]
    lib.td_fold.argtypes = [i, i, f, vp, vp, ll, vp, i, i, vp]
    lib.td_color.argtypes, lib.td_color.restype = [i, f], f
    lib.td_plan.argtypes = [vp, i, ll, i, vp]
    lib.td_sample_lds.argtypes, lib.td_sample_lds.restype = [vp, i], ll
    lib.td_choice.argtypes = [vp, i, vp]
    return lib


def check_case(name, a, recipe):
    """The conditions tools/make_time_decode_golden.py asserted when it wrote the fixture, asserted again on what was read."""
    rgb, rgb64, w = a['rgb'], a['rgb64'], a['render_weights']
    assert not np.isnan(rgb).any() and not np.isnan(rgb64).any(), name
    assert ((rgb > 0.05) & (rgb < 0.95)).mean() >= 0.5, name
    net = recipe['model_cfg']['color']['net']
    live = w > float(net.get('rm_weight_mask_thre', 1e-4))
    assert (~live.any(1)).sum() >= 1 and live.all(1).sum() >= 1, name
    if abs(float(net.get('rm_weight_mask_thre', 1e-4)) - 1e-3) < 1e-9:
        assert 0.1 < live.mean() < 0.9, name
    if net.get('densityMode', 'Density') != 'Density':
        assert (a['sigma_pre'] < 0).mean() >= 0.1 and (a['sigma_pre'] > 0).mean() >= 0.1, name
    assert np.abs(rgb.astype(np.float64) - rgb64).max() <= 2.5e-5, name


def _model(name, **kw):
    cfg, ds = CFG.model_config(name, **kw), CFG.dataset_scalars(name)
    return cfg, ds, plan.compile_model(cfg, ds, GRID)[1]


def _times(seed, n=64):
    """Seeded ray times: t = 0, keyframes exactly (offset 0), both signs of the offset, t close to 1 and 1 itself."""
    rng = np.random.default_rng(seed)
    fac = np.float32(12 * 49 / 50)
    on = (np.arange(12, dtype=np.float32) * np.float32(1.0 / fac)).astype(np.float32)
    t = np.concatenate([[0.0, 1.0, 0.999, 0.97], on, on[1:6] + np.float32(0.03), on[1:6] - np.float32(0.03), rng.random(n).astype(np.float32)])
    return np.ascontiguousarray(t, np.float32)


# ---------------------------------------------------------------- the header against the restatement
@pytest.mark.parametrize('fourier,fpk', [(0, 4), (1, 1), (1, 4), (1, 5), (1, 8)])
def test_basis_fold_and_offsets_equal_the_restatement(fourier, fpk):
    lib = host_lib()
    _, ds, hc = _model('technicolor_z_plane')
    t = _times(fpk)
    off = np.asarray([lib.td_offset(C.addressof(hc), float(v)) for v in t], np.float32)
    want_off = t.astype(np.float64) - TO.base_time(t, ds['num_keyframes'], ds['num_frames'])
    assert np.abs(off - want_off).max() <= 2e-7                     # float32 t - base_t; the keyframes' own offsets are exactly zero
    assert (off[4:16] == 0.0).all() and (off[16:21] > 0).all() and (off[21:26] < 0).all() and off[1] > 0.06
    fac = lib.td_scale(ds['num_keyframes'], ds['num_frames'])
    assert abs(fac - TO.scale(ds['num_keyframes'], ds['num_frames'])) <= 1e-6
    nb = TO.nb(fourier, fpk)
    assert lib.td_nb(fourier, fpk) == nb and lib.td_app_dim(5 if fourier else 4, fpk) == 3 * nb
    got = np.zeros((t.size, nb), np.float32)
    lib.td_basis(fourier, fpk, fac, t.ctypes.data, off.ctypes.data, t.size, got.ctypes.data)
    want = TO.basis(fourier, fpk, t, off, fac)
    # float32 arguments up to 2 pi (fpk - 1) 0.76: their rounding (<= 2e-6 at 33 rad) is the whole difference
    assert np.abs(got - want).max() <= 4e-6
    if fourier:                                                     # the frequency-0 terms: a constant 1 and a constant 0, kept
        assert (got[:, 1] == 1.0).all() and (got[:, 1 + fpk] == 0.0).all() and (got[:, 0] == t).all()
    rng = np.random.default_rng(10 + fpk)
    for groups, cols in ((3, 8), (1, 16)):
        w = ((rng.random((groups * nb, cols), dtype=np.float32) * 2 - 1) / np.float32(np.sqrt(cols))).astype(np.float32)
        out = np.zeros((t.size, groups, cols), np.float32)
        lib.td_fold(fourier, fpk, fac, t.ctypes.data, off.ctypes.data, t.size, w.ctypes.data, groups, cols, out.ctypes.data)
        assert np.abs(out - TO.fold(fourier, fpk, t, off, fac, w)).max() <= 1e-5


def test_activations_and_families():
    lib = host_lib()
    x = np.asarray([-2.0, -0.5, -0.25, 0.0, 0.7], np.float32)
    for shading in (1, 4, 5):                                        # SH, RGBtLinear, RGBtFourier: relu(x + 0.5)
        assert [lib.td_color(shading, float(v)) for v in x] == [0.0, 0.0, 0.25, 0.5, np.float32(1.2)]
    assert [lib.td_color(6, float(v)) for v in x] == [1.5, 0.0, 0.25, 0.5, np.float32(1.2)]      # RGBIdentity: |x + 0.5|
    assert [lib.td_family(s) for s in range(7)] == [0, 4, 0, 0, 7, 7, 2]
    feats = np.random.default_rng(3).standard_normal((5, 27)).astype(np.float32)
    t = np.linspace(0, 1, 5)
    c = TO.colour('RGBtFourier', 4, t, t * 0.01, 11.76, feats)
    assert c.shape == (5, 3) and (c >= 0).all()


# ---------------------------------------------------------------- configuration and ABI
def test_abi_is_additive():
    from hyperreel_amd import lib as L
    lib = host_lib()
    assert L.ABI_VERSION == 27
    assert lib.td_sizeof_config() == C.sizeof(plan.hr_config) == 2144
    assert lib.td_sizeof_desc() == C.sizeof(plan.hr_time_decode) == 12
    assert [n for n, _ in plan.hr_time_decode._fields_] == ['density_mode', 'frames_per_keyframe', 'num_frames']
    assert lib.td_max_fpk() == plan.TIME_MAX_FPK >= 8
    assert (plan.SHADING['RGBtLinear'], plan.SHADING['RGBtFourier'], plan.SHADING['RGBIdentity']) == (4, 5, 6)
    assert plan.DENSITY_MODE == {'Density': 0, 'DensityLinear': 1, 'DensityFourier': 2}
    header = open(os.path.join(HERE, '..', 'include', 'hyperreel_hip.h')).read()
    assert 'HR_SHADING_RGBT_LINEAR = 4, HR_SHADING_RGBT_FOURIER = 5, HR_SHADING_RGB_IDENTITY = 6' in header
    assert 'int hr_model_set_time_decode(hr_model* m, const hr_time_decode* desc);' in header


@pytest.mark.parametrize('name,kw,want', [
    ('technicolor_z_plane', dict(shading='RGBtLinear'), (4, 6, (0, 4, 50))),
    ('technicolor_z_plane', dict(shading='RGBtFourier'), (5, 27, (0, 4, 50))),
    ('technicolor_z_plane', dict(shading='RGBtFourier', frames_per_keyframe=8), (5, 51, (0, 8, 50))),
    ('neural_3d_z_plane', dict(density_mode='DensityLinear'), (1, 27, (1, 4, 50))),
    ('immersive_sphere', dict(shading='RGBtFourier', density_mode='DensityFourier', frames_per_keyframe=2), (5, 15, (2, 2, 50))),
    ('donerf_sphere', dict(shading='RGBIdentity'), (6, 3, None)),
])
def test_plan_accepts_the_five_modes(name, kw, want):
    cfg, ds, hc = _model(name, **kw)
    td = hc.time_decode
    assert (hc.shading, hc.app_dim, None if td is None else (td.density_mode, td.frames_per_keyframe, td.num_frames)) == want
    names = [n for n, _ in plan.upload_names(hc)]
    assert ('basis_mat_density.weight' in names) == (td is not None and td.density_mode != 0)
    assert dict(plan.upload_names(hc)).get('basis_mat_density.weight', 'color_model.net.basis_mat_density.weight') == 'color_model.net.basis_mat_density.weight'
    # 'auto', 'f16f8' and 'f16f8v' resolve to f16x3 in hr_mlp_choice, and only there
    out = (C.c_int * 3)()
    for want in ('auto', 'f16f8', 'f16f8v'):
        hw = plan.compile_model(cfg, ds, GRID, mlp_precision=want)[1]
        assert hw.mlp_precision == plan.MLP_PRECISION[want]
        host_lib().td_choice(C.addressof(hw), int(td is not None and td.density_mode != 0), out)
        assert list(out) == [plan.MLP_PRECISION['f16x3'], 0, 0], want
    sd = scenes.make_state_dict(cfg, ds, GRID, 5, 'dense', 1.0)
    net = 'model.color_model.net.'
    assert sd[net + 'basis_mat.weight'].shape[0] == hc.app_dim
    if td is not None and td.density_mode:
        assert sd[net + 'basis_mat_density.weight'].shape == (TO.nb(td.density_mode == 2, td.frames_per_keyframe), sum(cfg.color.net.n_lamb_sigma))


def test_an_sh_model_with_a_density_mode_still_verifies_nothing():
    """hr_mlp_choice: the density mode alone (not part of hr_config) takes the verified path away; without it the SH model keeps it."""
    _, _, hc = _model('technicolor_z_plane')
    out = (C.c_int * 3)()
    host_lib().td_choice(C.addressof(hc), 0, out)
    assert list(out) == [plan.MLP_PRECISION['f16f8'], 1, 0]
    host_lib().td_choice(C.addressof(hc), 1, out)
    assert list(out) == [plan.MLP_PRECISION['f16x3'], 0, 0]


@pytest.mark.parametrize('name,kw,word', [
    ('technicolor_z_plane', dict(shading='RGBIdentity'), 'RGBIdentity'),
    ('donerf_sphere', dict(shading='RGBtLinear'), 'static net'),
    ('donerf_sphere', dict(shading='RGBtFourier'), 'static net'),
    ('donerf_sphere', dict(density_mode='DensityFourier'), 'static net'),
    ('technicolor_z_plane', dict(shading='RGBtFourier', frames_per_keyframe=plan.TIME_MAX_FPK + 1), 'frames_per_keyframe'),
    ('technicolor_z_plane', dict(density_mode='DensityLinear', frames_per_keyframe=0), 'frames_per_keyframe'),
    ('technicolor_z_plane', dict(shading='MLP_Fea', density_mode='DensityLinear'), 'MLP shading'),
    ('technicolor_z_plane', dict(density_mode='DensityCubic'), 'DensityCubic'),
])
def test_plan_refuses_by_name(name, kw, word):
    cfg, ds = CFG.model_config(name, **kw), CFG.dataset_scalars(name)
    with pytest.raises(NotImplementedError, match=word):
        plan.compile_model(cfg, ds, GRID)


def test_plan_refuses_a_contradicting_data_dim_color():
    cfg, ds = CFG.model_config('technicolor_z_plane', shading='RGBtLinear'), CFG.dataset_scalars('technicolor_z_plane')
    cfg.color.net.data_dim_color = 27
    with pytest.raises(NotImplementedError, match='data_dim_color 27'):
        plan.compile_model(cfg, ds, GRID)
    cfg = CFG.model_config('donerf_sphere', shading='RGBIdentity')
    cfg.color.net.data_dim_color = 27
    with pytest.raises(NotImplementedError, match='data_dim_color 27'):
        plan.compile_model(cfg, CFG.dataset_scalars('donerf_sphere'), GRID)


# ---------------------------------------------------------------- the plan of the time kernel
@pytest.mark.parametrize('name,pclass,slots', [('technicolor_z_plane', 2, 24), ('neural_3d_z_plane', 1, 48), ('immersive_sphere', 1, 48)])
def test_plan_of_the_time_kernel(name, pclass, slots):
    lib = host_lib()
    _, _, hc = _model(name, shading='RGBtFourier', density_mode='DensityFourier')
    p_live = hc.preds_per_z
    base = lib.td_sample_lds(C.addressof(hc), p_live)
    out = np.zeros(11, np.int64)
    lib.td_plan(C.addressof(hc), p_live, 130, 0, out.ctypes.data)
    zp = 64 if 'neural' in name else 32
    rpb = 256 // zp
    assert out[:4].tolist() == [zp, pclass, 0, int(base > 65536)] and out[4] == (130 + rpb - 1) // rpb
    assert out[5] == base and out[6:9].tolist() == [0, 0, 1]          # a decode matrix per ray was always counted; no density row
    lib.td_plan(C.addressof(hc), p_live, 130, 1, out.ctypes.data)
    assert out[6] == slots and out[7] == base // 4 and out[5] == base + 4 * rpb * slots and out[7] % 4 == 0
    assert out[9] == 0 and out[10] == out[5]
    # the generic gather: one weight per density slot
    cfg, ds = CFG.model_config(name, density_mode='DensityLinear'), CFG.dataset_scalars(name)
    cfg.color.net.n_lamb_sigma, cfg.color.net.n_lamb_sh = [10, 4, 3], [10, 4, 3]
    hg = plan.compile_model(cfg, ds, GRID)[1]
    lib.td_plan(C.addressof(hg), hg.preds_per_z, 130, 1, out.ctypes.data)
    assert out[1] == 0 and out[6] == 4 * (3 + 1 + 1) and out[8] == 1           # (SH: a matrix per ray)
    cfg.color.net.n_lamb_sigma, cfg.color.net.n_lamb_sh = [6, 3, 2], [6, 3, 2]  # the classes go by channel groups: [6, 3, 2] is [8, 4, 4]'s
    hg = plan.compile_model(cfg, ds, GRID)[1]
    lib.td_plan(C.addressof(hg), hg.preds_per_z, 130, 1, out.ctypes.data)
    assert out[1] == 1 and out[6] == 48


# ---------------------------------------------------------------- fixtures and scenes
@pytest.mark.parametrize('case', WHOLE)
def test_fixture_conditions(case):
    g = Golden(case)
    check_case(case, g.arrays, g.recipe)
    assert g.rays.shape[0] == 130 and g.rgb.shape == (130, 3)
    if g.rays.shape[1] == 8:                                         # t = 0, a keyframe exactly, both signs, close to 1
        t = g.rays[:, -1]
        off = t.astype(np.float64) - TO.base_time(t, g.dataset['num_keyframes'], g.dataset['num_frames'])
        assert (t == 0).any() and (np.abs(off) < 1e-8).sum() >= 3 and (off > 0.02).any() and (off < -0.02).any() and (t > 0.99).any()
    _ = g.state_dict                                                 # the checksum: the scene regenerates


def test_the_fixtures_cover_what_was_asked():
    rows = {c: Golden(c).state_dict['model.color_model.net.basis_mat.weight'].shape[0] for c in WHOLE if 'rgbt' in c}
    assert {6, 9, 27, 33, 3 * (2 * plan.TIME_MAX_FPK + 1)} <= set(rows.values())
    nets = {c: Golden(c).recipe['model_cfg']['color']['net'] for c in WHOLE}
    assert any(n.get('white_bg') for n in nets.values()) and any(abs(float(n.get('rm_weight_mask_thre', 0)) - 1e-3) < 1e-9 for n in nets.values())
    assert {n.get('densityMode', 'Density') for n in nets.values()} == {'Density', 'DensityLinear', 'DensityFourier'}
    assert {n['shadingMode'] for n in nets.values()} >= {'RGBtLinear', 'RGBtFourier', 'RGBIdentity', 'SH'}
    assert {Golden(c).recipe['model'] for c in WHOLE} >= {'technicolor_z_plane', 'neural_3d_z_plane', 'immersive_sphere', 'donerf_sphere'}


def _digest(sd, keys=None):
    h = hashlib.sha256()
    for k in sorted(sd if keys is None else keys):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()[:32]


# sha256 over the sorted keys and bytes of scenes.make_state_dict(model, scalars, [12, 10, 8], 77, 'dense', 1.0) before the modes existed
PINNED = {'donerf_sphere': (27, 'ffa6a0879d8cd0ab677d0b2357d50ae3', {'basis_mat.weight': '5a9d275d', 'density_plane.0': '9eb0f6af', 'app_line.2': '82881b15'}),
          'technicolor_z_plane': (28, '2ba2be35a000be6722faaa9d42bd578f', {'basis_mat.weight': 'aaed9e47', 'basis_mat_density.weight': '28442df2',
                                                                           'density_plane_time.0': '50a8cd20', 'app_plane_space.0': '45a20546'})}


@pytest.mark.parametrize('name', sorted(PINNED))
def test_make_state_dict_draws_the_existing_modes_as_before(name):
    n, digest, keys = PINNED[name]
    cfg, ds = CFG.model_config(name), CFG.dataset_scalars(name)
    sd = scenes.make_state_dict(cfg, ds, [12, 10, 8], 77, 'dense', 1.0)
    assert len(sd) == n
    for k, d in keys.items():
        assert hashlib.sha256(np.ascontiguousarray(sd['model.color_model.net.' + k]).tobytes()).hexdigest()[:8] == d, k
    assert _digest(sd) == digest
    # a new mode changes only the tensors it reshapes: basis_mat_density is drawn last, over the one-row tensor
    if name == 'technicolor_z_plane':
        cfg2 = CFG.model_config(name, density_mode='DensityFourier')
        sd2 = scenes.make_state_dict(cfg2, ds, [12, 10, 8], 77, 'dense', 1.0)
        same = [k for k in sd if not k.endswith('basis_mat_density.weight')]
        assert sorted(sd2) == sorted(sd) and _digest(sd2, same) == _digest(sd, same)
        assert sd2['model.color_model.net.basis_mat_density.weight'].shape == (9, 8)


def test_the_host_model_takes_the_reference_state_dict_shapes():
    import torch
    from hyperreel_amd.models import HipLightfieldModel
    g = Golden('time_decode/d_technicolor_both_fourier')
    m = HipLightfieldModel(g.cfg, dataset=g.dataset, grid_size=g.grid)
    own = m.state_dict()
    assert tuple(own['color_model.net.basis_mat.weight'].shape) == (27, 8) and tuple(own['color_model.net.basis_mat_density.weight'].shape) == (9, 8)
    sd = {k[len('model.'):]: torch.from_numpy(np.asarray(v)) for k, v in g.state_dict.items()}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and not [k for k in missing if 'dummy_layer' not in k]
    with pytest.raises(NotImplementedError, match='DensityFourier'):          # the density modes stay inference only
        m.train()
        m.forward_train(torch.zeros(4, 8))


def grad_golden(case, white):
    """helpers.GradGolden of tests/golden/time_decode/grad/<case>_bg<white>.npz (tools/make_time_decode_golden.py: the reference's autograd)."""
    from helpers import GradGolden
    return GradGolden(os.path.join('..', 'time_decode', 'grad', case.split('/')[-1]), white)


GRAD_CASES = ['time_decode/a_technicolor_rgbt_linear', 'time_decode/b_technicolor_rgbt_fourier', 'time_decode/g_donerf_rgb_identity']


@functools.lru_cache(maxsize=None)
def train_time_lib():
    src = os.path.join(HERE, 'host_math', 'hr_train_time_host.cpp')
    deps = [src, os.path.join(HERE, '..', 'include', 'hyperreel_hip.h')] + [os.path.join(HERE, '..', 'hyperreel_amd', 'csrc', f)
                                                                           for f in ('hr_train.h', 'hr_time_decode.h', 'hr_mask.h', 'hr_plan.h', 'hr_grid.h', 'hr_math.h')]
    lib = C.CDLL(build_host_lib(os.path.join(HERE, 'host_math', '_build', 'libhr_train_time_host.so'), src, deps))
    lib.htt_unsupported.restype = C.c_char_p
    return lib


def _scene(g):
    return scenes.carve_half_space(scenes.scale_density(g.state_dict, g.recipe.get('density_scale', 1.0)), g.recipe['carve_x'])


@pytest.mark.parametrize('white', [0, 1])
@pytest.mark.parametrize('case', GRAD_CASES + ['time_decode/b_technicolor_rgbt_fourier_fpk5'])
def test_host_training_gradients_match_autograd_of_the_restatement(case, white):
    """csrc/hr_train.h as train_time_kernel.hip compiles it (HR_TRAIN_TIME; phases A, B, C per ray) against torch.autograd on the
    restatement (time_decode_oracle.time_port: TorchPort up to the weights, the colour from the definition).  Bars: test_train_host.py's."""
    import torch
    from test_train_host import FP, pack_grids
    htt = train_time_lib()
    g = Golden(case)
    _, hc = plan.compile_model(g.cfg, g.dataset, g.grid)
    assert htt.htt_unsupported(C.byref(hc)) is None and htt.htt_nbv(C.byref(hc)) == hc.app_dim // 3
    port = TO.time_port(g.cfg, g.dataset, _scene(g))
    rays = torch.from_numpy(np.ascontiguousarray(g.rays, np.float32))
    n = rays.shape[0]
    grids = [t for grp in (port.d_a, port.d_b, port.a_a, port.a_b) for t in grp]
    leaves = grids + [port.basis]
    for t in leaves:
        t.requires_grad_(True)
    with torch.no_grad():
        head0 = port._mlp(port._param_pe(rays))
    head = head0.clone().requires_grad_(True)
    rgb_ref = port.color(port.embed(rays, head=head), rays, train=True, white_bg=bool(white))
    G = torch.randn(rgb_ref.shape, generator=torch.Generator().manual_seed(3))
    (rgb_ref * G).sum().backward()
    assert bool(torch.isfinite(head.grad).all())
    # the restatement itself against the reference's own train-mode forward and basis_mat gradient, where a gradient fixture exists
    if case in GRAD_CASES:
        gg = grad_golden(case, white)
        assert np.abs(rgb_ref.detach().numpy() - gg.rgb).max() <= 2e-5

    planes, packed, ca_total = pack_grids(port, hc)
    gbuf = [(np.zeros_like(pa), np.zeros_like(pb)) for pa, pb, *_ in packed]
    g_a = (FP * 3)(*[b[0].ctypes.data_as(FP) for b in gbuf])
    g_b = (FP * 3)(*[b[1].ctypes.data_as(FP) for b in gbuf])
    basis = np.ascontiguousarray(port.basis.detach().numpy())
    d_basis = np.zeros_like(basis)
    rgb = np.zeros((n, 3), np.float32)
    d_head = np.zeros_like(head0.numpy())
    hnp, rnp, Gnp = np.ascontiguousarray(head0.numpy()), np.ascontiguousarray(rays.numpy()), np.ascontiguousarray(G.numpy())
    f = lambda a: a.ctypes.data_as(FP)
    assert htt.htt_train(C.byref(hc), f(rnp), f(hnp), C.c_longlong(n), f(Gnp), f(rgb), f(d_head), planes, g_a, g_b, f(basis), f(d_basis),
                         basis.shape[1], ca_total, white) == 0

    def close(got, ref, what):
        ref = np.asarray(ref, np.float64)
        scale = np.abs(ref).max()
        err = np.abs(np.asarray(got, np.float64) - ref).max()
        assert scale > 0, f'{what}: reference gradient is identically zero'
        assert err <= 2e-4 * scale + 1e-7, f'{what}: |err| {err:.3e} vs scale {scale:.3e}'

    ref_np = rgb_ref.detach().numpy()
    assert (np.abs(rgb - ref_np) <= 1e-5 * np.maximum(1.0, np.abs(ref_np))).all()          # the forward has no clamp
    close(d_head, head.grad.numpy(), 'd head')
    close(d_basis, port.basis.grad.numpy(), 'd basis_mat')
    for j, (pa, pb, nd, na, aoff) in enumerate(packed):
        ga, gb = gbuf[j]
        for name, got, ref_t, cnt, off in (('density a', ga, port.d_a[j], nd, 0), ('density b', gb, port.d_b[j], nd, 0),
                                           ('app a', ga, port.a_a[j], na, aoff), ('app b', gb, port.a_b[j], na, aoff)):
            if cnt:
                close(got[..., off:off + cnt], ref_t.grad.numpy()[0][:cnt].transpose(1, 2, 0), f'{name} {j}')
