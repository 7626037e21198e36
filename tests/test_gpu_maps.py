"""Per-ray depth, expected-point and opacity maps (hr_render_maps / hr_render_frame_maps, HipLightfieldModel.render(maps=...)).

The maps are the reference's fields=['distances', 'points'] -- sum_k w_k x[key]_k, tensorf_no_sample.py:254-278 -- and its
acc_map sum_k w_k (:232), written by the sample kernel in the launches that write the image.  Checked here:
  * the image is bit for bit the one without maps, on every family, arithmetic and plan (hr_render, hr_render_frame, cascades);
  * the maps against the reference's formula applied to its own per-sample values (goldens, or the CPU oracle);
  * the maps against torch sums over the diagnostics path's per-sample outputs (same values, another order of summation);
  * the verified fast path repairs the maps of the rays it re-renders, in every slice of its list;
  * million-ray calls, the reference's chunking, hipGraph replay, the frame-kernel option, the C ABI's edge cases, fast_fields.
`-m gpu` only."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from helpers import Golden
from hyperreel_amd import config as HC
from hyperreel_amd import lib as _lib
from hyperreel_amd import scenes
from hyperreel_amd.plan import hr_maps

pytestmark = pytest.mark.gpu

ALL = ('distances', 'points', 'acc')
KEYFRAME = ('technicolor', 'neural_3d', 'immersive')
GOLDEN_CASES = ['donerf_sphere_600', 'technicolor_full', 'immersive_full', 'neural_3d_full',
                'donerf_sphere_hostile', 'technicolor_hostile', 'immersive_hostile', 'neural_3d_hostile',
                'donerf_sphere_stiff', 'technicolor_stiff', 'immersive_stiff', 'neural_3d_stiff',
                'neural_3d_z_plane_small']
SMALL_CASES = ['donerf_sphere_small', 'donerf_cylinder_small', 'immersive_sphere_small', 'technicolor_z_plane_small',
               'neural_3d_z_plane_small']
CASCADES = ['sweep/technicolor_cascaded', 'sweep/shiny_z_plane_feedback']


def _emb(cfg):
    return cfg.embedding.embeddings


def _variant(name, edit, Z=None):
    cfg = HC.model_config(name, z_channels=Z)
    edit(cfg)
    return cfg


# the oracle-checked variants of test_gpu_parity.py that reach the maps' other code paths, rebuilt the same way
VARIANTS = {
    'static_sh_softplus_white': ('donerf', lambda: _variant('donerf_sphere', lambda c: c.color.net.update(
        white_bg=1, fea2denseAct='softplus', density_shift=-1.0, shadingMode='SH', data_dim_color=27))),
    'video_rgb_unsorted_thr': ('immersive', lambda: _variant('immersive_sphere', lambda c: (
        c.color.net.update(shadingMode='RGB', data_dim_color=3, rm_weight_mask_thre=1e-3),
        _emb(c).ray_intersect_0.intersect.update(sort=False)))),
    'z128_zplane': ('technicolor', lambda: _variant('technicolor_z_plane', lambda c: None, Z=128)),
    'z256_video_sphere': ('immersive', lambda: _variant('immersive_sphere', lambda c: None, Z=256)),
    'hidden128': ('donerf', lambda: _variant('donerf_cylinder', lambda c: _emb(c).ray_prediction_0.net.update(hidden_channels=128))),
}


class _Case:
    """cfg, dataset, weights, rays and (lazily) one model per arithmetic of a fixture."""

    def __init__(self, name, density='dense'):
        self.name = name
        self.iteration = None
        if name in VARIANTS:
            base, make = VARIANTS[name]
            self.cfg = make()
            self.ds = HC.dataset_scalars(base)
            self.sd = scenes.make_state_dict(self.cfg, self.ds, [33, 27, 30], seed=321, density=density, app_scale=1.0)
            video = self.cfg.color.net.type == 'tensor_vm_split_time'
            zp = _emb(self.cfg).ray_intersect_0.intersect.type == 'z_plane'
            self.rays = scenes.random_rays(515, 6, video, pos_mean=(0, 0, 1.0), pos_std=0.15, dir_mean=(0, 0, -1.2), dir_std=0.5) if zp \
                else scenes.random_rays(515, 6, video)
            self.golden = None
        else:
            g = Golden(name)
            self.golden = g
            self.cfg, self.ds, self.sd, self.iteration = g.cfg, g.dataset, g.state_dict, g.iteration
            self.rays = g.rays
            if name in CASCADES:
                self.rays = scenes.random_rays(515, 9, g.rays.shape[1] == 8, pos_mean=(0, 0, 1.0), pos_std=0.15, dir_mean=(0, 0, -1.2), dir_std=0.5)
        self.rays = np.ascontiguousarray(self.rays, np.float32)
        self.models = {}

    @property
    def keyframe(self):
        return self.cfg.color.net.type == 'tensor_vm_split_time' and self.rays.shape[1] == 8

    def model(self, precision, **kw):
        key = (precision, tuple(sorted(kw.items())))
        if key not in self.models:
            from gpu_common import to_torch_state_dict
            from hyperreel_amd.render import build_render_fn
            grid = [int(v) for v in self.sd['model.color_model.net.gridSize']]
            fn = build_render_fn(self.cfg, dataset=self.ds, grid_size=grid, mlp_precision=precision, **kw)
            fn.model.load_state_dict(to_torch_state_dict(self.sd), strict=False)
            if self.iteration is not None:
                fn.model.set_iter(self.iteration)
            self.models[key] = fn
        return self.models[key].model


_cases = {}


def _case(name, density='dense'):
    if (name, density) not in _cases:
        _cases.clear()
        torch.cuda.empty_cache()
        _cases[(name, density)] = _Case(name, density)
    return _cases[(name, density)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _tuple_bits(r):
    return torch.cat([_bits(r['rgb']), _bits(r['distances']), _bits(r['points']), _bits(r['acc'])], -1)


def _reference_maps(d, p, w):
    """The reference's formula on per-sample arrays d (B,Z), p (B,Z,3), w (B,Z), in float64, and the tolerance of each map entry from
    the per-sample tolerances of test_gpu_parity.py (5e-5 absolute on weights, 2e-5 relative on distances and points)."""
    d, p, w = (np.asarray(v, np.float64) for v in (d, p, w))
    B, Z = w.shape
    p = p.reshape(B, Z, 3)
    depth = (w * d).sum(-1, keepdims=True)
    pts = (w[..., None] * p).sum(1)
    acc = w.sum(-1, keepdims=True)
    tol_d = 5e-5 * np.abs(d).sum(-1, keepdims=True) + 2e-5 * (w * (1.0 + np.abs(d))).sum(-1, keepdims=True)
    tol_p = 5e-5 * np.abs(p).sum(1) + 2e-5 * (w[..., None] * (1.0 + np.abs(p))).sum(1)
    return (depth, pts, acc), (tol_d, tol_p, np.full_like(acc, Z * 5e-5))


def _check_against(name, got, ref, tol):
    worst = []
    for k, r, t in zip(ALL, ref, tol):
        g = got[k].cpu().numpy().astype(np.float64)
        err = np.abs(g - r)
        t = np.maximum(t, 1e-30)                     # a ray with no weight and no distance: its maps must be exact
        assert bool(np.all(np.isfinite(g))), f'{name} {k}: non-finite map entries'
        ratio = float((err / t).max())
        worst.append(f'{k} {float(err.max()):.2e} (worst err/bound {ratio:.2f})')
        assert ratio <= 1.0, f'{name} {k}: |err| {float(err[np.argmax(err / t)]):.3e} over its bound {float(t.flat[np.argmax(err / t)]):.3e}'
    print(f'{name}: ' + ', '.join(worst))


def _diag_check(name, m, rays):
    """Maps against torch sums over hr_render_fields' per-sample outputs of the same model (the safe tier: f16x3 / fp32)."""
    r = m.render(rays, maps=ALL)
    f = m.render(rays, want=('distances', 'points', 'render_weights'))
    torch.cuda.synchronize()
    assert torch.equal(r['rgb'], f['rgb']), f'{name}: the maps call and the diagnostics call render different images'
    w, d = f['render_weights'].double(), f['distances'].double()
    B, Z = w.shape
    p = f['points'].double().reshape(B, Z, 3)
    bound = 1e-6 * (1.0 + (w * d.abs()).sum(-1))
    for k, want in (('distances', (w * d).sum(-1, keepdim=True)), ('points', (w[..., None] * p).sum(1)), ('acc', w.sum(-1, keepdim=True))):
        err = (r[k].double() - want).abs().amax(-1)
        assert bool((err <= bound).all()), f'{name} {k}: {float(err.max()):.3e} from the diagnostics path\'s sums'


def _image_cases():
    # forced f16f8 where test_gpu_f16f8.py runs it (initialiser-scale fixtures); the exact-fp32 variant has no split kernels; the cascades
    # in the arithmetics of test_gpu_parity.py's cascade test
    out = []
    for c in GOLDEN_CASES + sorted(VARIANTS) + CASCADES:
        for p in ('auto', 'f16f8', 'f16x3', 'fp32'):
            if p == 'f16f8' and (c.endswith(('_hostile', '_stiff')) or c in CASCADES or c == 'hidden128'):
                continue
            if p == 'f16x3' and c == 'hidden128':
                continue
            out.append((c, p))
    return out


# ---- 1 + 3. the image does not change; the maps equal the diagnostics path's sums
@pytest.mark.parametrize('case,precision', _image_cases())
def test_maps_leave_the_image_unchanged(case, precision):
    c = _case(case)
    m = c.model(precision)
    rays = torch.from_numpy(c.rays).cuda()
    plain = m.render(rays)['rgb'].clone()
    r = m.render(rays, maps=ALL)
    torch.cuda.synchronize()
    assert torch.equal(_bits(r['rgb']), _bits(plain)), f'{case} {precision}: {int((r["rgb"] != plain).any(-1).sum())} pixels changed'
    assert r['distances'].shape == (rays.shape[0], 1) and r['points'].shape == (rays.shape[0], 3) and r['acc'].shape == (rays.shape[0], 1)
    assert bool(torch.isfinite(r['distances']).all() and torch.isfinite(r['points']).all() and torch.isfinite(r['acc']).all())
    if c.keyframe and case not in CASCADES:
        t = float(c.rays[0, -1])
        pf = m.render(rays, frame_time=t)['rgb'].clone()
        rf = m.render(rays, frame_time=t, maps=ALL)
        torch.cuda.synchronize()
        assert torch.equal(_bits(rf['rgb']), _bits(pf)), f'{case} {precision}: hr_render_frame_maps changed the frame\'s image'
        assert torch.equal(rf['acc'].isfinite(), torch.ones_like(rf['acc'], dtype=torch.bool))
    if precision == ('fp32' if case == 'hidden128' else 'f16x3'):
        _diag_check(f'{case} {precision}', m, rays)


@pytest.mark.parametrize('case', ['z128_zplane', 'z256_video_sphere'])
def test_every_wavefront_of_a_long_ray_adds_to_its_maps(case):
    """ZP > 64: a ray spans 2 or 4 wavefronts whose partial sums meet in LDS.  On a thin scene every wavefront's samples carry weight, so
    a partial sum that went missing moves the maps far beyond the diagnostics path's bound."""
    c = _case(case, density='thin')
    m = c.model('f16x3')
    rays = torch.from_numpy(c.rays).cuda()
    f = m.render(rays, want=('render_weights',))
    torch.cuda.synchronize()
    w = f['render_weights']
    B, Z = w.shape
    per_wave = w.view(B, Z // 64, 64).sum(-1).amax(0)
    assert bool((per_wave > 1e-3).all()), f'{case}: a wavefront carries no weight ({per_wave.tolist()}): the test would be vacuous'
    _diag_check(f'{case} thin f16x3', m, rays)


# ---- 2. against the reference's own numbers
@pytest.mark.parametrize('precision', ['auto', 'f16x3', 'fp32'])
@pytest.mark.parametrize('case', SMALL_CASES)
def test_maps_match_the_reference_formula_on_its_goldens(case, precision):
    c = _case(case)
    g = c.golden
    got = c.model(precision).render(torch.from_numpy(c.rays).cuda(), maps=ALL)
    torch.cuda.synchronize()
    Z = g.arrays['render_weights'].shape[1]
    if case.startswith('neural_3d'):
        assert Z == 64
    ref, tol = _reference_maps(g.arrays['distances'].reshape(-1, Z), g.arrays['points'], g.arrays['render_weights'])
    _check_against(f'{case} {precision}', got, ref, tol)


ORACLE_CASES = ['donerf_sphere_600', 'technicolor_full', 'immersive_full', 'neural_3d_full', 'donerf_sphere_hostile', 'technicolor_hostile',
                'immersive_hostile', 'neural_3d_hostile'] + sorted(VARIANTS) + CASCADES


@pytest.mark.parametrize('case,precision', [(c, p) for c in ORACLE_CASES for p in ('auto', 'fp32' if c == 'hidden128' else 'f16x3')])
def test_maps_match_the_cpu_oracle(case, precision):
    from hyperreel_oracle import HyperReelOracle
    c = _case(case)
    rays = c.rays[:1024]
    got = c.model(precision).render(torch.from_numpy(rays).cuda(), maps=ALL)
    torch.cuda.synchronize()
    ref = HyperReelOracle(c.cfg, c.ds, c.sd, iteration=c.iteration).render(rays, keep=('distances', 'points', 'render_weights'))
    w = ref['render_weights']
    Z = w.shape[1]
    ref_maps, tol = _reference_maps(ref['distances'].reshape(-1, Z), ref['points'], w)
    _check_against(f'{case} {precision}', got, ref_maps, tol)


# ---- 4. the verified fast path repairs the maps of the rays it re-renders
def _three(model, H, W):
    cfg, ds = HC.model_config(model), HC.dataset_scalars(model)
    sd = scenes.make_state_dict(cfg, ds, None, seed=7, density='dense', app_scale=1.0)
    from gpu_common import make_render_fn
    return {p: make_render_fn(cfg, ds, sd, mlp_precision=p).model for p in ('auto', 'f16f8', 'f16x3')}, scenes.benchmark_rays(model, H, W, frame=7)


def _check_repaired(what, ms, rays, expect_slices=False):
    out = {p: ms[p].render(rays, maps=ALL) for p in ms}
    torch.cuda.synchronize()
    auto = ms['auto']
    n_redo = auto.redo_count()
    assert auto.mlp_verified() and n_redo > 0 and not auto.redo_overflowed(), (n_redo, auto.redo_overflowed())
    if expect_slices:
        assert n_redo > auto.chunk_rays(), (n_redo, auto.chunk_rays())
    a, f, s = (_tuple_bits(out[p]) for p in ('auto', 'f16f8', 'f16x3'))
    is_fast, is_safe = (a == f).all(-1), (a == s).all(-1)
    assert bool((is_fast | is_safe).all()), f'{what}: {int((~(is_fast | is_safe)).sum())} rays are neither arithmetic\'s (rgb, depth, point, acc)'
    maps_differ = int((f[:, 3:] != s[:, 3:]).any(-1).sum())
    repaired = int((is_safe & ~is_fast).sum())
    assert maps_differ > 0 and repaired > 0, f'{what}: vacuous -- f16f8 and f16x3 maps differ on {maps_differ} rays, {repaired} repaired'
    assert repaired <= n_redo
    print(f'{what}: {n_redo} listed, {maps_differ} rays with f16f8 maps unlike the f16x3 ones, {repaired} repaired tuples')


@pytest.mark.parametrize('model', ['donerf_sphere', 'immersive_sphere'])
def test_verified_path_repairs_the_maps(model):
    ms, rays_np = _three(model, 800, 800)
    _check_repaired(f'{model} 800x800', ms, torch.from_numpy(rays_np).cuda())


def test_verified_path_repairs_the_maps_on_the_hostile_fixture():
    c = _case('donerf_sphere_hostile')
    ms = {p: c.model(p) for p in ('auto', 'f16f8', 'f16x3')}
    rays = torch.from_numpy(np.concatenate([c.rays] * 8, 0)).cuda()
    _check_repaired('donerf_sphere_hostile', ms, rays)


def test_verified_path_repairs_the_maps_in_every_slice_of_the_list():
    """test_gpu_full_res.py's tilted rays: Neural-3D 1352x1014 whose list fills past the head workspace (two slices)."""
    ms, rays_np = _three('neural_3d_z_plane', 1014, 1352)
    auto = ms['auto']
    rays = torch.from_numpy(rays_np).cuda()
    auto.render(rays)
    torch.cuda.synchronize()
    n, n0, chunk = rays.shape[0], auto.redo_count(), auto.chunk_rays()
    cap = min((max(32768, n // 16) + 63) & ~63, 1 << 22)
    target = (chunk + cap) // 2
    k = int(math.ceil(n / (target - n0)))
    lean = np.arange(0, n, k)
    d = np.array([0.6, 0.65, -0.4665], np.float32)
    rays_np = rays_np.copy()
    rays_np[lean, 3:6] = d / np.linalg.norm(d)
    for m in ms.values():
        m._render_calls = 1000                       # past the calls on which render() polls the sticky bits itself
    _check_repaired('neural_3d_z_plane 1352x1014 tilted', ms, torch.from_numpy(rays_np).cuda(), expect_slices=True)


# ---- 5. large calls, the reference's chunking, graph replay
def test_million_ray_call_equals_the_reference_chunks():
    ms, rays_np = _three('donerf_sphere', 1024, 1024)
    m = ms['auto']
    rays = torch.from_numpy(rays_np).cuda()
    assert rays.shape[0] == 1 << 20
    whole = m.render(rays, maps=ALL)
    torch.cuda.synchronize()
    parts = [m.render(rays[i:i + 65536], maps=ALL) for i in range(0, rays.shape[0], 65536)]
    torch.cuda.synchronize()
    for k in ('rgb',) + ALL:
        assert torch.equal(_bits(whole[k]), _bits(torch.cat([p[k] for p in parts], 0))), k


def test_maps_replay_from_a_hipgraph_into_fixed_buffers():
    c = _case('technicolor_full')
    m = c.model('auto')
    rays = torch.from_numpy(np.concatenate([c.rays] * 64, 0)).cuda()
    ref = {k: v.clone() for k, v in m.render(rays, maps=ALL).items()}
    B = rays.shape[0]
    bufs = {'distances': torch.empty((B, 1), device='cuda'), 'points': torch.empty((B, 3), device='cuda'), 'acc': torch.empty((B, 1), device='cuda')}
    rgb = torch.empty((B, 3), device='cuda')
    static_rays = rays.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.render(static_rays, out=rgb, maps=ALL, maps_out=bufs)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.render(static_rays, out=rgb, maps=ALL, maps_out=bufs)
    for _ in range(2):
        rgb.fill_(float('nan'))
        for v in bufs.values():
            v.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(rgb), _bits(ref['rgb']))
        for k in ALL:
            assert torch.equal(_bits(bufs[k]), _bits(ref[k])), k


# ---- 6. the frame-kernel option: a maps call takes the two-kernel path, same image
@pytest.mark.parametrize('case', ['donerf_sphere_600', 'technicolor_full'])
def test_maps_call_under_the_frame_kernel_option(case):
    c = _case(case)
    m = c.model('f16x3', frame_kernel=2)
    rays = torch.from_numpy(np.concatenate([c.rays] * 16, 0)).cuda()
    assert m.frame_kernel_active()
    fk = m.render(rays)['rgb'].clone()
    r = m.render(rays, maps=ALL)
    torch.cuda.synchronize()
    assert torch.equal(_bits(r['rgb']), _bits(fk))
    two = c.model('f16x3')
    ref = two.render(rays, maps=ALL)
    torch.cuda.synchronize()
    for k in ALL:
        assert torch.equal(_bits(r[k]), _bits(ref[k])), k


# ---- 7. the C ABI's edge cases
def test_c_abi_edge_cases():
    c = _case('donerf_sphere_600')
    m = c.model('auto')
    h = m.native()
    L = _lib.load()
    rays = torch.from_numpy(c.rays).cuda()
    B = rays.shape[0]
    ref = m.render(rays)['rgb'].clone()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.full((B, 3), float('nan'), device='cuda')
    assert L.hr_render_maps(h, C.c_void_p(rays.data_ptr()), B, C.c_void_p(out.data_ptr()), None, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(ref))
    out.fill_(float('nan'))
    empty = hr_maps()
    assert L.hr_render_maps(h, C.c_void_p(rays.data_ptr()), B, C.c_void_p(out.data_ptr()), C.byref(empty), st) == 0
    assert L.hr_render_frame_maps(h, C.c_void_p(rays.data_ptr()), B, 0.0, C.c_void_p(out.data_ptr()), C.byref(empty), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(ref))
    acc = torch.full((B,), -7.0, device='cuda')
    mp = hr_maps(acc_dev=acc.data_ptr())
    assert L.hr_render_maps(None, C.c_void_p(rays.data_ptr()), B, C.c_void_p(out.data_ptr()), C.byref(mp), st) == -1
    assert L.hr_render_frame_maps(None, C.c_void_p(rays.data_ptr()), B, 0.0, C.c_void_p(out.data_ptr()), C.byref(mp), st) == -1
    assert L.hr_render_maps(h, C.c_void_p(rays.data_ptr()), -1, C.c_void_p(out.data_ptr()), C.byref(mp), st) == -1
    assert L.hr_render_maps(h, None, B, C.c_void_p(out.data_ptr()), C.byref(mp), st) == -1
    assert L.hr_render_maps(h, C.c_void_p(rays.data_ptr()), B, None, C.byref(mp), st) == -1
    assert L.hr_render_maps(h, None, 0, None, C.byref(mp), st) == 0
    assert L.hr_render_frame_maps(h, None, 0, 0.0, None, C.byref(mp), st) == 0
    torch.cuda.synchronize()
    assert bool((acc == -7.0).all())                  # nothing was written by the refused and the empty calls
    # one map alone: the others stay untouched, the image is hr_render's
    assert L.hr_render_maps(h, C.c_void_p(rays.data_ptr()), B, C.c_void_p(out.data_ptr()), C.byref(mp), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(ref)) and torch.equal(acc[:, None], m.render(rays, maps=('acc',))['acc'])
    with pytest.raises(ValueError):
        m.render(rays, want=('distances',), maps=('acc',))
    with pytest.raises(ValueError):
        m.render(rays, maps=('depth',))


# ---- 8. fast_fields
@pytest.mark.parametrize('case', ['donerf_sphere_small', 'neural_3d_z_plane_small'])
def test_fast_fields_serves_distances_and_points(case):
    c = _case(case)
    g = c.golden
    rays = torch.from_numpy(c.rays).cuda()
    fast = c.model('auto', fast_fields=True)
    calls = []
    render = fast.render

    def spy(*a, **kw):
        calls.append(kw)
        return render(*a, **kw)

    fast.render = spy
    out = fast(rays, {'fields': ['distances', 'points', 'unknown_key']})
    torch.cuda.synchronize()
    assert set(out) == {'rgb', 'distances', 'points'} and calls and all('head' not in kw.get('want', ()) for kw in calls)
    Z = g.arrays['render_weights'].shape[1]
    ref, tol = _reference_maps(g.arrays['distances'].reshape(-1, Z), g.arrays['points'], g.arrays['render_weights'])
    got = dict(out, acc=torch.from_numpy(ref[2]).float())
    _check_against(f'{case} fast_fields', got, ref[:2] + (ref[2],), tol)
    # option off: the per-sample diagnostics path (it asks for the head export)
    slow = c.model('auto')
    seen = []
    render2 = slow.render

    def spy2(*a, **kw):
        seen.append(kw)
        return render2(*a, **kw)

    slow.render = spy2
    out2 = slow(rays, {'fields': ['distances', 'points']})
    torch.cuda.synchronize()
    assert any('head' in kw.get('want', ()) for kw in seen)
    for k in ('distances', 'points'):
        assert out2[k].shape == out[k].shape
