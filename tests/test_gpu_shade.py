"""Models with shadingMode MLP_Fea / MLP through the HIP path against the REFERENCE ITSELF (tests/golden/shading/[a-g]_*.npz: a shipped
YAML plus an edit, run through the reference by tools/make_shading_golden.py).  `-m gpu` only.  Bar: the project's 1e-4 L-inf on RGB."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import Golden
from hyperreel_amd import scenes
from test_shade_host import WHOLE

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4


def scene(g):
    """The fixture's scene: the seeded one (checksum checked by Golden), emptied where the recipe says."""
    return scenes.carve_half_space(scenes.scale_density(g.state_dict, g.recipe.get('density_scale', 1.0)), g.recipe['carve_x'])


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope='module')
def fns():
    cache = {}

    def get(case, grid_dtype='fp32', rounded=False, **kw):
        key = (case, grid_dtype, rounded, tuple(sorted(kw.items())))
        if key not in cache:
            from gpu_common import make_render_fn
            from test_gpu_parity import _round_grids_to_half
            g = Golden(case)
            sd = scene(g)
            fn = make_render_fn(g.cfg, g.dataset, _round_grids_to_half(sd) if rounded else sd, grid_dtype=grid_dtype, **kw)
            cache[key] = (g, fn, torch.from_numpy(g.rays).cuda())
        return cache[key]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


VIDEO = [c for c in WHOLE if 'technicolor' in c or 'immersive' in c]
STATIC = [c for c in WHOLE if c not in VIDEO]


@pytest.mark.parametrize('case', WHOLE)
def test_rgb_matches_the_reference(fns, case):
    g, fn, rays = fns(case)
    rgb = fn.model.render(rays)['rgb']
    torch.cuda.synchronize()
    got = rgb.cpu().numpy()
    err = np.abs(got - g.rgb).max(-1)
    print(f'{case}: L-inf {err.max():.3e} (the reference\'s float32 from its float64: {np.abs(g.rgb - g.arrays["rgb64"]).max():.3e})')
    assert np.isfinite(got).all()
    assert err.max() <= RGB_TOL, f'{case}: L-inf {err.max():.3e} at ray {int(err.argmax())} ({(err > RGB_TOL).sum()} rays over)'
    assert fn.model.mlp_precision_active() != 'f16f8' and not fn.model.mlp_verified() and not fn.model.frame_kernel_active()


@pytest.mark.parametrize('case', WHOLE)
def test_weights_match_the_reference(fns, case):
    """hr_render_fields: the image is the same one, and the compositing weights are the reference's."""
    g, fn, rays = fns(case)
    plain = fn.model.render(rays)['rgb'].clone()
    out = fn.model.render(rays, want=('render_weights',))
    torch.cuda.synchronize()
    assert torch.equal(_bits(out['rgb']), _bits(plain))
    assert np.abs(out['render_weights'].cpu().numpy() - g.arrays['render_weights']).max() <= 5e-5


@pytest.mark.parametrize('case', WHOLE)
def test_fp16_grids_equal_the_fp32_path_on_rounded_grids(fns, case):
    g, fn16, rays = fns(case, grid_dtype='fp16')
    _, fn32, _ = fns(case, rounded=True)
    a, b = fn16.model.render(rays)['rgb'], fn32.model.render(rays)['rgb']
    torch.cuda.synchronize()
    d = float((a - b).abs().max())
    assert d <= RGB_TOL, d
    assert 0.0 < float(np.abs(a.cpu().numpy() - g.rgb).max()) < 5e-3           # a genuinely different (rounded) scene, close to the fp32 one


@pytest.mark.parametrize('case', ['shading/a_donerf_fea_default', 'shading/e_technicolor_fea'])
def test_frame_entry_point(fns, case):
    """hr_render_frame: a static net renders the same bits; a keyframe net whose rays share one time agrees with hr_render as every
    other keyframe model does (one row of the time planes instead of a blend of two: ~1e-6)."""
    g, fn, rays = fns(case)
    video = rays.shape[1] == 8 and case in VIDEO
    r = rays.clone()
    if video:
        r[:, -1] = 0.25
    a = fn.model.render(r)['rgb'].clone()
    b = fn.model.render(r, frame_time=0.25 if video else 0.0)['rgb']
    torch.cuda.synchronize()
    if video:
        assert float((a - b).abs().max()) <= 5e-6
    else:
        assert torch.equal(_bits(a), _bits(b))
        assert np.abs(b.cpu().numpy() - g.rgb).max() <= RGB_TOL


@pytest.mark.parametrize('case', ['shading/c_donerf_fea_c40', 'shading/g_technicolor_thresh'])
def test_chunking_is_invisible(case):
    """hr_model_reserve(64) on 130 rays: three launches of the three kernels, the single-chunk image bit for bit."""
    from gpu_common import make_render_fn
    g = Golden(case)
    rays = torch.from_numpy(g.rays).cuda()
    whole = make_render_fn(g.cfg, g.dataset, scene(g))
    ref = whole.model.render(rays)['rgb'].clone()
    fn = make_render_fn(g.cfg, g.dataset, scene(g))
    fn.model.reserve(64)
    got = fn.model.render(rays)['rgb']
    torch.cuda.synchronize()
    assert fn.model.chunk_rays() == 64 and whole.model.chunk_rays() >= 130
    assert torch.equal(_bits(got), _bits(ref))


@pytest.mark.parametrize('case', ['shading/b_donerf_fea_pe2_c64', 'shading/e_technicolor_fea'])
def test_single_rays_dead_batches_and_repeats(fns, case):
    g, fn, rays = fns(case)
    ref = fn.model.render(rays)['rgb'].clone()
    again = fn.model.render(rays)['rgb']
    torch.cuda.synchronize()
    assert torch.equal(_bits(again), _bits(ref))                        # a second run: the same bits
    thresh = float(g.cfg.color.net.get('rm_weight_mask_thre', 1e-4))
    live = g.arrays['render_weights'] > thresh
    dead = np.flatnonzero(~live.any(1))
    assert dead.size >= 1
    for i in (0, int(dead[0]), int(np.argmax(live.sum(1))), rays.shape[0] - 1):   # one ray on its own
        one = fn.model.render(rays[i:i + 1].contiguous())['rgb']
        assert torch.equal(_bits(one), _bits(ref[i:i + 1])), i
    idx = torch.from_numpy(dead).cuda()
    only_dead = fn.model.render(rays[idx].contiguous())['rgb']          # a batch made only of rays without a live sample
    torch.cuda.synchronize()
    assert torch.equal(_bits(only_dead), _bits(ref[idx]))
    assert np.abs(only_dead.cpu().numpy() - g.rgb[dead]).max() <= RGB_TOL


def test_graph_replay_equals_eager(fns):
    g, fn, rays = fns('shading/a_donerf_fea_default')
    ref = fn.model.render(rays)['rgb'].clone()
    static_rays, rgb = rays.clone(), torch.empty_like(ref)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn.model.render(static_rays, out=rgb)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn.model.render(static_rays, out=rgb)
    for _ in range(3):
        rgb.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(rgb), _bits(ref))


@pytest.mark.parametrize('case', ['shading/b_donerf_fea_pe2_c64', 'shading/e_technicolor_fea'])
def test_all_occupied_volume_changes_nothing(fns, case):
    g, fn, rays = fns(case)
    ref = fn.model.render(rays)['rgb'].clone()
    net = fn.model.color_model.net
    net.register_buffer('alpha_volume', torch.ones(8, 8, 8, device='cuda'), persistent=False)
    net.register_buffer('alpha_aabb', net.aabb.detach().clone().reshape(2, 3), persistent=False)
    fn.model.set_occupancy(True)
    try:
        got = fn.model.render(rays)['rgb']
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _bits(ref))
    finally:
        fn.model.set_occupancy(False)


@pytest.mark.parametrize('case', ['shading/d_donerf_mlp_pe6', 'shading/e_technicolor_fea'])
def test_maps_entry_points_render_with_parity(fns, case):
    """hr_render_maps / hr_render_frame_maps (rendered, not refused): the same image, and the maps are the weighted sums of
    the diagnostics path's per-sample values."""
    g, fn, rays = fns(case)
    ref = fn.model.render(rays)['rgb'].clone()
    r = fn.model.render(rays, maps=('distances', 'points', 'acc'))
    d = fn.model.render(rays, want=('distances', 'points', 'render_weights'))
    torch.cuda.synchronize()
    assert torch.equal(_bits(r['rgb']), _bits(ref))
    w = d['render_weights'].double()
    assert float((r['acc'][:, 0].double() - w.sum(1)).abs().max()) <= 1e-5
    assert float((r['distances'][:, 0].double() - (w * d['distances'].double()).sum(1)).abs().max()) <= 1e-4 * max(1.0, float(d['distances'].abs().max()))
    assert float((r['points'].double() - (w[..., None] * d['points'].double()).sum(1)).abs().max()) <= 1e-4 * max(1.0, float(d['points'].abs().max()))
    if case in VIDEO:
        rt = rays.clone()
        rt[:, -1] = 0.25
        a = fn.model.render(rt, frame_time=0.25)['rgb'].clone()
        b = fn.model.render(rt, frame_time=0.25, maps=('acc',))
        torch.cuda.synchronize()
        assert torch.equal(_bits(b['rgb']), _bits(a))


def test_finalize_needs_the_descriptor_and_every_tensor():
    from hyperreel_amd import lib as L
    from hyperreel_amd import plan
    g = Golden('shading/b_donerf_fea_pe2_c64')
    _, hc = plan.compile_model(g.cfg, g.dataset, g.grid)
    lib = L.load()
    sd = {k[len('model.'):]: v for k, v in scene(g).items()}
    types = [e['type'] for e in g.cfg['embedding']['embeddings'].values()]
    idx = {'idx': types.index('ray_prediction'), 'pp_idx': -1, 'ct_idx': -1}
    tensors = [(abi, np.ascontiguousarray(sd[key.format(**idx)], np.float32)) for abi, key in plan.upload_names(hc)]

    def build(with_desc, skip=None):
        h = C.c_void_p()
        L.call('hr_model_create', C.byref(hc), C.byref(h))
        if with_desc:
            L.call('hr_model_set_shading_mlp', h, C.byref(hc.shade_mlp))
        for abi, t in tensors:
            if abi.startswith('renderModule') and not with_desc or abi == skip:
                continue
            L.call('hr_model_upload', h, abi.encode(), t.ctypes.data, t.nbytes)
        rc = lib.hr_model_finalize(h)
        msg = lib.hr_last_error().decode() if rc else ''
        lib.hr_model_destroy(h)
        return rc, msg

    torch.zeros(1, device='cuda')
    rc, msg = build(False)
    assert rc == -2 and 'hr_model_set_shading_mlp' in msg                # HR_E_STATE
    rc, msg = build(True, skip='renderModule.mlp.2.bias')
    assert rc == -2 and 'renderModule.mlp.2.bias' in msg
    assert build(True) == (0, '')
    h = C.c_void_p()                                                     # an RGB model takes no descriptor
    g2 = Golden('donerf_sphere_small')
    _, hc2 = plan.compile_model(g2.cfg, g2.dataset, g2.grid)
    L.call('hr_model_create', C.byref(hc2), C.byref(h))
    bad = plan.hr_shading_mlp(2, 2, 64)
    assert lib.hr_model_set_shading_mlp(h, C.byref(bad)) == -1 and b'shading' in lib.hr_last_error()
    lib.hr_model_destroy(h)
    h = C.c_void_p()                                                     # values out of range are refused by name
    L.call('hr_model_create', C.byref(hc), C.byref(h))
    for d, word in ((plan.hr_shading_mlp(7, 2, 64), b'view_pe'), (plan.hr_shading_mlp(2, 7, 64), b'fea_pe'), (plan.hr_shading_mlp(2, 2, 257), b'feature_c')):
        assert lib.hr_model_set_shading_mlp(h, C.byref(d)) == -1 and word in lib.hr_last_error()
    lib.hr_model_destroy(h)


def test_training_entry_points_refuse(fns):
    from hyperreel_amd import lib as L
    g, fn, rays = fns('shading/b_donerf_fea_pe2_c64')
    h = fn.model.native()
    feats = torch.empty((rays.shape[0], fn.model._hc.mlp_in), device='cuda')
    rc = L.load().hr_train_features(h, rays.data_ptr(), rays.shape[0], feats.data_ptr(), None)
    assert rc == -1 and b'MLP_Fea' in L.load().hr_last_error()
    fn.model.train()
    try:
        with pytest.raises(NotImplementedError, match='training with shadingMode MLP_Fea'):
            fn.model(rays)
    finally:
        fn.model.eval()


def test_an_rgb_model_is_unchanged_around_an_mlp_shaded_one(fns):
    from gpu_common import make_render_fn
    g = Golden('donerf_sphere_small')
    rays = torch.from_numpy(g.rays).cuda()
    fn = make_render_fn(g.cfg, g.dataset, g.state_dict)
    before = fn.model.render(rays)['rgb'].clone()
    _, shaded, srays = fns('shading/a_donerf_fea_default')
    shaded.model.render(srays)
    after = fn.model.render(rays)['rgb']
    torch.cuda.synchronize()
    assert torch.equal(_bits(after), _bits(before))
    assert np.abs(after.cpu().numpy() - g.rgb).max() <= RGB_TOL
