"""Models with a time-dependent decode mode (shadingMode RGBtLinear / RGBtFourier / RGBIdentity, densityMode DensityLinear /
DensityFourier) through the HIP path against the REFERENCE ITSELF (tests/golden/time_decode/*.npz: a shipped YAML plus the
toggle, run through the reference by tools/make_time_decode_golden.py).  `-m gpu` only.  Bar: the project's 1e-4 L-inf on RGB."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import Golden
from hyperreel_amd import scenes
from test_time_decode_host import GRAD_CASES, WHOLE, check_case, grad_golden

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4
DENSITY = [c for c in WHOLE if 'density' in c or 'both' in c or 'white_bg' in c]
VIDEO = [c for c in WHOLE if 'donerf' not in c]


def scene(g):
    """The fixture's scene: the seeded one (checksum checked by Golden; a Density* case's basis_mat_density is stored in full), thinned
    and emptied where the recipe says."""
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


@pytest.mark.parametrize('case', WHOLE)
def test_rgb_matches_the_reference(fns, case):
    """hr_render.  (Before the modes were built: NotImplementedError from plan.compile_config.)"""
    g, fn, rays = fns(case)
    check_case(case, g.arrays, g.recipe)
    rgb = fn.model.render(rays)['rgb']
    torch.cuda.synchronize()
    got = rgb.cpu().numpy()
    err = np.abs(got - g.rgb).max(-1)
    print(f'{case}: L-inf {err.max():.3e} (the reference\'s float32 from its float64: {np.abs(g.rgb - g.arrays["rgb64"]).max():.3e})')
    assert np.isfinite(got).all()
    assert err.max() <= RGB_TOL, f'{case}: L-inf {err.max():.3e} at ray {int(err.argmax())} ({(err > RGB_TOL).sum()} rays over)'
    assert fn.model.mlp_precision_active() != 'f16f8' and not fn.model.mlp_verified() and not fn.model.frame_kernel_active()


@pytest.mark.parametrize('case', WHOLE)
def test_fields_and_maps_match_the_reference(fns, case):
    """hr_render_fields: the same image, the reference's compositing weights, a density that is zero exactly where its weights say the
    sample is empty; hr_render_maps: the same image, `acc` the sum of the reference's weights."""
    g, fn, rays = fns(case)
    plain = fn.model.render(rays)['rgb'].clone()
    out = fn.model.render(rays, want=('render_weights', 'sigma'))
    maps = fn.model.render(rays, maps=('acc', 'distances'))
    torch.cuda.synchronize()
    want = g.arrays['render_weights']
    assert torch.equal(_bits(out['rgb']), _bits(plain)) and torch.equal(_bits(maps['rgb']), _bits(plain))
    assert np.abs(out['render_weights'].cpu().numpy() - want).max() <= 5e-5
    assert np.abs(maps['acc'][:, 0].cpu().numpy().astype(np.float64) - want.astype(np.float64).sum(1)).max() <= 1e-4
    sigma = out['sigma'].cpu().numpy()
    assert np.isfinite(sigma).all() and (sigma >= 0).all() and (sigma[want > 1e-4] > 0).all()


@pytest.mark.parametrize('case', ['time_decode/b_technicolor_rgbt_fourier', 'time_decode/d_technicolor_both_fourier', 'time_decode/e_neural_3d_both_fourier',
                                  'time_decode/g_donerf_rgb_identity'])
def test_frame_entry_points(fns, case):
    """hr_render_frame / hr_render_frame_maps: a static net renders the same bits; a keyframe net whose rays share one time agrees with
    hr_render as every other keyframe model does (one row of the time planes instead of a blend of two: ~1e-6)."""
    g, fn, rays = fns(case)
    video = case in VIDEO
    r = rays.clone()
    if video:
        r[:, -1] = 0.27
    a = fn.model.render(r)['rgb'].clone()
    b = fn.model.render(r, frame_time=0.27 if video else 0.0)['rgb'].clone()
    c = fn.model.render(r, frame_time=0.27 if video else 0.0, maps=('acc',))
    torch.cuda.synchronize()
    assert torch.equal(_bits(c['rgb']), _bits(b))
    if video:
        assert float((a - b).abs().max()) <= 5e-6
        assert float((a - fn.model.render(rays)['rgb']).abs().max()) > 1e-3          # the colour does depend on the ray's time
    else:
        assert torch.equal(_bits(a), _bits(b))
        assert np.abs(b.cpu().numpy() - g.rgb).max() <= RGB_TOL


@pytest.mark.parametrize('case', ['time_decode/b_technicolor_rgbt_fourier_fpk5', 'time_decode/c_technicolor_density_linear',
                                  'time_decode/e_neural_3d_both_fourier'])
def test_chunks_repeats_and_single_rays_give_the_same_bits(fns, case):
    """hr_model_reserve(64) on 130 rays: three launches; a second run; a ray on its own (every workgroup position, its own time basis)."""
    from gpu_common import make_render_fn
    g, whole, rays = fns(case)
    ref = whole.model.render(rays)['rgb'].clone()
    again = whole.model.render(rays)['rgb'].clone()
    fn = make_render_fn(g.cfg, g.dataset, scene(g))
    fn.model.reserve(64)
    got = fn.model.render(rays)['rgb']
    torch.cuda.synchronize()
    assert fn.model.chunk_rays() == 64 and whole.model.chunk_rays() >= 130
    assert torch.equal(_bits(got), _bits(ref)) and torch.equal(_bits(again), _bits(ref))
    for i in (0, 63, 64, 121, 126, 129):
        one = whole.model.render(rays[i:i + 1].contiguous())['rgb']
        assert torch.equal(_bits(one), _bits(ref[i:i + 1])), i


@pytest.mark.parametrize('case', ['time_decode/b_technicolor_rgbt_fourier_cap', 'time_decode/d_technicolor_both_fourier'])
def test_graph_replay_equals_eager(fns, case):
    g, fn, rays = fns(case)
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


@pytest.mark.parametrize('case', WHOLE)
def test_fp16_grids_equal_the_fp32_path_on_rounded_grids(fns, case):
    """float16 texels are supported: the float16 gathers on the model equal the float32 gathers on the model with rounded grids."""
    g, fn16, rays = fns(case, grid_dtype='fp16')
    _, fn32, _ = fns(case, rounded=True)
    a, b = fn16.model.render(rays)['rgb'], fn32.model.render(rays)['rgb']
    torch.cuda.synchronize()
    d = float((a - b).abs().max())
    assert d <= RGB_TOL, d
    assert 0.0 < float(np.abs(a.cpu().numpy() - g.rgb).max()) < 2e-2           # a genuinely different (rounded) scene, close to the fp32 one


@pytest.mark.parametrize('case', ['time_decode/a_technicolor_rgbt_linear', 'time_decode/d_technicolor_both_fourier'])
@pytest.mark.parametrize('precision', ['auto', 'f16f8v', 'f16x3', 'fp32'])
def test_mlp_precisions_resolve_and_render(fns, case, precision):
    """'auto', 'f16f8' and 'f16f8v' run f16x3 for the ray MLP of these models (hr_mlp_choice; nothing verified); every one within the bar."""
    g, fn, rays = fns(case, mlp_precision=precision)
    got = fn.model.render(rays)['rgb'].cpu().numpy()
    assert np.abs(got - g.rgb).max() <= RGB_TOL
    assert fn.model.mlp_precision_active() == ('fp32' if precision == 'fp32' else 'f16x3') and not fn.model.mlp_verified()


def test_an_rgb_model_is_unchanged_around_a_time_decode_one(fns):
    from gpu_common import make_render_fn
    g = Golden('donerf_sphere_small')
    rays = torch.from_numpy(g.rays).cuda()
    fn = make_render_fn(g.cfg, g.dataset, g.state_dict)
    before = fn.model.render(rays)['rgb'].clone()
    for case in ('time_decode/d_technicolor_both_fourier', 'time_decode/g_donerf_rgb_identity'):
        _, other, orays = fns(case)
        other.model.render(orays)
    after = fn.model.render(rays)['rgb']
    torch.cuda.synchronize()
    assert torch.equal(_bits(after), _bits(before))
    assert np.abs(after.cpu().numpy() - g.rgb).max() <= RGB_TOL


def test_all_occupied_volume_changes_nothing(fns):
    g, fn, rays = fns('time_decode/b_technicolor_rgbt_fourier')
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


def _tensors(g, hc):
    from hyperreel_amd import plan
    sd = {k[len('model.'):]: v for k, v in scene(g).items()}
    types = [e['type'] for e in g.cfg['embedding']['embeddings'].values()]
    idx = {'idx': types.index('ray_prediction'), 'pp_idx': -1, 'ct_idx': -1}
    return [(abi, np.ascontiguousarray(sd[key.format(**idx)], np.float32)) for abi, key in plan.upload_names(hc)]


def test_the_descriptor_is_needed_checked_and_refused_by_name():
    from hyperreel_amd import lib as L
    from hyperreel_amd import plan
    lib = L.load()
    torch.zeros(1, device='cuda')
    g = Golden('time_decode/d_technicolor_both_fourier')
    _, hc = plan.compile_model(g.cfg, g.dataset, g.grid)
    tensors = _tensors(g, hc)

    def build(desc):
        h = C.c_void_p()
        L.call('hr_model_create', C.byref(hc), C.byref(h))
        rc, msg = 0, ''
        if desc is not None:
            rc = lib.hr_model_set_time_decode(h, C.byref(desc))
            msg = lib.hr_last_error().decode() if rc else ''
        if rc == 0:
            for abi, t in tensors:
                if abi == 'basis_mat_density.weight' and (desc is None or desc.density_mode == 0):
                    continue
                L.call('hr_model_upload', h, abi.encode(), t.ctypes.data, t.nbytes)
            rc = lib.hr_model_finalize(h)
            msg = lib.hr_last_error().decode() if rc else ''
        lib.hr_model_destroy(h)
        return rc, msg

    rc, msg = build(None)
    assert rc == -2 and 'hr_model_set_time_decode' in msg                    # HR_E_STATE
    assert build(hc.time_decode) == (0, '')
    rc, msg = build(plan.hr_time_decode(2, plan.TIME_MAX_FPK + 1, 50))
    assert rc == -1 and 'frames_per_keyframe' in msg                         # over the cap
    rc, msg = build(plan.hr_time_decode(2, 5, 50))
    assert rc == -1 and 'data_dim_color' in msg                              # 27 rows are not 3 x 11
    rc, msg = build(plan.hr_time_decode(3, 4, 50))
    assert rc == -1 and 'density_mode' in msg
    # after an upload the descriptor comes too late
    h = C.c_void_p()
    L.call('hr_model_create', C.byref(hc), C.byref(h))
    abi, t = tensors[0]
    L.call('hr_model_upload', h, abi.encode(), t.ctypes.data, t.nbytes)
    assert lib.hr_model_set_time_decode(h, C.byref(hc.time_decode)) == -2
    lib.hr_model_destroy(h)
    # a static net takes no descriptor; RGBIdentity on the keyframe net and an RGBt shading on the static net are refused at creation
    g2 = Golden('donerf_sphere_small')
    _, hc2 = plan.compile_model(g2.cfg, g2.dataset, g2.grid)
    h = C.c_void_p()
    L.call('hr_model_create', C.byref(hc2), C.byref(h))
    assert lib.hr_model_set_time_decode(h, C.byref(plan.hr_time_decode(1, 4, 50))) == -1 and b'static net' in lib.hr_last_error()
    lib.hr_model_destroy(h)
    for shading, app_dim, word in ((plan.SHADING['RGBtLinear'], 6, b'keyframe net'),):
        hc2.shading, hc2.app_dim = shading, app_dim
        h = C.c_void_p()
        assert lib.hr_model_create(C.byref(hc2), C.byref(h)) == -1 and word in lib.hr_last_error()
    hc.shading, hc.app_dim = plan.SHADING['RGBIdentity'], 3
    h = C.c_void_p()
    assert lib.hr_model_create(C.byref(hc), C.byref(h)) == -1 and b'RGBIdentity' in lib.hr_last_error()
    # a Density* mode together with an MLP shading mode
    g3 = Golden('shading/e_technicolor_fea')
    _, hc3 = plan.compile_model(g3.cfg, g3.dataset, g3.grid)
    h = C.c_void_p()
    L.call('hr_model_create', C.byref(hc3), C.byref(h))
    assert lib.hr_model_set_time_decode(h, C.byref(plan.hr_time_decode(1, 4, 50))) == -1 and b'MLP shading' in lib.hr_last_error()
    lib.hr_model_destroy(h)


@pytest.mark.parametrize('case,word', [('time_decode/c_technicolor_density_fourier', 'DensityFourier'), ('time_decode/h_technicolor_linear_white_bg', 'DensityLinear')])
def test_density_modes_refuse_training_and_mask_updates_by_name(fns, case, word):
    """Density* modes are inference only: the training entry points, forward_train and updateAlphaMask / hr_dense_alpha say so."""
    from hyperreel_amd import lib as L
    g, fn, rays = fns(case)
    h = fn.model.native()
    feats = torch.empty((rays.shape[0], fn.model._hc.mlp_in), device='cuda')
    rc = L.load().hr_train_features(h, rays.data_ptr(), rays.shape[0], feats.data_ptr(), None)
    assert rc == -1 and b'Density' in L.load().hr_last_error()
    fn.model.train()
    try:
        with pytest.raises(NotImplementedError, match=word):
            fn.model(rays)
    finally:
        fn.model.eval()
    with pytest.raises(NotImplementedError, match=word):
        fn.model.color_model.net.updateAlphaMask((16, 16, 16))
    n = (C.c_int32 * 3)(8, 8, 8)
    out = torch.empty(512, device='cuda')
    rc = L.load().hr_dense_alpha(h, n, 0.01, 50, None, None, None, out.data_ptr(), None)
    assert rc == -1 and b'Density' in L.load().hr_last_error()


# ---------------------------------------------------------------- training, the three colour modes
FWD_TOL = 2e-5


def _train_fn(case, deterministic=False):
    from gpu_common import make_render_fn
    g = Golden(case)
    torch.manual_seed(0)
    fn = make_render_fn(g.cfg, g.dataset, scene(g))
    fn.train()
    fn.model.set_train_deterministic(deterministic)
    return g, fn


def _grads(fn, rays, G, white):
    for p in fn.parameters():
        p.grad = None
    rgb = fn.model.forward_train(rays, white_bg=bool(white))
    (rgb * G).sum().backward()
    torch.cuda.synchronize()
    return rgb.detach().clone(), {n: p.grad.detach().clone() for n, p in fn.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('white', [0, 1])
@pytest.mark.parametrize('case', GRAD_CASES)
def test_training_gradients_match_the_reference_autograd(case, white):
    """forward_train + backward against the REFERENCE'S OWN autograd in train mode (tests/golden/time_decode/grad): the un-clamped forward
    within 2e-5, every gradient within 1e-3 of the reference tensor's largest entry + 1e-7 (projections: GradGolden's rule), basis_mat's
    in full."""
    g, fn = _train_fn(case)
    gg = grad_golden(case, white)
    rays = torch.from_numpy(np.ascontiguousarray(g.rays[:gg.n_rays], np.float32)).cuda()
    rgb, grads = _grads(fn, rays, torch.from_numpy(gg.G).cuda(), white)
    print(f'{case} bg{white}: forward L-inf {np.abs(rgb.cpu().numpy() - gg.rgb).max():.3e}')
    assert np.abs(rgb.cpu().numpy() - gg.rgb).max() <= FWD_TOL
    assert 'model.color_model.net.basis_mat.weight' in gg.full
    checked = 0
    for name in gg.names():
        if name not in grads:
            assert not np.abs(gg.full.get(name, np.zeros(1))).max() > 0, name
            continue
        got = grads[name].cpu().numpy().astype(np.float64).ravel()
        if name in gg.full:
            want = gg.full[name].astype(np.float64).ravel()
            assert got.size == want.size, name
            err, scale = np.abs(got - want).max(), np.abs(want).max()
            print(f'  {name}: |err| {err:.3e} of max |g| {scale:.3e}')
            assert err <= 1e-3 * scale + 1e-7, f'{name}: |err| {err:.3e} vs max |g| {scale:.3e}'
        else:
            gg.check(name, got, 1e-3)
        checked += 1
    assert checked >= 12


def test_a_batch_on_keyframes_exactly(fns):
    """Every ray's time sits on a keyframe (time_offset == 0): the Fourier basis is [t, 1 ... 1, 0 ... 0], so in basis_mat's gradient the sine
    rows vanish exactly and the cosine rows of a colour all equal the frequency-0 one; the forward equals the inference render before its clamp."""
    case = 'time_decode/b_technicolor_rgbt_fourier'
    g, fn = _train_fn(case, deterministic=True)
    rays = torch.from_numpy(g.rays.copy()).cuda()
    fac = np.float32(g.dataset['num_keyframes'] * (g.dataset['num_frames'] - 1) / g.dataset['num_frames'])
    kf = (np.arange(rays.shape[0]) % g.dataset['num_keyframes']).astype(np.float32) * np.float32(1.0 / fac)
    rays[:, -1] = torch.from_numpy(kf.astype(np.float32)).cuda()
    G = torch.from_numpy(np.random.default_rng(5).standard_normal((rays.shape[0], 3)).astype(np.float32)).cuda()
    rgb, grads = _grads(fn, rays, G, 0)
    gb = grads['model.color_model.net.basis_mat.weight'].cpu().numpy().reshape(3, 9, -1)
    assert np.abs(gb[:, 1]).max() > 0 and not gb[:, 5:].any()
    for f in range(1, 4):
        assert np.abs(gb[:, 1 + f] - gb[:, 1]).max() <= 1e-6 * np.abs(gb[:, 1]).max()
    fn.eval()
    ref = fn.model.render(rays)['rgb']
    assert float((rgb.clamp(0, 1) - ref).abs().max()) <= 5e-5


@pytest.mark.parametrize('case', GRAD_CASES)
def test_the_deterministic_build_twice_bit_for_bit(case):
    g, fn = _train_fn(case, deterministic=True)
    rays = torch.from_numpy(g.rays).cuda()
    G = torch.from_numpy(np.random.default_rng(3).standard_normal((rays.shape[0], 3)).astype(np.float32)).cuda()
    rgb_a, a = _grads(fn, rays, G, 1)
    rgb_b, b = _grads(fn, rays, G, 1)
    assert torch.equal(_bits(rgb_a), _bits(rgb_b)) and sorted(a) == sorted(b) and len(a) >= 12
    for n in a:
        assert torch.equal(_bits(a[n]), _bits(b[n])), n
    # ... and equals the default build's to rounding
    _, fd = _train_fn(case, deterministic=False)
    _, d = _grads(fd, rays, G, 1)
    for n in a:
        if a[n].numel() == 0:                    # (a plane pair without channels: [8, 0, 0])
            continue
        scale = max(float(a[n].abs().max()), 1e-30)
        assert float((a[n] - d[n]).abs().max()) <= 1e-3 * scale + 1e-7, n


@pytest.mark.parametrize('case', ['time_decode/b_technicolor_rgbt_fourier', 'time_decode/a_technicolor_rgbt_linear'])
def test_three_graphed_replays_equal_the_eager_loop_in_the_deterministic_build(case):
    from hyperreel_amd.losses import HipImageLoss
    from hyperreel_amd.train import GraphedStep
    from test_gpu_graphed_step import BATCH, WARMUP, _optimizer, _rayset
    replays = 3

    def eager():
        g, fn = _train_fn(case, deterministic=True)
        model = fn.model
        rs, opt, loss_fn = _rayset(True), _optimizer(model), HipImageLoss('mse')
        losses = []
        for _ in range(WARMUP + replays):
            b = rs.sample(BATCH, step_tensor=opt.step_tensor, seed=7)
            loss, _sse = loss_fn.step_loss(model.forward_train(b['coords'], white_bg=False), b['rgb'], b['weight'])
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        return model, torch.stack(losses)

    def graphed():
        g, fn = _train_fn(case, deterministic=True)
        model = fn.model
        opt = _optimizer(model)
        gs = GraphedStep(model, opt, _rayset(True), BATCH, loss=HipImageLoss('mse'), seed=7, white_bg=False, warmup=WARMUP)
        losses = [gs.step()['loss'].clone() for _ in range(replays)]
        torch.cuda.synchronize()
        return model, torch.stack(losses)

    ma, la = eager()
    mb, lb = graphed()
    assert torch.isfinite(lb).all() and torch.equal(_bits(la[WARMUP:]), _bits(lb))
    pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
    for n in pa:
        assert torch.equal(_bits(pa[n].detach()), _bits(pb[n].detach())), n
    assert float((pa['color_model.net.basis_mat.weight'].detach().cpu() - torch.from_numpy(Golden(case).state_dict['model.color_model.net.basis_mat.weight'])).abs().max()) > 0
