"""The training step's background coin on the device: hr_train_set_background / Model.set_background_coin / GraphedStep(white_bg='coin').

The kernels' arithmetic per background does not change -- only where the decision comes from -- so a bound model at a step whose coin is
white (black) must give the bits of the unbound call with white_bg=True (False): rgb always, and every gradient in the deterministic build
(the default build's float atomics are not reproducible between any two calls)."""
import numpy as np
import pytest
import torch

from train_dispatch_common import BRANCH, _scene

pytestmark = pytest.mark.gpu

SEED = 11
# the two scenes of tests/test_gpu_graphed_step.py, one more lane-per-sample case and one thread-per-ray case (train_dispatch_common.BRANCH)
CASES = ['shiny_z_plane_tiny', 'technicolor_z_plane_tiny', 'shiny_z_plane_small', 'seeded_donerf_sphere_z96']


def _steps(seed, lo=0):
    """The first step >= lo whose coin is white, and the first whose coin is black."""
    from hyperreel_amd.train import background_coin
    white = next(s for s in range(lo, lo + 64) if background_coin(seed, s))
    black = next(s for s in range(lo, lo + 64) if not background_coin(seed, s))
    return white, black


def _model(name, deterministic, cfg_edit=None):
    from gpu_common import make_render_fn
    from hyperreel_amd import config as C
    sc = _scene(name)
    cfg = C.to_cfg(C.to_plain(sc.cfg))
    if cfg_edit:
        cfg_edit(cfg)
    torch.manual_seed(0)
    fn = make_render_fn(cfg, sc.dataset, sc.state_dict, iteration=sc.iteration)
    fn.train()
    fn.model.set_train_deterministic(deterministic)
    return fn.model, torch.from_numpy(sc.rays[:96]).cuda()


def _step_outputs(model, rays, white_bg):
    """rgb and every gradient of sum(rgb * G) for one forward / backward."""
    G = torch.from_numpy(np.random.default_rng(3).standard_normal((rays.shape[0], 3)).astype(np.float32)).cuda()
    for p in model.parameters():
        p.grad = None
    rgb = model.forward_train(rays, white_bg=white_bg)
    (rgb * G).sum().backward()
    torch.cuda.synchronize()
    return rgb.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('deterministic', [True, False])
@pytest.mark.parametrize('name', CASES)
def test_forward_and_backward_follow_the_coin(name, deterministic):
    assert BRANCH[name]['thread_per_ray'] == (name == 'seeded_donerf_sphere_z96')
    model, rays = _model(name, deterministic)
    s_white, s_black = _steps(SEED)
    want = {True: _step_outputs(model, rays, True), False: _step_outputs(model, rays, False)}
    assert not _same(want[True][0], want[False][0])
    count = torch.zeros((), dtype=torch.int64, device='cuda')
    model.set_background_coin(SEED, count)
    try:
        for step, white in ((s_white, True), (s_black, False), (s_white + 2 ** 40, None)):
            from hyperreel_amd.train import background_coin
            white = background_coin(SEED, step) if white is None else white
            count.fill_(step)
            rgb, grads = _step_outputs(model, rays, not white)      # the argument is ignored while the model is bound
            assert _same(rgb, want[white][0]), (step, white)
            assert sorted(grads) == sorted(want[white][1])
            if deterministic:
                for k in grads:
                    assert _same(grads[k], want[white][1][k]), (k, step, white)
    finally:
        model.set_background_coin(step_tensor=None)
    # unbound: the argument decides again
    assert _same(_step_outputs(model, rays, False)[0], want[False][0]) and _same(_step_outputs(model, rays, True)[0], want[True][0])


@pytest.mark.parametrize('key', ['white_bg', 'black_bg'])
def test_a_white_bg_configuration_is_white_and_a_black_bg_one_black_at_every_step(key):
    def edit(cfg):
        cfg.color.net[key] = 1
    model, rays = _model('shiny_z_plane_tiny', True, edit)
    white = key == 'white_bg'
    want_rgb, want_grads = _step_outputs(model, rays, white)
    other_rgb, _ = _step_outputs(model, rays, not white)
    assert not _same(want_rgb, other_rgb)
    count = torch.zeros((), dtype=torch.int64, device='cuda')
    model.set_background_coin(SEED, count)
    for step in _steps(SEED):
        count.fill_(step)
        rgb, grads = _step_outputs(model, rays, not white)
        assert _same(rgb, want_rgb), step
        assert all(_same(grads[k], want_grads[k]) for k in grads), step
    model.set_background_coin(step_tensor=None)


def test_the_binding_survives_a_new_native_model():
    model, rays = _model('shiny_z_plane_tiny', True)
    s_white, s_black = _steps(SEED)
    count = torch.full((), s_white, dtype=torch.int64, device='cuda')
    model.set_background_coin(SEED, count)
    model.upsample_volume_grid([32, 28, 24])                 # replaces the planes: the next call builds a new native model
    bound = _step_outputs(model, rays, False)[0]
    model.set_background_coin(step_tensor=None)
    assert _same(bound, _step_outputs(model, rays, True)[0]) and not _same(bound, _step_outputs(model, rays, False)[0])
    with pytest.raises(TypeError, match='int64'):
        model.set_background_coin(SEED, torch.zeros((), device='cuda'))


# ---------------------------------------------------------------------------------------------------- GraphedStep
REG_CFG = dict(type='tensorf', weight=dict(type='exponential_decay', start=1.0, decay=0.5, num_epochs=1), update_AlphaMask_list=[5, 9],
               lr_decay_target_ratio=0.1, n_iters=300, total_num_tv_iters=7, L1_weight_initial=8e-3, L1_weight_rest=4e-3, TV_weight_density=1.25,
               TV_weight_app=1.25)
STEPS_PER_EPOCH = 10


def _bg_seed(first, n):
    """The smallest seed whose coins over steps [first, first + n) show both backgrounds at least twice."""
    from hyperreel_amd.train import background_coin
    for seed in range(64):
        coins = [background_coin(seed, s) for s in range(first, first + n)]
        if 2 <= sum(coins) <= n - 2:
            return seed, coins
    raise AssertionError('no seed below 64 mixes the backgrounds')


@pytest.mark.parametrize('name', ['shiny_z_plane_tiny', 'technicolor_z_plane_tiny'])
def test_replays_equal_the_eager_loop_with_the_same_coins(name):
    """GraphedStep(white_bg='coin', regularizer=HipTensoRFRegularizer) in the deterministic build: six replays equal six eager steps that
    pass white_bg=background_coin(seed, step) and call accumulate(), bit for bit in parameters, `loss` and `sse`."""
    from test_gpu_graphed_step import BATCH, REPLAYS, WARMUP, _model as gs_model, _optimizer, _rayset
    from hyperreel_amd.losses import HipImageLoss
    from hyperreel_amd.train import GraphedStep, HipTensoRFRegularizer, background_coin
    seed, coins = _bg_seed(WARMUP, REPLAYS)
    assert True in coins and False in coins                  # both backgrounds occur within the six replayed steps
    # (a) eager
    ma, video = gs_model(name, True)
    rs, oa, loss_fn = _rayset(video), _optimizer(ma), HipImageLoss('mse')
    ra = HipTensoRFRegularizer(ma, REG_CFG, STEPS_PER_EPOCH)
    la, sa = [], []
    for step in range(WARMUP + REPLAYS):
        ra.set_iter(step)
        ra.sync()
        b = rs.sample(BATCH, step_tensor=oa.step_tensor, seed=7)
        loss, sse = loss_fn.step_loss(ma.forward_train(b['coords'], white_bg=background_coin(seed, step)), b['rgb'], b['weight'])
        oa.zero_grad(set_to_none=True)
        loss.backward()
        value = ra.accumulate()
        oa.step()
        la.append((loss.detach() + value).clone())
        sa.append(sse.clone())
    torch.cuda.synchronize()
    la, sa = torch.stack(la)[WARMUP:], torch.stack(sa)[WARMUP:]
    # (b) graphed
    mb, _ = gs_model(name, True)
    ob = _optimizer(mb)
    gs = GraphedStep(mb, ob, _rayset(video), BATCH, loss=HipImageLoss('mse'), seed=7, white_bg='coin', bg_seed=seed, warmup=WARMUP,
                     regularizer=HipTensoRFRegularizer(mb, REG_CFG, STEPS_PER_EPOCH))
    lb, sb = [], []
    for _ in range(REPLAYS):
        out = gs.step()
        lb.append(out['loss'].clone())
        sb.append(out['sse'].clone())
    torch.cuda.synchronize()
    lb, sb = torch.stack(lb), torch.stack(sb)
    assert oa.steps_done() == ob.steps_done() == WARMUP + REPLAYS
    print(f'{name}: seed {seed}, coins of the replayed steps {coins}; losses eager {la.tolist()} replayed {lb.tolist()}')
    assert torch.isfinite(lb).all() and _same(la, lb) and torch.equal(sa, sb)
    pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
    for k in pa:
        assert _same(pa[k], pb[k]), k
    # a frozen background would have ended elsewhere: the same run over black only
    mc, _ = gs_model(name, True)
    gc = GraphedStep(mc, _optimizer(mc), _rayset(video), BATCH, loss=HipImageLoss('mse'), seed=7, white_bg=False, warmup=WARMUP,
                     regularizer=HipTensoRFRegularizer(mc, REG_CFG, STEPS_PER_EPOCH))
    lc = torch.stack([gc.step()['loss'].clone() for _ in range(REPLAYS)])
    torch.cuda.synchronize()
    assert not _same(lb, lc)


def test_closing_the_graphed_step_unbinds_the_background():
    from test_gpu_graphed_step import BATCH, _model as gs_model, _optimizer, _rayset
    from hyperreel_amd.losses import HipImageLoss
    from hyperreel_amd.train import GraphedStep
    model, video = gs_model('shiny_z_plane_tiny', True)
    rays = torch.from_numpy(_scene('shiny_z_plane_tiny').rays[:96]).cuda()
    opt = _optimizer(model)
    gs = GraphedStep(model, opt, _rayset(video), BATCH, loss=HipImageLoss('mse'), seed=7, white_bg='coin', bg_seed=_bg_seed(1, 6)[0], warmup=1)
    gs.step()
    # bound: both arguments give the step's own background
    with torch.no_grad():
        bound = [model.forward_train(rays, white_bg=w).clone() for w in (False, True)]
        assert _same(bound[0], bound[1])
        gs.close()
        black, white = model.forward_train(rays, white_bg=False).clone(), model.forward_train(rays, white_bg=True).clone()
    torch.cuda.synchronize()
    assert not _same(black, white) and (_same(bound[0], black) or _same(bound[0], white))
    with pytest.raises(RuntimeError, match='recapture'):
        gs.step()
    gs.recapture(white_bg=False)                             # another setting: recorded over black, the model stays unbound
    gs.step()
    with torch.no_grad():
        assert not _same(model.forward_train(rays, white_bg=False), model.forward_train(rays, white_bg=True))
