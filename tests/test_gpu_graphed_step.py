"""hr_adam_step_dev (HipAdam(capturable=True)) against hr_adam_step, and hyperreel_amd.train.GraphedStep against the same steps taken
eagerly.

Adam: the two entry points run the same per-element arithmetic; what differs is where lr / (1 - beta1^t) and 1 / sqrt(1 - beta2^t) are formed
(double on the device: pow of the device's math library; double on the host: Python's).  The learning rates of the comparison are
float32-representable, so the device's float copy of them is exact and the bias corrections are the only difference.  Bar per element:
20 steps x lr x 2^-21 -- an update is of size about lr, one fp32 rounding of it is lr x 2^-23, four times that per step.

GraphedStep: in the deterministic build the recorded step runs the same kernels on the same inputs as the eager loop, so every parameter,
both moments, the count and every loss are bit-equal -- derived, not a tolerance.  Six replays: a memset node once produced garbage on
the second replay of a graph on this runtime, so the later replays are the point."""
import copy

import numpy as np
import pytest
import torch

from train_dispatch_common import _scene

pytestmark = pytest.mark.gpu

ADAM_SIZES = [1, 7, 64, 1000, 4099]
LR = [float(np.float32(1e-2)), float(np.float32(2e-3))]


def _adam_pair(capturable, seed=3):
    from hyperreel_amd.optim import HipAdam
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter((torch.randn(n, generator=g) * 0.3).cuda()) for n in ADAM_SIZES]
    groups = [{'params': ps[:2], 'lr': LR[0], 'weight_decay': 0.0}, {'params': ps[2:], 'lr': LR[1], 'weight_decay': 0.01}]
    return ps, HipAdam(groups, lr=1e-3, betas=(0.9, 0.99), eps=1e-8, capturable=capturable)


def _grads(ps, gen, scale=1.0):
    return [(torch.randn(p.shape, generator=gen) * scale).cuda() for p in ps]


def test_adam_step_dev_follows_adam_step_for_20_steps():
    a, host = _adam_pair(False)
    b, dev = _adam_pair(True)
    assert dev.step_tensor.dtype == torch.int64 and dev.steps_done() == 0
    gen = torch.Generator().manual_seed(11)
    for step in range(20):
        for pa, pb, g in zip(a, b, _grads(a, gen, 10.0 ** (-(step % 5)))):
            pa.grad, pb.grad = g.clone(), g.clone()
        host.step()
        dev.step()
    torch.cuda.synchronize()
    assert dev.steps_done() == 20
    differ = total = 0
    for i, (pa, pb) in enumerate(zip(a, b)):
        lr = LR[0] if i < 2 else LR[1]
        d = (pa.detach() - pb.detach()).abs()
        differ += int((d > 0).sum()); total += d.numel()
        print(f'tensor {i} ({pa.numel()} elements): max |difference| {d.max().item():.3e}, bar {20 * lr * 2.0 ** -21:.3e}, differing {int((d > 0).sum())}')
        assert d.max().item() <= 20 * lr * 2.0 ** -21, i
        for key in ('exp_avg', 'exp_avg_sq'):               # the moments never see the bias corrections (weight_decay reads the parameter)
            ma, mb = host.state[pa][key], dev.state[pb][key]
            assert (ma - mb).abs().max().item() <= 1e-6 * max(ma.abs().max().item(), 1e-30), (i, key)
    print(f'elements that differ at all after 20 steps: {differ} of {total} ({differ / total:.4%})')
    # the state under torch's names, `step` from the device count; it loads into the host-counting form and back
    sd = dev.state_dict()
    assert all(float(st['step']) == 20.0 and sorted(st) == ['exp_avg', 'exp_avg_sq', 'step'] for st in sd['state'].values())
    c, host2 = _adam_pair(False)
    host2.load_state_dict(copy.deepcopy(sd))
    assert all(float(host2.state[p]['step']) == 20.0 for p in c)
    d_, dev2 = _adam_pair(True)
    dev2.load_state_dict(copy.deepcopy(host2.state_dict()))
    assert dev2.steps_done() == 20 and all('step' not in dev2.state[p] and torch.equal(dev2.state[p]['exp_avg'], dev.state[q]['exp_avg']) for p, q in zip(d_, b))


def test_a_learning_rate_takes_effect_at_the_sync_and_only_then():
    runs = [_adam_pair(True) for _ in range(3)]              # A: lr changed early, synced late; B: never changed; C: changed and synced late
    gen = torch.Generator().manual_seed(2)
    gs = [_grads(runs[0][0], gen) for _ in range(3)]

    def step(k):
        for ps, opt in runs:
            for p, g in zip(ps, gs[k]):
                p.grad = g.clone()
            opt.step()

    same = lambda x, y: all(torch.equal(p, q) for p, q in zip(runs[x][0], runs[y][0]))
    step(0)
    for grp in runs[0][1].param_groups:
        grp['lr'] = grp['lr'] * 0.5                          # not synced: the device still holds the old rates
    step(1)
    torch.cuda.synchronize()
    assert same(0, 1) and same(0, 2)
    for grp in runs[2][1].param_groups:
        grp['lr'] = grp['lr'] * 0.5
    runs[0][1].sync_hyperparameters()
    runs[2][1].sync_hyperparameters()
    runs[1][1].sync_hyperparameters()                        # nothing changed: nothing happens
    step(2)
    torch.cuda.synchronize()
    assert same(0, 2) and not same(0, 1)
    assert [o.steps_done() for _, o in runs] == [3, 3, 3]


def test_adam_step_dev_replayed_from_a_graph_equals_eager_calls():
    (a, eager), (b, graphed) = _adam_pair(True), _adam_pair(True)
    gen = torch.Generator().manual_seed(5)
    g = _grads(a, gen)
    for pa, pb, gi in zip(a, b, g):
        pa.grad, pb.grad = gi.clone(), gi.clone()            # fixed gradient buffers: the recorded step reads these addresses
    eager.step()
    graphed.step()                                           # the first step allocates the moments
    torch.cuda.synchronize()
    saved = [(p.detach().clone(), graphed.state[p]['exp_avg'].clone(), graphed.state[p]['exp_avg_sq'].clone()) for p in b]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.step()
    torch.cuda.synchronize()
    assert graphed.steps_done() == 1                         # recording executes nothing
    for p, (pv, m, v) in zip(b, saved):                      # poison, then restore in place: the replay reads the buffers' current contents
        for t, src in ((p.data, pv), (graphed.state[p]['exp_avg'], m), (graphed.state[p]['exp_avg_sq'], v)):
            t.fill_(float('nan'))
            t.copy_(src)
    for _ in range(5):
        graph.replay()
        eager.step()
    torch.cuda.synchronize()
    assert eager.steps_done() == graphed.steps_done() == 6
    for pa, pb in zip(a, b):
        assert torch.equal(pa.view(torch.int32), pb.view(torch.int32)) and torch.isfinite(pb).all()
        for key in ('exp_avg', 'exp_avg_sq'):
            assert torch.equal(eager.state[pa][key].view(torch.int32), graphed.state[pb][key].view(torch.int32))


# ---------------------------------------------------------------------------------------------------- GraphedStep
W, H, BATCH, WARMUP, REPLAYS = 16, 12, 96, 3, 6


def _rayset(video):
    from hyperreel_amd.data import DeviceRaySet
    rng = np.random.default_rng(8)
    images = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    poses = np.tile(np.eye(4, dtype=np.float32)[:3], (3, 1, 1))          # looking down -z from z = 1, as the z_plane scenes' rays
    poses[:, :, 3] = [[0.0, 0.0, 1.0], [0.1, -0.05, 1.05], [-0.1, 0.05, 0.95]]
    K = np.array([[14.0, 0, W / 2], [0, 14.0, H / 2], [0, 0, 1]], np.float32)
    return DeviceRaySet(images, poses, K, [0.1, 0.45, 0.8] if video else None, [0, 1, 2] if video else None, (W, H))


def _model(name, deterministic):
    from gpu_common import make_render_fn
    sc = _scene(name)
    torch.manual_seed(0)                      # (parameters the fixture does not carry are drawn at construction)
    fn = make_render_fn(sc.cfg, sc.dataset, sc.state_dict, iteration=sc.iteration)
    fn.train()
    fn.model.set_train_deterministic(deterministic)
    return fn.model, sc.rays.shape[1] > 6


def _optimizer(model):
    from hyperreel_amd.optim import HipAdam
    return HipAdam([p for p in model.parameters() if p.requires_grad], lr=float(np.float32(1e-3)), betas=(0.9, 0.99), eps=1e-8, capturable=True)


def _eager_run(name, deterministic, steps=WARMUP + REPLAYS):
    """(a): the iteration written out, taken eagerly `steps` times."""
    from hyperreel_amd.losses import HipImageLoss
    model, video = _model(name, deterministic)
    rs, opt, loss_fn = _rayset(video), _optimizer(model), HipImageLoss('mse')
    losses = []
    for _ in range(steps):
        b = rs.sample(BATCH, step_tensor=opt.step_tensor, seed=7)
        loss, _sse = loss_fn.step_loss(model.forward_train(b['coords'], white_bg=False), b['rgb'], b['weight'])
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    return model, opt, torch.stack(losses)


def _graphed_run(name, deterministic):
    """(b): GraphedStep(warmup=3) and six replays."""
    from hyperreel_amd.losses import HipImageLoss
    from hyperreel_amd.train import GraphedStep
    model, video = _model(name, deterministic)
    opt = _optimizer(model)
    gs = GraphedStep(model, opt, _rayset(video), BATCH, loss=HipImageLoss('mse'), seed=7, white_bg=False, warmup=WARMUP)
    assert opt.steps_done() == WARMUP                        # the warm-up steps are genuine, the recording executes nothing
    losses, sses = [], []
    for _ in range(REPLAYS):
        out = gs.step()
        losses.append(out['loss'].clone())
        sses.append(out['sse'].clone())
    torch.cuda.synchronize()
    return model, opt, torch.stack(losses), torch.stack(sses), gs


@pytest.mark.parametrize('name', ['shiny_z_plane_tiny', 'technicolor_z_plane_tiny'])
def test_replays_equal_eager_steps_bit_for_bit_in_the_deterministic_build(name):
    ma, oa, la = _eager_run(name, True)
    mb, ob, lb, sse, _gs = _graphed_run(name, True)
    assert oa.steps_done() == ob.steps_done() == WARMUP + REPLAYS
    print(f'{name}: losses eager {la[WARMUP:].tolist()} replayed {lb.tolist()}')
    assert torch.isfinite(lb).all() and torch.isfinite(sse).all() and bool((sse > 0).all())
    assert torch.equal(la[WARMUP:].view(torch.int32), lb.view(torch.int32))
    assert len(set(lb.tolist())) == REPLAYS                  # six different batches: the sampler followed the device count
    pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
    assert sorted(pa) == sorted(pb)
    stepped = 0
    for k in pa:
        assert torch.equal(pa[k].view(torch.int32), pb[k].view(torch.int32)), k
        sa, sb = oa.state.get(pa[k], {}), ob.state.get(pb[k], {})
        assert sorted(sa) == sorted(sb), k
        for key in sa:
            assert torch.equal(sa[key].view(torch.int32), sb[key].view(torch.int32)), (k, key)
        stepped += len(sa) > 0
    assert stepped >= 10                                     # grids, basis_mat and the MLP all carry moments


EAGER_RUNS = 5


@pytest.mark.parametrize('name', ['shiny_z_plane_tiny', 'technicolor_z_plane_tiny'])
def test_replays_stay_within_the_eager_spread_in_the_default_build(name):
    """fp32 atomics: two runs of the default build differ by the order of their adds, so the replayed run is held to the spread of the EAGER
    runs' final losses, measured here (it comes from the eager path, never from the code under test): it may lie outside their range by
    no more than the range's width.

    The width is taken over five eager runs, not two, and is never taken to be below 4 ulp of the float32 loss.  Measured on an MI355X:
    at this size (96 rays, 8 samples) atomic collisions are rare and runs usually agree to the bit -- five eager runs in a row gave
    8.725523204e-02 (shiny) / 8.458372951e-02 (technicolor), a spread of exactly 0 -- while one replayed run in two visits gave
    8.725523949e-02: one float32 ulp (7.45e-9) away.  A two-run spread of 0 says "no reordering happened in these two runs", not "none can
    happen": held to it, any run of the default build, eager ones included, fails whenever its adds land in another order.  The loss is
    a float32: a run that deviates at all deviates by at least one ulp, and a deviation of a few ulps cannot be told from rounding of
    the final mean; 4 ulp (3e-8 at 0.087) is that resolution, three orders of magnitude below the step-to-step movement of the loss
    (1e-3 ... 1e-2 here), which is what a stale counter, a repeated batch or a missed clear would show up as."""
    finals = [float(_eager_run(name, False)[2][-1]) for _ in range(EAGER_RUNS)]
    _, ob, lb, sse, _gs = _graphed_run(name, False)
    assert ob.steps_done() == WARMUP + REPLAYS and torch.isfinite(lb).all() and torch.isfinite(sse).all()
    b = float(lb[-1])
    lo, hi = min(finals), max(finals)
    ulp = float(np.spacing(np.float32(hi)))
    spread = max(hi - lo, 4 * ulp)
    print(f'{name}: final loss of {EAGER_RUNS} eager runs {lo:.9e} ... {hi:.9e} (measured spread {hi - lo:.3e}, 4 ulp {4 * ulp:.3e}), replayed {b:.9e}')
    assert lo - spread <= b <= hi + spread


def test_a_replay_after_the_parameters_were_replaced_raises_and_recapture_resumes():
    from hyperreel_amd.train import GraphedStep
    name = 'shiny_z_plane_tiny'
    model, opt, _, _, gs = _graphed_run(name, True)
    with pytest.raises(TypeError, match='capturable=True'):
        GraphedStep(model, torch.optim.Adam(model.parameters()), gs.rayset, BATCH, loss=gs.loss)
    old_ids = {id(p) for p in model.parameters()}
    model.upsample_volume_grid([32, 28, 24])
    replaced = [k for k, p in model.named_parameters() if id(p) not in old_ids]
    assert len(replaced) >= 6, replaced
    with pytest.raises(RuntimeError, match=r'recapture\(\)'):
        gs.step()
    with pytest.raises(ValueError, match='does not hold'):
        gs.recapture()                                       # the old optimizer holds the replaced tensors
    new = _optimizer(model)
    gs.recapture(optimizer=new, warmup=1)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    out = gs.step()
    torch.cuda.synchronize()
    assert new.steps_done() == 2 and bool(torch.isfinite(out['loss']))
    changed = [k for k in replaced if not torch.equal(dict(model.named_parameters())[k], before[k])]
    print(f'replaced {len(replaced)} parameters, the replay changed {len(changed)} of them')
    assert changed and all(tuple(before[k].shape) == tuple(dict(model.named_parameters())[k].shape) for k in replaced)
    assert any(max(before[k].shape[2:]) == 32 for k in changed)          # ... at the new size
