"""hr_tensorf_reg (csrc/reg_kernel.hip) and hyperreel_amd.train.HipTensoRFRegularizer on the device.

The kernel against the reference's torch expressions (TVLoss.forward, torch.mean(torch.abs(x))) evaluated with autograd on the CPU in
float32, at the tolerances of tests/test_gpu_train.py::test_regularizers_match_the_reference_formulas: value 1e-5 relative, gradient
1e-5 * max|g| + 1e-12.  Shapes: the smallest at which the kernel can go wrong -- one row pair, odd widths, an L1-only line, a width
that takes the 16-byte path, the same width behind a pointer that does not (scalar path), tensors of more than one 4096-element
workgroup whose last one is ragged on either path, a tensor without channels, and twelve tensors in one call.

Then the regulariser object against tests/golden/reg (the reference's own regulariser, tools/make_reg_golden.py), and inside graphs."""
import ctypes as C

import numpy as np
import pytest
import torch

import reg_common as R

pytestmark = pytest.mark.gpu

WEIGHTS = (0.3, 1.7, 0.9)          # L1, density TV, appearance TV
L1, TVD, TVA = 0, 1, 2


def _plane(shape, seed, offset=0):
    """Random plane with zeros, negatives and -0.0 in it; offset: floats by which the device copy is moved off its 16-byte boundary."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * 0.5
    flat = x.view(-1)
    if flat.numel() >= 4:
        flat[0], flat[flat.numel() // 2], flat[-1] = 0.0, -0.0, -abs(float(flat[-1])) - 0.1
    g0 = torch.randn(shape, generator=g) * 1e-2
    return dict(x=x, g0=g0, offset=offset)


def _spec(shape, kind, seed, offset=0):
    """kind: 'density' (TV in slot 1 + L1), 'line' (L1 only), 'app' (TV in slot 2)."""
    d = _plane(shape, seed, offset)
    _, c, h, w = shape
    tv = kind in ('density', 'app') and c > 0
    d.update(kind=kind, kh=1e-2 * 2 / (c * (h - 1) * w) if tv else 0.0, kw=1e-2 * 2 / (c * h * (w - 1)) if tv else 0.0,
             kl=1.0 / (c * h * w) if kind != 'app' and c > 0 else 0.0,
             slot_tv={'density': TVD, 'app': TVA, 'line': -1}[kind], slot_l=-1 if kind == 'app' else L1)
    return d


def _device_copy(t, offset):
    """A contiguous device tensor of t's shape whose first element sits `offset` floats behind a 16-byte boundary."""
    buf = torch.zeros(t.numel() + 8, dtype=torch.float32, device='cuda')
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _table(specs, planes, grads):
    from hyperreel_amd import lib
    arr = (lib.hr_reg_tensor * max(len(specs), 1))()
    for e, s, p, g in zip(arr, specs, planes, grads):
        e.plane_dev, e.grad_dev = p.data_ptr() or None, g.data_ptr() or None
        e.channels, e.h, e.w = s['x'].shape[1:]
        e.kh, e.kw, e.kl = s['kh'], s['kw'], s['kl']
        e.slot_h = e.slot_w = s['slot_tv']
        e.slot_l = s['slot_l']
    return arr


def _run(specs, weights=WEIGHTS, add_grad=1):
    """One hr_tensorf_reg call: (loss[4], [gradient after the call]) on the CPU."""
    from hyperreel_amd import lib
    L = lib.load()
    planes = [_device_copy(s['x'], s['offset']) for s in specs]
    grads = [_device_copy(s['g0'], s['offset']) for s in specs]
    w = torch.tensor(weights, dtype=torch.float32, device='cuda')
    loss = torch.full((4,), float('nan'), dtype=torch.float32, device='cuda')
    plan = C.c_void_p()
    lib.check(L.hr_reg_plan_create(_table(specs, planes, grads), len(specs), C.byref(plan)), 'hr_reg_plan_create')
    try:
        lib.check(L.hr_tensorf_reg(plan, C.c_void_p(w.data_ptr()), C.c_void_p(loss.data_ptr()), add_grad,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'hr_tensorf_reg')
        torch.cuda.synchronize()
    finally:
        L.hr_reg_plan_destroy(plan)
    return loss.cpu(), [g.cpu().clone() for g in grads]


def _reference(specs, weights=WEIGHTS):
    """(total, [three unweighted terms], [g0 + autograd's gradient]) from the reference's expressions, float32 on the CPU."""
    xs = [s['x'].clone().requires_grad_(True) for s in specs]
    terms = [torch.zeros(()), torch.zeros(()), torch.zeros(())]
    for s, x in zip(specs, xs):
        if x.shape[1] == 0:
            continue
        if s['slot_l'] >= 0:
            terms[L1] = terms[L1] + torch.mean(torch.abs(x))
        if s['slot_tv'] >= 0:
            terms[s['slot_tv']] = terms[s['slot_tv']] + R.tv(x)
    total = weights[0] * terms[0] + weights[1] * terms[1] + weights[2] * terms[2]
    if total.requires_grad:
        total.backward()
    return float(total.detach()), [float(t.detach()) for t in terms], [s['g0'] + (x.grad if x.grad is not None else torch.zeros_like(x)) for s, x in zip(specs, xs)]


def _check(specs, weights=WEIGHTS):
    loss, grads = _run(specs, weights)
    total, terms, want = _reference(specs, weights)
    print(f'shapes {[tuple(s["x"].shape) for s in specs]}: value {float(loss[0]):.9e} reference {total:.9e}; terms {loss[1:].tolist()} reference {terms}')
    assert abs(float(loss[0]) - total) <= 1e-5 * abs(total)
    for k in range(3):
        assert abs(float(loss[1 + k]) - terms[k]) <= 1e-5 * abs(terms[k]), k
    for s, g, r in zip(specs, grads, want):
        if r.numel() == 0:
            continue
        err, scale = float((g - r).abs().max()), float(r.abs().max())
        assert torch.isfinite(g).all() and err <= 1e-5 * scale + 1e-12, (tuple(s['x'].shape), s['kind'], err, scale)
        active = (s['slot_l'] >= 0 and weights[s['slot_l']] != 0) or (s['slot_tv'] >= 0 and weights[s['slot_tv']] != 0)
        assert torch.equal(g, s['g0']) != active             # something was added exactly where a weight is not zero
    return loss, grads


SINGLE = {
    'one_row_pair': [((1, 1, 2, 2), 'density', 0)],
    'odd_width': [((1, 3, 2, 5), 'density', 0)],
    'l1_only_line': [((1, 4, 7, 1), 'line', 0)],
    'width_multiple_of_4': [((1, 2, 3, 4), 'density', 0)],
    'width_multiple_of_4_unaligned': [((1, 2, 3, 4), 'density', 1)],
    'two_workgroups_ragged': [((1, 5, 37, 29), 'density', 0)],                     # 5365 elements: rows and channels straddle the 4096 boundary
    'two_workgroups_ragged_16_byte': [((1, 3, 40, 44), 'app', 0)],                # 5280 elements on the 16-byte path
    'no_channels_is_skipped': [((1, 0, 9, 9), 'density', 0), ((1, 2, 4, 3), 'app', 0)],
}
MIXED = [((1, 1, 2, 2), 'density', 0), ((1, 4, 7, 1), 'line', 0), ((1, 3, 2, 5), 'app', 0), ((1, 2, 3, 4), 'density', 0), ((1, 2, 3, 1), 'line', 2),
         ((1, 5, 37, 29), 'app', 0), ((1, 3, 40, 44), 'density', 0), ((1, 3, 40, 1), 'line', 0), ((1, 2, 12, 8), 'app', 3), ((1, 0, 9, 9), 'density', 0),
         ((1, 8, 24, 28), 'density', 0), ((1, 6, 33, 21), 'app', 1)]


def _specs(rows):
    return [_spec(shape, kind, 100 + i, offset) for i, (shape, kind, offset) in enumerate(rows)]


@pytest.mark.parametrize('case', sorted(SINGLE))
def test_value_and_added_gradient_match_the_reference_expressions(case):
    _check(_specs(SINGLE[case]))


def test_twelve_tensors_in_one_call():
    assert len(MIXED) == 12 and any(int(np.prod(s)) % 4096 not in (0,) and int(np.prod(s)) > 4096 for s, _, _ in MIXED)
    _check(_specs(MIXED))
    _check(_specs(MIXED), weights=(4e-5, 0.0, 0.0))          # the TV cut: only L1 is left, the TV tensors get nothing but stay finite


def test_value_only_leaves_the_gradients_alone():
    specs = _specs(MIXED)
    loss, grads = _run(specs, add_grad=0)
    total, _, _ = _reference(specs)
    assert abs(float(loss[0]) - total) <= 1e-5 * abs(total)
    assert all(torch.equal(g, s['g0']) for g, s in zip(grads, specs))


def test_two_calls_on_the_same_inputs_give_the_same_bits():
    specs = _specs(MIXED)
    (la, ga), (lb, gb) = _run(specs), _run(specs)
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ga, gb))


def test_invalid_tables_are_refused_before_any_launch():
    from hyperreel_amd import lib
    L = lib.load()

    def create(specs, null_grad=None):
        planes = [_device_copy(s['x'], 0) for s in specs]
        grads = [_device_copy(s['g0'], 0) for s in specs]
        arr = _table(specs, planes, grads)
        if null_grad is not None:
            arr[null_grad].grad_dev = None
        plan = C.c_void_p()
        rc = L.hr_reg_plan_create(arr, len(specs), C.byref(plan))
        torch.cuda.synchronize()
        if rc == 0:
            L.hr_reg_plan_destroy(plan)
        return rc, (L.hr_last_error() or b'').decode(), grads, specs

    bad_tv = _spec((1, 2, 2, 3), 'density', 0)
    bad_tv['x'], bad_tv['g0'] = bad_tv['x'][:, :, :1, :].contiguous(), bad_tv['g0'][:, :, :1, :].contiguous()       # H == 1 with a TV term
    for what, (rc, msg, grads, specs) in {'tensor 1': create([_spec((1, 2, 3, 4), 'app', 0), bad_tv]),
                                          '13 tensors': create(_specs(MIXED + [((1, 1, 2, 2), 'app', 0)])),
                                          'tensor 2 has a null gradient': create(_specs(MIXED[:4]), null_grad=2)}.items():
        assert rc == lib.HR_E_INVALID and what in msg, (what, rc, msg)
        assert all(torch.equal(g.cpu(), s['g0']) for g, s in zip(grads, specs))          # nothing ran
    assert create(_specs(MIXED))[0] == 0


# ---------------------------------------------------------------------------------------------------- HipTensoRFRegularizer
def _model(f):
    from gpu_common import make_render_fn
    torch.manual_seed(0)
    fn = make_render_fn(f.cfg, f.dataset, f.state_dict)
    fn.train()
    return fn.model


@pytest.mark.parametrize('name', R.CASES)
def test_set_iter_sync_accumulate_give_the_reference_value_and_gradients(name):
    from hyperreel_amd.train import HipTensoRFRegularizer
    f = R.fixture(name)
    model = _model(f)
    reg = HipTensoRFRegularizer(model, f.recipe['reg'], f.recipe['steps_per_epoch'])
    params = dict(model.named_parameters())
    for i in f.iterations:
        for p in params.values():
            p.grad = None
        reg.set_iter(i)
        reg.sync()
        value = float(reg.accumulate())
        torch.cuda.synchronize()
        ref = float(f.arrays[f'it{i}/loss32'])
        warm = bool(f.arrays[f'it{i}/warming_up'])
        print(f'{name} iteration {i}: value {value:.9e} reference {ref:.9e} warming up {warm}')
        assert abs(value - ref) <= 1e-5 * abs(ref) and reg.warming_up() == warm
        n = 0
        for k, p in params.items():
            key = f'it{i}/grad/model.{k}'                     # the fixtures carry the render function's state_dict keys
            if p.grad is None:
                assert key not in f.arrays or not f.arrays[key].any(), k          # only tensors the regulariser lists receive a gradient
                continue
            got = p.grad.cpu()
            if warm or key not in f.arrays:                  # left out of the loss / outside [0, stop_iters): nothing is added
                assert not got.any(), (k, i)
                continue
            want = torch.from_numpy(f.arrays[key])
            assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()) + 1e-12, (k, i)
            n += 1
        recorded = sum(k.startswith(f'it{i}/grad/') for k in f.arrays)   # every gradient the reference's autograd produced was compared
        assert warm or (n == recorded and (n >= 2 or ref == 0.0)), (i, n, recorded)
    reg.close()


def test_weights_take_effect_at_sync_and_only_then_inside_a_graph():
    from hyperreel_amd.train import HipTensoRFRegularizer
    f = R.fixture('video_no_app')                            # weight 0.75, no decay: iterations 1 and 40 differ by the L1 switch alone
    model = _model(f)
    reg = HipTensoRFRegularizer(model, f.recipe['reg'], f.recipe['steps_per_epoch'])
    reg.set_iter(1)
    reg.sync()
    reg.accumulate()                                         # allocates the gradients and builds the table
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = reg.accumulate()
    replay = lambda: (graph.replay(), torch.cuda.synchronize(), float(out))[2]
    a = replay()
    assert replay() == a
    reg.set_iter(40)                                         # crosses the switch; the device still holds iteration 1's weights
    assert replay() == a
    reg.sync()
    b = replay()
    fa, fb = float(f.arrays['it1/loss32']), float(f.arrays['it40/loss32'])
    print(f'replays: {a:.9e} -> {b:.9e}; fixture {fa:.9e} -> {fb:.9e}')
    assert abs(a - fa) <= 1e-5 * abs(fa) and abs(b - fb) <= 1e-5 * abs(fb)
    assert abs((a - b) - (fa - fb)) <= 1e-5 * (abs(fa) + abs(fb)) and a != b
    reg.close()


def test_the_table_is_rebuilt_when_parameters_are_replaced():
    from hyperreel_amd.train import HipTensoRFRegularizer
    f = R.fixture('static_decay')
    model = _model(f)
    reg = HipTensoRFRegularizer(model, f.recipe['reg'], f.recipe['steps_per_epoch'])
    reg.set_iter(0)
    reg.sync()
    a = float(reg.accumulate())
    model.upsample_volume_grid([16, 12, 10])
    b = float(reg.accumulate())
    net = model.color_model.net
    want = sum(w * float(t) for w, t in zip(reg.weights, R.reference_terms([[p.detach().cpu() for p in g] for g in net._reg_planes()], net.video)))
    assert a != b and abs(b - want) <= 1e-5 * abs(want)
    assert all(p.grad is not None and tuple(p.grad.shape) == tuple(p.shape) for p, *_ in reg.terms())
    reg.close()


# ---------------------------------------------------------------------------------------------------- GraphedStep
REG_CFG = dict(type='tensorf', weight=dict(type='exponential_decay', start=1.0, decay=0.5, num_epochs=1), update_AlphaMask_list=[5, 9],
               lr_decay_target_ratio=0.1, n_iters=300, total_num_tv_iters=7, L1_weight_initial=8e-3, L1_weight_rest=4e-3, TV_weight_density=1.25,
               TV_weight_app=1.25)
STEPS_PER_EPOCH = 10


@pytest.mark.parametrize('name', ['shiny_z_plane_tiny', 'technicolor_z_plane_tiny'])
def test_replays_with_the_device_regulariser_equal_eager_steps_bit_for_bit(name):
    """GraphedStep(regularizer=HipTensoRFRegularizer) in the deterministic build against the iteration written out: the same kernels on
    the same inputs, so parameters and losses are bit-equal.  The nine steps cross the L1 switch (iteration 5) and the TV cut (after
    iteration 7) with a decaying weight: a replay that repeated one step's weights would not."""
    from test_gpu_graphed_step import BATCH, REPLAYS, WARMUP, _model as gs_model, _optimizer, _rayset
    from hyperreel_amd.losses import HipImageLoss
    from hyperreel_amd.train import GraphedStep, HipTensoRFRegularizer
    # (a) eager
    ma, video = gs_model(name, True)
    rs, oa, loss_fn = _rayset(video), _optimizer(ma), HipImageLoss('mse')
    ra = HipTensoRFRegularizer(ma, REG_CFG, STEPS_PER_EPOCH)
    la, values = [], []
    for step in range(WARMUP + REPLAYS):
        ra.set_iter(step)
        ra.sync()
        b = rs.sample(BATCH, step_tensor=oa.step_tensor, seed=7)
        loss, _sse = loss_fn.step_loss(ma.forward_train(b['coords'], white_bg=False), b['rgb'], b['weight'])
        oa.zero_grad(set_to_none=True)
        loss.backward()
        value = ra.accumulate()
        oa.step()
        la.append((loss.detach() + value).clone())
        values.append(value.clone())
    torch.cuda.synchronize()
    la, values = torch.stack(la), torch.stack(values)
    # (b) graphed
    mb, _ = gs_model(name, True)
    ob = _optimizer(mb)
    gs = GraphedStep(mb, ob, _rayset(video), BATCH, loss=HipImageLoss('mse'), seed=7, white_bg=False, warmup=WARMUP,
                     regularizer=HipTensoRFRegularizer(mb, REG_CFG, STEPS_PER_EPOCH))
    lb = torch.stack([gs.step()['loss'].clone() for _ in range(REPLAYS)])
    torch.cuda.synchronize()
    assert oa.steps_done() == ob.steps_done() == WARMUP + REPLAYS
    print(f'{name}: regulariser values {values.tolist()}; losses eager {la[WARMUP:].tolist()} replayed {lb.tolist()}')
    assert torch.isfinite(lb).all() and bool((values > 0).all())
    assert float(values[8]) < 0.1 * float(values[7])         # the TV cut happened ...
    assert torch.equal(la[WARMUP:].view(torch.int32), lb.view(torch.int32))
    pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
    for k in pa:
        assert torch.equal(pa[k].view(torch.int32), pb[k].view(torch.int32)), k
    # ... and the regulariser trains: without it the planes end elsewhere
    mc, _ = gs_model(name, True)
    oc = _optimizer(mc)
    gc = GraphedStep(mc, oc, _rayset(video), BATCH, loss=HipImageLoss('mse'), seed=7, white_bg=False, warmup=WARMUP)
    for _ in range(REPLAYS):
        gc.step()
    torch.cuda.synchronize()
    pc = dict(mc.named_parameters())
    assert any(not torch.equal(pb[k], pc[k]) for k in pb if 'density_plane' in k)
