"""`-m gpu`: the training image loss on the device (hr_image_loss, hyperreel_amd.losses) against the reference's own loss modules
(tests/golden/loss, tools/make_loss_golden.py) and the float64 oracle of tests/loss_oracle.py.

The bars are those of tests/loss_common.py: per loss variant 4 x the largest relative distance of the reference's float32 result from its
float64 one over the fixtures, never less than 1 float32 ulp of the array's largest magnitude.  The squared-error sum is fp32
differences and squares added in double, as hr_image_metrics' (tests/test_gpu_metrics.py): within 3 * 2^-24 of the float64 sum, 1e-6 is held.

Measured (MI355X): on all 36 fixture cases d_pred equals the reference's float32 autograd gradient bit for bit; the largest loss distance
is 3.0e-8 at a bar of 1.5e-7 (weighted_mae, B = 64), 0.32 of the bar at most (huber delta 0.1, B = 1); sse within 8.3e-9 relative.
B = 16 384 against the float64 oracle: loss within 0.13 of the bar, gradient within 0.32.  DESIGN.md 8b records the figures."""
import ctypes as C

import numpy as np
import pytest
import torch

import loss_common as LC
import loss_oracle as LO
from hyperreel_amd import lib as _lib
from hyperreel_amd import losses

pytestmark = pytest.mark.gpu

SSE_REL = 1e-6
GUARD = 64                      # floats after d_pred that a call must leave alone
SENTINEL = -12345.0


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _dev(a, misalign=False):
    """numpy -> device tensor; misalign: the data starts 4 bytes past a 16-byte boundary (the kernel's scalar-access form)"""
    a = np.ascontiguousarray(a, np.float32)
    if not misalign:
        return torch.from_numpy(a).cuda()
    buf = torch.empty((a.size + 1,), device='cuda')
    t = buf[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4
    return t


def _abi(pred, gt, weight, code, delta, want_grad=True, upstream=None, fill=None, misalign=False):
    """Through ctypes into the C ABI.  -> {'loss' float32, 'loss_sum', 'sse', 'pad', 'grad' (B, 3) float32 | None, 'guard', 'raw' (24 bytes)}.
    fill: byte the workspace, the result and d_pred are set to before the call (d_pred's guard floats hold SENTINEL either way)."""
    L = _lib.load()
    n = pred.numel() // 3
    nbytes = int(L.hr_image_loss_workspace(n))
    assert nbytes >= 16 and nbytes % 16 == 0
    ws = torch.empty((nbytes,), dtype=torch.uint8, device='cuda')
    out = torch.empty((24,), dtype=torch.uint8, device='cuda')
    gbuf = torch.empty((3 * n + GUARD + 1,), device='cuda')
    dp = gbuf[1:] if misalign else gbuf[:-1]
    if fill is not None:
        ws.fill_(fill)
        out.fill_(fill)
        dp.view(torch.uint8).fill_(fill)
    dp[3 * n:] = SENTINEL
    up = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device='cuda')
    rc = L.hr_image_loss(_ptr(pred), _ptr(gt), _ptr(weight), n, int(code), float(delta), _ptr(up), _ptr(out), _ptr(dp if want_grad else None),
                         _ptr(ws), _stream())
    assert rc == 0, L.hr_last_error()
    torch.cuda.synchronize()
    o = _lib.hr_loss_out.from_buffer_copy(out.cpu().numpy().tobytes())
    return {'loss': np.float32(o.loss), 'loss_sum': o.loss_sum, 'sse': o.sse, 'pad': o.pad, 'raw': out.cpu().numpy().tobytes(),
            'grad': dp[:3 * n].cpu().numpy().reshape(n, 3) if want_grad else None, 'guard': dp[3 * n:].cpu().numpy()}


@pytest.mark.parametrize('variant', list(LC.VARIANTS))
def test_fixture_batches_match_the_reference(variant):
    name, code, delta = LC.VARIANTS[variant]
    rows = 0
    for B in LC.BATCHES:
        p, g, w = LC.inputs(B)
        e = LC.expected(variant, B)
        o = LO.loss(name, p, g, w, delta)
        lbar, gbar = LC.loss_bar(variant, e['loss64']), LC.grad_bar(variant, e['grad64'])
        pd, gd, wd = _dev(p), _dev(g), _dev(w)
        got = _abi(pd, gd, wd, code, delta, fill=0xff)
        lerr = abs(float(got['loss']) - float(e['loss32']))
        gerr = float(np.abs(got['grad'].astype(np.float64) - e['grad32'].astype(np.float64)).max())
        serr = abs(got['sse'] - o['sse']) / o['sse']
        print(f'{variant} B={B}: loss {float(got["loss"]):.8e} err {lerr:.3e} (bar {lbar:.3e})  grad err {gerr:.3e} (bar {gbar:.3e})  '
              f'sse {got["sse"]:.8e} rel {serr:.2e}  grad bits differing from the reference {(got["grad"] != e["grad32"]).sum()}', flush=True)
        assert lerr <= lbar, (B, lerr, lbar)
        assert gerr <= gbar, (B, gerr, gbar)
        assert serr <= SSE_REL, (B, serr)
        assert got['pad'] == 0.0 and got['loss'] == np.float32(got['loss_sum'] / (3 * B))
        assert (got['guard'] == SENTINEL).all()
        # the loss alone (no d_pred), and the reference's call form on the multiplied tensors: the same sums
        alone = _abi(pd, gd, wd, code, delta, want_grad=False, fill=0xff)
        assert alone['raw'] == got['raw']
        pre = _abi(pd * wd, gd * wd, wd, code | _lib.HR_LOSS_PREMULTIPLIED, delta)
        assert pre['loss_sum'] == got['loss_sum'] and pre['loss'] == got['loss']
        assert np.abs((pre['grad'] * w).astype(np.float64) - e['grad32']).max() <= gbar
        rows += 1
    assert rows == len(LC.BATCHES)                               # no batch is left out of the comparison


def test_the_shipped_batch_size_against_the_oracle():
    """B = 16 384 from a seed (16 workgroups, every thread on the 16-byte path), every variant, against the float64 oracle."""
    B = 16384
    rng = np.random.default_rng(16384)
    g = rng.random((B, 3)).astype(np.float32)
    p = (g + rng.normal(0.0, 0.3, (B, 3))).astype(np.float32)
    w = rng.uniform(0.25, 2.0, (B, 1)).astype(np.float32)
    p[::19] = g[::19]
    w[5::31] = 0.0
    pd, gd, wd = _dev(p), _dev(g), _dev(w)
    for variant, (name, code, delta) in LC.VARIANTS.items():
        o = LO.loss(name, p, g, w, delta)
        got = _abi(pd, gd, wd, code, delta, fill=0xff)
        lbar, gbar = LC.loss_bar(variant, o['loss']), LC.grad_bar(variant, o['grad'])
        lerr, gerr = abs(float(got['loss']) - o['loss']), float(np.abs(got['grad'] - o['grad']).max())
        print(f'{variant} B={B}: loss err {lerr:.3e} (bar {lbar:.3e})  grad err {gerr:.3e} (bar {gbar:.3e})  sse rel {abs(got["sse"] - o["sse"]) / o["sse"]:.2e}', flush=True)
        assert lerr <= lbar and gerr <= gbar, variant
        assert abs(got['sse'] - o['sse']) <= SSE_REL * o['sse']
        assert abs(got['loss_sum'] - o['loss_sum']) <= 4 * LC.deviations_of(LC.load_file(variant))['loss_deviation'] * o['loss_sum']
        assert (got['guard'] == SENTINEL).all()


@pytest.mark.parametrize('variant', ['mse', 'weighted_mae', 'huber_delta0p1'])
def test_python_surface_forward_step_loss_and_backward(variant):
    name, code, delta = LC.VARIANTS[variant]
    B = 257
    p, g, w = LC.inputs(B)
    e = LC.expected(variant, B)
    gbar = LC.grad_bar(variant, e['grad64'])
    loss_fn = losses.get_loss({'type': name, 'delta': delta})
    gd, wd = _dev(g), _dev(w)
    batch = {'coords': torch.zeros((B, 6), device='cuda'), 'rgb': gd, 'weight': wd}
    pred = _dev(p).requires_grad_(True)
    a = loss_fn(pred * wd, gd * wd, **batch)                         # training_step's line
    a.backward()
    grad_a = pred.grad.clone()
    pred.grad = None
    b, sse = loss_fn.step_loss(pred, gd, wd)
    assert a.shape == b.shape == sse.shape == () and a.dtype == b.dtype == torch.float32 and sse.dtype == torch.float64
    assert b.requires_grad and not sse.requires_grad
    av, bv = float(a.detach()), float(b.detach())
    assert av == bv
    assert abs(bv - float(e['loss32'])) <= LC.loss_bar(variant, e['loss64'])
    assert abs(float(sse) - LO.loss(name, p, g, w, delta)['sse']) <= SSE_REL * float(sse)
    b.backward()
    grad_b = pred.grad.clone()
    for got in (grad_a, grad_b):
        assert np.abs(got.cpu().numpy().astype(np.float64) - e['grad32']).max() <= gbar
    pred.grad = None
    (3.0 * loss_fn.step_loss(pred, gd, wd)[0]).backward()            # an upstream factor scales the gradient by exactly 3
    assert torch.equal(pred.grad, 3.0 * grad_b)
    with torch.no_grad():
        c, _ = loss_fn.step_loss(pred, gd, wd)
    assert not c.requires_grad and float(c) == bv
    # fixed buffers, and what the surface refuses
    out = torch.empty((losses.OUT_DOUBLES,), dtype=torch.float64, device='cuda')
    ws = torch.empty((losses.workspace_doubles(B),), dtype=torch.float64, device='cuda')
    d, _ = loss_fn.step_loss(pred.detach(), gd, wd, out=out, workspace=ws)
    assert d.data_ptr() == out.data_ptr() + 16 and float(d) == bv
    with pytest.raises(ValueError, match='contiguous float32'):
        loss_fn.step_loss(pred.detach().double(), gd, wd)
    with pytest.raises(ValueError, match='contiguous float32'):
        loss_fn.step_loss(torch.empty((3, B), device='cuda').t(), gd, wd)
    with pytest.raises(ValueError, match='workspace'):
        loss_fn.step_loss(pred.detach(), gd, wd, workspace=torch.empty((0,), dtype=torch.float64, device='cuda'))
    with pytest.raises(RuntimeError, match='no CPU path'):
        loss_fn.step_loss(pred.detach(), gd.cpu(), wd)


def test_same_bits_on_every_call_stream_and_graph_replay():
    B = 4099
    variant = 'weighted_mse'
    _, code, delta = LC.VARIANTS[variant]
    p, g, w = LC.inputs(B)
    pd, gd, wd = _dev(p), _dev(g), _dev(w)
    p0, g0, w0 = pd.clone(), gd.clone(), wd.clone()
    ref = _abi(pd, gd, wd, code, delta, upstream=0.75, fill=0x00)
    again = _abi(pd, gd, wd, code, delta, upstream=0.75, fill=0xff)          # poisoned workspace, result and gradient
    assert again['raw'] == ref['raw'] and again['grad'].tobytes() == ref['grad'].tobytes()
    off = _abi(_dev(p, True), _dev(g, True), _dev(w, True), code, delta, upstream=0.75, fill=0xff, misalign=True)       # scalar accesses: the same order
    assert off['raw'] == ref['raw'] and off['grad'].tobytes() == ref['grad'].tobytes() and (off['guard'] == SENTINEL).all()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other = _abi(pd, gd, wd, code, delta, upstream=0.75, fill=0xff)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert other['raw'] == ref['raw'] and other['grad'].tobytes() == ref['grad'].tobytes()
    # a captured graph, buffers fixed; result, gradient and workspace poisoned before every replay
    L = _lib.load()
    out = torch.empty((losses.OUT_DOUBLES,), dtype=torch.float64, device='cuda')
    ws = torch.empty((losses.workspace_doubles(B),), dtype=torch.float64, device='cuda')
    dp = torch.empty((3 * B + GUARD,), device='cuda')
    up = torch.tensor([0.75], device='cuda')

    def call():
        rc = L.hr_image_loss(_ptr(pd), _ptr(gd), _ptr(wd), B, code, delta, _ptr(up), _ptr(out), _ptr(dp), _ptr(ws), _stream())
        assert rc == 0, L.hr_last_error()

    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(3):
        out.view(torch.uint8).fill_(0xff)
        ws.view(torch.uint8).fill_(0xff)
        dp.fill_(float('nan'))
        dp[3 * B:] = SENTINEL
        graph.replay()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == ref['raw']
        assert dp[:3 * B].cpu().numpy().tobytes() == ref['grad'].tobytes()
        assert (dp[3 * B:] == SENTINEL).all()
    assert torch.equal(pd, p0) and torch.equal(gd, g0) and torch.equal(wd, w0)
    # the Python surface is the same call
    m = losses.get_loss('weighted_mse')
    loss, sse = m.step_loss(pd, gd, wd)
    assert np.float32(float(loss)) == ref['loss'] and float(sse) == ref['sse']


@pytest.mark.parametrize('B', [1, 63, 65, 4099])
@pytest.mark.parametrize('misalign', [False, True])
def test_odd_sizes_write_nothing_beyond_the_gradient(B, misalign):
    """B = 1 and sizes that are no multiple of a thread's four rays, of the wavefront or of the workgroup: the guard floats behind d_pred keep
    their value, whichever access form the pointers select, and no weight pointer at all is every weight 1."""
    p, g, w = LC.inputs(B)
    for variant in ('mse', 'huber_delta1'):
        name, code, delta = LC.VARIANTS[variant]
        e = LC.expected(variant, B)
        got = _abi(_dev(p, misalign), _dev(g, misalign), _dev(w, misalign), code, delta, fill=0xff, misalign=misalign)
        assert (got['guard'] == SENTINEL).all() and got['guard'].size == GUARD
        assert np.isfinite(got['grad']).all()
        assert np.abs(got['grad'].astype(np.float64) - e['grad32']).max() <= LC.grad_bar(variant, e['grad64'])
        assert abs(float(got['loss']) - float(e['loss32'])) <= LC.loss_bar(variant, e['loss64'])
        none = _abi(_dev(p, misalign), _dev(g, misalign), None, code, delta, fill=0xff, misalign=misalign)
        o = LO.loss(name, p, g, None, delta)
        assert (none['guard'] == SENTINEL).all()
        assert abs(float(none['loss']) - o['loss']) <= LC.loss_bar(variant, o['loss'])
        assert np.abs(none['grad'] - o['grad']).max() <= LC.grad_bar(variant, o['grad'])


def test_refused_calls_on_the_device():
    L = _lib.load()
    x = torch.zeros((8, 3), device='cuda')
    out = torch.zeros((3,), dtype=torch.float64, device='cuda')
    ws = torch.zeros((2,), dtype=torch.float64, device='cuda')
    call = lambda n, t, d=1.0: L.hr_image_loss(_ptr(x), _ptr(x), None, n, t, d, None, _ptr(out), None, _ptr(ws), _stream())
    assert call(0, _lib.HR_LOSS_MSE) == -1 and L.hr_last_error()
    assert call(8, 5) == -1 and b'unknown loss type' in L.hr_last_error()
    assert call(8, _lib.HR_LOSS_HUBER, -1.0) == -1
    assert call(8, _lib.HR_LOSS_MSE) == 0
    torch.cuda.synchronize()
    assert out.tolist()[:2] == [0.0, 0.0]


def test_with_a_model_every_parameter_gets_a_finite_gradient():
    """forward_train -> step_loss -> backward on the smallest trainable fixture; the loss is the torch expression's."""
    from gpu_common import make_render_fn
    from helpers import Golden
    g = Golden('donerf_sphere_small')
    fn = make_render_fn(g.cfg, g.dataset, g.state_dict)
    fn.train()
    model = fn.model
    rays = torch.from_numpy(np.ascontiguousarray(g.rays, np.float32)).cuda()
    B = rays.shape[0]
    rng = np.random.default_rng(0)
    target = torch.from_numpy(rng.uniform(0.2, 0.8, (B, 3)).astype(np.float32)).cuda()
    weight = torch.from_numpy(rng.uniform(0.5, 1.5, (B, 1)).astype(np.float32)).cuda()
    params = [q for q in model.parameters() if q.requires_grad]
    # every parameter the torch expression of the loss reaches (the model also carries parameters this training path does not read)
    ((model.forward_train(rays, white_bg=False) * weight - target * weight) ** 2).mean().backward()
    reached = [q.grad is not None for q in params]
    assert sum(reached) >= 14                                    # 12 grid tensors, basis_mat, the MLP
    for q in params:
        q.grad = None
    loss_fn = losses.get_loss({'type': 'mse'})
    rgb = model.forward_train(rays, white_bg=False)
    loss, sse = loss_fn.step_loss(rgb, target, weight)
    loss.backward()
    torch.cuda.synchronize()
    assert [q.grad is not None for q in params] == reached
    assert all(bool(torch.isfinite(q.grad).all()) for q in params if q.grad is not None)
    assert all(float(q.grad.abs().max()) > 0 for q in params if q.grad is not None and q.numel() > 64)
    want = ((rgb.detach() * weight - target * weight) ** 2).mean()
    o = LO.loss('mse', rgb.detach().cpu().numpy(), target.cpu().numpy(), weight.cpu().numpy())
    loss = loss.detach()
    print(f'model: hip loss {float(loss):.8e} torch {float(want):.8e} float64 {o["loss"]:.8e} bar {LC.loss_bar("mse", o["loss"]):.3e}', flush=True)
    assert abs(float(loss) - float(want)) <= LC.loss_bar('mse', o['loss'])
    assert abs(float(sse) - float(((rgb.detach().double() - target.double()) ** 2).sum())) <= SSE_REL * float(sse)
    # the gradient that reaches the sample stage is the torch expression's: d_pred against autograd of the same expression
    leaf = rgb.detach().clone().requires_grad_(True)
    ((leaf * weight - target * weight) ** 2).mean().backward()
    leaf2 = rgb.detach().clone().requires_grad_(True)
    loss_fn.step_loss(leaf2, target, weight)[0].backward()
    assert np.abs(leaf2.grad.cpu().numpy() - leaf.grad.cpu().numpy()).max() <= LC.grad_bar('mse', o['grad'])
