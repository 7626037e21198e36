"""`-m gpu`: the training step's sample stage on every branch hr_launch_train dispatches to (csrc/train_kernel.hip), against torch.autograd
on the CPU restatement of the reference (oracle/torch_port.py).

Phase A is a lane-per-sample kernel for rays of up to 64 samples (hr_train_lanes_kernel<ZP, NB, PC>: 8, 4, 2 or 1 rays per wavefront) and a
thread-per-ray kernel above (hr_train_kernel<128 | 256>, which leaves no taps on the tape); phase B keeps its gradient window in LDS
(hr_train_gather_bwd_lines_kernel, keyed by keyframe interval for video nets, in two passes where the rows of all three pairs exceed the
LDS cap together) or falls back to global atomics.  Which branch a case takes is answered by the library's own hr_train_plan
(csrc/hr_plan.h, compiled for the host: helpers.train_branch); the table of cases is tests/train_dispatch_common.py.  One small case per branch:
  1. the stage alone, the raw head supplied to both sides (no LeakyReLU sign flips): un-clamped forward, dL/d head per head column on the
     column's own scale, basis_mat, every plane / line, the colour table;
  2. end to end through forward_train at mlp_precision='fp32': the MLP gradients too (hidden width 128, a cascade's point MLP);
  3. ragged batches (ray counts that fill no workgroup) and the empty batch;
  4. the deterministic build on the same branches.
Bars (the suite's device numbers): forward <= 2e-5 (relative above 1), every gradient entry <= 1e-3 of its tensor's largest reference entry
+ 1e-7; the host build of the same arithmetic holds 2e-4 on all of these cases (tests/test_train_host.py).  torch.autograd returns NaN on a ray
where a masked-out branch divides by zero; such rays (at most 4 per case) are dropped and the rest compared.  Every test prints its worst
error ratios before it asserts."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import train_branch
from test_gpu_train import _reference_grads
from torch_port import TorchPort
from train_dispatch_common import BRANCH, DETERMINISTIC, _assert_branch, _levels, _scene

pytestmark = pytest.mark.gpu

CASCADES = [c for c in BRANCH if BRANCH[c].get('cascade')]
# 4 x the port's own noise under a one-ulp move of rays and parameters, where the case needs it (test_forward_train_matches_autograd_end_to_end's docstring)
E2E_NOISE_BARS = {'shiny_z_tensorf_cascaded': {'point_mlp.4.weight': 4 * 5.00e-3, 'point_mlp.4.bias': 4 * 5.12e-3}}
GRID_NAMES = [f'{k}{j}' for k in ('d_a', 'd_b', 'a_a', 'a_b') for j in range(3)]
MAX_DROPPED = 4


class _Report:
    """Collects |err| / scale per compared tensor, prints them all, then asserts them all."""

    def __init__(self, title):
        self.title, self.rows, self.errors = title, [], []

    def forward(self, got, want, what='forward', tol=2e-5):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        r = float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()) if want.size else 0.0       # unsorted / unmasked variants reach 1e5
        self.rows.append((what, r / tol))
        if not r <= tol:
            self.errors.append(f'{what}: {r:.3e} > {tol:.1e}')

    def grad(self, what, got, want, tol=1e-3):
        want = np.asarray(want, np.float64)
        got = np.asarray(got, np.float64).reshape(want.shape)
        scale = float(np.abs(want).max())
        assert scale > 0, f'{self.title}: {what}: the reference gradient is identically zero'
        err = float(np.abs(got - want).max())
        self.rows.append((what, err / (tol * scale + 1e-7)))
        if not err <= tol * scale + 1e-7:
            self.errors.append(f'{what}: |err| {err:.3e} vs scale {scale:.3e}')

    def finish(self):
        worst = max(self.rows, key=lambda r: r[1])
        print(f'{self.title}: worst {worst[0]} at {worst[1]:.3f} of its bar; ' + ', '.join(f'{w} {r:.3f}' for w, r in self.rows))
        assert not self.errors, f'{self.title}: ' + '; '.join(self.errors)


def _np(t):
    return t.detach().cpu().numpy()


def _port_with_leaves(sc):
    port = TorchPort(sc.cfg, sc.dataset, sc.state_dict, iteration=sc.iteration)
    leaves = {}
    for name, grp in (('d_a', port.d_a), ('d_b', port.d_b), ('a_a', port.a_a), ('a_b', port.a_b)):
        for j, t in enumerate(grp):
            leaves[f'{name}{j}'] = t
    leaves['basis'] = port.basis
    keys = [k for k in sc.state_dict if k.endswith('color_embedding')]
    if keys and port.o.ds.get('val_all', False):         # per-camera colour table (ColorTransformEmbedding, dataset.val_all)
        leaves['table'] = port.color_table = torch.from_numpy(np.ascontiguousarray(sc.state_dict[keys[0]], np.float32))
    for t in leaves.values():
        t.requires_grad_(True)
    return port, leaves


@functools.lru_cache(maxsize=None)
def _stage_reference(name, n, white):
    """autograd of the port with the head supplied: head0 (the port's own MLP output: the ray MLP's, zeros for a ZeroMLP, the point MLP's for
    a cascade), the un-clamped rgb, dL/d head and dL/d every leaf for L = sum(rgb * G).  Rays with a non-finite reference gradient are dropped."""
    sc = _scene(name)
    coarse, hc = _levels(sc)
    port, leaves = _port_with_leaves(sc)
    rays = torch.from_numpy(sc.rays[:n])
    assert rays.shape[0] == n

    def run(rays):
        for t in leaves.values():
            t.grad = None
        with torch.no_grad():
            if coarse is not None:                           # the point MLP's own output, run once without a graph
                rec = {}
                orig = port._run_layers
                port._run_layers = lambda *a: rec.setdefault('h', orig(*a))
                port.embed(rays)
                port._run_layers = orig
                head0 = rec['h'].reshape(rays.shape[0], -1)
            elif port.o.zero_net:
                head0 = torch.zeros(rays.shape[0], hc.z_channels * hc.preds_per_z)
            else:
                head0 = port._mlp(port._param_pe(rays))
        head = head0.clone().requires_grad_(True)
        x = port.embed(rays, point_head=head.view(rays.shape[0] * coarse.z_channels, -1)) if coarse is not None else port.embed(rays, head=head)
        rgb = port.color(x, train=True, white_bg=bool(white))
        G = torch.randn(rgb.shape, generator=torch.Generator().manual_seed(3))
        (rgb * G).sum().backward()
        return head0, head, rgb, G

    head0, head, rgb, G = run(rays)
    ok = torch.isfinite(head.grad).all(-1)
    dropped = int((~ok).sum())
    if dropped:
        assert dropped <= MAX_DROPPED, f'{name}: the reference gradient is not finite on {dropped} rays'
        rays = rays[ok].contiguous()
        head0, head, rgb, G = run(rays)
    assert bool(torch.isfinite(head.grad).all())
    grads = {k: (None if t.grad is None else t.grad.numpy().copy()) for k, t in leaves.items()}
    assert all(g is None or np.isfinite(g).all() for g in grads.values()), name
    return SimpleNamespace(rays=rays.numpy().copy(), kept=ok.numpy().copy(), dropped=dropped, head0=head0.numpy().copy(), rgb=rgb.detach().numpy().copy(),
                           G=G.numpy().copy(), d_head=head.grad.numpy().copy(), grads=grads, z=hc.z_channels, p=hc.preds_per_z,
                           video=bool(hc.video), n_den=list(hc.n_den))


_MODELS = {}


def _model(name, deterministic=False):
    """One fp32-MLP model per scene and mode, in train mode, gradients cleared."""
    from gpu_common import make_render_fn
    key = (name, bool(deterministic))
    if key not in _MODELS:
        sc = _scene(name)
        fn = make_render_fn(sc.cfg, sc.dataset, sc.state_dict, mlp_precision='fp32', iteration=sc.iteration)
        fn.model.set_train_deterministic(deterministic)
        fn.train()
        _MODELS[key] = fn
    fn = _MODELS[key]
    for p in fn.parameters():
        p.grad = None
    return fn


def _stage_parameters(model):
    """SampleStage's tensor arguments after `white_bg`, and their names on the port's side."""
    from hyperreel_amd.train import grid_parameters
    vm = model.color_model.net
    params, names = [vm.basis_mat.weight, *grid_parameters(vm)], ['basis'] + GRID_NAMES
    if model._hc.color_table_views > 0:
        types = [e['type'] for e in model.cfg['embedding']['embeddings'].values()]
        params.append(model.embedding_model.embeddings[types.index('color_transform')].color_embedding)
        names.append('table')
    return params, names


def _compare_leaves(rep, grads, video, n_den, params, names):
    for what, p in zip(names, params):
        if p.numel() == 0:
            continue
        want = grads.get(what)
        if what in GRID_NAMES and (want is None or not np.abs(want).max() > 0):
            # only a plane pair the video net never samples (no density components) may go without a gradient
            assert video and n_den[int(what[-1])] == 0, f'{rep.title}: {what}: the reference gradient is identically zero'
            assert p.grad is None or not p.grad.abs().max().item() > 0, what
            continue
        assert want is not None and p.grad is not None, what
        assert bool(torch.isfinite(p.grad).all()), what
        rep.grad(what, _np(p.grad), want)


def _check_stage(name, n, white, deterministic=False):
    from hyperreel_amd import train as T
    branch = _assert_branch(name, n, deterministic)
    ref = _stage_reference(name, n, white)
    fn = _model(name, deterministic)
    model = fn.model
    h = model.native()
    hc = model._hc
    assert (hc.z_channels, hc.preds_per_z) == (ref.z, ref.p)
    rays = torch.from_numpy(ref.rays).cuda()
    head = torch.from_numpy(ref.head0).cuda().requires_grad_(True)
    params, names = _stage_parameters(model)
    rgb = T.SampleStage.apply(h, rays, head, bool(white), *params)
    (rgb * torch.from_numpy(ref.G).cuda()).sum().backward()
    torch.cuda.synchronize()

    rep = _Report(f'{name} n={ref.rays.shape[0]} white={white} stage [zp {branch["zp"]}, {"ray" if branch["thread_per_ray"] else "lanes"}, '
                  f'{branch["plane_class"]}, {"keyed" if branch["keyed"] else "static"}, {branch["phase_b"]}]')
    rep.forward(_np(rgb), ref.rgb)
    assert head.grad is not None and bool(torch.isfinite(head.grad).all())
    got_h, ref_h = _np(head.grad).reshape(-1, ref.z, ref.p), ref.d_head.reshape(-1, ref.z, ref.p)
    live = 0
    for col in range(ref.p):                              # every head column on its own scale (offsets, sigma, colour ...)
        if np.abs(ref_h[..., col]).max() > 0:
            rep.grad(f'd_head[{col}]', got_h[..., col], ref_h[..., col])
            live += 1
        else:
            assert not got_h[..., col].any(), f'd head column {col}: the reference is identically zero'
    assert live >= 3
    _compare_leaves(rep, ref.grads, ref.video, ref.n_den, params, names)
    rep.finish()
    return ref


@pytest.mark.parametrize('white', [0, 1])
@pytest.mark.parametrize('case', list(BRANCH))
def test_sample_stage_matches_autograd_with_the_head_supplied(case, white):
    """Section 1: SampleStage on the model's handle and parameters against the port, both fed the port's own head."""
    _check_stage(case, _scene(case).rays.shape[0], white)


def _mlp_layers(net):
    n = len(net.layers)
    return [(layer[0] if i < n - 1 else layer) for i, layer in enumerate(net.layers)]


@pytest.mark.parametrize('white', [0, 1])
@pytest.mark.parametrize('case', list(BRANCH))
def test_forward_train_matches_autograd_end_to_end(case, white):
    """Section 2: forward_train at mlp_precision='fp32' against the port run end to end: what section 1 compares (without dL/d head), plus the
    gradient of every weight and bias of the ray MLP and of a cascade's point MLP.

    shiny_z_tensorf_cascaded holds 1e-3 on every tensor but two: point_mlp.4.bias is 5.1e-3 of the tensor's largest reference entry off
    (|err| 1.072e-3 vs 2.094e-1) and point_mlp.4.weight 5.0e-3 (3.539e-4 vs 7.081e-2), on both backgrounds; the same model's stage-level
    check and coarse rows sit at 1e-6.  The whole error is row 16 of layer 4 (the next entry of the bias gradient is 7e-7 off): one
    LeakyReLU of the point MLP's 2 304 rows x 256 units x 5 layers takes the other branch -- row 187, unit 16 of layer 4 is +3.6e-8 in the
    port and -7.5e-9 through HipLinear, among activations of up to 5.2 that the two forwards compute 4.8e-6 apart and that an exact
    (float64) evaluation of the device's own inputs puts within 1.0e-8 of zero: the sign is below the rounding of either fp32 GEMM, no other
    activation of the network differs in sign, and there is no kernel arithmetic to correct.  It is the reference's own fp32 noise, measured
    on the port alone against its unmoved evaluation (tools/port_ulp_noise.py): with the rays and every parameter moved DOWN by one fp32 ulp the port flips the same
    unit and moves point_mlp.4.bias by 5.12e-3 of its largest entry (entry 16) and point_mlp.4.weight by 5.00e-3 (row 16) -- the device's
    figures -- and layers 0 to 3 by 3.8e-4 to 9.4e-4 at the entries where the device differs most (bias entries 40, 27, 124); moved UP,
    rays only or parameters only up: nothing above 1e-4; parameters only down, and 2 of 8 draws with a random direction per element: unit
    112 flips instead, 5.75e-4 (weight) and 5.01e-4 (bias).  Those two tensors are therefore held to 4 x the measured noise, 2.0e-2 and
    2.05e-2 (E2E_NOISE_BARS: the device sits at 0.25 of it); every other tensor of the case keeps 1e-3, as does every other case."""
    branch = _assert_branch(case)
    sc = _scene(case)
    n = sc.rays.shape[0]
    kept = _stage_reference(case, n, white).kept         # the rays whose reference gradient is finite
    rays = np.ascontiguousarray(sc.rays[kept])
    G = np.random.default_rng(3).standard_normal((rays.shape[0], 3)).astype(np.float32)
    rgb_ref, ref = _reference_grads(sc, rays, G, white)
    assert all(g is None or np.isfinite(g).all() for g in ref.values()), case
    coarse, hc = _levels(sc)

    fn = _model(case)
    model = fn.model
    rgb = model.forward_train(torch.from_numpy(rays).cuda(), white_bg=bool(white))
    assert rgb.requires_grad
    (rgb * torch.from_numpy(G).cuda()).sum().backward()
    torch.cuda.synchronize()

    rep = _Report(f'{case} n={rays.shape[0]} white={white} end to end [zp {branch["zp"]}]')
    rep.forward(_np(rgb), rgb_ref)
    params, names = _stage_parameters(model)
    _compare_leaves(rep, ref, bool(hc.video), list(hc.n_den), params, names)
    types = [e['type'] for e in model.cfg['embedding']['embeddings'].values()]
    lvl0 = coarse if coarse is not None else hc
    nets = []
    if lvl0.mlp_layers > 0:
        nets.append(('mlp', '', model.embedding_model.embeddings[types.index('ray_prediction')].net))
    else:
        assert not any(k.startswith('w') for k in ref), case          # ZeroMLP: no ray MLP on either side
    if coarse is not None:
        nets.append(('point_mlp', 'p', model.embedding_model.embeddings[types.index('point_prediction')].net))
    bars = E2E_NOISE_BARS.get(case, {})
    for what, prefix, net in nets:
        layers = _mlp_layers(net)
        assert len(layers) == len([k for k in ref if k.startswith(prefix + 'w')])
        if what == 'mlp':
            assert (layers[0].weight.shape[0], len(layers)) == (lvl0.mlp_hidden, lvl0.mlp_layers)
        for i, lin in enumerate(layers):
            for kind, p, want in (('weight', lin.weight, ref[f'{prefix}w{i}']), ('bias', lin.bias, ref[f'{prefix}b{i}'])):
                rep.grad(f'{what}.{i}.{kind}', _np(p.grad), want, tol=max(1e-3, bars.get(f'{what}.{i}.{kind}', 0.0)))
    rep.finish()


@pytest.mark.parametrize('case', CASCADES)
def test_coarse_rows_match_autograd(case):
    """Coarse level of a point_prediction cascade on its own (hr_rows_kernel / hr_rows_bwd_kernel): the rows handed to the point MLP against the
    port's `_rows`, and the gradient they send back to the ray MLP's raw head, per head column."""
    from hyperreel_amd import train as T
    _assert_branch(case)
    sc = _scene(case)
    coarse, fine = _levels(sc)
    port = TorchPort(sc.cfg, sc.dataset, sc.state_dict, iteration=sc.iteration)
    n = sc.rays.shape[0]
    rays = torch.from_numpy(sc.rays)
    with torch.no_grad():
        head0 = torch.zeros(n, coarse.z_channels * coarse.preds_per_z) if port.o.zero_net else port._mlp(port._param_pe(rays))
    head = head0.clone().requires_grad_(True)
    rows_ref = port.embed(rays, head=head)['_rows']
    G = torch.randn(rows_ref.shape, generator=torch.Generator().manual_seed(5))
    (rows_ref * G).sum().backward()
    assert rows_ref.shape == (n * coarse.z_channels, fine.casc_row_dim)
    ok = torch.isfinite(head.grad).all(-1)
    assert int((~ok).sum()) <= MAX_DROPPED
    ref = head.grad.numpy()

    fn = _model(case)
    h = fn.model.native()
    dhead = head0.cuda().requires_grad_(True)
    rows = T.CoarseRows.apply(h, rays.cuda(), dhead, coarse.z_channels, fine.casc_row_dim)
    (rows * G.cuda()).sum().backward()
    torch.cuda.synchronize()
    keep = ok.numpy()
    rep = _Report(f'{case} n={n} coarse rows [zp {train_branch(coarse, n)["zp"]}]')
    rep.forward(_np(rows).reshape(n, -1)[keep], rows_ref.detach().numpy().reshape(n, -1)[keep], 'rows')
    got = _np(dhead.grad)
    assert np.isfinite(got[keep]).all()
    if np.abs(ref[keep]).max() == 0:                      # a ZeroMLP ray level has a head nobody reads back
        assert port.o.zero_net and not got[keep].any()
        rep.finish()
        return
    P = coarse.preds_per_z
    ref_c, got_c = ref.reshape(n, coarse.z_channels, P)[keep], got.reshape(n, coarse.z_channels, P)[keep]
    live = 0
    for col in range(P):
        if np.abs(ref_c[..., col]).max() > 0:
            rep.grad(f'd_head[{col}]', got_c[..., col], ref_c[..., col])
            live += 1
        else:
            assert not got_c[..., col].any(), col
    assert live >= 1
    rep.finish()


RAGGED = ['shiny_z_plane_tiny',            # 32 rays per lanes workgroup
          'technicolor_z_plane_small',     # keyframe net: bucket kernel and grouped order
          'catacaustics_voxel']            # 16 rays per wavefront, one thread per ray


@pytest.mark.parametrize('white', [0, 1])
@pytest.mark.parametrize('n', [1, 15, 17, 33, 95])
@pytest.mark.parametrize('case', RAGGED)
def test_ragged_batches_match_autograd(case, n, white):
    """Section 3: ray counts that are no multiple of the rays per workgroup (or wavefront) of any of the stage's kernels."""
    ref = _check_stage(case, n, white)
    assert ref.dropped == 0 and ref.rays.shape[0] == n


@pytest.mark.parametrize('deterministic', [False, True])
@pytest.mark.parametrize('case', RAGGED)
def test_an_empty_batch_gives_zero_gradients(case, deterministic):
    """forward_train on no rays, the gradient buffers poisoned: the call succeeds, rgb is (0, 3), every gradient is finite and exactly zero."""
    from hyperreel_amd import train as T
    sc = _scene(case)
    fn = _model(case, deterministic)
    model = fn.model
    rays = torch.zeros((0, sc.rays.shape[1]), dtype=torch.float32, device='cuda')
    T.SampleStage.poison_outputs = True
    try:
        rgb = model.forward_train(rays, white_bg=False)
        assert tuple(rgb.shape) == (0, 3) and rgb.requires_grad
        (rgb * torch.zeros((0, 3), device='cuda')).sum().backward()
        torch.cuda.synchronize()
    finally:
        T.SampleStage.poison_outputs = False
    params, names = _stage_parameters(model)
    for what, p in zip(names, params):
        if p.numel():
            assert p.grad is not None, what
    seen = 0
    for what, p in fn.named_parameters():
        if p.grad is None:
            continue
        seen += 1
        assert bool(torch.isfinite(p.grad).all()) and not bool(p.grad.any()), what
    assert seen >= 3


@pytest.mark.parametrize('case', DETERMINISTIC)
def test_the_deterministic_build_on_the_same_branches(case):
    """Section 4: train_det_kernel.hip (64-bit fixed-point sums, the global-atomics kernel for everything): two evaluations agree bit for bit
    in every gradient, and lie within 1e-5 of the tensor's largest entry of the default mode's (the bar of
    test_gpu_train.py::test_deterministic_gradients_equal_the_default_ones_to_rounding), at |dL/d rgb| ~ 1."""
    _assert_branch(case)
    assert _assert_branch(case, deterministic=True)['phase_b'] == 'atomics'
    sc = _scene(case)
    rays = torch.from_numpy(sc.rays).cuda()
    G = torch.from_numpy(np.random.default_rng(3).standard_normal((rays.shape[0], 3)).astype(np.float32)).cuda()

    def grads(det):
        fn = _model(case, det)
        (fn.model.forward_train(rays, white_bg=False) * G).sum().backward()
        torch.cuda.synchronize()
        return {n: _np(p.grad).copy() for n, p in fn.named_parameters() if p.grad is not None}
    d0, d1, f = grads(True), grads(True), grads(False)
    assert set(d0) == set(f) and len(d0) >= 5
    worst = ('', 0.0)
    bad = []
    for n in d0:
        assert torch.equal(torch.from_numpy(d0[n]), torch.from_numpy(d1[n])), n
        if d0[n].size == 0:                       # (plane pairs without appearance components carry empty tensors)
            continue
        assert np.isfinite(d0[n]).all() and np.isfinite(f[n]).all(), n
        scale = max(float(np.abs(f[n]).max()), 1e-30)
        r = float(np.abs(d0[n] - f[n]).max()) / (1e-5 * scale)
        worst = max(worst, (n, r), key=lambda t: t[1])
        if not r <= 1.0:
            bad.append((n, r))
    print(f'{case} deterministic vs default: worst {worst[0]} at {worst[1]:.3f} of its bar')
    assert not bad, bad
