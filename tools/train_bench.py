"""Training-step timing: one optimizer step of the reference's loop (nlf/__init__.py:634-709: forward,
MSE image loss, backward, Adam) at the shipped batch size (conf/experiment/training/*.yaml: batch_size 16384) on the
full-size synthetic scene of bench.py.

    python tools/train_bench.py [--model donerf_sphere] [--batch 16384] [--steps 30] [--torch-gpu] [--hip-loss]

Prints one JSON line: ms per step of the HIP training path (hr_train_features + HipLinear MFMA GEMMs + hr_train_forward /
hr_train_backward) with the sample stage's forward and backward kernels timed on their own, and with --torch-gpu the
same step of the PyTorch-ROCm restatement of the reference (oracle/torch_port.py, autograd over grid_sample / sort /
cumprod) on the same GPU, weights and rays.  The oracle is only the comparator here, never the thing shipped.  --hip-loss: the image loss of the
step through hyperreel_amd.losses (hr_image_loss, weight 1) instead of the torch expression; the default stays the torch expression.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

from hyperreel_amd import config as C          # noqa: E402
from hyperreel_amd import scenes               # noqa: E402
from hyperreel_amd import lib as _hrlib        # noqa: E402
if os.environ.get('HR_LIB'):
    _hrlib.LIB_PATH = os.path.abspath(os.environ['HR_LIB'])     # a measurement variant (tools/build_variant.py)


def timed(fn, reps, warm=3, rounds=2):
    """ms per call: the better of `rounds` timed loops (a loop of 15 steps is 30-60 ms: one clock ramp or one allocator hiccup of the
    box moved a family's figure by a third between two runs of bench.py)"""
    for _ in range(warm):
        fn()
    best = float('inf')
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / reps * 1e3)
    return best


def train_step_figures(model_name='donerf_sphere', batch=16384, steps=30, torch_gpu=False, blas=True, hip_loss=False):
    """ms per optimizer step of the HIP training path and of its parts (bench.py quotes this for its `train_step` key)"""
    import types
    args = types.SimpleNamespace(model=model_name, batch=batch, steps=steps, torch_gpu=torch_gpu)
    from hyperreel_amd.render import build_render_fn
    from hyperreel_amd.train import SampleStage, grid_parameters, mlp_forward, ray_features
    cfg, ds = C.model_config(args.model), C.dataset_scalars(args.model)
    sd = scenes.make_state_dict(cfg, ds, None, seed=7, density='dense', app_scale=1.0)
    grid = [int(v) for v in sd['model.color_model.net.gridSize']]
    fn = build_render_fn(cfg, dataset=ds, grid_size=grid)
    fn.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    fn.train()
    model = fn.model
    rays_np = scenes.benchmark_rays(args.model, 800, 800, frame=7)
    idx = np.random.default_rng(0).choice(rays_np.shape[0], args.batch, replace=False)     # a training batch: random pixels
    rays = torch.from_numpy(np.ascontiguousarray(rays_np[idx])).cuda()
    target = torch.rand((args.batch, 3), device='cuda')
    params = [p for p in model.parameters() if p.requires_grad]
    from hyperreel_amd.optim import HipAdam
    opt = HipAdam(params, lr=1e-3, betas=(0.9, 0.99), eps=1e-8)              # the reference's Adam (utils/__init__.py:61-66) as one launch

    if hip_loss:
        from hyperreel_amd.losses import get_loss
        loss_fn, weight = get_loss({'type': 'mse'}), torch.ones((args.batch, 1), device='cuda')
        image_loss = lambda rgb: loss_fn.step_loss(rgb, target, weight)[0]
    else:
        image_loss = lambda rgb: ((rgb - target) ** 2).mean()

    def step():
        opt.zero_grad(set_to_none=True)
        loss = image_loss(model.forward_train(rays, white_bg=False))
        loss.backward()
        opt.step()

    ms_step = timed(step, args.steps, warm=6, rounds=3)         # (the first figure of the process: allocator and optimizer state settle in the warm-up)
    opt_hip, opt = opt, torch.optim.Adam(params, lr=1e-3, betas=(0.9, 0.99), eps=1e-8)      # the same step with torch's own (foreach) Adam
    ms_step_torch_adam = timed(step, args.steps)
    opt = opt_hip

    def fwd_bwd():
        for p in params:
            p.grad = None
        image_loss(model.forward_train(rays, white_bg=False)).backward()

    ms_fwd_bwd = timed(fwd_bwd, args.steps)
    # the sample stage alone
    h, hc = model._native, model._hc
    types = [e['type'] for e in cfg['embedding']['embeddings'].values()]
    pred = model.embedding_model.embeddings[types.index('ray_prediction')]
    with torch.no_grad():
        head = mlp_forward(pred.net, ray_features(h, rays, hc.mlp_in), hc.mlp_skip_mask)
    vm = model.color_model.net
    grids = grid_parameters(vm)
    with torch.no_grad():
        ms_stage_fwd = timed(lambda: SampleStage.apply(h, rays, head, False, vm.basis_mat.weight, *grids), args.steps)
    head_g = head.clone().requires_grad_(True)
    d_rgb = torch.rand((args.batch, 3), device='cuda')

    def stage_both():
        SampleStage.apply(h, rays, head_g, False, vm.basis_mat.weight, *grids).backward(d_rgb)

    ms_stage_both = timed(stage_both, args.steps)
    # the MLP alone, forward + backward: the split-precision MFMA GEMMs (HipLinear) next to the same layers through
    # torch's F.linear (rocBLAS / hipBLASLt fp32), the comparator they replaced
    import torch.nn.functional as F
    feats = ray_features(h, rays, hc.mlp_in)
    d_head = torch.rand_like(head) * 1e-3

    def mlp_hip():
        for p in params:
            p.grad = None
        mlp_forward(pred.net, feats, hc.mlp_skip_mask).backward(d_head)

    def mlp_blas():
        for p in params:
            p.grad = None
        x, inp, n = feats, feats, len(pred.net.layers)
        for i, layer in enumerate(pred.net.layers):
            lin = layer[0] if i < n - 1 else layer
            if (hc.mlp_skip_mask >> i) & 1:
                x = torch.cat([inp, x], -1)
            x = F.linear(x, lin.weight, lin.bias)
            if i < n - 1:
                x = F.leaky_relu(x, 0.01)
        x.backward(d_head)

    ms_mlp_hip = timed(mlp_hip, args.steps)
    ms_mlp_blas = timed(mlp_blas, args.steps) if blas else float('nan')
    # the opt-in forms of the step: the MLP's forward as one launch (train_fused_mlp), and the deterministic mode (64-bit fixed-point sums)
    from hyperreel_amd.train import mlp_forward_fused

    def mlp_fused():
        for p in params:
            p.grad = None
        mlp_forward_fused(h, rays, feats, pred.net, hc.mlp_skip_mask, hc.z_channels * hc.preds_per_z).backward(d_head)

    ms_mlp_fused = timed(mlp_fused, args.steps) if (hc.mlp_hidden == 256 and not model._coarse_hc) else float('nan')
    model.train_fused_mlp = True
    ms_step_fused = timed(step, args.steps)
    model.train_fused_mlp = False
    model.set_train_deterministic(True)
    ms_step_det = timed(step, args.steps)
    model.set_train_deterministic(False)
    out = {'workload': f'{args.model}: training step, batch {args.batch} rays x {hc.z_channels} samples, grid {grid[0]}x{grid[1]}x{grid[2]}',
           'hip_ms_per_step': round(ms_step, 3), 'hip_ms_forward_backward': round(ms_fwd_bwd, 3),
           'hip_ms_sample_stage_forward': round(ms_stage_fwd, 3),
           'hip_ms_sample_stage_backward': round(ms_stage_both - ms_stage_fwd, 3),
           'hip_ms_mlp_forward_backward': round(ms_mlp_hip, 3), 'rocblas_ms_mlp_forward_backward': round(ms_mlp_blas, 3),
           'hip_krays_per_s': round(args.batch / ms_step, 1),
           'torch_optim_adam_ms_per_step': round(ms_step_torch_adam, 3),
           'opt_in': {'fused_mlp_forward_ms_per_step': round(ms_step_fused, 3), 'fused_mlp_forward_backward_ms': round(ms_mlp_fused, 3),
                      'deterministic_ms_per_step': round(ms_step_det, 3)}}

    if args.torch_gpu:
        from torch_port import TorchPort
        port = TorchPort(cfg, ds, sd, device='cuda')
        leaves = [t.requires_grad_(True) for grp in (port.d_a, port.d_b, port.a_a, port.a_b) for t in grp if t.numel() > 0]
        leaves += [port.basis.requires_grad_(True)] + [t.requires_grad_(True) for wb in port.layers for t in wb]
        opt2 = torch.optim.Adam(leaves, lr=1e-3)

        def step_ref():
            opt2.zero_grad(set_to_none=True)
            loss = ((port.color(port.embed(rays), train=True, white_bg=False) - target) ** 2).mean()
            loss.backward()
            opt2.step()

        ms_ref = timed(step_ref, max(5, args.steps // 3))
        out['torch_rocm_port_ms_per_step'] = round(ms_ref, 3)
        out['speedup_vs_torch_rocm_port'] = round(ms_ref / ms_step, 2)
    if not blas:
        out.pop('rocblas_ms_mlp_forward_backward')
    if hip_loss:
        out['image_loss'] = 'hr_image_loss'
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', default='donerf_sphere')
    ap.add_argument('--batch', type=int, default=16384)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--torch-gpu', action='store_true')
    ap.add_argument('--hip-loss', action='store_true')
    args = ap.parse_args()
    print(json.dumps(train_step_figures(args.model, args.batch, args.steps, args.torch_gpu, hip_loss=args.hip_loss)))


if __name__ == '__main__':
    main()
