"""Cost of the training image loss: ms per loss forward + backward at the shipped batch (B = 16 384 rays), eager and replayed from a
captured hipGraph, of hyperreel_amd.losses (hr_image_loss: one call for the loss, train/psnr's squared error and d loss / d pred) beside
the torch expressions it replaces on the same device:
  torch_parent         ((pred - target) ** 2).mean() and its autograd backward -- what tools/train_bench.py and the tests wrote;
  torch_training_step  INRSystem.training_step's form (nlf/__init__.py:665-668): the two multiplies by the weight, the mean squared error,
                       its backward, and psnr_gpu's separate squared-error pass.
Then the whole training step (forward_train, loss, backward, HipAdam) with either loss.
python tools/loss_ab.py [--batch B] [--seconds S] [--rounds R] [--model NAME] [--no-step]
Each timed window is preceded by a time-based warm-up of the same call and lasts --seconds; the variants alternate inside a round and the
best window of each is reported beside all of them.  Nothing is asserted: one JSON line is printed.  Measurement aid (GPU box)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hyperreel_amd import config as C, scenes  # noqa: E402
from hyperreel_amd.losses import get_loss  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=16384)
ap.add_argument('--seconds', type=float, default=0.5, help='length of a timed window, and of the warm-up before it')
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--model', default='donerf_sphere')
ap.add_argument('--no-step', action='store_true', help='skip the whole-training-step comparison')
args = ap.parse_args()
assert torch.cuda.is_available(), 'tools/loss_ab.py measures on the HIP device'
B = args.batch


def timed(step, seconds):
    """ms per call: warm up for `seconds`, then time whole batches of calls until `seconds` have passed."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        step()
        torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(20):
            step()
        torch.cuda.synchronize()
        n += 20
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e3


def graph_of(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def alternate(steps):
    ms = {}
    for _ in range(args.rounds):
        for k, f in steps.items():
            ms.setdefault(k, []).append(timed(f, args.seconds))
    return {k: {'best': round(min(v), 4), 'all': [round(x, 4) for x in v]} for k, v in ms.items()}


rng = np.random.default_rng(0)
gt = torch.from_numpy(rng.random((B, 3)).astype(np.float32)).cuda()
pred = (gt + 0.1 * torch.randn((B, 3), device='cuda')).requires_grad_(True)
weight = torch.ones((B, 1), device='cuda')
loss_fn = get_loss({'type': 'mse'})


def hip():
    pred.grad = None
    loss, sse = loss_fn.step_loss(pred, gt, weight)
    loss.backward()


def torch_parent():
    pred.grad = None
    ((pred - gt) ** 2).mean().backward()


def torch_training_step():
    pred.grad = None
    loss = torch.nn.functional.mse_loss(pred * weight, gt * weight)
    psnr_mse = torch.mean((pred.detach() - gt) ** 2)          # psnr_gpu's pass (metrics.py:37-45), before its log10
    loss.backward()
    return psnr_mse


res = {'batch': B, 'seconds': args.seconds, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0)}
eager = {'hip': hip, 'torch_parent': torch_parent, 'torch_training_step': torch_training_step}
hip(); g_hip = pred.grad.clone()
torch_training_step(); g_torch = pred.grad.clone()
res['grad_max_abs_difference_hip_vs_torch'] = float((g_hip - g_torch).abs().max())
res['loss_forward_backward_ms_eager'] = alternate(eager)
graphs, why = {}, {}
for k, f in eager.items():
    try:
        graphs[k] = graph_of(f)
    except Exception as e:                                   # a form that cannot be captured is reported, not timed
        why[k] = f'not measured: {type(e).__name__}: {str(e)[:120]}'
res['loss_forward_backward_ms_graph'] = {**alternate({k: g.replay for k, g in graphs.items()}), **why}

if not args.no_step:
    from hyperreel_amd.optim import HipAdam
    from hyperreel_amd.render import build_render_fn
    cfg, ds = C.model_config(args.model), C.dataset_scalars(args.model)
    sd = scenes.make_state_dict(cfg, ds, None, seed=7, density='dense', app_scale=1.0)
    fn = build_render_fn(cfg, dataset=ds, grid_size=[int(v) for v in sd['model.color_model.net.gridSize']])
    fn.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    fn.train()
    model = fn.model
    rays_np = scenes.benchmark_rays(args.model, 800, 800, frame=7)
    rays = torch.from_numpy(np.ascontiguousarray(rays_np[rng.choice(rays_np.shape[0], B, replace=False)])).cuda()
    params = [p for p in model.parameters() if p.requires_grad]
    opt = HipAdam(params, lr=1e-3, betas=(0.9, 0.99), eps=1e-8)

    def step_with(image_loss):
        def step():
            opt.zero_grad(set_to_none=True)
            image_loss(model.forward_train(rays, white_bg=False)).backward()
            opt.step()
        return step

    def loss_and_psnr_torch(rgb):                            # training_step's two passes
        torch.mean((rgb.detach() - gt) ** 2)
        return torch.nn.functional.mse_loss(rgb * weight, gt * weight)

    res['model'] = args.model
    res['training_step_ms'] = alternate({'torch_parent_loss': step_with(lambda rgb: ((rgb - gt) ** 2).mean()),
                                         'hip_loss': step_with(lambda rgb: loss_fn.step_loss(rgb, gt, weight)[0]),
                                         'torch_training_step_loss': step_with(loss_and_psnr_torch)})
print(json.dumps(res), flush=True)
