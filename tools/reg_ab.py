"""What the TensoRF regulariser costs beside the training step, and what the one-call form (hr_tensorf_reg,
hyperreel_amd.train.HipTensoRFRegularizer.accumulate) saves over the per-plane path (PlaneReg / tv_loss / l1_mean: one forward and one
backward launch per plane, torch ops between them, autograd's add into .grad).

    python tools/reg_ab.py [--models donerf_sphere neural_3d_z_plane] [--batch 16384] [--steps 20] [--rounds 5] [--out FILE]

Per model, at its shipped final grid (DoNeRF: 600^3) on the synthetic scene of bench.py, ms per call, the median over `rounds` windows of
`steps` calls each, the variants' windows INTERLEAVED (variant A's window, B's, C's, then again), every window ended by a device synchronise:
  reg_alone    the regulariser on its own, adding into existing gradients: per_plane | fused, eager and replayed from a graph;
  step         the whole optimizer step (forward, hr_image_loss MSE, backward, regulariser, capturable HipAdam) on a fixed batch: none |
               per_plane | fused eager, none | fused replayed (GraphedStep).  `none` is the step without a regulariser: the differences to
               it are what the regulariser costs there.  The per-plane path inside a replayed step is not measured.
Both forms use the same weights (iteration 0 of conf/experiment/regularizers/tensorf/tv_4000_*.yaml).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hyperreel_amd import config as C          # noqa: E402
from hyperreel_amd import scenes               # noqa: E402

REG_CFG = dict(type='tensorf', weight=dict(type='exponential_decay', start=1.0, decay=1.0, num_epochs=100), update_AlphaMask_list=[4000, 8000],
               lr_decay_target_ratio=0.1, n_iters=30000, total_num_tv_iters=60000, L1_weight_initial=8e-5, L1_weight_rest=4e-5,
               TV_weight_density=0.0125, TV_weight_app=0.0125)


def interleaved(variants, steps, rounds, warm=3):
    """{name: median ms per call} with the variants' windows interleaved."""
    for fn in variants.values():
        for _ in range(warm):
            fn()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / steps * 1e3)
    return {k: round(statistics.median(v), 4) for k, v in ms.items()}, {k: [round(x, 4) for x in v] for k, v in ms.items()}


def graphed(fn, dev):
    """fn recorded once (after three eager calls on a side stream) -> a callable that replays it."""
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def measure(model_name, batch, steps, rounds):
    from hyperreel_amd.optim import HipAdam
    from hyperreel_amd.render import build_render_fn
    from hyperreel_amd.train import HipTensoRFRegularizer
    cfg, ds = C.model_config(model_name), C.dataset_scalars(model_name)
    sd = scenes.make_state_dict(cfg, ds, None, seed=7, density='dense', app_scale=1.0)
    grid = [int(v) for v in sd['model.color_model.net.gridSize']]
    fn = build_render_fn(cfg, dataset=ds, grid_size=grid)
    fn.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    fn.train()
    model, net = fn.model, fn.model.color_model.net
    dev = next(model.parameters()).device
    rays_np = scenes.benchmark_rays(model_name, 800, 800, frame=7)
    idx = np.random.default_rng(0).choice(rays_np.shape[0], batch, replace=False)
    rays = torch.from_numpy(np.ascontiguousarray(rays_np[idx])).cuda()
    target = torch.rand((batch, 3), device='cuda')
    params = [p for p in model.parameters() if p.requires_grad]
    reg = HipTensoRFRegularizer(model, REG_CFG, 4000)
    reg.set_iter(0)
    reg.sync()
    w = reg.weights
    elements = sum(p.numel() for p, *_ in reg.terms())

    def per_plane():
        return w[0] * net.density_L1() + w[1] * net.TV_loss_density(None) + w[2] * net.TV_loss_app(None)

    # ---- the regulariser alone, adding into gradients that exist (as behind the image loss's backward)
    for p, *_ in reg.terms():
        p.grad = torch.zeros_like(p)
    alone = {'per_plane_eager': lambda: per_plane().backward(), 'fused_eager': reg.accumulate}
    alone['per_plane_replayed'] = graphed(alone['per_plane_eager'], dev)
    alone['fused_replayed'] = graphed(alone['fused_eager'], dev)
    alone_ms, alone_all = interleaved(alone, steps, rounds)
    # the two forms agree: value and gradient of one call each on fresh gradients
    for p, *_ in reg.terms():
        p.grad = torch.zeros_like(p)
    v_fused = float(reg.accumulate())
    g_fused = [p.grad.clone() for p, *_ in reg.terms()]
    for p, *_ in reg.terms():
        p.grad = torch.zeros_like(p)
    loss = per_plane()
    loss.backward()
    v_plane = float(loss.detach())
    del loss            # (a live loss keeps the planes' AccumulateGrad nodes, made on this stream, alive into the recordings below)
    agree = max(float((a - p.grad).abs().max()) / max(float(p.grad.abs().max()), 1e-30) for a, (p, *_) in zip(g_fused, reg.terms()))

    # ---- the whole step on a fixed batch, replayed: GraphedStep itself, its sampler replaced by a copy of the fixed batch
    from hyperreel_amd.losses import HipImageLoss
    from hyperreel_amd.train import GraphedStep
    loss_fn, weight = HipImageLoss('mse'), torch.ones((batch, 1), device='cuda')

    class FixedBatch:
        device, ray_dim = dev, rays.shape[1]

        @staticmethod
        def sample(batch_size, step_tensor=None, seed=0, out=None):
            out['coords'].copy_(rays); out['rgb'].copy_(target); out['weight'].copy_(weight)
            return out

    new_opt = lambda: HipAdam(params, lr=1e-3, betas=(0.9, 0.99), eps=1e-8, capturable=True)
    recorded = {'none_replayed': GraphedStep(model, new_opt(), FixedBatch, batch, loss=loss_fn, white_bg=False, warmup=3),
                'fused_replayed': GraphedStep(model, new_opt(), FixedBatch, batch, loss=loss_fn, white_bg=False, warmup=3, regularizer=reg)}
    rep_ms, rep_all = interleaved({k: g.step for k, g in recorded.items()}, steps, rounds, warm=4)
    for g in recorded.values():
        g.close()

    # ---- ... and eager
    def make_step(kind):
        opt = new_opt()

        def step():
            loss = loss_fn.step_loss(model.forward_train(rays, white_bg=False), target, weight)[0]
            if kind == 'per_plane':
                loss = loss + per_plane()
            opt.zero_grad(set_to_none=True)
            loss.backward()
            if kind == 'fused':
                reg.accumulate()
            opt.step()
        return step

    step_ms, step_all = interleaved({f'{k}_eager': make_step(k) for k in ('none', 'per_plane', 'fused')}, steps, rounds, warm=4)
    reg.close()
    return {'workload': f'{model_name}: grid {grid[0]}x{grid[1]}x{grid[2]}, {len(reg.terms())} regularised tensors, {elements} elements, batch {batch}',
            'reg_alone_ms': alone_ms, 'step_ms': {**step_ms, **rep_ms},
            'reg_cost_in_step_ms': {'per_plane_eager': round(step_ms['per_plane_eager'] - step_ms['none_eager'], 4),
                                    'fused_eager': round(step_ms['fused_eager'] - step_ms['none_eager'], 4),
                                    'fused_replayed': round(rep_ms['fused_replayed'] - rep_ms['none_replayed'], 4)},
            # one HBM read of every plane + one read-modify-write of its gradient, over the fused call's replayed time
            'fused_replayed_gbytes_per_s': round(12.0 * elements / (alone_ms['fused_replayed'] * 1e-3) / 1e9, 1),
            'value_fused': v_fused, 'value_per_plane': v_plane, 'max_rel_gradient_difference': agree,
            'windows_ms': {'reg_alone': alone_all, 'step': {**step_all, **rep_all}}, 'steps_per_window': steps, 'rounds': rounds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', nargs='+', default=['donerf_sphere', 'neural_3d_z_plane'])
    ap.add_argument('--batch', type=int, default=16384)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/reg_ab.py measures on the HIP device; none is visible')
    out = {'date': time.strftime('%Y-%m-%d'), 'device': torch.cuda.get_device_name(0), 'results': [measure(m, args.batch, args.steps, args.rounds) for m in args.models]}
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
