"""Does replaying the training step from one graph pay?  ms per optimizer step of three forms of the same step, in interleaved rounds in
one process, on the four families tools/train_bench.py times (full-size synthetic scenes, batch 16384):

  eager        the existing loop: DeviceRaySet.batch (the epoch's order) -> forward_train -> HipImageLoss -> backward -> HipAdam (host step count)
  eager_dev    the same loop with DeviceRaySet.sample(step_tensor=...) and HipAdam(capturable=True): what GraphedStep records, taken eagerly
  graph        hyperreel_amd.train.GraphedStep: one replay per step

    python tools/train_graph_ab.py [--models donerf_sphere,...] [--batch 16384] [--steps 20] [--rounds 7]

Every form trains its own copy of the model on the same device-resident set (4 images of 400 x 400 from the benchmark camera).  A round
times `steps` steps of each form in turn, synchronising before and after; `host_ms` is the time the Python loop itself took to enqueue the
steps (read before the closing synchronisation): where it equals the step time the form is host-bound.  Prints one JSON line per family:
median and min - max over the rounds.  Measurement aid (GPU box)."""
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

FAMILIES = ['donerf_sphere', 'technicolor_z_plane', 'neural_3d_z_plane', 'immersive_sphere']


def make_rayset(name, n_images=4, side=400):
    from hyperreel_amd.data import DeviceRaySet
    video = not name.startswith('donerf')
    rng = np.random.default_rng(0)
    images = rng.integers(0, 256, (n_images, side, side, 3), dtype=np.uint8)
    poses = []
    for i in range(n_images):
        d = 0.02 * i
        poses.append(scenes.look_at_pose((0.05 + d, 0.03, 1.0), (0.0, 0.0, -1.0)) if 'z_plane' in name
                     else scenes.look_at_pose((0.3, d, 0.0), (1.0, 0.1, 0.05)))
    focal = 0.5 * side / np.tan(0.5 * np.radians(40.0))
    K = np.array([[focal, 0, side / 2.0], [0, focal, side / 2.0], [0, 0, 1]], np.float32)
    times = [i / max(n_images - 1, 1) for i in range(n_images)] if video else None
    return DeviceRaySet(images, np.stack(poses), K, times, [0] * n_images if video else None, (side, side))


def make_model(name):
    from hyperreel_amd.render import build_render_fn
    cfg, ds = C.model_config(name), C.dataset_scalars(name)
    sd = scenes.make_state_dict(cfg, ds, None, seed=7, density='dense', app_scale=1.0)
    grid = [int(v) for v in sd['model.color_model.net.gridSize']]
    fn = build_render_fn(cfg, dataset=ds, grid_size=grid)
    fn.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    fn.train()
    return fn.model


def family(name, batch, steps, rounds):
    from hyperreel_amd.losses import HipImageLoss
    from hyperreel_amd.optim import HipAdam
    from hyperreel_amd.train import GraphedStep
    rs = make_rayset(name)
    loss_fn = HipImageLoss('mse')
    adam = lambda m, cap: HipAdam([p for p in m.parameters() if p.requires_grad], lr=1e-3, betas=(0.9, 0.99), eps=1e-8, capturable=cap)

    m1 = make_model(name)
    o1 = adam(m1, False)
    count = [0]
    per_epoch = len(rs) // batch

    def eager():
        i = count[0]
        count[0] += 1
        b = rs.batch(i % per_epoch, batch, epoch=i // per_epoch)
        loss, _ = loss_fn.step_loss(m1.forward_train(b['coords'], white_bg=False), b['rgb'], b['weight'])
        o1.zero_grad(set_to_none=True)
        loss.backward()
        o1.step()

    m2 = make_model(name)
    o2 = adam(m2, True)
    out2 = {'coords': torch.empty((batch, rs.ray_dim), device='cuda'), 'rgb': torch.empty((batch, 3), device='cuda'), 'weight': torch.empty((batch, 1), device='cuda')}

    def eager_dev():
        b = rs.sample(batch, step_tensor=o2.step_tensor, seed=0, out=out2)
        loss, _ = loss_fn.step_loss(m2.forward_train(b['coords'], white_bg=False), b['rgb'], b['weight'])
        o2.zero_grad(set_to_none=True)
        loss.backward()
        o2.sync_hyperparameters()
        o2.step()

    m3 = make_model(name)
    o3 = adam(m3, True)
    for f in (eager, eager_dev):
        for _ in range(3):
            f()
    gs = GraphedStep(m3, o3, rs, batch, loss=loss_fn, seed=0, white_bg=False, warmup=3)
    forms = {'eager': eager, 'eager_dev': eager_dev, 'graph': gs.step}
    total = {k: [] for k in forms}
    host = {k: [] for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                f()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            total[k].append((t2 - t0) / steps * 1e3)
            host[k].append((t1 - t0) / steps * 1e3)
    res = {'model': name, 'batch': batch, 'steps_per_round': steps, 'rounds': rounds}
    for k in forms:
        res[k] = {'ms': round(statistics.median(total[k]), 4), 'min': round(min(total[k]), 4), 'max': round(max(total[k]), 4),
                  'host_ms': round(statistics.median(host[k]), 4)}
    res['final_loss_graph'] = float(gs.step()['loss'])
    res['steps_done'] = {'eager_dev': o2.steps_done(), 'graph': o3.steps_done()}
    rs.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default=','.join(FAMILIES))
    ap.add_argument('--batch', type=int, default=16384)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    for name in args.models.split(','):
        print(json.dumps(family(name, args.batch, args.steps, args.rounds)), flush=True)


if __name__ == '__main__':
    main()
