"""Cost of the per-ray maps (hr_render_maps): ms per frame of render() against render(maps=('distances', 'points', 'acc')), eager and
replayed from a captured hipGraph, timed in alternation in one process.  python tools/maps_ab.py [--rounds R] [--steps S] [--out F]
Frames: DoNeRF 800x800 (hr_render) and Technicolor 2048x1088 (hr_render_frame), mlp_precision 'auto'.  Measurement aid (GPU box)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hyperreel_amd import config as C, scenes  # noqa: E402
from hyperreel_amd.render import build_render_fn  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--out', default='')
args = ap.parse_args()
MAPS = ('distances', 'points', 'acc')
FRAMES = [('donerf_sphere', 800, 800, False), ('technicolor_z_plane', 1088, 2048, True)]


def timed(step, steps):
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def graph_of(render):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        render()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        render()
    return g


res = []
for model, H, W, frame in FRAMES:
    cfg, ds = C.model_config(model), C.dataset_scalars(model)
    sd = scenes.make_state_dict(cfg, ds, None, seed=7, density='dense', app_scale=1.0)
    grid = [int(v) for v in sd['model.color_model.net.gridSize']]
    fn = build_render_fn(cfg, dataset=ds, grid_size=grid)
    fn.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    m = fn.model
    rays_np = scenes.benchmark_rays(model, H, W, frame=7)
    rays = torch.from_numpy(rays_np).cuda()
    t = float(rays_np[0, -1]) if frame else None
    B = rays.shape[0]
    rgb = torch.empty((B, 3), device='cuda')
    bufs = {'distances': torch.empty((B, 1), device='cuda'), 'points': torch.empty((B, 3), device='cuda'), 'acc': torch.empty((B, 1), device='cuda')}
    plain = lambda: m.render(rays, out=rgb, frame_time=t)
    maps = lambda: m.render(rays, out=rgb, frame_time=t, maps=MAPS, maps_out=bufs)
    plain()
    ref = rgb.clone()
    maps()
    torch.cuda.synchronize()
    same = bool(torch.equal(rgb, ref))
    m._render_calls = 1000                       # past the calls on which render() polls the sticky bits (a synchronise each)
    gp, gm = graph_of(plain), graph_of(maps)
    ms = {'eager': [], 'eager_maps': [], 'graph': [], 'graph_maps': []}
    for _ in range(args.rounds):
        ms['eager'].append(timed(plain, args.steps))
        ms['eager_maps'].append(timed(maps, args.steps))
        ms['graph'].append(timed(gp.replay, args.steps))
        ms['graph_maps'].append(timed(gm.replay, args.steps))
    best = {k: min(v) for k, v in ms.items()}
    r = {'model': model, 'frame': f'{W}x{H}', 'frame_path': frame, 'rays': B, 'rgb_bit_identical': same,
         'ms_best': {k: round(v, 4) for k, v in best.items()},
         'maps_cost_pct': {'eager': round(100.0 * (best['eager_maps'] / best['eager'] - 1.0), 2),
                           'graph': round(100.0 * (best['graph_maps'] / best['graph'] - 1.0), 2)},
         'ms_all': {k: [round(x, 4) for x in v] for k, v in ms.items()}}
    print(json.dumps(r), flush=True)
    res.append(r)
    del gp, gm, fn, m
    torch.cuda.empty_cache()
if args.out:
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
