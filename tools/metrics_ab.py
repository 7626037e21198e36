"""Cost of scoring a frame: ms per call of hr_image_metrics (PSNR + SSIM sums, and the squared error alone), eager and replayed from a
captured hipGraph, beside (a) what the reference does -- the device-to-host copy of the frame plus the host SSIM, here the scipy oracle
of tests/metrics_oracle.py on the threads the process is given -- and (b) the render of the same frame.
python tools/metrics_ab.py [--seconds S] [--rounds R] [--host-reps N] [--out F]
Frames: 800x800, 1280x960, 1352x1014, 2048x1088 (DoNeRF sphere model, mlp_precision 'auto').  Each timed window is preceded by a
time-based warm-up of the same call and lasts --seconds.  Nothing is asserted: the numbers are printed.  Measurement aid (GPU box)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import metrics_oracle as MO  # noqa: E402
from hyperreel_amd import config as C, metrics, scenes  # noqa: E402
from hyperreel_amd.render import build_render_fn  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--seconds', type=float, default=0.5, help='length of a timed window, and of the warm-up before it')
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--host-reps', type=int, default=2)
ap.add_argument('--out', default='')
args = ap.parse_args()
FRAMES = [(800, 800), (960, 1280), (1014, 1352), (1088, 2048)]            # (h, w)
assert torch.cuda.is_available(), 'tools/metrics_ab.py measures on the HIP device'


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
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


cfg, ds = C.model_config('donerf_sphere'), C.dataset_scalars('donerf_sphere')
sd = scenes.make_state_dict(cfg, ds, None, seed=7, density='dense', app_scale=1.0)
fn = build_render_fn(cfg, dataset=ds, grid_size=[int(v) for v in sd['model.color_model.net.gridSize']])
fn.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
m = fn.model
res = []
for h, w in FRAMES:
    rays = torch.from_numpy(scenes.benchmark_rays('donerf_sphere', h, w, frame=7)).cuda()
    rgb = torch.empty((h * w, 3), device='cuda')
    m.render(rays, out=rgb)
    torch.cuda.synchronize()
    gt = torch.from_numpy(np.clip(rgb.cpu().numpy() + np.random.default_rng(1).normal(0, 0.02, (h * w, 3)), 0, 1).astype(np.float32)).cuda()
    out = torch.empty((4,), dtype=torch.float64, device='cuda')
    ws = torch.empty((metrics.workspace_doubles(h, w),), dtype=torch.float64, device='cuda')
    m._render_calls = 1000                       # past the calls on which render() polls the sticky bits (a synchronise each)
    steps = {'render': lambda: m.render(rays, out=rgb),
             'scores': lambda: metrics.image_scores(rgb, gt, h, w, out=out, workspace=ws),
             'sse_only': lambda: metrics.image_scores(rgb, gt, h, w, ssim=False, out=out, workspace=ws)}
    graphs = {k: graph_of(f) for k, f in steps.items()}
    ms = {}
    for _ in range(args.rounds):                 # the variants alternate inside a round
        for k, f in steps.items():
            ms.setdefault('eager_' + k, []).append(timed(f, args.seconds))
            ms.setdefault('graph_' + k, []).append(timed(graphs[k].replay, args.seconds))
    dev = metrics.scores_to_metrics(metrics.image_scores(rgb, gt, h, w), h, w)
    # (a) the reference's way: the frame to the host, then the host SSIM and PSNR
    host = []
    gt_np = gt.cpu().numpy()                     # the ground truth is on the host already in the reference's loop
    for _ in range(args.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = rgb.cpu().numpy()
        t1 = time.perf_counter()
        o = MO.scores(x, gt_np, h, w)
        host.append({'copy_ms': (t1 - t0) * 1e3, 'oracle_ms': (time.perf_counter() - t1) * 1e3})
    r = {'frame': f'{w}x{h}', 'pixels': h * w, 'threads': len(os.sched_getaffinity(0)), 'omp_num_threads': os.environ.get('OMP_NUM_THREADS'),
         'ms_best': {k: round(min(v), 4) for k, v in ms.items()}, 'ms_all': {k: [round(x, 4) for x in v] for k, v in ms.items()},
         'host_copy_ms_best': round(min(x['copy_ms'] for x in host), 3), 'host_oracle_ms_best': round(min(x['oracle_ms'] for x in host), 1),
         'device': dev, 'oracle': {'psnr': float(o['psnr']), 'ssim': o['ssim']}}
    print(json.dumps(r), flush=True)
    res.append(r)
    del graphs
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
