"""Cost of LPIPS on the device: ms per call of hr_lpips at 800x800 and 2048x1088, for both nets, on synthetic weights, beside
(a) the float32 torch restatement of tests/lpips_oracle.py's definition on the same device (PyTorch-ROCm's library convolutions),
(b) the reference's form: the frame copied to the host, then float32 torch on the threads the process is given,
and beside the render and the PSNR / SSIM sums of the same frame.  One call is also traced kernel by kernel for each layer's share.
python tools/lpips_ab.py [--seconds S] [--rounds R] [--host-reps N] [--nets alex,vgg] [--out F]
Each timed window is preceded by a time-based warm-up of the same call and lasts --seconds; the variants alternate inside a round and
every round's figure is kept, so the spread between windows is in the output.  Nothing is asserted: the numbers are printed.
Measurement aid (GPU box)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import lpips_oracle as LO  # noqa: E402
from hyperreel_amd import config as C, lpips as HL, metrics, scenes  # noqa: E402
from hyperreel_amd.render import build_render_fn  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--seconds', type=float, default=0.5, help='length of a timed window, and of the warm-up before it')
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--host-reps', type=int, default=2)
ap.add_argument('--nets', default='alex,vgg')
ap.add_argument('--out', default='')
args = ap.parse_args()
FRAMES = [(800, 800), (1088, 2048)]            # (h, w)
assert torch.cuda.is_available(), 'tools/lpips_ab.py measures on the HIP device'


def timed(step, seconds):
    """ms per call: warm up for `seconds`, then time whole batches of calls until `seconds` have passed."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        step()
        torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        n += 5
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e3


def torch_lpips(net, pred, gt, h, w, backbone, lin):
    """the definition in float32 torch ops on whatever device the tensors are on: both images as one batch of two"""
    x = torch.stack([pred.reshape(h, w, 3), gt.reshape(h, w, 3)]).permute(0, 3, 1, 2)
    x = (x * 2 - 1 - torch.tensor(LO.SHIFT, device=x.device).view(1, 3, 1, 1)) / torch.tensor(LO.SCALE, device=x.device).view(1, 3, 1, 1)
    keys, total = HL.backbone_keys(net), 0.0
    for l in LO.LAYERS[net]:
        if l[0] == 'pool':
            x = F.max_pool2d(x, l[1], l[2])
            continue
        wk, bk, _ = keys[l[1]]
        x = F.relu(F.conv2d(x, backbone[wk], backbone[bk], stride=l[2], padding=l[3]))
        if l[4] is not None:
            n = x / (torch.sqrt(torch.sum(x * x, dim=1, keepdim=True)) + 1e-10)
            d = (n[0:1] - n[1:2]) ** 2
            total = total + torch.mean(torch.sum(lin[HL.lin_keys(net)[l[4]][0]] * d, dim=1))
    return total


def layer_flop(net, h, w):
    """2 * M * N * K of every convolution, both images"""
    out, shapes = [], LO.layer_shapes(net, h, w)
    for l, (c, oh, ow) in zip(LO.LAYERS[net], shapes):
        if l[0] == 'conv':
            cin, cout, k = HL.CONVS[net][l[1]]
            out.append(2.0 * (2 * oh * ow) * cout * (k * k * cin))
        else:
            out.append(0.0)
    return out


def kernel_trace(step, net):
    """[(what, us)] of one call's kernels in launch order, averaged over three traced calls; None where the profiler gives no kernel times"""
    try:
        from torch.profiler import ProfilerActivity, profile
        step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(3):
                step()
            torch.cuda.synchronize()
        ev = sorted((e for e in prof.events() if 'hr_lpips' in e.name), key=lambda e: e.time_range.start)
        per_call = len(ev) // 3
        if per_call == 0 or len(ev) != per_call * 3:
            return None
        names = []
        for i, l in enumerate(LO.LAYERS[net]):
            names.append(f'layer {i} ' + (f'conv{l[1]}' if l[0] == 'conv' else 'pool'))
            if l[0] == 'conv' and l[4] is not None:
                names.append(f'head tap {l[4]}')
        names.append('finish')
        if len(names) != per_call:
            return None
        return [(names[j], sum(ev[c * per_call + j].device_time for c in range(3)) / 3.0) for j in range(per_call)]
    except Exception as e:        # a report, not a gate
        print(f'kernel trace unavailable: {e!r}', flush=True)
        return None


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
    m._render_calls = 1000                       # past the calls on which render() polls the sticky bits (a synchronise each)
    mout = torch.empty((4,), dtype=torch.float64, device='cuda')
    mws = torch.empty((metrics.workspace_doubles(h, w),), dtype=torch.float64, device='cuda')
    for net in args.nets.split(','):
        backbone, lin = HL.synthetic_weights(net, 1)
        scorer = HL.Lpips(net, backbone, lin)
        bb_dev, lin_dev = {k: v.cuda() for k, v in backbone.items()}, {k: v.cuda() for k, v in lin.items()}
        out = torch.empty((6,), dtype=torch.float64, device='cuda')
        ws = torch.empty((HL.workspace_doubles(net, h, w),), dtype=torch.float64, device='cuda')
        steps = {'hr_lpips': lambda: scorer.lpips_scores(rgb, gt, h, w, out=out, workspace=ws),
                 'torch_device': lambda: torch_lpips(net, rgb, gt, h, w, bb_dev, lin_dev),
                 'render': lambda: m.render(rays, out=rgb),
                 'psnr_ssim': lambda: metrics.image_scores(rgb, gt, h, w, out=mout, workspace=mws)}
        ms = {}
        with torch.no_grad():
            for _ in range(args.rounds):             # the variants alternate inside a round
                for k, f in steps.items():
                    ms.setdefault(k, []).append(timed(f, args.seconds))
            dev_total = float(scorer.lpips_scores(rgb, gt, h, w)[5])
            torch_total = float(torch_lpips(net, rgb, gt, h, w, bb_dev, lin_dev))
            # (b) the reference's way: the frame to the host, then float32 torch there (the ground truth is on the host already in its loop)
            gt_host, host = gt.cpu(), []
            for _ in range(args.host_reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                x = rgb.cpu()
                t1 = time.perf_counter()
                host_total = float(torch_lpips(net, x, gt_host, h, w, backbone, lin))
                host.append({'copy_ms': (t1 - t0) * 1e3, 'torch_ms': (time.perf_counter() - t1) * 1e3})
        trace = kernel_trace(steps['hr_lpips'], net)
        flop = layer_flop(net, h, w)
        r = {'frame': f'{w}x{h}', 'net': net, 'threads': len(os.sched_getaffinity(0)), 'torch_threads': torch.get_num_threads(),
             'ms_best': {k: round(min(v), 4) for k, v in ms.items()}, 'ms_all': {k: [round(x, 4) for x in v] for k, v in ms.items()},
             'host_copy_ms_best': round(min(x['copy_ms'] for x in host), 3) if host else None,
             'host_torch_ms_best': round(min(x['torch_ms'] for x in host), 1) if host else None,
             'gflop': round(sum(flop) / 1e9, 2), 'tflops_hr_lpips': round(sum(flop) / (min(ms['hr_lpips']) * 1e-3) / 1e12, 2),
             'totals': {'hr_lpips': dev_total, 'torch_device': torch_total, 'torch_host': host_total if host else None},
             'kernels_us': [(n, round(us, 1)) for n, us in trace] if trace else 'not measured'}
        print(json.dumps(r), flush=True)
        res.append(r)
        del scorer, ws, bb_dev, lin_dev
        torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
