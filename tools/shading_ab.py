"""What the MLP shading modes cost: DoNeRF's 800 x 800 frame, 32 samples per ray, on a 600^3 grid with shadingMode MLP_Fea (the
defaults, 390 -> 128 -> 128 -> 3, and featureC = 64 / fea_pe = 2), on bench.py's dense synthetic scene and on scenes.carve_density's
sparser one.

    python tools/shading_ab.py [--steps 10] [--rounds 3] [--out FILE]

Per (network, scene), one JSON line at the end:
  frame_ms        ms per frame of render() (median over `rounds` windows of `steps` frames, each ended by a device synchronise);
  sh_frame_ms     the same model and scene with shadingMode SH, for comparison;
  live_frac       samples with weight > rm_weight_mask_thre (hr_render_fields on the frame);
  executed_frac   rows of the shading kernel's tiles: a workgroup compacts the live rows of its 512-row span into 64-row tiles;
  shade_ms        hr_stage_shade over that many rows (timed on at most 4 M rows of seeded features and the frame's directions, scaled
                  linearly: a row's cost does not depend on its neighbours), shade_share = shade_ms / frame_ms;
  shade_tflops    2 (k0p hp + hp hp + 16 hp) flop per executed row / shade time: the matrix work the kernel issues, padding included;
  torch_ms        a float32 torch restatement of the network on the same device over the same number of rows (live rows only)."""
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from hyperreel_amd import config as C          # noqa: E402
from hyperreel_amd import lib as L             # noqa: E402
from hyperreel_amd import scenes               # noqa: E402

NETS = {'fea_default': dict(shadingMode='MLP_Fea'), 'fea_c64_pe2': dict(shadingMode='MLP_Fea', featureC=64, fea_pe=2)}


def timed(fn, steps, rounds):
    for _ in range(2):
        fn()
    ms = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / steps * 1e3)
    return statistics.median(ms)


def build(net_edit, carve, seed=7):
    from hyperreel_amd.render import build_render_fn
    cfg, ds = C.model_config('donerf_sphere'), C.dataset_scalars('donerf_sphere')
    for k, v in net_edit.items():
        cfg.color.net[k] = v
    cfg.color.net.data_dim_color = 27
    sd = scenes.make_state_dict(cfg, ds, None, seed=seed, density='dense', app_scale=1.0)
    if carve:
        sd = scenes.carve_density(sd)
    grid = [int(v) for v in sd['model.color_model.net.gridSize']]
    fn = build_render_fn(cfg, dataset=ds, grid_size=grid)
    fn.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return cfg, fn.eval()


def measure(name, net_edit, carve, steps, rounds):
    import shading_oracle as SO
    cfg, fn = build(net_edit, carve)
    m = fn.model
    rays = torch.from_numpy(scenes.benchmark_rays('donerf_sphere', 800, 800, frame=7)).cuda()
    out = torch.empty((rays.shape[0], 3), device='cuda')
    frame_ms = timed(lambda: m.render(rays, out=out), steps, rounds)
    thresh = float(cfg.color.net.get('rm_weight_mask_thre', 1e-4))
    live = m.render(rays, want=('render_weights',))['render_weights'] > thresh
    chunk, Z = m.chunk_rays(), live.shape[1]
    per = -(-rays.shape[0] // -(-rays.shape[0] // chunk))             # hr_even_chunk: equal launches, 64-ray multiples
    per = min(chunk, (per + 63) // 64 * 64)
    executed = 0
    for r0 in range(0, rays.shape[0], per):
        rows = live[r0:r0 + per].reshape(-1)
        pad = (-rows.numel()) % 512
        rows = torch.cat([rows, rows.new_zeros(pad)]) if pad else rows
        executed += int(((rows.view(-1, 512).sum(1) + 63) // 64).sum()) * 64
    n_live, n_all = int(live.sum()), live.numel()
    hc = m._hc
    view_pe, fea_pe, c = hc.shade_mlp.view_pe, hc.shade_mlp.fea_pe, hc.shade_mlp.feature_c
    n = max(64, min(executed, 4 << 20))
    g = torch.Generator(device='cuda').manual_seed(1)
    f = torch.randn((n, 27), device='cuda', generator=g)
    v = rays[torch.randint(0, rays.shape[0], (n,), device='cuda', generator=g), 3:6].contiguous()
    rgb = torch.empty((n, 3), device='cuda')
    h = m.native()
    shade_ms = timed(lambda: L.call('hr_stage_shade', h, f, v, n, rgb, L.stream(f.device), device=f.device), steps, rounds) * executed / n
    k0p, hp = (SO.width(net_edit['shadingMode'], view_pe, fea_pe) + 15) // 16 * 16, (c + 15) // 16 * 16
    flop = 2.0 * (k0p * hp + hp * hp + 16 * hp) * executed
    mlp = m.color_model.net.renderModule.mlp
    nl = max(64, min(n_live, 4 << 20))

    def torch_net():
        with torch.no_grad():
            return torch.sigmoid(mlp(SO.encode(net_edit['shadingMode'], view_pe, fea_pe, f[:nl], v[:nl])))
    torch_ms = timed(torch_net, steps, rounds) * n_live / nl
    del fn, m
    torch.cuda.empty_cache()
    _, sh = build(dict(shadingMode='SH'), carve)
    sh_ms = timed(lambda: sh.model.render(rays, out=out), steps, rounds)
    return {'net': name, 'scene': 'carved' if carve else 'dense', 'frame_ms': round(frame_ms, 3), 'sh_frame_ms': round(sh_ms, 3),
            'live_frac': round(n_live / n_all, 4), 'executed_frac': round(executed / n_all, 4), 'shade_ms': round(shade_ms, 3),
            'shade_share': round(shade_ms / frame_ms, 3), 'shade_tflops': round(flop / (shade_ms * 1e-3) / 1e12, 2), 'torch_ms': round(torch_ms, 3),
            'chunk_rays': chunk, 'width': SO.width(net_edit['shadingMode'], view_pe, fea_pe), 'featureC': c}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out')
    a = ap.parse_args()
    rows = []
    for name, edit in NETS.items():
        for carve in (False, True):
            rows.append(measure(name, edit, carve, a.steps, a.rounds))
            print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, 'w') as fjson:
            json.dump(rows, fjson, indent=1)


if __name__ == '__main__':
    main()
