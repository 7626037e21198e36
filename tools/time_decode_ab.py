"""What the time-dependent decode modes cost: ms per 800 x 800 frame of the technicolor and neural_3d keyframe models on
their shipped grids with each of shadingMode RGBtLinear / RGBtFourier, densityMode DensityLinear / DensityFourier and
RGBtFourier + DensityFourier, beside the SAME family with its shipped `SH` / `Density` -- built in one process and timed in alternation,
window after window (other work shares the device: a difference is only read against the spread of the same run).

    python tools/time_decode_ab.py [--steps 10] [--rounds 5] [--families technicolor_z_plane,neural_3d_z_plane] [--out FILE]

One synthetic scene per family (bench.py's dense seeded one; the new matrices are scenes.make_state_dict's draws).  Per (family, mode),
one JSON line: frame_ms (median over `rounds` windows of `steps` frames of render(), each window ended by a device synchronise),
frame_ms_min / frame_ms_max (the spread of the windows), base_ms (the family's SH / Density model: the same statistics, its windows
alternating with this mode's), ratio = frame_ms / base_ms, the arithmetic the ray MLP runs and whether the frame is verified.  The
shipped model renders with 'auto' (the verified fast path where it applies); `base_f16x3_ms` is the shipped model forced to the ray-MLP
arithmetic the new modes resolve to, so that `ratio_f16x3` isolates the sample stage's share of the difference."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hyperreel_amd import config as C          # noqa: E402
from hyperreel_amd import scenes               # noqa: E402

MODES = {
    'RGBtLinear': dict(shading='RGBtLinear'),
    'RGBtFourier': dict(shading='RGBtFourier'),
    'DensityLinear': dict(density_mode='DensityLinear'),
    'DensityFourier': dict(density_mode='DensityFourier'),
    'RGBtFourier+DensityFourier': dict(shading='RGBtFourier', density_mode='DensityFourier'),
}


def build(family, mlp_precision='auto', seed=7, **toggles):
    from hyperreel_amd.render import build_render_fn
    cfg, ds = C.model_config(family, **toggles), C.dataset_scalars(family)
    sd = scenes.make_state_dict(cfg, ds, None, seed=seed, density='dense', app_scale=1.0)
    grid = [int(v) for v in sd['model.color_model.net.gridSize']]
    fn = build_render_fn(cfg, dataset=ds, grid_size=grid, mlp_precision=mlp_precision)
    fn.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return fn.eval().model


def window(model, rays, out, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        model.render(rays, out=out)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def stats(ms):
    return round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)


def measure(family, steps, rounds):
    rays = torch.from_numpy(scenes.benchmark_rays(family, 800, 800, frame=7)).cuda()
    out = torch.empty((rays.shape[0], 3), device='cuda')
    base, base_x3 = build(family), build(family, mlp_precision='f16x3')
    rows = []
    for name, toggles in MODES.items():
        m = build(family, **toggles)
        models = {'mode': m, 'base': base, 'base_f16x3': base_x3}
        for mm in models.values():                       # every shape of the timed windows, twice
            mm.render(rays, out=out)
            mm.render(rays, out=out)
        ms = {k: [] for k in models}
        for _ in range(rounds):                          # alternating windows
            for k, mm in models.items():
                ms[k].append(window(mm, rays, out, steps))
        f, b, x = stats(ms['mode']), stats(ms['base']), stats(ms['base_f16x3'])
        rows.append({'family': family, 'mode': name, 'frame_ms': f[0], 'frame_ms_min': f[1], 'frame_ms_max': f[2],
                     'base_ms': b[0], 'base_ms_min': b[1], 'base_ms_max': b[2], 'ratio': round(f[0] / b[0], 3),
                     'base_f16x3_ms': x[0], 'base_f16x3_ms_min': x[1], 'base_f16x3_ms_max': x[2], 'ratio_f16x3': round(f[0] / x[0], 3),
                     'mlp': m.mlp_precision_active(), 'base_mlp': base.mlp_precision_active(), 'base_verified': bool(base.mlp_verified()),
                     'chunk_rays': m.chunk_rays(), 'steps': steps, 'rounds': rounds})
        print(json.dumps(rows[-1]), flush=True)
        del m, models
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--families', default='technicolor_z_plane,neural_3d_z_plane')
    ap.add_argument('--out')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_decode_ab.py measures on the GPU: no HIP device')
    rows = []
    for family in a.families.split(','):
        rows += measure(family, a.steps, a.rounds)
    if a.out:
        with open(a.out, 'w') as fjson:
            json.dump(rows, fjson, indent=1)


if __name__ == '__main__':
    main()
