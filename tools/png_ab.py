"""Cost of writing a rendered frame out as a PNG file, for the DoNeRF benchmark frame (synthetic seeded scene, shipped grid) at 800 x 800
RGB, 2048 x 1088 RGB and 800 x 800 RGBA (pack_display's bytes): ms per frame of
  render         model.render of the frame's rays, for scale
  encode         hr_png_encode from the float frame (RGBA: from the 8-bit pack), the file left in device memory
  encode_d2h     the same plus the copy of the length and of the file's bytes to the host (PngEncoder.encode)
  host_l1/l6     the path it replaces: frame to the host, to8b in numpy, PIL's PNG encoder at compress_level 1 and 6
and the sizes of all the files.  python tools/png_ab.py [--seconds S] [--rounds R] [--out F]
Each timed window is preceded by a time-based warm-up of the same call and lasts --seconds; the variants alternate inside a round and
the best window is quoted.  Nothing is asserted: the numbers are printed.  Measurement aid (GPU box)."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hyperreel_amd import config as HC  # noqa: E402
from hyperreel_amd import png, scenes  # noqa: E402
from hyperreel_amd.render import build_render_fn  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--seconds', type=float, default=0.5, help='length of a timed window, and of the warm-up before it')
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--model', default='donerf_sphere')
ap.add_argument('--out', default='')
args = ap.parse_args()
assert torch.cuda.is_available(), 'tools/png_ab.py measures on the HIP device'


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


def to8b(x):
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


cfg, ds = HC.model_config(args.model), HC.dataset_scalars(args.model)
sd = scenes.make_state_dict(cfg, ds, None, seed=7, density='dense', app_scale=1.0)
grid = [int(v) for v in sd['model.color_model.net.gridSize']]
fn = build_render_fn(cfg, dataset=ds, grid_size=grid)
fn.model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=False)
model = fn.model

from PIL import Image  # noqa: E402

results = []
for (w, h, rgba) in ((800, 800, False), (2048, 1088, False), (800, 800, True)):
    rays = torch.from_numpy(scenes.benchmark_rays(args.model, h, w, frame=7)).cuda()
    rgb = model.render(rays)['rgb'].clone()
    torch.cuda.synchronize()
    channels = 4 if rgba else 3
    frame = model.pack_display(rgb, h, w, rgba8=True).clone() if rgba else rgb
    enc = png.PngEncoder(w, h, channels)
    out = torch.empty(enc.bound, dtype=torch.uint8, device='cuda')
    length = torch.zeros(1, dtype=torch.int64, device='cuda')
    mode = 'RGBA' if rgba else 'RGB'

    def render():
        model.render(rays)

    def encode():
        enc.encode_device(frame, out=out, length=length)

    def encode_d2h():
        enc.encode(frame)

    def host(level):
        a = frame.cpu().numpy() if rgba else to8b(rgb.cpu().numpy())
        b = io.BytesIO()
        Image.fromarray(a.reshape(h, w, channels), mode).save(b, 'PNG', compress_level=level)
        return b.getvalue()

    variants = {'render': render, 'encode': encode, 'encode_d2h': encode_d2h, 'host_l1': lambda: host(1), 'host_l6': lambda: host(6)}
    best = {k: float('inf') for k in variants}
    for _ in range(args.rounds):
        for k, step in variants.items():
            best[k] = min(best[k], timed(step, args.seconds if not k.startswith('host') else min(args.seconds, 0.3)))
    data = enc.encode(frame)
    decoded = np.asarray(Image.open(io.BytesIO(data)))
    expect = frame.cpu().numpy().reshape(h, w, channels) if rgba else to8b(rgb.cpu().numpy()).reshape(h, w, 3)
    r = {'width': w, 'height': h, 'channels': channels, 'ms': {k: round(v, 4) for k, v in best.items()},
         'bytes': {'raw': h * w * channels, 'device': len(data), 'pil_level1': len(host(1)), 'pil_level6': len(host(6))},
         'decodes_to_the_frame': bool(np.array_equal(decoded, expect)), 'encode_below_render': bool(best['encode'] < best['render'])}
    results.append(r)
    print(json.dumps(r), flush=True)
    enc.close()

if args.out:
    with open(args.out, 'w') as f:
        json.dump({'model': args.model, 'grid': grid, 'results': results}, f, indent=1)
