"""Cost of writing a rendered frame out as a baseline JPEG file, for the DoNeRF benchmark frame (synthetic seeded scene, shipped grid) at
800 x 800 RGB, 2048 x 1088 RGB and 800 x 800 RGBA (pack_display's bytes), quality 90: ms per frame of
  render             model.render of the frame's rays, for scale
  png                hr_png_encode of the same frame, the file left in device memory
  jpeg_<sub>[_rst]   hr_jpeg_encode from the float frame (RGBA: from the 8-bit pack) in 4:2:0 and 4:4:4, without and with a restart marker per
                     MCU row, the file left in device memory
  ..._d2h            the same plus the copy of the length and of the file's bytes to the host (JpegEncoder.encode)
  host_pil           the path it replaces: frame to the host, to8b in numpy, PIL's save(f, 'JPEG', quality=90, subsampling=2)
and the sizes of all the files.  python tools/jpeg_ab.py [--seconds S] [--rounds R] [--out F]
Each timed window is preceded by a time-based warm-up of the same call and lasts --seconds; the variants alternate inside a round and
the best window is quoted.  Nothing is asserted beyond the device's 4:2:0 file being PIL's: the numbers are printed.
Per-kernel times come from a run of their own:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/jpeg_ab.py --kernels-only
(100 encodes of the 800 x 800 RGB frame in 4:2:0 and nothing else).  Measurement aid (GPU box)."""
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
from hyperreel_amd import jpeg, png, scenes  # noqa: E402
from hyperreel_amd.render import build_render_fn  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--seconds', type=float, default=0.4, help='length of a timed window, and of the warm-up before it')
ap.add_argument('--rounds', type=int, default=2)
ap.add_argument('--model', default='donerf_sphere')
ap.add_argument('--quality', type=int, default=90)
ap.add_argument('--kernels-only', action='store_true', help='100 encodes of the 800 x 800 RGB frame in 4:2:0, for a kernel trace')
ap.add_argument('--out', default='')
args = ap.parse_args()
assert torch.cuda.is_available(), 'tools/jpeg_ab.py measures on the HIP device'


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

if args.kernels_only:
    w, h = 800, 800
    rgb = model.render(torch.from_numpy(scenes.benchmark_rays(args.model, h, w, frame=7)).cuda())['rgb'].clone()
    enc = jpeg.JpegEncoder(w, h, 3, args.quality, '4:2:0')
    out = torch.empty(enc.bound, dtype=torch.uint8, device='cuda')
    length = torch.zeros(1, dtype=torch.int64, device='cuda')
    for _ in range(100):
        enc.encode_device(rgb, out=out, length=length)
    torch.cuda.synchronize()
    print(json.dumps({'encodes': 100, 'bytes': int(length.item())}))
    sys.exit(0)

results = []
for (w, h, rgba) in ((800, 800, False), (2048, 1088, False), (800, 800, True)):
    rays = torch.from_numpy(scenes.benchmark_rays(args.model, h, w, frame=7)).cuda()
    rgb = model.render(rays)['rgb'].clone()
    torch.cuda.synchronize()
    channels = 4 if rgba else 3
    frame = model.pack_display(rgb, h, w, rgba8=True).clone() if rgba else rgb
    penc = png.PngEncoder(w, h, channels)
    pout = torch.empty(penc.bound, dtype=torch.uint8, device='cuda')
    length = torch.zeros(1, dtype=torch.int64, device='cuda')
    encs = {f'jpeg_{sub.replace(":", "")}{"_rst" if rr else ""}': jpeg.JpegEncoder(w, h, channels, args.quality, sub, rr)
            for sub in ('4:2:0', '4:4:4') for rr in (0, 1)}
    outs = {k: torch.empty(e.bound, dtype=torch.uint8, device='cuda') for k, e in encs.items()}

    def host_pil():
        a = frame.cpu().numpy().reshape(h, w, 4)[..., :3] if rgba else to8b(rgb.cpu().numpy()).reshape(h, w, 3)
        b = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(a)).save(b, 'JPEG', quality=args.quality, subsampling=2)
        return b.getvalue()

    variants = {'render': lambda: model.render(rays), 'png': lambda: penc.encode_device(frame, out=pout, length=length), 'host_pil': host_pil}
    for k, e in encs.items():
        variants[k] = (lambda e=e, k=k: e.encode_device(frame, out=outs[k], length=length))
        variants[k + '_d2h'] = (lambda e=e: e.encode(frame))
    best = {k: float('inf') for k in variants}
    for _ in range(args.rounds):
        for k, step in variants.items():
            best[k] = min(best[k], timed(step, args.seconds if k != 'host_pil' else min(args.seconds, 0.3)))
    sizes = {k: len(e.encode(frame)) for k, e in encs.items()}
    sizes.update(raw=h * w * channels, png=len(penc.encode(frame)), pil=len(host_pil()))
    r = {'width': w, 'height': h, 'channels': channels, 'quality': args.quality, 'ms': {k: round(v, 4) for k, v in best.items()}, 'bytes': sizes,
         'device_file_is_pils': bool(encs['jpeg_420'].encode(frame) == host_pil()), 'jpeg_below_png': bool(best['jpeg_420'] < best['png']),
         'jpeg_below_render': bool(best['jpeg_420'] < best['render'])}
    results.append(r)
    print(json.dumps(r), flush=True)
    penc.close()
    for e in encs.values():
        e.close()

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump({'model': args.model, 'grid': grid, 'results': results}, f, indent=1)
