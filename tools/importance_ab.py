"""Cost of the importance subsample rule for one image pair of Immersive's shipped size (1280 x 960, fisheye camera, num_take =
round(W H / 8), direction limit -0.05): ms per
  importance   hr_rayset_set_image_importance of image 1 against image 0 (host bytes in: copy + select + mask + compaction + commit)
  set_image    hr_rayset_set_image_fisheye of the same bytes (the copy and commit both pay)
  torch_cpu    the reference's form: diff, torch.sort, threshold, mask on CPU float tensors (datasets/immersive.py:299-308)
  torch_gpu    the same torch lines on the device
python tools/importance_ab.py [--seconds S] [--rounds R] [--static F] [--out F]
Each timed window is preceded by a time-based warm-up of the same call and lasts --seconds; the variants alternate inside a round and
the best window is quoted.  Nothing is asserted: the numbers are printed.  Measurement aid (GPU box)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hyperreel_amd import lib as _lib  # noqa: E402
from hyperreel_amd.data import DeviceRaySet, Importance, make_camera, make_fisheye  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--seconds', type=float, default=0.5, help='length of a timed window, and of the warm-up before it')
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--static', type=float, default=0.0, help='fraction of pixels equal to the previous frame (ties at a threshold of 0)')
ap.add_argument('--out', default='')
args = ap.parse_args()
assert torch.cuda.is_available(), 'tools/importance_ab.py measures on the HIP device'
W, H = 1280, 960
TAKE = int(np.round(W * H * 0.125))
LIMIT = -0.05


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


rng = np.random.default_rng(0)
prev = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
cur = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
if args.static > 0:
    cur = np.where((rng.random((H, W)) < args.static)[..., None], prev, cur)
a = 1.45                                              # turned until the limit's contour crosses the image
pose = np.array([[np.cos(a), 0, np.sin(a), 0.1], [0, 1, 0, 0.0], [-np.sin(a), 0, np.cos(a), 0.2]], np.float32)
K = np.array([[600.0, 0, W / 2], [0, 600.0, H / 2], [0, 0, 1]], np.float32)
pair = (0.03, 0.004)
s = DeviceRaySet([prev, cur, cur], np.stack([pose] * 3), K, [0.0, 0.5, 1.0], [0, 0, 0], (W, H), subsample=[(1, 0), Importance(TAKE, 0, LIMIT), (1, 0)],
                 distortions=[pair] * 3)
L = _lib.load()
cam, fe = make_camera(pose, K, W, H, 0.0, 0.5), make_fisheye(pair)
cur_host = torch.from_numpy(cur)
cur_ptr = C.c_void_p(cur_host.data_ptr())
info = s.image_info(1)


def importance():
    _lib.check(L.hr_rayset_set_image_importance(s._h, 1, C.byref(cam), C.byref(fe), 0, TAKE, LIMIT, cur_ptr), 'hr_rayset_set_image_importance')


def set_image():                                      # slot 2: nobody's previous frame
    _lib.check(L.hr_rayset_set_image_fisheye(s._h, 2, C.byref(cam), C.byref(fe), 1, 0, cur_ptr), 'hr_rayset_set_image_fisheye')


rgb_c, last_c = torch.from_numpy(cur).reshape(-1, 3).float().div(255), torch.from_numpy(prev).reshape(-1, 3).float().div(255)
dz_c = s.batch(0, 0, indices=torch.arange(W * H, dtype=torch.int64, device='cuda'))['coords'][:, 5].cpu()
rgb_g, last_g, dz_g = rgb_c.cuda(), last_c.cuda(), dz_c.cuda()


def torch_lines(rgb, last, dz):
    diff = torch.abs(rgb - last).mean(-1)
    diff_sorted, _ = torch.sort(diff)
    mask = (diff > diff_sorted[-TAKE]) & (dz < LIMIT)
    return mask


variants = {'importance': importance, 'set_image': set_image, 'torch_cpu': lambda: torch_lines(rgb_c, last_c, dz_c),
            'torch_gpu': lambda: torch_lines(rgb_g, last_g, dz_g)}
ms = {}
for _ in range(args.rounds):
    for name, fn in variants.items():
        ms.setdefault(name, []).append(timed(fn, args.seconds))
res = {'image': [W, H], 'num_take': TAKE, 'dir_z_below': LIMIT, 'static': args.static, 'kept': info['count'], 'threshold': info['threshold'],
       'list_bytes': (TAKE - 1) * 4, 'threads': len(os.sched_getaffinity(0)), 'seconds': args.seconds, 'rounds': args.rounds,
       'torch_mask_kept': int(torch_lines(rgb_g, last_g, dz_g).sum()),
       'ms_best': {k: round(min(v), 5) for k, v in ms.items()}, 'ms_all': {k: [round(x, 5) for x in v] for k, v in ms.items()}}
res['ms_best']['select_compact'] = round(res['ms_best']['importance'] - res['ms_best']['set_image'], 5)
print(json.dumps(res), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
s.close()
