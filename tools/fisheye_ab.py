"""Cost of fisheye camera rays beside the pinhole calls: ms per 800 x 800 frame (hr_generate_rays_fisheye, hr_generate_rays_ndc with a
NULL ndc, hr_generate_rays) and per 16 384-ray batch of a training set (hr_rayset_set_image_fisheye with a lens vs without), and, with
--parent-lib, the same calls from another build of the library (the parent commit's), loaded beside this one.
python tools/fisheye_ab.py [--parent-lib PATH] [--out F]
Every variant: 0.5 s of warm-up, then three 0.5 s windows of back-to-back calls, synchronised at the window's ends (ms per call =
window / calls): 'ms' is the best window, 'spread' the distance from the best to the worst, 'windows' all three.  The calls are
launch-bound at these sizes.  Nothing is asserted: the numbers are printed.  Measurement aid."""
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
from hyperreel_amd.data import make_camera, make_fisheye  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--parent-lib', default='', help='another libhyperreel_hip.so whose calls are timed too')
ap.add_argument('--window', type=float, default=0.5)
ap.add_argument('--out', default='')
args = ap.parse_args()
assert torch.cuda.is_available(), 'tools/fisheye_ab.py measures on the HIP device'
L = _lib.load()
W = H = 800
BS = 16384
pose = np.concatenate([np.eye(3), np.array([[0.1], [0.2], [0.3]])], 1)
K = np.array([[420.0, 0, W / 2], [0, 420.0, H / 2], [0, 0, 1]])
cam = make_camera(pose, K, W, H, 1.0, 0.5)
fe = make_fisheye((0.03, 0.004))
rays = torch.empty((W * H, 8), device='cuda')
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731


def window_ms(step):
    """[ms per call] of three windows after one of warm-up"""
    def run(seconds):
        torch.cuda.synchronize()
        t0, n = time.perf_counter(), 0
        while time.perf_counter() - t0 < seconds:
            for _ in range(20):
                step()
            n += 20
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n
    run(args.window)
    return [run(args.window) for _ in range(3)]


def frame_call(handle, kind):
    if kind == 'fisheye':
        return lambda: handle.hr_generate_rays_fisheye(C.byref(cam), C.byref(fe), None, 8, 0, W * H, C.c_void_p(rays.data_ptr()), stream())
    if kind == 'pinhole':
        return lambda: handle.hr_generate_rays_ndc(C.byref(cam), None, 8, 0, W * H, C.c_void_p(rays.data_ptr()), stream())
    return lambda: handle.hr_generate_rays(C.byref(cam), 8, 0, W * H, C.c_void_p(rays.data_ptr()), stream())


n_img = 8
images = torch.randint(0, 256, (n_img, H, W, 3), dtype=torch.uint8, device='cuda')
times, ids = np.linspace(0, 1, n_img), np.arange(n_img)
out = {'coords': torch.empty((BS, 8), device='cuda'), 'rgb': torch.empty((BS, 3), device='cuda'), 'weight': torch.empty((BS, 1), device='cuda')}


def batch_call(handle, h):
    """hr_rayset_batch of set handle `h` through library `handle`, walking the epoch: a different batch every call"""
    state = {'i': 0}
    n_batches = int(handle.hr_rayset_size(h)) // BS

    def step():
        handle.hr_rayset_batch(h, (state['i'] % n_batches) * BS, BS, 0, 0, None, C.c_void_p(out['coords'].data_ptr()),
                               C.c_void_p(out['rgb'].data_ptr()), C.c_void_p(out['weight'].data_ptr()), stream())
        state['i'] += 1
    return step


def measure(handle):
    """{variant: three windows} of one build: the three frame calls, then a batch of a fisheye set and of a pinhole one"""
    w = {f'frame_{kind}': window_ms(frame_call(handle, kind)) for kind in ('fisheye', 'pinhole', 'plain')}
    for kind, lens in (('fisheye', fe), ('pinhole', None)):
        h = C.c_void_p()
        assert handle.hr_rayset_create(n_img, W, H, 8, None, C.byref(h)) == 0
        for i in range(n_img):
            assert handle.hr_rayset_set_image_fisheye(h, i, C.byref(make_camera(pose, K, W, H, ids[i], times[i])),
                                                      C.byref(lens) if lens is not None else None, 1, 0, C.c_void_p(images[i].data_ptr())) == 0
        w[f'batch_{kind}'] = window_ms(batch_call(handle, h))
        handle.hr_rayset_destroy(h)
    return w


windows = measure(L)
if args.parent_lib:
    P = C.CDLL(os.path.abspath(args.parent_lib))
    for name, restype, argtypes in _lib.SYMBOLS:
        if hasattr(P, name):
            getattr(P, name).restype, getattr(P, name).argtypes = restype, argtypes
    windows.update({f'{k}_parent': v for k, v in measure(P).items()})
res = {'frame': [W, H], 'batch': BS, 'ms': {k: round(min(v), 5) for k, v in windows.items()},
       'spread': {k: round(max(v) - min(v), 5) for k, v in windows.items()}, 'windows': {k: [round(x, 5) for x in v] for k, v in windows.items()}}
print(json.dumps(res), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
