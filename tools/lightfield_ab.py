"""Cost of making two-plane light-field rays: (1) ms per 1024 x 1024 view generated on the device (hr_generate_rays_lightfield) beside
the host's way -- the same (U * V, 6) list built with torch on the CPU (linspace, meshgrid, stack, normalise: the operations
utils/ray_utils.py:14-45 performs) and copied to the device; (2) ms per 16 384-ray batch of a light-field training set
(DeviceRaySet.from_lightfield) beside slicing 16 384 rows of a pinned host all_inputs (10 floats per ray) and copying them.
python tools/lightfield_ab.py [--iters N] [--warmup W] [--views V] [--out F]
Device work is timed with events on the current stream, the host construction with the wall clock around a synchronise; every
variant is warmed up, the variants alternate inside a round, and the median over all timed calls is quoted.  Both sides run in this
process.  Nothing is asserted: the numbers are printed.  Measurement aid (GPU box)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hyperreel_amd import lib as _lib  # noqa: E402
from hyperreel_amd.data import DeviceRaySet, make_lightfield  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=50, help='timed calls per variant and round')
ap.add_argument('--warmup', type=int, default=10)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--views', type=int, default=64, help='views of 512 x 512 in the training set')
ap.add_argument('--batch', type=int, default=16384)
ap.add_argument('--out', default='')
args = ap.parse_args()
assert torch.cuda.is_available(), 'tools/lightfield_ab.py measures on the HIP device'
BS = args.batch
L = _lib.load()


def event_ms(step, iters, warmup):
    """per-call device times: one event pair around every call"""
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def wall_ms(step, iters, warmup):
    """per-call wall times of host work that ends in a device copy"""
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


# ---- (1) one 1024 x 1024 view
U = V = 1024
lf = make_lightfield(U, V, st_scale=0.125, uv_scale=1.0)
rays_dev = torch.empty((U * V, 6), device='cuda')
pinned = torch.empty((U * V, 6)).pin_memory()
state = {'i': 0}


def device_view():
    s = -1.0 + 2.0 * (state['i'] % 17) / 16.0
    state['i'] += 1
    _lib.check(L.hr_generate_rays_lightfield(C.byref(lf), s, 0.25, 0, U * V, C.c_void_p(rays_dev.data_ptr()),
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'hr_generate_rays_lightfield')


def host_view():
    s = -1.0 + 2.0 * (state['i'] % 17) / 16.0
    state['i'] += 1
    u = torch.linspace(-1, 1, U, dtype=torch.float32) * lf.uv_scale
    v = torch.linspace(1, -1, V, dtype=torch.float32) / lf.aspect * lf.uv_scale
    vv, uu = torch.meshgrid(v, u, indexing='ij')
    o = torch.stack([torch.full_like(uu, s * lf.st_scale), torch.full_like(uu, 0.25 * lf.st_scale), torch.full_like(uu, lf.near)], -1)
    d = torch.stack([uu - o[..., 0], vv - o[..., 1], torch.full_like(uu, lf.far - lf.near)], -1)
    pinned.copy_(torch.cat([o, torch.nn.functional.normalize(d, dim=-1)], -1).view(-1, 6))
    rays_dev.copy_(pinned, non_blocking=True)


def copy_only():
    rays_dev.copy_(pinned, non_blocking=True)


# ---- (2) one batch of a training set
W = H = 512
gen = torch.Generator(device='cuda').manual_seed(0)


class Images:                                      # one image at a time: the set copies it into its own store
    def __len__(self):
        return args.views

    def __getitem__(self, i):
        return torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device='cuda', generator=gen)


side = int(np.ceil(np.sqrt(args.views)))
st = [((i % side) / max(side - 1, 1) * 2 - 1, -((i // side) / max(side - 1, 1) * 2 - 1)) for i in range(args.views)]
ray_set = DeviceRaySet.from_lightfield(Images(), st, make_lightfield(W, H, st_scale=0.125))
out = {'coords': torch.empty((BS, 6), device='cuda'), 'rgb': torch.empty((BS, 3), device='cuda'), 'weight': torch.empty((BS, 1), device='cuda')}
n_batches = len(ray_set) // BS
bstate = {'i': 0}


def device_batch():                                # walks the epoch: a different batch every call
    ray_set.batch(bstate['i'] % n_batches, BS, epoch=0, seed=0, out=out)
    bstate['i'] += 1


rows = 64 * BS
all_inputs = torch.rand((rows, 10)).pin_memory()   # the reference's feed: 6 + 3 + 1 floats per ray, the epoch's shuffle already applied
dst = torch.empty((BS, 10), device='cuda')


def host_batch():
    i = bstate['i'] % 64
    dst.copy_(all_inputs[i * BS:(i + 1) * BS], non_blocking=True)
    bstate['i'] += 1


variants = {'view_1024_device': (event_ms, device_view), 'view_1024_host_build_and_copy': (wall_ms, host_view), 'view_1024_copy_only': (event_ms, copy_only),
            f'batch_{BS}_device': (event_ms, device_batch), f'batch_{BS}_host_slice_and_copy': (wall_ms, host_batch)}
ms = {k: [] for k in variants}
for _ in range(args.rounds):
    for k, (timer, step) in variants.items():
        iters = max(5, args.iters // 5) if k == 'view_1024_host_build_and_copy' else args.iters
        ms[k] += timer(step, iters, max(2, args.warmup // 5) if k == 'view_1024_host_build_and_copy' else args.warmup)
res = {'batch': BS, 'threads': len(os.sched_getaffinity(0)), 'torch_threads': torch.get_num_threads(),
       'set': {'rays': len(ray_set), 'views': args.views, 'view_wh': [W, H]},
       'ms_median': {k: round(statistics.median(v), 5) for k, v in ms.items()},
       'ms_min': {k: round(min(v), 5) for k, v in ms.items()}, 'calls': {k: len(v) for k, v in ms.items()}}
print(json.dumps(res), flush=True)
ray_set.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
