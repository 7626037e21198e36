"""Cost of drawing a training batch: ms per hr_rayset_batch of 16 384 rays (DeviceRaySet.batch), eager and replayed from a captured
hipGraph, for the technicolor-shaped set with real pixels (800 images of 2048 x 1088, 5.3 GB of 8-bit pixels, NDC) and for the
small fixture set (tests/golden/camera/video_ndc.npz); beside it, from the same run, (a) the training step of
tools/train_bench.py on the technicolor model and (b) the reference's form of the feed: slicing 16 384 rows of a pinned host
all_inputs float tensor (12 floats per ray) and copying them to the device.
python tools/batch_ab.py [--seconds S] [--rounds R] [--images N] [--out F]
Each timed window is preceded by a time-based warm-up of the same call and lasts --seconds; the variants alternate inside a round and
the best window is quoted.  Nothing is asserted: the numbers are printed.  Measurement aid (GPU box)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from hyperreel_amd.data import DeviceRaySet  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--seconds', type=float, default=0.5, help='length of a timed window, and of the warm-up before it')
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--images', type=int, default=800, help='images of 2048 x 1088 in the large set')
ap.add_argument('--batch', type=int, default=16384)
ap.add_argument('--out', default='')
args = ap.parse_args()
assert torch.cuda.is_available(), 'tools/batch_ab.py measures on the HIP device'
BS = args.batch


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


def small_set():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'camera', 'video_ndc.npz')) as z:
        f = {k: z[k] for k in z.files}
    reps = 12                                      # 12 copies of the fixture's 27 images: more than two batches of 16 384
    tile = lambda a: np.concatenate([a] * reps, 0)
    fx, fy, near, w, h = [float(v) for v in f['ndc']]
    return DeviceRaySet(tile(f['images']), tile(f['poses']), tile(f['intrinsics']), tile(f['times']), tile(f['cam_ids']),
                        (int(f['img_wh'][0]), int(f['img_wh'][1])), ndc=dict(fx=fx, fy=fy, near=near, width=int(w), height=int(h)),
                        subsample=[(int(e), int(o)) for e, o in f['rules']] * reps)


def large_set(n_images):
    """technicolor's shape: 16 cameras x 50 frames of 2048 x 1088, every pixel kept, pixels from a seeded generator on the device"""
    W, H = 2048, 1088
    gen = torch.Generator(device='cuda').manual_seed(0)
    rng = np.random.default_rng(0)
    poses, Ks = [], []
    for i in range(n_images):
        a = np.radians(rng.uniform(-8, 8))
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        poses.append(np.concatenate([R, rng.uniform(-0.5, 0.5, (3, 1))], 1))
        Ks.append(np.array([[2400.0, 0, W / 2], [0, 2400.0, H / 2], [0, 0, 1]]))

    class Images:                                  # one image at a time: the set copies it into its own store
        def __len__(self):
            return n_images

        def __getitem__(self, i):
            return torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device='cuda', generator=gen)

    return DeviceRaySet(Images(), np.asarray(poses), np.asarray(Ks), [(i // 16) / 49.0 for i in range(n_images)], [i % 16 for i in range(n_images)],
                        (W, H), ndc=dict(fx=2400.0, fy=2400.0, near=0.95, width=W, height=H))


res = {'batch': BS, 'threads': len(os.sched_getaffinity(0))}
sets = {'small_fixture_set': small_set(), 'technicolor_shaped_set': large_set(args.images)}
steps, graphs, keep = {}, {}, []
for name, s in sets.items():
    out = {'coords': torch.empty((BS, s.ray_dim), device='cuda'), 'rgb': torch.empty((BS, 3), device='cuda'), 'weight': torch.empty((BS, 1), device='cuda')}
    keep.append(out)
    n_batches = len(s) // BS
    state = {'i': 0}

    def eager(s=s, out=out, n_batches=n_batches, state=state):      # walks the epoch: a different batch every call
        s.batch(state['i'] % n_batches, BS, epoch=0, seed=0, out=out)
        state['i'] += 1

    steps[name] = eager
    graphs[name] = graph_of(lambda s=s, out=out: s.batch(1, BS, epoch=0, seed=0, out=out))
    res[name] = {'rays': len(s), 'images': s.n_images, 'pixel_store_gb': round(s.n_images * s.width * s.height * 3 / 1e9, 3)}

# (b) the reference's feed: rows [i * BS, (i + 1) * BS) of a pinned host all_inputs (the epoch's shuffle already applied), to the device
rows = 64 * BS
all_inputs = torch.rand((rows, 12)).pin_memory()
dst = torch.empty((BS, 12), device='cuda')
hstate = {'i': 0}


def host_feed():
    i = hstate['i'] % 64
    dst.copy_(all_inputs[i * BS:(i + 1) * BS], non_blocking=True)
    hstate['i'] += 1


ms = {}
for _ in range(args.rounds):
    for name in sets:
        ms.setdefault('eager_' + name, []).append(timed(steps[name], args.seconds))
        ms.setdefault('graph_' + name, []).append(timed(graphs[name].replay, args.seconds))
    ms.setdefault('host_slice_copy', []).append(timed(host_feed, args.seconds))
res['ms_best'] = {k: round(min(v), 5) for k, v in ms.items()}
res['ms_all'] = {k: [round(x, 5) for x in v] for k, v in ms.items()}
print(json.dumps(res), flush=True)
for s in sets.values():
    s.close()
del sets, steps, graphs, keep
torch.cuda.empty_cache()

# (a) the training step the batch feeds
from train_bench import train_step_figures  # noqa: E402
fig = train_step_figures('technicolor_z_plane', BS, steps=30)
res['train_step'] = {k: v for k, v in fig.items() if isinstance(v, (int, float, str))}
print(json.dumps(res['train_step']), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
