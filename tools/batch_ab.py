"""Cost of drawing a training batch: ms per hr_rayset_batch of 16 384 rays (DeviceRaySet.batch), eager and replayed from a captured
hipGraph, for the technicolor-shaped set with real pixels (800 images of 2048 x 1088, 5.3 GB of 8-bit pixels, NDC) and for the
small fixture set (tests/golden/camera/video_ndc.npz); beside it, from the same run, (a) the training step of
tools/train_bench.py on the technicolor model and (b) the reference's form of the feed: slicing 16 384 rows of a pinned host
all_inputs float tensor (12 floats per ray) and copying them to the device.
A Blender-shaped pair rides along (100 images of 800 x 800, world rays): the same cameras as an RGB set and as an RGBA set composited
over white (DeviceRaySet(alpha='white')), and the donerf_sphere training step replayed from a GraphedStep fed by each.
--rgba-only measures that pair alone.
python tools/batch_ab.py [--seconds S] [--rounds R] [--images N] [--rgba-only] [--out F]
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
ap.add_argument('--rgba-only', action='store_true', help='only the Blender-shaped RGB / RGBA pair and the DoNeRF step fed by each')
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


def blender_set(alpha, n_images=100):
    """Blender's shape: 100 images of 800 x 800 on a circle about the origin looking inwards, every pixel kept; alpha=None takes the RGB
    bytes of the same RGBA images (pixels from a seeded generator on the device, alpha 0 / 255 on half of the images, any byte on the rest)"""
    W = H = 800
    gen = torch.Generator(device='cuda').manual_seed(1)
    poses = []
    for i in range(n_images):
        a = 2 * np.pi * i / n_images
        z = np.array([np.sin(a), 0.0, np.cos(a)])                       # the camera looks down -z of its frame, at the origin
        x = np.array([np.cos(a), 0.0, -np.sin(a)])
        poses.append(np.stack([x, np.array([0.0, 1.0, 0.0]), z, 4.0 * z], 1))
    K = np.array([[1111.0, 0, W / 2], [0, 1111.0, H / 2], [0, 0, 1]])

    class Images:
        def __len__(self):
            return n_images

        def __getitem__(self, i):
            img = torch.randint(0, 256, (H, W, 4), dtype=torch.uint8, device='cuda', generator=gen)
            if i % 2 == 0:
                img[..., 3] = (img[..., 3] >> 7) * 255
            return img if alpha else img[..., :3].contiguous()

    return DeviceRaySet(Images(), np.asarray(poses), K, None, None, (W, H), alpha=alpha)


res = {'batch': BS, 'threads': len(os.sched_getaffinity(0))}
sets = {} if args.rgba_only else {'small_fixture_set': small_set(), 'technicolor_shaped_set': large_set(args.images)}
sets.update({'blender_shaped_rgb_set': blender_set(None), 'blender_shaped_rgba_set': blender_set('white')})
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
    res[name] = {'rays': len(s), 'images': s.n_images, 'pixel_store_gb': round(s.n_images * s.width * s.height * s._channels / 1e9, 3)}

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
# the DoNeRF training step, replayed from one graph, fed by the RGB and by the RGBA set of the same cameras
from hyperreel_amd import config as HC, scenes  # noqa: E402
from hyperreel_amd.losses import HipImageLoss  # noqa: E402
from hyperreel_amd.optim import HipAdam  # noqa: E402
from hyperreel_amd.render import build_render_fn  # noqa: E402
from hyperreel_amd.train import GraphedStep  # noqa: E402


def donerf_step(rayset):
    cfg, ds = HC.model_config('donerf_sphere'), HC.dataset_scalars('donerf_sphere')
    sd = scenes.make_state_dict(cfg, ds, None, seed=7, density='dense', app_scale=1.0)
    fn = build_render_fn(cfg, dataset=ds, grid_size=[int(v) for v in sd['model.color_model.net.gridSize']])
    fn.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    fn.train()
    opt = HipAdam([p for p in fn.model.parameters() if p.requires_grad], lr=1e-3, betas=(0.9, 0.99), eps=1e-8, capturable=True)
    return GraphedStep(fn.model, opt, rayset, BS, loss=HipImageLoss('mse'), seed=0, white_bg=True, warmup=3)


fed = {name: donerf_step(sets[name]) for name in ('blender_shaped_rgb_set', 'blender_shaped_rgba_set')}
step_ms = {}
for _ in range(args.rounds):
    for name, gs in fed.items():
        step_ms.setdefault('donerf_step_fed_by_' + name, []).append(timed(gs.step, args.seconds))
ms.update(step_ms)
res['ms_best'] = {k: round(min(v), 5) for k, v in ms.items()}
res['ms_all'] = {k: [round(x, 5) for x in v] for k, v in ms.items()}
best = res['ms_best']
res['rgba_over_rgb'] = {k: round(best[f'{k}_blender_shaped_rgba_set'] / best[f'{k}_blender_shaped_rgb_set'], 4) for k in ('eager', 'graph', 'donerf_step_fed_by')}
del fed
print(json.dumps(res), flush=True)
for s in sets.values():
    s.close()
del sets, steps, graphs, keep
torch.cuda.empty_cache()

# (a) the training step the batch feeds
if not args.rgba_only:
    from train_bench import train_step_figures  # noqa: E402
    fig = train_step_figures('technicolor_z_plane', BS, steps=30)
    res['train_step'] = {k: v for k, v in fig.items() if isinstance(v, (int, float, str))}
    print(json.dumps(res['train_step']), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
