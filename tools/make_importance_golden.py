"""Generates tests/golden/importance/*.npz by running the REFERENCE'S OWN importance_subsample methods -- ImmersiveDataset's
(datasets/immersive.py:295-310) and Neural3DVideoDataset's (datasets/neural_3d.py:191-204), imported in-process through
oracle/refgen/ref_shim.py and called unbound with a namespace that carries the four rule numbers -- on seeded synthetic videos.  Run
where the reference tree exists:

    python tools/make_importance_golden.py

TEST INFRASTRUCTURE ONLY.  Each fixture stores the inputs (8-bit images in Immersive's load order, video-major; per image pose,
intrinsics, distortion, time, camera id, frame number, whether it is its video's first loaded frame; the rule numbers, the direction
limit, the NDC arguments), the float32 coords handed to the method (`video_coords`: one (W * H, 7) block per video, the image's time
is appended as column 7) and what the method made of them: per image `diff`, `threshold`, `num_take` and the kept pixels (`kept`,
image i's at `kept_rows[i]:kept_rows[i + 1]`), and `all_inputs`, composed as prepare_train_data composes it (immersive.py:330-420).
`kept` comes out of the same call: the pixel index rides in a spare coords column (exact below 2^24).

Fisheye coords are tests/fisheye_common.py's float64 evaluation rounded to float32 (OpenCV, which the reference calls, is not a
dependency here: that oracle states the same inverse); pinhole coords are the reference's get_ray_directions_K / get_rays /
get_ndc_rays_fx_fy, as in tools/make_camera_golden.py."""
import importlib
import os
import sys
import types
from types import SimpleNamespace
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, 'oracle', 'refgen'), os.path.join(ROOT, 'tests'), HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, 'tests', 'golden', 'importance')
BAND = 1e-5            # the fisheye direction bar's cap (tests/fisheye_common.py): no fixture pixel's d_z may lie this close to the limit

SHIPPED = dict(load_full_step=8, subsample_keyframe_step=4, subsample_keyframe_frac=0.25, subsample_frac=0.125)   # conf/experiment/dataset/immersive.yaml
CASES = {
    # Immersive's layout: 2 fisheye videos x 9 frames, its shipped steps and fractions, its direction limit; camera 1 is turned until the
    # d_z = -0.05 contour crosses its images
    'immersive_small': dict(wh=(24, 14), videos=2, frames=9, seed=211, rule=SHIPPED, dir_z_below=-0.05, ndc=None, method='immersive',
                            pairs=[(0.03, 0.004), (-0.05, 0.01)], yaw=[0.1, 1.5], crossing=1, static=None),
    # 95 % of the pixels equal the previous frame's: the threshold is 0 with thousands of ties; frames 2 and 3 are identical: nothing kept
    'static_background': dict(wh=(61, 47), videos=1, frames=5, seed=212, rule=SHIPPED, dir_z_below=-0.05, ndc=None, method='immersive',
                              pairs=[(0.2, -0.02)], yaw=[-0.07], crossing=None, static=dict(changed=0.05, same_as_previous=3)),
    # Neural 3D's variant: pinhole cameras through NDC, no direction test
    'neural3d_variant': dict(wh=(33, 7), videos=1, frames=6, seed=213, dir_z_below=None, method='neural_3d',
                             rule=dict(load_full_step=4, subsample_keyframe_step=2, subsample_keyframe_frac=0.25, subsample_frac=0.125),
                             ndc=dict(near=0.5), pairs=None, yaw=[0.05], crossing=None, static=None),
}


def _pose(ry, rx, t):
    cy, sy, cx, sx = np.cos(ry), np.sin(ry), np.cos(rx), np.sin(rx)
    R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return np.concatenate([R, np.asarray(t, np.float64)[:, None]], 1).astype(np.float32)


def make_inputs(name):
    """The seeded inputs of a case, as the arrays the fixture stores."""
    c = CASES[name]
    rng = np.random.default_rng(c['seed'])
    W, H = c['wh']
    V, F = c['videos'], c['frames']
    f0 = np.float32(0.85 * W)
    cam_pose = [_pose(c['yaw'][v], rng.uniform(-0.1, 0.1), rng.uniform(-0.4, 0.4, 3)) for v in range(V)]
    cam_K = [np.array([[f0 * rng.uniform(0.97, 1.03), 0, W / 2 + rng.uniform(-1, 1)], [0, f0 * rng.uniform(0.97, 1.03), H / 2 + rng.uniform(-1, 1)],
                       [0, 0, 1]], np.float32) for v in range(V)]
    images, poses, Ks, pairs, times, cam_ids, frames, first, video_of = [], [], [], [], [], [], [], [], []
    for v in range(V):                                   # Immersive's load order: every frame of video 0, then of video 1, ...
        img = None
        for fr in range(F):
            if img is None or c['static'] is None:
                img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            elif fr != c['static']['same_as_previous']:
                changed = rng.random((H, W)) < c['static']['changed']
                img = np.where(changed[..., None], rng.integers(0, 256, (H, W, 3), dtype=np.uint8), img)
            images.append(img)
            poses.append(cam_pose[v]); Ks.append(cam_K[v]); frames.append(fr); cam_ids.append(v); video_of.append(v); first.append(fr == 0)
            times.append(fr / (F - 1))
            if c['pairs']:
                pairs.append(c['pairs'][v])
    r = c['rule']
    d = dict(images=np.asarray(images, np.uint8), poses=np.asarray(poses, np.float32), intrinsics=np.asarray(Ks, np.float32),
             times=np.asarray(times, np.float64), cam_ids=np.asarray(cam_ids, np.int32), frames=np.asarray(frames, np.int32),
             first_of_video=np.asarray(first), video_of=np.asarray(video_of, np.int32), img_wh=np.asarray([W, H], np.int32), video=np.asarray(True),
             rule=np.asarray([r['load_full_step'], r['subsample_keyframe_step'], r['subsample_keyframe_frac'], r['subsample_frac']], np.float64),
             dir_z_below=np.asarray(np.nan if c['dir_z_below'] is None else c['dir_z_below'], np.float64))
    if c['pairs']:
        d['distortions'] = np.asarray(pairs, np.float64)
    if c['ndc']:
        d['ndc'] = np.asarray([float(f0), float(f0), c['ndc']['near'], W, H], np.float64)      # fx, fy, near, width, height
    return d


def reference_methods():
    """{'immersive': ImmersiveDataset.importance_subsample, 'neural_3d': Neural3DVideoDataset.importance_subsample}, the reference's
    own functions: its datasets package is registered without running its __init__ (which imports every dataset), and what an import
    asks for that this machine lacks is a MagicMock -- none of it is touched by the two methods."""
    import ref_shim
    ref_shim.install()
    if 'datasets' not in sys.modules or not getattr(sys.modules['datasets'], '__path__', [''])[0].startswith(ref_shim.REF):
        pkg = types.ModuleType('datasets')
        pkg.__path__ = [ref_shim.REF + '/datasets']
        sys.modules['datasets'] = pkg
    for n in ('omegaconf', 'PIL', 'imageio', 'scipy.spatial.transform', 'sklearn', 'sklearn.neighbors', 'iopath', 'iopath.common',
              'iopath.common.file_io'):
        try:
            importlib.import_module(n)
        except Exception:
            sys.modules[n] = MagicMock()
    for _ in range(32):
        try:
            from datasets.immersive import ImmersiveDataset
            from datasets.neural_3d import Neural3DVideoDataset
            break
        except ModuleNotFoundError as e:
            sys.modules[e.name] = MagicMock()
    return {'immersive': ImmersiveDataset.importance_subsample, 'neural_3d': Neural3DVideoDataset.importance_subsample}


def video_coords(d, name):
    """(videos, W * H, 7) float32: rays and camera id of every pixel of each video's camera, and the float64 d_z beside (None: pinhole)."""
    import fisheye_common
    import importance_common
    W, H = int(d['img_wh'][0]), int(d['img_wh'][1])
    out, dz = [], []
    for v in range(CASES[name]['videos']):
        i = int(np.nonzero(d['video_of'] == v)[0][0])
        if 'distortions' in d:
            r64 = importance_common.rays64(W, H, d['intrinsics'][i], d['poses'][i], tuple(float(k) for k in d['distortions'][i]), None)
            rays = torch.from_numpy(r64.astype(np.float32))
            dz.append(r64[:, 5])
        else:
            import make_camera_golden
            from utils import ray_utils as RU
            RU.create_meshgrid = make_camera_golden._pixel_grid
            directions = RU.get_ray_directions_K(H, W, torch.FloatTensor(d['intrinsics'][i]), centered_pixels=True)
            rays_o, rays_d = RU.get_rays(directions, torch.FloatTensor(d['poses'][i]))
            rays = torch.cat([rays_o, rays_d], dim=-1)
            fx, fy, near, nw, nh = [float(x) for x in d['ndc']]
            rays = RU.get_ndc_rays_fx_fy(int(nh), int(nw), fx, fy, near, rays)
        out.append(torch.cat([rays, torch.ones_like(rays[..., :1]) * int(d['cam_ids'][i])], dim=-1))
    return torch.stack(out, 0), dz


def make_case(name):
    c = CASES[name]
    d = make_inputs(name)
    method = reference_methods()[c['method']]
    r = c['rule']
    self = SimpleNamespace(load_full_step=r['load_full_step'], subsample_keyframe_step=r['subsample_keyframe_step'],
                           subsample_keyframe_frac=r['subsample_keyframe_frac'], subsample_frac=r['subsample_frac'])
    W, H = int(d['img_wh'][0]), int(d['img_wh'][1])
    n_pixels = W * H
    vcoords, dz = video_coords(d, name)
    limit = c['dir_z_below']
    if limit is not None:
        for v, z in enumerate(dz):                       # cap: 0 pixels inside the band where a float32 ray may fall on the other side
            assert int((np.abs(z - limit) < BAND).sum()) == 0, (name, v)
            if c['crossing'] == v:
                assert 0.2 <= float((z < limit).mean()) <= 0.8, (name, v, float((z < limit).mean()))
    index = torch.arange(n_pixels, dtype=torch.float32)[:, None]
    all_coords, all_rgb, diffs, thresholds, takes, kept, ties = [], [], [], [], [], [], 0
    last_rgb = None
    for i in range(d['images'].shape[0]):
        time = float(d['times'][i])
        coords = torch.cat([vcoords[int(d['video_of'][i])], torch.ones(n_pixels, 1) * time, index], -1)     # 8 columns + the pixel index
        rgb = torch.from_numpy(d['images'][i]).reshape(-1, 3).to(torch.float32).div(255)                     # ToTensor (torchvision is mocked)
        frame = int(np.round(time * (c['frames'] - 1)))                                                       # cur_frame, immersive.py:353
        assert frame == int(d['frames'][i])
        diff = np.full(n_pixels, np.nan, np.float32)
        threshold, take = np.float32(np.nan), 0
        if bool(d['first_of_video'][i]):                # frame_idx == 0: kept whole (immersive.py:368-371)
            c_kept, rgb_kept = coords, rgb
        else:
            c_kept, rgb_kept = method(self, coords, rgb, last_rgb, frame)
            if frame % r['load_full_step'] != 0:        # what the method thresholded, for the tests: the same torch expressions
                t_diff = torch.abs(rgb - last_rgb).mean(-1)
                frac = r['subsample_keyframe_frac'] if frame % r['subsample_keyframe_step'] == 0 else r['subsample_frac']
                take = int(np.round(n_pixels * frac))
                diff = t_diff.numpy()
                threshold = np.float32(torch.sort(t_diff)[0][-take])
                ties = max(ties, int((diff == threshold).sum()))
        last_rgb = rgb
        pixels = c_kept[:, 8].numpy().astype(np.int32)
        assert np.array_equal(pixels.astype(np.float32), c_kept[:, 8].numpy()) and (np.diff(pixels) > 0).all()
        all_coords.append(c_kept[:, :8]); all_rgb.append(rgb_kept)
        diffs.append(diff); thresholds.append(threshold); takes.append(take); kept.append(pixels)
    assert ties >= 2, (name, 'no image with ties at its threshold')
    all_coords, all_rgb = torch.cat(all_coords, 0), torch.cat(all_rgb, 0)
    all_weights = torch.ones_like(all_coords[..., 0:1])   # get_weights, datasets/base.py:191-194
    d['video_coords'] = vcoords.numpy()
    d['diff'] = np.asarray(diffs, np.float32)
    d['threshold'] = np.asarray(thresholds, np.float32)
    d['num_take'] = np.asarray(takes, np.int64)
    d['kept'] = np.concatenate(kept).astype(np.int32)
    d['kept_rows'] = np.concatenate([[0], np.cumsum([len(k) for k in kept])]).astype(np.int64)
    d['all_inputs'] = torch.cat([all_coords, all_rgb, all_weights], -1).numpy()
    return d


def main():
    os.makedirs(OUT, exist_ok=True)
    for name in CASES:
        d = make_case(name)
        path = os.path.join(OUT, f'{name}.npz')
        np.savez_compressed(path, **d)
        counts = np.diff(d['kept_rows'])
        tied = [int((d['diff'][i] == d['threshold'][i]).sum()) for i in range(len(counts))]
        print(f"{name}: {d['all_inputs'].shape[0]} rays, kept {counts.tolist()}, num_take {d['num_take'].tolist()}, ties at the threshold {tied}, "
              f'{os.path.getsize(path) / 1024:.0f} KB')


if __name__ == '__main__':
    main()
