"""Generates tests/golden/camera/*.npz by running the REFERENCE'S OWN ray functions (imported in-process through
oracle/refgen/ref_shim.py) on seeded synthetic cameras and images.  Run where the reference tree exists:

    python tools/make_camera_golden.py

TEST INFRASTRUCTURE ONLY.  Each fixture stores the inputs (poses, intrinsics, times, camera ids, frame numbers, 8-bit images
from a seeded generator, the subsample parameters, the NDC arguments) and what the reference makes of them: `all_inputs`,
the float32 (rays, ray_dim + 4) tensor its datasets train from, composed as datasets/technicolor.py does
(get_coords :360-396, subsample :211-236, prepare_train_data / update_all_data :238-282).  Beside it `coords64`: the same
formulas evaluated in float64 on the same float32 inputs.  The distance between the two is how far one correct float32
evaluation lies from the exact value; the tests' tolerance is derived from it (tests/test_camera_host.py)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'oracle', 'refgen'))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, 'tests', 'golden', 'camera')

# case -> recipe.  wh: the images' size; ndc_wh: the dataset size NDC is taken at (None: no NDC); video: 8-column rays
CASES = {
    # technicolor's layout: 3 cameras x 9 frames in load order (frame-major), its shipped subsample steps, smaller fractions' inverse
    'video_ndc': dict(wh=(24, 14), cams=3, frames=9, video=True, ndc_wh=(24, 14), near=0.95, seed=101,
                      rule=dict(load_full_step=8, subsample_keyframe_step=4, subsample_keyframe_frac=0.25, subsample_frac=0.125)),
    # one static pinhole image, world-space rays, 6 columns, odd sizes
    'static_pinhole': dict(wh=(61, 47), cams=1, frames=1, video=False, ndc_wh=None, near=None, seed=102, rule=None),
    # frames of 64 x 36 with a scaled K through the NDC of a 128 x 72 dataset (the viewer's case, utils/gui_utils.py:151-158)
    'ndc_other_size': dict(wh=(64, 36), cams=2, frames=2, video=True, ndc_wh=(128, 72), near=1.0, seed=103,
                           rule=dict(load_full_step=2, subsample_keyframe_step=1, subsample_keyframe_frac=0.2, subsample_frac=0.2)),
}


def _rot(rng, deg):
    """a rotation of up to ~deg degrees about a random axis (Rodrigues), float64"""
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    a = np.radians(deg) * rng.uniform(0.3, 1.0)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx)


def make_inputs(name):
    """The seeded inputs of a case, as the arrays the fixture stores."""
    c = CASES[name]
    rng = np.random.default_rng(c['seed'])
    W, H = c['wh']
    n = c['cams'] * c['frames']
    cam_pose = [np.concatenate([_rot(rng, 10.0), rng.uniform(-0.5, 0.5, (3, 1))], 1) for _ in range(c['cams'])]
    sw, sh = (W / c['ndc_wh'][0], H / c['ndc_wh'][1]) if c['ndc_wh'] else (1.0, 1.0)
    base_w, base_h = c['ndc_wh'] if c['ndc_wh'] else (W, H)
    f0 = np.float32(1.2 * base_w)
    cam_K = []
    for _ in range(c['cams']):
        f = np.float32(f0 * rng.uniform(0.97, 1.03))
        cam_K.append(np.array([[f * sw, 0, (base_w / 2 + rng.uniform(-2, 2)) * sw], [0, f * sh, (base_h / 2 + rng.uniform(-2, 2)) * sh], [0, 0, 1]]))
    poses, Ks, times, cam_ids, frames = [], [], [], [], []
    for fr in range(c['frames']):                       # technicolor's image order: all cameras of frame 0, then of frame 1, ...
        for cam in range(c['cams']):
            poses.append(cam_pose[cam]); Ks.append(cam_K[cam]); frames.append(fr); cam_ids.append(cam)
            times.append(fr / (c['frames'] - 1) if c['frames'] > 1 else 0.0)
    d = dict(images=rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8), poses=np.asarray(poses, np.float32), intrinsics=np.asarray(Ks, np.float32),
             times=np.asarray(times, np.float64), cam_ids=np.asarray(cam_ids, np.int32), frames=np.asarray(frames, np.int32),
             img_wh=np.asarray([W, H], np.int32), video=np.asarray(c['video']))
    if c['ndc_wh']:
        d['ndc'] = np.asarray([float(f0), float(f0), c['near'], c['ndc_wh'][0], c['ndc_wh'][1]], np.float64)      # fx, fy, near, width, height
    if c['rule']:
        r = c['rule']
        d['rule'] = np.asarray([r['load_full_step'], r['subsample_keyframe_step'], r['subsample_keyframe_frac'], r['subsample_frac']], np.float64)
    return d


def _pixel_grid(H, W, normalized_coordinates=False, device='cpu'):
    """ref_shim mocks kornia; this is the grid kornia.create_meshgrid documents for normalized_coordinates=False:
    (1, H, W, 2) float32, [..., 0] = x (column), [..., 1] = y (row), unnormalised, row-major."""
    assert not normalized_coordinates
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    return torch.stack([x, y], -1)[None]


def reference_all_inputs(d):
    """The reference's functions composed as datasets/technicolor.py composes them.  Returns (all_inputs float32, rules [(every, offset)])."""
    import ref_shim
    ref_shim.install()
    from utils import ray_utils as RU
    RU.create_meshgrid = _pixel_grid
    W, H = int(d['img_wh'][0]), int(d['img_wh'][1])
    video = bool(d['video'])
    keyframe_offset = frame_offset = 0
    all_coords, all_rgb, rules = [], [], []
    for idx in range(d['poses'].shape[0]):
        K = torch.FloatTensor(d['intrinsics'][idx])
        c2w = torch.FloatTensor(d['poses'][idx])
        directions = RU.get_ray_directions_K(H, W, K, centered_pixels=True)
        rays_o, rays_d = RU.get_rays(directions, c2w)
        rays = torch.cat([rays_o, rays_d], dim=-1)
        if 'ndc' in d:                                    # to_ndc: the DATASET's img_wh, K and near as Python numbers
            fx, fy, near, nw, nh = [float(v) for v in d['ndc']]
            rays = RU.get_ndc_rays_fx_fy(int(nh), int(nw), fx, fy, near, rays)
        if video:
            rays = torch.cat([rays, torch.ones_like(rays[..., :1]) * int(d['cam_ids'][idx])], dim=-1)
            rays = torch.cat([rays, torch.ones_like(rays[..., :1]) * float(d['times'][idx])], dim=-1)
        rgb = torch.from_numpy(d['images'][idx]).reshape(-1, 3).to(torch.float32).div(255)        # ToTensor (torchvision is mocked by the shim)
        if 'rule' in d:                                   # subsample(): the checkerboard mask with the running offsets
            full, key, kfrac, frac = int(d['rule'][0]), int(d['rule'][1]), float(d['rule'][2]), float(d['rule'][3])
            frame = int(d['frames'][idx])
            if frame % full == 0:
                rules.append((1, 0))
            else:
                if frame % key == 0:
                    every, offset = int(np.round(1.0 / kfrac)), keyframe_offset
                    keyframe_offset += 1
                else:
                    every, offset = int(np.round(1.0 / frac)), frame_offset
                    frame_offset += 1
                pixels = RU.get_pixels_for_image(H, W).reshape(-1, 2).long()
                mask = ((pixels[..., 0] + pixels[..., 1] + offset) % every) == 0.0
                rays, rgb = rays[mask].view(-1, rays.shape[-1]), rgb[mask].view(-1, rgb.shape[-1])
                rules.append((every, offset))
        else:
            rules.append((1, 0))
        all_coords.append(rays)
        all_rgb.append(rgb)
    all_coords, all_rgb = torch.cat(all_coords, 0), torch.cat(all_rgb, 0)
    all_weights = torch.ones_like(all_coords[..., 0:1])   # get_weights, datasets/base.py:191-194
    return torch.cat([all_coords, all_rgb, all_weights], -1).numpy(), rules


def coords_float64(d, rules):
    """The same formulas in float64 on the same float32 inputs (numpy; not the reference): columns 0..5 of every kept ray."""
    W, H = int(d['img_wh'][0]), int(d['img_wh'][1])
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    x, y = x.reshape(-1), y.reshape(-1)
    out = []
    for idx in range(d['poses'].shape[0]):
        K, c2w = d['intrinsics'][idx].astype(np.float64), d['poses'][idx].astype(np.float64)
        dirs = np.stack([(x - K[0, 2] + 0.5) / K[0, 0], -(y - K[1, 2] + 0.5) / K[1, 1], -np.ones_like(x)], -1)
        rd = dirs @ c2w[:, :3].T
        rd = rd / np.maximum(np.linalg.norm(rd, axis=-1, keepdims=True), 1e-12)
        ro = np.broadcast_to(c2w[:, 3], rd.shape)
        if 'ndc' in d:
            fx, fy, near, nw, nh = [float(v) for v in d['ndc']]
            near = float(np.float32(near))              # the tensor arithmetic sees the float32 of the Python number
            t = -(near + ro[:, 2]) / rd[:, 2]
            ro = ro + t[:, None] * rd
            ox_oz, oy_oz = ro[:, 0] / ro[:, 2], ro[:, 1] / ro[:, 2]
            sx, sy = float(np.float32(-1. / (nw / (2. * fx)))), float(np.float32(-1. / (nh / (2. * fy))))
            o2 = 1. + 2. * near / ro[:, 2]
            ro, rd = (np.stack([sx * ox_oz, sy * oy_oz, o2], -1),
                      np.stack([sx * (rd[:, 0] / rd[:, 2] - ox_oz), sy * (rd[:, 1] / rd[:, 2] - oy_oz), 1 - o2], -1))
        rays = np.concatenate([ro, rd], -1)
        every, offset = rules[idx]
        out.append(rays[((x.astype(np.int64) + y.astype(np.int64) + offset) % every) == 0])
    return np.concatenate(out, 0)


def make_case(name):
    d = make_inputs(name)
    d['all_inputs'], rules = reference_all_inputs(d)
    d['rules'] = np.asarray(rules, np.int32)
    d['coords64'] = coords_float64(d, rules)
    assert d['coords64'].shape[0] == d['all_inputs'].shape[0]
    return d


def main():
    os.makedirs(OUT, exist_ok=True)
    for name in CASES:
        d = make_case(name)
        path = os.path.join(OUT, f'{name}.npz')
        np.savez_compressed(path, **d)
        dist = np.abs(d['all_inputs'][:, :6].astype(np.float64) - d['coords64'])
        print(f"{name}: {d['all_inputs'].shape[0]} rays, |fp32 - fp64| origins {dist[:, :3].max():.3e} directions {dist[:, 3:].max():.3e}, "
              f'{os.path.getsize(path) / 1024:.0f} KB')


if __name__ == '__main__':
    main()
