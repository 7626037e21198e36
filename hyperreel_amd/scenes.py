"""Synthetic scenes: seeded random weights in the reference's state_dict layout, and rays.

There is no network for datasets or checkpoints, so benchmarks and tests render
random-weight scenes.  Weights follow the distributions
of the reference's own initialisers:

  MLP           nn.Linear default (Kaiming-uniform, a=sqrt(5)): U(+-1/sqrt(fan_in))
                for weight and bias (nlf/nets/mlp.py:127-154; weight_init `none`)
  density       relu:     1e-2 * clamp(U(0,1), 1e-2, 1e8)   (tensorf_base.py:973-987)
                softplus: 0.1 * N(0,1)                      (:957-971)
                'dense' variant: U(0, 0.5) so that alpha spans (0,1) and the
                transmittance / compositing path is exercised
  appearance    0.1 * N(0,1)                                (tensorf_base.py:932-944)
  basis_mat     nn.Linear default, no bias                  (tensorf_base.py:907-909)

The generator is numpy's PCG64 so the same seed reproduces the same scene on
the authoring container (where goldens are made) and on the GPU box.

Rays: `random_rays` mirrors the Gaussian sampler of datasets/random.py:111-125;
`pinhole_rays` follows utils/ray_utils.py:98-135 + datasets/base.py:485-518
(pixel centres +0.5, -z forward, normalised directions, optional cam_id/time).
"""
import math

import numpy as np

from .config import n_to_reso

MAT_MODE = [[0, 1], [0, 2], [1, 2]]
VEC_MODE = [2, 1, 0]
MAT_MODE_TIME = [[2, 3], [1, 3], [0, 3]]

EMB = 'model.embedding_model.embeddings.'
NET = 'model.color_model.net.'


def mlp_in_channels(pred_cfg):
    """RayPredictionEmbedding.in_channels (nlf/embedding/ray.py:231-262)."""
    total = 0
    for p in pred_cfg['params'].values():
        n_in = p['end'] - p['start']
        par = p['param']
        n = par.get('n_dims', par.get('in_channels', n_in))
        pe = p.get('pe')
        if pe is not None:
            k = 2 * pe['n_freqs']
            n = n * (k if pe.get('exclude_identity', False) else k + 1)
        total += n
    return total


def _stage_layer_shapes(stage, n_out):
    net = stage['net']
    if net['type'] == 'zero':                   # ZeroMLP: no Linear on the path (its unused Linear(1,1) is `net.layer`)
        return []
    n_in = mlp_in_channels(stage)
    W = net['hidden_channels']
    D = net['depth'] - 2
    skips = list(net.get('skips', []))
    shapes = []
    for i in range(D + 2):
        if i == 0:
            shapes.append((W, n_in))
        elif i == D + 1:
            # (a skip into the last Linear: the reference sizes it (n_out, W) and then fails in forward on cat([input, x]); the
            #  kernels and the packer define it like every other skip layer, hr_mlp_pack.h: layer_in)
            shapes.append((n_out, W + (n_in if i in skips else 0)))
        elif i in skips:
            shapes.append((W, W + n_in))
        else:
            shapes.append((W, W))
    return shapes


def mlp_layer_shapes(cfg):
    """[(out, in)] of the D+2 Linear layers of the ray_prediction net (nlf/nets/mlp.py:127-147)."""
    emb = cfg['embedding']['embeddings']
    pred = next(e for e in emb.values() if e['type'] == 'ray_prediction')
    return _stage_layer_shapes(pred, pred['z_channels'] * sum(o['channels'] for o in pred['outputs'].values()))


def point_mlp_layer_shapes(stage):
    """Same for a point_prediction stage: out = channels * (out_z // in_z) per point (embedding/point.py:106-125)."""
    per = int(stage.get('out_z_channels', 1)) // int(stage.get('in_z_channels', 1))
    return _stage_layer_shapes(stage, per * sum(o['channels'] for o in stage['outputs'].values()))


def _uniform(rng, shape, bound):
    return ((rng.random(shape, dtype=np.float32) * np.float32(2.0) - np.float32(1.0)) * np.float32(bound)).astype(np.float32)


# mlp variants of make_state_dict: (factor of every hidden Linear's weight and bias, factor of the last Linear, bias shift of the last Linear)
#   'hostile'  head x 128 next to the initialiser's (2^5 x 4), biases shifted by -2 / 0 / +2 from one head column to the next
#   'stiff'    head x 15 (1.5^5 x 2), shift 1
# The recipe VERDICT r5 names (hidden x 3, last x 8: head x 1944) is beyond what fp32 ITSELF reproduces on the full-size grids: two correct
# fp32 evaluations of the reference's algorithm (numpy's BLAS order vs torch's) then differ by more than 1e-4 RGB on 29 of 8 448 Neural-3D
# rays (1.7e-4 max), 3 of 8 448 at (2, 8, 3); (2, 4, 2) stays at 4e-5 -- the largest of the scan that leaves the 1e-4 bar meaningful.
MLP_VARIANTS = {'hostile': (2.0, 4.0, 2.0), 'stiff': (1.5, 2.0, 1.0)}


def _hostile_layer(w, b, last, colour_cols=None, variant='hostile'):
    """What a trained sample-prediction MLP can look like next to its initialiser: hidden weights and biases scaled (activations grow
    layer by layer), the last Linear scaled again with its bias shifted from one head column to the next, so that the head's sigmoids and
    tanhs run into saturation on one side and through their steep middle on the other.  The colour scale / shift columns (identity
    activations straight into the pixel) are scaled back to the initialiser's magnitude instead: blown-out colours would be clamped to
    0 / 1 and hide every error of the geometry behind them."""
    hid, fin, sh = MLP_VARIANTS[variant]
    if not last:
        return (w * np.float32(hid)).astype(np.float32), (b * np.float32(hid)).astype(np.float32)
    n = b.shape[0]
    fac = np.full(n, fin, np.float32)
    shift = (np.arange(n) % 3 - 1).astype(np.float32) * np.float32(sh)
    if colour_cols is not None:
        fac[colour_cols] = np.float32(1.0 / hid ** 5)
        shift[colour_cols] = np.float32(0.0)
    return (w * fac[:, None]).astype(np.float32), (b * fac + shift).astype(np.float32)


def _colour_columns(pred):
    """Boolean mask over the last Linear's outputs (sample-major: index = k * P + column) of the color_* heads."""
    per = []
    for name, o in pred['outputs'].items():
        per += [name.startswith('color')] * int(o['channels'])
    return np.tile(np.asarray(per, bool), int(pred['z_channels']))


def make_state_dict(cfg, dataset, grid_size=None, seed=0, density='dense', app_scale=0.1, mlp='default'):
    """{reference state_dict key: float32 ndarray} for a random-weight scene.

    grid_size: [Nx, Ny, Nz]; defaults to the config's final resolution.
    density: 'dense' | 'default' (the reference initialiser).
    app_scale: std of the appearance planes/lines (reference: 0.1; tests use 1.0 so
    that decoded colours span the whole [0,1] range instead of hugging 0.5).
    mlp: 'default' (the reference initialiser) | 'hostile' | 'stiff' (MLP_VARIANTS: the same draws, scaled and shifted)."""
    rng = np.random.default_rng(seed)
    net = cfg['color']['net']
    if grid_size is None:
        grid_size = n_to_reso(net['N_voxel_final'], net['aabb'])
    N = [int(v) for v in grid_size]
    sd = {}
    emb = cfg['embedding']['embeddings']
    pred_idx = [i for i, e in enumerate(emb.values()) if e['type'] == 'ray_prediction'][0]
    shapes = mlp_layer_shapes(cfg)
    for i, (o, n_in) in enumerate(shapes):
        mid = '.0' if i < len(shapes) - 1 else ''
        b = 1.0 / math.sqrt(n_in)
        sd[f'{EMB}{pred_idx}.net.layers.{i}{mid}.weight'] = _uniform(rng, (o, n_in), b)
        sd[f'{EMB}{pred_idx}.net.layers.{i}{mid}.bias'] = _uniform(rng, (o,), b)
        if mlp != 'default':
            kw, kb = f'{EMB}{pred_idx}.net.layers.{i}{mid}.weight', f'{EMB}{pred_idx}.net.layers.{i}{mid}.bias'
            pred = next(e for e in emb.values() if e['type'] == 'ray_prediction')
            sd[kw], sd[kb] = _hostile_layer(sd[kw], sd[kb], i == len(shapes) - 1, _colour_columns(pred), mlp)

    for pi, e in enumerate(emb.values()):        # point_prediction cascades: a second MLP, one row per coarse sample
        if e['type'] != 'point_prediction':
            continue
        pshapes = point_mlp_layer_shapes(e)
        for i, (o, n_in) in enumerate(pshapes):
            mid = '.0' if i < len(pshapes) - 1 else ''
            b = 1.0 / math.sqrt(n_in)
            sd[f'{EMB}{pi}.net.layers.{i}{mid}.weight'] = _uniform(rng, (o, n_in), b)
            sd[f'{EMB}{pi}.net.layers.{i}{mid}.bias'] = _uniform(rng, (o,), b)
    if not shapes:                              # ZeroMLP carries an unused nn.Linear(1, 1) (nlf/nets/mlp.py:27)
        sd[f'{EMB}{pred_idx}.net.layer.weight'] = _uniform(rng, (1, 1), 1.0)
        sd[f'{EMB}{pred_idx}.net.layer.bias'] = _uniform(rng, (1,), 1.0)
    for i, e in enumerate(emb.values()):        # ColorTransformEmbedding table (reference init: zeros)
        if e['type'] == 'color_transform':
            sd[f'{EMB}{i}.color_embedding'] = rng.standard_normal((int(dataset.get('total_images_per_frame', 1)), 12),
                                                                  dtype=np.float32)
    act = net.get('fea2denseAct', 'softplus')

    def dens(shape):
        if density == 'dense':
            return (rng.random(shape, dtype=np.float32) * np.float32(0.5)).astype(np.float32)
        if act == 'softplus':
            return (rng.standard_normal(shape, dtype=np.float32) * np.float32(0.1)).astype(np.float32)
        return (np.clip(rng.random(shape, dtype=np.float32), 1e-2, 1e8) * np.float32(1e-2)).astype(np.float32)

    def app(shape):
        return (rng.standard_normal(shape, dtype=np.float32) * np.float32(app_scale)).astype(np.float32)

    nd, na = list(net['n_lamb_sigma']), list(net['n_lamb_sh'])
    video = net['type'] == 'tensor_vm_split_time'
    K = int(dataset['num_keyframes'])
    sd[NET + 'aabb'] = np.asarray(net['aabb'], np.float32)
    sd[NET + 'gridSize'] = np.asarray(N, np.int64)
    for i in range(3):
        m0, m1 = MAT_MODE[i]
        if video:
            t0 = MAT_MODE_TIME[i][0]
            sd[f'{NET}density_plane_space.{i}'] = dens((1, nd[i], N[m1], N[m0]))
            sd[f'{NET}density_plane_time.{i}'] = dens((1, nd[i], K, N[t0]))
        else:
            sd[f'{NET}density_plane.{i}'] = dens((1, nd[i], N[m1], N[m0]))
            sd[f'{NET}density_line.{i}'] = dens((1, nd[i], N[VEC_MODE[i]], 1))
    for i in range(3):
        m0, m1 = MAT_MODE[i]
        if video:
            t0 = MAT_MODE_TIME[i][0]
            sd[f'{NET}app_plane_space.{i}'] = app((1, na[i], N[m1], N[m0]))
            sd[f'{NET}app_plane_time.{i}'] = app((1, na[i], K, N[t0]))
        else:
            sd[f'{NET}app_plane.{i}'] = app((1, na[i], N[m1], N[m0]))
            sd[f'{NET}app_line.{i}'] = app((1, na[i], N[VEC_MODE[i]], 1))
    app_dim = int(net.get('data_dim_color', 27))
    sd[NET + 'basis_mat.weight'] = _uniform(rng, (app_dim, sum(na)), 1.0 / math.sqrt(max(sum(na), 1)))
    if video:
        sd[NET + 'basis_mat_density.weight'] = _uniform(rng, (1, sum(nd)), 1.0 / math.sqrt(max(sum(nd), 1)))
    # MLP shading modes: renderModule.mlp.{0,2,4} (tensorf_base.py:38-69, 106-135), drawn LAST so that every other tensor of a seed is
    # what it was.  nn.Linear's default U(+-1/sqrt(fan_in)), last bias 0 as the reference sets it; the last weight x 4 spreads the
    # colours over (0.1, 0.9) instead of hugging 0.5 without saturating the sigmoid
    mode = net.get('shadingMode', 'MLP_PE')
    if mode in ('MLP_Fea', 'MLP'):
        view_pe, fea_pe, C_ = int(net.get('view_pe', 6)), int(net.get('fea_pe', 6)), int(net.get('featureC', 128))
        width = app_dim + 3 + 2 * 3 * view_pe + (2 * app_dim * fea_pe if mode == 'MLP_Fea' else 0)
        for i, (o, n_in) in zip((0, 2, 4), ((C_, width), (C_, C_), (3, C_))):
            b = 1.0 / math.sqrt(n_in)
            sd[f'{NET}renderModule.mlp.{i}.weight'] = _uniform(rng, (o, n_in), b * (4.0 if i == 4 else 1.0))
            sd[f'{NET}renderModule.mlp.{i}.bias'] = _uniform(rng, (o,), b) if i != 4 else np.zeros((o,), np.float32)
    # densityMode DensityLinear / DensityFourier: basis_mat_density has one row per function of the time basis (tensorf_dynamic.py:69-74,
    # 122-124).  Drawn LAST, over the one-row tensor every keyframe scene carries, so that every other tensor of a seed is what it was.
    # (The RGBt* colour modes need nothing here: basis_mat is drawn above with data_dim_color = 3 nb rows.)
    dmode = net.get('densityMode', 'Density')
    if video and dmode != 'Density':
        from .plan import frames_per_keyframe, time_basis_size
        rows = time_basis_size(dmode, frames_per_keyframe(net, dataset))
        sd[NET + 'basis_mat_density.weight'] = _uniform(rng, (rows, sum(nd)), 1.0 / math.sqrt(max(sum(nd), 1)))
    return sd


def state_dict_checksum(sd):
    """Order-independent fingerprint used by the golden fixtures."""
    return float(sum(float(np.sum(np.asarray(v, np.float64))) * (1 + (len(k) % 7)) for k, v in sorted(sd.items())))


# --------------------------------------------------------------------------- rays
def _normalize(v):
    n = np.sqrt(np.sum(v * v, -1, keepdims=True, dtype=np.float32))
    return (v / np.maximum(n, np.float32(1e-12))).astype(np.float32)


def random_rays(n, seed=0, video=False, pos_mean=(0.0, 0.0, 0.0), pos_std=0.1, dir_mean=(0.0, 0.0, 0.0),
                dir_std=1.0, times=None):
    """Gaussian rays about a mean (datasets/random.py:111-125)."""
    rng = np.random.default_rng(seed)
    o = np.asarray(pos_mean, np.float32)[None] + rng.standard_normal((n, 3), dtype=np.float32) * np.float32(pos_std)
    d = _normalize(np.asarray(dir_mean, np.float32)[None] + rng.standard_normal((n, 3), dtype=np.float32) * np.float32(dir_std))
    rays = np.concatenate([o, d], -1).astype(np.float32)
    if video:
        t = rng.random((n, 1), dtype=np.float32) if times is None else np.asarray(times, np.float32).reshape(-1, 1)
        rays = np.concatenate([rays, np.zeros((n, 1), np.float32), np.broadcast_to(t, (n, 1))], -1).astype(np.float32)
    return rays


def look_at_pose(eye, target, up=(0.0, 1.0, 0.0)):
    """3x4 camera-to-world with -z forward (nerf_pl convention used by get_rays)."""
    eye = np.asarray(eye, np.float64)
    f = np.asarray(target, np.float64) - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, np.float64))
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    return np.stack([r, u, -f, eye], 1).astype(np.float32)


def pinhole_rays(H, W, fov_deg, c2w, cam_id=None, time=None):
    """get_ray_directions_K(centered_pixels=True) + get_rays (utils/ray_utils.py:98-135)."""
    focal = np.float32(0.5 * W / math.tan(0.5 * math.radians(fov_deg)))
    cx, cy = np.float32(W / 2.0), np.float32(H / 2.0)
    j, i = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing='ij')
    dirs = np.stack([(i - cx + np.float32(0.5)) / focal, -(j - cy + np.float32(0.5)) / focal,
                     -np.ones_like(i)], -1).reshape(-1, 3)
    c2w = np.asarray(c2w, np.float32)
    d = _normalize(dirs @ c2w[:, :3].T)
    o = np.broadcast_to(c2w[:, 3][None], d.shape)
    rays = np.concatenate([o, d], -1).astype(np.float32)
    if time is not None:
        n = rays.shape[0]
        rays = np.concatenate([rays, np.full((n, 1), 0.0 if cam_id is None else cam_id, np.float32),
                               np.full((n, 1), time, np.float32)], -1)
    return np.ascontiguousarray(rays, np.float32)


def benchmark_rays(model_name, H=800, W=800, frame=0, num_frames=50):
    """The BASELINE ray sets: an inside-out orbit camera for the
    sphere/cylinder scenes, a forward-facing camera at z=+1 for the z-plane scenes."""
    video = not model_name.startswith('donerf')
    t = None
    if video:
        t = frame / float(max(num_frames - 1, 1))
    if 'z_plane' in model_name:
        pose = look_at_pose((0.05, 0.03, 1.0), (0.0, 0.0, -1.0))
    else:
        pose = look_at_pose((0.3, 0.0, 0.0), (1.0, 0.1, 0.05))
    return pinhole_rays(H, W, 40.0, pose, cam_id=0 if video else None, time=t)


def scale_density(sd, factor):
    """The scene with every density plane (not the lines / time planes) multiplied by `factor`: a thinner medium, whose transmittance
    decays over the whole ray instead of the first few samples.  Returns a new dict."""
    return {k: ((v * np.float32(factor)).astype(np.float32) if 'density_plane' in k and 'time' not in k else v) for k, v in sd.items()}


def carve_half_space(sd, frac=0.5):
    """Empties the scene where x lies in the lower `frac` of its axis: every density factor that spans x (the planes of pairs 0 and
    1, the line or time plane of pair 2) vanishes there, so with a relu density a ray that stays on that side has no sample with a
    weight and a ray that stays on the other side keeps all of its own.  Returns a new dict."""
    out = dict(sd)
    for k, v in sd.items():
        if 'density_' not in k:
            continue
        j, kind = int(k.rsplit('.', 1)[1]), k.split('.')[-2]
        v = v.copy()
        if j in (0, 1) and kind in ('density_plane', 'density_plane_space'):       # (1, C, N[m1], Nx)
            v[..., :int(frac * v.shape[3])] = 0.0
        elif j == 2 and kind == 'density_line':                                    # (1, C, Nx, 1)
            v[:, :, :int(frac * v.shape[2])] = 0.0
        elif j == 2 and kind == 'density_plane_time':                              # (1, C, K, Nx)
            v[..., :int(frac * v.shape[3])] = 0.0
        out[k] = v
    return out


def carve_density(sd, lo=(0.25, 0.3, 0.2), hi=(0.75, 0.8, 0.7)):
    """Empties the scene outside a sub-box (fractions of each axis) so that occupancy tests have something to find:
    only plane pair 0 keeps density, its plane vanishes outside [lo, hi] in x / y and its line (or, for keyframe nets,
    the spatial axis of its time plane) outside [lo, hi] in z.  Returns a new dict."""
    out = dict(sd)
    for k, v in sd.items():
        if 'density_' not in k:
            continue
        v = v.copy()
        j = int(k.rsplit('.', 1)[1])
        if j != 0:
            v[...] = 0.0
        elif k.split('.')[-2] in ('density_plane', 'density_plane_space'):         # (1, C, Ny, Nx)
            ny, nx = v.shape[2], v.shape[3]
            keep = np.zeros((ny, nx), bool)
            keep[int(lo[1] * ny):int(hi[1] * ny), int(lo[0] * nx):int(hi[0] * nx)] = True
            v *= keep[None, None]
        elif k.split('.')[-2] == 'density_line':                                   # (1, C, Nz, 1)
            nz = v.shape[2]
            keep = np.zeros(nz, bool)
            keep[int(lo[2] * nz):int(hi[2] * nz)] = True
            v *= keep[None, None, :, None]
        else:                                                                      # density_plane_time (1, C, K, Nz)
            nz = v.shape[3]
            keep = np.zeros(nz, bool)
            keep[int(lo[2] * nz):int(hi[2] * nz)] = True
            v *= keep[None, None, None, :]
        out[k] = v
    return out
