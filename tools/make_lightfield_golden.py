"""Generates tests/golden/lightfield/*.npz by running the REFERENCE'S OWN two-plane ray functions (imported in-process through
oracle/refgen/ref_shim.py) on seeded synthetic light fields.  Run where the reference tree exists:

    python tools/make_lightfield_golden.py

TEST INFRASTRUCTURE ONLY.  Each fixture stores the scalar parameters, 8-bit images from a seeded generator, the views' (s, t) --
from the reference's LightfieldDataset.get_coord or StanfordLightfieldDataset.normalize_coord, called unbound on a bare object that
carries only the attributes they read -- and `rays`: what get_lightfield_rays / get_epi_rays (utils/ray_utils.py:14-78) return,
float32, views concatenated in the order of prepare_train_data's loops, t outer and s inner (datasets/lightfield.py:106-141; the
method itself stops at a leftover exit() on line 120 and is not run).  Beside it `coords64`: the same formulas evaluated in float64
by numpy on the same float32 inputs.  The distance between the two is how far one correct float32 evaluation lies from the exact
value; the tests' tolerance is derived from it (tests/lightfield_common.py).

near and far are chosen float32-representable: the reference forms far - near from Python numbers in double, the library from the
struct's float32 fields, and the two agree exactly when the fields hold the numbers exactly."""
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'oracle', 'refgen'))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, 'tests', 'golden', 'lightfield')

# case -> recipe.  wh: U x V of a view (U x S of an EPI); grid: (rows, cols) of the camera rig; step: every step-th row and column is a view
CASES = {
    # the defaults of datasets/lightfield.py: planes at -1 and 0, both scales 1, (s, t) from get_coord on a regular 2 x 3 rig
    'default_plane': dict(kind='view', wh=(37, 23), grid=(2, 3), step=1, st_scale=1.0, uv_scale=1.0, near=-1.0, far=0.0, seed=201, coords='grid'),
    # a Stanford config's shape: st_scale 0.125 (conf/experiment/dataset/stanford_*.yaml), (s, t) from normalize_coord of an irregular 5 x 5
    # rig (positions as the file names carry them, jittered), every second camera a training view
    'stanford_like': dict(kind='view', wh=(33, 21), grid=(5, 5), step=2, st_scale=0.125, uv_scale=0.8, near=-0.75, far=0.5, seed=202, coords='file'),
    # an epipolar slice with S != U
    'epi': dict(kind='epi', wh=(37, 19), aspect=37.0 / 23.0, st_scale=0.5, uv_scale=1.25, near=-1.0, far=0.0, v=0.3, t=-0.2, seed=203),
    # linspace(a, b, 1) == [a]: one column of pixels, and a slice of one camera position
    'one_wide': dict(kind='view', wh=(1, 23), grid=(1, 2), step=1, st_scale=1.0, uv_scale=1.0, near=-1.0, far=0.0, seed=204, coords='grid'),
    'epi_one_row': dict(kind='epi', wh=(29, 1), aspect=1.5, st_scale=0.25, uv_scale=1.0, near=-1.0, far=0.0, v=-0.6, t=0.45, seed=205),
}


def reference():
    """The reference's ray functions and the two dataset classes whose coordinate methods are called unbound."""
    import ref_shim
    ref_shim.install()
    for name in ('iopath', 'iopath.common', 'iopath.common.file_io', 'omegaconf', 'PIL', 'PIL.Image'):     # import-time only
        try:
            __import__(name)
        except Exception:
            sys.modules[name] = MagicMock()
    pkg = types.ModuleType('datasets')                    # the package without its __init__ (which imports every dataset)
    pkg.__path__ = [os.path.join(ref_shim.REF, 'datasets')]
    sys.modules['datasets'] = pkg
    from datasets.lightfield import LightfieldDataset
    from datasets.stanford import StanfordLightfieldDataset
    from utils import ray_utils as RU
    return RU, LightfieldDataset, StanfordLightfieldDataset


def make_inputs(name, ref):
    """The seeded inputs of a case and the reference's (s, t), as the arrays the fixture stores."""
    _, Lf, St = ref
    c = CASES[name]
    rng = np.random.default_rng(c['seed'])
    W, H = c['wh']
    d = dict(kind=np.asarray(c['kind']), width=np.asarray(W, np.int32), height=np.asarray(H, np.int32),
             aspect=np.asarray(c.get('aspect', float(W) / H), np.float64),                       # datasets/stanford.py:66
             st_scale=np.asarray(c['st_scale'], np.float64), uv_scale=np.asarray(c['uv_scale'], np.float64),
             near=np.asarray(c['near'], np.float64), far=np.asarray(c['far'], np.float64))
    if c['kind'] == 'epi':
        d['v'], d['t'] = np.asarray(c['v'], np.float64), np.asarray(c['t'], np.float64)
        return d
    rows, cols = c['grid']
    d['rows'], d['cols'] = np.asarray(rows, np.int32), np.asarray(cols, np.int32)
    st_idx = [(s_idx, t_idx) for t_idx in range(0, rows, c['step']) for s_idx in range(0, cols, c['step'])]       # lightfield.py:107-108
    d['st_idx'] = np.asarray(st_idx, np.int32)
    if c['coords'] == 'grid':
        ds = object.__new__(Lf)
        ds.rows, ds.cols = rows, cols
        st = [Lf.get_coord(ds, idx) for idx in st_idx]
    else:
        # camera (x, y) per image in file order (idx = t_idx * cols + s_idx, stanford.py:112): a jittered grid, y growing downwards
        xy = [(12.5 * s + rng.uniform(-2, 2) + 100.0, -(9.0 * t + rng.uniform(-2, 2)) + 40.0) for t in range(rows) for s in range(cols)]
        d['camera_coords'] = np.asarray(xy, np.float64)
        ds = object.__new__(St)
        ds.rows, ds.cols = rows, cols
        ds.camera_coords = [(float(x), float(y)) for x, y in xy]
        st = [St.normalize_coord(ds, ds.camera_coords[t_idx * cols + s_idx]) for s_idx, t_idx in st_idx]
    d['st'] = np.asarray([[float(s), float(t)] for s, t in st], np.float64)
    d['images'] = rng.integers(0, 256, (len(st_idx), H, W, 3), dtype=np.uint8)
    return d


def reference_rays(d, ref):
    RU = ref[0]
    W, H = int(d['width']), int(d['height'])
    kw = dict(st_scale=float(d['st_scale']), uv_scale=float(d['uv_scale']), near=float(d['near']), far=float(d['far']))
    if str(d['kind']) == 'epi':
        return RU.get_epi_rays(W, float(d['v']), H, float(d['t']), float(d['aspect']), **kw).numpy()
    return np.concatenate([RU.get_lightfield_rays(W, H, float(s), float(t), float(d['aspect']), **kw).numpy() for s, t in d['st']], 0)


def coords_float64(d):
    """The same formulas in float64 on the same float32 inputs (numpy; not the reference)."""
    f = lambda k: float(np.float32(d[k]))          # the tensor arithmetic sees the float32 of each Python number
    W, H = int(d['width']), int(d['height'])
    aspect, st_scale, uv_scale, near = f('aspect'), f('st_scale'), f('uv_scale'), f('near')
    dz = float(np.float32(float(d['far']) - float(d['near'])))
    u = np.linspace(-1.0, 1.0, W) * uv_scale

    def rays(os_, ot, u_, v_):
        os_, ot, u_, v_ = np.broadcast_arrays(os_, ot, u_, v_)
        dirs = np.stack([u_ - os_, v_ - ot, np.full(u_.shape, dz)], -1)
        dirs = dirs / np.maximum(np.linalg.norm(dirs, axis=-1, keepdims=True), 1e-12)
        return np.concatenate([np.stack([os_, ot, np.full(u_.shape, near)], -1), dirs], -1).reshape(-1, 6)

    if str(d['kind']) == 'epi':
        s = np.linspace(-1.0, 1.0, H) / aspect * st_scale
        return rays(s[:, None], f('t') * st_scale, u[None, :], f('v') * uv_scale)
    v = np.linspace(1.0, -1.0, H) / aspect * uv_scale
    out = []
    for s, t in d['st']:
        out.append(rays(float(np.float32(s)) * st_scale, float(np.float32(t)) * st_scale, u[None, :], v[:, None]))
    return np.concatenate(out, 0)


def make_case(name, ref):
    d = make_inputs(name, ref)
    d['rays'] = reference_rays(d, ref)
    d['coords64'] = coords_float64(d)
    assert d['rays'].dtype == np.float32 and d['rays'].shape == d['coords64'].shape
    return d


def main():
    os.makedirs(OUT, exist_ok=True)
    ref = reference()
    for name in CASES:
        d = make_case(name, ref)
        path = os.path.join(OUT, f'{name}.npz')
        np.savez_compressed(path, **d)
        dist = np.abs(d['rays'].astype(np.float64) - d['coords64'])
        print(f"{name}: {d['rays'].shape[0]} rays, |fp32 - fp64| origins {dist[:, :3].max():.3e} directions {dist[:, 3:].max():.3e}, "
              f'{os.path.getsize(path) / 1024:.0f} KB')


if __name__ == '__main__':
    main()
