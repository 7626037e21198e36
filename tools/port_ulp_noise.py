"""The CPU restatement's own fp32 noise on a case of tests/test_gpu_train_dispatch.py: its end-to-end gradients with the rays and / or
every parameter moved by one fp32 ulp (all up, all down, rays only, parameters only) against the unmoved evaluation, per tensor as a
fraction of the tensor's largest entry (figures above 1e-4, with the index of the worst entry).  No GPU needed.  This is where
E2E_NOISE_BARS of that file comes from.

    python tools/port_ulp_noise.py [case]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle')]
import numpy as np
from types import SimpleNamespace
import test_gpu_train_dispatch as D

case = sys.argv[1] if len(sys.argv) > 1 else 'shiny_z_tensorf_cascaded'
sc = D._scene(case)


def move(a, direction):
    a = np.asarray(a)
    if a.dtype != np.float32 or a.size == 0 or direction == 0:
        return a
    return np.nextafter(a, np.float32(np.inf * direction)).astype(np.float32)


for white in (0, 1):
    rays = sc.rays
    G = np.random.default_rng(3).standard_normal((rays.shape[0], 3)).astype(np.float32)
    rgb0, g0 = D._reference_grads(sc, rays, G, white)
    for label, dr, dp in (('all up', 1, 1), ('all down', -1, -1), ('rays up', 1, 0), ('rays down', -1, 0), ('params up', 0, 1), ('params down', 0, -1)):
        sd = {k: (move(v, dp) if 'gridSize' not in k and 'aabb' not in k else v) for k, v in sc.state_dict.items()}
        sc1 = SimpleNamespace(cfg=sc.cfg, dataset=sc.dataset, state_dict=sd, iteration=sc.iteration, grid=sc.grid)
        rgb1, g1 = D._reference_grads(sc1, move(rays, dr), G, white)
        out = []
        for k in g0:
            if g0[k] is None or g0[k].size == 0:
                continue
            d = np.abs(g1[k].astype(np.float64) - g0[k])
            r = float(d.max() / np.abs(g0[k]).max())
            if r > 1e-4:
                out.append(f'{k} {r:.2e}@{int(d.argmax())}')
        print(f'white {white} {label}: rgb {float(np.abs(rgb1 - rgb0).max()):.1e};', ' '.join(out), flush=True)
