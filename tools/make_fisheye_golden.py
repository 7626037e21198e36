"""The fisheye cases of tests/fisheye_common.py through OpenCV, as the reference computes them (datasets/immersive.py:43-48, 514-564):
cv2.fisheye.undistortPoints(K = I, D = (k1, k2, 0, 0)) on the float32 pixel directions, then normalise, rotate, normalise and, for the
NDC variant, get_ndc_rays_fx_fy -- the remaining steps in float32 numpy.  One npz per case, pair and NDC variant: `rays` (n, 6) float32
from OpenCV's undistortion, `coords64` the float64 oracle, and the largest distance between them.
python tools/make_fisheye_golden.py [--out DIR]      (default tests/golden/fisheye)
OpenCV is not a dependency of this repository: where cv2 cannot be imported this exits with a message.  No test reads the output; it is
for comparing OpenCV's fixed iteration count with the model's inverse, which is the library's contract."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

try:
    import cv2
except ImportError:
    sys.exit('tools/make_fisheye_golden.py: cv2 (OpenCV) is not installed here; nothing written.  The tests do not need these files.')

import fisheye_common as FC  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'fisheye'))
args = ap.parse_args()
os.makedirs(args.out, exist_ok=True)


def cv2_undistort(k1, k2, dx, dy, dtype):
    pts = np.stack([dx, dy], -1).astype(np.float32)[:, None]
    out = cv2.fisheye.undistortPoints(pts, np.eye(3, dtype=np.float32), np.array([k1, k2, 0.0, 0.0], np.float32))[:, 0]
    return out[:, 0].astype(dtype), out[:, 1].astype(dtype)


for name, pair, ndc in FC.all_cases():
    FC.undistort, keep = cv2_undistort, FC.undistort            # the float32 evaluation with OpenCV in place of the Newton solve
    try:
        rays = FC.rays(name, pair, ndc, np.float32)
    finally:
        FC.undistort = keep
    ref = FC.oracle(name, pair, ndc)
    dist = float(np.abs(rays - ref).max())
    tag = f'{name}_k{pair[0]}_{pair[1]}_{"ndc" if ndc else "world"}'
    np.savez_compressed(os.path.join(args.out, tag + '.npz'), rays=rays, coords64=ref, pair=np.float64(pair), distance=dist)
    print(f'{tag}: OpenCV vs the oracle, L-inf {dist:.3e}', flush=True)
