"""Generates tests/golden/resize/*.npz by running PIL's own Image.resize on 8-bit RGB images -- the call every PIL-based dataset of the
reference makes in get_rgb (datasets/llff.py:145-163).  Run where PIL imports:

    python tools/make_resize_golden.py

TEST INFRASTRUCTURE ONLY.  The shapes, filters and the three inputs of a shape (random bytes, random 0 / 255, a checkerboard: a fixed
integer hash, tests/resize_common.py `inputs`) are resize_common's; a fixture holds `src_wh`, `dst_wh`, `filter`, `seed`, the inputs'
crc32 (`src_crc32`), PIL's bytes (`expected`: (3, h2, w2, 3)) and `pil_version`.  One file per shape and filter keeps each to a few tens
of KB.  `twostep_*`: get_rgb's two calls, `filter` to `mid_wh` and Image.BOX to `dst_wh`."""
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, 'tests'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import resize_common as RC  # noqa: E402

PIL_FILTER = {'lanczos': Image.LANCZOS, 'bilinear': Image.BILINEAR, 'bicubic': Image.BICUBIC, 'box': Image.BOX}


def pil_steps(image, steps):
    """Image.resize(wh, filter) for every (wh, filter) of `steps` in turn, as get_rgb chains them"""
    img = Image.fromarray(np.ascontiguousarray(image), 'RGB')
    for wh, filt in steps:
        img = img.resize(tuple(wh), PIL_FILTER[filt])
    return np.asarray(img)


def make_case(src_wh, dst_wh, filt, mid_wh=None):
    seed = RC.seed_of(src_wh, dst_wh)
    src = RC.inputs(src_wh, seed)
    steps = [(dst_wh, filt)] if mid_wh is None else [(mid_wh, filt), (dst_wh, 'box')]
    f = dict(src_wh=np.array(src_wh, np.int32), dst_wh=np.array(dst_wh, np.int32), filter=np.array(filt), seed=np.array(seed, np.int64),
             src_crc32=RC.crc(src), expected=np.stack([pil_steps(im, steps) for im in src]), pil_version=np.array(PIL.__version__))
    if mid_wh is not None:
        f['mid_wh'] = np.array(mid_wh, np.int32)
    return f


def main():
    os.makedirs(RC.GOLDEN, exist_ok=True)
    total = 0
    cases = [(RC.case_name(s, d, filt), (s, d, filt)) for s, d in RC.SHAPES for filt in RC.FILTERS]
    cases += [(RC.twostep_name(s, m, d, filt), (s, d, filt, m)) for s, m, d, filt in RC.TWOSTEP]
    for name, args in cases:
        path = os.path.join(RC.GOLDEN, f'{name}.npz')
        np.savez_compressed(path, **make_case(*args))
        total += os.path.getsize(path)
        print(f'{name}: {os.path.getsize(path)} bytes', flush=True)
    print(f'{len(cases)} fixtures, {total} bytes, PIL {PIL.__version__}')


if __name__ == '__main__':
    main()
