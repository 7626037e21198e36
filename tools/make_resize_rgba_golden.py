"""Generates tests/golden/resize_rgba/*.npz by running PIL's own Image.resize on 8-bit RGBA images -- the call the reference's RGBA
datasets make in get_rgb (datasets/blender.py:61-70, donerf.py:240-249) before they composite over white.  Run where PIL imports:

    python tools/make_resize_rgba_golden.py

TEST INFRASTRUCTURE ONLY.  The shapes, filters and the three inputs of a shape (random bytes, random 0 / 255 in all four channels,
random colours under a 0 / 255 alpha checkerboard: a fixed integer hash, tests/resize_rgba_common.py `inputs`) are resize_rgba_common's;
a fixture holds `src_wh`, `dst_wh`, `filter`, `seed`, the inputs' crc32 (`src_crc32`), PIL's bytes (`expected`: (3, h2, w2, 4)),
`pil_version` and `reach`: how many resampled premultiplied values took the two rare branches of the un-premultiply (the clamp at
c' > a', the copy at a' == 0 with c' > 0), counted on the numpy statement of the rule after it has been found equal to PIL's bytes.
Over the set both must be reached, or the fixtures would not pin them: that is asserted here.  One file per shape and filter keeps each
to a few tens of KB.  `twostep_*`: get_rgb's two calls, `filter` to `mid_wh` and Image.BOX to `dst_wh`, each a full RGBA resize."""
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
import resize_rgba_common as RA  # noqa: E402

PIL_FILTER = {'lanczos': Image.LANCZOS, 'bilinear': Image.BILINEAR, 'bicubic': Image.BICUBIC, 'box': Image.BOX}


def pil_steps(image, steps):
    """Image.resize(wh, filter) of an RGBA image for every (wh, filter) of `steps` in turn, as get_rgb chains them"""
    img = Image.fromarray(np.ascontiguousarray(image), 'RGBA')
    for wh, filt in steps:
        img = img.resize(tuple(wh), PIL_FILTER[filt])
    assert img.mode == 'RGBA'
    return np.asarray(img)


def make_case(src_wh, dst_wh, filt, mid_wh=None):
    seed = RA.seed_of(src_wh, dst_wh)
    src = RA.inputs(src_wh, seed)
    steps = [(dst_wh, filt)] if mid_wh is None else [(mid_wh, filt), (dst_wh, 'box')]
    expected = np.stack([pil_steps(im, steps) for im in src])
    # the branches the first step's un-premultiply took: on the numpy statement's premultiplied bytes, which give PIL's bytes
    first_wh = steps[0][0]
    if tuple(first_wh) == tuple(src_wh):
        reach = np.zeros(2, np.int64)
    else:
        pre = RC.np_resize(RA.np_premultiply(src), first_wh, filt)
        assert RA.np_unpremultiply(pre).tobytes() == np.stack([pil_steps(im, steps[:1]) for im in src]).tobytes(), (src_wh, first_wh, filt)
        reach = RA.reach(pre)
    f = dict(src_wh=np.array(src_wh, np.int32), dst_wh=np.array(dst_wh, np.int32), filter=np.array(filt), seed=np.array(seed, np.int64),
             src_crc32=RA.crc(src), expected=expected, pil_version=np.array(PIL.__version__), reach=reach)
    if mid_wh is not None:
        f['mid_wh'] = np.array(mid_wh, np.int32)
    return f


def main():
    os.makedirs(RA.GOLDEN, exist_ok=True)
    total, reached = 0, np.zeros(2, np.int64)
    cases = [(RA.case_name(s, d, filt), (s, d, filt)) for s, d, filt in RA.CASES]
    cases += [(RA.twostep_name(s, m, d, filt), (s, d, filt, m)) for s, m, d, filt in RA.TWOSTEP]
    for name, args in cases:
        path = os.path.join(RA.GOLDEN, f'{name}.npz')
        f = make_case(*args)
        np.savez_compressed(path, **f)
        total += os.path.getsize(path)
        reached += f['reach']
        print(f'{name}: {os.path.getsize(path)} bytes, reach {f["reach"].tolist()}', flush=True)
    assert reached[0] > 0, 'no resampled value with 0 < alpha < 255 and colour > alpha: the clamp of the un-premultiply is not pinned'
    assert reached[1] > 0, 'no resampled value with alpha 0 and colour > 0: the copy at alpha 0 is not pinned'
    print(f'{len(cases)} fixtures, {total} bytes, PIL {PIL.__version__}; un-premultiply branches reached: clamp {reached[0]}, alpha 0 {reached[1]}')


if __name__ == '__main__':
    main()
