"""Writes tests/golden/png_decode/*.npz: PNG files as PIL writes them and what PIL's convert('L' | 'RGB' | 'RGBA') reads back from them,
the fixtures of tests/test_png_decode_host.py and tests/test_gpu_png_decode.py.

    python tools/make_png_decode_golden.py

One archive per shape: the cases' names, their files' bytes one after another ('files', 'offsets') and PIL's pixels in the three
modes, stacked ('L', 'RGB', 'RGBA').  Files: colour types 0 / 2 / 4 / 6 (PIL modes L, RGB, LA, RGBA), written at compress_level 0 / 1 / 6 / 9 and with
optimize=True, contents noise, gradient and flat.  The small shapes take every combination; 64 x 33 and 130 x 70 take every variant on
the gradient and, to keep the folder small, one variant per colour type on noise and on the flat image (130 x 70: noise as L and RGBA
only).  PIL cuts IDAT chunks at its output buffer, 64 KB, which none of these files reaches: the 130 x 70 files are written with
ImageFile.MAXBLOCK = 4096, so that they hold several IDAT chunks.  The archive records the PIL version it came from ('pil_version').
"""
import io
import os
import struct
import sys

import numpy as np
import PIL
from PIL import Image, ImageFile

MAXBLOCK = ImageFile.MAXBLOCK

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'png_decode')
SHAPES = [(1, 1), (1, 7), (7, 1), (3, 5), (17, 9), (64, 33), (130, 70)]          # (w, h)
MODES = {'L': 1, 'RGB': 3, 'LA': 2, 'RGBA': 4}
VARIANTS = {'l0': dict(compress_level=0), 'l1': dict(compress_level=1), 'l6': dict(compress_level=6), 'l9': dict(compress_level=9),
            'opt': dict(optimize=True)}
CONTENTS = ['noise', 'gradient', 'flat']


def content(kind, w, h, c, rng):
    if kind == 'noise':
        return rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if kind == 'gradient':
        yy, xx = np.mgrid[0:h, 0:w]
        return ((xx[..., None] * 3 + yy[..., None] * 2 + np.arange(c) * 50) & 255).astype(np.uint8)
    return np.broadcast_to(np.array([200, 17, 90, 128][:c], np.uint8), (h, w, c)).copy()


def n_idat(data):
    at, n = 8, 0
    while at < len(data):
        ln, = struct.unpack('>I', data[at:at + 4])
        n += data[at + 4:at + 8] == b'IDAT'
        at += 12 + ln
    return n


def main():
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for w, h in SHAPES:
        rng = np.random.default_rng(100 * w + h)
        small = w * h <= 17 * 9
        last = (w, h) == SHAPES[-1]
        ImageFile.MAXBLOCK = 4096 if last else MAXBLOCK        # PIL's output buffer, and so the size of an IDAT chunk
        names, files, pixels = [], [], {'L': [], 'RGB': [], 'RGBA': []}
        pick = 0
        for mode, c in MODES.items():
            for kind in CONTENTS:
                if last and kind == 'noise' and mode in ('RGB', 'LA'):
                    continue
                variants = list(VARIANTS)
                if not small and kind != 'gradient':
                    variants = [variants[pick % len(variants)]]
                    pick += 1
                px = content(kind, w, h, c, rng)
                im = Image.fromarray(px[..., 0] if c == 1 else px, mode)
                for v in variants:
                    buf = io.BytesIO()
                    im.save(buf, 'PNG', **VARIANTS[v])
                    data = buf.getvalue()
                    names.append(f'{mode}_{kind}_{v}')
                    files.append(np.frombuffer(data, np.uint8))
                    for om in pixels:
                        pixels[om].append(np.asarray(Image.open(io.BytesIO(data)).convert(om)).reshape(h, w, -1))
                    if last and v in ('l0', 'l6'):
                        print(f'  {names[-1]}: {len(data)} bytes, {n_idat(data)} IDAT', file=sys.stderr)
        path = os.path.join(OUT, f'w{w}_h{h}.npz')
        np.savez_compressed(path, pil_version=np.array(PIL.__version__), names=np.array(names), files=np.concatenate(files),
                            offsets=np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64),
                            **{om: np.stack(v) for om, v in pixels.items()})
        total += os.path.getsize(path)
        print(f'{path}: {len(names)} files, {os.path.getsize(path)} bytes')
    print(f'{total} bytes in all')


if __name__ == '__main__':
    main()
