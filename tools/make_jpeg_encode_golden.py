"""Writes tests/golden/jpeg_encode/*.npz: seeded input images and the complete files PIL writes for them,

    Image.fromarray(a).save(f, 'JPEG', quality=q, subsampling=s[, restart_marker_rows=r])

which hr_jpeg_encode and its host build must reproduce byte for byte (tests/test_jpeg_encode_host.py, tests/test_gpu_jpeg_encode.py).
Needs PIL (the fixtures are PIL 12.2.0 / libjpeg-turbo's) and the host build of csrc/hr_jpeg_encode.h, whose scan statistics say
whether the set holds what it must: a scan with stuffed bytes, one with an F0 code, a DC category 11 and an AC category 10.

    python tools/make_jpeg_encode_golden.py

An archive holds: names; meta (n, 7) int32 = width, height, channels, quality, subsampling, restart rows, 1 for a float32 input;
inputs / in_offsets, the inputs' raw bytes one after another; files / offsets, PIL's files likewise.  A float input lies in
[-0.5, 1.5] and PIL gets to8b of it; an RGBA input goes to PIL as its convert('RGB'), which drops the alpha byte."""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, '..', 'tests', 'golden', 'jpeg_encode')
SMALL = [(1, 1), (3, 3), (4, 4), (8, 8), (9, 7), (7, 9), (16, 16), (17, 17), (33, 15), (15, 33), (40, 24), (2, 70), (70, 2)]      # width x height
LARGE = (136, 104)      # 4:2:0: 9 x 7 MCUs of 6 blocks = 378 blocks, 4:4:4 663: two and three workgroups of the block scan; scans of 3 KB and more
MODES = [('grey', 1, 0), ('444', 3, 0), ('422', 3, 1), ('420', 3, 2)]
QUALITIES = [1, 50, 90, 100]
CONTENTS = ['noise', 'binary', 'ramp', 'flat']


def to8b(x):
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def content(kind, w, h, c, seed):
    """uint8 (h, w, c): noise, 0 / 255 noise, a ramp, a flat colour, 8 x 8 squares of 0 and 255 ('checker'), half-black half-white blocks
    ('steps')"""
    rng = np.random.default_rng(seed)
    if kind == 'noise':
        a = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    elif kind == 'binary':
        a = (rng.integers(0, 2, (h, w, c)) * 255).astype(np.uint8)
    elif kind == 'ramp':
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([(x * 255 // max(w - 1, 1) + 3 * y + 40 * k) % 256 for k in range(c)], -1).astype(np.uint8)
    elif kind == 'flat':
        a = np.broadcast_to(np.array([200, 77, 31, 128][:c], np.uint8), (h, w, c)).copy()
    elif kind == 'checker':
        y, x = np.mgrid[0:h, 0:w]
        a = np.repeat(((((x // 8) + (y // 8)) & 1) * 255).astype(np.uint8)[..., None], c, -1)
    elif kind == 'steps':
        y, x = np.mgrid[0:h, 0:w]
        a = np.repeat((((x // 4) & 1) * 255).astype(np.uint8)[..., None], c, -1)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a)


def as_float(a, seed):
    """float32 in [-0.5, 1.5] whose to8b is not `a` but close to it: bytes spread over their bins, the ends beyond [0, 1]"""
    rng = np.random.default_rng(seed)
    x = (a.astype(np.float32) + rng.random(a.shape, dtype=np.float32)) / 256.0
    x = np.where(a == 0, -0.5 * rng.random(a.shape, dtype=np.float32), x)
    x = np.where(a == 255, 1.0 + 0.5 * rng.random(a.shape, dtype=np.float32), x)
    return np.ascontiguousarray(x.astype(np.float32))


def pil_file(a, quality, subsampling, restart_rows):
    """PIL's file for a uint8 (h, w, c) array, c 1, 3 or 4 (alpha dropped by convert('RGB'))"""
    from PIL import Image
    im = Image.fromarray(a[..., 0]) if a.shape[2] == 1 else Image.fromarray(a).convert('RGB') if a.shape[2] == 4 else Image.fromarray(a)
    kw = {'restart_marker_rows': restart_rows} if restart_rows else {}
    if a.shape[2] != 1:
        kw['subsampling'] = subsampling
    f = io.BytesIO()
    im.save(f, 'JPEG', quality=quality, **kw)
    return f.getvalue()


def cases_of(w, h, large=False):
    """[(name, channels, quality, subsampling, restart_rows, content, is_float)]"""
    out = []
    if large:
        return [('grey_noise_q90', 1, 90, 0, 0, 'noise', 0), ('420_binary_q100', 3, 100, 2, 0, 'binary', 0), ('420_noise_q90_rst1', 3, 90, 2, 1, 'noise', 0),
                ('422_ramp_q50', 3, 50, 1, 0, 'ramp', 0), ('444_noise_q50_rst2', 3, 50, 0, 2, 'noise', 0)]
    for mode, c, sub in MODES:
        for q in QUALITIES:
            for kind in CONTENTS:
                out.append((f'{mode}_{kind}_q{q}', c, q, sub, 0, kind, 0))
    if (w, h) in ((16, 16), (17, 17), (40, 24), (2, 70), (70, 2)):
        for rr in (1, 2):
            out += [(f'420_noise_q90_rst{rr}', 3, 90, 2, rr, 'noise', 0), (f'grey_binary_q100_rst{rr}', 1, 100, 0, rr, 'binary', 0),
                    (f'422_ramp_q50_rst{rr}', 3, 50, 1, rr, 'ramp', 0), (f'444_noise_q50_rst{rr}', 3, 50, 0, rr, 'noise', 0)]
    if (w, h) in ((1, 1), (9, 7), (17, 17), (40, 24)):
        out += [('420_rgba_noise_q90', 4, 90, 2, 0, 'noise', 0), ('444_rgba_ramp_q50', 4, 50, 0, 0, 'ramp', 0), ('422_rgba_binary_q100', 4, 100, 1, 0, 'binary', 0),
                ('420_noise_q90_f32', 3, 90, 2, 0, 'noise', 1), ('grey_ramp_q50_f32', 1, 50, 0, 0, 'ramp', 1), ('444_binary_q100_f32', 3, 100, 0, 0, 'binary', 1),
                ('420_rgba_noise_q50_f32', 4, 50, 2, 0, 'noise', 1)]
    if (w, h) in ((16, 16), (40, 24)):
        out += [('grey_checker_q100', 1, 100, 0, 0, 'checker', 0), ('420_checker_q100', 3, 100, 2, 0, 'checker', 0), ('grey_steps_q100', 1, 100, 0, 0, 'steps', 0),
                ('444_steps_q100_rst1', 3, 100, 0, 1, 'steps', 0)]
    return out


def build(w, h, large=False):
    names, meta, inputs, files = [], [], [], []
    for i, (name, c, q, sub, rr, kind, is_float) in enumerate(cases_of(w, h, large)):
        a = content(kind, w, h, c, 1000 * w + 10 * h + i)
        x = as_float(a, 7 + i) if is_float else a
        names.append(name)
        meta.append((w, h, c, q, sub, rr, is_float))
        inputs.append(x.tobytes())
        files.append(pil_file(to8b(x) if is_float else a, q, sub, rr))
    return names, np.array(meta, np.int32), inputs, files


def pack(blobs):
    off = np.zeros(len(blobs) + 1, np.int64)
    off[1:] = np.cumsum([len(b) for b in blobs])
    return np.frombuffer(b''.join(blobs), np.uint8), off


def main():
    sys.path.insert(0, os.path.join(HERE, '..'))
    from hyperreel_amd import jpeg
    os.makedirs(OUT, exist_ok=True)
    seen = {'stuffed': 0, 'zrl': 0, 'max_dc_cat': 0, 'max_ac_cat': 0}
    total = differ = 0
    for w, h in SMALL + [LARGE]:
        names, meta, inputs, files = build(w, h, (w, h) == LARGE)
        for name, m, x, f in zip(names, meta, inputs, files):
            a = np.frombuffer(x, np.float32 if m[6] else np.uint8).reshape(h, w, m[2])
            got, st = jpeg.encode_host(a, quality=int(m[3]), subsampling=int(m[4]), restart_rows=int(m[5]), with_stats=True)
            total += 1
            differ += got != f
            if got == f:                                              # the statistics are those of PIL's scan only when the bytes are
                for k in seen:
                    seen[k] = max(seen[k], st[k])
        fb, fo = pack(files)
        ib, io_ = pack(inputs)
        path = os.path.join(OUT, f'w{w}_h{h}.npz')
        np.savez_compressed(path, names=np.array(names), meta=meta, inputs=ib, in_offsets=io_, files=fb, offsets=fo)
        print(f'{path}: {len(names)} files, {os.path.getsize(path)} bytes')
        assert os.path.getsize(path) < 256 * 1024, path
    print(f'{total} files, {differ} differ from the host build; seen: {seen}')
    assert seen['stuffed'] > 0 and seen['zrl'] > 0 and seen['max_dc_cat'] == 11 and seen['max_ac_cat'] == 10, seen


if __name__ == '__main__':
    main()
