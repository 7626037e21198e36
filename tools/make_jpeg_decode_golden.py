"""Writes tests/golden/jpeg_decode/*.npz: JPEG files as PIL writes them and what PIL's convert('L' | 'RGB' | 'RGBA') reads back from
them, the fixtures of tests/test_jpeg_decode_host.py and tests/test_gpu_jpeg_decode.py.  Needs PIL only.

    python tools/make_jpeg_decode_golden.py

  w<W>_h<H>.npz  'golden': one archive per size: the cases' names, their files' bytes one after another ('files', 'offsets') and PIL's pixels
                 in the three modes, stacked ('L', 'RGB', 'RGBA').  Greyscale, 4:4:4, 4:2:2 and 4:2:0; smooth, noise, flat and 0/255
                 content; quality 30 and 95, one each of 1 and 100; optimize=True; restart_marker_blocks 1 and 3, restart_marker_rows 1.
                 The small sizes take every combination; from 33 x 31 up the noisy contents are thinned to keep the folder small (the
                 lists are VARIANTS_BIG and NOISY_BIG below).
  hand.npz       PIL files of 17 x 13 edited here: fill bytes before markers, a COM segment and an APP1 holding a whole small JPEG, the
                 tables merged into one DQT and one DHT segment, one table a segment, a table defined twice, DRI 0, other component ids,
                 bytes after EOI.  PIL's own decode of the edited file is the expectation.
  refused.npz    what the decoder refuses: PIL's progressive and CMYK files, and frame headers edited to 4:1:1 and 4:4:0, which PIL here
                 does not write ('files' only).
  idct.npz       one-block 8 x 8 grey files written bit by bit with PIL's own tables (all-ones quantisation): a single coefficient at
                 +-1 and at +-1023 (DC: +-2047) in each of the 64 positions; 'coefs' (natural order) and PIL's 'L'.
Every archive records the versions it came from ('pil_version', 'libjpeg_turbo_version').
"""
import io
import os
import struct

import numpy as np
import PIL
from PIL import Image, features

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'jpeg_decode')
SIZES = [(1, 1), (7, 1), (1, 7), (3, 5), (4, 4), (5, 2), (8, 8), (16, 16), (17, 13), (33, 31), (64, 33), (130, 70)]        # (w, h)
SUBS = {'grey': None, '444': 0, '422': 1, '420': 2}
VARIANTS = [(f'{c}_q{q}', c, q, {}) for c in ('smooth', 'noise', 'flat', 'bw') for q in (30, 95)] + [
    ('smooth_q1', 'smooth', 1, {}), ('noise_q100', 'noise', 100, {}), ('noise_q95_opt', 'noise', 95, dict(optimize=True)),
    ('smooth_q30_opt', 'smooth', 30, dict(optimize=True)), ('noise_q95_rst1', 'noise', 95, dict(restart_marker_blocks=1)),
    ('smooth_q95_rst3', 'smooth', 95, dict(restart_marker_blocks=3)), ('noise_q30_rstrows', 'noise', 30, dict(restart_marker_rows=1))]
# from 33 x 31 up: these variants in every subsampling ...
VARIANTS_BIG = {(33, 31): ('smooth_q30', 'smooth_q95', 'flat_q95', 'smooth_q1', 'smooth_q30_opt', 'smooth_q95_rst3'),
                (64, 33): ('smooth_q30', 'flat_q95', 'smooth_q1', 'smooth_q30_opt', 'smooth_q95_rst3'),
                (130, 70): ('flat_q95',)}
# ... and the noisy ones only here: {size: {variant: subsamplings}}
NOISY_BIG = {(33, 31): {'noise_q100': ('420', '422'), 'noise_q95': ('444', 'grey'), 'bw_q30': ('420',), 'noise_q95_opt': ('422',),
                        'noise_q95_rst1': ('444', '420'), 'noise_q30_rstrows': ('422', 'grey')},
             (64, 33): {'noise_q95': ('420', 'grey'), 'noise_q95_opt': ('444',), 'noise_q95_rst1': ('grey',), 'noise_q30_rstrows': ('422',)},
             (130, 70): {'noise_q95': ('420', 'grey'), 'noise_q95_rst1': ('grey',), 'smooth_q1': ('444', '422'), 'smooth_q95_rst3': ('grey',)}}
MODES = ('L', 'RGB', 'RGBA')


def image(content, w, h, grey, seed):
    rng = np.random.default_rng(seed)
    c = 1 if grey else 3
    if content == 'noise':
        a = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    elif content == 'bw':
        a = (rng.integers(0, 2, (h, w, c)) * 255).astype(np.uint8)
    elif content == 'flat':
        a = np.broadcast_to(np.array([200, 40, 120][:c], np.uint8), (h, w, c)).copy()
    else:
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), 255 - (x + y) * 255 // max(w + h - 2, 1)][:c], -1).astype(np.uint8)
    return Image.fromarray(a[..., 0] if grey else a)


def save(im, sub, quality, **kw):
    b = io.BytesIO()
    if SUBS[sub] is None:
        im.save(b, 'JPEG', quality=quality, **kw)
    else:
        im.save(b, 'JPEG', quality=quality, subsampling=SUBS[sub], **kw)
    return b.getvalue()


def pil_pixels(data):
    out = {}
    for m in MODES:
        a = np.asarray(Image.open(io.BytesIO(data)).convert(m))
        out[m] = a.reshape(a.shape[0], a.shape[1], -1)
    return out


def versions():
    return dict(pil_version=PIL.__version__, libjpeg_turbo_version=str(features.version('libjpeg_turbo')))


def write(name, names, files, pixels=None, **more):
    off = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
    arrays = dict(names=np.array(names), files=np.frombuffer(b''.join(files), np.uint8), offsets=off, **versions(), **more)
    if pixels is not None:
        arrays.update({m: np.stack([p[m] for p in pixels]) for m in MODES})
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, **arrays)
    print(f'{name}: {len(names)} files, {os.path.getsize(path)} bytes')


# ---- the container, for the edits ----
def segments(data):
    """[(marker, payload)] up to and including SOS, then the rest of the file (entropy data, EOI and whatever follows)"""
    assert data[:2] == b'\xff\xd8'
    p, out = 2, []
    while True:
        assert data[p] == 0xFF
        mk, n = data[p + 1], struct.unpack('>H', data[p + 2:p + 4])[0]
        out.append((mk, data[p + 4:p + 2 + n]))
        p += 2 + n
        if mk == 0xDA:
            return out, data[p:]


def join(segs, rest, fill=0):
    return b'\xff\xd8' + b''.join(b'\xff' * (fill + 1) + bytes([mk]) + struct.pack('>H', len(pl) + 2) + pl for mk, pl in segs) + rest


def split_tables(mk, payload):
    out = []
    while payload:
        n = 65 if mk == 0xDB else 17 + sum(payload[1:17])
        out.append(payload[:n])
        payload = payload[n:]
    return out


def hand_files():
    w, h = 17, 13
    base = save(image('smooth', w, h, False, 5), '420', 90)
    noisy = save(image('noise', w, h, False, 6), '422', 95, restart_marker_blocks=2)
    thumb = save(image('noise', 8, 8, False, 7), '444', 50)
    out = {}
    for tag, data in (('smooth420', base), ('noise422rst', noisy)):
        segs, rest = segments(data)
        eoi = rest.rindex(b'\xff\xd9')
        out[f'{tag}_fill'] = join(segs, rest[:eoi] + b'\xff\xff\xff\xd9', fill=2)
        out[f'{tag}_com_app1'] = join(segs[:1] + [(0xFE, b'a comment \xff\xd9 with a marker inside'), (0xE1, b'Exif\0\0' + thumb)] + segs[1:], rest)
        tables = {mk: [t for m, pl in segs if m == mk for t in split_tables(mk, pl)] for mk in (0xDB, 0xC4)}
        others = [s for s in segs if s[0] not in (0xDB, 0xC4)]
        out[f'{tag}_merged'] = join(others[:-2] + [(0xDB, b''.join(tables[0xDB]))] + others[-2:-1] + [(0xC4, b''.join(tables[0xC4]))] + others[-1:], rest)
        out[f'{tag}_one_table_a_segment'] = join(others[:-2] + [(0xDB, t) for t in tables[0xDB]] + others[-2:-1] + [(0xC4, t) for t in tables[0xC4]] + others[-1:], rest)
        wrong = bytes([tables[0xDB][0][0]]) + bytes([99] * 64)
        out[f'{tag}_redefined'] = join(segs[:1] + [(0xDB, wrong), (0xC4, tables[0xC4][1][:1] + tables[0xC4][0][1:])] + segs[1:], rest)
        if not any(mk == 0xDD for mk, _ in segs):
            out[f'{tag}_dri0'] = join(segs[:-1] + [(0xDD, b'\0\0')] + segs[-1:], rest)
        renamed = []
        for mk, pl in segs:
            if mk == 0xC0:
                pl = bytearray(pl)
                for i in range(3):
                    pl[6 + 3 * i] = (10, 20, 200)[i]
            elif mk == 0xDA:
                pl = bytearray(pl)
                for i in range(3):
                    pl[1 + 2 * i] = (10, 20, 200)[i]
            renamed.append((mk, bytes(pl)))
        out[f'{tag}_ids'] = join(renamed, rest)
        out[f'{tag}_after_eoi'] = data + b'\xff\xd0junk\xff\xd9\xff\xda\x00'
    return w, h, out


# ---- one block, bit by bit ----
NATURAL = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43,
           36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def codes_of(table):
    counts, vals = table[1:17], table[17:]
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def one_block(template, coefs_zz):
    """the template's file with its entropy data replaced by one block of the given coefficients (zig-zag order)"""
    segs, rest = segments(template)
    tables = {t[0]: codes_of(t) for mk, pl in segs if mk == 0xC4 for t in split_tables(mk, pl)}
    dc, ac = tables[0x00], tables[0x10]
    bits = []

    def put(value, n):
        bits.extend((value >> (n - 1 - i)) & 1 for i in range(n))

    def amplitude(v):
        s = abs(v).bit_length()
        return s, (v if v > 0 else v + (1 << s) - 1)

    s, a = amplitude(coefs_zz[0])
    put(*dc[s]); put(a, s)
    run = 0
    for k in range(1, 64):
        if coefs_zz[k] == 0:
            run += 1
            continue
        while run > 15:
            put(*ac[0xF0]); run -= 16
        s, a = amplitude(coefs_zz[k])
        put(*ac[(run << 4) | s]); put(a, s)
        run = 0
    if run:
        put(*ac[0x00])
    bits += [1] * (-len(bits) % 8)
    raw = bytes(int(''.join(map(str, bits[i:i + 8])), 2) for i in range(0, len(bits), 8))
    return join(segs, raw.replace(b'\xff', b'\xff\x00') + b'\xff\xd9')


def idct_files():
    template = save(Image.fromarray(np.full((8, 8), 128, np.uint8)), 'grey', 100)
    assert all(v == 1 for mk, pl in segments(template)[0] if mk == 0xDB for v in pl[1:])
    names, files, coefs, pixels = [], [], [], []
    for k in range(64):
        top = 2047 if k == 0 else 1023
        for v in (1, -1, top, -top):
            zz = [0] * 64
            zz[k] = v
            data = one_block(template, zz)
            nat = np.zeros(64, np.int16)
            nat[NATURAL[k]] = v
            names.append(f'k{k}_{v}'); files.append(data); coefs.append(nat)
            pixels.append(np.asarray(Image.open(io.BytesIO(data)).convert('L')))
    return names, files, np.stack(coefs), np.stack(pixels)


def main():
    os.makedirs(OUT, exist_ok=True)
    for w, h in SIZES:
        names, files, pixels = [], [], []
        for si, sub in enumerate(SUBS):
            for vi, (vname, content, q, kw) in enumerate(VARIANTS):
                if w * h >= 1000 and vname not in VARIANTS_BIG[(w, h)] and sub not in NOISY_BIG[(w, h)].get(vname, ()):
                    continue
                data = save(image(content, w, h, sub == 'grey', 1000 * si + vi), sub, q, **kw)
                names.append(f'{sub}_{vname}'); files.append(data); pixels.append(pil_pixels(data))
        write(f'w{w}_h{h}', names, files, pixels)
    w, h, hand = hand_files()
    write('hand', list(hand), list(hand.values()), [pil_pixels(d) for d in hand.values()])
    refused = {'progressive': save(image('smooth', 17, 13, False, 1), '420', 80, progressive=True)}
    b = io.BytesIO()
    image('smooth', 17, 13, False, 2).convert('CMYK').save(b, 'JPEG', quality=80)
    refused['cmyk'] = b.getvalue()
    # PIL's '4:1:1' is its old name for 4:2:0, and it writes no 4:4:0: other sampling factors come from an edit of the frame header
    for tag, hv in (('edited_411', 0x41), ('edited_440', 0x12)):
        segs, rest = segments(save(image('smooth', 17, 13, False, 3), '420', 80))
        segs = [(mk, pl[:7] + bytes([hv]) + pl[8:]) if mk == 0xC0 else (mk, pl) for mk, pl in segs]
        refused[tag] = join(segs, rest)
    write('refused', list(refused), list(refused.values()))
    names, files, coefs, px = idct_files()
    write('idct', names, files, coefs=coefs, L=px)


if __name__ == '__main__':
    main()
