"""Shared by tests/test_jpeg_decode_host.py and tests/test_gpu_jpeg_decode.py: the fixtures of tests/golden/jpeg_decode
(tools/make_jpeg_decode_golden.py), files damaged by hand with the status each must give, seeded single-byte mutations, and PIL's own verdict
on a file's bytes."""
import importlib.util
import io
import os
import struct
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'jpeg_decode')
SRC = os.path.join(HERE, 'host_math', 'hr_jpeg_decode_host.cpp')
MODES = {'L': 1, 'RGB': 3, 'RGBA': 4}
SIZES = [(1, 1), (7, 1), (1, 7), (3, 5), (4, 4), (5, 2), (8, 8), (16, 16), (17, 13), (33, 31), (64, 33), (130, 70)]
OK, NO_SOI, BAD_MARKER, UNSUPPORTED, SIZE_MISMATCH, BAD_TABLE, BAD_CODE, BAD_COEF, BAD_RESTART, TRUNCATED, TOO_LONG, BAD_OFFSETS = range(12)
_cache = {}


def tool():
    """tools/make_jpeg_decode_golden.py as a module: its segment splitter and its one-block writer"""
    if 'tool' not in _cache:
        spec = importlib.util.spec_from_file_location('make_jpeg_decode_golden', os.path.join(HERE, '..', 'tools', 'make_jpeg_decode_golden.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _cache['tool'] = mod
    return _cache['tool']


def _archive(stem):
    z = np.load(os.path.join(GOLDEN, stem + '.npz'))
    files, off = z['files'], z['offsets']
    return z, [files[off[i]:off[i + 1]].tobytes() for i in range(len(off) - 1)]


def golden_files():
    """[(name, (w, h), file bytes, {'L' | 'RGB' | 'RGBA': PIL's pixels (h, w, c)})] from the per-size archives"""
    if 'golden' not in _cache:
        out = []
        for w, h in SIZES:
            z, files = _archive(f'w{w}_h{h}')
            for i, name in enumerate(z['names']):
                out.append((f'w{w}_h{h}_{name}', (w, h), files[i], {m: z[m][i] for m in MODES}))
        _cache['golden'] = out
    return _cache['golden']


def hand_files():
    """the same of hand.npz: PIL files edited by the golden tool, PIL's decode of the edited file"""
    if 'hand' not in _cache:
        z, files = _archive('hand')
        _cache['hand'] = [(f'hand_{name}', (17, 13), files[i], {m: z[m][i] for m in MODES}) for i, name in enumerate(z['names'])]
    return _cache['hand']


def refused_files():
    z, files = _archive('refused')
    return dict(zip([str(n) for n in z['names']], files))


def idct_cases():
    """(names, files, coefficients (n, 64) in natural order, PIL's pixels (n, 8, 8))"""
    z, files = _archive('idct')
    return [str(n) for n in z['names']], files, z['coefs'], z['L']


def named(name):
    """(file bytes, pixels) of a golden or hand case"""
    for n, _, d, px in golden_files() + hand_files():
        if n == name:
            return d, px
    raise KeyError(name)


def scan_range(data):
    """(first byte of entropy data, offset of the EOI marker) of a PIL-written file"""
    segs, rest = tool().segments(data)
    lo = len(data) - len(rest)
    return lo, lo + rest.rindex(b'\xff\xd9')


def pil_verdict(data, mode):
    """PIL's pixels (h, w, c) for a file's bytes, or None where PIL raises"""
    from PIL import Image
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('error', Image.DecompressionBombWarning)
            im = Image.open(io.BytesIO(data))
            if im.format != 'JPEG':
                return None
            a = np.asarray(im.convert(mode))
        return a.reshape(a.shape[0], a.shape[1], -1)
    except Exception:
        return None


def damaged_files():
    """{'size': (17, 13), 'good': (bytes, RGB pixels), 'files': {name: bytes}}; DAMAGED_STATUS says what each must give"""
    if 'damaged' not in _cache:
        t = tool()
        good, px = named('w17_h13_420_noise_q95')
        rst, _ = named('w17_h13_444_noise_q95_rst1')
        lo, eoi = scan_range(good)
        segs, rest = t.segments(good)
        files = {}
        files['no_soi'] = b'\x00' + good[1:]
        files['overlong_segment'] = good[:4] + b'\xff\xff' + good[6:]
        files['no_sos'] = good[:lo - (2 + 2 + len(segs[-1][1]))] + b'\xff\xd9'
        files['progressive'] = refused_files()['progressive']
        files['cmyk'] = refused_files()['cmyk']
        files['other_size'] = named('w16_h16_420_noise_q95')[0]
        files['no_dht'] = t.join([s for s in segs if s[0] != 0xC4], rest)
        files['no_dqt'] = t.join([s for s in segs if s[0] != 0xDB], rest)
        files['sixteen_ones'] = good[:lo] + b'\xff\x00\xff\x00' + good[lo + 4:]
        # one 8 x 8 grey block: a DC code, then four ZRL: the fourth runs past coefficient 63
        names, blocks, _, _ = idct_cases()
        one = blocks[0]
        bsegs, brest = t.segments(one)
        tables = {tb[0]: t.codes_of(tb) for mk, pl in bsegs if mk == 0xC4 for tb in t.split_tables(mk, pl)}
        bits = []
        for code, n in [tables[0x00][0]] + [tables[0x10][0xF0]] * 4:
            bits += [(code >> (n - 1 - i)) & 1 for i in range(n)]
        bits += [1] * (-len(bits) % 8)
        raw = bytes(int(''.join(map(str, bits[i:i + 8])), 2) for i in range(0, len(bits), 8))
        files['run_past_63'] = t.join(bsegs, raw.replace(b'\xff', b'\xff\x00') + b'\xff\xd9')
        at = rst.index(b'\xff\xd1', scan_range(rst)[0])
        files['rst_out_of_order'] = rst[:at + 1] + b'\xd3' + rst[at + 2:]
        files['rst_missing'] = rst[:at] + rst[at + 2:]
        files['cut_in_scan'] = good[:(lo + eoi) // 2]
        files['no_eoi'] = good[:eoi]
        files['two_bytes_more'] = good[:eoi] + b'\x12\x34' + good[eoi:]
        _cache['damaged'] = {'size': (17, 13), 'good': (good, px['RGB']), 'files': files}
    return _cache['damaged']


DAMAGED_STATUS = {'no_soi': NO_SOI, 'overlong_segment': BAD_MARKER, 'no_sos': BAD_MARKER, 'progressive': UNSUPPORTED, 'cmyk': UNSUPPORTED,
                  'other_size': SIZE_MISMATCH, 'no_dht': BAD_TABLE, 'no_dqt': BAD_TABLE, 'sixteen_ones': BAD_CODE, 'run_past_63': BAD_COEF,
                  'rst_out_of_order': BAD_RESTART, 'rst_missing': BAD_RESTART, 'cut_in_scan': TRUNCATED, 'no_eoi': TRUNCATED,
                  'two_bytes_more': TOO_LONG}
# run_past_63 is an 8 x 8 grey file of its own: it is decoded at its own size
DAMAGED_OWN_SIZE = {'run_past_63': (8, 8)}


def mutations(data, count, seed):
    """`count` copies of a file with one byte changed each, spread over the header and the entropy data"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        b = bytearray(data)
        at = int(rng.integers(2, len(b)))
        b[at] ^= int(rng.integers(1, 256))
        out.append(bytes(b))
    return out


def mutation_sources():
    return [named(n)[0] for n in ('w17_h13_420_noise_q95', 'w17_h13_422_smooth_q30_opt', 'w17_h13_grey_noise_q95_rst1', 'w17_h13_444_noise_q30_rstrows')]


def pack(path, cases):
    """the stand-alone program's input: cases [(w, h, file bytes, RGBA pixels)]"""
    with open(path, 'wb') as f:
        f.write(struct.pack('<i', len(cases)))
        for w, h, data, rgba in cases:
            f.write(struct.pack('<iiq', w, h, len(data)) + data + np.ascontiguousarray(rgba).tobytes())
