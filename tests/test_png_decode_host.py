"""CPU tests of the PNG decoder's format statement (hyperreel_amd/csrc/hr_png_decode.h) through its host build (png.decode_host): exact
pixels for PIL's files, hand-built files and the project's own; damaged files against zlib's verdict; a stand-alone sanitizer run; the
bindings.  tests/test_gpu_png_decode.py holds the kernels to the same bytes and statuses."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import png_common as P
import png_decode_common as D
from helpers import build_host_lib


def _decode(data, mode, size=None):
    from hyperreel_amd import png
    return png.decode_host(data, mode, size=size, with_status=True)


# ---- exactness --------------------------------------------------------------------------------------------------------------------------
def test_fixtures_are_there():
    cases = D.golden_files()
    assert len(cases) >= 300
    multi = [n for n, d, _ in cases if len(D.split(d)[1]) > 1]
    assert multi, 'no fixture file with more than one IDAT chunk'


@pytest.mark.parametrize('group', ['golden', 'hand', 'own'])
def test_exact_pixels_in_every_mode(group):
    """0 bytes differ, no tolerance: PIL's files against PIL's convert, hand-built files against the array that was compressed, the
    project's own files against the frame that was encoded"""
    if group == 'golden':
        cases = D.golden_files()
    else:
        cases = [(n, d, {m: D.convert(im, m) for m in D.MODES}) for n, d, im in (D.hand_files() if group == 'hand' else D.own_files())]
    assert len(cases) >= {'golden': 300, 'hand': 60, 'own': 30}[group], len(cases)
    bad = []
    for name, data, want in cases:
        for mode in D.MODES:
            got, st = _decode(data, mode)
            if st != D.OK or got.shape != want[mode].shape or not np.array_equal(got, want[mode]):
                bad.append((name, mode, st))
    assert not bad, bad[:10]


def test_hand_files_hold_what_they_are_for():
    files = {n: d for n, d, _ in D.hand_files()}
    assert all(len(p) == 1 for p in D.split(files['one_byte_idat'])[1][:-1]) and len(D.split(files['one_byte_idat'])[1]) > 100
    assert [len(p) for p in D.split(files['cuts_l9_default'])[1][:5]] == list(D.IDAT_CUTS)
    # block types: level 0 stores, Z_FIXED gives type 1, the default strategy type 2 (the first block's header bits)
    first = {n: (D.split(files[n])[1][0][2] >> 1) & 3 for n in ('l0_default_c3', 'l9_fixed_c3', 'l9_default_c3')}
    assert first == {'l0_default_c3': 0, 'l9_fixed_c3': 1, 'l9_default_c3': 2}
    # the far-match files hold 32 of their 40 rows: the last 8 rows are matches 32768 and 32767 bytes back
    assert (1 + 341 * 3) * 32 == 32768
    assert len(files['far_match']) < 32768 + 300 and len(files['far_match_32767']) < 32768 + 300
    assert len(files['flat_run']) < 400
    # ... and the decoder reads them: the cases the builder exists for, by name
    for name in ('one_byte_idat', 'cuts_l9_default', 'far_match', 'far_match_32767', 'flat_run', 'empty_idat'):
        data, im = next((d, im) for n, d, im in D.hand_files() if n == name)
        got, st = _decode(data, 'RGB')
        assert st == D.OK and np.array_equal(got, D.convert(im, 'RGB')), name


def test_length_and_distance_tables():
    """RFC 1951 3.2.5, restated here as the lists the RFC prints"""
    build_host_lib(os.path.join(D.HERE, 'host_math', '_build', 'libhr_png_decode_host.so'), D.SRC, _deps())
    lib = C.CDLL(os.path.join(D.HERE, 'host_math', '_build', 'libhr_png_decode_host.so'))
    for f in (lib.hd_length_base, lib.hd_length_ebits, lib.hd_dist_base, lib.hd_dist_ebits):
        f.argtypes, f.restype = [C.c_uint32], C.c_uint32
    lengths = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    lext = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    dists = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385,
             24577]
    dext = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in range(2)]
    assert [lib.hd_length_base(257 + i) for i in range(29)] == lengths
    assert [lib.hd_length_ebits(257 + i) for i in range(29)] == lext
    assert [lib.hd_dist_base(i) for i in range(30)] == dists
    assert [lib.hd_dist_ebits(i) for i in range(30)] == dext
    lib.hd_convert_pixel.argtypes, lib.hd_convert_pixel.restype = [C.c_uint32, C.c_int32, C.c_int32], C.c_uint32
    rng = np.random.default_rng(3)
    px = rng.integers(0, 256, (500, 1, 4), dtype=np.uint8)
    for c in (1, 2, 3, 4):
        for mode, oc in D.MODES.items():
            want = D.convert(px[..., :c], mode)
            for i in range(len(px)):
                packed = int.from_bytes(px[i, 0, :c].tobytes(), 'little')
                got = lib.hd_convert_pixel(packed, c, oc)
                assert list(got.to_bytes(4, 'little')[:oc]) == list(want[i, 0]), (c, mode, px[i, 0])


def _deps():
    csrc = os.path.join(D.HERE, '..', 'hyperreel_amd', 'csrc')
    return [D.SRC, os.path.join(csrc, 'hr_png_decode.h'), os.path.join(csrc, 'hr_png.h'), os.path.join(csrc, 'hr_math.h'),
            os.path.join(D.HERE, '..', 'include', 'hyperreel_hip.h')]


# ---- damaged files ----------------------------------------------------------------------------------------------------------------------
def _mutation_sources():
    small = P.image('disc', 17, 9, 3)
    grey = P.image('noise', 7, 5, 1)
    return [(D.build_png(small, 9), small), (D.build_png(small, 0), small), (D.build_png(small, 9, 'fixed'), small),
            (D.build_png(small, 9, 'huffman', cuts=D.IDAT_CUTS), small), (D.build_png(grey, 6), grey),
            (D.build_png(np.full((9, 17, 3), 5, np.uint8), 9, filters=0), np.full((9, 17, 3), 5, np.uint8))]


def test_single_byte_mutations_against_zlib():
    """480 seeded single-byte mutations of IDAT payloads, CRCs recomputed, and 480 more whose Adler-32 is made to fit when the deflate
    data still inflates (the checksum would otherwise refuse nearly all of them before a pixel is looked at): the decoder accepts exactly
    when zlib.decompress of the joined payload succeeds, the length is h (1 + w c) and every filter byte is at most 4, and then gives
    the numpy-unfiltered pixels; otherwise a status that is not 0 and an all-zero image"""
    rng = np.random.default_rng(2024)
    accepted = refused = 0
    for data, im in _mutation_sources():
        h, w, c = im.shape
        mode = 'L' if c == 1 else 'RGB'
        for k in range(160):
            bad, stream = D.mutate_idat(data, rng, mend_adler=k >= 80)
            want = D.zlib_verdict(stream, w, h, c)
            got, st = _decode(bad, mode, size=(w, h))
            if want is None:
                assert st != D.OK and not got.any(), (st, stream.hex())
                refused += 1
            else:
                assert st == D.OK and np.array_equal(got, want), (st, stream.hex())
                accepted += 1
    assert refused > 100 and accepted > 10, (accepted, refused)        # both sides of the rule were exercised


@pytest.mark.parametrize('name', sorted(D.DAMAGED_STATUS))
def test_named_damage_gives_its_status(name):
    dm = D.damaged_files()
    got, st = _decode(dm['files'][name], 'RGB', size=dm['size'])
    assert st == D.DAMAGED_STATUS[name]
    assert got.shape == (9, 17, 3) and not got.any()


def test_truncation_at_every_byte():
    dm = D.damaged_files()
    good, im = dm['good']
    got, st = _decode(good, 'RGB', size=dm['size'])
    assert st == D.OK and np.array_equal(got, im)
    for n in range(len(good)):
        got, st = _decode(good[:n], 'RGB', size=dm['size'])
        assert st == D.TRUNCATED and not got.any(), n
    # a stream that ends inside its IDAT chunks, the container intact: the reader runs out, not the file
    before, payloads, after = D.split(good)
    for n in range(len(payloads[0])):
        got, st = _decode(D.join(before, [payloads[0][:n]], after), 'RGB', size=dm['size'])
        assert st == D.TRUNCATED and not got.any(), n


def test_code_length_sets_as_zlib_takes_them():
    """dynamic blocks written bit by bit: an over-subscribed and an incomplete literal set are refused, a lone distance code of one bit
    and an absent distance code are taken -- each as zlib.decompress decides"""
    cases = _dynamic_block_cases()
    verdicts = {}
    for name, (stream, raw) in cases.items():
        try:
            ok = D.zlib.decompress(stream) == raw
        except D.zlib.error:
            ok = False
        data = D.assemble(D.ihdr(len(raw) - 1, 1, 1), stream)
        got, st = _decode(data, 'L', size=(len(raw) - 1, 1))
        verdicts[name] = (ok, st)
        assert (st == D.OK) == ok, (name, st)
        if ok:
            assert got.tobytes() == raw[1:]
        else:
            assert st == D.BAD_CODE and not got.any()
    assert {n: v[0] for n, v in verdicts.items()} == {'lone_distance_code': True, 'no_distance_code': True, 'oversubscribed': False,
                                                      'unassigned_distance_code': False, 'incomplete': False, 'repeat_without_previous': False}


def _canonical(table):
    codes, code = {}, 0
    for bits in range(1, 16):
        for s in sorted(table):
            if table[s] == bits:
                codes[s] = (code, bits)
                code += 1
        code <<= 1
    return codes


def _dynamic_block(lit_lens, dist_lens, symbols, repeat_first=False):
    """a zlib stream of one final dynamic block, without its Adler-32.  lit_lens / dist_lens: {symbol: code length}.  The code-length
    code gives the lengths 0..15 four bits each, so a length l travels as the 4-bit code l and the header needs no run coding; with
    repeat_first, length 15 gives its code to symbol 16, which is then sent first: a repeat with nothing before it"""
    n_lit = max(max(lit_lens) + 1, 257)
    n_dist = max(dist_lens) + 1 if dist_lens else 1
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    used = set(range(15)) | ({16} if repeat_first else {15})
    w = D.Bits()
    w.put(1, 1); w.put(2, 2)
    w.put(n_lit - 257, 5); w.put(n_dist - 1, 5); w.put(19 - 4, 4)
    for s in order:
        w.put(4 if s in used else 0, 3)
    if repeat_first:
        w.code(15, 4); w.put(0, 2)
    for l in [lit_lens.get(i, 0) for i in range(n_lit)] + [dist_lens.get(i, 0) for i in range(n_dist)]:
        w.code(l, 4)
    lit, dist = _canonical(lit_lens), _canonical(dist_lens)
    for s in symbols:
        if isinstance(s, tuple) and s[0] == 'bits':      # ('bits', value, count): a code written as it stands, assigned or not
            w.code(s[1], s[2])
        elif isinstance(s, tuple):       # (length symbol, distance symbol); none with extra bits here
            w.code(*lit[s[0]]); w.code(*dist[s[1]])
        else:
            w.code(*lit[s])
    return b'\x78\x9c' + w.bytes()


def _dynamic_block_cases():
    """{name: (zlib stream, the 5 filtered bytes of a 4 x 1 grey image it stands for)}"""
    adler = lambda raw: struct.pack('>I', D.zlib.adler32(raw))
    raw, run = bytes([0, 65, 66, 65, 66]), bytes([0, 65, 65, 65, 65])
    full = {0: 2, 65: 2, 66: 2, 256: 2}
    return {
        'no_distance_code': (_dynamic_block(full, {}, [0, 65, 66, 65, 66, 256]) + adler(raw), raw),
        'lone_distance_code': (_dynamic_block({0: 2, 65: 2, 256: 2, 257: 2}, {0: 1}, [0, 65, (257, 0), 256]) + adler(run), run),
        # the lone distance code is the bit 0; the bit 1 after a length is the unassigned one, here in the stream's last byte but one:
        # a bad code, not a truncation, the Adler-32's 32 bits follow it
        'unassigned_distance_code': (_dynamic_block({0: 2, 65: 2, 256: 2, 257: 2}, {0: 1}, [0, 65, 257, ('bits', 1, 1), 256]) + adler(run), run),
        'oversubscribed': (_dynamic_block({0: 1, 65: 1, 66: 2, 256: 2}, {}, []) + bytes(8), raw),
        'incomplete': (_dynamic_block({0: 2, 65: 2, 256: 2}, {}, []) + bytes(8), raw),
        'repeat_without_previous': (_dynamic_block(full, {}, [], repeat_first=True) + bytes(8), raw),
    }


# ---- the stand-alone sanitizer run --------------------------------------------------------------------------------------------------
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan']


def test_standalone_sanitizer_run(tmp_path):
    """hr_png_decode_host.cpp's own main decodes the good files into heap blocks of exactly the image's size under AddressSanitizer and
    UndefinedBehaviorSanitizer, then 4000 and more copies damaged by a seeded generator, each in a heap block of its own length: no report,
    every call returns, the good files have 0 bad bytes, a refused file an all-zero image.  A program of its own with the runtimes
    linked in statically; nothing is loaded into Python.  A compiler that cannot link the runtimes into a one-line program skips."""
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    r = subprocess.run(['g++', *SANITIZE, '-o', str(tmp_path / 'probe'), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip('the compiler here cannot link the sanitizer runtimes: ' + (r.stderr.strip().splitlines() or ['?'])[-1])
    exe = str(tmp_path / 'hr_png_decode_standalone')
    r = subprocess.run(['g++', '-O1', '-g', *SANITIZE, '-DHR_PNG_DECODE_STANDALONE', '-o', exe, D.SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = [(n, d, im) for n, d, im in D.hand_files() if im.size <= 61 * 47 * 4 or n in ('far_match', 'far_match_32767', 'flat_run')]
    cases += [(n, d, px['RGBA']) for n, d, px in D.golden_files()[::7]]
    pack = tmp_path / 'pack.bin'
    with open(pack, 'wb') as f:
        f.write(struct.pack('<i', len(cases)))
        for name, data, im in cases:
            h, w = im.shape[:2]
            f.write(struct.pack('<iiq', w, h, len(data)) + data + D.convert(im, 'RGBA').tobytes())
    per_file = 4000 // len(cases) + 1
    r = subprocess.run([exe, str(pack), str(per_file)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith(f'{len(cases)} good files, 0 refused, 0 bad bytes; {per_file * len(cases)} damaged'), r.stdout
    assert r.stdout.strip().endswith('0 refused with a non-zero image') and 'runtime error' not in r.stderr and 'Sanitizer' not in r.stderr, r.stdout + r.stderr


# ---- the public functions and the bindings ----------------------------------------------------------------------------------------------
def test_decode_host_raises_with_the_status_name():
    from hyperreel_amd import png
    dm = D.damaged_files()
    with pytest.raises(png.PngDecodeError) as e:
        png.decode_host(dm['files']['flipped_adler'], 'RGB')
    assert e.value.status == D.BAD_ADLER and 'BAD_ADLER' in str(e.value)
    assert np.array_equal(png.decode_host(dm['good'][0], 'RGB'), dm['good'][1])
    assert png.STATUS_NAMES[D.BAD_FILTER] == 'BAD_FILTER' and len(png.STATUS_NAMES) == 16


def test_bindings_and_abi_version():
    from hyperreel_amd import lib
    names = {s[0] for s in lib.SYMBOLS}
    header = open(os.path.join(D.HERE, '..', 'include', 'hyperreel_hip.h')).read()
    for sym in ('hr_png_probe', 'hr_png_decoder_create', 'hr_png_decode', 'hr_png_decoder_destroy'):
        assert sym in names and sym + '(' in header, sym
    assert lib.ABI_VERSION == 27 and '#define HR_ABI_VERSION 27' in header
    assert C.sizeof(lib.hr_png_info) == 32
    for i, name in enumerate(lib.PNG_STATUS_NAMES[1:], 1):
        short = {'BAD_SIGNATURE': 'SIGNATURE', 'BAD_CHUNK': 'CHUNK', 'BAD_CRC': 'CRC', 'SIZE_MISMATCH': 'SIZE', 'BAD_ZLIB_HEADER': 'ZLIB_HEADER',
                 'BAD_BLOCK': 'BLOCK', 'BAD_CODE': 'CODE', 'BAD_DISTANCE': 'DISTANCE', 'BAD_ADLER': 'ADLER', 'BAD_FILTER': 'FILTER',
                 'BAD_OFFSETS': 'OFFSETS'}.get(name, name)
        assert f'#define HR_PNG_E_{short} {i} ' in header or f'#define HR_PNG_E_{short} {i}\n' in header, name
