"""CPU tests of the JPEG decoder's format statement (hyperreel_amd/csrc/hr_jpeg_decode.h) through its host build (jpeg.decode_host): exact
pixels for PIL's files and the hand-edited ones at two subsequence lengths; the rounds the self-synchronising Huffman decode takes; the
IDCT on single coefficients; narrow chroma planes; damaged files against PIL's own verdict; a stand-alone sanitizer run; the bindings.
tests/test_gpu_jpeg_decode.py holds the kernels to the same bytes, statuses and rounds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import jpeg_decode_common as D


def _decode(data, mode, size=None, subseq_bits=0):
    from hyperreel_amd import jpeg
    return jpeg.decode_host(data, mode, size=size, with_status=True, subseq_bits=subseq_bits, with_rounds=True)


# ---- exactness --------------------------------------------------------------------------------------------------------------------------
def test_fixtures_are_there():
    cases = D.golden_files()
    assert len(cases) >= 600
    for w, h in D.SIZES:
        for sub in ('grey', '444', '422', '420'):
            assert any(n.startswith(f'w{w}_h{h}_{sub}_') for n, *_ in cases), (w, h, sub)
    rst, _ = D.named('w130_h70_grey_noise_q95_rst1')
    lo, eoi = D.scan_range(rst)
    assert sum(rst[lo:eoi].count(bytes([0xFF, 0xD0 + k])) for k in range(8)) == 17 * 9 - 1          # more than eight intervals
    assert len(D.hand_files()) >= 14 and set(D.refused_files()) >= {'progressive', 'cmyk'}


@pytest.mark.parametrize('subseq_bits', [0, 128])
@pytest.mark.parametrize('group', ['golden', 'hand'])
def test_exact_pixels_in_every_mode(group, subseq_bits):
    """0 bytes differ from PIL's arrays, no tolerance, status OK"""
    cases = D.golden_files() if group == 'golden' else D.hand_files()
    bad = []
    for name, size, data, want in cases:
        for mode in D.MODES:
            got, st, _ = _decode(data, mode, subseq_bits=subseq_bits)
            if st != D.OK or got.shape != want[mode].shape or not np.array_equal(got, want[mode]):
                bad.append((name, mode, st))
    assert not bad, bad[:10]


def test_rounds_are_fewer_than_subsequences():
    """130 x 70 noise at quality 95 without restart markers, cut into subsequences of 128 bits: the lanes synchronise -- the decode is
    not one serial chain through the subsequences.  Measured here: 735 subsequences, 169 rounds: a block of this
    file spans five subsequences, the worst case for finding the block phase; at the default 1024 bits the same file takes 20."""
    data, want = D.named('w130_h70_420_noise_q95')
    lo, eoi = D.scan_range(data)
    n_sub = -(-(eoi - lo) // 16)
    got, st, rounds = _decode(data, 'RGB', subseq_bits=128)
    print(f'{n_sub} subsequences of 128 bits, {rounds} rounds')
    assert st == D.OK and np.array_equal(got, want['RGB'])
    assert n_sub >= 64
    assert 1 <= rounds < n_sub
    # one subsequence over the whole scan is the serial walk: one round
    assert _decode(data, 'RGB', subseq_bits=1 << 20)[2] == 1


def test_idct_single_coefficients():
    """a single coefficient at +-1 and at its extreme in each of the 64 positions: direct calls into the header against PIL's decode of the
    one-block files the golden tool wrote bit by bit, and the files themselves through the decoder"""
    from hyperreel_amd import jpeg
    host = jpeg.decode_host_lib()
    names, files, coefs, want = D.idct_cases()
    assert len(names) == 256
    qt = np.ones(64, np.uint8)
    for i, name in enumerate(names):
        out = np.empty(64, np.uint8)
        c = np.ascontiguousarray(coefs[i])
        wide = host.hr_jpeg_host_idct(c.ctypes.data_as(C.c_void_p), qt.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        assert wide == 0 and np.array_equal(out.reshape(8, 8), want[i]), name
        got, st, _ = _decode(files[i], 'L')
        assert st == D.OK and np.array_equal(got[..., 0], want[i]), name


@pytest.mark.parametrize('sub', ['422', '420'])
def test_narrow_chroma_planes(sub):
    """chroma planes 1, 2 and 3 samples wide: up to 2 libjpeg replicates instead of filtering"""
    widths = {}
    for name, (w, h), data, want in D.golden_files():
        if f'_{sub}_' in name and w <= 6:
            widths.setdefault((w + 1) // 2, []).append(name)
            got, st, _ = _decode(data, 'RGB')
            assert st == D.OK and np.array_equal(got, want['RGB']), name
    assert set(widths) >= {1, 2, 3}, sorted(widths)


# ---- damaged files ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(D.DAMAGED_STATUS))
def test_named_damage_gives_its_status(name):
    dm = D.damaged_files()
    size = D.DAMAGED_OWN_SIZE.get(name, dm['size'])
    got, st, _ = _decode(dm['files'][name], 'RGB', size=size)
    assert st == D.DAMAGED_STATUS[name]
    assert got.shape == (size[1], size[0], 3) and not got.any()


def _contract(data, size, mode='RGB', subseq_bits=0):
    """either the status is not OK and the image zero, or the pixels are PIL's; where PIL raises, the status is not OK"""
    got, st, _ = _decode(data, mode, size=size, subseq_bits=subseq_bits)
    want = D.pil_verdict(data, mode)
    if st != D.OK:
        assert not got.any()
        return False
    assert want is not None, 'accepted a file PIL refuses'
    assert want.shape == got.shape and np.array_equal(got, want), 'accepted a file with other pixels than PIL'
    return True


def test_truncation_at_every_byte():
    dm = D.damaged_files()
    good, im = dm['good']
    got, st, _ = _decode(good, 'RGB', size=dm['size'])
    assert st == D.OK and np.array_equal(got, im)
    for n in range(len(good)):
        got, st, _ = _decode(good[:n], 'RGB', size=dm['size'])
        assert st != D.OK and not got.any(), n
    lo, eoi = D.scan_range(good)
    for n in range(lo, eoi):                                          # the entropy data cut short, the EOI in place
        got, st, _ = _decode(good[:n] + b'\xff\xd9', 'RGB', size=dm['size'])
        assert st != D.OK and not got.any(), n


def test_single_byte_mutations_obey_the_contract():
    """400 seeded single-byte mutations across header and entropy data of four files, at both subsequence lengths"""
    accepted = refused = 0
    for k, data in enumerate(D.mutation_sources()):
        for i, bad in enumerate(D.mutations(data, 100, 2026 + k)):
            ok = _contract(bad, (17, 13), subseq_bits=128 if i & 1 else 0)
            accepted += ok
            refused += not ok
    assert refused > 100 and accepted > 20, (accepted, refused)        # both sides of the rule were exercised


# ---- the stand-alone sanitizer run --------------------------------------------------------------------------------------------------
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan']


def test_standalone_sanitizer_run(tmp_path):
    """hr_jpeg_decode_host.cpp's own main decodes good files into heap blocks of exactly the image's size under AddressSanitizer and
    UndefinedBehaviorSanitizer, then 4000 and more copies damaged by a seeded generator, each in a heap block of its own length: no report,
    every call returns, the good files have 0 bad bytes, a refused file an all-zero image.  A program of its own with the runtimes
    linked in statically; nothing is loaded into Python.  A compiler that cannot link the runtimes into a one-line program skips."""
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    r = subprocess.run(['g++', *SANITIZE, '-o', str(tmp_path / 'probe'), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip('the compiler here cannot link the sanitizer runtimes: ' + (r.stderr.strip().splitlines() or ['?'])[-1])
    exe = str(tmp_path / 'hr_jpeg_decode_standalone')
    r = subprocess.run(['g++', '-O1', '-g', *SANITIZE, '-o', exe, D.SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = [(w, h, d, px['RGBA']) for n, (w, h), d, px in D.hand_files() + D.golden_files()[::9] if w * h <= 33 * 31]
    cases += [(w, h, d, px['RGBA']) for n, (w, h), d, px in D.golden_files() if n in ('w130_h70_420_noise_q95', 'w130_h70_grey_noise_q95_rst1')]
    D.pack(tmp_path / 'pack.bin', cases)
    per_file = 4000 // len(cases) + 1
    r = subprocess.run([exe, str(tmp_path / 'pack.bin'), str(per_file)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith(f'{len(cases)} good files, 0 refused, 0 bad bytes; {per_file * len(cases)} damaged'), r.stdout
    assert r.stdout.strip().endswith('0 refused with a non-zero image') and 'runtime error' not in r.stderr and 'Sanitizer' not in r.stderr, r.stdout + r.stderr


# ---- the public functions and the bindings ----------------------------------------------------------------------------------------------
def test_decode_host_raises_with_the_status_name():
    from hyperreel_amd import jpeg
    dm = D.damaged_files()
    with pytest.raises(jpeg.JpegDecodeError) as e:
        jpeg.decode_host(dm['files']['rst_out_of_order'], 'RGB')
    assert e.value.status == D.BAD_RESTART and e.value.status_name == 'BAD_RESTART' and 'BAD_RESTART' in str(e.value)
    assert np.array_equal(jpeg.decode_host(dm['good'][0], 'RGB'), dm['good'][1])
    with pytest.raises(ValueError):
        jpeg.decode_host(dm['good'][0], 'RGB', subseq_bits=100)
    with pytest.raises(ValueError):
        jpeg.decode_host(dm['good'][0], 'LA')


def test_host_probe_says_unsupported_beforehand():
    from hyperreel_amd import jpeg, lib
    host = jpeg.decode_host_lib()
    info = lib.hr_jpeg_info()
    for name, data in D.refused_files().items():
        assert host.hr_jpeg_host_probe(data, len(data), C.byref(info)) == D.UNSUPPORTED and not info.supported, name
        assert (info.width, info.height) == (17, 13), name
    good = D.damaged_files()['good'][0]
    assert host.hr_jpeg_host_probe(good, len(good), C.byref(info)) == D.OK
    assert (info.width, info.height, info.components, info.h_samp, info.v_samp, info.restart_interval, info.supported) == (17, 13, 3, 2, 2, 0, 1)


def test_bindings_and_abi_version():
    from hyperreel_amd import lib
    names = {s[0]: s for s in lib.SYMBOLS}
    header = open(os.path.join(D.HERE, '..', 'include', 'hyperreel_hip.h')).read()
    for sym in ('hr_jpeg_probe', 'hr_jpeg_decoder_create', 'hr_jpeg_decode', 'hr_jpeg_decoder_destroy'):
        assert sym in names and sym + '(' in header, sym
    assert len(names['hr_jpeg_decoder_create'][2]) == 6 and len(names['hr_jpeg_decode'][2]) == 9
    assert lib.ABI_VERSION == 27 and '#define HR_ABI_VERSION 27' in header
    assert C.sizeof(lib.hr_jpeg_info) == 32
    short = {'NO_SOI': 'SOI', 'BAD_MARKER': 'MARKER', 'SIZE_MISMATCH': 'SIZE', 'BAD_TABLE': 'TABLE', 'BAD_CODE': 'CODE', 'BAD_COEF': 'COEF',
             'BAD_RESTART': 'RESTART', 'BAD_OFFSETS': 'OFFSETS'}
    assert len(lib.JPEG_STATUS_NAMES) == 12
    for i, name in enumerate(lib.JPEG_STATUS_NAMES[1:], 1):
        s = short.get(name, name)
        assert f'#define HR_JPEG_E_{s} {i} ' in header or f'#define HR_JPEG_E_{s} {i}\n' in header, name
