"""CPU tests of the JPEG encoder's format statement (hyperreel_amd/csrc/hr_jpeg_encode.h) through its host build (jpeg.encode_host): PIL's
bytes, header included, on every fixture and live against the installed PIL on shapes outside them; the quantiser against the division
on every pair; the int32 FDCT against an int64 statement; the bound; the project's own decoder on every file; the refusals and bindings;
a stand-alone sanitizer run.  tests/test_gpu_jpeg_encode.py holds the kernels to the same bytes."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

import jpeg_encode_common as E


def _encode(a, opts, **more):
    from hyperreel_amd import jpeg
    return jpeg.encode_host(E.frame_of(a), channels=a.shape[2], **opts, **more)


# ---- PIL's bytes ------------------------------------------------------------------------------------------------------------------------
def test_fixtures_are_there():
    """the shapes, modes, qualities and contents the rules can go wrong at, and the four conditions on the scans: stuffed bytes, an F0 code,
    a DC category 11, an AC category 10 (the statistics are the host encoder's, whose bytes test_host_equals_pil_on_every_fixture holds
    to PIL's)"""
    cases = E.golden()
    t = E.tool()
    assert len(cases) >= 900
    names = {n for n, *_ in cases}
    for w, h in t.SMALL:
        for mode, _, _ in t.MODES:
            for q in t.QUALITIES:
                for kind in t.CONTENTS:
                    assert f'w{w}_h{h}_{mode}_{kind}_q{q}' in names
    assert sum('_rst1' in n for n in names) >= 10 and sum('_rst2' in n for n in names) >= 10
    assert sum('_rgba_' in n for n in names) >= 8 and sum(a.dtype == np.float32 for _, a, _, _ in cases) >= 8
    for _, a, _, _ in cases:
        if a.dtype == np.float32:
            assert not np.isnan(a).any() and a.min() >= -0.5 and a.max() <= 1.5
    w, h = t.LARGE
    assert E.plan(w, h, 3, 2)['n_wg'] >= 2 and E.plan(w, h, 3, 0)['n_wg'] >= 3
    assert any(n.startswith(f'w{w}_h{h}_') and len(E.scan_of(f)) >= 3 * 1024 for n, _, _, f in cases)      # three chunks of the stuffing pass
    seen = {'stuffed': 0, 'zrl': 0, 'max_dc_cat': 0, 'max_ac_cat': 0}
    for _, a, opts, _ in cases:
        st = _encode(a, opts, with_stats=True)[1]
        seen = {k: max(v, st[k]) for k, v in seen.items()}
    assert seen['stuffed'] > 0 and seen['zrl'] > 0 and seen['max_dc_cat'] == 11 and seen['max_ac_cat'] == 10, seen
    assert any(b'\xff\x00' in E.scan_of(f) for _, _, _, f in cases)


def test_host_equals_pil_on_every_fixture():
    """0 bytes differ from PIL's files, SOI to EOI"""
    bad = [name for name, a, opts, want in E.golden() if _encode(a, opts) != want]
    print(f'{len(E.golden())} fixture files, {len(bad)} differ')
    assert not bad, bad[:10]


def test_live_against_the_installed_pil():
    """seeded shapes outside the fixtures, every mode, seven qualities, restart markers, float and RGBA input: 0 differing bytes"""
    bad = [name for name, a, opts in E.live_cases() if _encode(a, opts) != E.pil_file(a, **opts)]
    assert len(E.live_cases()) >= 35 and not bad, bad[:10]


# ---- the parts --------------------------------------------------------------------------------------------------------------------------
def test_quantiser_equals_the_division_on_every_pair():
    """every |c| <= 32767 and every table entry 1..255: (|c| + d / 2) / d with d = 8 q, the sign put back"""
    lib = E.host_lib()
    c = np.arange(-32767, 32768, dtype=np.int32)
    out = np.empty_like(c)
    for q in range(1, 256):
        d = 8 * q
        lib.hje_quant_many(c.ctypes.data_as(C.c_void_p), c.size, d, out.ctypes.data_as(C.c_void_p))
        want = np.sign(c) * ((np.abs(c) + (d >> 1)) // d)
        assert np.array_equal(out, want), q


def test_quality_scaling():
    lib = E.host_lib()
    for q in (1, 2, 25, 49, 50, 51, 75, 90, 99, 100):
        scale = 5000 // q if q < 50 else 200 - 2 * q
        for base in (1, 10, 16, 17, 99, 121, 255):
            assert lib.hje_quant_entry(base, q) == min(max((base * scale + 50) // 100, 1), 255), (q, base)


def test_fdct_int32_equals_int64_on_extreme_blocks():
    """0 / 255 checkerboards of every period, steps, constant extremes and noise: the 32-bit arithmetic holds every intermediate"""
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:8, 0:8]
    blocks = [np.full((8, 8), v) for v in (0, 255, 128)]
    for p in (1, 2, 4):
        for pat in (((x // p) + (y // p)) & 1, (x // p) & 1, (y // p) & 1):
            blocks += [pat * 255, (1 - pat) * 255]
    blocks += [(x >= k) * 255 for k in range(1, 8)] + [(y >= k) * 255 for k in range(1, 8)] + [(x + y >= k) * 255 for k in range(1, 15)]
    blocks += list(rng.integers(0, 256, (200, 8, 8))) + list(rng.integers(0, 2, (200, 8, 8)) * 255)
    samples = np.ascontiguousarray(np.stack(blocks).astype(np.int32))
    want = E.fdct_int64(samples)
    lib = E.host_lib()
    got = np.empty((8, 8), np.int32)
    for i in range(len(samples)):
        lib.hje_fdct(samples[i].ctypes.data_as(C.c_void_p), got.ctypes.data_as(C.c_void_p))
        assert np.array_equal(got, want[i]), i
    assert np.abs(want).max() <= 32767 and np.abs(want).max() >= 8 * 127 * 8      # the DC of a white block, scaled by 8, is there


def _dht_lengths(data):
    """{(class, id): {symbol: code length}} of a file's DHT segments"""
    out, p = {}, 2
    while data[p + 1] != 0xDA:
        mk, ln = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        if mk == 0xC4:
            s = data[p + 4:p + 2 + ln]
            counts, vals = s[1:17], s[17:]
            k, tab = 0, {}
            for length, n in enumerate(counts, 1):
                for _ in range(n):
                    tab[vals[k]] = length
                    k += 1
            out[(s[0] >> 4, s[0] & 15)] = tab
        p += 2 + ln
    return out


def test_bound_is_derived_from_the_longest_codes_and_holds():
    """per block the longest DC code and 63 times the longest AC code of PIL's own tables, with their magnitude bits, and an EOB; doubled
    for stuffing, plus header, markers and a pad byte per interval.  0 / 255 noise at quality 100, the longest files there are, stay
    inside it in every mode."""
    from hyperreel_amd import jpeg
    tabs = _dht_lengths(next(f for n, _, _, f in E.golden() if n == 'w16_h16_420_noise_q90'))
    dc = max(length + sym for (cls, _), tab in tabs.items() if cls == 0 for sym, length in tab.items())
    ac = max(length + (sym & 15) for (cls, _), tab in tabs.items() if cls == 1 for sym, length in tab.items())
    eob = max(tab[0] for (cls, _), tab in tabs.items() if cls == 1)
    assert E.host_lib().hje_max_block_bits() == dc + 63 * ac + eob == 22 + 63 * 26 + 4
    t = E.tool()
    for w, h in [(1, 1), (8, 8), (17, 17), (40, 24), (70, 2), (136, 104)]:
        for mode, c, sub in t.MODES + [('rgba', 4, 2)]:
            for rr in (0, 1):
                p = E.plan(w, h, c, sub, rr)
                assert p['bound'] == p['head_bytes'] + 2 * p['raw_max'] + 2 * (p['n_int'] - 1) + 2
                assert p['raw_max'] == -(-p['n_blocks'] * (dc + 63 * ac + eob) // 8) + p['n_int']
                a = t.content('binary', w, h, c, 3)
                data = _encode(a, {'quality': 100, 'subsampling': E.SUBS[sub], 'restart_rows': rr})
                assert len(data) <= p['bound'] and len(data) - len(E.scan_of(data)) - 2 == p['head_bytes']
                assert p['bound'] == jpeg.host_lib().hr_jpeg_host_bound(w, h, c, sub, rr)


def test_own_decoder_reads_every_file_as_pil_does():
    """jpeg.decode_host of every fixture file (the encoder's bytes) and of every live file equals PIL's decode of it"""
    from PIL import Image
    from hyperreel_amd import jpeg
    files = [(n, f) for n, _, _, f in E.golden()] + [(n, _encode(a, opts)) for n, a, opts in E.live_cases()]
    for name, data in files:
        want = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
        assert np.array_equal(jpeg.decode_host(data, 'RGB'), want), name


# ---- the public functions and the bindings ----------------------------------------------------------------------------------------------
def test_refusals():
    from hyperreel_amd import jpeg
    host = jpeg.host_lib()
    ok = (16, 9, 3, 2, 0)
    assert host.hr_jpeg_host_bound(*ok) > 0
    for bad in ((0, 9, 3, 2, 0), (16, 0, 3, 2, 0), (65536, 9, 3, 2, 0), (16, 65536, 3, 2, 0), (16, 9, 2, 2, 0), (16, 9, 5, 2, 0), (16, 9, 3, 3, 0),
                (16, 9, 3, -1, 0), (16, 9, 1, 2, 0), (16, 9, 1, 1, 0), (16, 9, 3, 2, -1), (65535, 9, 3, 0, 8), (65535, 65535, 3, 0, 0)):
        assert host.hr_jpeg_host_bound(*bad) == -1, bad
    assert host.hr_jpeg_host_bound(65535, 9, 3, 0, 7) > 0             # 8192 MCUs a row: seven rows fit a DRI segment, eight do not
    a = np.zeros((9, 16, 3), np.uint8)
    for opts in ({'quality': 0}, {'quality': 101}, {'subsampling': '4:1:1'}, {'subsampling': 3}, {'restart_rows': -1}, {'channels': 2}):
        with pytest.raises(ValueError):
            jpeg.encode_host(a, **opts)
    with pytest.raises(ValueError):
        jpeg.encode_host(a[..., 0], subsampling='4:2:0')              # grey takes 4:4:4 only
    with pytest.raises(ValueError):
        jpeg.encode_host(a.astype(np.float64))
    cap = host.hr_jpeg_host_bound(*ok)
    buf = np.full(cap, 0xA5, np.uint8)
    assert host.hr_jpeg_host_encode(a.ctypes.data_as(C.c_void_p), 0, 16, 9, 3, 90, 2, 0, buf.ctypes.data_as(C.c_void_p), cap - 1, None) == -1
    assert host.hr_jpeg_host_encode(a.ctypes.data_as(C.c_void_p), 2, 16, 9, 3, 90, 2, 0, buf.ctypes.data_as(C.c_void_p), cap, None) == -1
    assert (buf == 0xA5).all()
    n = host.hr_jpeg_host_encode(a.ctypes.data_as(C.c_void_p), 0, 16, 9, 3, 90, 2, 0, buf.ctypes.data_as(C.c_void_p), cap, None)
    assert n > 0 and (buf[n:] == 0xA5).all() and buf[:n].tobytes() == jpeg.encode_host(a)


def test_nan_is_zero_and_alpha_is_ignored():
    from hyperreel_amd import jpeg
    rng = np.random.default_rng(9)
    x = rng.random((17, 23, 3), dtype=np.float32) * 2 - 0.5
    holes = rng.random(x.shape) < 0.1
    assert jpeg.encode_host(np.where(holes, np.float32(np.nan), x)) == jpeg.encode_host(np.where(holes, np.float32(0), x))
    rgba = rng.integers(0, 256, (17, 23, 4), dtype=np.uint8)
    assert jpeg.encode_host(rgba, quality=75) == jpeg.encode_host(np.ascontiguousarray(rgba[..., :3]), quality=75)


def test_bindings_and_abi_version():
    from hyperreel_amd import jpeg, lib
    names = {s[0]: s for s in lib.SYMBOLS}
    header = open(os.path.join(E.HERE, '..', 'include', 'hyperreel_hip.h')).read()
    for sym, nargs in (('hr_jpeg_bound', 6), ('hr_jpeg_encoder_create', 7), ('hr_jpeg_encode', 7), ('hr_jpeg_encoder_destroy', 1)):
        assert sym in names and sym + '(' in header and len(names[sym][2]) == nargs, sym
    assert lib.ABI_VERSION == 27 and '#define HR_ABI_VERSION 27' in header
    assert (lib.HR_JPEG_444, lib.HR_JPEG_422, lib.HR_JPEG_420) == (0, 1, 2)
    for name, value in (('HR_JPEG_444', 0), ('HR_JPEG_422', 1), ('HR_JPEG_420', 2)):
        assert f'#define {name} {value}\n' in header
    assert jpeg.SUBSAMPLINGS == {'4:4:4': 0, '4:2:2': 1, '4:2:0': 2}
    for attr in ('JpegEncoder', 'save_jpeg', 'encode_host', 'bound', 'build_host'):
        assert hasattr(jpeg, attr), attr


# ---- the stand-alone sanitizer run --------------------------------------------------------------------------------------------------
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan']


def test_standalone_sanitizer_run(tmp_path):
    """hr_jpeg_encode_host.cpp's own main encodes 520 generated images -- every mode, four qualities, bytes and floats with NaNs, with
    and without restart markers -- from heap blocks of exactly the image's size into heap blocks of exactly the bound under
    AddressSanitizer and UndefinedBehaviorSanitizer: no report, every file starts with SOI, ends with EOI, is the same twice, and a
    capacity one below the bound is refused.  A program of its own with the runtimes linked in statically; nothing is loaded into Python.
    A compiler that cannot link the runtimes into a one-line program skips."""
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    r = subprocess.run(['g++', *SANITIZE, '-o', str(tmp_path / 'probe'), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip('the compiler here cannot link the sanitizer runtimes: ' + (r.stderr.strip().splitlines() or ['?'])[-1])
    exe = str(tmp_path / 'hr_jpeg_encode_standalone')
    r = subprocess.run(['g++', '-O1', '-g', *SANITIZE, '-o', exe, E.SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, '1'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == '520 images, 0 bad' and 'runtime error' not in r.stderr and 'Sanitizer' not in r.stderr, r.stdout + r.stderr
