"""CPU: the host build of hyperreel_amd/csrc/hr_png.h -- the functions the kernels of png_kernel.hip are made of -- against zlib, PIL and
numpy restatements of its rules (tests/png_common.py).  tests/test_gpu_png.py then demands the device's bytes equal this encoder's."""
import ctypes as C
import heapq
import io
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import png_common as P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, '..')


# ---- checksums ------------------------------------------------------------------------------------------------------------------------
def _pieces(rng, total, cuts):
    """a random buffer of `total` bytes cut at `cuts` random places: empty pieces, 1-byte pieces and one beyond 5552 bytes included"""
    buf = rng.integers(0, 256, total, dtype=np.uint8)
    at = sorted({0, total, min(1, total), min(2, total), 7000 if total > 14000 else total, *rng.integers(0, total + 1, cuts).tolist()})
    edges = [0, 0] + at[1:]          # an empty piece first
    return buf, [(edges[i], edges[i + 1]) for i in range(len(edges) - 1)]


@pytest.mark.parametrize('seed,total', [(0, 0), (1, 1), (2, 300), (3, 20000), (4, 70001)])
def test_crc32_partials_combine(seed, total):
    lib = P.host_lib()
    buf, pieces = _pieces(np.random.default_rng(seed), total, 6)
    assert any(b - a == 0 for a, b in pieces)
    if total >= 20000:
        assert any(b - a > 5552 for a, b in pieces) and any(b - a == 1 for a, b in pieces)
    acc = 0
    for a, b in pieces:          # crc0(A || B) = shift(crc0(A), |B|) ^ crc0(B)
        part = buf[a:b].copy()
        acc = lib.hp_crc_shift(acc, b - a) ^ lib.hp_crc0(part.ctypes.data_as(C.c_void_p), b - a)
    assert lib.hp_crc_final(acc, total) == zlib.crc32(buf.tobytes())
    # ... and as the lanes merge them: every piece shifted by the bytes after it, in any order
    acc2 = 0
    for a, b in reversed(pieces):
        part = buf[a:b].copy()
        acc2 ^= lib.hp_crc_shift(lib.hp_crc0(part.ctypes.data_as(C.c_void_p), b - a), total - b)
    assert acc2 == acc


@pytest.mark.parametrize('seed,total', [(0, 0), (1, 1), (2, 300), (3, 20000), (4, 70001)])
def test_adler32_partials_combine(seed, total):
    lib = P.host_lib()
    buf, pieces = _pieces(np.random.default_rng(100 + seed), total, 6)
    if total >= 20000:
        buf[:] = 255          # the largest sums: the deferred modulo's worst case
    a_acc, b_acc = C.c_uint32(0), C.c_uint32(0)
    for lo, hi in pieces:
        part = buf[lo:hi].copy()
        a, b = C.c_uint32(), C.c_uint32()
        lib.hp_adler_part(part.ctypes.data_as(C.c_void_p), hi - lo, C.byref(a), C.byref(b))
        lib.hp_adler_combine(a_acc.value, b_acc.value, a.value, b.value, hi - lo, C.byref(a_acc), C.byref(b_acc))
    assert lib.hp_adler_final(a_acc.value, b_acc.value, total) == zlib.adler32(buf.tobytes())


# ---- code lengths ---------------------------------------------------------------------------------------------------------------------
def _huffman_cost_and_depth(counts):
    """unrestricted Huffman: (total cost, greatest depth)"""
    heap = [(int(c), i, 0) for i, c in enumerate(counts) if c]
    if len(heap) == 1:
        return heap[0][0], 1
    heapq.heapify(heap)
    cost, tick = 0, len(counts)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], tick, max(a[2], b[2]) + 1))
        tick += 1
    return cost, heap[0][2]


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


_one_literal = np.zeros(286, np.uint32)
_one_literal[[65, 256]] = [1, 1]
HISTOGRAMS = {
    'fibonacci30': (np.array(_fib(30) + [0] * 256, np.uint32), 15),             # unrestricted depth 29
    'all286_once': (np.ones(286, np.uint32), 15),
    'eob_and_one_literal': (_one_literal, 15),
    'geometric19': (np.array([3 ** i for i in range(19)], np.uint32), 7),       # unrestricted depth 18
    'flat19': (np.full(19, 5, np.uint32), 7),
    'typical': (np.random.default_rng(5).integers(0, 400, 286).astype(np.uint32), 15),
}


@pytest.mark.parametrize('name', list(HISTOGRAMS))
def test_code_lengths(name):
    counts, limit = HISTOGRAMS[name]
    lens = np.zeros(len(counts), np.uint8)
    P.host_lib().hp_code_lengths(counts.ctypes.data_as(C.c_void_p), len(counts), limit, lens.ctypes.data_as(C.c_void_p))
    used = counts > 0
    assert (lens[~used] == 0).all()
    assert (lens[used] >= 1).all() and lens.max() <= limit
    if used.sum() >= 2:
        assert sum(1 << (limit - int(l)) for l in lens[used]) == 1 << limit, 'Kraft sum is not exactly 1'
    cost = int((counts.astype(np.int64) * lens).sum())
    best, depth = _huffman_cost_and_depth(counts)
    if name in ('fibonacci30', 'geometric19'):
        assert depth > limit, 'the histogram was meant to need the limit'
    if depth <= limit:
        assert cost == best
    else:
        assert cost >= best
    # rarer symbols never get shorter codes; equal counts are ordered by index
    order = sorted(np.flatnonzero(used), key=lambda i: (counts[i], i))
    assert all(lens[order[i]] >= lens[order[i + 1]] for i in range(len(order) - 1))


# ---- whole files ----------------------------------------------------------------------------------------------------------------------
MODES = {1: 'L', 3: 'RGB', 4: 'RGBA'}
FILE_CASES = [(c, w, h, content) for c in P.CHANNELS for (w, h) in P.shapes(c) for content in P.CONTENTS]


@pytest.mark.parametrize('c,w,h,content', FILE_CASES, ids=[f'c{c}_w{w}h{h}_{k}' for c, w, h, k in FILE_CASES])
def test_whole_file(c, w, h, content):
    im = P.image(content, w, h, c)
    data, filt, tok, rows = P.encode_host(im, c, details=True)
    px, mode = P.decode(data)
    assert mode == MODES[c] and px.shape == (h, w, c)
    assert np.array_equal(px, im)
    kinds = [t for t, _ in P.chunks(data)]          # (every CRC is checked in there)
    assert kinds == ['IHDR'.encode()] + [b'IDAT'] * P.plan(w, h, c)['n_strips'] + [b'IEND']
    assert zlib.decompress(P.idat(data)) == filt.tobytes()
    assert np.array_equal(filt, P.np_filters(im)[rows, np.arange(h)])
    assert len(data) <= P.bound(w, h, c)
    raw = h * (1 + w * c)
    if content == 'noise':
        assert len(data) > raw, 'noise is stored: nothing shorter exists'
    if (c, w, h, content) in CONSTANT_BELOW_ONE_PERCENT:
        assert len(data) < raw / 100


# Where a constant image's file must be below 1 % of the raw bytes.  The file's frame (signature, IHDR, IEND, zlib header, Adler-32) is 63
# bytes and a strip's (chunk, marker, a table of a handful of symbols) about 45, so a tiny image cannot be; the strip-edge shapes and
# the wide row (30 KB and more) can wherever the run rule gives long matches:
#   black: every filter costs 0, None wins and the filter bytes are zeros too, so a strip is one run -- 258 bytes a token of a few bits;
#   white: row 0 is Sub (ff .. ff 00 ...), every other row Up (02 00 00 ...).  The filter byte cuts the run, so a row costs two literals
#          and one match per 258 bytes, about 3 bytes: below 1 % of rows of 901 and 1201 bytes, not of the grey rows of 301.
CONSTANT_BELOW_ONE_PERCENT = {(c, w, h, content) for c in P.CHANNELS for (w, h) in P.shapes(c)[5:] for content in ('white', 'black')
                              if c > 1 or content == 'black'}


@pytest.mark.parametrize('mode', [0, 1, 2, 3, 4])
def test_fixed_filters_round_trip(mode):
    im = P.image('disc', 61, 47, 3)
    data, filt, tok, rows = P.encode_host(im, 3, mode, details=True)
    assert (rows == mode).all()
    assert np.array_equal(filt, P.np_filters(im)[mode])
    assert np.array_equal(P.decode(data)[0], im)


def test_product_encode_host_is_the_same_encoder():
    from hyperreel_amd import png
    im = P.image('disc', 61, 47, 3)
    assert png.encode_host(im) == P.encode_host(im, 3)
    assert png.encode_host(im, filter='paeth') == P.encode_host(im, 3, 4)
    assert png.encode_host(im[..., 0]) == P.encode_host(im[..., :1], 1)
    for bad in (np.zeros((3, 4, 2), np.uint8), np.zeros((0, 4, 3), np.uint8), np.zeros((3, 4, 3), np.float64), np.zeros(5, np.uint8)):
        with pytest.raises(ValueError):
            png.encode_host(bad)
    # a row beyond 2^27 bytes, an image beyond 2^30: refused before anything is read (a strip's bit counts are 32-bit)
    lib = png.host_lib()
    assert lib.hr_png_host_bound(1 << 27, 1, 1) == -1 and lib.hr_png_host_bound(1 << 20, 1 << 10, 3) == -1
    assert lib.hr_png_host_bound((1 << 27) - 1, 1, 1) > 1 << 27


# ---- the run rule ---------------------------------------------------------------------------------------------------------------------
def _run_image():
    """one strip of a grey image under filter 0 whose bytes (filter bytes included) hold runs of exactly 2, 3, 4, 258, 259, 260, 261, 262
    and 517 after a literal, then a run that reaches the strip's last byte -- and goes on into the next strip"""
    w = 1500
    rps = P.plan(w, 1, 1)['rows_per_strip']
    assert rps >= 3
    values, v = [], 10
    for follow in (2, 3, 4, 258, 259, 260, 261, 262, 517):
        values += [v] * (1 + follow)
        v += 1
    flat = np.empty(w * (rps + 1), np.uint8)
    flat[:] = 200                                   # the closing run: to the strip's end and across it
    body = np.array(values, np.uint8)
    rows = flat.reshape(rps + 1, w)
    # lay the runs inside rows so that no filter byte (0) interrupts one: each run gets a row of its own where it fits
    at_row, x = 0, 0
    for follow in (2, 3, 4, 258, 259, 260, 261, 262, 517):
        run = body[:1 + follow]
        body = body[1 + follow:]
        if x + len(run) > w - 1:
            at_row, x = at_row + 1, 0
        rows[at_row, x:x + len(run)] = run
        x += len(run)
    assert at_row < rps - 1
    return rows.reshape(rps + 1, w, 1), rps


def test_run_rule_tokens():
    im, rps = _run_image()
    data, filt, tok, rows = P.encode_host(im, 1, 0, details=True)
    row_bytes = im.shape[1] + 1
    strip = filt.reshape(-1)[:rps * row_bytes]
    expect = P.np_tokens(strip)
    assert np.array_equal(tok[:rps * row_bytes], expect)
    # the strip holds every run length asked for (the literal at its head counted)
    edges = np.flatnonzero(np.diff(strip.astype(np.int32)) != 0)
    run_lengths = set(np.diff(np.concatenate([[-1], edges, [len(strip) - 1]])).tolist())
    assert {1 + f for f in (2, 3, 4, 258, 259, 260, 261, 262, 517)} <= run_lengths
    assert strip[-1] == 200 and filt.reshape(-1)[rps * row_bytes + 1] == 200          # the closing run reaches the end; its value goes on
    # the run that reaches the strip's end stops there: the next strip starts with literals
    assert tok[rps * row_bytes - 1] == P.TOK_COVERED or tok[rps * row_bytes - 1] < P.TOK_MATCH
    assert np.array_equal(tok[rps * row_bytes:], P.np_tokens(filt.reshape(-1)[rps * row_bytes:]))
    assert tok[rps * row_bytes] < P.TOK_MATCH and tok[rps * row_bytes + 1] < P.TOK_MATCH
    assert np.array_equal(P.decode(data)[0], im)


def test_run_rule_black_image_joins_filter_bytes():
    w, c = 300, 1
    rps = P.plan(w, 1, c)['rows_per_strip']
    im = P.image('black', w, rps + 2, c)
    data, filt, tok, rows = P.encode_host(im, c, 0, details=True)
    n = rps * (w + 1)
    assert not filt.any()
    assert np.array_equal(tok[:n], P.np_tokens(np.zeros(n, np.uint8)))
    assert tok[0] == 0 and tok[1] == P.TOK_MATCH + 255 and (tok[:n] < P.TOK_MATCH).sum() <= 3
    assert np.array_equal(P.decode(data)[0], im)


@pytest.mark.parametrize('follow', [0, 1, 2, 3, 4, 257, 258, 259, 260, 261, 262, 516, 517, 518, 519, 1000])
def test_token_of_every_position(follow):
    lib = P.host_lib()
    got = np.array([lib.hp_token(77, k, follow) for k in range(follow + 1)], np.uint16)
    assert np.array_equal(got, P.np_tokens(np.full(follow + 1, 77, np.uint8)))


@pytest.mark.parametrize('slices', [1, 2, 7, 256])
def test_tokens_sliced_as_the_kernel_slices_them(slices):
    """the kernel cuts a strip into one slice per thread and joins runs across slices: any cut gives the whole strip's tokens"""
    rng = np.random.default_rng(slices)
    parts = []
    for _ in range(60):
        parts.append(np.full(int(rng.choice([1, 2, 3, 4, 5, 40, 257, 258, 259, 260, 300, 517, 900])), rng.integers(0, 4), np.uint8))
    b = np.concatenate(parts + [rng.integers(0, 3, 500, dtype=np.uint8), np.zeros(3000, np.uint8)])
    for data in (b, b[:100], np.zeros(5000, np.uint8), b[:1]):
        data = np.ascontiguousarray(data)
        tok = np.zeros(len(data), np.uint16)
        P.host_lib().hp_tokens_sliced(data.ctypes.data_as(C.c_void_p), len(data), slices, tok.ctypes.data_as(C.c_void_p))
        assert np.array_equal(tok, P.np_tokens(data))


# ---- filter choice --------------------------------------------------------------------------------------------------------------------
def _strict_cases():
    """per filter a two-row grey image in which that filter is the strict minimum on row 1"""
    rng = np.random.default_rng(3)
    w = 64
    noise = rng.integers(0, 256, w, dtype=np.uint8)
    small = np.where(np.arange(w) % 2 == 0, 2, 254).astype(np.uint8)          # +2, -2, +2 ...: cheap as it stands, twice as dear as a difference
    ramp = (np.arange(w) * 5 % 256).astype(np.uint8)
    cases = {
        0: np.stack([noise, small]),                                 # small values under noise: None
        1: np.stack([noise, np.full(w, 90, np.uint8)]),              # a constant under noise: Sub
        # the row above plus 0, 2, 0, 2 ... over a slow ripple: Up pays the 2s; Paeth takes the left pixel after every 2 and pays more
        2: np.stack([100 + np.arange(w) % 3, 100 + np.arange(w) % 3 + 2 * (np.arange(w) % 2)]).astype(np.uint8),
    }
    # Average: the row that the average predictor reproduces exactly, under a steep ramp
    top = (np.arange(w) * 37 % 256).astype(np.uint8)
    row = np.zeros(w, np.int64)
    for x in range(w):
        row[x] = (((row[x - 1] if x else 0) + int(top[x])) >> 1)
    cases[3] = np.stack([top, row.astype(np.uint8)])
    # Paeth: its own prediction under noise, plus 40 at every fourth byte: after each of those the left and the upper-left pixel differ,
    # so the predictor moves between left, up and upper left where Up and Sub keep to one of them
    top2 = rng.integers(0, 256, w, dtype=np.uint8)
    row2 = np.zeros(w, np.int64)
    for x in range(w):
        a, b, cc = (row2[x - 1] if x else 0), int(top2[x]), (int(top2[x - 1]) if x else 0)
        p = a + b - cc
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - cc)
        row2[x] = ((a if (pa <= pb and pa <= pc) else (b if pb <= pc else cc)) + (40 if x % 4 == 1 else 0)) & 255
    cases[4] = np.stack([top2, row2.astype(np.uint8)])
    return {f: im[..., None] for f, im in cases.items()}


def test_filter_strict_minimum_per_filter():
    for f, im in _strict_cases().items():
        filters = P.np_filters(im)
        v = filters[:, 1, 1:].astype(np.int64)
        cost = np.minimum(v, 256 - v).sum(-1)
        assert (cost[f] < np.delete(cost, f)).all(), f'filter {f} is not the strict minimum of the test image: {cost}'
        rows = P.encode_host(im, 1, details=True)[3]
        assert rows[1] == f


def test_filter_choice_matches_numpy():
    images = list(_strict_cases().values()) + [P.image(content, 61, 47, c) for c in P.CHANNELS for content in P.CONTENTS]
    for im in images:
        rows = P.encode_host(im, im.shape[2], details=True)[3]
        assert np.array_equal(rows, P.np_choose(P.np_filters(im)))


def test_filter_tie_keeps_the_lower_index():
    im = np.zeros((3, 9, 3), np.uint8)              # all five filters cost 0 on a black image: None
    rows = P.encode_host(im, 3, details=True)[3]
    assert (rows == 0).all()
    # first row: no row above, so Up == None and Paeth == Sub exactly; on a ramp Sub (1) beats None and ties with Paeth (4)
    im = (np.arange(40, dtype=np.uint8) * 2 + 100)[None, :, None]
    filters = P.np_filters(im)
    v = filters[:, 0, 1:].astype(np.int64)
    cost = np.minimum(v, 256 - v).sum(-1)
    assert cost[1] == cost[4] and cost[1] < cost[0] and cost[1] < cost[3] and cost[0] == cost[2]
    assert P.encode_host(im, 1, details=True)[3][0] == 1


# ---- float input ----------------------------------------------------------------------------------------------------------------------
def _float_values():
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    edge = np.concatenate([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2))]).astype(np.float32)
    special = np.array([-1.0, -0.0, 0.0, 1.0, 1.5, 1e30, -1e30, np.inf, -np.inf, np.nan, 0.5, 0.999999, 1e-8], np.float32)
    return np.concatenate([special, edge])


def test_float_input_is_to8b():
    x = _float_values()
    x = np.concatenate([x, np.zeros((-len(x)) % 3, np.float32)])
    got = P.to8b_host(x)
    finite = np.isfinite(x)
    assert np.array_equal(got[finite], P.to8b_reference(x[finite]))
    assert got[np.isnan(x)].tolist() == [0] and got[np.isposinf(x)].tolist() == [255] and got[np.isneginf(x)].tolist() == [0]
    # ... and the encoder reads a float frame through exactly that function
    frame = x.reshape(1, -1, 3)
    data = P.encode_host(frame, 3)
    assert np.array_equal(P.decode(data)[0], got.reshape(frame.shape))
    assert data == P.encode_host(got.reshape(frame.shape), 3)


# ---- size -----------------------------------------------------------------------------------------------------------------------------
def test_size_against_zlib_rle_on_the_same_filtered_bytes():
    """white background around a textured disc, 800 x 800 RGB: per-strip tables over literals and distance-1 runs against zlib's Z_RLE
    with whole-stream tables over the same filtered bytes.  The bar is the comparator x 1.03: the allowance covers the per-strip table,
    the 5-byte alignment marker and the 12-byte chunk overhead (about 120 B a strip, 0.4 % at 32 KB strips)."""
    im = P.image('disc', 800, 800, 3)
    data, filt, tok, rows = P.encode_host(im, 3, details=True)
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
    ref = len(co.compress(filt.tobytes()) + co.flush())
    from PIL import Image
    sizes = {}
    for level in (1, 6):
        b = io.BytesIO()
        Image.fromarray(im).save(b, 'PNG', compress_level=level)
        sizes[level] = len(b.getvalue())
    print(f'file {len(data)} B, Z_RLE stream {ref} B, ratio {len(data) / ref:.4f}; PIL level 1 {sizes[1]} B, level 6 {sizes[6]} B')
    assert len(data) <= ref * 1.03
    assert np.array_equal(P.decode(data)[0], im)


# ---- the stand-alone sanitizer run ----------------------------------------------------------------------------------------------------
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan']


def test_standalone_sanitizer_run(tmp_path):
    """hr_png_host.cpp's own main encodes the shapes into heap blocks of exactly hr_png_bound bytes under AddressSanitizer and
    UndefinedBehaviorSanitizer: a program of its own with the runtimes linked in statically, started in the environment the suite
    has; nothing is loaded into Python.  A compiler that cannot link the runtimes into a one-line program skips the test."""
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    r = subprocess.run(['g++', *SANITIZE, '-o', str(tmp_path / 'probe'), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip('the compiler here cannot link the sanitizer runtimes: ' + (r.stderr.strip().splitlines() or ['?'])[-1])
    exe = str(tmp_path / 'hr_png_standalone')
    r = subprocess.run(['g++', '-O1', '-g', *SANITIZE, '-ffp-contract=off', '-DHR_PNG_STANDALONE', '-o', exe, P.SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r'\d+ images, 0 bad', r.stdout)


# ---- bindings -------------------------------------------------------------------------------------------------------------------------
def test_bindings_and_abi_version():
    from hyperreel_amd import lib
    names = {s[0] for s in lib.SYMBOLS}
    header = open(os.path.join(ROOT, 'include', 'hyperreel_hip.h')).read()
    for name in ('hr_png_bound', 'hr_png_encoder_create', 'hr_png_encode', 'hr_png_encoder_destroy'):
        assert name in names
        assert re.search(rf'\b{name}\(', header)
        assert hasattr(lib.load(), name)
    assert '#define HR_ABI_VERSION 27' in header and lib.ABI_VERSION == 27
    assert (lib.HR_PNG_U8, lib.HR_PNG_F32_TO8B, lib.HR_PNG_FILTER_ADAPTIVE) == (0, 1, 5)
    assert '#define HR_PNG_FILTER_ADAPTIVE 5' in header
