"""Shared by tests/test_png_decode_host.py and tests/test_gpu_png_decode.py: PNG files built by hand from the standard library's zlib and
numpy -- the oracle is the array that was compressed, no imaging library enters --, PIL's files with PIL's pixels from
tests/golden/png_decode (tools/make_png_decode_golden.py), the project's own files (png.encode_host), PIL's conversions restated in
numpy, and damaged files."""
import glob
import os
import struct
import zlib

import numpy as np

import png_common as P

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'png_decode')
SRC = os.path.join(HERE, 'host_math', 'hr_png_decode_host.cpp')
MODES = {'L': 1, 'RGB': 3, 'RGBA': 4}
COLOR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}
SIGNATURE = b'\x89PNG\r\n\x1a\n'
IDAT_CUTS = (1, 2, 7, 1, 13)
STRATEGIES = {'default': zlib.Z_DEFAULT_STRATEGY, 'fixed': zlib.Z_FIXED, 'huffman': zlib.Z_HUFFMAN_ONLY, 'rle': zlib.Z_RLE}
(OK, BAD_SIGNATURE, BAD_CHUNK, BAD_CRC, UNSUPPORTED, SIZE_MISMATCH, BAD_ZLIB_HEADER, BAD_BLOCK, BAD_CODE, BAD_DISTANCE, TRUNCATED, TOO_LONG,
 TOO_SHORT, BAD_ADLER, BAD_FILTER, BAD_OFFSETS) = range(16)

_cache = {}


# ---- files by hand ----------------------------------------------------------------------------------------------------------------------
def chunk(typ, payload):
    return struct.pack('>I', len(payload)) + typ + payload + struct.pack('>I', zlib.crc32(typ + payload))


def ihdr(w, h, channels, depth=8, color_type=None, interlace=0):
    return chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth, COLOR_TYPE[channels] if color_type is None else color_type, 0, 0, interlace))


def filtered_bytes(im, filters='cycle'):
    """(h, 1 + w c) uint8: row y of an (h, w, c) image under PNG filter y % 5 ('cycle') or the one given"""
    all5 = P.np_filters(im)
    rows = np.arange(im.shape[0]) % 5 if filters == 'cycle' else np.full(im.shape[0], filters)
    return np.ascontiguousarray(all5[rows, np.arange(im.shape[0])])


def deflate(raw, level=6, strategy='default'):
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, STRATEGIES[strategy])
    return co.compress(bytes(raw)) + co.flush()


def assemble(head, stream, cuts=None, extra=()):
    """a file from its IHDR chunk and zlib stream: the stream cut into IDAT chunks of `cuts` bytes and then the rest; `extra`: ancillary
    chunks between IHDR and the first IDAT"""
    parts, at = [], 0
    for n in (cuts or ()):
        if at + n < len(stream):
            parts.append(stream[at:at + n])
            at += n
    parts.append(stream[at:])
    return SIGNATURE + head + b''.join(extra) + b''.join(chunk(b'IDAT', p) for p in parts) + chunk(b'IEND', b'')


def build_png(im, level=6, strategy='default', filters='cycle', cuts=None, extra=()):
    h, w, c = im.shape
    return assemble(ihdr(w, h, c), deflate(filtered_bytes(im, filters).tobytes(), level, strategy), cuts, extra)


class Bits:
    """a DEFLATE stream written bit by bit"""

    def __init__(self):
        self.bits = []

    def put(self, value, n):             # a field: LSB first
        self.bits += [(value >> i) & 1 for i in range(n)]

    def code(self, value, n):            # a Huffman code: MSB first
        self.bits += [(value >> (n - 1 - i)) & 1 for i in range(n)]

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def far_match_raw(dist):
    """40 rows of 1024 filtered bytes (filter 0) whose last 8192 bytes repeat what lies `dist` bytes before them"""
    rng = np.random.default_rng(dist)
    raw = rng.integers(0, 256, 32768 + 8192, dtype=np.uint8)
    raw[0:32768:1024] = 0                                  # the filter bytes
    for k in range(8):                                    # ... and the bytes that the matches copy onto filter bytes
        raw[32768 + 1024 * k - dist] = 0
    for i in range(32768, 32768 + 8192):
        raw[i] = raw[i - dist]
    assert not raw[0::1024].any()
    return raw


def far_match_file(dist=32768):
    """zlib's own compressor never looks 32768 bytes back (its reach ends 262 bytes short of the window), so this stream is written by
    hand: the first 32 rows in one stored block, then a fixed-Huffman block of matches of length 258 (and one of 194) at distance
    `dist` -- distance symbol 29 with its 13 extra bits -- for the last 8 rows.  The output passes 32768 bytes, so the window wraps
    under the matches; at 32767 a match's source slots in the window are, but for one, the slots the same match writes.
    Returns (file, the (40, 341, 3) pixels)."""
    raw = far_match_raw(dist).tobytes()
    w = Bits()
    w.put(1, 1); w.put(1, 2)                              # final, fixed codes
    for n in [258] * 31 + [194]:
        if n == 258:
            w.code(0b11000000 + 285 - 280, 8)             # length symbol 285, no extra bits
        else:
            w.code(0b11000000 + 282 - 280, 8); w.put(194 - 163, 5)
        w.code(29, 5); w.put(dist - 24577, 13)
    w.code(0, 7)                                          # end of block
    stream = b'\x78\x01\x00' + struct.pack('<HH', 32768, 32768 ^ 0xFFFF) + raw[:32768] + w.bytes() + struct.pack('>I', zlib.adler32(raw))
    assert zlib.decompress(stream) == raw
    pixels = np.frombuffer(raw, np.uint8).reshape(40, 1024)[:, 1:].reshape(40, 341, 3)
    return assemble(ihdr(341, 40, 3), stream), np.ascontiguousarray(pixels)


def hand_files():
    """[(name, file bytes, (h, w, c) pixels)]: every block type, IDAT boundaries anywhere, the window's edge, the longest run"""
    if 'hand' in _cache:
        return _cache['hand']
    out = []
    rng = np.random.default_rng(5)
    disc = {c: P.image('disc', 61, 47, c) for c in (1, 3, 4)}
    la = np.ascontiguousarray(np.stack([P.image('disc', 61, 47, 1)[..., 0], P.image('noise', 61, 47, 1)[..., 0]], -1))
    for level in (0, 1, 9):
        for strategy in STRATEGIES:
            for c, im in list(disc.items()) + [(2, la)]:
                if c in (1, 2) and strategy in ('huffman', 'rle') and level != 9:
                    continue
                out.append((f'l{level}_{strategy}_c{c}', build_png(im, level, strategy), im))
    small = rng.integers(0, 256, (9, 17, 3), dtype=np.uint8)
    for strategy in STRATEGIES:
        for level in (0, 9):
            out.append((f'cuts_l{level}_{strategy}', build_png(small, level, strategy, cuts=IDAT_CUTS), small))
    out.append(('one_byte_idat', build_png(P.image('noise', 20, 12, 3), 9, cuts=(1,) * 4000), P.image('noise', 20, 12, 3)))
    text = [chunk(b'tEXt', b'Comment\x00hand built'), chunk(b'gAMA', struct.pack('>I', 45455))]
    out.append(('ancillary', build_png(small, 6, extra=text), small))
    stream = deflate(filtered_bytes(small).tobytes())
    out.append(('empty_idat', SIGNATURE + ihdr(17, 9, 3) + b''.join(chunk(b'IDAT', p) for p in (b'', stream[:5], b'', stream[5:])) + chunk(b'IEND', b''),
                small))
    out.append(('far_match',) + far_match_file(32768))
    out.append(('far_match_32767',) + far_match_file(32767))
    flat = np.full((40, 300, 3), 77, np.uint8)
    out.append(('flat_run', build_png(flat, 9, filters=0), flat))
    for f in range(5):
        out.append((f'filter{f}_rgba', build_png(P.image('disc', 61, 47, 4), 6, filters=f), P.image('disc', 61, 47, 4)))
        out.append((f'filter{f}_grey_1px_wide', build_png(P.image('noise', 1, 7, 1), 6, filters=f), P.image('noise', 1, 7, 1)))
    _cache['hand'] = out
    return out


def own_files():
    """[(name, file bytes, pixels)]: files of the project's own encoder (png.encode_host) at png_common.shapes"""
    if 'own' not in _cache:
        from hyperreel_amd import png
        out = []
        for c in P.CHANNELS:
            for i, (w, h) in enumerate(P.shapes(c)):
                im = P.image(P.CONTENTS[i % len(P.CONTENTS)], w, h, c)
                out.append((f'own_c{c}_w{w}_h{h}', png.encode_host(im, c), im))
        _cache['own'] = out
    return _cache['own']


def golden_files():
    """[(name, file bytes, {'L' | 'RGB' | 'RGBA': PIL's pixels (h, w, c)})] from tests/golden/png_decode"""
    if 'golden' not in _cache:
        out = []
        for path in sorted(glob.glob(os.path.join(GOLDEN, '*.npz'))):
            z = np.load(path)
            stem = os.path.basename(path)[:-4]
            files, off = z['files'], z['offsets']
            pixels = {m: z[m] for m in MODES}
            for i, name in enumerate(z['names']):
                out.append((f'{stem}_{name}', files[off[i]:off[i + 1]].tobytes(), {m: pixels[m][i] for m in MODES}))
        _cache['golden'] = out
    return _cache['golden']


def convert(im, mode):
    """PIL's convert of an (h, w, c) image with c = 1 (L), 2 (LA), 3 (RGB) or 4 (RGBA), restated: grey replicates, an absent alpha is 255,
    alpha is dropped without compositing, colour to L is ITU-R 601-2 in PIL's integers"""
    c = im.shape[-1]
    grey = c <= 2
    alpha = im[..., -1:] if c in (2, 4) else np.full(im.shape[:2] + (1,), 255, np.uint8)
    if mode == 'L':
        if grey:
            return np.ascontiguousarray(im[..., :1])
        v = im[..., :3].astype(np.uint32)
        return ((v[..., 0:1] * 19595 + v[..., 1:2] * 38470 + v[..., 2:3] * 7471 + 0x8000) >> 16).astype(np.uint8)
    rgb = np.repeat(im[..., :1], 3, -1) if grey else im[..., :3]
    return np.ascontiguousarray(rgb if mode == 'RGB' else np.concatenate([rgb, alpha], -1))


def all_cases():
    """[(name, file bytes, {mode: expected pixels})] of everything above"""
    if 'all' not in _cache:
        made = [(n, d, {m: convert(im, m) for m in MODES}) for n, d, im in hand_files() + own_files()]
        _cache['all'] = golden_files() + made
    return _cache['all']


def size_of(data):
    w, h = struct.unpack('>II', data[16:24])
    return w, h


# ---- damaged files ----------------------------------------------------------------------------------------------------------------------
def split(data):
    """(bytes before the first IDAT, [IDAT payloads], bytes after the last IDAT)"""
    at, first, last, payloads = 8, None, None, []
    while at < len(data):
        n, = struct.unpack('>I', data[at:at + 4])
        if data[at + 4:at + 8] == b'IDAT':
            first = at if first is None else first
            payloads.append(data[at + 8:at + 8 + n])
            last = at + 12 + n
        at += 12 + n
    return data[:first], payloads, data[last:]


def join(before, payloads, after):
    return before + b''.join(chunk(b'IDAT', p) for p in payloads) + after


def mutate_idat(data, rng, mend_adler=False):
    """one byte of the IDAT payloads changed, the chunks' CRCs recomputed: (file, the joined payload).  mend_adler: the byte lies in the
    deflate data, and when that still inflates to its end the Adler-32 behind it is made to fit, so that the damage reaches the pixels"""
    before, payloads, after = split(data)
    stream = bytearray(b''.join(payloads))
    i = int(rng.integers(2, len(stream) - 4)) if mend_adler else int(rng.integers(0, len(stream)))
    stream[i] ^= int(rng.integers(1, 256))
    if mend_adler:
        try:
            co = zlib.decompressobj(-15)
            raw = co.decompress(bytes(stream[2:-4]))
            if co.eof and not co.unused_data:
                stream[-4:] = struct.pack('>I', zlib.adler32(raw))
        except zlib.error:
            pass
    cut, out = 0, []
    for p in payloads:
        out.append(bytes(stream[cut:cut + len(p)]))
        cut += len(p)
    return join(before, out, after), bytes(stream)


def zlib_verdict(stream, w, h, c):
    """what zlib and numpy make of a damaged stream: the (h, w, c) pixels, or None when zlib.decompress fails, the length is not
    h (1 + w c) or a filter byte is above 4"""
    try:
        raw = zlib.decompress(stream)
    except zlib.error:
        return None
    if len(raw) != h * (1 + w * c):
        return None
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + w * c)
    if rows[:, 0].max() > 4:
        return None
    return np_unfilter(rows, c)


def np_unfilter(rows, c):
    """the pixels (h, w, c) of filtered rows (h, 1 + w c), in int arithmetic"""
    h, n = rows.shape[0], rows.shape[1] - 1
    out = np.zeros((h, n), np.int32)
    prev = np.zeros(n, np.int32)
    for y in range(h):
        f, x = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        cur = np.zeros(n, np.int32)
        if f == 0:
            cur = x
        elif f == 2:
            cur = (x + prev) & 255
        else:
            for i in range(n):
                a = cur[i - c] if i >= c else 0
                b = prev[i]
                cc = prev[i - c] if i >= c else 0
                if f == 1:
                    p = a
                elif f == 3:
                    p = (a + b) >> 1
                else:
                    q = a + b - cc
                    pa, pb, pc = abs(q - a), abs(q - b), abs(q - cc)
                    p = a if (pa <= pb and pa <= pc) else (b if pb <= pc else cc)
                cur[i] = (x[i] + p) & 255
        out[y] = cur
        prev = cur
    return out.astype(np.uint8).reshape(h, n // c, c)


def damaged_files():
    """{name: (file bytes, (w, h))} of one small good file damaged in named ways; (w, h) the size a decoder for the good file has"""
    if 'damaged' not in _cache:
        im = P.image('disc', 17, 9, 3)
        good = build_png(im, 9)
        before, payloads, after = split(good)
        flipped_crc = bytearray(good)
        flipped_crc[len(before) + 8 + len(payloads[0])] ^= 0x40
        adler = bytearray(payloads[0])
        adler[-1] ^= 1
        rows = filtered_bytes(im)
        rows[4, 0] = 7
        mid = len(before) + 8 + len(payloads[0]) // 2
        d = {
            'flipped_crc': bytes(flipped_crc),
            'flipped_adler': join(before, [bytes(adler)], after),
            'truncated_mid_idat': good[:mid],
            'filter_byte_7': assemble(ihdr(17, 9, 3), deflate(rows.tobytes())),
            'header_16_bit': assemble(ihdr(17, 9, 3, depth=16), deflate(bytes(9 * (1 + 17 * 6)))),
            'header_palette': assemble(ihdr(17, 9, 1, color_type=3), deflate(bytes(9 * 18)), extra=[chunk(b'PLTE', bytes(6))]),
            'header_interlaced': assemble(ihdr(17, 9, 3, interlace=1), payloads[0]),
            'other_size': build_png(P.image('disc', 16, 9, 3), 9),
            'bad_signature': b'\x89PNG\r\n\x1a\x0b' + good[8:],
            'no_idat': SIGNATURE + ihdr(17, 9, 3) + chunk(b'IEND', b''),
            'idat_apart': join(before, [payloads[0][:10]], chunk(b'tEXt', b'a\x00b') + chunk(b'IDAT', payloads[0][10:]) + after),
            'too_short': assemble(ihdr(17, 9, 3), deflate(filtered_bytes(im).tobytes()[:-1])),
            'too_long': assemble(ihdr(17, 9, 3), deflate(filtered_bytes(im).tobytes() + b'\x00')),
            'zlib_header': join(before, [b'\x78\x02' + payloads[0][2:]], after),
            'block_type_3': assemble(ihdr(17, 9, 3), b'\x78\x9c\x07' + bytes(8)),
            'stored_len': assemble(ihdr(17, 9, 3), b'\x78\x9c\x01\x05\x00\xfa\xfe' + bytes(9)),
            'distance_too_far': assemble(ihdr(17, 9, 3), b'\x78\x9c\x03\x02' + bytes(8)),
        }
        _cache['damaged'] = {'good': (good, im), 'files': d, 'size': (17, 9)}
    return _cache['damaged']


DAMAGED_STATUS = {
    'flipped_crc': BAD_CRC, 'flipped_adler': BAD_ADLER, 'truncated_mid_idat': TRUNCATED, 'filter_byte_7': BAD_FILTER,
    'header_16_bit': UNSUPPORTED, 'header_palette': UNSUPPORTED, 'header_interlaced': UNSUPPORTED, 'other_size': SIZE_MISMATCH,
    'bad_signature': BAD_SIGNATURE, 'no_idat': BAD_CHUNK, 'idat_apart': BAD_CHUNK, 'too_short': TOO_SHORT, 'too_long': TOO_LONG,
    'zlib_header': BAD_ZLIB_HEADER, 'block_type_3': BAD_BLOCK, 'stored_len': BAD_BLOCK, 'distance_too_far': BAD_DISTANCE,
}
