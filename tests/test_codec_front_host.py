"""The image codecs' shared host layer (hyperreel_amd/_codec.py, build.build_host_library): the packing of a batch of files, the decode
errors and the one g++ command line.  No GPU, no built library."""
import os

import numpy as np
import pytest

import helpers
from hyperreel_amd import _codec, build, jpeg, png


def _bounds(host, n):
    return host[:8 * (n + 1)].view(np.int64).tolist()


def test_pack_files_layout():
    host = _codec.pack_files([], 1, 100)
    assert host.dtype == np.uint8 and host.size == 16 and _bounds(host, 0) == [0]
    host = _codec.pack_files([b''], 1, 100)
    assert _bounds(host, 1) == [0, 0] and host[16:].size == 0
    host = _codec.pack_files([b'ab', b'', b'cde'], 5, 100)
    assert _bounds(host, 3) == [0, 2, 2, 5]
    assert host[48:].tobytes() == b'abcde'


def test_pack_files_refusals():
    with pytest.raises(ValueError, match='3 files for a decoder of max_images 2'):
        _codec.pack_files([b'a', b'b', b'c'], 2, 100)
    with pytest.raises(ValueError, match='5 bytes of files for a decoder of max_file_bytes 4: create it with a larger one'):
        _codec.pack_files([b'abc', b'de'], 2, 4)


@pytest.mark.parametrize('cls, status, text', [(png.PngDecodeError, 3, 'image 1: PNG status 3 (BAD_CRC)'),
                                               (jpeg.JpegDecodeError, 1, 'image 1: JPEG status 1 (NO_SOI)')])
def test_decode_errors(cls, status, text):
    e = cls(1, status)
    assert isinstance(e, ValueError) and isinstance(e, _codec.DecodeError)
    assert str(e) == text and (e.index, e.status, e.status_name) == (1, status, text[text.index('(') + 1:-1])
    assert cls(0, 99).status_name == '99' and str(cls(0, 99)).endswith('status 99 (99)')
    assert str(cls(1, status, what='x.png: image')) == 'x.png: ' + text
    assert png.MODES == {'L': 1, 'RGB': 3, 'RGBA': 4} and png.PngDecoder.Error is png.PngDecodeError and jpeg.JpegDecoder.Error is jpeg.JpegDecodeError


def test_one_builder(tmp_path, monkeypatch):
    """tests/helpers.build_host_lib is the package's builder: the same g++ command line but for -O1 where the product has -O2"""
    commands = []

    def run(cmd, check):
        assert check
        commands.append(list(cmd))
        open(cmd[cmd.index('-o') + 1], 'w').close()

    monkeypatch.setattr(build.subprocess, 'run', run)
    src, out = str(tmp_path / 'x.cpp'), str(tmp_path / 'sub' / 'libx.so')
    open(src, 'w').close()
    for builder in (build.build_host_library, helpers.build_host_lib):
        assert builder(out, src, [src]) == out and os.path.exists(out)
        assert builder(out, src, [src]) == out          # up to date: no second compile
        os.remove(out)
    product, test = commands
    assert product == ['g++', '-O2', '-ffp-contract=off', '-fno-fast-math', '-shared', '-fPIC', '-o', f'{out}.{os.getpid()}.tmp', src]
    assert test == [a if a != '-O2' else '-O1' for a in product]
    # the product's libraries go through the same function, at its default
    monkeypatch.setattr(build, 'build_host_library', lambda out, src, deps, opt='-O2': (out, src, opt))
    for built, name in ((png.build_host(), 'png_host'), (png.build_decode_host(), 'png_decode_host'), (jpeg.build_decode_host(), 'jpeg_decode_host')):
        assert built == (os.path.join(build.LIB_DIR, f'libhr_{name}.so'), os.path.join(build.CSRC, name + '.cpp'), '-O2')
