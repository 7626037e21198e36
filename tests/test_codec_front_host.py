"""The image codecs' shared host layer (hyperreel_amd/_codec.py, build.build_host_library): the packing of a batch of files, the decode
errors, the one g++ command line, and the geometry and checks of the encoders' frames, buffers and arrays.  No GPU, no built library."""
import os

import numpy as np
import pytest
import torch

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
    for built, name in ((png.build_host(), 'png_host'), (png.build_decode_host(), 'png_decode_host'), (jpeg.build_decode_host(), 'jpeg_decode_host'),
                        (jpeg.build_host(), 'jpeg_encode_host')):
        assert built == (os.path.join(build.LIB_DIR, f'libhr_{name}.so'), os.path.join(build.CSRC, name + '.cpp'), '-O2')


W, H = 61, 47
CPU = torch.device('cpu')


def test_frame_geometry():
    assert _codec.frame_geometry(torch.zeros(H, W, 3)) == (W, H, 3)
    assert _codec.frame_geometry(torch.zeros(H, W)) == (W, H, 1)
    assert _codec.frame_geometry(torch.zeros(H * W, 3), width=W, height=H) == (W, H, 3)
    assert _codec.frame_geometry(torch.zeros(H * W), width=W, height=H) == (W, H, 1)
    for flat, given in ((torch.zeros(H * W), {'height': H}), (torch.zeros(H * W), {}), (torch.zeros(H * W, 3), {'width': W})):
        with pytest.raises(ValueError, match=r'^a flat \(H \* W, C\) frame needs width and height$'):
            _codec.frame_geometry(flat, **given)


@pytest.mark.parametrize('dtype', [torch.float32, torch.uint8])
def test_check_frame_accepts(dtype):
    for shape, c in (((H, W, 3), 3), ((H * W, 3), 3), ((H, W), 1), ((H, W, 1), 1), ((H * W, 4), 4)):
        frame = torch.ones(shape, dtype=dtype)
        got = _codec.check_frame(frame, CPU, W, H, c)
        assert got is frame
    wide = (torch.arange(H * W * 4) % 251).to(dtype).reshape(H, W, 4)
    view = wide[..., :3]
    assert not view.is_contiguous()
    got = _codec.check_frame(view, CPU, W, H, 3)
    assert got.is_contiguous() and got.shape == (H, W, 3) and got.dtype == dtype and torch.equal(got, view)


@pytest.mark.parametrize('frame, text', [
    (torch.zeros(H, W, 3, dtype=torch.float64), 'frame must be float32 or uint8, got torch.float64'),
    (torch.zeros(H, W, 4), f'frame ({H}, {W}, 4) is not ({H}, {W}, 3) or ({H * W}, 3)'),
    (torch.zeros(H, W - 1, 3), f'frame ({H}, {W - 1}, 3) is not ({H}, {W}, 3) or ({H * W}, 3)'),
    (np.zeros((H, W, 3), np.float32), 'frame must be a tensor on cpu'),
    (torch.zeros(H, W, 3, device='meta'), 'frame must be a tensor on cpu')], ids=['float64', 'four_wide', 'count', 'array', 'device'])
def test_check_frame_refuses(frame, text):
    with pytest.raises(ValueError) as e:
        _codec.check_frame(frame, CPU, W, H, 3)
    assert str(e.value) == text


def test_check_out_and_length():
    bound = 1000
    exact = torch.empty(bound, dtype=torch.uint8)
    assert _codec.check_out(exact, CPU, bound) is exact
    text = 'out must be a contiguous uint8 tensor of at least 1000 bytes on cpu'
    for bad in (torch.empty(bound - 1, dtype=torch.uint8), torch.empty(bound, dtype=torch.int8), torch.empty(2 * bound, dtype=torch.uint8)[::2],
                torch.empty(bound, dtype=torch.uint8, device='meta')):
        with pytest.raises(ValueError) as e:
            _codec.check_out(bad, CPU, bound)
        assert str(e.value) == text
    one = torch.empty(1, dtype=torch.int64)
    assert _codec.check_length(one, CPU) is one
    for bad in (torch.empty(1, dtype=torch.int32), torch.empty(2, dtype=torch.int64), torch.empty(1, dtype=torch.int64, device='meta')):
        with pytest.raises(ValueError) as e:
            _codec.check_length(bad, CPU)
        assert str(e.value) == 'length must be an int64 tensor of one element on cpu'


def test_array_geometry():
    for dtype in (np.uint8, np.float32):
        a = np.zeros((H, W, 3), dtype)
        got, c, h, w = _codec.array_geometry(a)
        assert got is a and (c, h, w) == (3, H, W)
        assert _codec.array_geometry(np.zeros((H, W), dtype))[1:] == (1, H, W)
        assert _codec.array_geometry(np.zeros((H, W, 4), dtype), channels=3)[1:] == (3, H, W)
        assert _codec.array_geometry(np.zeros((H, W), dtype), channels=np.int64(4))[1:] == (4, H, W)
    sliced = np.zeros((H, W, 4), np.uint8)[..., :3]
    got = _codec.array_geometry(sliced)[0]
    assert got.flags['C_CONTIGUOUS'] and got.shape == (H, W, 3)
    for bad, said in ((np.zeros((H, W, 3), np.float64), f'float64 ({H}, {W}, 3)'), (np.zeros((1, H, W, 3), np.uint8), f'uint8 (1, {H}, {W}, 3)')):
        with pytest.raises(ValueError) as e:
            _codec.array_geometry(bad)
        assert str(e.value) == 'array must be uint8 or float32 of shape (H, W, C) or (H, W), got ' + said


@pytest.mark.parametrize('cls', [png.PngEncoder, jpeg.JpegEncoder])
def test_encoders_are_the_front_end(cls):
    """a format's encoder states its symbols, its constructor and its options; the frame, out and length checks and encode are the base's"""
    assert issubclass(cls, _codec.Encoder) and issubclass(_codec.Encoder, _codec.HandleOwner)
    assert not {'_frame', 'encode', 'close', '__del__'} & set(vars(cls))
    assert set(vars(cls)) - {'__module__', '__doc__', '__qualname__', '__firstlineno__', '__static_attributes__'} <= {
        'CREATE', 'ENCODE', 'DESTROY', 'BOUND', '__init__', 'encode_device'}
    assert 'encode_device' not in vars(jpeg.JpegEncoder)
    fmt = cls.__module__.rsplit('.', 1)[1]
    assert (cls.CREATE, cls.ENCODE, cls.DESTROY, cls.BOUND) == tuple(f'hr_{fmt}_{f}' for f in ('encoder_create', 'encode', 'encoder_destroy', 'bound'))
    assert 'no byte past it is written' in _codec.Encoder.encode_device.__doc__
