"""JPEG training images decoded on the device (csrc/hr_jpeg_decode.h, jpeg_decode_kernel.hip), png.py's sibling.

    images_u8 = load_jpeg(paths, 'RGB')         # (n, H, W, 3) uint8 on the device
    dec = JpegDecoder(4032, 3024, max_images=8)
    images_u8 = dec.decode(list_of_bytes, 'RGB')

replaces  np.stack([np.asarray(Image.open(p).convert('RGB')) for p in paths])  and its upload (datasets/llff.py, shiny.py: the cameras'
full-size JPEGs): the host reads the files' bytes and copies them to the device once; the markers, Huffman decoding -- parallel inside one
stream -- libjpeg's IDCT, chroma upsampling, colour conversion and PIL's convert run there, byte for byte as PIL 12.2 / libjpeg-turbo 3.1
give them.  Baseline and extended sequential Huffman files at 8 bits, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0, one scan, with or without
restart markers; probe() tells beforehand.  Progressive, arithmetic, CMYK and other samplings are refused by name: decode those with PIL.
"""
import collections
import ctypes as C
import os

import numpy as np

from . import lib as _lib
from .png import MODES, _build_host, _channels_of_mode

_HERE = os.path.dirname(os.path.abspath(__file__))
_DEC_SRC = os.path.join(_HERE, 'csrc', 'jpeg_decode_host.cpp')
_DEC_DEPS = [_DEC_SRC] + [os.path.join(_HERE, 'csrc', h) for h in ('hr_jpeg_decode.h', 'hr_png_decode.h', 'hr_png.h', 'hr_math.h')] + [
    os.path.join(_HERE, '..', 'include', 'hyperreel_hip.h')]
_DEC_LIB = os.path.join(_HERE, '_build', 'libhr_jpeg_decode_host.so')
_dec_host = None
STATUS_NAMES = _lib.JPEG_STATUS_NAMES


class JpegDecodeError(ValueError):
    """A file of a batch did not decode: .index is its place in the batch, .status the code, .status_name its name (STATUS_NAMES)"""

    def __init__(self, index, status, what='image'):
        self.index, self.status = int(index), int(status)
        self.status_name = STATUS_NAMES[self.status] if 0 <= self.status < len(STATUS_NAMES) else str(self.status)
        super().__init__(f'{what} {self.index}: JPEG status {self.status} ({self.status_name})')


JpegInfo = collections.namedtuple('JpegInfo', 'width height components h_samp v_samp restart_interval supported status')


def _info_tuple(info):
    return JpegInfo(info.width, info.height, info.components, info.h_samp, info.v_samp, info.restart_interval, bool(info.supported), info.status)


def probe(data):
    """hr_jpeg_probe: (width, height, components, h_samp, v_samp, restart_interval, supported, status) from the markers of a file's bytes up
    to its scan; `supported` says whether the decoder takes the file, `status` why not.  Raises for bytes without SOI or a frame header."""
    data = bytes(data)
    info = _lib.hr_jpeg_info()
    _lib.call('hr_jpeg_probe', data, len(data), C.byref(info))
    return _info_tuple(info)


class JpegDecoder:
    """Decodes batches of up to max_images JPEG files of width x height on the device.  max_file_bytes bounds the files' total size in one
    call of decode (None: the raw RGB size of max_images images, which no sensible file exceeds; a larger batch is refused).  subseq_bits:
    the length of the pieces a stream is cut into for the parallel Huffman decode, 0 for the default (1024), else a multiple of 32 from 128
    up; the pixels do not depend on it.  The decoder owns its device workspace: one decode at a time per decoder."""

    def __init__(self, width, height, max_images=1, max_file_bytes=None, subseq_bits=0, device=None):
        import torch
        self.width, self.height, self.max_images, self.subseq_bits = int(width), int(height), int(max_images), int(subseq_bits)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if max_file_bytes is None:
            max_file_bytes = self.max_images * (self.height * self.width * 3 + 4096)
        self.max_file_bytes = int(max_file_bytes)
        self._files = None
        self._h = C.c_void_p()
        _lib.call('hr_jpeg_decoder_create', self.width, self.height, self.max_images, self.max_file_bytes, self.subseq_bits, C.byref(self._h),
                  device=self.device)

    def close(self):
        if getattr(self, '_h', None):
            _lib.call('hr_jpeg_decoder_destroy', self._h)
            self._h = None
            self._files = None

    def __del__(self):
        try:
            self.close()
        except Exception:          # interpreter teardown: the library or this module's globals may already be gone
            pass

    def decode_device(self, files_dev, offsets_dev, n, mode='RGB', out=None, status=None, rounds=None):
        """Enqueues the decode on torch's current stream: files_dev a uint8 tensor of max_file_bytes bytes or more holding the files one
        after another, offsets_dev an int64 tensor of n + 1 bounds.  Returns (out (n, H, W, C) uint8, status (n,) int32): status 0 is a
        decoded image, anything else (STATUS_NAMES) an all-zero one.  rounds: an int32 tensor of n elements that gets the rounds the
        Huffman decode took per image.  No allocation when `out` and `status` are given, no synchronisation: capturable in a graph, with
        files_dev and offsets_dev refilled between replays."""
        import torch
        c, n = _channels_of_mode(mode), int(n)
        for name, t, dtype, count in (('files_dev', files_dev, torch.uint8, self.max_file_bytes), ('offsets_dev', offsets_dev, torch.int64, n + 1)):
            if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != dtype or not t.is_contiguous() or t.numel() < count:
                raise ValueError(f'{name} must be a contiguous {dtype} tensor of at least {count} elements on {self.device}')
        if out is None:
            out = torch.empty((n, self.height, self.width, c), dtype=torch.uint8, device=self.device)
        elif out.dtype != torch.uint8 or out.device != self.device or not out.is_contiguous() or out.numel() != n * self.height * self.width * c:
            raise ValueError(f'out must be a contiguous uint8 tensor ({n}, {self.height}, {self.width}, {c}) on {self.device}')
        if status is None:
            status = torch.empty(n, dtype=torch.int32, device=self.device)
        for name, t in (('status', status), ('rounds', rounds)):
            if t is not None and (t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous() or t.numel() != n):
                raise ValueError(f'{name} must be a contiguous int32 tensor of {n} elements on {self.device}')
        # an empty batch passes the library's own n_images == 0 path: nothing is launched
        _lib.call('hr_jpeg_decode', self._h, files_dev, offsets_dev, n, c, out, status, rounds, _lib.stream(self.device), device=self.device)
        return out, status

    def upload(self, files):
        """(files_dev, offsets_dev) of a list of files' bytes: one host-to-device copy of the concatenated files (the offsets, n + 1
        int64, ride in front of them in the same buffer).  The device buffer belongs to the decoder and is reused: the two tensors
        are valid until the next upload.  More than max_file_bytes in all is refused."""
        import torch
        if len(files) > self.max_images:
            raise ValueError(f'{len(files)} files for a decoder of max_images {self.max_images}')
        sizes = [len(f) for f in files]
        total = sum(sizes)
        if total > self.max_file_bytes:
            raise ValueError(f'{total} bytes of files for a decoder of max_file_bytes {self.max_file_bytes}: create it with a larger one')
        head = 8 * (self.max_images + 1)
        if self._files is None:
            self._files = torch.empty(head + max(self.max_file_bytes, 1), dtype=torch.uint8, device=self.device)
        used = 8 * (len(files) + 1)
        host = np.empty(head + total, np.uint8)
        host[:used].view(np.int64)[:] = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)])
        at = head
        for f in files:
            host[at:at + len(f)] = np.frombuffer(f, np.uint8)
            at += len(f)
        self._files[:host.size].copy_(torch.from_numpy(host))
        return self._files[head:], self._files[:used].view(torch.int64)

    def decode(self, files, mode='RGB'):
        """uint8 (n, H, W, C) on the device from a list of files' bytes: one host-to-device copy of the concatenated files, one read-back
        of the n statuses.  Raises JpegDecodeError for the first file that did not decode.  The tensor goes to DeviceResize.__call__,
        reference_resize and DeviceRaySet as it is."""
        files = list(files)
        if len(files) > self.max_images:
            raise ValueError(f'{len(files)} files for a decoder of max_images {self.max_images}')
        files_dev, offsets_dev = self.upload(files)
        out, status = self.decode_device(files_dev, offsets_dev, len(files), mode)
        st = status.cpu().numpy()
        if st.any():
            i = int(np.flatnonzero(st)[0])
            raise JpegDecodeError(i, st[i])
        return out


def load_jpeg(paths, mode='RGB', device=None):
    """uint8 (n, H, W, C) on the device from JPEG files: reads them, probes the first and checks the rest against its size.  Raises
    ValueError naming the path for a file the decoder does not take (progressive, CMYK, ...: decode those with PIL) or of another size."""
    paths = list(paths)
    files = []
    for p in paths:
        with open(p, 'rb') as f:
            files.append(f.read())
    if not files:
        raise ValueError('load_jpeg: no paths')
    first = probe(files[0])
    for p, data in zip(paths, files):
        info = probe(data)
        if not info.supported:
            raise ValueError(f'{p}: JPEG status {info.status} ({STATUS_NAMES[info.status]}) in its header: not decoded on the device')
        if (info.width, info.height) != (first.width, first.height):
            raise ValueError(f'{p}: {info.width} x {info.height}, the first file is {first.width} x {first.height}')
    dec = JpegDecoder(first.width, first.height, max_images=len(files), max_file_bytes=sum(len(f) for f in files), device=device)
    try:
        return dec.decode(files, mode)
    except JpegDecodeError as e:
        raise JpegDecodeError(e.index, e.status, what=f'{paths[e.index]}: image') from None
    finally:
        dec.close()


def build_decode_host():
    """g++ build of csrc/jpeg_decode_host.cpp, as png.build_host"""
    return _build_host(_DEC_LIB, _DEC_SRC, _DEC_DEPS)


def decode_host_lib():
    """the host build of csrc/hr_jpeg_decode.h (csrc/jpeg_decode_host.cpp), loaded once"""
    global _dec_host
    if _dec_host is None:
        _dec_host = C.CDLL(build_decode_host())
        _dec_host.hr_jpeg_host_probe.argtypes = [C.c_char_p, C.c_int64, C.POINTER(_lib.hr_jpeg_info)]
        _dec_host.hr_jpeg_host_probe.restype = C.c_int32
        _dec_host.hr_jpeg_host_decode.argtypes = [C.c_char_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                                  C.POINTER(_lib.hr_jpeg_info), C.POINTER(C.c_int32)]
        _dec_host.hr_jpeg_host_decode.restype = C.c_int32
        _dec_host.hr_jpeg_host_idct.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _dec_host.hr_jpeg_host_idct.restype = C.c_int32
    return _dec_host


def decode_host(data, mode='RGB', size=None, with_status=False, subseq_bits=0, with_rounds=False):
    """The pixels (H, W, C) of a file's bytes as a numpy array, decoded on the host by the header the kernels are built from: byte for
    byte, status for status and round for round what the device gives.  Needs no GPU.  size: (width, height) the file must have (a
    decoder's), default its own.  Raises JpegDecodeError -- or, with_status, returns (array, status), the array all zeros when the
    status is not 0; with_rounds appends the rounds the Huffman decode took."""
    host = decode_host_lib()
    data = bytes(data)
    c = _channels_of_mode(mode)
    if subseq_bits != 0 and (subseq_bits < 128 or subseq_bits % 32):
        raise ValueError(f'subseq_bits {subseq_bits} must be 0 or a multiple of 32 from 128 up')
    info = _lib.hr_jpeg_info()
    rounds = C.c_int32(0)
    if size is None:
        st = host.hr_jpeg_host_probe(data, len(data), C.byref(info))
        if info.width < 1 or info.height < 1:
            if with_status:
                return (np.zeros((0, 0, c), np.uint8), st or 2) + ((0,) if with_rounds else ())
            raise JpegDecodeError(0, st or 2)
        w, h, ew, eh = info.width, info.height, -1, -1
    else:
        w, h = int(size[0]), int(size[1])
        ew, eh = w, h
    if h * w * c > 1 << 31:
        raise ValueError(f'{w} x {h} x {c} is more than 2^31 bytes')
    out = np.empty((h, w, c), np.uint8)
    st = host.hr_jpeg_host_decode(data, len(data), ew, eh, c, int(subseq_bits), out.ctypes.data_as(C.c_void_p), C.byref(info), C.byref(rounds))
    if with_status:
        return (out, int(st)) + ((int(rounds.value),) if with_rounds else ())
    if st:
        raise JpegDecodeError(0, st)
    return (out, int(rounds.value)) if with_rounds else out
