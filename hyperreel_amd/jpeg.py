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

import numpy as np

from . import _codec
from . import lib as _lib
from .build import host_library

STATUS_NAMES = _lib.JPEG_STATUS_NAMES
# the host build of csrc/hr_jpeg_decode.h (csrc/jpeg_decode_host.cpp): g++ once, loaded once
build_decode_host, decode_host_lib = host_library('jpeg_decode_host', ('hr_jpeg_decode.h', 'hr_png_decode.h', 'hr_png.h', 'hr_math.h'), {
    'hr_jpeg_host_probe': (C.c_int32, [C.c_char_p, C.c_int64, C.POINTER(_lib.hr_jpeg_info)]),
    'hr_jpeg_host_decode': (C.c_int32, [C.c_char_p, C.c_int64] + [C.c_int32] * 4 + [C.c_void_p, C.POINTER(_lib.hr_jpeg_info), C.POINTER(C.c_int32)]),
    'hr_jpeg_host_idct': (C.c_int32, [C.c_void_p] * 3)})


class JpegDecodeError(_codec.DecodeError):
    """A file of a batch did not decode: .index is its place in the batch, .status the code, .status_name its name (STATUS_NAMES)"""
    FORMAT, STATUS_NAMES = 'JPEG', STATUS_NAMES


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


class JpegDecoder(_codec.Decoder):
    """Decodes batches of up to max_images JPEG files of width x height on the device.  max_file_bytes bounds the files' total size in one
    call of decode (None: the raw RGB size of max_images images, which no sensible file exceeds; a larger batch is refused).  subseq_bits:
    the length of the pieces a stream is cut into for the parallel Huffman decode, 0 for the default (1024), else a multiple of 32 from 128
    up; the pixels do not depend on it.  The decoder owns its device workspace: one decode at a time per decoder."""
    CREATE, DECODE, DESTROY = 'hr_jpeg_decoder_create', 'hr_jpeg_decode', 'hr_jpeg_decoder_destroy'
    Error, probe, MORE_OUTPUTS = JpegDecodeError, staticmethod(probe), ('rounds',)

    def __init__(self, width, height, max_images=1, max_file_bytes=None, subseq_bits=0, device=None):
        self.subseq_bits = int(subseq_bits)
        super().__init__(width, height, max_images, max_file_bytes, device, self.subseq_bits)

    def default_file_bytes(self):
        return self.max_images * (self.height * self.width * 3 + 4096)

    def decode_device(self, files_dev, offsets_dev, n, mode='RGB', out=None, status=None, rounds=None):
        """_codec.Decoder.decode_device; rounds: an int32 tensor of n elements that gets the rounds the Huffman decode took per image"""
        return super().decode_device(files_dev, offsets_dev, n, mode, out, status, rounds=rounds)

    @staticmethod
    def refusal(info):
        return f'JPEG status {info.status} ({STATUS_NAMES[info.status]}) in its header: not decoded on the device'


def load_jpeg(paths, mode='RGB', device=None):
    """uint8 (n, H, W, C) on the device from JPEG files: reads them, probes the first and checks the rest against its size.  Raises
    ValueError naming the path for a file the decoder does not take (progressive, CMYK, ...: decode those with PIL) or of another size."""
    return JpegDecoder.load(paths, mode, device)


def decode_host(data, mode='RGB', size=None, with_status=False, subseq_bits=0, with_rounds=False):
    """The pixels (H, W, C) of a file's bytes as a numpy array, decoded on the host by the header the kernels are built from: byte for
    byte, status for status and round for round what the device gives.  Needs no GPU.  size: (width, height) the file must have (a
    decoder's), default its own.  Raises JpegDecodeError -- or, with_status, returns (array, status), the array all zeros when the
    status is not 0; with_rounds appends the rounds the Huffman decode took."""
    host = decode_host_lib()
    data = bytes(data)
    c = _codec.channels_of_mode(mode)
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
