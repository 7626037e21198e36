"""JPEG files on the device, png.py's sibling: training images decoded (csrc/hr_jpeg_decode.h, jpeg_decode_kernel.hip) and
rendered frames encoded (csrc/hr_jpeg_encode.h, jpeg_encode_kernel.hip).

    images_u8 = load_jpeg(paths, 'RGB')         # (n, H, W, 3) uint8 on the device
    dec = JpegDecoder(4032, 3024, max_images=8)
    images_u8 = dec.decode(list_of_bytes, 'RGB')

replaces  np.stack([np.asarray(Image.open(p).convert('RGB')) for p in paths])  and its upload (datasets/llff.py, shiny.py: the cameras'
full-size JPEGs): the host reads the files' bytes and copies them to the device once; the markers, Huffman decoding -- parallel inside one
stream -- libjpeg's IDCT, chroma upsampling, colour conversion and PIL's convert run there, byte for byte as PIL 12.2 / libjpeg-turbo 3.1
give them.  Baseline and extended sequential Huffman files at 8 bits, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0, one scan, with or without
restart markers; probe() tells beforehand.  Progressive, arithmetic, CMYK and other samplings are refused by name: decode those with PIL.

    enc = JpegEncoder(800, 800, quality=90, subsampling='4:2:0')      # RGB; channels=4 for pack_display's RGBA8, 1 for a map
    data = enc.encode(rgb)                      # bytes of a complete baseline JPEG file
    save_jpeg('frame.jpg', rgb)

replaces  Image.fromarray(to8b(rgb.cpu().numpy())).save(f, 'JPEG', quality=90, subsampling=2) : the frame stays on the device, to8b is
fused into the encoder's first read, and the host copies the file's bytes -- PIL 12.2's own, byte for byte -- and nothing else.
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


class hr_jpeg_enc_stats(C.Structure):
    """What hr_jpeg_host_encode reports of a scan (csrc/hr_jpeg_encode.h)."""
    _fields_ = [('stuffed', C.c_int64), ('zrl', C.c_int64), ('max_dc_cat', C.c_int32), ('max_ac_cat', C.c_int32)]


# ... and of csrc/hr_jpeg_encode.h (csrc/jpeg_encode_host.cpp)
build_host, host_lib = host_library('jpeg_encode_host', ('hr_jpeg_encode.h', 'hr_jpeg_decode.h', 'hr_png_decode.h', 'hr_png.h', 'hr_math.h'), {
    'hr_jpeg_host_bound': (C.c_int64, [C.c_int32] * 5),
    'hr_jpeg_host_encode': (C.c_int64, [C.c_void_p] + [C.c_int32] * 7 + [C.c_void_p, C.c_int64, C.POINTER(hr_jpeg_enc_stats)])})
SUBSAMPLINGS = {'4:4:4': _lib.HR_JPEG_444, '4:2:2': _lib.HR_JPEG_422, '4:2:0': _lib.HR_JPEG_420}


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


# ---- encoding ---------------------------------------------------------------------------------------------------------------------------
def _subsampling(subsampling):
    """the C ABI's number of '4:4:4' | '4:2:2' | '4:2:0' or of PIL's 0 | 1 | 2"""
    if isinstance(subsampling, str):
        if subsampling not in SUBSAMPLINGS:
            raise ValueError(f'subsampling {subsampling!r}: one of {sorted(SUBSAMPLINGS)} or PIL\'s number 0, 1, 2')
        subsampling = SUBSAMPLINGS[subsampling]
    return int(subsampling)


def bound(width, height, channels=3, subsampling='4:2:0', restart_rows=0):
    """hr_jpeg_bound: a capacity in bytes that always holds the file"""
    n = C.c_int64()
    _lib.call('hr_jpeg_bound', int(width), int(height), int(channels), _subsampling(subsampling), int(restart_rows), C.byref(n))
    return int(n.value)


class JpegEncoder(_codec.Encoder):
    """Encodes (height, width, channels) frames on the device as baseline JPEG files: channels 1 (grey, subsampling '4:4:4'), 3 (RGB) or 4
    (RGBA, the alpha byte ignored).  quality 1..100 and subsampling '4:4:4' | '4:2:2' | '4:2:0' as PIL's save; restart_rows > 0 puts a
    restart marker after every so many MCU rows.  _codec.Encoder says what a frame is."""
    CREATE, ENCODE, DESTROY, BOUND = 'hr_jpeg_encoder_create', 'hr_jpeg_encode', 'hr_jpeg_encoder_destroy', 'hr_jpeg_bound'

    def __init__(self, width, height, channels=3, quality=90, subsampling='4:2:0', restart_rows=0, device=None):
        self.quality, self.restart_rows = int(quality), int(restart_rows)
        self.subsampling = _subsampling(subsampling)
        super().__init__(width, height, channels, device, (self.quality, self.subsampling, self.restart_rows), (self.subsampling, self.restart_rows))


def save_jpeg(path, frame, width=None, height=None, **options):
    """Writes a device frame (H, W, C) or (H, W) -- or (H * W, C) with width and height given -- as a JPEG file; options: JpegEncoder's
    quality, subsampling, restart_rows.  A grey frame is written 4:4:4 unless a subsampling is asked for."""
    width, height, channels = _codec.frame_geometry(frame, width, height)
    if channels == 1:
        options.setdefault('subsampling', '4:4:4')
    enc = JpegEncoder(width, height, channels, device=frame.device, **options)
    try:
        data = enc.encode(frame)
    finally:
        enc.close()
    with open(path, 'wb') as f:
        f.write(data)
    return len(data)


def encode_host(array, channels=None, quality=90, subsampling='4:2:0', restart_rows=0, with_stats=False):
    """The same file from a numpy array (H, W, C) or (H, W), uint8 or float32, encoded on the host by the header the kernels are built
    from: byte for byte what the device writes.  Needs no GPU.  A grey array takes subsampling '4:4:4' only, as the device does.
    with_stats: (bytes, {'stuffed', 'zrl', 'max_dc_cat', 'max_ac_cat'}) of the scan."""
    host = host_lib()
    array, channels, h, w = _codec.array_geometry(array, channels)
    sub = _subsampling(subsampling)
    cap = host.hr_jpeg_host_bound(w, h, channels, sub, int(restart_rows)) if array.size == h * w * channels and 1 <= int(quality) <= 100 else -1
    if cap < 0:
        raise ValueError(f'array {array.shape}, quality {quality}, subsampling {subsampling}, restart_rows {restart_rows}: not an image and options '
                         f'the encoder takes (channels 1, 3 or 4; 1 x 1 to 65535 x 65535; quality 1..100; grey only 4:4:4)')
    file = np.empty(cap, np.uint8)
    stats = hr_jpeg_enc_stats()
    n = host.hr_jpeg_host_encode(array.ctypes.data_as(C.c_void_p), _lib.HR_PNG_U8 if array.dtype == np.uint8 else _lib.HR_PNG_F32_TO8B, w, h, channels,
                                 int(quality), sub, int(restart_rows), file.ctypes.data_as(C.c_void_p), file.size, C.byref(stats))
    if n < 0:
        raise RuntimeError('hr_jpeg_encode_host refused the image')
    data = file[:n].tobytes()
    if with_stats:
        return data, {'stuffed': stats.stuffed, 'zrl': stats.zrl, 'max_dc_cat': stats.max_dc_cat, 'max_ac_cat': stats.max_ac_cat}
    return data
