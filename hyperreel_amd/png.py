"""PNG files on the device: rendered frames encoded (csrc/hr_png.h, png_kernel.hip) and training images decoded
(csrc/hr_png_decode.h, png_decode_kernel.hip).

    enc = PngEncoder(800, 800)                  # RGB; channels=4 for pack_display's RGBA8, 1 for a map
    data = enc.encode(rgb)                      # bytes of a complete PNG file
    save_png('frame.png', rgb)

replaces  Image.fromarray(to8b(rgb.cpu().numpy())).save(f) : the frame stays on the device, to8b is fused into the encoder's first read,
and the host copies the file's bytes, nothing else.  A float frame goes through to8b exactly as the display pack's does:
(uint8)(255 * clip(x, 0, 1)), NaN giving 0 -- numpy's own cast of NaN is undefined, so a frame with NaNs has no reference bytes.

    images_u8 = load_png(paths, 'RGB')          # (n, H, W, 3) uint8 on the device
    dec = PngDecoder(800, 800, max_images=16)
    images_u8 = dec.decode(list_of_bytes, 'RGBA')

replaces  np.stack([np.asarray(Image.open(p).convert('RGB')) for p in paths])  and its upload: the host reads the files' bytes and copies
them to the device once; the container's checksums, inflate, the PNG filters and PIL's convert run there, one image per workgroup.  8 bits a
sample, colour type 0 / 2 / 4 / 6, no interlace; probe() tells beforehand; JPEG files go to hyperreel_amd.jpeg (data.load_images picks by signature), and a caller keeps PIL for
palette, 16-bit and interlaced PNGs.
"""
import collections
import ctypes as C

import numpy as np

from . import _codec
from . import lib as _lib
from .build import host_library
from ._codec import MODES  # noqa: F401

FILTERS = {'adaptive': _lib.HR_PNG_FILTER_ADAPTIVE, 'none': 0, 'sub': 1, 'up': 2, 'average': 3, 'paeth': 4}
STATUS_NAMES = _lib.PNG_STATUS_NAMES
# the host builds of csrc/hr_png.h (csrc/png_host.cpp) and csrc/hr_png_decode.h (csrc/png_decode_host.cpp): g++ once, loaded once
build_host, host_lib = host_library('png_host', ('hr_png.h', 'hr_math.h'), {
    'hr_png_host_bound': (C.c_int64, [C.c_int32] * 3),
    'hr_png_host_encode': (C.c_int64, [C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p, C.c_int64] + [C.c_void_p] * 3)})
build_decode_host, decode_host_lib = host_library('png_decode_host', ('hr_png_decode.h', 'hr_png.h', 'hr_math.h'), {
    'hr_png_host_probe': (C.c_int32, [C.c_char_p, C.c_int64, C.POINTER(_lib.hr_png_info)]),
    'hr_png_host_decode': (C.c_int32, [C.c_char_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(_lib.hr_png_info)])})


def _filter_mode(filter):
    if isinstance(filter, str):
        if filter not in FILTERS:
            raise ValueError(f'filter {filter!r}: one of {sorted(FILTERS)} or a PNG filter number 0..4')
        return FILTERS[filter]
    return int(filter)


def bound(width, height, channels=3):
    """hr_png_bound: a capacity in bytes that always holds the file"""
    n = C.c_int64()
    _lib.call('hr_png_bound', int(width), int(height), int(channels), C.byref(n))
    return int(n.value)


class PngEncoder(_codec.Encoder):
    """Encodes (height, width, channels) frames on the device as PNG files: _codec.Encoder says what a frame is.  filter, per call: a
    name of FILTERS or a PNG filter number 0..4."""
    CREATE, ENCODE, DESTROY, BOUND = 'hr_png_encoder_create', 'hr_png_encode', 'hr_png_encoder_destroy', 'hr_png_bound'

    def __init__(self, width, height, channels=3, device=None):
        super().__init__(width, height, channels, device)

    def encode_device(self, frame, out=None, filter='adaptive', length=None):
        """_codec.Encoder.encode_device; filter: see the class"""
        return self._encode(frame, out, length, (_filter_mode(filter),))


def save_png(path, frame, width=None, height=None, filter='adaptive'):
    """Writes a device frame (H, W, C) or (H, W) -- or (H * W, C) with width and height given -- as a PNG file"""
    width, height, channels = _codec.frame_geometry(frame, width, height)
    enc = PngEncoder(width, height, channels, device=frame.device)
    try:
        data = enc.encode(frame, filter=filter)
    finally:
        enc.close()
    with open(path, 'wb') as f:
        f.write(data)
    return len(data)


def encode_host(array, channels=None, filter='adaptive'):
    """The same file from a numpy array (H, W, C) or (H, W), uint8 or float32, encoded on the host by the header the kernels are built
    from: byte for byte what the device writes.  Needs no GPU (and is as slow as a CPU encoder)."""
    host = host_lib()
    array, channels, h, w = _codec.array_geometry(array, channels)
    cap = host.hr_png_host_bound(w, h, channels) if array.size == h * w * channels else -1
    if cap < 0:
        raise ValueError(f'array {array.shape} is not an (H, W, {channels}) image the encoder takes (channels 1, 3 or 4; at least 1 x 1)')
    file = np.empty(cap, np.uint8)
    n = host.hr_png_host_encode(array.ctypes.data_as(C.c_void_p), _lib.HR_PNG_U8 if array.dtype == np.uint8 else _lib.HR_PNG_F32_TO8B,
                                _filter_mode(filter), w, h, channels, file.ctypes.data_as(C.c_void_p), file.size, None, None, None)
    if n < 0:
        raise RuntimeError('hr_png_encode_host refused the image')
    return file[:n].tobytes()


# ---- decoding ---------------------------------------------------------------------------------------------------------------------------
class PngDecodeError(_codec.DecodeError):
    """A file of a batch did not decode: .index is its place in the batch, .status the code, .status_name its name (STATUS_NAMES)"""
    FORMAT, STATUS_NAMES = 'PNG', STATUS_NAMES


PngInfo = collections.namedtuple('PngInfo', 'width height bit_depth color_type channels interlace supported')


def _info_tuple(info):
    return PngInfo(info.width, info.height, info.bit_depth, info.color_type, info.channels, info.interlace, bool(info.supported))


def probe(data):
    """hr_png_probe: (width, height, bit_depth, color_type, channels, interlace, supported) from the signature and IHDR of a file's bytes;
    `supported` says whether the decoder takes the file.  Raises for bytes that do not start as a PNG file does."""
    data = bytes(data)
    info = _lib.hr_png_info()
    _lib.call('hr_png_probe', data, len(data), C.byref(info))
    return _info_tuple(info)


class PngDecoder(_codec.Decoder):
    """Decodes batches of up to max_images PNG files of width x height on the device.  max_file_bytes bounds the files' total size in
    one call of decode (None: the raw size of max_images RGBA images plus 1/8, which no sensible file exceeds; a larger batch is
    refused).  The decoder owns its device workspace: one decode at a time per decoder."""
    CREATE, DECODE, DESTROY = 'hr_png_decoder_create', 'hr_png_decode', 'hr_png_decoder_destroy'
    Error, probe = PngDecodeError, staticmethod(probe)

    def default_file_bytes(self):
        return self.max_images * (self.height * (1 + 4 * self.width) * 9 // 8 + 4096)

    @staticmethod
    def refusal(info):
        return f'bit depth {info.bit_depth}, colour type {info.color_type}, interlace {info.interlace} is not decoded on the device'


def load_png(paths, mode='RGB', device=None):
    """uint8 (n, H, W, C) on the device from PNG files: reads them, probes the first and checks the rest against its size.  Raises
    ValueError naming the path for a file the decoder does not take (palette, 16 bits, interlaced: decode those with PIL) or of another
    size."""
    return PngDecoder.load(paths, mode, device)


def decode_host(data, mode='RGB', size=None, with_status=False):
    """The pixels (H, W, C) of a file's bytes as a numpy array, decoded on the host by the header the kernels are built from: byte for
    byte, and status for status, what the device gives.  Needs no GPU.  size: (width, height) the file must have (a decoder's), default
    its own.  Raises PngDecodeError -- or, with_status, returns (array, status), the array all zeros when the status is not 0."""
    host = decode_host_lib()
    data = bytes(data)
    c = _codec.channels_of_mode(mode)
    info = _lib.hr_png_info()
    if size is None:
        st = host.hr_png_host_probe(data, len(data), C.byref(info))
        if st:
            if with_status:
                return np.zeros((0, 0, c), np.uint8), st
            raise PngDecodeError(0, st)
        w, h, ew, eh = info.width, info.height, -1, -1
    else:
        w, h = int(size[0]), int(size[1])
        ew, eh = w, h
    if h * w * c > 1 << 31:
        raise ValueError(f'{w} x {h} x {c} is more than 2^31 bytes')
    out = np.empty((h, w, c), np.uint8)
    st = host.hr_png_host_decode(data, len(data), ew, eh, c, out.ctypes.data_as(C.c_void_p), C.byref(info))
    if with_status:
        return out, int(st)
    if st:
        raise PngDecodeError(0, st)
    return out
