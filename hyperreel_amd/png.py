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
import os
import subprocess

import numpy as np

from . import lib as _lib

FILTERS = {'adaptive': _lib.HR_PNG_FILTER_ADAPTIVE, 'none': 0, 'sub': 1, 'up': 2, 'average': 3, 'paeth': 4}

_HERE = os.path.dirname(os.path.abspath(__file__))
_HOST_SRC = os.path.join(_HERE, 'csrc', 'png_host.cpp')
_HOST_DEPS = [_HOST_SRC, os.path.join(_HERE, 'csrc', 'hr_png.h'), os.path.join(_HERE, 'csrc', 'hr_math.h'),
              os.path.join(_HERE, '..', 'include', 'hyperreel_hip.h')]
_HOST_LIB = os.path.join(_HERE, '_build', 'libhr_png_host.so')
_host = None
_DEC_SRC = os.path.join(_HERE, 'csrc', 'png_decode_host.cpp')
_DEC_DEPS = _HOST_DEPS[1:] + [_DEC_SRC, os.path.join(_HERE, 'csrc', 'hr_png_decode.h')]
_DEC_LIB = os.path.join(_HERE, '_build', 'libhr_png_decode_host.so')
_dec_host = None
MODES = {'L': 1, 'RGB': 3, 'RGBA': 4}
STATUS_NAMES = _lib.PNG_STATUS_NAMES


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


class PngEncoder:
    """Encodes (height, width, channels) frames on the device: channels 1 (grey), 3 (RGB) or 4 (RGBA).  A frame is a device tensor:
    float32 (H, W, C) or (H * W, C) -- what model.render* returns -- or (H, W) for channels 1, turned into bytes by to8b as it is read;
    or uint8 of the same shapes (pack_display's RGBA8 with channels=4).  A frame that is not contiguous (a [..., :3] slice of a wider
    buffer) is copied into a contiguous one first.  The encoder owns its device workspace: one encode at a time per encoder."""

    def __init__(self, width, height, channels=3, device=None):
        import torch
        self.width, self.height, self.channels = int(width), int(height), int(channels)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self._h = C.c_void_p()
        _lib.call('hr_png_encoder_create', self.width, self.height, self.channels, C.byref(self._h), device=self.device)
        self.bound = bound(self.width, self.height, self.channels)

    def close(self):
        if getattr(self, '_h', None):
            _lib.call('hr_png_encoder_destroy', self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:          # interpreter teardown: the library or this module's globals may already be gone
            pass

    def _frame(self, frame):
        import torch
        if not isinstance(frame, torch.Tensor) or frame.device != self.device:
            raise ValueError(f'frame must be a tensor on {self.device}')
        if frame.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f'frame must be float32 or uint8, got {frame.dtype}')
        if frame.numel() != self.height * self.width * self.channels or (frame.dim() > 1 and self.channels > 1 and frame.shape[-1] != self.channels):
            raise ValueError(f'frame {tuple(frame.shape)} is not ({self.height}, {self.width}, {self.channels}) or ({self.height * self.width}, {self.channels})')
        return frame.contiguous()

    def encode_device(self, frame, out=None, filter='adaptive', length=None):
        """Enqueues the encode on torch's current stream and returns (uint8 buffer of `bound` bytes, int64 length tensor of one element):
        the file is buffer[:length].  No allocation when `out` and `length` are given, no synchronisation: capturable in a graph, with
        `frame` a contiguous buffer that is refilled between replays."""
        import torch
        frame = self._frame(frame)
        if out is None:
            out = torch.empty(self.bound, dtype=torch.uint8, device=self.device)
        elif out.dtype != torch.uint8 or out.device != self.device or not out.is_contiguous() or out.numel() < self.bound:
            raise ValueError(f'out must be a contiguous uint8 tensor of at least {self.bound} bytes on {self.device}')
        if length is None:
            length = torch.empty(1, dtype=torch.int64, device=self.device)
        elif length.dtype != torch.int64 or length.device != self.device or length.numel() != 1:
            raise ValueError(f'length must be an int64 tensor of one element on {self.device}')
        _lib.call('hr_png_encode', self._h, frame, _lib.HR_PNG_U8 if frame.dtype == torch.uint8 else _lib.HR_PNG_F32_TO8B, _filter_mode(filter), out,
                  out.numel(), length, _lib.stream(self.device), device=self.device)
        return out, length

    def encode(self, frame, filter='adaptive'):
        """The file's bytes: one device-to-host copy of the length, one of that many bytes"""
        out, length = self.encode_device(frame, filter=filter)
        n = int(length.item())
        return out[:n].cpu().numpy().tobytes()


def _channels_of(frame, channels):
    if channels is not None:
        return int(channels)
    return 1 if frame.ndim == 2 else int(frame.shape[-1])


def save_png(path, frame, width=None, height=None, filter='adaptive'):
    """Writes a device frame (H, W, C) or (H, W) -- or (H * W, C) with width and height given -- as a PNG file"""
    if frame.dim() == 3 or (frame.dim() == 2 and width is None):
        height, width = frame.shape[:2]
        channels = 1 if frame.dim() == 2 else frame.shape[2]
    else:
        if width is None or height is None:
            raise ValueError('a flat (H * W, C) frame needs width and height')
        channels = frame.shape[-1] if frame.dim() == 2 else 1
    enc = PngEncoder(width, height, channels, device=frame.device)
    try:
        data = enc.encode(frame, filter=filter)
    finally:
        enc.close()
    with open(path, 'wb') as f:
        f.write(data)
    return len(data)


def _build_host(lib, src, deps):
    import fcntl
    os.makedirs(os.path.dirname(lib), exist_ok=True)
    with open(lib + '.lock', 'w') as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
            tmp = f'{lib}.{os.getpid()}.tmp'
            subprocess.run(['g++', '-O2', '-ffp-contract=off', '-fno-fast-math', '-shared', '-fPIC', '-o', tmp, src], check=True)
            os.replace(tmp, lib)
    return lib


def build_host():
    """g++ build of csrc/png_host.cpp (once; one builder at a time, the library appears atomically)"""
    return _build_host(_HOST_LIB, _HOST_SRC, _HOST_DEPS)


def build_decode_host():
    """g++ build of csrc/png_decode_host.cpp, as build_host"""
    return _build_host(_DEC_LIB, _DEC_SRC, _DEC_DEPS)


def host_lib():
    """the host build of csrc/hr_png.h (csrc/png_host.cpp), loaded once"""
    global _host
    if _host is None:
        _host = C.CDLL(build_host())
        _host.hr_png_host_bound.argtypes = [C.c_int32, C.c_int32, C.c_int32]
        _host.hr_png_host_bound.restype = C.c_int64
        _host.hr_png_host_encode.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                             C.c_void_p, C.c_void_p]
        _host.hr_png_host_encode.restype = C.c_int64
    return _host


def encode_host(array, channels=None, filter='adaptive'):
    """The same file from a numpy array (H, W, C) or (H, W), uint8 or float32, encoded on the host by the header the kernels are built
    from: byte for byte what the device writes.  Needs no GPU (and is as slow as a CPU encoder)."""
    host = host_lib()
    array = np.ascontiguousarray(array)
    if array.dtype not in (np.uint8, np.float32) or array.ndim not in (2, 3):
        raise ValueError(f'array must be uint8 or float32 of shape (H, W, C) or (H, W), got {array.dtype} {array.shape}')
    channels = _channels_of(array, channels)
    h, w = array.shape[:2]
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
class PngDecodeError(ValueError):
    """A file of a batch did not decode: .index is its place in the batch, .status the code, .status_name its name (STATUS_NAMES)"""

    def __init__(self, index, status, what='image'):
        self.index, self.status = int(index), int(status)
        self.status_name = STATUS_NAMES[self.status] if 0 <= self.status < len(STATUS_NAMES) else str(self.status)
        super().__init__(f'{what} {self.index}: PNG status {self.status} ({self.status_name})')


def _channels_of_mode(mode):
    if mode not in MODES:
        raise ValueError(f'mode {mode!r}: one of {sorted(MODES)}')
    return MODES[mode]


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


class PngDecoder:
    """Decodes batches of up to max_images PNG files of width x height on the device.  max_file_bytes bounds the files' total size in
    one call of decode (None: the raw size of max_images RGBA images plus 1/8, which no sensible file exceeds; a larger batch is
    refused).  The decoder owns its device workspace: one decode at a time per decoder."""

    def __init__(self, width, height, max_images=1, max_file_bytes=None, device=None):
        import torch
        self.width, self.height, self.max_images = int(width), int(height), int(max_images)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if max_file_bytes is None:
            max_file_bytes = self.max_images * (self.height * (1 + 4 * self.width) * 9 // 8 + 4096)
        self.max_file_bytes = int(max_file_bytes)
        self._files = None
        self._h = C.c_void_p()
        _lib.call('hr_png_decoder_create', self.width, self.height, self.max_images, self.max_file_bytes, C.byref(self._h), device=self.device)

    def close(self):
        if getattr(self, '_h', None):
            _lib.call('hr_png_decoder_destroy', self._h)
            self._h = None
            self._files = None

    def __del__(self):
        try:
            self.close()
        except Exception:          # interpreter teardown: the library or this module's globals may already be gone
            pass

    def decode_device(self, files_dev, offsets_dev, n, mode='RGB', out=None, status=None):
        """Enqueues the decode on torch's current stream: files_dev a uint8 tensor of max_file_bytes bytes or more holding the files one
        after another, offsets_dev an int64 tensor of n + 1 bounds.  Returns (out (n, H, W, C) uint8, status (n,) int32): status 0 is a
        decoded image, anything else (STATUS_NAMES) an all-zero one.  No allocation when `out` and `status` are given, no synchronisation:
        capturable in a graph, with files_dev and offsets_dev refilled between replays."""
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
        elif status.dtype != torch.int32 or status.device != self.device or not status.is_contiguous() or status.numel() != n:
            raise ValueError(f'status must be a contiguous int32 tensor of {n} elements on {self.device}')
        # an empty batch passes the library's own n_images == 0 path: nothing is launched
        _lib.call('hr_png_decode', self._h, files_dev, offsets_dev, n, c, out, status, _lib.stream(self.device), device=self.device)
        return out, status

    def upload(self, files):
        """(files_dev, offsets_dev) of a list of files' bytes: one host-to-device copy of the concatenated files (the offsets, n + 1
        int64, ride in front of them in the same buffer).  The device buffer belongs to the decoder and is reused: the two tensors
        are valid until the next upload.  More than max_file_bytes in all is refused -- the decoder, and with it any graph captured
        over decode_device, stays as it was created."""
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
        of the n statuses.  Raises PngDecodeError for the first file that did not decode.  The tensor goes to DeviceResize.__call__,
        reference_resize and DeviceRaySet as it is."""
        files = list(files)
        if len(files) > self.max_images:
            raise ValueError(f'{len(files)} files for a decoder of max_images {self.max_images}')
        files_dev, offsets_dev = self.upload(files)
        out, status = self.decode_device(files_dev, offsets_dev, len(files), mode)
        st = status.cpu().numpy()
        if st.any():
            i = int(np.flatnonzero(st)[0])
            raise PngDecodeError(i, st[i])
        return out


def load_png(paths, mode='RGB', device=None):
    """uint8 (n, H, W, C) on the device from PNG files: reads them, probes the first and checks the rest against its size.  Raises
    ValueError naming the path for a file the decoder does not take (palette, 16 bits, interlaced: decode those with PIL) or of another
    size."""
    paths = list(paths)
    files = []
    for p in paths:
        with open(p, 'rb') as f:
            files.append(f.read())
    if not files:
        raise ValueError('load_png: no paths')
    first = probe(files[0])
    for p, data in zip(paths, files):
        info = probe(data)
        if not info.supported:
            raise ValueError(f'{p}: bit depth {info.bit_depth}, colour type {info.color_type}, interlace {info.interlace} is not decoded on the device')
        if (info.width, info.height) != (first.width, first.height):
            raise ValueError(f'{p}: {info.width} x {info.height}, the first file is {first.width} x {first.height}')
    dec = PngDecoder(first.width, first.height, max_images=len(files), max_file_bytes=sum(len(f) for f in files), device=device)
    try:
        return dec.decode(files, mode)
    except PngDecodeError as e:
        raise PngDecodeError(e.index, e.status, what=f'{paths[e.index]}: image') from None
    finally:
        dec.close()


def decode_host_lib():
    """the host build of csrc/hr_png_decode.h (csrc/png_decode_host.cpp), loaded once"""
    global _dec_host
    if _dec_host is None:
        _dec_host = C.CDLL(build_decode_host())
        _dec_host.hr_png_host_probe.argtypes = [C.c_char_p, C.c_int64, C.POINTER(_lib.hr_png_info)]
        _dec_host.hr_png_host_probe.restype = C.c_int32
        _dec_host.hr_png_host_decode.argtypes = [C.c_char_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(_lib.hr_png_info)]
        _dec_host.hr_png_host_decode.restype = C.c_int32
    return _dec_host


def decode_host(data, mode='RGB', size=None, with_status=False):
    """The pixels (H, W, C) of a file's bytes as a numpy array, decoded on the host by the header the kernels are built from: byte for
    byte, and status for status, what the device gives.  Needs no GPU.  size: (width, height) the file must have (a decoder's), default
    its own.  Raises PngDecodeError -- or, with_status, returns (array, status), the array all zeros when the status is not 0."""
    host = decode_host_lib()
    data = bytes(data)
    c = _channels_of_mode(mode)
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
