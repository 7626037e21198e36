"""Rendered frames as PNG files, encoded on the device (csrc/hr_png.h, png_kernel.hip).

    enc = PngEncoder(800, 800)                  # RGB; channels=4 for pack_display's RGBA8, 1 for a map
    data = enc.encode(rgb)                      # bytes of a complete PNG file
    save_png('frame.png', rgb)

replaces  Image.fromarray(to8b(rgb.cpu().numpy())).save(f) : the frame stays on the device, to8b is fused into the encoder's first read,
and the host copies the file's bytes, nothing else.  A float frame goes through to8b exactly as the display pack's does:
(uint8)(255 * clip(x, 0, 1)), NaN giving 0 -- numpy's own cast of NaN is undefined, so a frame with NaNs has no reference bytes.
"""
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


def build_host():
    """g++ build of csrc/png_host.cpp (once; one builder at a time, the library appears atomically)"""
    import fcntl
    os.makedirs(os.path.dirname(_HOST_LIB), exist_ok=True)
    with open(_HOST_LIB + '.lock', 'w') as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if not os.path.exists(_HOST_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_HOST_LIB) for d in _HOST_DEPS):
            tmp = f'{_HOST_LIB}.{os.getpid()}.tmp'
            subprocess.run(['g++', '-O2', '-ffp-contract=off', '-fno-fast-math', '-shared', '-fPIC', '-o', tmp, _HOST_SRC], check=True)
            os.replace(tmp, _HOST_LIB)
    return _HOST_LIB


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
