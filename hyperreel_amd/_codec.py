"""What the image codecs share (png.py, jpeg.py): the output modes, the error's base, the packing of a batch of files, the geometry and
the checks of a frame to encode, and the decoder and encoder front ends around a native handle.  A format's module states its C symbols,
its status names and its own arguments, nothing else."""
import ctypes as C

import numpy as np

from . import lib as _lib

MODES = {'L': 1, 'RGB': 3, 'RGBA': 4}


def channels_of_mode(mode):
    if mode not in MODES:
        raise ValueError(f'mode {mode!r}: one of {sorted(MODES)}')
    return MODES[mode]


class HandleOwner:
    """Owns one handle of the library, self._h, which the C symbol named DESTROY frees: close() any number of times, and at the latest
    when the object goes."""
    DESTROY = None
    _h = None

    def close(self):
        if self._h:
            _lib.call(self.DESTROY, self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:          # interpreter teardown: the library or this module's globals may already be gone
            pass


class DecodeError(ValueError):
    """A file of a batch did not decode: .index is its place in the batch, .status the code, .status_name its name (STATUS_NAMES)"""
    FORMAT, STATUS_NAMES = None, ()

    def __init__(self, index, status, what='image'):
        self.index, self.status = int(index), int(status)
        self.status_name = self.STATUS_NAMES[self.status] if 0 <= self.status < len(self.STATUS_NAMES) else str(self.status)
        super().__init__(f'{what} {self.index}: {self.FORMAT} status {self.status} ({self.status_name})')


def pack_files(files, max_images, max_file_bytes):
    """The host uint8 array a decoder's upload copies to the device: the n + 1 int64 bounds of the files, from 0, at the front, the files
    one after another from byte 8 * (max_images + 1).  More than max_images files or max_file_bytes bytes in all are refused."""
    if len(files) > max_images:
        raise ValueError(f'{len(files)} files for a decoder of max_images {max_images}')
    sizes = [len(f) for f in files]
    total = sum(sizes)
    if total > max_file_bytes:
        raise ValueError(f'{total} bytes of files for a decoder of max_file_bytes {max_file_bytes}: create it with a larger one')
    head = 8 * (max_images + 1)
    host = np.empty(head + total, np.uint8)
    host[:8 * (len(files) + 1)].view(np.int64)[:] = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)])
    at = head
    for f in files:
        host[at:at + len(f)] = np.frombuffer(f, np.uint8)
        at += len(f)
    return host


class Decoder(HandleOwner):
    """Decodes batches of up to max_images files of width x height on the device; max_file_bytes bounds the files' total size in one call
    of decode (None: the subclass's default_file_bytes; a larger batch is refused).  The decoder owns its device workspace: one decode at a
    time per decoder.  A subclass states CREATE, DECODE and DESTROY (C symbols; create_args follow max_file_bytes in CREATE), Error,
    MORE_OUTPUTS (per-image int32 outputs of DECODE after status), probe, default_file_bytes and refusal."""
    CREATE = DECODE = Error = probe = None
    MORE_OUTPUTS = ()

    def __init__(self, width, height, max_images=1, max_file_bytes=None, device=None, *create_args):
        import torch
        self.width, self.height, self.max_images = int(width), int(height), int(max_images)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_file_bytes = int(self.default_file_bytes() if max_file_bytes is None else max_file_bytes)
        self._files = None
        self._h = C.c_void_p()
        _lib.call(self.CREATE, self.width, self.height, self.max_images, self.max_file_bytes, *create_args, C.byref(self._h), device=self.device)

    def close(self):
        super().close()
        self._files = None

    def decode_device(self, files_dev, offsets_dev, n, mode='RGB', out=None, status=None, **more):
        """Enqueues the decode on torch's current stream: files_dev a uint8 tensor of max_file_bytes bytes or more holding the files one
        after another, offsets_dev an int64 tensor of n + 1 bounds.  Returns (out (n, H, W, C) uint8, status (n,) int32): status 0 is a
        decoded image, anything else (STATUS_NAMES) an all-zero one.  more: MORE_OUTPUTS by name, int32 tensors of n elements or None.
        No allocation when `out` and `status` are given, no synchronisation: capturable in a graph, with files_dev and offsets_dev
        refilled between replays."""
        import torch
        if set(more) - set(self.MORE_OUTPUTS):
            raise TypeError(f'decode_device: unexpected arguments {sorted(set(more) - set(self.MORE_OUTPUTS))}')
        more = [(name, more.get(name)) for name in self.MORE_OUTPUTS]
        c, n = channels_of_mode(mode), int(n)
        for name, t, dtype, count in (('files_dev', files_dev, torch.uint8, self.max_file_bytes), ('offsets_dev', offsets_dev, torch.int64, n + 1)):
            if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != dtype or not t.is_contiguous() or t.numel() < count:
                raise ValueError(f'{name} must be a contiguous {dtype} tensor of at least {count} elements on {self.device}')
        if out is None:
            out = torch.empty((n, self.height, self.width, c), dtype=torch.uint8, device=self.device)
        elif out.dtype != torch.uint8 or out.device != self.device or not out.is_contiguous() or out.numel() != n * self.height * self.width * c:
            raise ValueError(f'out must be a contiguous uint8 tensor ({n}, {self.height}, {self.width}, {c}) on {self.device}')
        if status is None:
            status = torch.empty(n, dtype=torch.int32, device=self.device)
        for name, t in [('status', status)] + more:
            if t is not None and (t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous() or t.numel() != n):
                raise ValueError(f'{name} must be a contiguous int32 tensor of {n} elements on {self.device}')
        # an empty batch passes the library's own n_images == 0 path: nothing is launched
        _lib.call(self.DECODE, self._h, files_dev, offsets_dev, n, c, out, status, *[t for _, t in more], _lib.stream(self.device), device=self.device)
        return out, status

    def upload(self, files):
        """(files_dev, offsets_dev) of a list of files' bytes: one host-to-device copy of pack_files' array, the offsets in front of the
        concatenated files.  The device buffer belongs to the decoder and is reused: the two tensors are valid until the next upload.
        More than max_file_bytes in all is refused -- the decoder, and with it any graph captured over decode_device, stays as it was
        created."""
        import torch
        host = pack_files(files, self.max_images, self.max_file_bytes)
        head = 8 * (self.max_images + 1)
        if self._files is None:
            self._files = torch.empty(head + max(self.max_file_bytes, 1), dtype=torch.uint8, device=self.device)
        self._files[:host.size].copy_(torch.from_numpy(host))
        return self._files[head:], self._files[:8 * (len(files) + 1)].view(torch.int64)

    def decode(self, files, mode='RGB'):
        """uint8 (n, H, W, C) on the device from a list of files' bytes: one host-to-device copy of the concatenated files, one read-back
        of the n statuses.  Raises Error (PngDecodeError, JpegDecodeError) for the first file that did not decode.  The tensor goes to
        DeviceResize.__call__, reference_resize and DeviceRaySet as it is."""
        files = list(files)
        files_dev, offsets_dev = self.upload(files)
        out, status = self.decode_device(files_dev, offsets_dev, len(files), mode)
        st = status.cpu().numpy()
        if st.any():
            i = int(np.flatnonzero(st)[0])
            raise self.Error(i, st[i])
        return out

    @classmethod
    def load(cls, paths, mode='RGB', device=None):
        """uint8 (n, H, W, C) on the device from files: reads them, probes the first and checks the rest against its size.  Raises
        ValueError naming the path for a file the decoder does not take (cls.refusal says why) or of another size."""
        paths = list(paths)
        files = []
        for p in paths:
            with open(p, 'rb') as f:
                files.append(f.read())
        if not files:
            raise ValueError(f'load_{cls.Error.FORMAT.lower()}: no paths')
        first = cls.probe(files[0])
        for p, data in zip(paths, files):
            info = cls.probe(data)
            if not info.supported:
                raise ValueError(f'{p}: {cls.refusal(info)}')
            if (info.width, info.height) != (first.width, first.height):
                raise ValueError(f'{p}: {info.width} x {info.height}, the first file is {first.width} x {first.height}')
        dec = cls(first.width, first.height, max_images=len(files), max_file_bytes=sum(len(f) for f in files), device=device)
        try:
            return dec.decode(files, mode)
        except cls.Error as e:
            raise cls.Error(e.index, e.status, what=f'{paths[e.index]}: image') from None
        finally:
            dec.close()


# ---- encoding ---------------------------------------------------------------------------------------------------------------------------
def frame_geometry(frame, width=None, height=None):
    """(width, height, channels) of a frame (H, W, C) or (H, W) -- or, with width and height given, of a flat (H * W, C) or (H * W,) one"""
    if frame.dim() == 3 or (frame.dim() == 2 and width is None):
        height, width = frame.shape[:2]
        channels = 1 if frame.dim() == 2 else frame.shape[2]
    else:
        if width is None or height is None:
            raise ValueError('a flat (H * W, C) frame needs width and height')
        channels = frame.shape[-1] if frame.dim() == 2 else 1
    return int(width), int(height), int(channels)


torch = None      # the module, from the first check of a tensor on: the checks run in every encode, and encode_host needs numpy alone


def _bind_torch():
    global torch
    import torch


def check_frame(frame, device, width, height, channels):
    """The frame an encoder of width x height x channels on `device` takes, contiguous: float32 or uint8, (H, W, C), (H * W, C) or, for
    channels 1, (H, W).  Anything else is refused."""
    if torch is None:
        _bind_torch()
    if not isinstance(frame, torch.Tensor) or frame.device != device:
        raise ValueError(f'frame must be a tensor on {device}')
    if frame.dtype is not torch.float32 and frame.dtype is not torch.uint8:
        raise ValueError(f'frame must be float32 or uint8, got {frame.dtype}')
    if frame.numel() != height * width * channels or (frame.dim() > 1 and channels > 1 and frame.shape[-1] != channels):
        raise ValueError(f'frame {tuple(frame.shape)} is not ({height}, {width}, {channels}) or ({height * width}, {channels})')
    return frame.contiguous()


def check_out(out, device, bound):
    if torch is None:
        _bind_torch()
    if out.dtype is not torch.uint8 or out.device != device or not out.is_contiguous() or out.numel() < bound:
        raise ValueError(f'out must be a contiguous uint8 tensor of at least {bound} bytes on {device}')
    return out


def check_length(length, device):
    if torch is None:
        _bind_torch()
    if length.dtype is not torch.int64 or length.device != device or length.numel() != 1:
        raise ValueError(f'length must be an int64 tensor of one element on {device}')
    return length


def array_geometry(array, channels=None):
    """(the array made contiguous, channels, height, width) of a numpy image (H, W, C) or (H, W), uint8 or float32: the front of the
    formats' encode_host.  channels: the caller's, else 1 for (H, W) and C otherwise."""
    array = np.ascontiguousarray(array)
    if array.dtype not in (np.uint8, np.float32) or array.ndim not in (2, 3):
        raise ValueError(f'array must be uint8 or float32 of shape (H, W, C) or (H, W), got {array.dtype} {array.shape}')
    if channels is None:
        channels = 1 if array.ndim == 2 else array.shape[-1]
    return array, int(channels), int(array.shape[0]), int(array.shape[1])


class Encoder(HandleOwner):
    """Encodes (height, width, channels) frames on the device: channels 1 (grey), 3 (RGB) or 4 (RGBA).  A frame is a device tensor:
    float32 (H, W, C) or (H * W, C) -- what model.render* returns -- or (H, W) for channels 1, turned into bytes by to8b as it is read;
    or uint8 of the same shapes (pack_display's RGBA8 with channels=4).  A frame that is not contiguous (a [..., :3] slice of a wider
    buffer) is copied into a contiguous one first.  The encoder owns its device workspace: one encode at a time per encoder.  A subclass
    states CREATE, ENCODE, DESTROY and BOUND (C symbols; create_args follow channels in CREATE, bound_args in BOUND) and, where ENCODE has
    arguments of its own between pixel_type and file_dev, an encode_device that takes them after `out` and hands them to _encode."""
    CREATE = ENCODE = BOUND = None

    def __init__(self, width, height, channels=3, device=None, create_args=(), bound_args=()):
        import torch
        self.width, self.height, self.channels = int(width), int(height), int(channels)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self._h = C.c_void_p()
        _lib.call(self.CREATE, self.width, self.height, self.channels, *create_args, C.byref(self._h), device=self.device)
        n = C.c_int64()
        _lib.call(self.BOUND, self.width, self.height, self.channels, *bound_args, C.byref(n))
        self.bound = int(n.value)

    def _encode(self, frame, out, length, options):
        """encode_device with the format's own arguments of ENCODE as a tuple"""
        device = self.device
        frame = check_frame(frame, device, self.width, self.height, self.channels)          # binds torch
        out = torch.empty(self.bound, dtype=torch.uint8, device=device) if out is None else check_out(out, device, self.bound)
        length = torch.empty(1, dtype=torch.int64, device=device) if length is None else check_length(length, device)
        _lib.call(self.ENCODE, self._h, frame, _lib.HR_PNG_U8 if frame.dtype is torch.uint8 else _lib.HR_PNG_F32_TO8B, *options, out, out.numel(),
                  length, _lib.stream(device), device=device)
        return out, length

    def encode_device(self, frame, out=None, length=None):
        """Enqueues the encode on torch's current stream and returns (uint8 buffer of `bound` bytes, int64 length tensor of one element):
        the file is buffer[:length], and no byte past it is written.  No allocation when `out` and `length` are given, no
        synchronisation: capturable in a graph, with `frame` a contiguous buffer that is refilled between replays."""
        return self._encode(frame, out, length, ())

    def encode(self, frame, *options, **named):
        """The file's bytes: one device-to-host copy of the length, one of that many bytes.  options: what follows `out` in encode_device."""
        out, length = self.encode_device(frame, None, *options, **named)
        return out[:int(length.item())].cpu().numpy().tobytes()
