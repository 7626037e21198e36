"""The training feed on the device (include/hyperreel_hip.h: hr_rayset_*).

The reference's datasets build `all_inputs`, a host float tensor of ray_dim + 4 floats per training ray
(datasets/base.py:130-143, datasets/technicolor.py:238-282), shuffle it on the host every epoch (base.py:202-227) and
slice batches out of it (format_batch, base.py:278-284).  A DeviceRaySet keeps the 8-bit images in device memory with
one camera and one subsample rule per image, and computes a batch's rays when they are drawn.  Nothing here reads
files: decoding images stays with the caller.  No CPU path: a missing library or a failing call raises.

Immersive's fisheye cameras (datasets/immersive.py:43-48, 514-523) pass `distortions=`: each image's (k1, k2), undistorted per ray on the
device.  Its subsample rule, importance_subsample (immersive.py:295-310), depends on the pixels: `subsample=` takes one
Importance(...) per such image (DeviceRaySet.importance_rule) and the device selects, masks and compacts the kept pixels into a list
(hr_rayset_set_image_importance).

DeviceRaySet.from_lightfield does the same for the two-plane light-field datasets (datasets/lightfield.py,
datasets/stanford.py): a position (s, t) on the camera plane per view instead of a camera.

DeviceResize / reference_resize are the stage in front of the set: the resize every PIL-based dataset applies to a decoded image in
get_rgb (datasets/llff.py:145-163), on the device and byte for byte as PIL computes it (hr_image_resize)."""
import collections
import ctypes as C

import numpy as np
import torch

from . import lib as _lib
from ._codec import HandleOwner
from .plan import hr_camera, hr_fisheye, hr_lightfield, hr_ndc

# subsample rules of the reference's datasets that are not the checkerboard: named so that the refusal can say which
UNSUPPORTED_RULES = {
    'random_subsample': 'datasets/neural_3d.py:152-166 draws np.random.permutation per image',
    'importance_subsample': 'datasets/immersive.py:295-310, datasets/neural_3d.py:191-204: it depends on the pixels, so it has no name-only form '
                            '-- pass one Importance(num_take, prev, dir_z_below) per image, as DeviceRaySet.importance_rule builds them',
    'test_subsample': 'datasets/neural_3d.py:187-189 masks on a ray coordinate',
    'fisheye': 'a camera model, not a subsample rule: pass distortions= (datasets/immersive.py:43-48,514-523; DESIGN 3h)',
}


class Importance(collections.namedtuple('Importance', ['num_take', 'prev', 'dir_z_below'], defaults=(None, None))):
    """One image's importance rule in DeviceRaySet(subsample=[...]) (importance_subsample, datasets/immersive.py:295-310): keep the pixels
    whose mean absolute difference to image `prev` (default: the image before this one) is strictly greater than the num_take-th largest
    of the image, and whose ray has coords[..., 5] < dir_z_below (None: no direction test, datasets/neural_3d.py:191-204)."""
    __slots__ = ()


def _parse_rules(subsample, n, n_pixels, lightfield=False, alpha=None):
    """None | a rule name | one (every, offset) or Importance per image -> the per-image list, checked before any library call."""
    if isinstance(subsample, str):
        _refuse_rule(subsample)
    if subsample is None:
        return [(1, 0)] * n
    rules = []
    for i, r in enumerate(subsample):
        if isinstance(r, Importance):
            if lightfield:
                raise ValueError(f'view {i}: the importance rule compares video frames of posed cameras; a light-field set takes (every, offset) pairs only')
            if alpha is not None:
                raise ValueError(f'image {i}: the importance rule compares 8-bit RGB frames (the reference\'s importance datasets load RGB); '
                                 f'a set with alpha={alpha!r} takes (every, offset) pairs only')
            take, prev = int(r.num_take), (i - 1 if r.prev is None else int(r.prev))
            if take < 1:
                raise ValueError(f'image {i}: Importance num_take {take} < 1 (with 0 the reference\'s diff_sorted[-0] is the minimum and its rule '
                                 'silently keeps nearly every pixel: refused)')
            if take > n_pixels:
                raise ValueError(f'image {i}: Importance num_take {take} > the image\'s {n_pixels} pixels')
            if prev == i or not 0 <= prev < n:
                raise ValueError(f'image {i}: Importance prev {prev} must be another image of the set\'s {n}')
            rules.append(Importance(take, prev, None if r.dir_z_below is None else float(r.dir_z_below)))
        else:
            every, offset = r
            rules.append((int(every), int(offset)))
    return rules


current_stream = _lib.stream            # (the name callers outside the package know it by)


def _refuse_rule(rule):
    """Raises for a subsample rule that is not the checkerboard, saying which of the reference's it is when it is one of them."""
    why = UNSUPPORTED_RULES.get(rule) if isinstance(rule, str) else None
    raise NotImplementedError(f'subsample rule {rule!r} is not supported' + (f' ({why})' if why else '')
                              + ': only the checkerboard rule (x + y + offset) % every == 0 is')


def make_ndc(ndc):
    """None | hr_ndc | dict(fx, fy, near, width, height) -> hr_ndc or None."""
    if ndc is None or isinstance(ndc, hr_ndc):
        return ndc
    missing = [k for k in ('fx', 'fy', 'near', 'width', 'height') if k not in ndc]
    if missing or len(ndc) != 5:
        raise ValueError(f'ndc needs exactly fx, fy, near, width, height; got {sorted(ndc)}')
    out = hr_ndc()
    out.fx, out.fy, out.near = float(ndc['fx']), float(ndc['fy']), float(ndc['near'])
    out.width, out.height = int(ndc['width']), int(ndc['height'])
    return out


def make_camera(pose, K, width, height, cam_id=0.0, time=0.0):
    """3x4 camera-to-world `pose`, 3x3 intrinsics `K` -> hr_camera."""
    cam = hr_camera()
    p = np.asarray(pose, np.float32)[:3, :4].reshape(-1)
    for i in range(12):
        cam.c2w[i] = float(p[i])
    Km = np.asarray(K, np.float32)
    cam.fx, cam.fy, cam.cx, cam.cy = float(Km[0, 0]), float(Km[1, 1]), float(Km[0, 2]), float(Km[1, 2])
    cam.width, cam.height = int(width), int(height)
    cam.cam_id, cam.time = float(cam_id), float(time)
    return cam


def make_fisheye(distortion):
    """None | hr_fisheye | (k1, k2) -> hr_fisheye or None: the first two coefficients of a camera's radial distortion, what
    ImmersiveDataset.get_coords passes to cv2.fisheye.undistortPoints as D = (k1, k2, 0, 0) (datasets/immersive.py:43-48).  Longer
    sequences are refused: the reference reads two coefficients and so does the kernel.  (0, 0) means no distortion: the library treats
    it as the pinhole camera, like None (include/hyperreel_hip.h says how that differs from OpenCV's reading of zeros)."""
    if distortion is None or isinstance(distortion, hr_fisheye):
        return distortion
    k = np.asarray(distortion, np.float64).reshape(-1)
    if k.shape != (2,) or not np.isfinite(k).all():
        raise ValueError(f'fisheye distortion needs exactly two finite coefficients (k1, k2); got {distortion!r}')
    out = hr_fisheye()
    out.k1, out.k2 = float(k[0]), float(k[1])
    return out


def make_lightfield(width, height, aspect=None, st_scale=1.0, uv_scale=1.0, near=-1.0, far=0.0):
    """The arguments of get_lightfield_rays / get_epi_rays (utils/ray_utils.py:14-78) besides the position -> hr_lightfield.
    width x height: U x V of a view, U x S of an epipolar slice.  aspect: W / H of the images by default (datasets/stanford.py:66);
    near, far: the planes' z (datasets/lightfield.py:56-57)."""
    lf = hr_lightfield()
    lf.width, lf.height = int(width), int(height)
    lf.aspect = float(width) / float(height) if aspect is None else float(aspect)
    lf.st_scale, lf.uv_scale, lf.near, lf.far = float(st_scale), float(uv_scale), float(near), float(far)
    return lf


def lightfield_coord(s_idx, t_idx, rows, cols):
    """LightfieldDataset.get_coord (datasets/lightfield.py:185-191): grid indices (fractional ones too) -> (s, t) in [-1, 1], t
    pointing up; a grid of one column / row sits at 0."""
    s = (s_idx / (cols - 1)) * 2 - 1 if cols > 1 else 0
    t = -(((t_idx / (rows - 1)) * 2 - 1) if rows > 1 else 0)
    return (s, t)


def stanford_normalize_coord(coord, camera_coords):
    """StanfordLightfieldDataset.normalize_coord (datasets/stanford.py:82-106): a camera position (x, y) read from a file name ->
    (s, t), x over the rig's x range to [-1, 1], y likewise and divided by the rig's aspect.  camera_coords: every camera's (x, y)."""
    xs = [c[0] for c in camera_coords]
    ys = [c[1] for c in camera_coords]
    x_range, y_range = (np.min(xs), np.max(xs)), (np.min(ys), np.max(ys))
    aspect = (x_range[1] - x_range[0]) / (y_range[1] - y_range[0])
    norm_x = ((coord[0] - x_range[0]) / (x_range[1] - x_range[0])) * 2 - 1
    norm_y = (((coord[1] - y_range[0]) / (y_range[1] - y_range[0])) * 2 - 1) / aspect
    return (norm_x, norm_y)


def _as_u8_image(img, i, H, W, channels=3):
    img = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))
    if img.dtype != torch.uint8 or tuple(img.shape) != (H, W, channels):
        raise ValueError(f'image {i}: expected uint8 ({H}, {W}, {channels}), got {img.dtype} {tuple(img.shape)}')
    return img.contiguous()


def _alpha_channels(alpha):
    """alpha=None: 8-bit RGB, 3 bytes a pixel; 'white': 8-bit RGBA composited over white, 4."""
    if alpha is None:
        return 3
    if alpha != 'white':
        raise ValueError(f"alpha must be None (8-bit RGB images) or 'white' (8-bit RGBA images over white, the reference's only background); got {alpha!r}")
    return 4


class DeviceRaySet(HandleOwner):
    """images_u8: (n, H, W, 3) uint8 (numpy, or a torch tensor on the host or the device), RGB as Image.convert("RGB") holds
    them; poses (n, 3, 4); intrinsics (n, 3, 3) or one (3, 3); times, cam_ids: (n) or None (6-column rays); img_wh = (W, H);
    ndc: None | dict(fx, fy, near, width, height) | hr_ndc; alpha: None, or 'white' -- images_u8 is then (n, H, W, 4) uint8, RGBA as
    Image.convert("RGBA") holds them, and a row's rgb is the pixel over white, rgb * a + (1 - a) on bytes / 255, bit for bit what the
    reference's RGBA datasets train on (datasets/blender.py:61-70, donerf.py:240-249); subsample: None (every pixel) or, per image, one (every, offset)
    (DeviceRaySet.video_rule builds the reference's) or one Importance(...) (DeviceRaySet.importance_rule), mixed freely; distortions: None (pinhole cameras) or (n, 2), each image's fisheye (k1, k2)
    (ImmersiveDataset.distortions[idx][:2]).  Element e of the set is row e of the reference's all_inputs."""

    def __init__(self, images_u8, poses, intrinsics, times, cam_ids, img_wh, ndc=None, subsample=None, device=None, distortions=None, alpha=None):
        if isinstance(subsample, str):
            _refuse_rule(subsample)
        self._channels = _alpha_channels(alpha)
        W, H = int(img_wh[0]), int(img_wh[1])
        poses = np.asarray(poses, np.float32)
        n = poses.shape[0]
        rules = _parse_rules(subsample, n, W * H, alpha=alpha)
        Ks = np.asarray(intrinsics, np.float32)
        Ks = np.broadcast_to(Ks, (n, 3, 3)) if Ks.ndim == 2 else Ks
        self.ray_dim = 8 if times is not None else 6
        times = np.zeros(n) if times is None else np.asarray(times, np.float64)
        cam_ids = np.zeros(n) if cam_ids is None else np.asarray(cam_ids, np.float64)
        if distortions is not None:
            distortions = np.asarray(distortions, np.float64)
            if distortions.shape != (n, 2):
                raise ValueError(f'distortions must be None or an ({n}, 2) array of (k1, k2) per image, got shape {distortions.shape}')
            distortions = [make_fisheye(d) for d in distortions]
        self._ndc = make_ndc(ndc)

        def create(handle):
            _lib.call('hr_rayset_create', n, W, H, self.ray_dim, C.byref(self._ndc) if self._ndc is not None else None, handle)

        def set_image(i, every, offset, pixels):
            cam = make_camera(poses[i], Ks[i], W, H, cam_ids[i], times[i])
            if distortions is None:
                _lib.call('hr_rayset_set_image', self._h, i, C.byref(cam), every, offset, pixels)
            else:
                _lib.call('hr_rayset_set_image_fisheye', self._h, i, C.byref(cam), C.byref(distortions[i]), every, offset, pixels)

        def set_importance(i, rule, pixels):
            cam = make_camera(poses[i], Ks[i], W, H, cam_ids[i], times[i])
            _lib.call('hr_rayset_set_image_importance', self._h, i, C.byref(cam), C.byref(distortions[i]) if distortions is not None else None,
                      rule.prev, rule.num_take, float('nan') if rule.dir_z_below is None else rule.dir_z_below, pixels)

        self._fill(images_u8, n, W, H, rules, device, create, set_image, (Ks, times, cam_ids),
                   'images, poses, intrinsics, times, cam_ids and subsample must describe the same number of images', set_importance)

    @classmethod
    def from_lightfield(cls, images_u8, st, lightfield, subsample=None, device=None, alpha=None):
        """A set of two-plane light-field views (hr_rayset_create_lightfield): images_u8 (n, V, U, 3) uint8 as for the constructor
        ((n, V, U, 4) with alpha='white'),
        st: (n, 2) the views' (s, t) -- lightfield_coord or stanford_normalize_coord of each -- in the order the reference's
        prepare_train_data visits them, t outer and s inner (datasets/lightfield.py:106-141); lightfield: make_lightfield(...).
        Element e is row e of that order's concatenated get_lightfield_rays; rays have 6 columns."""
        if isinstance(subsample, str):
            _refuse_rule(subsample)
        if not isinstance(lightfield, hr_lightfield):
            raise TypeError('lightfield must be an hr_lightfield (data.make_lightfield)')
        st = np.asarray(st, np.float64).reshape(-1, 2)
        n = st.shape[0]
        channels = _alpha_channels(alpha)
        rules = _parse_rules(subsample, n, int(lightfield.width) * int(lightfield.height), lightfield=True, alpha=alpha)
        self = cls.__new__(cls)
        self._channels = channels
        self.ray_dim = 6
        self._ndc = None
        self._lightfield = lightfield

        def create(handle):
            _lib.call('hr_rayset_create_lightfield', n, C.byref(lightfield), handle)

        def set_view(i, every, offset, pixels):
            _lib.call('hr_rayset_set_view', self._h, i, float(st[i, 0]), float(st[i, 1]), every, offset, pixels)

        self._fill(images_u8, n, int(lightfield.width), int(lightfield.height), rules, device, create, set_view, (),
                   'images, st and subsample must describe the same number of views')
        return self

    def _fill(self, images_u8, n, W, H, rules, device, create, set_one, per_image, mismatch, set_importance=None):
        """The constructors' shared tail: one rule per image (_parse_rules), every per-image sequence n long (else ValueError(mismatch)),
        the device, the handle -- create(pointer to it) -- then for each image in turn set_one(i, every, offset, pixels), or
        set_importance(i, rule, pixels) under an Importance rule, and the set's size.  The callables check their own C call."""
        if not all(len(seq) == n for seq in (images_u8, rules, *per_image)):
            raise ValueError(mismatch)
        channels = self._channels
        if channels == 4:                      # an RGBA set checks its images before any device work: RGB bytes would be read as RGBA
            images_u8 = [_as_u8_image(images_u8[i], i, H, W, 4) for i in range(n)]
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.width, self.height, self.n_images = W, H, n
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            create(C.byref(self._h))
            if channels == 4:
                _lib.call('hr_rayset_set_pixel_format', self._h, _lib.HR_PIXELS_RGBA8_WHITE)
            for i in range(n):
                img = _as_u8_image(images_u8[i], i, H, W, channels)
                if isinstance(rules[i], Importance):
                    set_importance(i, rules[i], img)
                else:
                    set_one(i, rules[i][0], rules[i][1], img)
        self._size = int(_lib.call('hr_rayset_size', self._h))

    def __len__(self):
        return self._size

    DESTROY = 'hr_rayset_destroy'          # HandleOwner: close(), and a __del__ that survives interpreter teardown

    def batch(self, batch_idx, batch_size, epoch=0, seed=0, indices=None, out=None):
        """Rows [batch_idx * batch_size, + batch_size) of the epoch's order (the last batch of an epoch is short), or the set
        elements `indices` (int64 tensor on the device).  Returns {'coords', 'rgb', 'weight'} -- the keys format_batch yields
        (datasets/base.py:278-284) -- as fresh float32 tensors, or written into `out`'s tensors (fixed buffers for a captured graph)."""
        if indices is not None:
            if indices.dtype != torch.int64 or indices.device != self.device or not indices.is_contiguous():
                raise ValueError('indices must be a contiguous int64 tensor on the set\'s device')
            first, n = 0, indices.numel()
        else:
            first = int(batch_idx) * int(batch_size)
            n = min(int(batch_size), self._size - first)
            if n <= 0:
                raise IndexError(f'batch {batch_idx} of {batch_size} starts beyond the set\'s {self._size} rays')
        out = self._outputs(n, out)
        _lib.call('hr_rayset_batch', self._h, first, n, int(seed), int(epoch), indices, out['coords'], out['rgb'], out['weight'],
                  _lib.stream(self.device), device=self.device)
        return out

    def _outputs(self, n, out):
        """Fresh output tensors of n rows, or the caller's after a shape / dtype / device check."""
        if out is None:
            return {'coords': torch.empty((n, self.ray_dim), dtype=torch.float32, device=self.device),
                    'rgb': torch.empty((n, 3), dtype=torch.float32, device=self.device),
                    'weight': torch.empty((n, 1), dtype=torch.float32, device=self.device)}
        for k, cols in (('coords', self.ray_dim), ('rgb', 3), ('weight', 1)):
            t = out[k]
            if t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous() or tuple(t.shape) != (n, cols):
                raise ValueError(f"out['{k}'] must be a contiguous float32 ({n}, {cols}) tensor on the set's device")
        return out

    @staticmethod
    def check_step_tensor(step_tensor, device):
        """The device word hr_rayset_sample reads its step from: one int64 or uint64 element on `device` (HipAdam's step_tensor is one)."""
        if not isinstance(step_tensor, torch.Tensor):
            raise TypeError('step_tensor must be a torch tensor')
        if step_tensor.dtype not in (torch.int64, torch.uint64):
            raise ValueError(f'step_tensor must be int64 or uint64, got {step_tensor.dtype}')
        if step_tensor.numel() != 1:
            raise ValueError(f'step_tensor must hold one element, got {tuple(step_tensor.shape)}')
        if step_tensor.device != torch.device(device):
            raise ValueError(f"step_tensor is on {step_tensor.device}, the set on {device}")
        return step_tensor

    def sample(self, n, step=0, seed=0, step_tensor=None, out=None, want_elements=False):
        """n rows drawn WITH replacement (hr_rayset_sample): what RandomSampler(replacement=True) feeds the reference's loop under
        `sample_with_replacement: True`, every shipped training config's setting -- uniform and independent over the set, fixed by
        (seed, step, row), not torch's stream.  `step`: this training step's number; or `step_tensor`, a one-element int64 / uint64
        tensor on the set's device that the kernel reads when it runs (HipAdam(capturable=True).step_tensor): a captured call then
        draws a new batch on every replay.  Returns the dict of `batch` (fresh tensors, or `out`'s), plus 'elements' (n int64: the
        set element of each row; taken from out['elements'] when `out` has it) with want_elements."""
        n = int(n)
        if n < 0:
            raise ValueError(f'sample: n = {n}')
        if step_tensor is not None:
            self.check_step_tensor(step_tensor, self.device)
        had_out = out is not None
        out = self._outputs(n, out)
        elements = None
        if want_elements:
            elements = out.get('elements') if had_out else None
            if elements is None:
                elements = torch.empty((n,), dtype=torch.int64, device=self.device)
            elif elements.dtype != torch.int64 or elements.device != self.device or not elements.is_contiguous() or tuple(elements.shape) != (n,):
                raise ValueError(f"out['elements'] must be a contiguous int64 ({n},) tensor on the set's device")
            out = dict(out, elements=elements)
        _lib.call('hr_rayset_sample', self._h, n, int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF, step_tensor,
                  out['coords'], out['rgb'], out['weight'], elements, _lib.stream(self.device), device=self.device)
        return out

    def order(self, first, n, epoch=0, seed=0):
        """The set elements of rows [first, first + n) of the epoch's order: (n) int64 on the device."""
        out = torch.empty((int(n),), dtype=torch.int64, device=self.device)
        _lib.call('hr_rayset_order', self._h, int(first), int(n), int(seed), int(epoch), out, _lib.stream(self.device), device=self.device)
        return out

    def kept_pixels(self, i):
        """The row-major pixel indices y * W + x of image i's rays in the set, in set order: (count) int32 on the device."""
        n = self.image_info(i)['count']
        out = torch.empty((n,), dtype=torch.int32, device=self.device)
        _lib.call('hr_rayset_image_pixels', self._h, int(i), 0, n, out, _lib.stream(self.device), device=self.device)
        return out

    def image_info(self, i):
        """hr_rayset_image_info of image i as a dict: count, num_take, every, offset, is_list, prev, threshold, dir_z_below (None: no test)."""
        info = _lib.hr_rayset_image_info()
        _lib.call('hr_rayset_image_info', self._h, int(i), C.byref(info))
        d = {k: getattr(info, k) for k, _ in info._fields_}
        d['is_list'] = bool(d['is_list'])
        d['dir_z_below'] = None if np.isnan(d['dir_z_below']) else d['dir_z_below']
        return d

    @staticmethod
    def importance_rule(frames, n_pixels, load_full_step, subsample_keyframe_step, subsample_keyframe_frac, subsample_frac, first_of_video,
                        dir_z_below=-0.05):
        """Immersive's rule over images in its load order, video-major (prepare_train_data, datasets/immersive.py:330-389): `frames` holds
        each image's frame number, `first_of_video` whether it is the first loaded frame of its video.  Such a frame, and one divisible by
        load_full_step, keeps every pixel: (1, 0).  Any other compares with the image before it: Importance(round(n_pixels * frac), i - 1,
        dir_z_below), frac = subsample_keyframe_frac for a frame divisible by subsample_keyframe_step, else subsample_frac
        (importance_subsample, immersive.py:295-310).  dir_z_below=None: Neural 3D's variant without the direction test
        (datasets/neural_3d.py:191-204).  Returns the list DeviceRaySet(subsample=) takes."""
        frames = [int(f) for f in frames]
        first = [bool(f) for f in first_of_video]
        if len(first) != len(frames):
            raise ValueError('frames and first_of_video must describe the same images')
        out = []
        for i, f in enumerate(frames):
            if first[i] or f % load_full_step == 0:
                out.append((1, 0))
            else:
                frac = subsample_keyframe_frac if f % subsample_keyframe_step == 0 else subsample_frac
                out.append(Importance(int(np.round(n_pixels * frac)), i - 1, dir_z_below))
        return out

    @staticmethod
    def video_rule(frame, load_full_step=1, subsample_keyframe_step=1, subsample_keyframe_frac=1.0, subsample_frac=1.0,
                   keyframe_offset=0, frame_offset=0, rule='regular_subsample'):
        """The reference's checkerboard rule over images in load order (datasets/technicolor.py:211-236,
        datasets/neural_3d.py:168-185): `frame` holds each image's frame number; a frame divisible by load_full_step keeps every
        pixel, one divisible by subsample_keyframe_step keeps every round(1 / subsample_keyframe_frac)-th with the running
        keyframe_offset, any other every round(1 / subsample_frac)-th with the running frame_offset.  The counters start at the
        given values (Neural 3D resets both to the video's index per video, neural_3d.py:225-226).  Returns [(every, offset)]."""
        if rule != 'regular_subsample':
            _refuse_rule(rule)
        frames = [int(frame)] if np.isscalar(frame) else [int(f) for f in frame]
        out = []
        for f in frames:
            if f % load_full_step == 0:
                out.append((1, 0))
            elif f % subsample_keyframe_step == 0:
                out.append((int(np.round(1.0 / subsample_keyframe_frac)), keyframe_offset))
                keyframe_offset += 1
            else:
                out.append((int(np.round(1.0 / subsample_frac)), frame_offset))
                frame_offset += 1
        return out


# ---- the resize in front of the set (hr_image_resize) --------------------------------------------------------------------
# filter names -> PIL's Image.Resampling numbers, which the C ABI takes
RESIZE_FILTERS = {'lanczos': 1, 'bilinear': 2, 'bicubic': 3, 'box': 4}


def _resize_filter(name):
    if name not in RESIZE_FILTERS:
        raise ValueError(f'resize filter {name!r} is not one of {sorted(RESIZE_FILTERS)} (PIL\'s NEAREST and HAMMING are not provided)')
    return RESIZE_FILTERS[name]


def _resize_wh(wh, what):
    try:
        w, h = wh
        ok = int(w) == w and int(h) == h and int(w) >= 1 and int(h) >= 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f'{what} must be (width, height), two integers of at least 1; got {wh!r}')
    return int(w), int(h)


RESIZE_MODES = {'RGB': 3, 'RGBA': 4}          # PIL's mode names -> bytes of a pixel


def _resize_mode(mode):
    if mode not in RESIZE_MODES:
        raise ValueError(f'resize mode {mode!r} is not one of {sorted(RESIZE_MODES)} (PIL\'s other modes, LA among them, are not provided)')
    return RESIZE_MODES[mode]


def _as_u8_batch(images_u8, wh=None, channels=3):
    """(n, H, W, 3) or (H, W, 3) uint8 as numpy, a host tensor or a device tensor -> a contiguous (n, H, W, 3) tensor where it lives
    (channels=4: the same of RGBA images)"""
    if not isinstance(images_u8, torch.Tensor):
        a = np.ascontiguousarray(images_u8)
        images_u8 = torch.from_numpy(a if a.flags.writeable else a.copy())        # (torch refuses to wrap a read-only array silently)
    t = images_u8
    if t.ndim == 3:
        t = t[None]
    if t.dtype != torch.uint8 or t.ndim != 4 or t.shape[-1] != channels or t.shape[0] < 1:
        raise ValueError(f'images must be uint8 (n, H, W, {channels}) or (H, W, {channels}), 8-bit {"RGBA" if channels == 4 else "RGB"}; '
                         f'got {t.dtype} {tuple(t.shape)}')
    if wh is not None and (t.shape[2], t.shape[1]) != tuple(wh):
        raise ValueError(f'images are {t.shape[2]} x {t.shape[1]} (W x H), the resize was made for {wh[0]} x {wh[1]}')
    return t.contiguous()


class DeviceResize(HandleOwner):
    """PIL's Image.resize of 8-bit RGB images -- or, with mode='RGBA', of 8-bit RGBA images, (.., 4) wherever (.., 3) stands below:
    PIL resamples them premultiplied and converts back -- on the device, byte for byte: src_wh = (W, H) -> dst_wh = (W2, H2) with filter 'lanczos' |
    'bicubic' | 'bilinear' | 'box' (Image.LANCZOS, BICUBIC -- Image.resize's default -- BILINEAR, BOX), up to max_images images a launch.
    Calling it with images_u8 takes (n, H, W, 3) or (H, W, 3) uint8 as numpy, a host tensor or a device tensor and returns a device uint8 tensor
    (n, H2, W2, 3), which DeviceRaySet accepts as images_u8; it runs on torch's current stream, and more than max_images images go in
    chunks.  The plan (coefficients computed on the host, the 8-bit image between the horizontal and the vertical pass) lives until
    close().  No CPU path: a missing library or a failing call raises.

    Out of scope: cv2.resize, which datasets/immersive.py:579, neural_3d.py:416 and donerf.py:242 call (another arithmetic, and two of
    those calls pass the filter where cv2 takes dst); decoding image files (load_images below: hyperreel_amd.png.load_png, hyperreel_amd.jpeg.load_jpeg); modes other than 8-bit RGB and RGBA (LA among them);
    Image.resize's box= and reducing_gap=."""

    def __init__(self, src_wh, dst_wh, filter='lanczos', max_images=1, device=None, mode='RGB'):
        self.mode, self._channels = mode, _resize_mode(mode)
        self.src_wh, self.dst_wh = _resize_wh(src_wh, 'src_wh'), _resize_wh(dst_wh, 'dst_wh')
        self.filter = filter
        number = _resize_filter(filter)
        self.max_images = int(max_images)
        if self.max_images < 1:
            raise ValueError(f'max_images {max_images} < 1')
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self._h = C.c_void_p()
        _lib.call('hr_resize_plan_create_rgba' if self._channels == 4 else 'hr_resize_plan_create', self.src_wh[0], self.src_wh[1], self.dst_wh[0], self.dst_wh[1], number, self.max_images,
                  C.byref(self._h), device=self.device)

    DESTROY = 'hr_resize_plan_destroy'          # HandleOwner: close(), and a __del__ that survives interpreter teardown

    def __call__(self, images_u8, out=None):
        """out: None (a fresh tensor) or a contiguous uint8 (n, H2, W2, 3) tensor on the plan's device (a fixed buffer for a captured graph)"""
        if not getattr(self, '_h', None):
            raise RuntimeError('DeviceResize is closed')
        ch = self._channels
        src = _as_u8_batch(images_u8, self.src_wh, ch).to(self.device)
        n, (W2, H2) = src.shape[0], self.dst_wh
        if out is None:
            out = torch.empty((n, H2, W2, ch), dtype=torch.uint8, device=self.device)
        elif out.dtype != torch.uint8 or out.device != self.device or not out.is_contiguous() or tuple(out.shape) != (n, H2, W2, ch):
            raise ValueError(f'out must be a contiguous uint8 ({n}, {H2}, {W2}, {ch}) tensor on {self.device}')
        per_src, per_dst = src.shape[1] * src.shape[2] * ch, H2 * W2 * ch
        with torch.cuda.device(self.device):
            for first in range(0, n, self.max_images):
                _lib.call('hr_image_resize', self._h, C.c_void_p(src.data_ptr() + first * per_src), min(self.max_images, n - first),
                          C.c_void_p(out.data_ptr() + first * per_dst), _lib.stream(self.device))
        return out


def reference_resize(images_u8, _img_wh, img_wh=None, first='lanczos', device=None, mode='RGB'):
    """get_rgb's two steps (datasets/llff.py:145-163): img.resize(_img_wh, Image.LANCZOS), then img.resize(img_wh, Image.BOX) when
    img_wh differs from _img_wh.  A step at equal size is no operation (Image.resize returns a copy).  first='bicubic' is
    datasets/catacaustics.py:298, whose img.resize(wh) takes PIL's default.  images_u8 as for DeviceResize; returns a device uint8
    tensor (n, H, W, 3) of the last size.  mode='RGBA': (.., 4) images as Image.convert('RGBA') holds them (datasets/blender.py:61-70,
    donerf.py:240-249); each step is then a full RGBA resize, the image between the two un-premultiplied 8-bit RGBA.  Out of scope: see
    DeviceResize."""
    channels = _resize_mode(mode)
    wh1 = _resize_wh(_img_wh, '_img_wh')
    wh2 = wh1 if img_wh is None else _resize_wh(img_wh, 'img_wh')
    _resize_filter(first)
    x = _as_u8_batch(images_u8, channels=channels)
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    for wh, name in ((wh1, first), (wh2, 'box')):
        if (x.shape[2], x.shape[1]) != wh:
            step = DeviceResize((x.shape[2], x.shape[1]), wh, name, max_images=min(x.shape[0], 8), device=device, mode=mode)
            try:
                x = step(x)
            finally:
                torch.cuda.current_stream(device).synchronize()      # the plan's memory goes with it
                step.close()
    return x.to(device)


def load_images(paths, mode='RGB', device=None):
    """uint8 (n, H, W, C) on the device from image files of one format, PNG or JPEG, told by each file's first bytes (a directory such
    as LLFF's images/ may hold either): png.load_png or jpeg.load_jpeg.  A list that mixes the two is refused, naming the first file
    that differs; so is a file that is neither."""
    from . import jpeg, png
    paths = list(paths)
    if not paths:
        raise ValueError('load_images: no paths')
    kinds = []
    for p in paths:
        with open(p, 'rb') as f:
            head = f.read(8)
        kind = 'PNG' if head == b'\x89PNG\r\n\x1a\n' else 'JPEG' if head[:2] == b'\xff\xd8' else None
        if kind is None:
            raise ValueError(f'{p}: neither a PNG signature nor a JPEG SOI marker')
        if kinds and kind != kinds[0]:
            raise ValueError(f'{p} is a {kind} file, {paths[0]} a {kinds[0]} file: load_images takes one format a call')
        kinds.append(kind)
    return (png.load_png if kinds[0] == 'PNG' else jpeg.load_jpeg)(paths, mode, device)


def as_float(images_u8_dev):
    """(n, H, W, 3) uint8 -> (n * H * W, 3) float32, x / 255: ToTensor followed by view(3, -1).permute(1, 0), the ground truth get_rgb
    hands model.evaluate.  A plain torch op: no kernel of the library is involved."""
    if images_u8_dev.dtype != torch.uint8 or images_u8_dev.shape[-1] != 3:
        raise ValueError(f'as_float takes uint8 (..., 3) images, got {images_u8_dev.dtype} {tuple(images_u8_dev.shape)}')
    return images_u8_dev.reshape(-1, 3).float().div(255)


def composite_white(images_rgba_u8_dev):
    """(n, H, W, 4) uint8 RGBA -> (n * H * W, 3) float32 over white: ToTensor, view(4, -1).permute(1, 0), then
    img[:, :3] * img[:, -1:] + (1 - img[:, -1:]) (datasets/blender.py:61-70), as_float's counterpart for an RGBA dataset: the ground
    truth get_rgb hands model.evaluate, and bit for bit the rgb a DeviceRaySet(alpha='white') row holds.  Plain torch ops, each one
    float32 rounding and the division a true one: no kernel of the library is involved."""
    if images_rgba_u8_dev.dtype != torch.uint8 or images_rgba_u8_dev.shape[-1] != 4:
        raise ValueError(f'composite_white takes uint8 (..., 4) images, got {images_rgba_u8_dev.dtype} {tuple(images_rgba_u8_dev.shape)}')
    # a device tensor as the divisor: torch's device kernels divide by a host scalar as a multiplication by 1 / 255, which differs on 126 bytes
    x = images_rgba_u8_dev.reshape(-1, 4).float() / torch.full((), 255.0, dtype=torch.float32, device=images_rgba_u8_dev.device)
    a = x[:, 3:]
    prod = x[:, :3] * a
    return prod + (1 - a)
