"""LPIPS on the device: the third score of a results table, next to metrics.py's PSNR and SSIM (hr_lpips).

Replaces the reference's host-side scoring (metrics.py:54-58 compute_lpips: images * 2 - 1, `.cpu()`, lpips_model.forward;
utils/tensorf_utils.py:76-88 rgb_lpips: nets 'alex' and 'vgg', version '0.1', normalize=True).  The definition -- LPIPS v0.1 in eval
mode -- is stated once in csrc/hr_lpips.h.

The pretrained weights are the caller's: torchvision's backbone state dict and the lpips package's lin layers.  None are shipped.

    model = Lpips.from_files('alexnet.pth', 'alex_lin.pth', net='alex')
    t = model.lpips_scores(rgb, gt, h, w)        # 6 doubles on the device: layer[0..4], total; nothing synchronises
    d = float(t[5])                              # the one `.cpu()`

There is no CPU path: tensors that are not on the HIP device raise.
"""
import ctypes as C
import math

import torch

from . import lib as _lib
from ._codec import HandleOwner

NETS = {'alex': _lib.HR_LPIPS_ALEX, 'vgg': _lib.HR_LPIPS_VGG}
# (cin, cout, kernel) of every convolution, in order, and its index in torchvision's `features`; csrc/hr_lpips.h is the table the kernels run
CONVS = {
    'alex': [(3, 64, 11), (64, 192, 5), (192, 384, 3), (384, 256, 3), (256, 256, 3)],
    'vgg': [(3, 64, 3), (64, 64, 3), (64, 128, 3), (128, 128, 3), (128, 256, 3), (256, 256, 3), (256, 256, 3), (256, 512, 3), (512, 512, 3), (512, 512, 3),
            (512, 512, 3), (512, 512, 3), (512, 512, 3)],
}
FEATURE_INDEX = {'alex': [0, 3, 6, 8, 10], 'vgg': [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]}
TAP_CHANNELS = {'alex': [64, 192, 384, 256, 256], 'vgg': [64, 128, 256, 512, 512]}
MIN_SIZE = {'alex': 31, 'vgg': 16}


def _net(net):
    if net not in NETS:
        raise ValueError(f'net {net!r}: one of {sorted(NETS)}')
    return net


def backbone_keys(net):
    """[(weight key, bias key, weight shape)] of the backbone state dict: torchvision's features.N.weight|bias"""
    return [(f'features.{n}.weight', f'features.{n}.bias', (cout, cin, k, k)) for n, (cin, cout, k) in zip(FEATURE_INDEX[_net(net)], CONVS[net])]


def lin_keys(net):
    """[(key, shape)] of the lin state dict: the lpips package's lin{k}.model.1.weight, a 1x1 convolution without bias"""
    return [(f'lin{k}.model.1.weight', (1, c, 1, 1)) for k, c in enumerate(TAP_CHANNELS[_net(net)])]


def _take(sd, key, shape, what):
    if key not in sd:
        raise KeyError(f'{what} state dict has no {key!r}')
    t = sd[key]
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
        raise ValueError(f'{what} state dict: {key!r} must be a tensor of shape {tuple(shape)}, got {tuple(getattr(t, "shape", ()))}')
    return t.detach()


def synthetic_weights(net, seed=0):
    """(backbone_state_dict, lin_state_dict) of the real shapes with seeded values on the CPU: He-scaled convolutions (normal, variance
    2 / fan_in), a small positive bias (uniform in [0, 0.1]) and lin uniform in [0, 1].  What the tests, tools/lpips_ab.py and a smoke
    run score with -- the numbers mean nothing as a perceptual distance."""
    g = torch.Generator().manual_seed(int(seed))
    backbone, lin = {}, {}
    for wk, bk, shape in backbone_keys(net):
        fan_in = shape[1] * shape[2] * shape[3]
        backbone[wk] = torch.randn(shape, generator=g, dtype=torch.float32) * math.sqrt(2.0 / fan_in)
        backbone[bk] = torch.rand((shape[0],), generator=g, dtype=torch.float32) * 0.1
    for key, shape in lin_keys(net):
        lin[key] = torch.rand(shape, generator=g, dtype=torch.float32)
    return backbone, lin


def workspace_doubles(net, h, w):
    """Length of the float64 workspace tensor a call on an h x w frame needs."""
    return (int(_lib.call('hr_lpips_workspace', NETS[_net(net)], int(h), int(w))) + 7) // 8


class Lpips(HandleOwner):
    """An LPIPS scorer on one device: the backbone's and the lin layers' weights, packed for the convolution kernels (hr_lpips_create).
    backbone_state_dict: torchvision's alexnet / vgg16 state dict (features.N.weight|bias; other keys are ignored); lin_state_dict: the
    lpips package's (lin{k}.model.1.weight).  A missing key or a wrong shape raises and names it."""
    DESTROY = 'hr_lpips_destroy'

    def __init__(self, net, backbone_state_dict, lin_state_dict, device=None):
        self.net = _net(net)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('Lpips lives on the HIP device; there is no CPU path')
        weights, biases, lins = [], [], []
        for wk, bk, shape in backbone_keys(self.net):
            weights.append(_take(backbone_state_dict, wk, shape, 'backbone'))
            biases.append(_take(backbone_state_dict, bk, shape[:1], 'backbone'))
        for key, shape in lin_keys(self.net):
            lins.append(_take(lin_state_dict, key, shape, 'lin'))
        keep = [[t.to(device=self.device, dtype=torch.float32).contiguous() for t in group] for group in (weights, biases, lins)]
        arrays = [(C.c_void_p * len(group))(*[t.data_ptr() for t in group]) for group in keep]
        self._h = C.c_void_p()
        _lib.call('hr_lpips_create', NETS[self.net], *arrays, C.byref(self._h), device=self.device)

    @classmethod
    def from_files(cls, backbone_path, lin_path, net=None, device=None):
        """The two files a user saves from their own installs: torch.save(torchvision.models.alexnet(weights=...)
        .state_dict(), backbone_path) and the lpips package's weights/v0.1/{alex,vgg}.pth.  net: 'alex' or 'vgg'; None reads it off the
        lin file's first layer (192 channels in lin1: alex; 128: vgg)."""
        backbone = torch.load(backbone_path, map_location='cpu', weights_only=True)
        lin = torch.load(lin_path, map_location='cpu', weights_only=True)
        if net is None:
            probe = lin.get('lin1.model.1.weight')
            if probe is None:
                raise KeyError("lin state dict has no 'lin1.model.1.weight'")
            net = {192: 'alex', 128: 'vgg'}.get(int(probe.shape[1]))
            if net is None:
                raise ValueError(f"lin state dict: 'lin1.model.1.weight' has {int(probe.shape[1])} channels, neither alex's 192 nor vgg's 128")
        return cls(net, backbone, lin, device=device)

    def _check_image(self, name, t, h, w):
        if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
            raise RuntimeError(f'{name} must be a tensor on the HIP device; there is no CPU path')
        if t.device != self.device:
            raise ValueError(f'{name} is on {t.device}, the Lpips object on {self.device}')
        if t.numel() != h * w * 3:
            raise ValueError(f'{name} must hold h * w * 3 = {h * w * 3} values, got {tuple(t.shape)}')
        return t.contiguous().float()

    def lpips_scores(self, pred, gt, h, w, out=None, workspace=None):
        """pred, gt: (h*w, 3) float32 in [0, 1] on the HIP device (what render() returns) -> float64 device tensor [layer0 .. layer4, total]
        (hr_lpips_scores), enqueued on the current stream without a synchronisation.  out: an existing (6,) float64 device tensor;
        workspace: an existing float64 device tensor of at least workspace_doubles(net, h, w) elements (a captured graph's fixed buffers).
        The distance of a frame is not the sum over its tiles -- receptive fields cross the cuts -- so on image-parallel ranks score the
        gathered frame on one rank."""
        h, w = int(h), int(w)
        if not self._h:
            raise RuntimeError('the Lpips object is closed')
        pred = self._check_image('pred', pred, h, w)
        gt = self._check_image('gt', gt, h, w)
        dev = self.device
        if out is None:
            out = torch.empty((6,), dtype=torch.float64, device=dev)
        elif out.shape != (6,) or out.dtype != torch.float64 or out.device != dev or not out.is_contiguous():
            raise ValueError('out must be a contiguous (6,) float64 tensor on the images\' device')
        need = workspace_doubles(self.net, h, w)
        if need == 0:
            raise ValueError(f'{self.net} needs a frame of at least {MIN_SIZE[self.net]} x {MIN_SIZE[self.net]} pixels (and 2 * h * w below 2^31), got {h} x {w}')
        if workspace is None:
            workspace = torch.empty((need,), dtype=torch.float64, device=dev)
        elif workspace.dtype != torch.float64 or workspace.device != dev or not workspace.is_contiguous() or workspace.numel() < need:
            raise ValueError(f'workspace must be a contiguous float64 tensor of at least {need} elements on the images\' device')
        _lib.call('hr_lpips', self._h, pred, gt, h, w, out, workspace, _lib.stream(dev), device=dev)
        return out
