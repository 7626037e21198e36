"""Image scores on the device: MSE / PSNR / SSIM of a rendered frame against its ground truth (hr_image_metrics).

Replaces the reference's host-side scoring of every validation image (nlf/__init__.py:976-980, metrics.py:25-35: scikit-image's
peak_signal_noise_ratio(data_range=1.0) and structural_similarity(win_size=11, gaussian_weights=True, multichannel=True,
data_range=1.0) after `.cpu().numpy()`) and its per-step psnr_gpu (metrics.py:37-45, nlf/__init__.py:668).

    t = image_scores(rgb, gt, h, w)          # 4 doubles on the device, nothing synchronises
    m = scores_to_metrics(t, h, w)           # {'mse', 'psnr', 'ssim'} as Python floats: the one `.cpu()`

There is no CPU path: tensors that are not on the HIP device raise.
"""
import math

import torch

from . import lib as _lib

SSIM_RADIUS = 5          # the 11-tap Gaussian window; scores are means over the pixels at least this far from every border


def workspace_doubles(h, w):
    """Length of the float64 workspace tensor a call on an h x w frame needs."""
    return max(int(_lib.call('hr_image_metrics_workspace', int(h), int(w))) // 8, 1)


def _check_image(name, t, h, w, device=None):
    if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
        raise RuntimeError(f'{name} must be a tensor on the HIP device; there is no CPU path')
    if device is not None and t.device != device:
        raise ValueError(f'{name} is on {t.device}, pred on {device}')
    if t.numel() != h * w * 3:
        raise ValueError(f'{name} must hold h * w * 3 = {h * w * 3} values, got {tuple(t.shape)}')
    return t.contiguous().float()


def image_scores(pred, gt, h, w, ssim=True, out=None, workspace=None):
    """pred, gt: (h*w, 3) float32 on the HIP device (what render() returns) -> float64 device tensor
    [sse, ssim_sum_r, ssim_sum_g, ssim_sum_b] (hr_image_scores), enqueued on the current stream without a synchronisation.
    ssim=False: the squared-error sum alone (any h, w >= 1; the SSIM sums are 0).  out: an existing (4,) float64 device tensor;
    workspace: an existing float64 device tensor of at least workspace_doubles(h, w) elements (a captured graph's fixed buffers)."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f'bad image shape {h} x {w}')
    pred = _check_image('pred', pred, h, w)
    gt = _check_image('gt', gt, h, w, pred.device)
    dev = pred.device
    if out is None:
        out = torch.empty((4,), dtype=torch.float64, device=dev)
    elif out.shape != (4,) or out.dtype != torch.float64 or out.device != dev or not out.is_contiguous():
        raise ValueError('out must be a contiguous (4,) float64 tensor on the images\' device')
    need = workspace_doubles(h, w)
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.float64, device=dev)
    elif workspace.dtype != torch.float64 or workspace.device != dev or not workspace.is_contiguous() or workspace.numel() < need:
        raise ValueError(f'workspace must be a contiguous float64 tensor of at least {need} elements on the images\' device')
    _lib.call('hr_image_metrics', pred, gt, h, w, int(bool(ssim)), out, workspace, _lib.stream(dev), device=dev)
    return out


def scores_to_metrics(t, h, w):
    """The four sums of image_scores (a tensor, or any 4 numbers) -> {'mse', 'psnr', 'ssim'} as Python floats.  psnr is inf for an
    exact match; ssim is nan where it was not computed (ssim=False leaves its sums at 0) or the frame is smaller than the window."""
    sse, s0, s1, s2 = (float(v) for v in (t.detach().cpu().tolist() if isinstance(t, torch.Tensor) else t))
    h, w = int(h), int(w)
    mse = sse / (3.0 * h * w)
    psnr = math.inf if sse == 0.0 else -10.0 * math.log10(mse)
    n = (h - 2 * SSIM_RADIUS) * (w - 2 * SSIM_RADIUS)
    s = s0 + s1 + s2
    ssim = s / (3.0 * n) if (h > 2 * SSIM_RADIUS and w > 2 * SSIM_RADIUS and s != 0.0) else math.nan
    return {'mse': mse, 'psnr': psnr, 'ssim': ssim}
