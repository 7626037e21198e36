"""Test oracle of the image scores (hr_image_metrics): scikit-image's structural_similarity(win_size=11, gaussian_weights=True,
multichannel=True, data_range=1.0) and peak_signal_noise_ratio(data_range=1.0), restated with scipy.ndimage.gaussian_filter
(scikit-image is not a dependency).  Lives in the test tree: the product never imports it.

dtype=np.float64 is the oracle; dtype=np.float32 is the same formula with float32 images and filter outputs, the yardstick the device's
distance from the oracle is held against (tests/test_gpu_metrics.py)."""
import numpy as np
from scipy.ndimage import gaussian_filter

SIGMA, TRUNCATE, RADIUS = 1.5, 3.5, 5
assert int(TRUNCATE * SIGMA + 0.5) == RADIUS


def ssim_map(pred, gt, h, w, dtype=np.float64):
    """S of every pixel and channel, (h, w, 3) in `dtype`; pred, gt: (h*w, 3)."""
    x = np.asarray(pred, dtype).reshape(h, w, 3)
    y = np.asarray(gt, dtype).reshape(h, w, 3)

    def f(a):
        return gaussian_filter(a, sigma=(SIGMA, SIGMA, 0), truncate=TRUNCATE, mode='reflect')      # scikit-image's border mode; cropped away

    ux, uy, uxx, uyy, uxy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy            # population covariance (gaussian_weights=True: cov_norm = 1)
    c1, c2 = dtype(0.01 ** 2), dtype(0.03 ** 2)
    return ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))


def scores(pred, gt, h, w, dtype=np.float64, ssim=True):
    """{'sse', 'ssim_sum' (3,), 'mse', 'psnr', 'ssim'}: sums accumulated in float64 whatever `dtype` the maps are computed in."""
    x = np.asarray(pred, dtype).reshape(-1)
    y = np.asarray(gt, dtype).reshape(-1)
    d = x - y
    sse = float(np.sum((d * d).astype(np.float64)))
    out = {'sse': sse, 'mse': sse / (3.0 * h * w), 'psnr': np.inf if sse == 0.0 else -10.0 * np.log10(sse / (3.0 * h * w))}
    if ssim:
        S = ssim_map(pred, gt, h, w, dtype)[RADIUS:h - RADIUS, RADIUS:w - RADIUS].astype(np.float64)
        out['ssim_sum'] = S.sum(axis=(0, 1))
        out['ssim'] = float(out['ssim_sum'].sum() / (3.0 * (h - 2 * RADIUS) * (w - 2 * RADIUS)))
    return out
