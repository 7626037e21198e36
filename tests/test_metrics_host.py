"""Image scores without a GPU: hr_image_scores (include/hyperreel_hip.h) against its ctypes mirror, the bound entry points, the test
oracle (tests/metrics_oracle.py) against closed forms -- so that it is not only compared with code written to match it -- and the host
arithmetic of hyperreel_amd.metrics.scores_to_metrics."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import metrics_oracle as MO
from helpers import build_host_lib
from hyperreel_amd import lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'c_abi', 'metrics_layout.c')
OUT = os.path.join(HERE, 'c_abi', '_build', 'libhr_metrics_layout.so')
C1, C2 = 0.01 ** 2, 0.03 ** 2


@pytest.fixture(scope='module')
def ml():
    build_host_lib(OUT, SRC, [SRC, os.path.join(HERE, '..', 'include', 'hyperreel_hip.h')])
    m = C.CDLL(OUT)
    m.hs_scores_offset.argtypes = [C.c_int]
    return m


def test_hr_image_scores_layout_matches_c(ml):
    assert ml.hs_scores_sizeof() == C.sizeof(lib.hr_image_scores) == 32
    assert [n for n, _ in lib.hr_image_scores._fields_] == ['sse', 'ssim_sum']
    assert ml.hs_scores_offset(0) == lib.hr_image_scores.sse.offset == 0
    assert ml.hs_scores_offset(1) == lib.hr_image_scores.ssim_sum.offset == 8
    assert ml.hs_ssim_channels() == 3


def test_metrics_entry_points_are_bound_at_abi_27(ml):
    assert lib.ABI_VERSION == 27 == ml.hs_abi_version()
    bound = {name: (res, args) for name, res, args in lib.SYMBOLS}
    assert bound['hr_image_metrics_workspace'] == (C.c_size_t, [C.c_int32, C.c_int32])
    assert bound['hr_image_metrics'] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p])


def test_library_exports_the_metrics_and_sizes_their_workspace():
    """No GPU: the workspace size is host arithmetic, and the argument checks come before any launch."""
    L = lib.load()
    assert L.hr_image_metrics_workspace(0, 5) == 0 and L.hr_image_metrics_workspace(5, -1) == 0
    for h, w in ((1, 1), (3, 5), (11, 11), (47, 61), (800, 800), (1014, 1352), (1088, 2048), (11, 4096), (4096, 11)):
        tiles = -(-w // 32) * -(-h // 16)                       # one slot of four doubles per workgroup, whichever kernel runs
        blocks = -(-(3 * h * w) // 4096)
        assert L.hr_image_metrics_workspace(h, w) == 32 * max(tiles, blocks), (h, w)
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    assert L.hr_image_metrics(p, p, 10, 64, 1, p, p, None) == -1 and b'11 x 11' in L.hr_last_error()
    assert L.hr_image_metrics(p, p, 64, 10, 1, p, p, None) == -1
    assert L.hr_image_metrics(p, p, 0, 64, 0, p, p, None) == -1 and b'shape' in L.hr_last_error()
    assert L.hr_image_metrics(None, p, 16, 16, 0, p, p, None) == -1 and b'null' in L.hr_last_error()
    assert L.hr_image_metrics(p, p, 16, 16, 0, p, None, None) == -1


def test_python_surface_refuses_cpu_tensors():
    import torch
    from hyperreel_amd import metrics
    x = torch.zeros((16 * 16, 3))
    with pytest.raises(RuntimeError, match='no CPU path'):
        metrics.image_scores(x, x, 16, 16)


# ---- the oracle against closed forms
def test_oracle_constant_images():
    h, w = 23, 31
    for a, b in ((0.25, 0.75), (1.0, 0.0), (0.6, 0.6), (0.0, 0.0)):
        x, y = np.full((h * w, 3), a, np.float32), np.full((h * w, 3), b, np.float32)
        s = MO.scores(x, y, h, w)
        a64, b64 = float(np.float32(a)), float(np.float32(b))
        assert s['mse'] == pytest.approx((a64 - b64) ** 2, rel=1e-13, abs=0)
        # variances and the covariance vanish: S = (2ab + C1) / (a^2 + b^2 + C1)
        assert s['ssim'] == pytest.approx((2 * a64 * b64 + C1) / (a64 ** 2 + b64 ** 2 + C1), rel=1e-9)
        assert s['psnr'] == (np.inf if a == b else pytest.approx(-10 * math.log10((a64 - b64) ** 2), rel=1e-12))


def test_oracle_identical_images_score_one():
    h, w = 40, 33
    x = np.random.default_rng(5).random((h * w, 3)).astype(np.float32)
    s = MO.scores(x, x.copy(), h, w)
    assert s['sse'] == 0.0 and s['psnr'] == np.inf
    assert abs(s['ssim'] - 1.0) <= 1e-12
    assert np.allclose(s['ssim_sum'], (h - 10) * (w - 10), rtol=1e-12)


def test_oracle_one_interior_pixel_against_the_weights_multiplied_out():
    """11 x 11: the crop leaves the centre pixel, whose window is the whole image -- no border handling takes part."""
    rng = np.random.default_rng(11)
    x, y = rng.random((121, 3)).astype(np.float32), rng.random((121, 3)).astype(np.float32)
    k = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-k * k / (2 * 1.5 ** 2))
    g /= g.sum()
    W = np.outer(g, g)                                         # separable: the 2-D window is the outer product
    assert abs(W.sum() - 1.0) < 1e-15
    s = MO.scores(x, y, 11, 11)
    for c in range(3):
        X, Y = x[:, c].astype(np.float64).reshape(11, 11), y[:, c].astype(np.float64).reshape(11, 11)
        ux, uy = (W * X).sum(), (W * Y).sum()
        vx, vy, vxy = (W * X * X).sum() - ux * ux, (W * Y * Y).sum() - uy * uy, (W * X * Y).sum() - ux * uy
        S = (2 * ux * uy + C1) * (2 * vxy + C2) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        assert s['ssim_sum'][c] == pytest.approx(S, rel=1e-11), c
    assert s['sse'] == pytest.approx(((x.astype(np.float64) - y) ** 2).sum(), rel=1e-13)


def test_oracle_float32_yardstick_is_close_but_not_equal():
    """The float32 evaluation the device is measured against really is a float32 evaluation."""
    h, w = 47, 61
    rng = np.random.default_rng(3)
    y = rng.random((h * w, 3)).astype(np.float32)
    x = np.clip(y + rng.normal(0, 0.02, y.shape), 0, 1).astype(np.float32)
    s64, s32 = MO.scores(x, y, h, w), MO.scores(x, y, h, w, dtype=np.float32)
    assert MO.ssim_map(x, y, h, w, np.float32).dtype == np.float32
    assert 0 < abs(s64['ssim'] - s32['ssim']) < 1e-5
    assert s32['sse'] == pytest.approx(s64['sse'], rel=1e-6)


# ---- scores_to_metrics
def test_scores_to_metrics_arithmetic():
    import torch
    from hyperreel_amd.metrics import scores_to_metrics
    h, w = 20, 30
    n = (h - 10) * (w - 10)
    m = scores_to_metrics([1.8, 0.9 * n, 0.8 * n, 0.7 * n], h, w)
    assert m['mse'] == pytest.approx(1.8 / (3 * h * w), rel=1e-15)
    assert m['psnr'] == pytest.approx(-10 * math.log10(1.8 / (3 * h * w)), rel=1e-15)
    assert m['ssim'] == pytest.approx(0.8, rel=1e-14)
    assert set(m) == {'mse', 'psnr', 'ssim'} and all(type(v) is float for v in m.values())
    t = torch.tensor([0.0, float(n), float(n), float(n)], dtype=torch.float64)
    m = scores_to_metrics(t, h, w)
    assert m['mse'] == 0.0 and m['psnr'] == math.inf and m['ssim'] == 1.0
    m = scores_to_metrics([2.5, 0.0, 0.0, 0.0], 3, 5)            # ssim=False: no SSIM to report
    assert m['mse'] == pytest.approx(2.5 / 45) and math.isnan(m['ssim'])
