"""Shared by tests/test_loss_host.py and tests/test_gpu_loss.py: the loss fixtures (tests/golden/loss/*.npz, written by
tools/make_loss_golden.py from the reference's own loss modules), the host build of hyperreel_amd/csrc/hr_loss.h, and the bars both
suites hold the loss and its gradient to.

The bars are not constants of these files.  How far one correct float32 evaluation lands from the exact value is a property of the
formulas and the inputs, so it is measured on the reference: per loss variant, the DEVIATION of an array (the loss, or the gradient of
one batch) is the largest |reference float32 - reference float64| divided by the largest float64 magnitude in that array, and the
variant's figure is the largest deviation over its six batches.  An implementation may be 4 x that figure away from the reference's
float32 result, relative to the same magnitude -- the factor covers an equally valid order of the sum and of the gradient's products --
and the bar is never less than 1 ulp (float32 spacing) of that magnitude.  The figures are recomputed from the arrays here; each
file's `meta` records them, and tests/test_loss_host.py holds the record to the recomputation."""
import ctypes as C
import json
import os

import numpy as np

from helpers import build_host_lib
from hyperreel_amd import lib as _lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'loss')
SRC = os.path.join(HERE, 'host_math', 'hr_loss_host.cpp')
OUT = os.path.join(HERE, 'host_math', '_build', 'libhr_loss_host.so')
BATCHES = [1, 63, 64, 65, 257, 4099]
FACTOR = 4.0
# fixture file -> (type name, HR_LOSS_* code, delta)
VARIANTS = {'mse': ('mse', _lib.HR_LOSS_MSE, 1.0), 'weighted_mse': ('weighted_mse', _lib.HR_LOSS_WEIGHTED_MSE, 1.0), 'mae': ('mae', _lib.HR_LOSS_MAE, 1.0),
            'weighted_mae': ('weighted_mae', _lib.HR_LOSS_WEIGHTED_MAE, 1.0), 'huber_delta1': ('huber', _lib.HR_LOSS_HUBER, 1.0),
            'huber_delta0p1': ('huber', _lib.HR_LOSS_HUBER, 0.1)}
_cache = {}


def load_file(stem):
    if stem not in _cache:
        with np.load(os.path.join(GOLDEN, f'{stem}.npz')) as z:
            _cache[stem] = {k: z[k] for k in z.files}
    return _cache[stem]


def meta(variant):
    return json.loads(bytes(load_file(variant)['meta']).decode())


def inputs(B):
    z = load_file('inputs')
    return z[f'b{B}/pred'], z[f'b{B}/gt'], z[f'b{B}/weight']


def expected(variant, B):
    """{'loss32', 'grad32', 'loss64', 'grad64'} of one variant and batch"""
    z = load_file(variant)
    return {k: z[f'b{B}/{k}'] for k in ('loss32', 'grad32', 'loss64', 'grad64')}


def deviations_of(arrays):
    """{'loss_deviation', 'grad_deviation'} of one variant's arrays (keys b<B>/...): the largest relative distance of the reference's
    float32 result from its float64 one over the batches"""
    dl = dg = 0.0
    for B in BATCHES:
        l32, l64 = float(arrays[f'b{B}/loss32']), float(arrays[f'b{B}/loss64'])
        g32, g64 = arrays[f'b{B}/grad32'].astype(np.float64), arrays[f'b{B}/grad64']
        dl = max(dl, abs(l32 - l64) / abs(l64))
        dg = max(dg, float(np.abs(g32 - g64).max() / np.abs(g64).max()))
    return {'loss_deviation': dl, 'grad_deviation': dg}


def bars_of(dev):
    """the relative part of the bars; the 1-ulp floor depends on the array and is applied by loss_bar / grad_bar"""
    return {'loss_bar_rel': FACTOR * dev['loss_deviation'], 'grad_bar_rel': FACTOR * dev['grad_deviation']}


def _rel(variant):
    if ('rel', variant) not in _cache:
        _cache[('rel', variant)] = bars_of(deviations_of(load_file(variant)))
    return _cache[('rel', variant)]


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


def loss_bar(variant, loss64):
    """absolute bar on a loss whose exact value is loss64"""
    return max(_rel(variant)['loss_bar_rel'] * abs(float(loss64)), _ulp(loss64))


def grad_bar(variant, grad64):
    """absolute, elementwise bar on a gradient array whose exact value is grad64"""
    m = float(np.abs(grad64).max())
    return max(_rel(variant)['grad_bar_rel'] * m, _ulp(m))


def host_lib():
    deps = [SRC, os.path.join(HERE, '..', 'hyperreel_amd', 'csrc', 'hr_loss.h'), os.path.join(HERE, '..', 'include', 'hyperreel_hip.h')]
    build_host_lib(OUT, SRC, deps)
    lib = C.CDLL(OUT)
    lib.hl_offsetof_out.argtypes = [C.c_int]
    lib.hl_type_code.argtypes = [C.c_int]
    lib.hl_type_valid.argtypes = [C.c_int32]
    lib.hl_blocks.argtypes = [C.c_int64]
    lib.hl_blocks.restype = C.c_int64
    lib.hl_image_loss.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.POINTER(_lib.hr_loss_out), C.c_void_p]
    lib.hl_image_loss.restype = None
    return lib


def host_loss(lib, code, delta, pred, gt, weight=None, upstream=None, want_grad=True):
    """hr_loss.h compiled for the host over a batch -> {'loss', 'loss_sum', 'sse', 'pad', 'grad'}"""
    pred, gt = np.ascontiguousarray(pred, np.float32), np.ascontiguousarray(gt, np.float32)
    n = pred.size // 3
    w = None if weight is None else np.ascontiguousarray(weight, np.float32)
    up = None if upstream is None else np.asarray([upstream], np.float32)
    grad = np.full(pred.shape, np.nan, np.float32) if want_grad else None
    out = _lib.hr_loss_out()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    lib.hl_image_loss(ptr(pred), ptr(gt), ptr(w), n, int(code), float(delta), ptr(up), C.byref(out), ptr(grad))
    return {'loss': np.float32(out.loss), 'loss_sum': out.loss_sum, 'sse': out.sse, 'pad': out.pad, 'grad': grad}
