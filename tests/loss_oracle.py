"""Test oracle of the training image loss (hr_image_loss): the five loss modules of the reference that INRSystem.training_step can call
(losses.py: huber | mse | weighted_mse | mae | weighted_mae) through its expression `loss(pred * weight, rgb * weight, **batch)`
(nlf/__init__.py:665), restated in float64 numpy with the derivative written out.  Lives in the test tree: the product never imports it.
tests/test_loss_host.py holds it to the reference's own float64 results (tests/golden/loss)."""
import numpy as np

TYPES = ('mse', 'weighted_mse', 'mae', 'weighted_mae', 'huber')


def loss(type, pred, gt, weight=None, delta=1.0, premultiplied=False):
    """{'loss', 'grad' (B, 3), 'sse', 'loss_sum'} in float64.  weight: (B, 1) or None (1).  premultiplied: pred and gt already carry the
    weight (d = pred - gt and d d / d pred = 1); otherwise d = pred * weight - gt * weight and d d / d pred = weight."""
    p, g = np.asarray(pred, np.float64).reshape(-1, 3), np.asarray(gt, np.float64).reshape(-1, 3)
    w = np.ones((p.shape[0], 1)) if weight is None else np.asarray(weight, np.float64).reshape(-1, 1)
    d = p - g if premultiplied else p * w - g * w
    c = np.ones_like(w) if premultiplied else w
    if type == 'mse':
        term, dterm = d * d, 2.0 * d
    elif type == 'weighted_mse':
        term, dterm = w * d * d, 2.0 * w * d
    elif type == 'mae':
        term, dterm = np.abs(d), np.sign(d)
    elif type == 'weighted_mae':
        term, dterm = w * np.abs(d), w * np.sign(d)
    elif type == 'huber':
        z = np.abs(d)
        term = np.where(z < delta, 0.5 * d * d, delta * (z - 0.5 * delta))
        dterm = np.where(z < delta, d, delta * np.sign(d))
    else:
        raise KeyError(type)
    n = term.size
    return {'loss': float(term.sum() / n), 'loss_sum': float(term.sum()), 'grad': dterm * c / n, 'sse': float(((p - g) ** 2).sum())}
