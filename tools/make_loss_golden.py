"""Generates tests/golden/loss/*.npz by running the REFERENCE'S OWN loss modules (losses.py: loss_dict, imported in-process through
oracle/refgen/ref_shim.py) on seeded batches, through the exact expression of INRSystem.training_step (nlf/__init__.py:665):

    image_loss = self.loss(results['rgb'] * weight, rgb * weight, **batch)

Run where the reference tree exists:

    python tools/make_loss_golden.py

TEST INFRASTRUCTURE ONLY.  inputs.npz holds the batches (`b<B>/pred`, `b<B>/gt`, `b<B>/weight`); one file per loss variant holds, per
batch, the module's float32 loss and its autograd gradient with respect to the prediction (`b<B>/loss32`, `b<B>/grad32`) and the same two
quantities from the same module on float64 tensors (`b<B>/loss64`, `b<B>/grad64`).  The distance between the two is how far one correct
float32 evaluation lies from the exact value; the tests' bars are derived from it (tests/loss_common.py) and recorded in each file's `meta`."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'oracle', 'refgen'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, 'tests', 'golden', 'loss')
BATCHES = [1, 63, 64, 65, 257, 4099]
# variant (file name) -> the reference's cfg.training.loss
VARIANTS = {'mse': dict(type='mse'), 'weighted_mse': dict(type='weighted_mse'), 'mae': dict(type='mae'), 'weighted_mae': dict(type='weighted_mae'),
            'huber_delta1': dict(type='huber', delta=1.0), 'huber_delta0p1': dict(type='huber', delta=0.1)}


class Cfg(dict):
    """what the reference reads from its OmegaConf node: attribute access and `in`"""
    __getattr__ = dict.__getitem__


def make_inputs(B):
    """The seeded batch of B rays: un-clamped predictions, weights other than 1, and the rows every branch of the five types turns on."""
    rng = np.random.default_rng(1000 + B)
    one, tenth = np.float32(1.0), np.float32(0.1)                     # the two huber deltas as the float32 kernels see them
    up, down = (lambda v: np.nextafter(np.float32(v), np.float32(4.0))), (lambda v: np.nextafter(np.float32(v), np.float32(0.0)))
    if B == 1:                                                        # |d| exactly 1.0, exactly 0.1, and pred == gt
        return (np.asarray([[1.0, tenth, 0.5]], np.float32), np.asarray([[0.0, 0.0, 0.5]], np.float32), np.ones((1, 1), np.float32))
    gt = rng.random((B, 3)).astype(np.float32)
    pred = (gt + rng.normal(0.0, 0.3, (B, 3))).astype(np.float32)     # training mode does not clamp: values leave [0, 1]
    weight = rng.uniform(0.25, 2.0, (B, 1)).astype(np.float32)
    i = np.arange(B)
    pred[(i % 17) == 0] = gt[(i % 17) == 0]                           # rows with pred == gt exactly (row 0 among them)
    weight[(i % 23) == 1] = 0.0                                       # rows with w == 0 (row 1 among them)
    weight[(i % 29) == 2] = 1.0
    rows = {2: (1.0, [0, 0, 0], [one, -one, down(one)]),              # |d| == delta 1.0 on both signs, and just inside
            3: (1.0, [0, 0, 0], [up(one), tenth, -tenth]),            # just outside 1.0; |d| == delta 0.1 on both signs
            4: (1.0, [0, 0, 0], [down(tenth), up(tenth), -up(tenth)]),
            5: (2.0, [0.25, 0.25, 0.25], [0.75, -0.25, 0.3]),         # through the weight: 2 * 0.75 - 2 * 0.25 == 1.0 exactly
            6: (1.5, [0.5, 0.5, 0.5], [-0.75, 1.5, 2.25]),            # far outside [0, 1]
            7: (0.0, [0.2, 0.4, 0.6], [0.2, 0.4, 0.6])}               # w == 0 and pred == gt
    for r, (w, g, p) in rows.items():
        weight[r], gt[r], pred[r] = w, np.asarray(g, np.float32), np.asarray(p, np.float32)
    return pred, gt, weight


def reference_loss(cfg, pred, gt, weight, dtype):
    """(loss, d loss / d pred) of the reference's module through training_step's expression, on tensors of `dtype`."""
    import ref_shim
    ref_shim.install()
    from losses import loss_dict
    module = loss_dict[cfg['type']](Cfg(cfg))
    p = torch.from_numpy(pred).to(dtype).requires_grad_(True)
    rgb, w = torch.from_numpy(gt).to(dtype), torch.from_numpy(weight).to(dtype)
    batch = {'coords': torch.zeros((pred.shape[0], 6), dtype=dtype), 'rgb': rgb, 'weight': w}
    loss = module(p * w, rgb * w, **batch)
    loss.backward()
    return loss.detach().numpy().copy(), p.grad.numpy().copy()


def make_all():
    """{file stem: {key: array}} of every fixture file, `meta` included."""
    import loss_common as LC
    torch.set_num_threads(1)
    inputs, files = {}, {v: {} for v in VARIANTS}
    for B in BATCHES:
        pred, gt, weight = make_inputs(B)
        inputs[f'b{B}/pred'], inputs[f'b{B}/gt'], inputs[f'b{B}/weight'] = pred, gt, weight
        for v, cfg in VARIANTS.items():
            l32, g32 = reference_loss(cfg, pred, gt, weight, torch.float32)
            l64, g64 = reference_loss(cfg, pred, gt, weight, torch.float64)
            assert l32.dtype == np.float32 and g32.dtype == np.float32 and l64.dtype == np.float64 and g64.dtype == np.float64
            files[v].update({f'b{B}/loss32': l32, f'b{B}/grad32': g32, f'b{B}/loss64': l64, f'b{B}/grad64': g64})
    for v, cfg in VARIANTS.items():
        dev = LC.deviations_of(files[v])
        meta = dict(cfg=cfg, batches=BATCHES, torch=torch.__version__, **dev, **LC.bars_of(dev))
        files[v]['meta'] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    return {'inputs': inputs, **files}


def main():
    os.makedirs(OUT, exist_ok=True)
    for stem, arrays in make_all().items():
        path = os.path.join(OUT, f'{stem}.npz')
        np.savez_compressed(path, **arrays)
        meta = json.loads(bytes(arrays['meta']).decode()) if 'meta' in arrays else {}
        print(f'{stem}: {os.path.getsize(path) / 1024:.0f} KB  ' + '  '.join(f'{k} {v:.3e}' for k, v in meta.items() if isinstance(v, float) and k != 'delta'))


if __name__ == '__main__':
    main()
