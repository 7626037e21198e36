"""The life of a model's hr_model handle as the sequence of library calls it causes (models.native_action decides):
every symbol the package calls is recorded through a proxy over the loaded library, and the images of the handles that were kept,
re-uploaded, re-configured or re-created are compared bit for bit.  `-m gpu` only; 256 rays per call."""
import warnings

import numpy as np
import pytest
import torch

from helpers import Golden, linf
from hyperreel_amd import lib
from hyperreel_amd.plan import upload_names

pytestmark = pytest.mark.gpu

N_RAYS = 256
RGB_TOL = 1e-4                                          # BASELINE.json north_star, as tests/test_gpu_parity.py
IGNORED = ('hr_model_get_option', 'hr_last_error')      # the overflow guard's polls on a model's first render calls; error texts
SETUP = {'hr_model_set_option', 'hr_train_set_background'}


class Recorder:
    """Stands where lib.load() keeps the ctypes handle: every symbol that is called is noted by name, then called."""

    def __init__(self, real):
        self._real, self.names = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def recorded(*args):
            if name not in IGNORED:
                self.names.append(name)
            return fn(*args)
        recorded.restype = fn.restype
        return recorded

    def take(self):
        out, self.names = self.names, []
        return out


@pytest.fixture
def rec(monkeypatch):
    r = Recorder(lib.load())
    monkeypatch.setattr(lib, '_lib', r)
    yield r
    import gc
    gc.collect()                                        # models of this test destroy their handles while the proxy still stands


def _model(case, iteration=None):
    from gpu_common import make_render_fn
    g = Golden(case)
    fn = make_render_fn(g.cfg, g.dataset, g.state_dict, iteration=iteration)
    rays = torch.from_numpy(np.ascontiguousarray(g.rays[:N_RAYS], np.float32)).cuda()
    return g, fn, fn.model, rays


def _render(m, rays):
    out = m.render(rays)['rgb'].clone()
    torch.cuda.synchronize()
    return out


def _n_uploads(m):
    return len(upload_names(m._hc, m._coarse_hc))


def _touch(p, factor=1.0):
    with torch.no_grad():                               # as an optimizer updates it: the version moves (through `.data` it would not)
        p.mul_(factor)


def _check_first_render(seq, m, reserve=False):
    """create, the option and background calls, hr_model_reserve iff asked for, every tensor once, finalize, the render."""
    n = _n_uploads(m)
    assert seq[0] in ('hr_model_create', 'hr_model_create_cascade')
    k = 1
    while seq[k] in SETUP:
        k += 1
    assert k >= 3                                       # at least the frame-kernel and determinism options and the background
    if reserve:
        assert seq[k] == 'hr_model_reserve'
        k += 1
    assert seq[k:] == ['hr_model_upload'] * n + ['hr_model_finalize', 'hr_render'], seq


def test_first_render_creates_second_keeps_and_an_update_uploads(rec):
    g, fn, m, rays = _model('donerf_sphere_small')
    assert rec.take() == []                             # building and loading a model touches no handle
    first = _render(m, rays)
    seq = rec.take()
    _check_first_render(seq, m)
    assert 'hr_model_reserve' not in seq
    assert linf(first.cpu().numpy(), g.rgb[:N_RAYS]) <= RGB_TOL
    # b. nothing moved
    second = _render(m, rays)
    assert rec.take() == ['hr_render']
    assert torch.equal(first, second)
    # c. an in-place update of one plane: the same handle, every tensor again
    handle = m._native.value
    _touch(m.color_model.net.density_plane[0])
    third = _render(m, rays)
    assert rec.take() == ['hr_model_upload'] * _n_uploads(m) + ['hr_model_finalize', 'hr_render']
    assert m._native.value == handle
    assert torch.equal(first, third)


def test_a_schedule_move_reconfigures_a_single_level_handle(rec):
    g, fn, m, rays = _model('sweep/variant_ease_iter6000')      # never told an iteration: converged
    converged = _render(m, rays)
    rec.take()
    m.set_iter(g.iteration)
    moved = _render(m, rays)
    assert rec.take() == ['hr_model_update_config', 'hr_render']
    assert linf(moved.cpu().numpy(), g.rgb[:N_RAYS]) <= RGB_TOL         # the reference's image at that iteration
    assert linf(g.rgb[:N_RAYS], converged.cpu().numpy()) > 1e-3         # ... where its schedules are active
    m.set_iter(g.iteration + 0)                                          # told the same iteration again: nothing to do
    _render(m, rays)
    assert rec.take() == ['hr_render']
    m.set_iter(10_000_000)
    assert torch.equal(_render(m, rays), converged)
    assert rec.take() == ['hr_model_update_config', 'hr_render']


def test_grid_growth_recreates_the_handle_with_its_reserve(rec):
    g, fn, m, rays = _model('donerf_sphere_small')
    m.reserve(4096)
    seq = rec.take()
    assert seq[-1] == 'hr_model_reserve'                # reserve() itself, behind the first native()
    _check_first_render(seq[:-1] + ['hr_render'], m, reserve=True)
    _render(m, rays)
    assert rec.take() == ['hr_render']
    m.upsample_volume_grid([v + 1 for v in m.grid_size])
    assert set(rec.take()) == {'hr_upsample_plane'}
    _render(m, rays)
    seq = rec.take()
    assert seq[0] == 'hr_model_destroy'
    _check_first_render(seq[1:], m, reserve=True)         # a re-created handle gets the remembered reserve again


def test_a_cascade_whose_parameters_and_schedule_moved_is_created_and_uploaded_once(rec):
    from hyperreel_amd.models import HipLightfieldModel
    g, fn, m, rays = _model('sweep/technicolor_cascaded')
    converged_cfg = bytes(m._compile(m.grid_size)[1])
    _render(m, rays)
    _check_first_render(rec.take(), m)
    _touch(m.color_model.net.density_plane_space[0], 1.01)
    m.set_iter(1000)
    assert bytes(m._compile(m.grid_size)[1]) != converged_cfg           # inside a window of the cascade's schedules
    moved = _render(m, rays)
    seq = rec.take()
    n = _n_uploads(m)
    assert seq.count('hr_model_destroy') == 1 and seq.count('hr_model_create_cascade') == 1 and seq.count('hr_model_update_config') == 0
    assert seq.count('hr_model_upload') == n and seq.count('hr_model_finalize') == 1, seq      # (before: everything twice)
    assert seq[0] == 'hr_model_destroy'
    _check_first_render(seq[1:], m)
    fresh = HipLightfieldModel(g.cfg, dataset=g.dataset, grid_size=g.grid).cuda()
    fresh.load_state_dict(m.state_dict())
    fresh.set_iter(1000)
    assert torch.equal(_render(fresh, rays), moved)
    del fresh
    rec.take()
    # the schedule alone, on the way back: one re-creation as well
    m.set_iter(10_000_000)
    _render(m, rays)
    seq = rec.take()
    assert seq[0] == 'hr_model_destroy'
    _check_first_render(seq[1:], m)


def test_training_steps_upload_nothing_and_the_next_render_uploads_once(rec):
    from hyperreel_amd.optim import HipAdam
    g, fn, m, rays = _model('donerf_sphere_small')
    before = _render(m, rays)
    fn.train()
    opt = HipAdam([p for n, p in m.named_parameters() if p.requires_grad and 'dummy' not in n], lr=1e-3)
    rgb = m.forward_train(rays, white_bg=False)
    assert rec.take()[-1] == 'hr_train_forward'
    (rgb ** 2).mean().backward()
    opt.step()
    rgb2 = m.forward_train(rays, white_bg=False)
    seq = rec.take()
    assert 'hr_train_backward' in seq and seq.count('hr_adam_step') == 1 and seq[-1] == 'hr_train_forward'
    assert not {'hr_model_upload', 'hr_model_finalize', 'hr_model_create', 'hr_model_destroy', 'hr_model_update_config'} & set(seq), seq
    assert not torch.equal(rgb, rgb2)                   # the step's values reached the kernels without an upload
    fn.eval()
    stepped = _render(m, rays)                          # HipAdam moved the versions of what it stepped: the handle's copies are stale
    assert rec.take() == ['hr_model_upload'] * _n_uploads(m) + ['hr_model_finalize', 'hr_render']
    assert not torch.equal(stepped, before)
    _render(m, rays)
    assert rec.take() == ['hr_render']


def test_a_forward_with_fields_leaves_no_request_behind(rec):
    from hyperreel_amd import train as T
    g, fn, m, rays = _model('donerf_sphere_small')
    m.set_train_deterministic(True)                     # gradient sums in fixed point: two backward passes agree bit for bit
    with torch.no_grad():
        ref = m.render(rays, want=('distances', 'points', 'render_weights'))
    fn.train()
    plain = m.forward_train(rays, white_bg=False)
    rec.take()
    rgb, f = m.forward_train(rays, white_bg=False, want_fields=True)
    assert rec.take()[-1] == 'hr_train_forward_fields'
    assert torch.equal(rgb, plain) and rgb.requires_grad
    assert sorted(f) == ['distances', 'head', 'points', 'render_weights']
    for k in ('distances', 'points', 'render_weights'):
        assert f[k].shape == ref[k].shape and not f[k].requires_grad
        assert float((f[k] - ref[k]).abs().max()) <= 2e-5 * max(1.0, float(ref[k].abs().max())), k       # the bar of tests/test_gpu_train.py
    assert not hasattr(T.SampleStage, 'want_fields') and not hasattr(T.SampleStage, 'fields_out')
    again = m.forward_train(rays, white_bg=False)
    seq = rec.take()
    assert seq[-1] == 'hr_train_forward' and 'hr_train_forward_fields' not in seq
    assert torch.equal(again, plain)
    (rgb * 2).sum().backward()                          # the stage with fields carries the colour's gradient like the plain one
    grads = [p.grad.clone() for p in m.color_model.net.parameters() if p.grad is not None]
    for p in m.parameters():
        p.grad = None
    (again * 2).sum().backward()
    plain_grads = [p.grad for p in m.color_model.net.parameters() if p.grad is not None]
    assert len(grads) == len(plain_grads) > 0 and all(torch.equal(a, b) for a, b in zip(grads, plain_grads))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        out = fn(rays, fields=['distances'])            # forward()'s train-mode branch rides on the same stage
    assert out['rgb'].requires_grad and not out['distances'].requires_grad
