"""Every instantiation of the render sample stage's kernels on the device against the reference restatement of its kind
(tests/render_dispatch_common.py: one row per instantiation; tests/test_render_dispatch_host.py shows that a row lands where it claims and
that its scene spreads the compositing weight over all sample indices).  `-m gpu` only.

Every model is built with mlp_precision='fp32': the head is the oracle's chain and the call renders launch by launch (nothing verified, no
frame kernel), so a difference is the sample kernel's.  Bars, the suite's own: rgb 1e-4, render_weights 5e-5, distances 2e-5 relative
(tests/test_gpu_parity.py), `acc` against the summed reference weights 1e-4 (tests/test_gpu_time_decode.py), hr_render_frame against
hr_render 5e-6 (test_frame_entry_points)."""
import numpy as np
import pytest
import torch

import render_dispatch_common as R

pytestmark = pytest.mark.gpu

RGB_TOL, WEIGHT_TOL, DIST_TOL, ACC_TOL, FRAME_TOL = 1e-4, 5e-5, 2e-5, 1e-4, 5e-6


class _Report:
    """Collects error / bar per compared quantity, prints them all, then asserts them all."""

    def __init__(self, title):
        self.title, self.rows, self.errors = title, [], []

    def add(self, what, err, tol):
        self.rows.append((what, err / tol))
        if not err <= tol:
            self.errors.append(f'{what}: {err:.3e} > {tol:.1e}')

    def linf(self, what, got, want, tol):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        assert np.isfinite(got).all(), what
        self.add(what, float(np.abs(got - want).max()), tol)

    def relative(self, what, got, want, tol):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        assert np.isfinite(got).all(), what
        self.add(what, float((np.abs(got - want) / (1.0 + np.abs(want))).max()), tol)

    def finish(self):
        worst = max(self.rows, key=lambda r: r[1])
        print(f'{self.title}: worst error / bar {worst[1]:.3f} ({worst[0]}); ' + ', '.join(f'{w} {r:.3f}' for w, r in self.rows))
        assert not self.errors, f'{self.title}: ' + '; '.join(self.errors)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _np(t):
    return t.detach().cpu().numpy()


def _model(name):
    from gpu_common import make_render_fn
    sc = R.scene(name)
    fn = make_render_fn(sc.cfg, sc.dataset, sc.state_dict, mlp_precision='fp32', grid_dtype=R.DTYPE[R.ROWS[name]['inst'][1]])
    return sc, fn.model, torch.from_numpy(sc.rays).cuda()


def _check_row(name):
    """The image, the compositing weights, the distances and the opacity map of the row's model against the row's reference (a float16
    row: the reference on the half-rounded scene); the image of the maps call and of a ray rendered on its own, bit for bit."""
    sc, model, rays = _model(name)
    ref = R.reference(name)
    plain = model.render(rays)['rgb'].clone()
    out = model.render(rays, want=('distances', 'render_weights'))
    fields = {k: v.clone() for k, v in out.items()}
    maps = model.render(rays, maps=('acc', 'distances'))
    maps = {k: v.clone() for k, v in maps.items()}
    ones = {i: model.render(rays[i:i + 1].contiguous())['rgb'].clone() for i in (0, R.N_RAYS - 1, R.workgroup_edge(name))}
    torch.cuda.synchronize()
    assert not model.mlp_verified() and not model.frame_kernel_active() and model.mlp_precision_active() == 'fp32'
    rep = _Report(f'{name} {R.ROWS[name]["inst"]}')
    rep.linf('rgb', _np(plain), ref['rgb'], RGB_TOL)
    rep.linf('rgb (diagnostics call)', _np(fields['rgb']), ref['rgb'], RGB_TOL)
    rep.linf('render_weights', _np(fields['render_weights']), ref['render_weights'], WEIGHT_TOL)
    rep.relative('distances', _np(fields['distances']), ref['distances'], DIST_TOL)
    rep.linf('acc', _np(maps['acc'][:, 0]), ref['render_weights'].astype(np.float64).sum(1), ACC_TOL)
    rep.finish()
    assert torch.equal(_bits(maps['rgb']), _bits(plain)), 'the image of the maps call'
    for i, one in ones.items():
        assert torch.equal(_bits(one), _bits(plain[i:i + 1])), f'ray {i} on its own'
    return sc, model, rays


@pytest.mark.parametrize('name', R.rows_of('decode'))
def test_decode_row_matches_the_oracle(name):
    """hr_sample_kernel (hr_render) and hr_sample_maps_kernel (hr_render_maps, hr_render_fields) <ZP, HALF, PC, NB> against HyperReelOracle.
    A keyframe net additionally through hr_render_frame with every ray at one time: the float32 nets run the NB 2 instantiation of their
    class there, on a blended time row."""
    sc, model, rays = _check_row(name)
    if sc.video:
        r = rays.clone()
        r[:, -1] = 0.27
        a = model.render(r)['rgb'].clone()
        b = model.render(r, frame_time=0.27)['rgb'].clone()
        c = model.render(r, frame_time=0.27, maps=('acc',))['rgb'].clone()
        torch.cuda.synchronize()
        d = float((a - b).abs().max())
        print(f'{name}: hr_render_frame against hr_render {d:.3e} (bar {FRAME_TOL:.0e})')
        assert d <= FRAME_TOL, d
        assert torch.equal(_bits(c), _bits(b))
        assert float((a - model.render(rays)['rgb']).abs().max()) > 1e-3          # the image does depend on the ray's time


@pytest.mark.parametrize('name', R.rows_of('time', 'time_density'))
def test_time_row_matches_the_restatement(name):
    """hr_sample_time_kernel <ZP, HALF, PC, TD> against time_decode_oracle.time_port."""
    _check_row(name)


@pytest.mark.parametrize('name', R.rows_of('shade'))
def test_shade_row_matches_the_restatement(name):
    """hr_sample_shade_export_kernel and hr_sample_shade_import_kernel <ZP, HALF>, the colour network between them, against
    shading_oracle.shade_port."""
    _check_row(name)
