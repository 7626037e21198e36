"""The render sample stage's dispatch without a GPU (tests/render_dispatch_common.py): every row lands on the instantiation it claims --
answered by the library's own hr_sample_form_plan (csrc/hr_plan.h, compiled for the host) --, the claimed sets are the compiled ones, every
row's scene meets the conditions that make a comparison on it worth something, computed from the reference restatements alone, and the two
restatements the table adds (time_decode_oracle.time_port's density modes, shading_oracle.shade_port) agree with the reference-made
fixtures."""
import numpy as np
import pytest

import render_dispatch_common as R
from helpers import Golden, sample_plan
from hyperreel_amd import scenes

RGB_TOL, WEIGHT_TOL = 1e-4, 5e-5               # the device tests' bars (tests/test_gpu_parity.py)


# ---------------------------------------------------------------- the table
def test_the_claimed_sets_are_the_compiled_sets():
    """60 + 60 + 72 + 8 + 8, enumerated from the rule in hr_plan.h: no instantiation without a row, no row without an instantiation."""
    compiled, claimed = R.compiled_sets(), R.claimed_sets()
    assert {k: len(v) for k, v in compiled.items()} == {'hr_sample_kernel': 60, 'hr_sample_maps_kernel': 60, 'hr_sample_time_kernel': 72,
                                                         'hr_sample_shade_export_kernel': 8, 'hr_sample_shade_import_kernel': 8}
    for kernel in compiled:
        assert claimed[kernel] == compiled[kernel], (kernel, sorted(compiled[kernel] ^ claimed[kernel]))
    assert len(R.ROWS) == 60 + 72 + 8


def test_the_rotations_reach_every_mode():
    td3 = [R.ROWS[n] for n in R.rows_of('time_density')]
    assert {r['shading'] for r in td3} == {'RGB', 'SH', 'RGBtLinear', 'RGBtFourier'}
    assert {r['density_mode'] for r in td3} == {'DensityLinear', 'DensityFourier'}
    for pc in (0, 1, 2):                                 # ... in every plane class, and both modes under both texel formats
        assert {(r['shading'], r['density_mode']) for r in td3 if r['inst'][2] == pc} == {(s, d) for s in R.DENSITY_SHADING for d in R.DENSITY_MODE}
    td1 = [R.ROWS[n] for n in R.rows_of('time')]
    assert {r['shading'] for r in td1} == {'RGBtLinear', 'RGBtFourier', 'RGBIdentity'}
    for half in (0, 1):
        assert {r['shading'] for r in td1 if r['inst'][1] == half} == {'RGBtLinear', 'RGBtFourier', 'RGBIdentity'}
    shade = [R.ROWS[n] for n in R.rows_of('shade')]
    assert sorted(r['shading'] for r in shade) == ['MLP'] * 4 + ['MLP_Fea'] * 4
    assert {(r['shading'], r['inst'][1]) for r in shade} == {(m, h) for m in ('MLP', 'MLP_Fea') for h in (0, 1)}


@pytest.mark.parametrize('name', sorted(R.ROWS))
def test_row_lands_on_the_instantiation_it_claims(name):
    hc = R.assert_instantiation(name)
    sc = R.scene(name)
    assert sc.rays.shape == (R.N_RAYS, 8 if sc.video else 6)
    zp = R.ROWS[name]['inst'][0]
    assert R.N_RAYS % (256 // zp) != 0 or zp > 64         # no workgroup is full except where a workgroup holds one ray
    assert R.ROWS[name]['z'] & (R.ROWS[name]['z'] - 1) and zp // 2 < R.ROWS[name]['z'] < zp
    if R.ROWS[name]['kind'] == 'decode' and sc.video:    # inside hr_render_frame a float32 keyframe net takes the line form
        _, half, pc, nb = R.ROWS[name]['inst']
        assert nb == 4 and sample_plan(hc, R.N_RAYS, frame_lines=True)[1] == (zp, half, pc, 4 if half else 2)


# ---------------------------------------------------------------- the scenes, from the reference alone
@pytest.mark.parametrize('name', sorted(R.ROWS))
def test_scene_conditions(name):
    """Conditions, not measurements: every quarter of the sample-index range holds at least 0.05 of the summed compositing weight, at
    least 0.95 of the sample indices carry a weight above 1e-3 on some ray, the image is no constant, and a float16 row's half-rounded
    scene renders another image than the float32 scene."""
    ref = R.reference(name)
    w, rgb = ref['render_weights'].astype(np.float64), ref['rgb']
    z = R.ROWS[name]['z']
    assert w.shape == (R.N_RAYS, z) and rgb.shape == (R.N_RAYS, 3) and np.isfinite(rgb).all()
    quarters = [w[:, i * z // 4:(i + 1) * z // 4].sum() / w.sum() for i in range(4)]
    assert min(quarters) >= 0.05, quarters
    assert (w > 1e-3).any(0).mean() >= 0.95
    assert rgb.std() > 0.01
    if R.ROWS[name]['inst'][1]:
        assert np.abs(rgb - R.reference(name, half=False)['rgb']).max() > 0


def test_the_unthinned_scene_would_not_do():
    """The finding behind DENSITY_SCALE: at density 1 the back half of a 200-sample ray carries no weight."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'oracle'))
    from hyperreel_oracle import HyperReelOracle
    sc = R.scene('decode_z200_fp32_pc1_nb2')
    w = HyperReelOracle(sc.cfg, sc.dataset, scenes.scale_density(sc.state_dict, 1.0 / R.DENSITY_SCALE)).render(sc.rays, keep='all')['render_weights']
    assert w[:, :50].sum() / w.sum() >= 0.95 and w[:, 100:].sum() / w.sum() < 1e-3
    assert (w > 1e-3).any(0).mean() < 0.6


# ---------------------------------------------------------------- the restatements the table adds, against the reference's own output
def _fixture_scene(g):
    return scenes.carve_half_space(scenes.scale_density(g.state_dict, g.recipe.get('density_scale', 1.0)), g.recipe['carve_x'])


@pytest.mark.parametrize('case', ['time_decode/c_technicolor_density_fourier', 'time_decode/c_technicolor_density_linear',
                                  'time_decode/d_technicolor_both_fourier', 'time_decode/e_neural_3d_both_fourier',
                                  'time_decode/a_technicolor_rgbt_linear', 'time_decode/g_donerf_rgb_identity',
                                  'time_decode/h_technicolor_linear_white_bg'])
def test_time_port_equals_the_reference(case):
    """time_decode_oracle.time_port with its density modes against fixtures the reference wrote (c_*, d_*, e_*, and the white-background
    one), and two colour-only ones through the same code."""
    from time_decode_oracle import time_port
    g = Golden(case)
    got = time_port(g.cfg, g.dataset, _fixture_scene(g)).fields(g.rays)
    print(f'{case}: rgb {np.abs(got["rgb"] - g.rgb).max():.3e}, weights {np.abs(got["render_weights"] - g.arrays["render_weights"]).max():.3e}')
    assert np.abs(got['rgb'] - g.rgb).max() <= RGB_TOL
    assert np.abs(got['render_weights'] - g.arrays['render_weights']).max() <= WEIGHT_TOL
    if 'sigma_pre' in g.arrays and g.cfg.color.net.get('densityMode', 'Density') != 'Density':
        want = g.arrays['sigma_pre'].ravel()                 # the reference's density features of its valid samples, in their order
        assert got['valid'].sum() == want.size and np.abs(got['sigma_pre'][got['valid']] - want).max() <= 1e-5 * max(1.0, np.abs(want).max())


def _shading_cases():
    from test_shade_host import WHOLE
    return WHOLE


@pytest.mark.parametrize('case', _shading_cases())
def test_shade_port_equals_the_reference(case):
    """shading_oracle.shade_port against fixtures shading/a..g."""
    from shading_oracle import shade_port
    g = Golden(case)
    got = shade_port(g.cfg, g.dataset, _fixture_scene(g)).fields(g.rays)
    print(f'{case}: rgb {np.abs(got["rgb"] - g.rgb).max():.3e}, weights {np.abs(got["render_weights"] - g.arrays["render_weights"]).max():.3e}')
    assert np.abs(got['rgb'] - g.rgb).max() <= RGB_TOL
    assert np.abs(got['render_weights'] - g.arrays['render_weights']).max() <= WEIGHT_TOL
