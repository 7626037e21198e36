"""CPU check of the MLP-arithmetic rules in hyperreel_amd/csrc/hr_plan.h ("MLP arithmetic"), compiled for the host
(tests/host_math/hr_plan_host.cpp): which arithmetic a model's MLP runs and whether the verified fast path is on (hr_mlp_choice), the
strided sample of a caller's calibration rays (hr_calib_sample), the margins (hr_band_margins), the listed fraction (hr_listed_frac) and
the rule that gives the fast path up (hr_verify_fallback).  The expectations are worked out by hand in the docstrings and tables, not
taken from the code."""
import numpy as np
import pytest

from helpers import band_margins, calib_sample, listed_frac, mlp_choice, mlp_limits, verify_fallback
from hyperreel_amd import config as C
from hyperreel_amd import plan

P = plan.MLP_PRECISION
OK, E_INVALID, E_RANGE = 0, -1, -5                  # include/hyperreel_hip.h
F32 = np.float32
LIMIT = F32(8188.0)                                 # 65504 / 8 = 8188 exactly
FITS = [3.0, 120.0, 80.0, 41.0, 8187.0, 0.5]        # DoNeRF's MLP has six Linears: one maximum each, all below 8188
TOO_LARGE = [3.0, 120.0, 1.0e4, 41.0, 17.0, 0.5]
NOT_A_NUMBER = [3.0, 120.0, 80.0, float('nan'), 17.0, 0.5]


def _config(model='donerf_sphere', mlp_precision='auto'):
    return plan.compile_config(C.model_config(model), C.dataset_scalars(model), [28, 24, 20], mlp_precision=mlp_precision)


def _not_verifiable(hc):
    hc.origin_scale = 0.5                           # a sphere whose origins the head moves: no margin is derived for it
    return hc


def test_limits():
    """65504 / 8 = 8188; the floor 1e-6; a twentieth of the rays; 6e-5 of the 1e-4 budget."""
    assert mlp_limits() == (F32(65504.0) / F32(8.0), F32(1e-6), F32(0.05), F32(6e-5)) and mlp_limits()[0] == LIMIT


# (requested arithmetic, the activations fit, the model can be verified) -> (active arithmetic, verified, calibration needed, status);
# None where the status is an error (the arithmetic is then not read)
#   fp32 / bf16x3 are taken as asked, nothing is measured;
#   auto: fits -> f16f8 + verified where the model can be verified, f16x3 where not; does not fit -> bf16x3;
#   a forced fp16 mode is itself where it fits and HR_E_RANGE where not;
#   f16f8v: HR_E_INVALID on a model that cannot be verified (whatever its range), else f16f8 + verified / HR_E_RANGE
TABLE = {}
for fits in (True, False):
    for cv in (True, False):
        TABLE['fp32', fits, cv] = ('fp32', 0, False, OK)
        TABLE['bf16x3', fits, cv] = ('bf16x3', 0, False, OK)
        for forced in ('f16x3', 'f16x2', 'f16f8'):
            TABLE[forced, fits, cv] = (forced, 0, True, OK) if fits else (None, 0, True, E_RANGE)
    TABLE['f16f8v', fits, False] = (None, 0, True, E_INVALID)
for cv in (True, False):
    TABLE['auto', False, cv] = ('bf16x3', 0, True, OK)
TABLE['auto', True, True] = ('f16f8', 1, True, OK)
TABLE['auto', True, False] = ('f16x3', 0, True, OK)
TABLE['f16f8v', True, True] = ('f16f8', 1, True, OK)
TABLE['f16f8v', False, True] = (None, 0, True, E_RANGE)


def _check(got, want):
    assert got[1:] == want[1:], (got, want)
    if want[0] is not None:
        assert got[0] == P[want[0]], (got, want)


@pytest.mark.parametrize('can_verify', [True, False])
@pytest.mark.parametrize('act,fits', [(FITS, True), (TOO_LARGE, False), (NOT_A_NUMBER, False)], ids=['fits', 'too_large', 'nan'])
@pytest.mark.parametrize('want', sorted(P, key=P.get))
def test_choice_table(want, act, fits, can_verify):
    """The whole table above on DoNeRF's sphere net (32 samples, six 256-wide Linears, fixed origins, the MIP-NeRF contraction: it can
    be verified) and on the same net with origin_scale = 0.5 (it cannot).  A NaN in one layer does not fit, like 1e4 in one layer."""
    assert len(TABLE) == 7 * 2 * 2
    hc = _config(mlp_precision=want)
    assert (hc.isect_type, hc.origin_scale, hc.z_channels, hc.mlp_layers, hc.mlp_hidden) == (plan.ISECT['sphere'], 0.0, 32, 6, 256)
    if not can_verify:
        _not_verifiable(hc)
    _check(mlp_choice(hc, act), TABLE[want, fits, can_verify])


def test_fits_edges():
    """8188.0 itself does not fit (the test is <), the float below it (8188 - 2^-11: 8188 lies in [2^12, 2^13), spacing 2^(12 - 23)) does, in
    whichever layer it stands; infinity does not; a maximum beyond the model's six Linears is not read."""
    below = np.nextafter(LIMIT, F32(0))
    assert float(LIMIT) - float(below) == 2.0 ** -11
    hc = _config(mlp_precision='f16x3')
    for layer in range(6):
        act = [1.0] * 6
        act[layer] = float(below)
        assert mlp_choice(hc, act) == (P['f16x3'], 0, True, OK)
        act[layer] = 8188.0
        assert mlp_choice(hc, act)[3] == E_RANGE
        act[layer] = float('inf')
        assert mlp_choice(hc, act)[3] == E_RANGE
    assert mlp_choice(hc, [1.0] * 6 + [float('inf'), float('nan')]) == (P['f16x3'], 0, True, OK)
    auto = _config()
    assert mlp_choice(auto, [float(below)] * 6) == (P['f16f8'], 1, True, OK)
    assert mlp_choice(auto, [1.0] * 5 + [8188.0]) == (P['bf16x3'], 0, True, OK)


def test_before_a_measurement_the_choice_says_whether_one_is_needed():
    """With nothing measured (all zero) the answer's needs_calibration decides whether the range kernel runs at all: never for fp32,
    bf16x3, a ZeroMLP (auto: f16x3, whose kernels write no head) and auto on a width the split kernels are not written for (fp32); a
    width the range kernel does not cover is HR_E_INVALID for every mode that needs it."""
    zero = [0.0] * 8
    for want, needs in (('fp32', False), ('bf16x3', False), ('auto', True), ('f16x3', True), ('f16x2', True), ('f16f8', True), ('f16f8v', True)):
        assert mlp_choice(_config(mlp_precision=want), zero)[2] == needs
    hc = _config()
    hc.mlp_layers = 0
    assert mlp_choice(hc, zero) == (P['f16x3'], 0, False, OK)
    hc.mlp_precision = P['f16x2']
    assert mlp_choice(hc, zero) == (P['f16x2'], 0, False, OK)
    hc = _config()
    hc.mlp_hidden = 128
    assert mlp_choice(hc, FITS) == (P['fp32'], 0, False, OK)
    for want in ('auto', 'f16x3', 'f16x2', 'f16f8', 'f16f8v'):
        assert mlp_choice(_config(mlp_precision=want), FITS, range_supported=False)[2:] == (True, E_INVALID)
    for want in ('fp32', 'bf16x3'):
        assert mlp_choice(_config(mlp_precision=want), FITS, range_supported=False) == (P[want], 0, False, OK)


def _defeats():
    def cascade(hc):
        return dict(cascade_level=True)

    def samples(hc):
        hc.z_channels = 65                          # a ray's samples no longer sit in one wavefront

    def one_layer(hc):
        hc.mlp_layers = 1

    def sphere_origin(hc):
        hc.origin_scale = 0.5

    def donerf_contract(hc):
        hc.contract_type = plan.CONTRACT['donerf']
    return [pytest.param(f, id=f.__name__) for f in (cascade, samples, one_layer, sphere_origin, donerf_contract)]


@pytest.mark.parametrize('defeat', _defeats())
def test_each_reason_alone_defeats_the_verified_path(defeat):
    """DoNeRF's sphere net with activations that fit is verified under auto; with ONE of: a level of a cascade, 65 samples per ray, a
    single Linear, a sphere whose origins move, the DoNeRF contraction, auto gives f16x3 without verification and a forced f16f8v is
    HR_E_INVALID.  (64 samples, two Linears and the other contractions leave it on.)"""
    for want, good, bad in (('auto', (P['f16f8'], 1, True, OK), (P['f16x3'], 0, True, OK)), ('f16f8v', (P['f16f8'], 1, True, OK), None)):
        hc = _config(mlp_precision=want)
        assert mlp_choice(hc, FITS) == good
        kw = defeat(hc) or {}
        got = mlp_choice(hc, FITS, **kw)
        assert got == bad if bad else got[3] == E_INVALID, got
    hc = _config()
    hc.z_channels, hc.mlp_layers = 64, 2
    for ct in ('identity', 'mipnerf', 'bbox'):
        hc.contract_type = plan.CONTRACT[ct]
        assert mlp_choice(hc, FITS[:2]) == (P['f16f8'], 1, True, OK)


def test_width_128_defeats_it_too():
    """Width 128: auto never reaches the question (fp32, nothing measured); a forced f16f8v is HR_E_INVALID."""
    hc = _config()
    hc.mlp_hidden = 128
    assert mlp_choice(hc, FITS) == (P['fp32'], 0, False, OK)
    hc.mlp_precision = P['f16f8v']
    assert mlp_choice(hc, FITS)[3] == E_INVALID


def test_windowed_encoding_beyond_16_takes_f16f8_away():
    """The f16f8 kernels' v_sin / v_cos encoding is held to pe_base_mult * freq_mult^n_freqs <= 16 per windowed group (6e-8 x 16 ~ 1e-6 of
    phase on a coordinate of order one).  DoNeRF's net has one frequency (2); 2^4 = 16 is inside, the float above 16 (base 1 + 2^-23), 2^5
    and 8 x 2^2 = 32 are beyond: auto and a forced f16f8 / f16f8v are then f16x3 without verification (HR_E_RANGE where the activations
    do not fit, as for a forced f16x3; auto: bf16x3), the other arithmetics as asked.  BasicPE (IEEE sinf in every kernel), a group
    without PE and one without frequencies do not count, a second group does.  A fall-back, not a refusal: shipped nets are beyond the
    limit and are rendered under a forced f16f8 (tests/test_gpu_f16f8.py).  plan.py's mirror agrees case by case."""
    up = float(np.nextafter(F32(1), F32(2)))
    cases = [(1, 2.0, 1.0, True), (4, 2.0, 1.0, True), (2, 4.0, 1.0, True), (3, 2.0, 2.0, True), (4, 2.0, up, False), (5, 2.0, 1.0, False),
             (2, 2.0, 8.0, False), (8, 2.0, 1.0, False), (0, 2.0, 16.0, True), (0, 2.0, 17.0, True), (4, -2.0, 1.0, True), (5, -2.0, 1.0, False)]
    for n, mult, base, ok in cases:
        for want in sorted(P, key=P.get):
            hc = _config(mlp_precision=want)
            g = hc.groups[0]
            assert g.pe_type == plan.PE['windowed']
            g.pe_n_freqs, g.pe_freq_mult, g.pe_base_mult = n, mult, base
            assert plan.fast_sincos_ok(hc) == ok, (n, mult, base)
            got = mlp_choice(hc, FITS)
            if ok or want in ('fp32', 'bf16x3', 'f16x3', 'f16x2'):
                _check(got, TABLE[want, True, True])
                _check(mlp_choice(hc, TOO_LARGE), TABLE[want, False, True])
            else:
                assert got == (P['f16x3'], 0, True, OK), (want, n, mult, base)
                far = mlp_choice(hc, TOO_LARGE)
                assert far == (P['bf16x3'], 0, True, OK) if want == 'auto' else far[2:] == (True, E_RANGE), (want, far)
    hc = _config(mlp_precision='f16f8')
    hc.groups[0].pe_n_freqs = 8
    hc.groups[0].pe_type = plan.PE['basic']
    assert plan.fast_sincos_ok(hc) and mlp_choice(hc, FITS) == (P['f16f8'], 0, True, OK)
    hc.groups[0].pe_type = plan.PE[None]
    assert plan.fast_sincos_ok(hc) and mlp_choice(hc, FITS) == (P['f16f8'], 0, True, OK)
    hc = _config('neural_3d_z_plane', mlp_precision='f16f8v')           # two groups: the rays' and the time column's
    assert hc.n_groups == 2 and mlp_choice(hc, FITS) == (P['f16f8'], 1, True, OK)
    hc.groups[1].pe_n_freqs = 5
    assert not plan.fast_sincos_ok(hc) and mlp_choice(hc, FITS) == (P['f16x3'], 0, True, OK)
    # the five benchmark families: at most 4
    for model in C.MODEL_NAMES:
        hc = _config(model)
        for i in range(hc.n_groups):
            assert hc.groups[i].pe_base_mult * hc.groups[i].pe_freq_mult ** hc.groups[i].pe_n_freqs <= 4.0
    # every arithmetic still compiles beyond the limit (nothing is refused)
    cfg = C.model_config('donerf_sphere')
    cfg.embedding.embeddings.ray_prediction_0.params.ray.pe.update(n_freqs=5, exclude_identity=True)
    ds = C.dataset_scalars('donerf_sphere')
    for want in sorted(P, key=P.get):
        hc = plan.compile_config(cfg, ds, [28, 24, 20], mlp_precision=want)
        assert hc.mlp_in == 60 and hc.mlp_precision == P[want] and not plan.fast_sincos_ok(hc)


def test_shipped_sweep_nets_beyond_the_limit_still_compile_under_f16f8():
    """Why the rule falls back instead of refusing: of the shipped YAMLs' fixtures, stanford_z_plane_mem encodes its two-plane coordinates
    with six frequencies (2^6 = 64) and two more nets sit at the limit itself (2^4).  All of them compile under a forced f16f8, and the
    one beyond the limit resolves to f16x3."""
    from helpers import Golden, sweep_cases
    top = {}
    for case in sweep_cases():
        g = Golden(case)
        if plan.is_cascade(g.cfg):
            continue
        try:
            hc = plan.compile_config(g.cfg, g.dataset, g.grid, mlp_precision='f16f8')
        except NotImplementedError as e:
            assert 'hidden_channels == 256' in str(e), (case, e)          # (the 128-wide nets have the exact fp32 MLP only)
            continue
        freqs = [hc.groups[i].pe_base_mult * hc.groups[i].pe_freq_mult ** hc.groups[i].pe_n_freqs for i in range(hc.n_groups)
                 if hc.groups[i].pe_type == plan.PE['windowed'] and hc.groups[i].pe_n_freqs > 0]
        top[case] = max(freqs, default=0.0)
        assert plan.fast_sincos_ok(hc) == (top[case] <= 16.0)
        if top[case] > 16.0:
            assert mlp_choice(hc, [1.0] * 8) == (P['f16x3'], 0, True, OK)
    assert top['sweep/stanford_z_plane_mem'] == 64.0 and sorted(c for c, v in top.items() if v > 16.0) == ['sweep/stanford_z_plane_mem']
    assert sum(v == 16.0 for v in top.values()) >= 2


def test_intersections_the_margins_are_derived_for():
    """Axis planes (z_plane, voxel_grid), the euclidean distance, sphere and cylinder with fixed origins; not the resized sphere /
    cylinder (sphere_new, cylinder_new) nor the deformable voxel grid.  The shipped families: all five are verified under auto."""
    for model in C.MODEL_NAMES:
        assert mlp_choice(_config(model), FITS) == (P['f16f8'], 1, True, OK), model
    hc = _config('technicolor_z_plane')
    want = {'z_plane': 1, 'sphere': 1, 'cylinder': 1, 'sphere_new': 0, 'cylinder_new': 0, 'euclidean_distance_unified': 1, 'voxel_grid': 1,
            'deformable_voxel_grid': 0}
    assert set(want) == set(plan.ISECT)
    for name, verified in want.items():
        hc.isect_type = plan.ISECT[name]
        assert mlp_choice(hc, FITS) == (P['f16f8'] if verified else P['f16x3'], verified, True, OK), name
    for name in ('sphere', 'cylinder'):
        hc.isect_type, hc.origin_scale = plan.ISECT[name], 0.25
        assert mlp_choice(hc, FITS)[1] == 0
        hc.origin_scale = 0.0


@pytest.mark.parametrize('n,stride,keep', [(160000, 3, 53334), (65536, 1, 65536), (65537, 2, 32769), (1, 1, 1), (640000, 10, 64000)])
def test_calib_sample(n, stride, keep):
    """stride = ceil(n / 65 536), keep = ceil(n / stride): 160 000 / 65 536 = 2.44 -> 3, rays 0, 3, ... 159 999: 53 334 of them
    (= 160 000 // 3 + 1, what tests/test_gpu_verified.py reads back); 65 536 all; 65 537 every other one: 32 769; an 800 x 800 frame
    every tenth."""
    assert calib_sample(n) == (stride, keep)
    assert keep <= 65536 and (keep - 1) * stride < n <= keep * stride


def test_band_margins():
    """band = max(1e-6, 4 max(d_zc, d_dist_n)), band_q = max(1e-6, 4 d_geo_n), band_off = 4 d_off, in float32.  No differences: the
    floor, and no offset margin.  4 x 1e-7 = 4e-7 is still below the floor.  Above it the larger of the two normalised differences
    counts: (1e-6, 5e-7) and (5e-7, 1e-6) both give 4e-6."""
    floor = F32(1e-6)
    assert band_margins(0.0, 0.0, 0.0, 0.0) == (floor, floor, F32(0))
    assert band_margins(1e-7, 1e-7, 1e-7, 1e-7) == (floor, floor, F32(4) * F32(1e-7))
    four = F32(4) * F32(1e-6)
    assert band_margins(1e-6, 5e-7, 3e-7, 2e-3) == (four, F32(4) * F32(3e-7), F32(4) * F32(2e-3))
    assert band_margins(5e-7, 1e-6, 0.0, 0.0) == (four, floor, F32(0))
    assert four > floor and F32(4) * F32(3e-7) > floor


def test_verify_fallback():
    """0: the fast path stays -- at a listed fraction of 0.05 and an image difference of 6e-5 exactly (the tests are > and, for the
    image, not <=); 1: one float above 0.05; 2: one float above 6e-5, or not a number; both: 2 (the image's reason wins)."""
    frac, rgb = F32(0.05), F32(6e-5)
    up = lambda v: np.nextafter(v, F32(1))
    assert verify_fallback(0.0, 0.0) == 0 and verify_fallback(frac, rgb) == 0
    assert verify_fallback(up(frac), rgb) == 1
    assert verify_fallback(frac, up(rgb)) == 2
    assert verify_fallback(0.0, float('nan')) == 2
    assert verify_fallback(up(frac), up(rgb)) == 2 and verify_fallback(1.0, float('inf')) == 2


def test_listed_frac():
    """Synthetic rays (calibrated 1): listed / well-conditioned rays -- 100 of 2000 of the 4096 = 0.05; fewer than 64 well-conditioned
    rays: not measured, 0.  The caller's rays (calibrated 2): the ill-conditioned ones count as listed -- 1000 rays, 800 well
    conditioned of which 200 are listed (0.25, exact in float32): (200 + 0.25 x 800) / 1000 = 0.4; 100 rays of which 10 are well
    conditioned (no image to judge by): (90 + 0) / 100 = 0.9."""
    assert listed_frac(1, 4096, 2000, 100) == F32(0.05)
    assert listed_frac(1, 4096, 4096, 0) == F32(0)
    assert listed_frac(1, 4096, 63, 63) == F32(0) and listed_frac(1, 4096, 64, 64) == F32(1)
    assert listed_frac(2, 1000, 800, 200) == F32(0.4)
    assert listed_frac(2, 100, 10, 5) == F32(0.9)
    assert listed_frac(2, 4096, 4096, 0) == F32(0)
