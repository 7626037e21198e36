"""Fisheye camera rays without a GPU: the fisheye part of hyperreel_amd/csrc/hr_camera.h compiled for the host against the float64
oracle of tests/fisheye_common.py, the solver's step count and round trip, the tangent it uses, the invertibility rule, the bound entry
points and the refusals that happen before anything touches a device.

The bar for ray coordinates is fisheye_common.bars(): 4 x the distance between a numpy float32 evaluation of the same steps and the
float64 oracle per column group over all cases, capped at 1e-5 (measured: origins 3.05e-6 -> the cap 1e-5, directions 1.24e-6 -> bar
4.97e-6; the host build lands at 2.57e-6 / 1.04e-6).  Every test prints what it measured.

An all-zero pair means "no distortion given" in this interface and is the pinhole camera, like a NULL hr_fisheye: both are asserted
bit for bit against hr_pixel_ray, and the oracle skips the undistortion for (0, 0) as the contract does.  (The model itself, and OpenCV,
would read zeros as the lens theta_d = theta; the header documents the convention and how to ask for that lens.)"""
import ctypes as C
import os

import numpy as np
import pytest

import fisheye_common as FC
from hyperreel_amd import data, lib
from hyperreel_amd.plan import hr_camera, hr_fisheye, hr_ndc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def hf():
    return FC.host_lib()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_the_cases_are_the_documented_ones():
    assert FC.PAIRS == [(0.0, 0.0), (0.03, 0.004), (-0.05, 0.01), (0.2, -0.02)]
    assert [FC.CASES[n][:2] for n in ('centred', 'one_pixel', 'off_centre', 'short_focal')] == [(24, 14), (1, 1), (33, 7), (24, 14)]
    for pair in FC.PAIRS:
        assert FC.invertible(*pair), pair
    for name in FC.CASES:
        td = FC.corner_theta_d(name)
        print(f'{name}: corner theta_d {td:.4f}', flush=True)
        assert td < np.pi / 2
        for pair in FC.PAIRS:                                   # and the undistorted angle stays in the quadrant too
            assert float(FC.solve_theta(pair[0], pair[1], np.array([td]), np.float64)[0]) < np.pi / 2 - 0.1
    assert abs(FC.corner_theta_d('short_focal') - 1.2) < 0.01
    W, H, K, _ = FC.CASES['off_centre']
    assert (K[0, 2], K[1, 2]) == (10.5, 2.5) and abs(K[0, 2] - W / 2) > 5                  # pixel (10, 2) sits on the principal point
    for name, px in (('off_centre', [[10, 2]]), ('one_pixel', [[0, 0]])):
        for pair in FC.PAIRS:
            r = FC.rays(name, pair, None, np.float64, pixels=np.array(px))
            pin = FC.rays(name, None, None, np.float64, pixels=np.array(px))
            assert np.array_equal(r, pin), (name, pair)                                     # theta_d = 0: the unchanged branch


def test_the_bars_come_from_the_float32_evaluation():
    d, b = FC.reference_distances(), FC.bars()
    print(f'numpy float32 vs the float64 oracle: {d}; bars: {b}', flush=True)
    for k in ('origins', 'directions'):
        assert 0.0 < d[k] < 1e-5 and b[k] == min(4.0 * d[k], 1e-5)


@pytest.mark.parametrize('name', list(FC.CASES))
def test_host_header_against_the_oracle(hf, name):
    for pair in FC.PAIRS:
        for ndc in (None, FC.NDC):
            got = FC.host_rays(hf, name, pair, ndc)
            assert np.isfinite(got).all()
            FC.check_coords(got, FC.oracle(name, pair, ndc), f'{name} {pair} ndc={ndc is not None} (host build of hr_camera.h)')
            if ndc is None:
                assert np.array_equal(got[:, :3], np.broadcast_to(FC.CASES[name][3][:, 3], (got.shape[0], 3)))


def test_a_pixel_range_is_the_same_rows(hf):
    whole = FC.host_rays(hf, 'off_centre', FC.PAIRS[3], FC.NDC)
    n = whole.shape[0]
    for first, cnt in ((0, 7), (5, 100), (n - 9, 9), (n, 0)):
        part = FC.host_rays(hf, 'off_centre', FC.PAIRS[3], FC.NDC, first, cnt)
        assert np.array_equal(part.view(np.uint32), whole[first:first + cnt].view(np.uint32))


def _pinhole(hf, name, ndc):
    W, H = FC.CASES[name][:2]
    cam, nd = FC.camera_of(name), data.make_ndc(ndc)
    out = np.full((W * H, 6), np.nan, np.float32)
    hf.hf_pinhole_rays(C.byref(cam), C.byref(nd) if nd is not None else None, 0, W * H, _ptr(out))
    return out


def test_a_null_distortion_is_hr_pixel_ray_bit_for_bit(hf):
    for name in FC.CASES:
        for ndc in (None, FC.NDC):
            assert np.array_equal(FC.host_rays(hf, name, None, ndc).view(np.uint32), _pinhole(hf, name, ndc).view(np.uint32)), (name, ndc)


def test_the_zero_pair_equals_hr_pixel_ray_bit_for_bit(hf):
    """... and a tiny coefficient is the way to ask for the plain equidistant lens: that does move the pixels."""
    for name in FC.CASES:
        for ndc in (None, FC.NDC):
            assert np.array_equal(FC.host_rays(hf, name, (0.0, 0.0), ndc).view(np.uint32), _pinhole(hf, name, ndc).view(np.uint32)), (name, ndc)
    lens = FC.host_rays(hf, 'short_focal', (1e-30, 0.0), None)
    assert float(np.abs(lens - _pinhole(hf, 'short_focal', None)).max()) > 0.1


def _true_theta(pair, theta_d32):
    return FC.solve_theta(pair[0], pair[1], theta_d32.astype(np.float64), np.float64)


def test_round_trip_theta_to_theta_d_and_back(hf):
    """theta -> theta_d through the polynomial (float64, rounded to float32) -> the header's theta.  The bound: the float32 residual
    theta (1 + k1 theta^2 + k2 theta^4) - theta_d carries about three roundings of half an ulp of theta_d, Newton's fixed point sits
    within that over f' >= 0.8875 (the smallest over the pairs) of the root, and the update rounds once more: (1.5 / 0.8875 + 0.5) ulp
    = 2.2 ulp, plus the polynomial's inner roundings -- 4 ulp of max(theta, theta_d)."""
    theta = np.linspace(0.0, 1.3, 200001)
    steps = hf.hf_newton_steps()
    for k1, k2 in FC.PAIRS:
        td = (theta * (1 + k1 * theta ** 2 + k2 * theta ** 4)).astype(np.float32)
        td = td[td <= 1.3]
        got = np.empty_like(td)
        hf.hf_theta(k1, k2, _ptr(td), td.size, steps, _ptr(got))
        want = _true_theta((k1, k2), td)
        err = np.abs(got - want)
        bound = 4 * np.spacing(np.maximum(td, got)).astype(np.float64)
        print(f'({k1}, {k2}): |theta - root| max {float(err.max()):.3e}, worst ratio to its bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}', flush=True)
        assert (err <= bound).all()
        assert got[0] == 0.0
        if (k1, k2) == (0.0, 0.0):
            assert np.array_equal(got, td)


def test_the_step_count_is_where_the_iterate_stops_improving(hf):
    """The float32 iterate never comes to rest (the residual's rounding keeps moving it), so `no longer moves` is read as: its largest
    distance to the root has stopped shrinking, and further steps only walk the rounding cycle -- two iterates that are both within the
    round trip's 4 ulp of the root are within 8 ulp of each other.  Printed per pair.  On these ranges the plateau begins after 3 steps
    (2 leave 2.7e-5 for the strongest pair); the header takes 6, the margin for invertible pairs stronger than the tests'.  Asserted: 2
    steps are not enough, the plateau begins at or before the header's count, and beyond it nothing moves by more than the cycle."""
    steps = hf.hf_newton_steps()
    td = np.concatenate([np.linspace(0, 1.3, 100001), np.random.default_rng(0).uniform(0, 1.3, 100000)]).astype(np.float32)
    ulp = float(np.spacing(np.float32(1.3)))
    slowest = 0
    for k1, k2 in FC.PAIRS[1:]:
        want = _true_theta((k1, k2), td)
        it = []
        for s in range(steps + 7):
            out = np.empty_like(td)
            hf.hf_theta(k1, k2, _ptr(td), td.size, s, _ptr(out))
            it.append(out)
        err = [float(np.abs(o - want).max()) for o in it]
        print(f'({k1}, {k2}): max |theta - root| after 0.. steps: ' + ' '.join(f'{e:.2e}' for e in err), flush=True)
        plateau = min(err[steps:])
        slowest = max(slowest, next(s for s in range(len(err)) if err[s] <= plateau + ulp / 2))
        assert err[steps] <= plateau + ulp / 2
        for s in range(steps, steps + 6):
            assert float(np.abs(it[s + 1] - it[s]).max()) <= 8 * ulp
        if (k1, k2) == FC.PAIRS[3]:
            assert err[2] > 10 * plateau
    print(f'the plateau is reached after {slowest} steps; the header takes {steps}', flush=True)
    assert 2 < slowest <= steps


def test_the_tangent_of_ieee_operations(hf):
    x = np.linspace(0.0, 1.55, 1000001).astype(np.float32)
    got = np.empty_like(x)
    hf.hf_tan(_ptr(x), x.size, _ptr(got))
    want = np.tan(x.astype(np.float64))
    ulp = np.abs(got - want)[1:] / np.spacing(want[1:].astype(np.float32))
    print(f'hr_tan_quadrant on [0, 1.55]: max {float(ulp.max()):.3f} ulp', flush=True)
    assert got[0] == 0.0 and float(ulp.max()) <= 3.0


def test_non_invertible_pairs_are_refused(hf):
    for pair in FC.PAIRS:
        assert hf.hf_invertible(*pair) == 1, pair
    for pair in FC.NOT_INVERTIBLE:
        assert not FC.invertible(*pair) and hf.hf_invertible(*pair) == 0, pair
    rng = np.random.default_rng(3)
    pairs = np.stack([rng.uniform(-0.3, 0.3, 4000), rng.uniform(-0.06, 0.06, 4000)], -1).astype(np.float32)
    margin = np.array([(1 + 3 * float(a) * t ** 2 + 5 * float(b) * t ** 4).min() for a, b in pairs for t in [np.linspace(0, np.pi / 2, 20001)]])
    clear = np.abs(margin) > 1e-6                               # the grid and the closed form may differ only on the boundary itself
    got = np.array([hf.hf_invertible(float(a), float(b)) for a, b in pairs])
    assert clear.sum() > 3900 and 500 < got.sum() < 3500
    assert np.array_equal(got[clear] == 1, margin[clear] > 0)
    # the C ABI refuses them on the host, before any launch: these calls pass without a device, the buffer is never written
    L = lib.load()
    buf = np.full((16, 6), np.nan, np.float32)
    cam = FC.camera_of('centred')
    for pair in FC.NOT_INVERTIBLE:
        fe = hr_fisheye(*pair)
        assert L.hr_generate_rays_fisheye(C.byref(cam), C.byref(fe), None, 6, 0, 16, _ptr(buf), None) == -1
        assert 'not invertible' in L.hr_last_error().decode() and 'hr_generate_rays_fisheye' in L.hr_last_error().decode()
    good = hr_fisheye(0.03, 0.004)

    def refused(rc, word):
        msg = L.hr_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    refused(L.hr_generate_rays_fisheye(None, C.byref(good), None, 6, 0, 16, _ptr(buf), None), 'null')
    refused(L.hr_generate_rays_fisheye(C.byref(cam), C.byref(good), None, 6, 0, 16, None, None), 'null')
    refused(L.hr_generate_rays_fisheye(C.byref(cam), C.byref(good), None, 7, 0, 16, _ptr(buf), None), 'ray_dim')
    refused(L.hr_generate_rays_fisheye(C.byref(cam), C.byref(good), None, 6, 24 * 14 - 2, 4, _ptr(buf), None), 'pixel range')
    refused(L.hr_generate_rays_fisheye(C.byref(cam), C.byref(good), None, 6, -1, 4, _ptr(buf), None), 'pixel range')
    # a range whose first + n does not fit int64 is outside the image like any other; the three camera entries share the check, and
    # each message names its entry
    big = 2 ** 63 - 1
    refused(L.hr_generate_rays_fisheye(C.byref(cam), C.byref(good), None, 6, big, 4, _ptr(buf), None), 'hr_generate_rays_fisheye: pixel range')
    refused(L.hr_generate_rays_fisheye(C.byref(cam), C.byref(good), None, 6, 4, big, _ptr(buf), None), 'hr_generate_rays_fisheye: pixel range')
    refused(L.hr_generate_rays_ndc(C.byref(cam), None, 6, big, 4, _ptr(buf), None), 'hr_generate_rays_ndc: pixel range')
    refused(L.hr_generate_rays(C.byref(cam), 6, big, big, _ptr(buf), None), 'hr_generate_rays: pixel range')
    refused(L.hr_generate_rays(C.byref(cam), 5, 0, 4, _ptr(buf), None), 'hr_generate_rays: ray_dim')
    bad_ndc = data.make_ndc(dict(fx=0.0, fy=1.0, near=1.0, width=8, height=8))
    refused(L.hr_generate_rays_fisheye(C.byref(cam), C.byref(good), C.byref(bad_ndc), 6, 0, 4, _ptr(buf), None), 'hr_ndc')
    assert L.hr_generate_rays_fisheye(C.byref(cam), C.byref(good), None, 6, 5, 0, None, None) == 0          # an empty range: nothing to launch
    img = np.zeros((14, 24, 3), np.uint8)
    refused(L.hr_rayset_set_image_fisheye(None, 0, C.byref(cam), C.byref(good), 1, 0, _ptr(img)), 'null')
    assert np.isnan(buf).all()


def test_make_fisheye_and_the_set_arguments():
    assert data.make_fisheye(None) is None
    fe = data.make_fisheye((0.03, 0.004))
    assert isinstance(fe, hr_fisheye) and (fe.k1, fe.k2) == (np.float32(0.03), np.float32(0.004)) and data.make_fisheye(fe) is fe
    assert (data.make_fisheye(np.array([-0.05, 0.01], np.float32)).k1) == np.float32(-0.05)
    for bad in ((0.1,), (0.1, 0.2, 0.0, 0.0), (float('nan'), 0.0), 0.1):
        with pytest.raises(ValueError, match='two finite coefficients'):
            data.make_fisheye(bad)
    poses = np.tile(np.eye(4, dtype=np.float32)[:3], (2, 1, 1))
    imgs = np.zeros((2, 4, 4, 3), np.uint8)
    K = np.array([[4.0, 0, 2], [0, 4.0, 2], [0, 0, 1]])
    for bad in (np.zeros((3, 2)), np.zeros((2, 4)), np.zeros(2)):
        with pytest.raises(ValueError, match='distortions must be None or an'):
            data.DeviceRaySet(imgs, poses, K, None, None, (4, 4), distortions=bad)
    with pytest.raises(ValueError, match='two finite coefficients'):
        data.DeviceRaySet(imgs, poses, K, None, None, (4, 4), distortions=np.array([[0.0, 0.0], [np.inf, 0.0]]))
    # 'fisheye' was never a subsample rule: the name is still refused as one, and the refusal now points at distortions=
    with pytest.raises(NotImplementedError, match='distortions='):
        data.DeviceRaySet(imgs, poses, K, None, None, (4, 4), subsample='fisheye')


def test_entry_points_are_bound_and_exported(hf):
    assert lib.ABI_VERSION == 27
    bound = {name: (res, args) for name, res, args in lib.SYMBOLS}
    assert bound['hr_generate_rays_fisheye'] == (C.c_int, [C.POINTER(hr_camera), C.POINTER(hr_fisheye), C.POINTER(hr_ndc), C.c_int32, C.c_int64,
                                                           C.c_int64, C.c_void_p, C.c_void_p])
    assert bound['hr_rayset_set_image_fisheye'] == (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(hr_camera), C.POINTER(hr_fisheye), C.c_int32, C.c_int32,
                                                              C.c_void_p])
    L = lib.load()                                          # raises when the library does not export one of them
    assert L.hr_abi_version() == 27
    with open(os.path.join(HERE, '..', 'include', 'hyperreel_hip.h')) as fh:
        header = fh.read()
    for name in ('hr_generate_rays_fisheye', 'hr_rayset_set_image_fisheye'):
        assert f'int {name}(' in header
    assert [n for n, _ in hr_fisheye._fields_] == ['k1', 'k2'] and C.sizeof(hr_fisheye) == hf.hf_sizeof_fisheye() == 8
