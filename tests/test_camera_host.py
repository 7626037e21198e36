"""CPU check of hyperreel_amd/csrc/hr_camera.h -- the arithmetic of hr_generate_rays_ndc and hr_rayset_batch, compiled for the
host by g++ into a test-only library -- against the reference's own rays (tests/golden/camera, tools/make_camera_golden.py),
a brute-force subsample mask, and exhaustive bijection counts; and of DeviceRaySet.video_rule against the reference's running
offsets.  The kernels' indexing, stores and the set's tables are covered by tests/test_gpu_rays.py.

Tolerance: camera_common.py derives it from the fixtures (4 x the reference's own float32-to-float64 distance, capped at 1e-5).
Measured: the reference lies 4.2e-7 (origins) / 3.9e-7 (directions) from float64, so the bars are 1.7e-6 / 1.5e-6; the header
lies 4.8e-7 / 4.8e-7 from the reference and 4.2e-7 / 3.7e-7 from float64 -- as close to the exact value as the reference is.  It
follows the reference's operation order, but not to the bit: the pinhole direction already differs by one ulp (1.2e-7: torch's matmul
and F.normalize sum in another order, the 2e-7 of tests/test_gpu_parity.py), and NDC carries that through its divisions."""
import ctypes as C
import os

import numpy as np
import pytest

import camera_common as CC
from hyperreel_amd import scenes
from hyperreel_amd.plan import hr_camera, hr_ndc


@pytest.fixture(scope='module')
def hc():
    return CC.host_lib()


def test_struct_layouts_match_c(hc):
    assert hc.hc_sizeof_camera() == C.sizeof(hr_camera) and hc.hc_sizeof_ndc() == C.sizeof(hr_ndc) == 20


def test_fixtures_are_the_expected_set():
    assert CC.fixture_names() == sorted(CC.CASES)
    for name in CC.CASES:
        f = CC.load(name)
        assert f['all_inputs'].dtype == np.float32 and f['all_inputs'].shape == (f['coords64'].shape[0], CC.ray_dim(f) + 4)
        assert os.path.getsize(os.path.join(CC.GOLDEN, f'{name}.npz')) < 1 << 20
    f = CC.load('ndc_other_size')                       # the NDC's dataset size differs from the generated frame's
    assert (int(f['ndc'][3]), int(f['ndc'][4])) != (int(f['img_wh'][0]), int(f['img_wh'][1]))


def test_pinhole_rays_match_scenes(hc):
    """hr_pixel_ray without NDC == get_ray_directions_K(centered) + get_rays as restated in scenes.pinhole_rays, within the
    2e-7 the device test of hr_generate_rays holds (tests/test_gpu_parity.py)."""
    from hyperreel_amd.data import make_camera
    for (H, W, fov) in [(40, 56, 40.0), (47, 61, 65.0)]:
        pose = scenes.look_at_pose((0.3, 0.1, -0.2), (1.0, 0.4, 0.3))
        focal = np.float32(0.5 * W / np.tan(0.5 * np.radians(fov)))
        K = np.array([[focal, 0, W / 2.0], [0, focal, H / 2.0], [0, 0, 1]], np.float32)
        cam = make_camera(pose, K, W, H)
        got = np.empty((H * W, 6), np.float32)
        hc.hc_pixel_rays(C.byref(cam), None, 0, H * W, got.ctypes.data_as(C.c_void_p))
        ref = scenes.pinhole_rays(H, W, fov, pose)
        assert float(np.abs(got - ref).max()) <= 2e-7


def test_ndc_rays_against_the_reference(hc):
    dist = CC.reference_distances()
    bars = CC.bars()
    print(f"reference |fp32 - fp64|: origins {dist['origins']:.3e}, directions {dist['directions']:.3e}; bars {bars['origins']:.3e} / {bars['directions']:.3e}")
    assert 0.0 < bars['origins'] <= CC.CAP and 0.0 < bars['directions'] <= CC.CAP
    assert 4.0 * max(dist.values()) <= CC.CAP          # no fixture camera is ill-conditioned (a d_z near zero)
    for name in CC.CASES:
        f = CC.load(name)
        got = CC.host_rays(hc, f)
        ref = f['all_inputs'][:, :6]
        assert got.shape == ref.shape
        d_o, d_d = float(np.abs(got[:, :3] - ref[:, :3]).max()), float(np.abs(got[:, 3:] - ref[:, 3:]).max())
        d64_o = float(np.abs(got[:, :3].astype(np.float64) - f['coords64'][:, :3]).max())
        d64_d = float(np.abs(got[:, 3:].astype(np.float64) - f['coords64'][:, 3:]).max())
        print(f'{name}: header vs reference origins {d_o:.3e} directions {d_d:.3e}; header vs float64 origins {d64_o:.3e} directions {d64_d:.3e}')
        assert d_o <= bars['origins'] and d_d <= bars['directions'], name
        assert d64_o <= bars['origins'] and d64_d <= bars['directions'], name


def _brute(w, h, every, offset):
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    m = ((x + y + offset) % every) == 0
    return np.stack([x[m], y[m]], -1).astype(np.int32)          # row-major order


def test_subsample_closed_form_exhaustive(hc):
    checked = 0
    for w in range(1, 21):
        for h in range(1, 21):
            for every in range(1, 10):
                for offset in range(0, 2 * every + 1):
                    ref = _brute(w, h, every, offset)
                    n = hc.hc_subsample_count(w, h, every, offset)
                    assert n == len(ref), (w, h, every, offset)
                    got = np.empty((n, 2), np.int32)
                    hc.hc_subsample_pixels(w, h, every, offset, 0, n, got.ctypes.data_as(C.c_void_p))
                    assert np.array_equal(got, ref), (w, h, every, offset)
                    checked += 1
    assert checked == 20 * 20 * sum(2 * e + 1 for e in range(1, 10))


@pytest.mark.parametrize('w,h', [(2048, 1088), (1352, 1014)])
@pytest.mark.parametrize('every', [1, 4, 8, 10, 50])      # the shipped fractions: 1, 0.25, 0.125 (technicolor), 0.1, 0.02 (neural_3d)
def test_subsample_closed_form_shipped_sizes(hc, w, h, every):
    for offset in (0, 1, every - 1, every, 3 * every + 2, 799):
        ref = _brute(w, h, every, offset)
        n = hc.hc_subsample_count(w, h, every, offset)
        assert n == len(ref)
        got = np.empty((n, 2), np.int32)
        hc.hc_subsample_pixels(w, h, every, offset, 0, n, got.ctypes.data_as(C.c_void_p))
        assert np.array_equal(got, ref)


KEYS = [(0, 0), (0, 1), (12345, 7)]


def test_perm_is_a_bijection(hc):
    keys = [hc.hc_perm_key(s, e) for s, e in KEYS]
    assert len(set(keys)) == 3
    for key in keys:
        assert hc.hc_perm_not_bijective(1, 4097, key) == 0
        for n in (65521, 65537, 1048573, 1048583):           # primes on both sides of 2^16 and 2^20
            assert hc.hc_perm_not_bijective(n, n, key) == 0
    # index 0 .. n-1 never maps outside [0, n), and different (seed, epoch) give different orders
    n = 1048583
    orders = []
    for key in keys:
        out = np.empty(n, np.uint64)
        hc.hc_perm(n, key, 0, n, out.ctypes.data_as(C.c_void_p))
        assert int(out.max()) == n - 1 and int(out.min()) == 0
        assert np.array_equal(np.sort(out), np.arange(n, dtype=np.uint64))
        orders.append(out)
    for a in range(3):
        for b in range(a + 1, 3):
            assert float((orders[a] == orders[b]).mean()) < 1e-3
    assert float((orders[0] == np.arange(n, dtype=np.uint64)).mean()) < 1e-3          # and none is the identity
    # beyond 2^30: spot rows of the technicolor-shaped set stay inside
    big = 800 * 2048 * 1088
    out = np.empty(4096, np.uint64)
    for first in (0, big // 2, big - 4096):
        hc.hc_perm(big, keys[0], first, 4096, out.ctypes.data_as(C.c_void_p))
        assert int(out.max()) < big and len(np.unique(out)) == 4096


def test_video_rule_reproduces_the_fixtures():
    from hyperreel_amd.data import DeviceRaySet
    seen = 0
    for name in CC.CASES:
        f = CC.load(name)
        if 'rule' not in f:
            continue
        full, key, kfrac, frac = int(f['rule'][0]), int(f['rule'][1]), float(f['rule'][2]), float(f['rule'][3])
        rules = DeviceRaySet.video_rule(f['frames'], load_full_step=full, subsample_keyframe_step=key, subsample_keyframe_frac=kfrac,
                                        subsample_frac=frac)
        assert rules == [(int(e), int(o)) for e, o in f['rules']], name
        assert sum(hi - lo for lo, hi in CC.image_rows(f)) == f['all_inputs'].shape[0]
        seen += 1
    assert seen == 2
    f = CC.load('video_ndc')                                    # 3 cameras x 9 frames, steps 8 / 4, fractions 0.25 / 0.125
    every = [int(e) for e, _ in f['rules']]
    assert every[:3] == [1, 1, 1] and every[12:15] == [4, 4, 4] and every[3:6] == [8, 8, 8] and every[24:] == [1, 1, 1]
    assert [int(o) for _, o in f['rules'][12:15]] == [0, 1, 2] and [int(o) for _, o in f['rules'][3:12]] == list(range(9))
    for rule in ('random_subsample', 'importance_subsample', 'fisheye'):
        with pytest.raises(NotImplementedError, match=rule):
            DeviceRaySet.video_rule([0, 1], rule=rule)
        with pytest.raises(NotImplementedError, match=rule):
            DeviceRaySet(None, None, None, None, None, (4, 4), subsample=rule)
    for rule in (None, b'regular_subsample', 3):              # anything that is not the one supported name, a string or not
        with pytest.raises(NotImplementedError, match='not supported'):
            DeviceRaySet.video_rule([0, 1], rule=rule)


@pytest.mark.reference
@pytest.mark.parametrize('name', ['video_ndc'])
def test_fixture_regenerates_bit_for_bit(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_camera_golden', os.path.join(CC.HERE, '..', 'tools', 'make_camera_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    new, old = mod.make_case(name), CC.load(name)
    assert sorted(new) == sorted(old)
    for k in old:
        a, b = np.asarray(new[k]), old[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
