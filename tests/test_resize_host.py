"""PIL's 8-bit resize without a GPU: hr_resize.h compiled for the host against a numpy statement of the arithmetic, against the fixtures
PIL wrote (tools/make_resize_golden.py) and against PIL itself where it imports; the accumulator check; which kernel an axis gets; the
refusals of DeviceResize / reference_resize that need no device; the bindings."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import resize_common as RC
from hyperreel_amd import data
from hyperreel_amd import lib as hlib

CASES = [(s, d, f) for s, d in RC.SHAPES for f in RC.FILTERS]


def _axes():
    """every axis of a fixture that a pass runs on, and the further ones"""
    seen = []
    for (w, h), (w2, h2) in RC.SHAPES:
        for a in ((w, w2), (h, h2)):
            if a[0] != a[1] and a not in seen:
                seen.append(a)
    return seen + RC.AXES


@pytest.mark.parametrize('filt', RC.FILTERS)
def test_coefficients_equal_the_numpy_statement(filt):
    for n_in, n_out in _axes():
        bounds, k = RC.host_coeffs(n_in, n_out, filt)
        ref_bounds, ref_k = RC.np_coeffs(n_in, n_out, filt)
        assert k.shape == ref_k.shape, (n_in, n_out)
        assert np.array_equal(bounds, ref_bounds), (n_in, n_out)
        assert np.array_equal(k, ref_k), (n_in, n_out)
        # a row's taps stay inside the axis, rows are zero past their n, and the bounds never step back
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= n_in).all() and (bounds[:, 1] <= k.shape[1]).all()
        assert all((k[i, bounds[i, 1]:] == 0).all() for i in range(n_out))
        assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(1)) >= 0).all()


def test_ksize_of_the_named_cases():
    assert RC.host_coeffs(264, 33, 'lanczos')[1].shape[1] == 49       # the LLFF ratio
    assert RC.host_coeffs(4032, 504, 'lanczos')[1].shape[1] == 49
    assert RC.host_coeffs(100, 7, 'lanczos')[1].shape[1] == 87
    assert RC.host_coeffs(2704, 1352, 'lanczos')[1].shape[1] == 13
    assert RC.host_coeffs(16, 37, 'lanczos')[1].shape[1] == 7         # enlargement: the filter's own support
    assert RC.host_coeffs(16, 37, 'box')[1].shape[1] == 3
    lib = RC.host_lib()
    assert lib.hrz_ksize(0, 4, 1) == 0 and lib.hrz_ksize(4, 0, 1) == 0 and lib.hrz_ksize(4, 4, 0) == 0 and lib.hrz_ksize(4, 4, 5) == 0


@pytest.mark.parametrize('src_wh,dst_wh,filt', CASES, ids=[RC.case_name(*c) for c in CASES])
def test_host_two_pass_equals_the_fixture(src_wh, dst_wh, filt):
    f = RC.load(RC.case_name(src_wh, dst_wh, filt))
    assert RC.wh(f, 'src_wh') == src_wh and RC.wh(f, 'dst_wh') == dst_wh and str(f['filter']) == filt
    got = RC.host_resize(f['src'], dst_wh, filt)
    assert got.shape == f['expected'].shape
    assert got.tobytes() == f['expected'].tobytes()
    if src_wh[0] * src_wh[1] <= 4096:                                  # the numpy statement too, where it is quick
        assert RC.np_resize(f['src'], dst_wh, filt).tobytes() == f['expected'].tobytes()


@pytest.mark.parametrize('src_wh,mid_wh,dst_wh,filt', RC.TWOSTEP)
def test_host_two_steps_equal_the_fixture(src_wh, mid_wh, dst_wh, filt):
    f = RC.load(RC.twostep_name(src_wh, mid_wh, dst_wh, filt))
    assert RC.wh(f, 'mid_wh') == mid_wh
    got = RC.host_resize(RC.host_resize(f['src'], mid_wh, filt), dst_wh, 'box')
    assert got.tobytes() == f['expected'].tobytes()


def test_every_fixture_is_listed_and_small():
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(RC.GOLDEN, '*.npz')))
    want = sorted([RC.case_name(*c) for c in CASES] + [RC.twostep_name(*c) for c in RC.TWOSTEP])
    assert names == want
    assert max(os.path.getsize(os.path.join(RC.GOLDEN, n + '.npz')) for n in names) < 64 * 1024


@pytest.mark.parametrize('filt', RC.FILTERS)
def test_host_two_pass_equals_live_pil(filt):
    pytest.importorskip('PIL')
    rng = np.random.default_rng(5)
    for (w, h), (w2, h2) in [((37, 29), (16, 11)), ((16, 11), (37, 29)), ((50, 31), (123, 7)), ((123, 77), (50, 31)), ((300, 2), (19, 2)), ((2, 300), (2, 19)),
                             ((64, 64), (8, 8)), ((31, 31), (31, 31))]:
        img = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
        img[1] = (img[1] >> 7) * 255
        assert RC.host_resize(img, (w2, h2), filt).tobytes() == RC.pil_resize(img, (w2, h2), filt).tobytes(), ((w, h), (w2, h2))


def test_accumulator_check():
    worst = 0
    for filt in RC.FILTERS:
        for n_in, n_out in _axes():
            k = RC.host_coeffs(n_in, n_out, filt)[1]
            verdict, bad = RC.host_check(k)
            assert verdict == RC.FIT_MAD24 and bad == -1, (filt, n_in, n_out)        # int32 holds, and so does the 24-bit multiply-add
            worst = max(worst, int(np.abs(k.astype(np.int64)).sum(1).max()))
    print(f'largest sum|k| of a row: {worst / (1 << 22):.4f} * 2^22 -> 255 * sum + 2^21 = {255 * worst + (1 << 21):.4e} (2^31 = {2 ** 31:.4e})', flush=True)
    assert 255 * worst + (1 << 21) < 2 ** 31
    # hand-made rows: the bound itself, one short of it, one coefficient too wide for 24 bits
    limit = (2 ** 31 - 2 ** 21 - 1) // 255                        # the largest sum|k| with 255 * sum + 2^21 < 2^31
    fine = np.array([[1 << 22, 0, 0], [limit - 5, -5, 0]], np.int32)
    assert RC.host_check(fine) == (RC.ROWS_OK, -1)                # holds, but |k| >= 2^23: no 24-bit form
    over = np.array([[1 << 22, 0, 0], [limit - 5, -6, 0], [1 << 30, 1 << 30, 1 << 30]], np.int32)
    assert RC.host_check(over) == (RC.OVERFLOW, 1)
    assert RC.host_check(np.array([[(1 << 23) - 1, -5], [5, -(1 << 23) + 1]], np.int32)) == (RC.FIT_MAD24, -1)
    assert RC.host_check(np.array([[-(1 << 23), 5]], np.int32)) == (RC.ROWS_OK, -1)


def test_which_kernel_serves_an_axis():
    def plan(vertical, n_in, n_out, filt='lanczos'):
        bounds, k = RC.host_coeffs(n_in, n_out, filt)
        p = RC.host_axis_plan(vertical, bounds, k.shape[1])
        for tile in ([p['tile']] if p['staged'] else []):         # the span is the most any tile reads
            assert p['span'] == max(int(bounds[min(i + tile, n_out) - 1].sum() - bounds[i, 0]) for i in range(0, n_out, tile))
        return p

    assert plan(0, 264, 33)['staged'] == 1 and plan(0, 4032, 504)['staged'] == 1 and plan(0, 2704, 1352)['staged'] == 1
    assert plan(0, 100, 7)['staged'] == 0                         # ksize 87: 64 coefficient rows alone pass the budget
    assert plan(1, 200, 25)['staged'] == 1 and plan(1, 3024, 378) == dict(plan(1, 3024, 378), staged=1, tile=4)    # LLFF: 49 + 3 * 8 rows
    assert plan(1, 100, 7)['staged'] == 0                         # 87 rows of 272 bytes pass it
    assert plan(1, 1030, 515)['tile'] == 8 and plan(1, 11, 29)['tile'] == 8
    for vertical in (0, 1):
        for n_in, n_out in _axes():
            for filt in RC.FILTERS:
                p = plan(vertical, n_in, n_out, filt)
                assert not p['staged'] or 0 < p['lds_bytes'] <= 20 * 1024
                assert not p['staged'] or vertical or (p['row_pitch'] % 16 == 0 and p['row_pitch'] >= p['span'] * 3 + 15)


def test_refusals_without_a_device():
    for bad in ((0, 4), (4, 0), (-1, 4), (4,), 7, (2.5, 4), None):
        with pytest.raises(ValueError, match='src_wh'):
            data.DeviceResize(bad, (4, 4))
        with pytest.raises(ValueError, match='dst_wh'):
            data.DeviceResize((4, 4), bad)
        with pytest.raises(ValueError, match='_img_wh'):
            data.reference_resize(np.zeros((4, 4, 3), np.uint8), bad)
    for filt in ('nearest', 'hamming', 'LANCZOS', 1, None):
        with pytest.raises(ValueError, match='filter'):
            data.DeviceResize((4, 4), (2, 2), filter=filt)
        with pytest.raises(ValueError, match='filter'):
            data.reference_resize(np.zeros((4, 4, 3), np.uint8), (2, 2), first=filt)
    for n in (0, -2):
        with pytest.raises(ValueError, match='max_images'):
            data.DeviceResize((4, 4), (2, 2), max_images=n)
    with pytest.raises(ValueError, match='img_wh'):
        data.reference_resize(np.zeros((4, 4, 3), np.uint8), (2, 2), img_wh=(0, 1))
    for images in (np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4), np.uint8), np.zeros((0, 4, 4, 3), np.uint8),
                   np.zeros((1, 1, 4, 4, 3), np.uint8)):
        with pytest.raises(ValueError, match='8-bit RGB'):
            data.reference_resize(images, (2, 2))
    with pytest.raises(ValueError, match='made for 5 x 4'):
        data._as_u8_batch(np.zeros((4, 4, 3), np.uint8), (5, 4))
    import torch
    with pytest.raises(ValueError, match='uint8'):
        data.as_float(torch.zeros((2, 2, 3)))
    x = torch.arange(24, dtype=torch.uint8).reshape(1, 2, 4, 3)
    got = data.as_float(x)
    assert got.shape == (8, 3) and got.dtype == torch.float32 and torch.equal(got, x.reshape(-1, 3).float() / 255)
    assert 'cv2.resize' in data.DeviceResize.__doc__ and 'reducing_gap' in data.DeviceResize.__doc__


def test_entry_points_are_bound_and_exported():
    names = [s[0] for s in hlib.SYMBOLS]
    for name in ('hr_resize_plan_create', 'hr_image_resize', 'hr_resize_plan_destroy'):
        assert names.count(name) == 1
    L = hlib.load()
    assert L.hr_abi_version() == 27 and hlib.ABI_VERSION == 27
    assert L.hr_resize_plan_create.argtypes == [C.c_int32] * 6 + [C.POINTER(C.c_void_p)]
    assert L.hr_image_resize.restype is C.c_int and L.hr_resize_plan_destroy.restype is None
    header = open(os.path.join(RC.HERE, '..', 'include', 'hyperreel_hip.h')).read()
    for name in ('hr_resize_plan_create', 'hr_image_resize', 'hr_resize_plan_destroy'):
        assert name + '(' in header
    assert '#define HR_ABI_VERSION 27' in header
    # the argument checks come before any device work
    h = C.c_void_p()
    for args, word in (((0, 4, 2, 2, 1, 1), 'source size'), ((4, 4, 2, 0, 1, 1), 'destination size'), ((4, 4, 2, 2, 0, 1), 'filter'),
                       ((4, 4, 2, 2, 5, 1), 'filter'), ((4, 4, 2, 2, 1, 0), 'max_images'), (((1 << 20) + 1, 4, 2, 2, 1, 1), 'beyond')):
        assert L.hr_resize_plan_create(*args, C.byref(h)) == -1 and not h.value
        assert word in L.hr_last_error().decode(), (args, L.hr_last_error())
    assert L.hr_resize_plan_create(4, 4, 2, 2, 1, 1, None) == -1 and 'out' in L.hr_last_error().decode()
    assert L.hr_image_resize(None, None, 1, None, None) == -1 and 'plan' in L.hr_last_error().decode()
    L.hr_resize_plan_destroy(None)
