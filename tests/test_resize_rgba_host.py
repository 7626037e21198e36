"""PIL's RGBA resize and the white composite without a GPU: hr_premultiply / hr_unpremultiply of hr_resize.h compiled for the host
against PIL's own conversions on all 65 536 (colour, alpha) pairs, the host two-pass between them against every fixture PIL wrote
(tools/make_resize_rgba_golden.py), the axis plans with 4 bytes per pixel, the refusals of the new arguments that need no device, and
the bindings."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

import resize_common as RC
import resize_rgba_common as RA
from hyperreel_amd import data
from hyperreel_amd import lib as hlib


def _pil():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


def test_premultiply_equals_pil_on_every_pair():
    pre, _ = RA.host_tables()
    c, a = np.mgrid[0:256, 0:256]
    assert np.array_equal(pre, (((c * a + 128) >> 8) + (c * a + 128)) >> 8)                  # the rule as the issue states it
    img = RA.all_pairs()
    want = RA.np_premultiply(img)
    Image = _pil()
    if Image is not None:
        pil = np.asarray(Image.fromarray(img, 'RGBA').convert('RGBa'))
        assert pil.tobytes() == want.tobytes()
        want = pil
    # channel 0 of the all-pairs image is (c, a) = (y, x): the table itself; the pixel form gives the whole image
    assert np.array_equal(want[..., 0], pre) and np.array_equal(want[..., 3], img[..., 3])
    got = img.copy()
    RA.host_lib().hrz4_premultiply_pixels(got.ctypes.data_as(C.c_void_p), 256 * 256)
    assert got.tobytes() == want.tobytes()


def test_unpremultiply_equals_pil_on_every_pair():
    _, un = RA.host_tables()
    img = RA.all_pairs()                                                                     # read as raw RGBa: c' > a' included
    want = RA.np_unpremultiply(img)
    Image = _pil()
    if Image is not None:
        pil = np.asarray(Image.frombytes('RGBa', (256, 256), img.tobytes()).convert('RGBA'))
        assert pil.tobytes() == want.tobytes()
        want = pil
    assert np.array_equal(want[..., 0], un)
    # the branches: copied at alpha 0 and 255, clamped where the colour exceeds the alpha, else the truncated quotient
    c = np.arange(256)
    assert np.array_equal(un[:, 0], c) and np.array_equal(un[:, 255], c)
    assert un[200, 100] == 255 and un[100, 200] == (255 * 100) // 200 and un[1, 2] == 127 and un[254, 254] == 255 and un[253, 254] == 253


@pytest.mark.parametrize('src_wh,dst_wh,filt', RA.CASES, ids=[RA.case_name(*c) for c in RA.CASES])
def test_host_resize_equals_the_fixture(src_wh, dst_wh, filt):
    f = RA.load(RA.case_name(src_wh, dst_wh, filt))
    assert RA.wh(f, 'src_wh') == src_wh and RA.wh(f, 'dst_wh') == dst_wh and str(f['filter']) == filt
    got, pre = RA.host_resize(f['src'], dst_wh, filt, want_premultiplied=True)
    assert got.shape == f['expected'].shape
    assert got.tobytes() == f['expected'].tobytes()
    if src_wh != dst_wh:
        assert np.array_equal(RA.reach(pre), f['reach'])
    if src_wh[0] * src_wh[1] <= 4096:                                  # the numpy statement too, where it is quick
        assert RA.np_resize(f['src'], dst_wh, filt).tobytes() == f['expected'].tobytes()


@pytest.mark.parametrize('src_wh,mid_wh,dst_wh,filt', RA.TWOSTEP)
def test_host_two_steps_equal_the_fixture(src_wh, mid_wh, dst_wh, filt):
    f = RA.load(RA.twostep_name(src_wh, mid_wh, dst_wh, filt))
    assert RA.wh(f, 'mid_wh') == mid_wh
    got = RA.host_resize(RA.host_resize(f['src'], mid_wh, filt), dst_wh, 'box')           # between the steps: un-premultiplied 8-bit RGBA
    assert got.tobytes() == f['expected'].tobytes()


def test_every_fixture_is_listed_small_and_both_branches_are_reached():
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(RA.GOLDEN, '*.npz')))
    want = sorted([RA.case_name(*c) for c in RA.CASES] + [RA.twostep_name(*c) for c in RA.TWOSTEP])
    assert names == want
    assert max(os.path.getsize(os.path.join(RA.GOLDEN, n + '.npz')) for n in names) < 128 * 1024
    reached = sum(RA.load(n)['reach'] for n in names)
    assert reached[0] > 0 and reached[1] > 0, reached
    # the cases the issue names reach both on their 0 / 255 content alone
    for name in (RA.case_name((65, 47), (32, 23), 'lanczos'), RA.case_name((17, 9), (40, 21), 'lanczos')):
        f = RA.load(name)
        _, pre = RA.host_resize(f['src'][1:2], RA.wh(f, 'dst_wh'), 'lanczos', want_premultiplied=True)
        assert (RA.reach(pre) > 0).all(), (name, RA.reach(pre))
    # an equal-size fixture is a copy: alpha 0 with a colour keeps its bytes
    f = RA.load(RA.case_name((12, 10), (12, 10), 'lanczos'))
    assert f['expected'].tobytes() == f['src'].tobytes() and ((f['src'][..., 3] == 0) & (f['src'][..., :3].max(-1) > 0)).any()


@pytest.mark.parametrize('filt', RA.FILTERS)
def test_host_resize_equals_live_pil(filt):
    pytest.importorskip('PIL')
    rng = np.random.default_rng(11)
    for (w, h), (w2, h2) in [((37, 29), (16, 11)), ((16, 11), (37, 29)), ((50, 31), (50, 7)), ((50, 31), (123, 31)), ((31, 31), (31, 31))]:
        img = rng.integers(0, 256, (2, h, w, 4), dtype=np.uint8)
        img[1] = (img[1] >> 7) * 255
        assert RA.host_resize(img, (w2, h2), filt).tobytes() == RA.pil_resize(img, (w2, h2), filt).tobytes(), ((w, h), (w2, h2))


def test_plans_with_four_bytes_a_pixel_fit_their_lds_budget():
    seen = []
    for (w, h), (w2, h2) in RA.SHAPES:
        for a in ((w, w2), (h, h2)):
            if a[0] != a[1] and a not in seen:
                seen.append(a)
    staged = {}
    for vertical in (0, 1):
        for n_in, n_out in seen + RC.AXES + [(800, 400)]:
            for filt in RA.FILTERS:
                bounds, k = RC.host_coeffs(n_in, n_out, filt)
                p3, p4 = RC.host_axis_plan(vertical, bounds, k.shape[1]), RA.host_axis_plan(vertical, bounds, k.shape[1], 4)
                assert RA.host_axis_plan(vertical, bounds, k.shape[1], 3) == p3                      # the default is 3 bytes: nothing moved
                assert not p4['staged'] or 0 < p4['lds_bytes'] <= 20 * 1024
                if vertical:
                    assert p4 == p3                                                                   # a vertical tile spans bytes
                elif p4['staged']:
                    assert p4['row_pitch'] % 16 == 0 and p4['row_pitch'] >= p4['span'] * 4 + 15
                    assert p4['lds_bytes'] == 64 * k.shape[1] * 4 + 4 * p4['row_pitch']
                staged[(vertical, n_in, n_out, filt)] = p4['staged']
    # the paths the fixtures take with 4 bytes a pixel: staged and general, on both axes; Blender's 800 -> 400 is staged
    assert staged[(0, 264, 33, 'lanczos')] == 1 and staged[(1, 200, 25, 'lanczos')] == 1
    assert staged[(0, 100, 7, 'lanczos')] == 0 and staged[(1, 100, 7, 'lanczos')] == 0
    assert staged[(0, 800, 400, 'lanczos')] == 1 and staged[(1, 800, 400, 'lanczos')] == 1
    # a wide span that 3-byte pixels still stage and 4-byte pixels do not: the choice follows the bytes of a pixel
    bounds, k = RC.host_coeffs(4032, 504, 'lanczos')
    assert RC.host_axis_plan(0, bounds, k.shape[1])['staged'] == 1
    p4 = RA.host_axis_plan(0, bounds, k.shape[1], 4)
    assert p4['staged'] == (64 * k.shape[1] * 4 + 4 * ((p4['span'] * 4 + 30) // 16 * 16) <= 20 * 1024)


def test_refusals_without_a_device():
    rgb, rgba = np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 4), np.uint8)
    for mode in ('LA', 'rgba', 'L', 4, None):
        with pytest.raises(ValueError, match='mode'):
            data.DeviceResize((4, 4), (2, 2), mode=mode)
        with pytest.raises(ValueError, match='mode'):
            data.reference_resize(rgba, (2, 2), mode=mode)
    with pytest.raises(ValueError, match='8-bit RGBA'):                # wrong channel count for the mode, both ways
        data.reference_resize(rgb, (2, 2), mode='RGBA')
    with pytest.raises(ValueError, match='8-bit RGB;'):
        data.reference_resize(rgba, (2, 2))
    with pytest.raises(ValueError, match='8-bit RGB;'):
        data.reference_resize(rgba, (2, 2), mode='RGB')
    with pytest.raises(ValueError, match='made for 5 x 4'):
        data._as_u8_batch(rgba, (5, 4), channels=4)
    assert tuple(data._as_u8_batch(rgba, (4, 4), channels=4).shape) == (1, 4, 4, 4)
    with pytest.raises(ValueError, match='filter'):
        data.DeviceResize((4, 4), (2, 2), filter='nearest', mode='RGBA')

    poses = np.tile(np.eye(4, dtype=np.float32)[:3], (2, 1, 1))
    K = np.array([[30, 0, 2], [0, 30, 2], [0, 0, 1]], np.float32)
    with pytest.raises(ValueError, match='alpha'):
        data.DeviceRaySet(np.zeros((2, 4, 4, 4), np.uint8), poses, K, None, None, (4, 4), alpha='black')
    with pytest.raises(ValueError, match=r'expected uint8 \(4, 4, 4\)'):           # alpha='white' with (H, W, 3) images
        data.DeviceRaySet(np.zeros((2, 4, 4, 3), np.uint8), poses, K, None, None, (4, 4), alpha='white')
    with pytest.raises(ValueError, match='importance'):                            # an importance rule on an RGBA set
        data.DeviceRaySet(np.zeros((2, 4, 4, 4), np.uint8), poses, K, None, None, (4, 4), alpha='white', subsample=[(1, 0), data.Importance(3)])
    lf = data.make_lightfield(4, 4)
    with pytest.raises(ValueError, match='alpha'):
        data.DeviceRaySet.from_lightfield(np.zeros((2, 4, 4, 4), np.uint8), [(0, 0), (1, 0)], lf, alpha=1)
    with pytest.raises(ValueError, match=r'expected uint8 \(4, 4, 4\)'):
        data.DeviceRaySet.from_lightfield(np.zeros((2, 4, 4, 3), np.uint8), [(0, 0), (1, 0)], lf, alpha='white')

    with pytest.raises(ValueError, match='uint8'):
        data.composite_white(torch.zeros((2, 2, 4)))
    with pytest.raises(ValueError, match='uint8'):
        data.composite_white(torch.zeros((2, 2, 3), dtype=torch.uint8))


def _rule5(rgba_u8):
    """the reference's expression on the host (datasets/blender.py:61-70): ToTensor, then img[:, :3] * img[:, -1:] + (1 - img[:, -1:])"""
    img = torch.from_numpy(np.array(rgba_u8)).reshape(-1, 4).float().div(255)          # (a copy: fixtures are read-only)
    return img[:, :3] * img[:, -1:] + (1 - img[:, -1:])


def test_composite_white_has_the_reference_bits_on_every_pair():
    img = RA.all_pairs()
    got = data.composite_white(torch.from_numpy(img))
    assert got.dtype == torch.float32 and tuple(got.shape) == (65536, 3)
    assert torch.equal(got.view(torch.int32), _rule5(img).view(torch.int32))
    # what the rule is not: the multiplication by 1 / 255, and the contracted multiply-add
    x = img.reshape(-1, 4).astype(np.float32)
    assert int((x * np.float32(1 / 255) != x / np.float32(255)).sum()) > 0
    c, a = (x[:, :3] / np.float32(255)).astype(np.float64), (x[:, 3:] / np.float32(255))
    fused = (c * a.astype(np.float64) + (np.float32(1) - a).astype(np.float64)).astype(np.float32)     # one rounding: an fma's result
    assert int((fused != got.numpy()).sum()) > 0


def test_entry_points_are_bound_and_exported():
    names = [s[0] for s in hlib.SYMBOLS]
    for name in ('hr_resize_plan_create_rgba', 'hr_rayset_set_pixel_format'):
        assert names.count(name) == 1
    L = hlib.load()
    assert L.hr_abi_version() == 27 and hlib.ABI_VERSION == 27
    assert L.hr_resize_plan_create_rgba.argtypes == [C.c_int32] * 6 + [C.POINTER(C.c_void_p)] and L.hr_resize_plan_create_rgba.restype is C.c_int
    assert L.hr_rayset_set_pixel_format.argtypes == [C.c_void_p, C.c_int32] and L.hr_rayset_set_pixel_format.restype is C.c_int
    assert (hlib.HR_PIXELS_RGB8, hlib.HR_PIXELS_RGBA8_WHITE) == (0, 1)
    header = open(os.path.join(RC.HERE, '..', 'include', 'hyperreel_hip.h')).read()
    for name in ('hr_resize_plan_create_rgba', 'hr_rayset_set_pixel_format'):
        assert name + '(' in header
    assert 'HR_PIXELS_RGB8 = 0, HR_PIXELS_RGBA8_WHITE = 1' in header and '#define HR_ABI_VERSION 27' in header
    # the argument checks come before any device work
    h = C.c_void_p()
    for args, word in (((0, 4, 2, 2, 1, 1), 'source size'), ((4, 4, 2, 0, 1, 1), 'destination size'), ((4, 4, 2, 2, 0, 1), 'filter'),
                       ((4, 4, 2, 2, 1, 0), 'max_images'), (((1 << 20) + 1, 4, 2, 2, 1, 1), 'beyond')):
        assert L.hr_resize_plan_create_rgba(*args, C.byref(h)) == -1 and not h.value
        assert word in L.hr_last_error().decode(), (args, L.hr_last_error())
    assert L.hr_resize_plan_create_rgba(4, 4, 2, 2, 1, 1, None) == -1 and 'out' in L.hr_last_error().decode()
    assert L.hr_rayset_set_pixel_format(None, 1) == -1 and 'null set' in L.hr_last_error().decode()
