"""`-m gpu`: hr_resize_plan_create_rgba / hr_image_resize / DeviceResize(mode='RGBA') / reference_resize(mode='RGBA') against the bytes
PIL wrote for RGBA images (tests/golden/resize_rgba, tools/make_resize_rgba_golden.py).  Equality of bytes, no tolerance anywhere.
Every fixture runs as one batch of three images (random bytes, random 0 / 255, an alpha checkerboard) from a source at a 16-byte
boundary and from sources 4 and 12 bytes past one (RGBA pixels are read as aligned words: a source is 4-byte aligned); the fixtures
cover the staged and the general kernel on both axes, each axis alone, and the copy (tests/resize_rgba_common.py SHAPES).  Nothing here
provokes a fault: the refused calls are refused on the host before anything is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import resize_common as RC
import resize_rgba_common as RA
from hyperreel_amd import data
from hyperreel_amd import lib as _lib
from hyperreel_amd.data import DeviceResize, reference_resize

pytestmark = pytest.mark.gpu


def _same(got, expected):
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == expected.shape
    bad = int((got != expected).sum())
    assert bad == 0, f'{bad} of {expected.size} bytes differ'


def _shifted(images, shift):
    """the images in device memory, their first byte `shift` bytes past an allocation's start"""
    flat = torch.from_numpy(np.array(images)).reshape(-1)
    buf = torch.zeros(flat.numel() + 32, dtype=torch.uint8, device='cuda')
    buf[shift:shift + flat.numel()] = flat.cuda()
    return buf[shift:shift + flat.numel()].view(images.shape)


@pytest.mark.parametrize('src_wh,dst_wh,filt', RA.CASES, ids=[RA.case_name(*c) for c in RA.CASES])
def test_bytes_equal_pil(src_wh, dst_wh, filt):
    f = RA.load(RA.case_name(src_wh, dst_wh, filt))
    r = DeviceResize(src_wh, dst_wh, filt, max_images=3, mode='RGBA')
    try:
        got = r(f['src'])                                             # numpy on the host: a fresh, aligned device copy
        assert got.is_cuda and tuple(got.shape) == (3, dst_wh[1], dst_wh[0], 4)
        _same(got, f['expected'])
        for shift in (4, 12):
            src = _shifted(f['src'], shift)
            assert src.data_ptr() % 16 == shift
            _same(r(src), f['expected'])
    finally:
        r.close()


def test_the_named_cases_take_the_kernel_they_are_for():
    """which kernel a fixture's axis runs on is hr_resize.h's decision: the host build answers, with 4 bytes a pixel"""
    def staged(vertical, n_in, n_out):
        bounds, k = RC.host_coeffs(n_in, n_out, 'lanczos')
        return RA.host_axis_plan(vertical, bounds, k.shape[1], 4)['staged']
    assert staged(0, 264, 33) == 1 and staged(1, 200, 25) == 1            # ksize 49 on the staged kernels
    assert staged(0, 100, 7) == 0 and staged(1, 100, 7) == 0              # ksize 87 on the general kernel
    assert staged(0, 1030, 515) == 1 and staged(1, 1030, 515) == 1        # several workgroups along the axis
    assert staged(0, 37, 16) == 1 and staged(1, 23, 9) == 1               # each axis alone, on the staged kernels ...
    assert ((100, 3), (7, 3)) in RA.SHAPES and ((3, 100), (3, 7)) in RA.SHAPES       # ... and on the general one


def test_every_pair_through_premultiply_and_unpremultiply():
    """256 x 256 -> 512 x 256 with BOX: each tap is a single weight of 1, so the output is unpremultiply(premultiply(.)) of every
    (colour, alpha) pair, twice over"""
    img = RA.all_pairs()
    try:
        want = RA.pil_resize(img[None], (512, 256), 'box')
        assert want.tobytes() == RA.host_resize(img[None], (512, 256), 'box').tobytes()
    except ImportError:
        want = RA.host_resize(img[None], (512, 256), 'box')
    assert want[0, :, 0::2].tobytes() == RA.np_unpremultiply(RA.np_premultiply(img)).tobytes()
    r = DeviceResize((256, 256), (512, 256), 'box', mode='RGBA')
    _same(r(img), want)
    r.close()
    # the vertical kernel's conversions on the same pairs: 256 x 256 -> 256 x 512
    r = DeviceResize((256, 256), (256, 512), 'box', mode='RGBA')
    _same(r(img), RA.host_resize(img[None], (256, 512), 'box'))
    r.close()


def test_an_equal_size_call_converts_nothing():
    f = RA.load(RA.case_name((12, 10), (12, 10), 'lanczos'))
    src = np.array(f['src'])
    src[0, :, ::2, 3] = 0                                                 # alpha 0 over colours that a premultiply would zero
    assert ((src[..., 3] == 0) & (src[..., :3].max(-1) > 0)).sum() > 50
    r = DeviceResize((12, 10), (12, 10), 'lanczos', max_images=3, mode='RGBA')
    _same(r(src), src)
    r.close()
    _same(reference_resize(src, (12, 10), (12, 10), mode='RGBA'), src)


@pytest.mark.parametrize('src_wh,mid_wh,dst_wh,filt', RA.TWOSTEP)
def test_filter_then_box_is_get_rgb(src_wh, mid_wh, dst_wh, filt):
    f = RA.load(RA.twostep_name(src_wh, mid_wh, dst_wh, filt))
    got = reference_resize(f['src'], mid_wh, dst_wh, first=filt, mode='RGBA')
    assert tuple(got.shape) == (3, dst_wh[1], dst_wh[0], 4)
    _same(got, f['expected'])
    one = RA.load(RA.case_name((65, 47), (32, 23), 'lanczos'))            # each step is no operation at equal size
    _same(reference_resize(one['src'], (32, 23), mode='RGBA'), one['expected'])
    _same(reference_resize(one['src'], (32, 23), (32, 23), mode='RGBA'), one['expected'])


def test_batch_of_three_through_plans_of_two_and_one():
    src_wh, dst_wh = (65, 47), (32, 23)
    f = RA.load(RA.case_name(src_wh, dst_wh, 'lanczos'))
    with_two = DeviceResize(src_wh, dst_wh, 'lanczos', max_images=2, mode='RGBA')
    _same(with_two(f['src']), f['expected'])
    one = DeviceResize(src_wh, dst_wh, 'lanczos', mode='RGBA')            # max_images=1: three launches
    _same(one(f['src']), f['expected'])
    # the C call itself refuses what the plan was not made for, before any launch
    L = _lib.load()
    src, dst = torch.zeros(3 * 47 * 65 * 4 + 16, dtype=torch.uint8, device='cuda'), torch.zeros(3 * 23 * 32 * 4 + 16, dtype=torch.uint8, device='cuda')
    for n in (0, 3, -1):
        assert L.hr_image_resize(with_two._h, C.c_void_p(src.data_ptr()), n, C.c_void_p(dst.data_ptr()), None) == -1
        assert 'n_images' in L.hr_last_error().decode()
    for s_off, d_off in ((1, 0), (0, 2)):                                 # a pixel is one aligned word
        assert L.hr_image_resize(with_two._h, C.c_void_p(src.data_ptr() + s_off), 1, C.c_void_p(dst.data_ptr() + d_off), None) == -1
        assert '4-byte aligned' in L.hr_last_error().decode()
    torch.cuda.synchronize()
    assert int(dst.sum()) == 0
    with pytest.raises(ValueError, match='8-bit RGBA'):
        one(np.zeros((47, 65, 3), np.uint8))
    with pytest.raises(ValueError, match='out must be'):
        one(f['src'], out=torch.empty((3, 23, 32, 3), dtype=torch.uint8, device='cuda'))
    with_two.close()
    one.close()


def test_captured_in_a_graph_and_replayed_on_fresh_inputs():
    src_wh, dst_wh = (37, 29), (16, 11)
    f = RA.load(RA.case_name(src_wh, dst_wh, 'lanczos'))
    r = DeviceResize(src_wh, dst_wh, 'lanczos', max_images=3, mode='RGBA')
    src = torch.zeros((3, 29, 37, 4), dtype=torch.uint8, device='cuda')
    out = torch.zeros((3, 11, 16, 4), dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r(src, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r(src, out=out)                                                   # one hr_image_resize: no copy from the host, no allocation
    first = np.array(f['src'])
    second = np.ascontiguousarray(first[::-1, :, ::-1])
    for images, want in ((first, f['expected']), (second, RA.host_resize(second, dst_wh, 'lanczos'))):
        src.copy_(torch.from_numpy(images))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _same(out, want)
    del graph
    r.close()


@pytest.mark.parametrize('src_wh,dst_wh', [((37, 29), (16, 11)), ((37, 23), (37, 9)), ((37, 23), (16, 23)), ((100, 3), (7, 3)), ((3, 100), (3, 7)),
                                           ((12, 10), (12, 10)), ((257, 9), (256, 9))])
def test_nothing_outside_the_destination_is_written(src_wh, dst_wh):
    f = RA.load(RA.case_name(src_wh, dst_wh, 'lanczos'))
    L = _lib.load()
    n_out = 2 * dst_wh[0] * dst_wh[1] * 4
    plan = C.c_void_p()
    _lib.check(L.hr_resize_plan_create_rgba(src_wh[0], src_wh[1], dst_wh[0], dst_wh[1], 1, 2, C.byref(plan)), 'hr_resize_plan_create_rgba')
    src = torch.from_numpy(np.array(f['src'][:2])).cuda()
    for pad in (64, 4):                                                   # the destination at a 16-byte boundary and 4 bytes past one
        buf = torch.full((pad + n_out + 64,), 0xA5, dtype=torch.uint8, device='cuda')
        _lib.check(L.hr_image_resize(plan, C.c_void_p(src.data_ptr()), 2, C.c_void_p(buf.data_ptr() + pad), data.current_stream(buf.device)),
                   'hr_image_resize')
        got = buf.cpu().numpy()
        assert (got[:pad] == 0xA5).all() and (got[pad + n_out:] == 0xA5).all()
        assert got[pad:pad + n_out].tobytes() == f['expected'][:2].tobytes()
    L.hr_resize_plan_destroy(plan)
