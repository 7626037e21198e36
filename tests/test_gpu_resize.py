"""`-m gpu`: hr_image_resize / DeviceResize / reference_resize against the bytes PIL wrote (tests/golden/resize,
tools/make_resize_golden.py).  Equality of bytes, no tolerance anywhere.  The shapes are the smallest at which a kernel can still go
wrong (tests/resize_common.py SHAPES says what each is for); every one runs under all four filters on random bytes, random 0 / 255 and a
checkerboard, as one batch of three images, from a source at a 16-byte boundary and from one that starts an odd number of bytes past
it (rows of 3-byte pixels are staged through aligned 16-byte loads).  Nothing here provokes a fault: the refused calls are refused on
the host before anything is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import resize_common as RC
from hyperreel_amd import data
from hyperreel_amd import lib as _lib
from hyperreel_amd.data import DeviceRaySet, DeviceResize, reference_resize

pytestmark = pytest.mark.gpu

CASES = [(s, d, f) for s, d in RC.SHAPES for f in RC.FILTERS]


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


@pytest.mark.parametrize('src_wh,dst_wh,filt', CASES, ids=[RC.case_name(*c) for c in CASES])
def test_bytes_equal_pil(src_wh, dst_wh, filt):
    f = RC.load(RC.case_name(src_wh, dst_wh, filt))
    r = DeviceResize(src_wh, dst_wh, filt, max_images=3)
    try:
        got = r(f['src'])                                             # numpy on the host: a fresh, aligned device copy
        assert got.is_cuda and tuple(got.shape) == (3, dst_wh[1], dst_wh[0], 3)
        _same(got, f['expected'])
        for shift in (1, 7):
            src = _shifted(f['src'], shift)
            assert src.data_ptr() % 16 == shift
            _same(r(src), f['expected'])
    finally:
        r.close()


def test_the_named_cases_take_the_kernel_they_are_for():
    """which kernel a fixture's axis runs on is hr_resize.h's decision: the host build answers for the table above"""
    def staged(vertical, n_in, n_out):
        bounds, k = RC.host_coeffs(n_in, n_out, 'lanczos')
        return RC.host_axis_plan(vertical, bounds, k.shape[1])['staged']
    assert staged(0, 264, 33) == 1 and staged(1, 200, 25) == 1            # ksize 49 on the staged kernels
    assert staged(0, 100, 7) == 0 and staged(1, 100, 7) == 0              # ksize 87 on the general kernel
    assert staged(0, 1030, 515) == 1 and staged(1, 1030, 515) == 1        # several workgroups along the axis


def test_batch_of_three_through_a_plan_of_two():
    src_wh, dst_wh = (65, 47), (32, 23)
    f = RC.load(RC.case_name(src_wh, dst_wh, 'lanczos'))
    with_two = DeviceResize(src_wh, dst_wh, 'lanczos', max_images=2)
    _same(with_two(f['src']), f['expected'])
    one = DeviceResize(src_wh, dst_wh, 'lanczos')                         # max_images=1: three launches
    _same(one(f['src']), f['expected'])
    # the C call itself refuses what the plan was not made for, before any launch
    L = _lib.load()
    src, dst = torch.zeros(3 * 47 * 65 * 3, dtype=torch.uint8, device='cuda'), torch.zeros(3 * 23 * 32 * 3, dtype=torch.uint8, device='cuda')
    for n in (0, 3, -1):
        assert L.hr_image_resize(with_two._h, C.c_void_p(src.data_ptr()), n, C.c_void_p(dst.data_ptr()), None) == -1
        assert 'n_images' in L.hr_last_error().decode()
    assert L.hr_image_resize(with_two._h, None, 1, C.c_void_p(dst.data_ptr()), None) == -1 and 'src_dev' in L.hr_last_error().decode()
    assert L.hr_image_resize(with_two._h, C.c_void_p(src.data_ptr()), 1, None, None) == -1 and 'dst_dev' in L.hr_last_error().decode()
    torch.cuda.synchronize()
    assert int(dst.sum()) == 0
    with_two.close()
    one.close()
    with pytest.raises(RuntimeError, match='closed'):
        one(f['src'])


def test_inputs_from_the_host_and_the_device_one_plan_two_inputs():
    src_wh, dst_wh = (37, 29), (16, 11)
    f = RC.load(RC.case_name(src_wh, dst_wh, 'bicubic'))
    r = DeviceResize(src_wh, dst_wh, 'bicubic', max_images=3)
    host = torch.from_numpy(np.array(f['src']))
    for images in (f['src'], host, host.cuda()):
        _same(r(images), f['expected'])
    single = r(f['src'][1])                                               # (H, W, 3)
    assert tuple(single.shape) == (1, 11, 16, 3)
    _same(single, f['expected'][1:2])
    # the same plan on other pixels: nothing of the first call lingers
    other = np.ascontiguousarray(f['src'][::-1, ::-1])
    _same(r(other), RC.host_resize(other, dst_wh, 'bicubic'))
    _same(r(f['src']), f['expected'])
    with pytest.raises(ValueError, match='made for 37 x 29'):
        r(np.zeros((29, 38, 3), np.uint8))
    with pytest.raises(ValueError, match='out must be'):
        r(f['src'], out=torch.empty((3, 11, 16, 3), dtype=torch.uint8))
    r.close()


def test_on_a_stream_of_its_own():
    src_wh, dst_wh = (264, 200), (33, 25)
    f = RC.load(RC.case_name(src_wh, dst_wh, 'lanczos'))
    r = DeviceResize(src_wh, dst_wh, 'lanczos', max_images=3)
    src = torch.from_numpy(np.array(f['src'])).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = r(src)
    stream.synchronize()
    _same(got, f['expected'])
    r.close()


@pytest.mark.parametrize('src_wh,mid_wh,dst_wh,filt', RC.TWOSTEP)
def test_lanczos_then_box_is_get_rgb(src_wh, mid_wh, dst_wh, filt):
    f = RC.load(RC.twostep_name(src_wh, mid_wh, dst_wh, filt))
    _same(reference_resize(f['src'], mid_wh, dst_wh, first=filt), f['expected'])
    # each step is no operation at equal size
    one = RC.load(RC.case_name(src_wh, dst_wh, 'lanczos'))
    _same(reference_resize(one['src'], dst_wh), one['expected'])
    _same(reference_resize(one['src'], dst_wh, dst_wh), one['expected'])
    _same(reference_resize(one['src'], src_wh, src_wh), one['src'])
    box = RC.load(RC.case_name(src_wh, dst_wh, 'box'))
    _same(reference_resize(box['src'], src_wh, dst_wh), box['expected'])


def test_a_ray_set_built_from_the_resized_images():
    src_wh, dst_wh = (65, 47), (32, 23)
    f = RC.load(RC.case_name(src_wh, dst_wh, 'lanczos'))
    images = reference_resize(f['src'], dst_wh)
    W, H = dst_wh
    poses = np.tile(np.eye(4, dtype=np.float32)[:3], (3, 1, 1))
    K = np.array([[30, 0, W / 2], [0, 30, H / 2], [0, 0, 1]], np.float32)
    s = DeviceRaySet(images, poses, K, None, None, dst_wh)
    assert len(s) == 3 * W * H
    elements = torch.tensor([0, 1, W * H - 1, W * H, 2 * W * H + 17, 3 * W * H - 1] + list(range(5, 3 * W * H, 97)), dtype=torch.int64, device='cuda')
    rgb = s.batch(0, 0, indices=elements)['rgb'].cpu().numpy()
    want = f['expected'].reshape(-1, 3)[elements.cpu().numpy()].astype(np.float32) / np.float32(255)
    assert rgb.dtype == np.float32 and np.array_equal(rgb.view(np.uint32), want.view(np.uint32))
    gt = data.as_float(images)                                            # model.evaluate's ground truth: a torch op, by definition x.float().div(255)
    assert tuple(gt.shape) == (3 * W * H, 3) and gt.dtype == torch.float32 and torch.equal(gt, images.reshape(-1, 3).float().div(255))
    assert np.abs(gt.cpu().numpy() - f['expected'].reshape(-1, 3) / 255.0).max() < 1e-7
    s.close()


def test_captured_in_a_graph_and_replayed_on_fresh_inputs():
    src_wh, dst_wh = (37, 29), (16, 11)
    f = RC.load(RC.case_name(src_wh, dst_wh, 'lanczos'))
    r = DeviceResize(src_wh, dst_wh, 'lanczos', max_images=3)
    src = torch.zeros((3, 29, 37, 3), dtype=torch.uint8, device='cuda')
    out = torch.zeros((3, 11, 16, 3), dtype=torch.uint8, device='cuda')
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
    for images, want in ((first, f['expected']), (second, RC.host_resize(second, dst_wh, 'lanczos'))):
        src.copy_(torch.from_numpy(images))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _same(out, want)
    del graph
    r.close()


@pytest.mark.parametrize('src_wh,dst_wh', [((37, 29), (16, 11)), ((40, 30), (40, 13)), ((40, 30), (17, 30)), ((100, 3), (7, 3)), ((3, 100), (3, 7)),
                                           ((12, 10), (12, 10)), ((257, 9), (256, 9))])
def test_nothing_outside_the_destination_is_written(src_wh, dst_wh):
    f = RC.load(RC.case_name(src_wh, dst_wh, 'lanczos'))
    L = _lib.load()
    n_out = 2 * dst_wh[0] * dst_wh[1] * 3
    plan = C.c_void_p()
    _lib.check(L.hr_resize_plan_create(src_wh[0], src_wh[1], dst_wh[0], dst_wh[1], 1, 2, C.byref(plan)), 'hr_resize_plan_create')
    src = torch.from_numpy(np.array(f['src'][:2])).cuda()
    for pad in (64, 3):                                                   # the destination at an aligned and at an odd address
        buf = torch.full((pad + n_out + 64,), 0xA5, dtype=torch.uint8, device='cuda')
        _lib.check(L.hr_image_resize(plan, C.c_void_p(src.data_ptr()), 2, C.c_void_p(buf.data_ptr() + pad), data.current_stream(buf.device)),
                   'hr_image_resize')
        got = buf.cpu().numpy()
        assert (got[:pad] == 0xA5).all() and (got[pad + n_out:] == 0xA5).all()
        assert got[pad:pad + n_out].tobytes() == f['expected'][:2].tobytes()
    L.hr_resize_plan_destroy(plan)
