"""`-m gpu`: hr_jpeg_encode / JpegEncoder / save_jpeg against PIL's files (tests/golden/jpeg_encode) and against the host build of the same
header: equality of bytes, no tolerance anywhere.  Nothing here provokes a fault: the refused calls are refused on the host before
anything is launched."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

import encoder_front_common as F
import jpeg_encode_common as E
from hyperreel_amd import jpeg
from hyperreel_amd import lib as _lib

pytestmark = pytest.mark.gpu

_encoders = {}


def _encoder(w, h, c, quality, subsampling, restart_rows):
    key = (w, h, c, quality, subsampling, restart_rows)
    if key not in _encoders:
        _encoders[key] = jpeg.JpegEncoder(w, h, c, quality, subsampling, restart_rows)
    return _encoders[key]


def _device_file(a, opts, extra=64):
    """(the file's bytes, the whole capacity buffer afterwards, the length): the buffer is filled with 0xA5 first"""
    h, w, c = a.shape
    enc = _encoder(w, h, c, opts['quality'], opts['subsampling'], opts['restart_rows'])
    buf = torch.full((enc.bound + extra,), 0xA5, dtype=torch.uint8, device='cuda')
    out, length = enc.encode_device(torch.from_numpy(E.frame_of(a)).cuda(), out=buf)
    torch.cuda.synchronize()
    n = int(length.item())
    assert 0 < n <= enc.bound
    whole = out.cpu().numpy()
    return whole[:n].tobytes(), whole, n


def _groups():
    """the fixtures by archive, so that a failure names its shape"""
    out = {}
    for case in E.golden():
        out.setdefault(case[0].split('_')[0] + '_' + case[0].split('_')[1], []).append(case)
    return out


@pytest.mark.parametrize('shape', sorted(_groups()))
def test_bytes_equal_pil_on_every_fixture(shape):
    """uint8, float32 and RGBA input: 0 bytes differ from PIL's file, the length is exact, nothing is written past it"""
    bad = []
    for name, a, opts, want in _groups()[shape]:
        got, whole, n = _device_file(a, opts)
        if got != want or not (whole[n:] == 0xA5).all():
            bad.append((name, n, len(want)))
    for enc in _encoders.values():
        enc.close()
    _encoders.clear()
    assert not bad, bad[:10]


def test_bytes_equal_host_outside_the_fixtures():
    bad = []
    for name, a, opts in E.live_cases():
        got, whole, n = _device_file(a, opts)
        want = jpeg.encode_host(E.frame_of(a), channels=a.shape[2], **opts)
        if got != want or not (whole[n:] == 0xA5).all():
            bad.append((name, n, len(want)))
    assert not bad, bad[:10]


def test_nan_frame_equals_zeros():
    rng = np.random.default_rng(9)
    x = rng.random((40, 56, 3), dtype=np.float32) * 2 - 0.5
    holes = rng.random(x.shape) < 0.1
    enc = jpeg.JpegEncoder(56, 40, quality=90)
    with_nan = enc.encode(torch.from_numpy(np.where(holes, np.float32(np.nan), x)).cuda())
    with_zero = enc.encode(torch.from_numpy(np.where(holes, np.float32(0), x)).cuda())
    assert with_nan == with_zero == jpeg.encode_host(np.where(holes, np.float32(0), x))
    enc.close()


def test_two_encoders_on_two_streams():
    t = E.tool()
    w, h = 96, 80
    arrays = [t.content('noise', w, h, 3, 1), t.content('ramp', w, h, 3, 2)]
    options = [{'quality': 90, 'subsampling': '4:2:0', 'restart_rows': 0}, {'quality': 50, 'subsampling': '4:4:4', 'restart_rows': 1}]
    expect = [jpeg.encode_host(a, **o) for a, o in zip(arrays, options)]
    frames = [torch.from_numpy(a).cuda() for a in arrays]
    F.two_encoders_on_two_streams([jpeg.JpegEncoder(w, h, 3, **o) for o in options], frames, expect)


def test_graph_capture_replays_over_a_changing_frame():
    """one captured encode_device, three replays with the frame refilled between them: the eager bytes each time"""
    t = E.tool()
    w, h, c = 96, 80, 3
    inputs = [torch.from_numpy(t.as_float(t.content(k, w, h, c, 4), 5)).cuda() for k in ('noise', 'flat', 'binary')]
    F.graph_capture_replays_over_a_changing_frame(jpeg.JpegEncoder(w, h, c, quality=90, subsampling='4:2:0', restart_rows=2), inputs)


def test_device_decoder_reads_the_devices_file_as_pil_does():
    from PIL import Image
    t = E.tool()
    for (w, h), sub, rr in (((65, 33), '4:2:0', 0), ((40, 24), '4:2:2', 1), ((31, 18), '4:4:4', 0)):
        a = t.content('noise', w, h, 3, 6)
        enc = jpeg.JpegEncoder(w, h, 3, quality=90, subsampling=sub, restart_rows=rr)
        data = enc.encode(torch.from_numpy(a).cuda())
        want = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
        dec = jpeg.JpegDecoder(w, h)
        got = dec.decode([data], 'RGB')
        torch.cuda.synchronize()
        assert np.array_equal(got[0].cpu().numpy(), want), (w, h, sub)
        dec.close()
        enc.close()


def test_flat_frame_sliced_frame_grey_map_and_save_jpeg(tmp_path):
    t = E.tool()
    w, h = 61, 47
    a = t.as_float(t.content('ramp', w, h, 3, 8), 8)
    enc = jpeg.JpegEncoder(w, h)
    expect = jpeg.encode_host(a)
    assert enc.encode(torch.from_numpy(a).cuda().reshape(h * w, 3)) == expect
    wide = torch.from_numpy(np.concatenate([a, np.full((h, w, 1), 0.25, np.float32)], -1)).cuda()
    assert not wide[..., :3].is_contiguous() and enc.encode(wide[..., :3]) == expect
    grey = t.content('noise', w, h, 1, 9)[..., 0]
    path = str(tmp_path / 'map.jpg')
    n = jpeg.save_jpeg(path, torch.from_numpy(grey).cuda(), quality=75)
    data = open(path, 'rb').read()
    assert n == len(data) and data == jpeg.encode_host(grey, quality=75, subsampling='4:4:4')
    F.front_end_refusals(enc)
    enc.close()


def test_refusals_leave_the_output_untouched():
    L = _lib.load()
    w, h, c, q, sub, rr = 16, 9, 3, 90, 2, 0
    cap = jpeg.bound(w, h, c, sub, rr)
    n = C.c_int64(-7)
    assert L.hr_jpeg_bound(w, h, c, sub, rr, C.byref(n)) == 0 and n.value == cap == jpeg.host_lib().hr_jpeg_host_bound(w, h, c, sub, rr)
    for bad in ((0, h, c, q, sub, rr), (w, 0, c, q, sub, rr), (65536, h, c, q, sub, rr), (w, 65536, c, q, sub, rr), (w, h, 2, q, sub, rr),
                (w, h, 0, q, sub, rr), (w, h, 5, q, sub, rr), (w, h, c, 0, sub, rr), (w, h, c, 101, sub, rr), (w, h, c, q, 3, rr), (w, h, c, q, -1, rr),
                (w, h, 1, q, 2, rr), (w, h, 1, q, 1, rr), (w, h, c, q, sub, -1), (65535, h, c, q, 0, 8)):
        handle = C.c_void_p()
        assert L.hr_jpeg_encoder_create(*bad, C.byref(handle)) == _lib.HR_E_INVALID and not handle.value, bad
        assert L.hr_last_error()
        if bad[3] == q:
            assert L.hr_jpeg_bound(bad[0], bad[1], bad[2], bad[4], bad[5], C.byref(n)) == _lib.HR_E_INVALID, bad
    assert L.hr_jpeg_bound(w, h, c, sub, rr, None) == _lib.HR_E_INVALID
    assert L.hr_jpeg_encoder_create(w, h, c, q, sub, rr, None) == _lib.HR_E_INVALID
    handle = C.c_void_p()
    assert L.hr_jpeg_encoder_create(w, h, c, q, sub, rr, C.byref(handle)) == 0
    px = torch.zeros((h, w, c), dtype=torch.uint8, device='cuda')
    out = torch.full((cap,), 0xA5, dtype=torch.uint8, device='cuda')
    length = torch.full((1,), -3, dtype=torch.int64, device='cuda')
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p, o, ln = C.c_void_p(px.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(length.data_ptr())
    refused = [(None, p, 0, o, cap, ln), (handle, None, 0, o, cap, ln), (handle, p, 0, None, cap, ln), (handle, p, 0, o, cap, None), (handle, p, 2, o, cap, ln),
               (handle, p, -1, o, cap, ln), (handle, p, 0, o, cap - 1, ln), (handle, p, 0, o, 0, ln)]
    for args in refused:
        assert L.hr_jpeg_encode(*args, s) == _lib.HR_E_INVALID, args
        assert L.hr_last_error()
    torch.cuda.synchronize()
    assert (out == 0xA5).all() and int(length.item()) == -3
    assert L.hr_jpeg_encode(handle, p, 0, o, cap, ln, s) == 0
    torch.cuda.synchronize()
    assert out[:int(length.item())].cpu().numpy().tobytes() == jpeg.encode_host(np.zeros((h, w, c), np.uint8))
    L.hr_jpeg_encoder_destroy(handle)
