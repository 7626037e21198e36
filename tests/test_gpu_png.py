"""`-m gpu`: hr_png_encode / PngEncoder / save_png against the host build of the same header (tests/png_common.py): equality of bytes, no
tolerance anywhere.  Shapes: the small ones, every strip edge from hr_png_plan for each channel count, and a row wider than the strip
budget.  Nothing here provokes a fault: the refused calls are refused on the host before anything is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import encoder_front_common as F
import png_common as P
from hyperreel_amd import lib as _lib
from hyperreel_amd import png

pytestmark = pytest.mark.gpu

# channels x shapes x contents = 150 cases; the pixel type and the filter mode rotate through the product, so that every (type, mode)
# pair meets every channel count, several contents and several shapes
CASES = []
for c in P.CHANNELS:
    for si, (w, h) in enumerate(P.shapes(c)):
        for ci, content in enumerate(P.CONTENTS):
            CASES.append((c, w, h, content, (si + ci) % 2, P.FILTER_MODES[(si + 2 * ci + c) % 6]))
assert {(t, m) for _, _, _, _, t, m in CASES} == {(t, m) for t in (0, 1) for m in P.FILTER_MODES}

_encoders = {}


def _encoder(w, h, c):
    if (w, h, c) not in _encoders:
        _encoders[(w, h, c)] = png.PngEncoder(w, h, c)
    return _encoders[(w, h, c)]


def _frame(content, w, h, c, pixel_type):
    im = P.image(content, w, h, c)
    return P.as_float(im) if pixel_type == P.F32 else np.array(im)


def _device_file(enc, frame, mode, extra=64):
    """(bytes of the file, the whole capacity buffer afterwards): the buffer is filled with 0xA5 first"""
    buf = torch.full((enc.bound + extra,), 0xA5, dtype=torch.uint8, device='cuda')
    out, length = enc.encode_device(torch.from_numpy(frame).cuda(), out=buf, filter=mode)
    torch.cuda.synchronize()
    n = int(length.item())
    assert 0 < n <= enc.bound
    whole = out.cpu().numpy()
    return whole[:n].tobytes(), whole, n


@pytest.mark.parametrize('c,w,h,content,pixel_type,mode', CASES, ids=[f'c{c}_w{w}h{h}_{k}_t{t}_f{m}' for c, w, h, k, t, m in CASES])
def test_bytes_equal_host(c, w, h, content, pixel_type, mode):
    frame = _frame(content, w, h, c, pixel_type)
    expect = P.encode_host(frame, c, mode)
    got, whole, n = _device_file(_encoder(w, h, c), frame, mode)
    assert n == len(expect)
    assert got == expect
    assert (whole[n:] == 0xA5).all(), 'bytes beyond the reported length were written'
    assert np.array_equal(P.decode(got)[0], P.image(content, w, h, c))


def test_same_frame_twice_and_two_encoders_on_two_streams():
    c, (w, h) = 3, P.shapes(3)[8]
    frames = [torch.from_numpy(P.as_float(P.image(k, w, h, c))).cuda() for k in ('disc', 'ramp')]
    expect = [P.encode_host(P.as_float(P.image(k, w, h, c)), c) for k in ('disc', 'ramp')]
    F.two_encoders_on_two_streams([png.PngEncoder(w, h, c), png.PngEncoder(w, h, c)], frames, expect)


def test_graph_capture_replays_over_a_changing_frame():
    c, (w, h) = 3, P.shapes(3)[7]
    inputs = [torch.from_numpy(P.as_float(P.image(k, w, h, c))).cuda() for k in ('disc', 'white', 'noise')]
    F.graph_capture_replays_over_a_changing_frame(png.PngEncoder(w, h, c), inputs)


def test_sliced_float_frame():
    w, h = 61, 47
    wide = torch.from_numpy(np.concatenate([P.as_float(P.image('disc', w, h, 3)), np.full((h, w, 1), 0.25, np.float32)], -1)).cuda()
    view = wide[..., :3]
    assert not view.is_contiguous()
    assert _encoder(w, h, 3).encode(view) == P.encode_host(P.as_float(P.image('disc', w, h, 3)), 3)


def test_flat_frame_grey_map_and_save_png(tmp_path):
    w, h = 61, 47
    rgb = torch.from_numpy(P.as_float(P.image('disc', w, h, 3))).cuda()
    assert _encoder(w, h, 3).encode(rgb.reshape(h * w, 3)) == P.encode_host(P.as_float(P.image('disc', w, h, 3)), 3)
    grey = torch.from_numpy(np.array(P.image('ramp', w, h, 1))[..., 0]).cuda()
    path = str(tmp_path / 'map.png')
    n = png.save_png(path, grey)
    data = open(path, 'rb').read()
    assert n == len(data) and data == P.encode_host(P.image('ramp', w, h, 1), 1)
    px, mode = P.decode(data)
    assert mode == 'L' and np.array_equal(px, P.image('ramp', w, h, 1))


def test_refusals_leave_the_output_untouched():
    L = _lib.load()
    w, h, c = 16, 9, 3
    cap = P.bound(w, h, c)
    n = C.c_int64(-7)
    assert L.hr_png_bound(w, h, c, C.byref(n)) == 0 and n.value == cap
    for bad in ((0, h, c), (w, 0, c), (-1, h, c), (w, h, 2), (w, h, 0), (w, h, 5), (1 << 27, 1, 1), (1 << 25, 1, 4), (1 << 20, 1 << 10, 3)):
        assert L.hr_png_bound(*bad, C.byref(n)) == _lib.HR_E_INVALID
        handle = C.c_void_p()
        assert L.hr_png_encoder_create(*bad, C.byref(handle)) == _lib.HR_E_INVALID and not handle.value
    assert L.hr_png_bound(w, h, c, None) == _lib.HR_E_INVALID
    assert L.hr_png_encoder_create(w, h, c, None) == _lib.HR_E_INVALID
    handle = C.c_void_p()
    assert L.hr_png_encoder_create(w, h, c, C.byref(handle)) == 0
    px = torch.zeros((h, w, c), dtype=torch.uint8, device='cuda')
    out = torch.full((cap,), 0xA5, dtype=torch.uint8, device='cuda')
    length = torch.full((1,), -3, dtype=torch.int64, device='cuda')
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p, o, ln = C.c_void_p(px.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(length.data_ptr())
    A = _lib.HR_PNG_FILTER_ADAPTIVE
    refused = [
        (None, p, 0, A, o, cap, ln), (handle, None, 0, A, o, cap, ln), (handle, p, 0, A, None, cap, ln), (handle, p, 0, A, o, cap, None),
        (handle, p, 2, A, o, cap, ln), (handle, p, -1, A, o, cap, ln), (handle, p, 0, 6, o, cap, ln), (handle, p, 0, -1, o, cap, ln),
        (handle, p, 0, A, o, cap - 1, ln), (handle, p, 0, A, o, 0, ln),
    ]
    for args in refused:
        assert L.hr_png_encode(*args, s) == _lib.HR_E_INVALID, args
        assert L.hr_last_error()
    torch.cuda.synchronize()
    assert (out == 0xA5).all() and int(length.item()) == -3
    assert L.hr_png_encode(handle, p, 0, A, o, cap, ln, s) == 0
    torch.cuda.synchronize()
    assert out[:int(length.item())].cpu().numpy().tobytes() == P.encode_host(np.zeros((h, w, c), np.uint8), c)
    L.hr_png_encoder_destroy(handle)
    F.front_end_refusals(_encoder(61, 47, 3))


def test_render_then_save_png(tmp_path):
    """the smallest fixture model, a 64 x 48 view, save_png: PIL reads back to8b of the rendered tensor"""
    from gpu_common import make_render_fn
    from helpers import Golden
    from hyperreel_amd import scenes
    g = Golden('donerf_sphere_small')
    fn = make_render_fn(g.cfg, g.dataset, g.state_dict)
    w, h = 64, 48
    rays = torch.from_numpy(scenes.benchmark_rays(g.recipe['model'], h, w, frame=7)).cuda()
    rgb = fn.model.render(rays)['rgb']
    assert rgb.shape == (h * w, 3)
    path = str(tmp_path / 'frame.png')
    png.save_png(path, rgb, width=w, height=h)
    from PIL import Image
    im = Image.open(path)
    assert im.mode == 'RGB' and im.size == (w, h)
    expect = P.to8b_reference(rgb.cpu().numpy()).reshape(h, w, 3)
    assert np.isfinite(rgb.cpu().numpy()).all()
    assert np.array_equal(np.asarray(im), expect)
    assert len(set(expect.reshape(-1).tolist())) > 8, 'the view shows nothing'
