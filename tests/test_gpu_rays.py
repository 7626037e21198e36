"""`-m gpu`: camera rays, plain and with NDC (hr_generate_rays, hr_generate_rays_ndc, generate_rays / render_camera with ndc=) and the device-resident training
feed (hr_rayset_*, hyperreel_amd.data.DeviceRaySet) against the reference's own rays and all_inputs (tests/golden/camera, written
by tools/make_camera_golden.py) and against hyperreel_amd/csrc/hr_camera.h compiled for the host.

The bar for ray coordinates is camera_common.bars(): 4 x the reference's own float32-to-float64 distance per column group, capped
at 1e-5 (1.7e-6 origins / 1.5e-6 directions on the committed fixtures).  Colours and weights are exact.  Nothing here provokes a
fault: the refused calls are refused on the host before anything is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import camera_common as CC
from helpers import Golden
from hyperreel_amd import lib as _lib
from hyperreel_amd.data import DeviceRaySet, make_camera, make_ndc

pytestmark = pytest.mark.gpu

_fns = {}


def _fn(case):
    if case not in _fns:
        from gpu_common import make_render_fn
        g = Golden(case)
        _fns[case] = (g, make_render_fn(g.cfg, g.dataset, g.state_dict, iteration=g.iteration))
    return _fns[case]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _abi_rays(cam, nd, ray_dim, lo, n, ndc_call=True, base=None):
    L = _lib.load()
    out = torch.full((n, ray_dim), float('nan'), device='cuda') if base is None else base
    if ndc_call:
        rc = L.hr_generate_rays_ndc(C.byref(cam), C.byref(nd) if nd is not None else None, ray_dim, lo, n, C.c_void_p(out.data_ptr()), _stream())
    else:
        rc = L.hr_generate_rays(C.byref(cam), ray_dim, lo, n, C.c_void_p(out.data_ptr()), _stream())
    assert rc == 0, L.hr_last_error()
    torch.cuda.synchronize()
    return out


def _set_of(f, device=None):
    rules = [(int(e), int(o)) for e, o in f['rules']]
    video = bool(f['video'])
    return DeviceRaySet(f['images'], f['poses'], f['intrinsics'], f['times'] if video else None, f['cam_ids'] if video else None,
                        (int(f['img_wh'][0]), int(f['img_wh'][1])), ndc=CC.ndc_of(f), subsample=rules)


def _check_coords(got, ref, bars, what):
    d_o, d_d = float(np.abs(got[:, :3] - ref[:, :3]).max()), float(np.abs(got[:, 3:6] - ref[:, 3:6]).max())
    print(f'{what}: origins {d_o:.3e} (bar {bars["origins"]:.3e}) directions {d_d:.3e} (bar {bars["directions"]:.3e})', flush=True)
    assert d_o <= bars['origins'] and d_d <= bars['directions'], what
    if got.shape[1] == 8:
        assert np.array_equal(got[:, 6:], ref[:, 6:]), what


def test_null_ndc_is_generate_rays():
    f = CC.load('static_pinhole')
    W, H = int(f['img_wh'][0]), int(f['img_wh'][1])
    cam = make_camera(f['poses'][0], f['intrinsics'][0], W, H, 2.0, 0.375)
    for rd in (6, 8):
        for lo, n in ((0, W * H), (500, 1500), (W * H - 7, 7), (3, 0)):
            a = _abi_rays(cam, None, rd, lo, n, ndc_call=True)
            b = _abi_rays(cam, None, rd, lo, n, ndc_call=False)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (rd, lo, n)
            assert n == 0 or not torch.isnan(a).any()


@pytest.mark.parametrize('name', ['centred', 'short_focal'])
def test_the_plain_entry_against_the_host_header(name):
    """hr_generate_rays itself (test_null_ndc_is_generate_rays compares two entries of one kernel) on fisheye_common's 24 x 14 cameras --
    336 pixels: two workgroups, the second partly empty -- bit for bit the host-compiled hr_pixel_ray, into rows on 16- / 8-byte
    boundaries and into rows one float off them (the kernel's 16- and 8-byte stores take either), whole image and sub-ranges, the empty
    ones too: every element of the range written, the 64 guard floats on either side untouched."""
    import fisheye_common as FC
    from test_gpu_fisheye import GUARD, _ranges
    L, hf = _lib.load(), FC.host_lib()
    W, H = FC.CASES[name][:2]
    size = W * H
    assert (W, H) == (24, 14) and 256 < size < 512
    cam = FC.camera_of(name, 3.0, 0.25)
    host = np.full((size, 6), np.nan, np.float32)
    hf.hf_pinhole_rays(C.byref(cam), None, 0, size, host.ctypes.data_as(C.c_void_p))
    assert not np.isnan(host).any()
    for rd in (6, 8):
        for misalign in (0, 1):
            for first, n in [(0, size)] + _ranges(size):
                flat = torch.full((GUARD + misalign + n * rd + GUARD,), float('nan'), device='cuda')
                out = flat[GUARD + misalign:GUARD + misalign + n * rd].view(n, rd)
                assert n == 0 or out.data_ptr() % 16 == 4 * misalign
                rc = L.hr_generate_rays(C.byref(cam), rd, first, n, C.c_void_p(out.data_ptr()), _stream())
                assert rc == 0, L.hr_last_error()
                torch.cuda.synchronize()
                what = (name, rd, misalign, first, n)
                assert torch.isnan(flat[:GUARD + misalign]).all() and torch.isnan(flat[GUARD + misalign + n * rd:]).all(), what
                got = out.cpu().numpy()
                assert not np.isnan(got).any(), what
                assert np.array_equal(got[:, :6].view(np.uint32), host[first:first + n].view(np.uint32)), what
                if rd == 8:
                    assert np.array_equal(got[:, 6:], np.broadcast_to(np.float32([3.0, 0.25]), (n, 2))), what


@pytest.mark.parametrize('name', CC.CASES)
def test_generate_rays_against_the_reference_and_the_host_header(name):
    """Whole frames of every full-resolution image of the fixture: within the bar of the reference's rays, and bit for bit what
    hr_camera.h gives when the host compiler builds it (the same source, IEEE operations, no contraction on either side)."""
    hc = CC.host_lib()
    f = CC.load(name)
    bars = CC.bars()
    nd = CC.ndc_struct(f)
    W, H = int(f['img_wh'][0]), int(f['img_wh'][1])
    rd = CC.ray_dim(f)
    rows = CC.image_rows(f)
    seen = 0
    for i, (e, o) in enumerate(f['rules']):
        if int(e) != 1:
            continue
        cam = CC.camera_of(f, i)
        got = _abi_rays(cam, nd, rd, 0, W * H).cpu().numpy()
        _check_coords(got, f['all_inputs'][rows[i][0]:rows[i][1], :rd], bars, f'{name} image {i}')
        host = np.empty((W * H, 6), np.float32)
        hc.hc_pixel_rays(C.byref(cam), C.byref(nd) if nd is not None else None, 0, W * H, host.ctypes.data_as(C.c_void_p))
        assert np.array_equal(got[:, :6].view(np.uint32), host.view(np.uint32)), (name, i)
        # a pixel sub-range into a buffer that starts off a 16-byte boundary (the same stores take it)
        lo, n = W + 3, 2 * W + 5
        flat = torch.full((n * rd + 1,), float('nan'), device='cuda')
        part = _abi_rays(cam, nd, rd, lo, n, base=flat[1:].view(n, rd)).cpu().numpy()
        assert np.array_equal(part.view(np.uint32), got[lo:lo + n].view(np.uint32))
        seen += 1
    assert seen >= 1


@pytest.mark.parametrize('case,fixture,image', [('technicolor_z_plane_small', 'video_ndc', 0), ('technicolor_z_plane_small', 'video_ndc', 24),
                                                ('neural_3d_z_plane_small', 'ndc_other_size', 0)])
def test_render_camera_with_ndc(case, fixture, image):
    from hyperreel_oracle import HyperReelOracle
    g, fn = _fn(case)
    m = fn.model
    f = CC.load(fixture)
    assert int(f['rules'][image][0]) == 1
    W, H = int(f['img_wh'][0]), int(f['img_wh'][1])
    t, cam_id = float(f['times'][image]), float(f['cam_ids'][image])
    nd = CC.ndc_of(f)
    rays = m.generate_rays(f['poses'][image], f['intrinsics'][image], W, H, time=t, cam_id=cam_id, ndc=nd)
    again = m.generate_rays(f['poses'][image], f['intrinsics'][image], W, H, time=t, cam_id=cam_id, ndc=make_ndc(nd))
    assert torch.equal(rays.view(torch.int32), again.view(torch.int32))
    lo, hi = CC.image_rows(f)[image]
    ref_rays = np.ascontiguousarray(f['all_inputs'][lo:hi, :8])
    _check_coords(rays.cpu().numpy(), ref_rays, CC.bars(), f'{fixture} image {image}')
    want = m.render(rays, frame_time=t)['rgb'].clone()
    got = m.render_camera(f['poses'][image], f['intrinsics'][image], W, H, time=t, cam_id=cam_id, ndc=nd)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    part = m.render_camera(f['poses'][image], f['intrinsics'][image], W, H, time=t, cam_id=cam_id, pixel_range=(W, 3 * W), ndc=nd)
    assert part.shape == (2 * W, 3)
    # without ndc the keyword changes nothing: today's call, today's bits
    plain = m.generate_rays(f['poses'][image], f['intrinsics'][image], W, H, time=t, cam_id=cam_id)
    plain_kw = m.generate_rays(f['poses'][image], f['intrinsics'][image], W, H, time=t, cam_id=cam_id, ndc=None)
    assert torch.equal(plain.view(torch.int32), plain_kw.view(torch.int32)) and not torch.equal(plain, rays)
    # the oracle's render of the REFERENCE's NDC rays
    ref = HyperReelOracle(g.cfg, g.dataset, g.state_dict, iteration=g.iteration).render(ref_rays)['rgb']
    err = float(np.abs(got.cpu().numpy() - ref).max())
    print(f'{case} / {fixture} image {image}: L-inf RGB vs the oracle on the reference\'s rays {err:.3e}; mean rgb {float(ref.mean()):.3f}', flush=True)
    assert err <= 1e-4


@pytest.mark.parametrize('name', CC.CASES)
def test_batch_in_set_order_is_all_inputs(name):
    f = CC.load(name)
    s = _set_of(f)
    ref = f['all_inputs']
    rd = CC.ray_dim(f)
    assert len(s) == ref.shape[0] and s.ray_dim == rd
    idx = torch.arange(len(s), dtype=torch.int64, device='cuda')
    b = s.batch(0, 0, indices=idx)
    torch.cuda.synchronize()
    assert b['coords'].shape == (len(s), rd) and b['rgb'].shape == (len(s), 3) and b['weight'].shape == (len(s), 1)
    assert np.array_equal(b['rgb'].cpu().numpy(), ref[:, rd:rd + 3])
    assert np.array_equal(b['weight'].cpu().numpy(), ref[:, -1:])
    _check_coords(b['coords'].cpu().numpy(), ref[:, :rd], CC.bars(), name)
    # bit for bit the host-compiled header
    host = CC.host_rays(CC.host_lib(), f)
    assert np.array_equal(b['coords'][:, :6].cpu().numpy().view(np.uint32), host.view(np.uint32))
    # a caller's index outside the set: a NaN row of weight 0, nothing read
    odd = torch.tensor([0, -1, len(s), len(s) - 1], dtype=torch.int64, device='cuda')
    o = s.batch(0, 0, indices=odd)
    assert torch.isnan(o['coords'][1:3]).all() and torch.isnan(o['rgb'][1:3]).all() and o['weight'].flatten().tolist() == [1.0, 0.0, 0.0, 1.0]
    assert torch.equal(o['coords'][0], b['coords'][0]) and torch.equal(o['coords'][3], b['coords'][-1])
    s.close()


def _rows(b):
    return torch.cat([b['coords'], b['rgb'], b['weight']], 1)


def _sorted_rows(x):
    x = x.cpu().numpy()
    return x[np.lexsort(x.T[::-1])]


def test_an_epoch_draws_every_ray_once():
    f = CC.load('ndc_other_size')
    s = _set_of(f)
    n, bs = len(s), 1024                          # the small set in several batches, the last one short
    assert n % bs != 0
    full = _rows(s.batch(0, 0, indices=torch.arange(n, dtype=torch.int64, device='cuda')))

    def epoch(e, seed=0, batch=bs):
        parts = [_rows(s.batch(i, batch, epoch=e, seed=seed)) for i in range((n + batch - 1) // batch)]
        assert parts[-1].shape[0] == n - (len(parts) - 1) * batch
        return torch.cat(parts, 0)

    e0 = epoch(0)
    order = s.order(0, n, epoch=0)
    assert torch.equal(torch.sort(order).values, torch.arange(n, dtype=torch.int64, device='cuda'))      # each element exactly once
    assert torch.equal(e0.view(torch.int32), full[order].view(torch.int32))                                # and the rows are those elements
    assert np.array_equal(_sorted_rows(e0).view(np.uint32), _sorted_rows(full).view(np.uint32))
    assert torch.equal(epoch(0, batch=16384).view(torch.int32), e0.view(torch.int32))                     # one batch of 16 384 > the set: short
    e1, s1 = epoch(1), epoch(0, seed=1)
    assert not torch.equal(e1, e0) and not torch.equal(s1, e0) and not torch.equal(s1, e1)
    assert float((s.order(0, n, epoch=1) == order).float().mean()) < 0.01
    assert torch.equal(epoch(0).view(torch.int32), e0.view(torch.int32))                                  # the same (seed, epoch) twice
    with pytest.raises(IndexError):
        s.batch((n + bs - 1) // bs, bs)
    # another stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = epoch(0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(other.view(torch.int32), e0.view(torch.int32))
    # replayed from a captured graph into NaN-poisoned outputs: every output element is written
    out = {'coords': torch.empty((bs, s.ray_dim), device='cuda'), 'rgb': torch.empty((bs, 3), device='cuda'), 'weight': torch.empty((bs, 1), device='cuda')}
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.batch(2, bs, epoch=0, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.batch(2, bs, epoch=0, out=out)
    for _ in range(3):
        for t in out.values():
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_rows(out).view(torch.int32), e0[2 * bs:3 * bs].view(torch.int32))
    s.close()


def test_an_epoch_in_batches_of_16384():
    """The reference's batch size on a set larger than one batch: 12 copies of the video fixture's images."""
    f = CC.load('video_ndc')
    reps = 12
    rules = [(int(e), int(o)) for e, o in f['rules']] * reps
    tile = lambda a: np.concatenate([a] * reps, 0)
    s = DeviceRaySet(tile(f['images']), tile(f['poses']), tile(f['intrinsics']), tile(f['times']), tile(f['cam_ids']),
                     (int(f['img_wh'][0]), int(f['img_wh'][1])), ndc=CC.ndc_of(f), subsample=rules)
    n, bs = len(s), 16384
    assert n == reps * f['all_inputs'].shape[0] and n > 2 * bs and n % bs != 0
    full = _rows(s.batch(0, 0, indices=torch.arange(n, dtype=torch.int64, device='cuda')))
    assert np.array_equal(full[:, 8:].cpu().numpy(), tile(f['all_inputs'])[:, 8:])
    parts = [_rows(s.batch(i, bs, epoch=3, seed=5)) for i in range((n + bs - 1) // bs)]
    assert [p.shape[0] for p in parts] == [bs] * (n // bs) + [n % bs]
    order = s.order(0, n, epoch=3, seed=5)
    assert torch.equal(torch.sort(order).values, torch.arange(n, dtype=torch.int64, device='cuda'))
    assert torch.equal(torch.cat(parts, 0).view(torch.int32), full[order].view(torch.int32))
    s.close()


def test_bijection_at_the_shipped_scale():
    """The technicolor-shaped set (800 images of 2048 x 1088, every pixel: 1 782 579 200 > 2^30 rays): the epoch's order, walked in
    chunks, marks every element exactly once.  The pixel store is allocated (5.3 GB) but never read: only the order is asked for."""
    L = _lib.load()
    W, H, N = 2048, 1088, 800
    h = C.c_void_p()
    assert L.hr_rayset_create(N, W, H, 8, None, C.byref(h)) == 0, L.hr_last_error()
    try:
        img = torch.zeros((H, W, 3), dtype=torch.uint8, device='cuda')
        pose = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
        K = np.array([[2400.0, 0, W / 2], [0, 2400.0, H / 2], [0, 0, 1]])
        for i in range(N):
            cam = make_camera(pose, K, W, H, float(i % 16), (i // 16) / 49.0)
            assert L.hr_rayset_set_image(h, i, C.byref(cam), 1, 0, C.c_void_p(img.data_ptr())) == 0, L.hr_last_error()
        size = int(L.hr_rayset_size(h))
        assert size == N * W * H == 1782579200 and size > 1 << 30
        mark = torch.zeros((size,), dtype=torch.bool, device='cuda')
        chunk = 1 << 26
        buf = torch.empty((chunk,), dtype=torch.int64, device='cuda')
        lo_seen, hi_seen = size, -1
        for first in range(0, size, chunk):
            n = min(chunk, size - first)
            assert L.hr_rayset_order(h, first, n, 7, 2, C.c_void_p(buf.data_ptr()), _stream()) == 0, L.hr_last_error()
            part = buf[:n]
            lo_seen, hi_seen = min(lo_seen, int(part.min())), max(hi_seen, int(part.max()))
            assert lo_seen >= 0 and hi_seen < size             # checked BEFORE the elements index anything
            mark[part] = True
        # `size` rows were drawn; all `size` elements are marked, so none was drawn twice
        assert int(mark.sum(dtype=torch.int64)) == size
        assert (lo_seen, hi_seen) == (0, size - 1)
        del mark, buf
    finally:
        L.hr_rayset_destroy(h)


def test_a_training_step_fed_by_the_set():
    g, fn = _fn('technicolor_z_plane_small')
    f = CC.load('video_ndc')
    s = _set_of(f)
    fn.train()
    try:
        m = fn.model
        b = s.batch(0, 2048, epoch=0, seed=1)
        assert all(v.dtype == torch.float32 and v.is_contiguous() and v.device.type == 'cuda' for v in b.values())
        assert b['coords'].shape == (2048, 8) and b['rgb'].shape == (2048, 3) and b['weight'].shape == (2048, 1)
        params = [p for p in m.parameters() if p.requires_grad]
        for p in params:
            p.grad = None
        loss = (b['weight'] * (m.forward_train(b['coords'], white_bg=False) - b['rgb']) ** 2).mean()
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and float(loss.detach()) > 0.0
        grads = [p.grad for p in params if p.grad is not None]
        assert grads and all(torch.isfinite(gr).all() for gr in grads) and any(float(gr.abs().max()) > 0 for gr in grads)
        for p in params:
            p.grad = None
    finally:
        fn.eval()
        s.close()


def test_refused_calls():
    L = _lib.load()
    f = CC.load('static_pinhole')
    s = _set_of(f)
    n = len(s)
    buf = torch.empty((16, 8), device='cuda')
    p = C.c_void_p(buf.data_ptr())

    def refused(rc, word):
        msg = L.hr_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    refused(L.hr_rayset_batch(s._h, n - 8, 16, 0, 0, None, p, p, p, _stream()), 'outside')           # first + n > size: not a wrap
    refused(L.hr_rayset_batch(s._h, -1, 4, 0, 0, None, p, p, p, _stream()), 'outside')
    refused(L.hr_rayset_order(s._h, n, 1, 0, 0, p, _stream()), 'outside')
    refused(L.hr_rayset_batch(None, 0, 4, 0, 0, None, p, p, p, _stream()), 'null set')
    refused(L.hr_rayset_order(None, 0, 4, 0, 0, p, _stream()), 'null set')
    assert L.hr_rayset_size(None) < 0
    assert L.hr_rayset_batch(s._h, n, 0, 0, 0, None, p, p, p, _stream()) == 0                         # an empty range at the end is fine
    h = C.c_void_p()
    refused(L.hr_rayset_create(2, 8, 8, 7, None, C.byref(h)), 'ray_dim')
    refused(L.hr_rayset_create(0, 8, 8, 6, None, C.byref(h)), 'bad shape')
    bad = make_ndc(dict(fx=0.0, fy=1.0, near=1.0, width=8, height=8))
    refused(L.hr_rayset_create(2, 8, 8, 6, C.byref(bad), C.byref(h)), 'hr_ndc')
    assert not h.value
    W, H = int(f['img_wh'][0]), int(f['img_wh'][1])
    cam = make_camera(f['poses'][0], f['intrinsics'][0], W, H)
    img = np.zeros((H, W, 3), np.uint8)
    ip = C.c_void_p(img.ctypes.data)
    refused(L.hr_rayset_set_image(s._h, 0, C.byref(cam), 0, 0, ip), 'every')
    refused(L.hr_rayset_set_image(s._h, 0, C.byref(cam), 2, -1, ip), 'every')
    refused(L.hr_rayset_set_image(s._h, 1, C.byref(cam), 1, 0, ip), 'image 1')
    refused(L.hr_rayset_set_image(s._h, 0, C.byref(cam), 1, 0, None), 'null')
    small = make_camera(f['poses'][0], f['intrinsics'][0], W - 1, H)
    refused(L.hr_rayset_set_image(s._h, 0, C.byref(small), 1, 0, ip), 'bad camera')
    refused(L.hr_generate_rays_ndc(C.byref(cam), None, 5, 0, 4, p, _stream()), 'ray_dim')
    refused(L.hr_generate_rays_ndc(C.byref(cam), C.byref(bad), 6, 0, 4, p, _stream()), 'hr_ndc')
    refused(L.hr_generate_rays_ndc(C.byref(cam), None, 6, W * H - 2, 4, p, _stream()), 'pixel range')
    assert len(s) == n and int(L.hr_rayset_size(s._h)) == n                                            # the refused calls changed nothing
    with pytest.raises(RuntimeError, match='hr_rayset_batch.*outside'):
        _lib.check(L.hr_rayset_batch(s._h, n, 1, 0, 0, None, p, p, p, _stream()), 'hr_rayset_batch')
    with pytest.raises(ValueError, match='ndc needs'):
        make_ndc(dict(fx=1.0, fy=1.0, near=1.0))
    s.close()
