"""`-m gpu`: fisheye camera rays (hr_generate_rays_fisheye, generate_rays / render_camera with fisheye=) and training sets of fisheye
images (hr_rayset_set_image_fisheye, DeviceRaySet(distortions=)) against hyperreel_amd/csrc/hr_camera.h compiled for the host, bit for
bit, and against the float64 oracle of tests/fisheye_common.py within its bars (4 x the numpy float32 evaluation's own distance to the
oracle, capped at 1e-5: origins 1e-5, directions 4.97e-6).  Colours and weights are exact.  Nothing here provokes a fault: the refused
calls are refused on the host before anything is launched.

A NULL hr_fisheye / fisheye=None and an all-zero pair are both the pinhole call, bit for bit (the interface's convention for "no
distortion given": include/hyperreel_hip.h)."""
import ctypes as C

import numpy as np
import pytest
import torch

import fisheye_common as FC
from helpers import Golden
from hyperreel_amd import lib as _lib
from hyperreel_amd.data import DeviceRaySet, make_fisheye, make_ndc
from hyperreel_amd.plan import hr_fisheye

pytestmark = pytest.mark.gpu

GUARD = 64


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _abi_rays(name, pair, ndc, rd, first, n, cam_id=3.0, time=0.25, misalign=0):
    """One C-ABI call into a NaN-filled buffer with 64 guard floats on either side: every element of the range is written, no other."""
    L = _lib.load()
    cam, fe, nd = FC.camera_of(name, cam_id, time), make_fisheye(pair), make_ndc(ndc)
    flat = torch.full((GUARD + misalign + n * rd + GUARD,), float('nan'), device='cuda')
    out = flat[GUARD + misalign:GUARD + misalign + n * rd].view(n, rd)
    rc = L.hr_generate_rays_fisheye(C.byref(cam), C.byref(fe) if fe is not None else None, C.byref(nd) if nd is not None else None, rd, first, n,
                                    C.c_void_p(out.data_ptr()), _stream())
    assert rc == 0, L.hr_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(flat[:GUARD + misalign]).all() and torch.isnan(flat[GUARD + misalign + n * rd:]).all()
    assert not torch.isnan(out).any()
    return out


def _ranges(size):
    """(first, n): the head, an odd middle piece, a piece ending at the last pixel, an empty one inside and one at the end"""
    mid = (min(5, size - 1), max(1, min(size - 6, 2 * size // 3)))
    return [(0, min(size, 7)), mid, (size - min(size, 9), min(size, 9)), (min(3, size), 0), (size, 0)]


@pytest.mark.parametrize('name', list(FC.CASES))
def test_generate_rays_against_the_host_header_and_the_oracle(name):
    hf = FC.host_lib()
    W, H = FC.CASES[name][:2]
    size = W * H
    for pair in FC.PAIRS:
        for ndc in (None, FC.NDC):
            host = FC.host_rays(hf, name, pair, ndc)
            for rd in (6, 8):
                full = _abi_rays(name, pair, ndc, rd, 0, size)
                got = full.cpu().numpy()
                assert np.array_equal(got[:, :6].view(np.uint32), host.view(np.uint32)), (name, pair, ndc, rd)     # the same source, bit for bit
                if rd == 8:
                    assert np.array_equal(got[:, 6:], np.broadcast_to(np.float32([3.0, 0.25]), (size, 2)))
                FC.check_coords(got, FC.oracle(name, pair, ndc), f'{name} {pair} ndc={ndc is not None} rd={rd}')
                if pair != FC.PAIRS[1]:
                    continue
                for first, n in _ranges(size):
                    part = _abi_rays(name, pair, ndc, rd, first, n)
                    assert torch.equal(_bits(part), _bits(full[first:first + n])), (name, rd, first, n)
                first, n = _ranges(size)[1]                     # off a 16-byte boundary: the same stores take it
                part = _abi_rays(name, pair, ndc, rd, first, n, misalign=1)
                assert torch.equal(_bits(part), _bits(full[first:first + n]))


def _pinhole(name, ndc, rd, first, n):
    L = _lib.load()
    cam, nd = FC.camera_of(name, 3.0, 0.25), make_ndc(ndc)
    out = torch.full((n, rd), float('nan'), device='cuda')
    if nd is None:
        rc = L.hr_generate_rays(C.byref(cam), rd, first, n, C.c_void_p(out.data_ptr()), _stream())
    else:
        rc = L.hr_generate_rays_ndc(C.byref(cam), C.byref(nd), rd, first, n, C.c_void_p(out.data_ptr()), _stream())
    assert rc == 0, L.hr_last_error()
    torch.cuda.synchronize()
    return out


def test_no_distortion_is_generate_rays_bit_for_bit():
    for name in ('centred', 'off_centre'):
        W, H = FC.CASES[name][:2]
        for ndc in (None, FC.NDC):
            for rd in (6, 8):
                for first, n in ((0, W * H), (5, 100), (W * H - 7, 7)):
                    a = _abi_rays(name, None, ndc, rd, first, n)
                    assert torch.equal(_bits(a), _bits(_pinhole(name, ndc, rd, first, n))), (name, ndc, rd, first, n)


def test_a_zero_pair_is_generate_rays_bit_for_bit():
    for name in ('centred', 'off_centre'):
        W, H = FC.CASES[name][:2]
        for ndc in (None, FC.NDC):
            for rd in (6, 8):
                a = _abi_rays(name, (0.0, 0.0), ndc, rd, 0, W * H)
                b = _pinhole(name, ndc, rd, 0, W * H)
                assert torch.equal(_bits(a), _bits(b)), (name, ndc, rd)


def _set(ndc, video=True):
    names = FC.SET_NAMES
    poses = np.stack([FC.CASES[n][3] for n in names])
    Ks = np.stack([FC.CASES[n][2] for n in names])
    return DeviceRaySet(FC.set_images(), poses, Ks, FC.SET_TIMES if video else None, FC.SET_CAM_IDS if video else None, (24, 14), ndc=ndc,
                        subsample=FC.SET_RULES, distortions=np.array(FC.SET_PAIRS))


def _rows(b):
    return torch.cat([b['coords'], b['rgb'], b['weight']], 1)


@pytest.mark.parametrize('ndc', [None, FC.NDC], ids=['world', 'ndc'])
@pytest.mark.parametrize('video', [True, False], ids=['8col', '6col'])
def test_a_set_of_fisheye_images(ndc, video):
    hf = FC.host_lib()
    coords64, rgb, rows = FC.set_oracle(ndc)
    s = _set(ndc, video)
    n, rd = len(s), 8 if video else 6
    assert n == coords64.shape[0] == sum(len(FC.set_kept(i)) for i in range(3)) and 336 < n < 3 * 336 and s.ray_dim == rd
    idx = torch.arange(n, dtype=torch.int64, device='cuda')
    b = s.batch(0, 0, indices=idx)
    torch.cuda.synchronize()
    got = b['coords'].cpu().numpy()
    FC.check_coords(got, coords64, f'set ndc={ndc is not None} rd={rd}')
    assert np.array_equal(b['rgb'].cpu().numpy(), rgb) and np.array_equal(b['weight'].cpu().numpy(), np.ones((n, 1), np.float32))
    nd = make_ndc(ndc)
    for i, (lo, hi) in enumerate(rows):                          # bit for bit the host-compiled header, image by image
        cam, fe = FC.camera_of(FC.SET_NAMES[i]), make_fisheye(FC.SET_PAIRS[i])
        host = np.empty((24 * 14, 6), np.float32)
        k = hf.hf_subsampled_rays(C.byref(cam), C.byref(fe), C.byref(nd) if nd is not None else None, FC.SET_RULES[i][0], FC.SET_RULES[i][1],
                                  host.ctypes.data_as(C.c_void_p))
        assert k == hi - lo and np.array_equal(got[lo:hi, :6].view(np.uint32), host[:k].view(np.uint32)), i
        if video:
            assert np.array_equal(got[lo:hi, 6:], np.broadcast_to(np.float32([FC.SET_CAM_IDS[i], FC.SET_TIMES[i]]), (k, 2)))
    full = _rows(b)
    # batch, sample and batch(indices=) agree bit for bit
    order = s.order(0, n, epoch=1, seed=4)
    assert torch.equal(torch.sort(order).values, idx)
    bs = 200
    e = torch.cat([_rows(s.batch(i, bs, epoch=1, seed=4)) for i in range((n + bs - 1) // bs)], 0)
    assert torch.equal(_bits(e), _bits(full[order]))
    assert torch.equal(_bits(_rows(s.batch(0, 0, indices=order[:bs].contiguous()))), _bits(e[:bs]))
    drawn = s.sample(300, step=7, seed=2, want_elements=True)
    el = drawn['elements']
    assert int(el.min()) >= 0 and int(el.max()) < n
    assert torch.equal(_bits(_rows(drawn)), _bits(full[el]))
    # a second stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _rows(s.batch(1, bs, epoch=1, seed=4))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(_bits(other), _bits(e[bs:2 * bs]))
    # a captured graph replayed into NaN-poisoned fixed buffers
    out = {'coords': torch.empty((bs, rd), device='cuda'), 'rgb': torch.empty((bs, 3), device='cuda'), 'weight': torch.empty((bs, 1), device='cuda')}
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.batch(1, bs, epoch=1, seed=4, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.batch(1, bs, epoch=1, seed=4, out=out)
    for _ in range(2):
        for t in out.values():
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(_rows(out)), _bits(e[bs:2 * bs]))
    s.close()


def test_generation_replays_from_a_graph():
    L = _lib.load()
    name, pair = 'short_focal', FC.PAIRS[3]
    want = _abi_rays(name, pair, FC.NDC, 8, 0, 24 * 14)
    cam, fe, nd = FC.camera_of(name, 3.0, 0.25), make_fisheye(pair), make_ndc(FC.NDC)
    out = torch.empty((24 * 14, 8), device='cuda')
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert L.hr_generate_rays_fisheye(C.byref(cam), C.byref(fe), C.byref(nd), 8, 0, 24 * 14, C.c_void_p(out.data_ptr()), _stream()) == 0
    for _ in range(2):
        out.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(want))


def test_pinhole_and_fisheye_images_mix_and_bad_calls_are_refused():
    L = _lib.load()
    s = _set(None)
    n = len(s)
    idx = torch.arange(n, dtype=torch.int64, device='cuda')
    before = _rows(s.batch(0, 0, indices=idx)).clone()
    img = np.ascontiguousarray(FC.set_images()[0])
    ip = C.c_void_p(img.ctypes.data)
    cam = FC.camera_of('centred', FC.SET_CAM_IDS[0], FC.SET_TIMES[0])

    def refused(rc, word):
        msg = L.hr_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    for pair in FC.NOT_INVERTIBLE:
        refused(L.hr_rayset_set_image_fisheye(s._h, 0, C.byref(cam), C.byref(hr_fisheye(*pair)), 1, 0, ip), 'not invertible')
    good = make_fisheye(FC.SET_PAIRS[0])
    refused(L.hr_rayset_set_image_fisheye(s._h, 3, C.byref(cam), C.byref(good), 1, 0, ip), 'image 3')
    refused(L.hr_rayset_set_image_fisheye(s._h, 0, C.byref(cam), C.byref(good), 0, 0, ip), 'every')
    refused(L.hr_rayset_set_image_fisheye(s._h, 0, C.byref(cam), C.byref(good), 1, 0, None), 'null')
    assert torch.equal(_bits(_rows(s.batch(0, 0, indices=idx))), _bits(before))            # the refused calls changed nothing
    # image 0 set again without a distortion: its rows become the pinhole rays, the other images keep their bits
    assert L.hr_rayset_set_image_fisheye(s._h, 0, C.byref(cam), None, 1, 0, ip) == 0, L.hr_last_error()
    after = _rows(s.batch(0, 0, indices=idx))
    assert torch.equal(_bits(after[336:]), _bits(before[336:])) and not torch.equal(after[:336, :6], before[:336, :6])
    assert torch.equal(_bits(after[:336, :6]), _bits(_pinhole('centred', None, 6, 0, 336)))
    s.close()
    from hyperreel_amd.data import make_lightfield
    lfs = DeviceRaySet.from_lightfield(np.zeros((1, 14, 24, 3), np.uint8), [(0.0, 0.0)], make_lightfield(24, 14))
    refused(L.hr_rayset_set_image_fisheye(lfs._h, 0, C.byref(cam), C.byref(good), 1, 0, ip), 'light-field')
    lfs.close()
    with pytest.raises(RuntimeError, match='not invertible'):
        DeviceRaySet(FC.set_images(), np.stack([FC.CASES['centred'][3]] * 3), FC.CASES['centred'][2], None, None, (24, 14),
                     distortions=np.array([[0.0, 0.0], [-0.5, 0.1], [0.0, 0.0]]))


def test_render_camera_with_a_fisheye():
    from gpu_common import make_render_fn
    from hyperreel_oracle import HyperReelOracle
    g = Golden('immersive_sphere_small')
    m = make_render_fn(g.cfg, g.dataset, g.state_dict, iteration=g.iteration).model
    name, pair = 'centred', FC.PAIRS[1]
    W, H, K, pose = FC.CASES[name]
    t, cam_id = 0.25, 3.0
    rays = m.generate_rays(pose, K, W, H, time=t, cam_id=cam_id, fisheye=pair)
    rd = rays.shape[1]
    assert torch.equal(_bits(rays), _bits(_abi_rays(name, pair, None, rd, 0, W * H)))
    assert torch.equal(_bits(m.generate_rays(pose, K, W, H, time=t, cam_id=cam_id, fisheye=make_fisheye(pair))), _bits(rays))
    plain = m.generate_rays(pose, K, W, H, time=t, cam_id=cam_id)
    assert torch.equal(_bits(m.generate_rays(pose, K, W, H, time=t, cam_id=cam_id, fisheye=None)), _bits(plain)) and not torch.equal(plain, rays)
    want = m.render(rays, frame_time=t)['rgb'].clone()
    got = m.render_camera(pose, K, W, H, time=t, cam_id=cam_id, fisheye=pair)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want))
    part = m.render_camera(pose, K, W, H, time=t, cam_id=cam_id, pixel_range=(W, 3 * W), fisheye=pair)
    assert torch.equal(_bits(part), _bits(want[W:3 * W]))
    # the oracle's render of the ORACLE's rays
    ref_rays = FC.oracle(name, pair, None).astype(np.float32)
    if rd == 8:
        ref_rays = np.concatenate([ref_rays, np.broadcast_to(np.float32([cam_id, t]), (W * H, 2))], 1)
    ref = HyperReelOracle(g.cfg, g.dataset, g.state_dict, iteration=g.iteration).render(np.ascontiguousarray(ref_rays))['rgb']
    err = float(np.abs(got.cpu().numpy() - ref).max())
    print(f'immersive_sphere_small through a fisheye {pair}: L-inf RGB vs the oracle on the oracle\'s rays {err:.3e}; mean rgb {float(ref.mean()):.3f}, '
          f'std {float(ref.std()):.3f}', flush=True)
    assert err <= 1e-4
