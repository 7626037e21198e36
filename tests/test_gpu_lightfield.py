"""`-m gpu`: two-plane light-field rays (hr_generate_rays_lightfield, hr_generate_rays_epi, generate_lightfield_rays /
render_lightfield_view / generate_epi_rays / render_epi) and light-field training sets (hr_rayset_create_lightfield,
hr_rayset_set_view, DeviceRaySet.from_lightfield) against the reference's own get_lightfield_rays / get_epi_rays
(tests/golden/lightfield, written by tools/make_lightfield_golden.py) and against hyperreel_amd/csrc/hr_lightfield.h compiled for
the host.  Reads only committed fixtures.

The bar for ray coordinates is lightfield_common.bars(): 4 x the reference's own float32-to-float64 distance per column group,
capped at 1e-5 (origins 5.4e-8, directions 2.7e-6 on the committed fixtures); origins are asserted bit for bit; colours and
weights are exact.  Nothing here provokes a fault: the refused calls are refused on the host before anything is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import lightfield_common as LC
from helpers import Golden
from hyperreel_amd import lib as _lib
from hyperreel_amd.data import DeviceRaySet, make_camera, make_lightfield

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


def _abi_rays(lf, epi, a, b, lo, n, base=None):
    """One C-ABI call into a NaN-filled buffer: every element must have been overwritten."""
    L = _lib.load()
    out = torch.full((n, 6), float('nan'), device='cuda') if base is None else base
    fn = L.hr_generate_rays_epi if epi else L.hr_generate_rays_lightfield
    rc = fn(C.byref(lf), float(a), float(b), lo, n, C.c_void_p(out.data_ptr()), _stream())
    assert rc == 0, L.hr_last_error()
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ranges(size):
    """(first, n): the head, an odd middle piece, a piece ending at the last row, an empty one inside and one at the end"""
    mid = (min(5, size - 1), max(1, min(size - 6, 2 * size // 3)))
    return [(0, min(size, 7)), mid, (size - min(size, 9), min(size, 9)), (min(3, size), 0), (size, 0)]


@pytest.mark.parametrize('name', LC.VIEW_CASES)
def test_view_rays_against_the_reference_and_the_host_header(name):
    f = LC.load(name)
    lf = LC.lightfield_of(f)
    size = int(f['width']) * int(f['height'])
    host = LC.host_rays(LC.host_lib(), f)
    for i, (s, t) in enumerate(f['st']):
        lo, hi = LC.view_rows(f, i)
        full = _abi_rays(lf, False, s, t, 0, size)
        got = full.cpu().numpy()
        LC.check_coords(got, f['rays'][lo:hi], f'{name} view {i}')
        assert np.array_equal(got.view(np.uint32), host[lo:hi].view(np.uint32)), (name, i)        # the same source, bit for bit
        if i > 1:
            continue
        for first, n in _ranges(size):
            part = _abi_rays(lf, False, s, t, first, n)
            assert torch.equal(_bits(part), _bits(full[first:first + n])), (name, i, first, n)
        # a range into a buffer that starts off an 8-byte boundary (the same stores take it)
        first, n = _ranges(size)[1]
        flat = torch.full((n * 6 + 1,), float('nan'), device='cuda')
        part = _abi_rays(lf, False, s, t, first, n, base=flat[1:].view(n, 6))
        assert torch.equal(_bits(part), _bits(full[first:first + n])) and torch.isnan(flat[0])


@pytest.mark.parametrize('name', LC.EPI_CASES)
def test_epi_rays_against_the_reference_and_the_host_header(name):
    f = LC.load(name)
    lf = LC.lightfield_of(f)
    size = int(f['width']) * int(f['height'])
    v, t = float(f['v']), float(f['t'])
    full = _abi_rays(lf, True, v, t, 0, size)
    got = full.cpu().numpy()
    LC.check_coords(got, f['rays'], name)
    assert np.array_equal(got.view(np.uint32), LC.host_rays(LC.host_lib(), f).view(np.uint32))
    for first, n in _ranges(size):
        part = _abi_rays(lf, True, v, t, first, n)
        assert torch.equal(_bits(part), _bits(full[first:first + n])), (name, first, n)
    first, n = _ranges(size)[1]
    flat = torch.full((n * 6 + 1,), float('nan'), device='cuda')
    part = _abi_rays(lf, True, v, t, first, n, base=flat[1:].view(n, 6))
    assert torch.equal(_bits(part), _bits(full[first:first + n])) and torch.isnan(flat[0])


def _set_of(f, subsample=None):
    return DeviceRaySet.from_lightfield(f['images'], f['st'], LC.lightfield_of(f), subsample=subsample)


def _rows(b):
    return torch.cat([b['coords'], b['rgb'], b['weight']], 1)


@pytest.mark.parametrize('name', LC.VIEW_CASES)
def test_set_elements_are_the_generated_rays(name):
    """Element e of a from_lightfield set: views in index order, row-major within a view; the ray bit for bit what
    hr_generate_rays_lightfield gives for that pixel, the colour u8 / 255 exactly, weight 1."""
    f = LC.load(name)
    lf = LC.lightfield_of(f)
    size = int(f['width']) * int(f['height'])
    s = _set_of(f)
    n = len(s)
    assert n == f['rays'].shape[0] == size * len(f['st']) and s.ray_dim == 6
    b = s.batch(0, 0, indices=torch.arange(n, dtype=torch.int64, device='cuda'))
    torch.cuda.synchronize()
    assert b['coords'].shape == (n, 6) and b['rgb'].shape == (n, 3) and b['weight'].shape == (n, 1)
    gen = torch.cat([_abi_rays(lf, False, sv, tv, 0, size) for sv, tv in f['st']], 0)
    assert torch.equal(_bits(b['coords']), _bits(gen))
    LC.check_coords(b['coords'].cpu().numpy(), f['rays'], f'{name} set')
    want_rgb = f['images'].reshape(-1, 3).astype(np.float32) / np.float32(255.0)
    assert np.array_equal(b['rgb'].cpu().numpy(), want_rgb)
    assert np.array_equal(b['weight'].cpu().numpy(), np.ones((n, 1), np.float32))
    # a caller's index outside the set: a NaN row of weight 0, nothing read
    odd = torch.tensor([0, -1, n, n - 1], dtype=torch.int64, device='cuda')
    o = s.batch(0, 0, indices=odd)
    assert torch.isnan(o['coords'][1:3]).all() and torch.isnan(o['rgb'][1:3]).all() and o['weight'].flatten().tolist() == [1.0, 0.0, 0.0, 1.0]
    assert torch.equal(_bits(o['coords'][0]), _bits(b['coords'][0])) and torch.equal(_bits(o['coords'][3]), _bits(b['coords'][-1]))
    s.close()


def test_the_checkerboard_rule_on_views():
    """The same rule as on posed images: view i keeps the pixels with (x + y + offset) % every == 0, in row-major order."""
    f = LC.load('default_plane')
    W, H = int(f['width']), int(f['height'])
    rules = [(1, 0), (3, 0), (3, 1), (4, 2), (1, 0), (7, 5)]
    s = _set_of(f, subsample=rules)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    keep = np.concatenate([(((x + y + o) % e) == 0).reshape(-1) for e, o in rules])
    assert len(s) == int(keep.sum())
    b = s.batch(0, 0, indices=torch.arange(len(s), dtype=torch.int64, device='cuda'))
    full = _set_of(f)
    a = full.batch(0, 0, indices=torch.arange(len(full), dtype=torch.int64, device='cuda'))
    sel = torch.from_numpy(np.nonzero(keep)[0]).cuda()
    assert torch.equal(_bits(_rows(b)), _bits(_rows(a)[sel]))
    s.close()
    full.close()


def test_an_epoch_draws_every_ray_once_and_replays_from_a_graph():
    f = LC.load('stanford_like')
    s = _set_of(f)
    n, bs = len(s), 1024
    assert n % bs != 0
    full = _rows(s.batch(0, 0, indices=torch.arange(n, dtype=torch.int64, device='cuda')))
    parts = [_rows(s.batch(i, bs, epoch=2, seed=7)) for i in range((n + bs - 1) // bs)]
    assert parts[-1].shape[0] == n % bs
    e0 = torch.cat(parts, 0)
    order = s.order(0, n, epoch=2, seed=7)
    assert torch.equal(torch.sort(order).values, torch.arange(n, dtype=torch.int64, device='cuda'))      # each element exactly once
    assert torch.equal(_bits(e0), _bits(full[order]))                                                     # and the rows are those elements
    assert not torch.equal(order, s.order(0, n, epoch=3, seed=7))
    # the permutation is the set size's and the key's alone: a posed set of the same size draws the same order
    W, H = int(f['width']), int(f['height'])
    k = len(f['st'])
    posed = DeviceRaySet(f['images'], np.tile(np.eye(4, dtype=np.float32)[:3], (k, 1, 1)), np.array([[40.0, 0, W / 2], [0, 40.0, H / 2], [0, 0, 1]]),
                         None, None, (W, H))
    assert torch.equal(posed.order(0, n, epoch=2, seed=7), order)
    posed.close()
    # one batch replayed from a captured graph into NaN-poisoned fixed buffers, with the runtime's default queue settings
    out = {'coords': torch.empty((bs, 6), device='cuda'), 'rgb': torch.empty((bs, 3), device='cuda'), 'weight': torch.empty((bs, 1), device='cuda')}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.batch(2, bs, epoch=2, seed=7, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.batch(2, bs, epoch=2, seed=7, out=out)
    for _ in range(3):
        for t in out.values():
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(_rows(out)), _bits(e0[2 * bs:3 * bs]))
    s.close()


def test_view_and_epi_generation_replay_from_a_graph():
    f, e = LC.load('default_plane'), LC.load('epi')
    L = _lib.load()
    lf, le = LC.lightfield_of(f), LC.lightfield_of(e)
    nv, ne = int(f['width']) * int(f['height']), int(e['width']) * int(e['height'])
    sv, tv = (float(v) for v in f['st'][4])
    want_v = _abi_rays(lf, False, sv, tv, 0, nv)
    want_e = _abi_rays(le, True, float(e['v']), float(e['t']), 0, ne)
    out_v, out_e = torch.empty((nv, 6), device='cuda'), torch.empty((ne, 6), device='cuda')
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert L.hr_generate_rays_lightfield(C.byref(lf), sv, tv, 0, nv, C.c_void_p(out_v.data_ptr()), _stream()) == 0
        assert L.hr_generate_rays_epi(C.byref(le), float(e['v']), float(e['t']), 0, ne, C.c_void_p(out_e.data_ptr()), _stream()) == 0
    for _ in range(2):
        out_v.fill_(float('nan'))
        out_e.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out_v), _bits(want_v)) and torch.equal(_bits(out_e), _bits(want_e))


def test_render_lightfield_view_and_epi():
    """On the shipped Stanford model: the render forms are render() of the generated rays bit for bit, and two half-ranges are the
    whole view.  The camera plane stands at z = 1 looking down -z, where the fixture's own rays stand."""
    g, fn = _fn('sweep/stanford_z_plane_small')
    m = fn.model
    lf = make_lightfield(37, 23, st_scale=0.125, uv_scale=0.4, near=1.0, far=0.0)
    s, t = 0.35, -0.6
    n = 37 * 23
    rays = m.generate_lightfield_rays(s, t, lf)
    assert rays.shape == (n, 6) and torch.equal(_bits(rays), _bits(_abi_rays(lf, False, s, t, 0, n)))
    want = m.render(rays)['rgb'].clone()
    got = m.render_lightfield_view(s, t, lf)
    torch.cuda.synchronize()
    assert got.shape == (n, 3) and torch.isfinite(got).all()
    assert torch.equal(_bits(got), _bits(want))
    print(f'stanford_z_plane_small view: mean rgb {float(got.mean()):.3f}, std {float(got.std()):.3f}', flush=True)
    half = (n + 1) // 2
    a = m.render_lightfield_view(s, t, lf, pixel_range=(0, half)).clone()
    b = m.render_lightfield_view(s, t, lf, pixel_range=(half, n)).clone()
    assert a.shape == (half, 3) and b.shape == (n - half, 3)
    assert torch.equal(_bits(torch.cat([a, b], 0)), _bits(want))
    assert torch.equal(_bits(m.generate_lightfield_rays(s, t, lf, pixel_range=(half, n))), _bits(rays[half:]))
    le = make_lightfield(37, 19, aspect=37.0 / 23.0, st_scale=0.125, uv_scale=0.4, near=1.0, far=0.0)
    v = 0.1
    er = m.generate_epi_rays(v, t, le)
    assert er.shape == (37 * 19, 6) and torch.equal(_bits(er), _bits(_abi_rays(le, True, v, t, 0, 37 * 19)))
    want_e = m.render(er)['rgb'].clone()
    got_e = m.render_epi(v, t, le)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got_e), _bits(want_e)) and torch.isfinite(got_e).all()
    with pytest.raises(TypeError, match='make_lightfield'):
        m.generate_lightfield_rays(s, t, dict(width=37, height=23))


def test_mismatched_set_kinds_and_bad_arguments_are_refused():
    L = _lib.load()
    f = LC.load('default_plane')
    W, H = int(f['width']), int(f['height'])
    lfs = _set_of(f)
    n = len(lfs)
    k = len(f['st'])
    posed = DeviceRaySet(f['images'], np.tile(np.eye(4, dtype=np.float32)[:3], (k, 1, 1)), np.array([[40.0, 0, W / 2], [0, 40.0, H / 2], [0, 0, 1]]),
                         None, None, (W, H))
    img = np.zeros((H, W, 3), np.uint8)
    ip = C.c_void_p(img.ctypes.data)
    cam = make_camera(np.eye(4)[:3], np.array([[40.0, 0, W / 2], [0, 40.0, H / 2], [0, 0, 1]]), W, H)

    def refused(rc, word):
        msg = L.hr_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    before = _rows(lfs.batch(0, 0, indices=torch.arange(n, dtype=torch.int64, device='cuda'))).clone()
    before_p = _rows(posed.batch(0, 0, indices=torch.arange(n, dtype=torch.int64, device='cuda'))).clone()
    refused(L.hr_rayset_set_image(lfs._h, 0, C.byref(cam), 1, 0, ip), 'hr_rayset_set_view')
    refused(L.hr_rayset_set_view(posed._h, 0, 0.0, 0.0, 1, 0, ip), 'hr_rayset_set_image')
    refused(L.hr_rayset_set_view(lfs._h, k, 0.0, 0.0, 1, 0, ip), f'view {k}')
    refused(L.hr_rayset_set_view(lfs._h, 0, 0.0, 0.0, 0, 0, ip), 'every')
    refused(L.hr_rayset_set_view(lfs._h, 0, 0.0, 0.0, 2, -1, ip), 'every')
    refused(L.hr_rayset_set_view(lfs._h, 0, float('nan'), 0.0, 1, 0, ip), 'non-finite')
    refused(L.hr_rayset_set_view(lfs._h, 0, 0.0, 0.0, 1, 0, None), 'null')
    buf = torch.empty((16, 6), device='cuda')
    p = C.c_void_p(buf.data_ptr())
    refused(L.hr_rayset_batch(lfs._h, n - 8, 16, 0, 0, None, p, p, p, _stream()), 'outside')
    lf = LC.lightfield_of(f)
    refused(L.hr_generate_rays_lightfield(C.byref(lf), 0.0, 0.0, W * H - 2, 4, p, _stream()), 'outside')
    refused(L.hr_generate_rays_epi(C.byref(lf), 0.0, 0.0, -1, 4, p, _stream()), 'outside')
    refused(L.hr_generate_rays_lightfield(C.byref(lf), 0.0, 0.0, 0, 4, None, _stream()), 'null output')
    bad = make_lightfield(W, H, aspect=0.0)
    refused(L.hr_generate_rays_lightfield(C.byref(bad), 0.0, 0.0, 0, 4, p, _stream()), 'bad hr_lightfield')
    # the refused calls changed nothing
    assert len(lfs) == n and int(L.hr_rayset_size(lfs._h)) == n
    assert torch.equal(_bits(_rows(lfs.batch(0, 0, indices=torch.arange(n, dtype=torch.int64, device='cuda')))), _bits(before))
    assert torch.equal(_bits(_rows(posed.batch(0, 0, indices=torch.arange(n, dtype=torch.int64, device='cuda')))), _bits(before_p))
    with pytest.raises(ValueError, match='same number of views'):
        DeviceRaySet.from_lightfield(f['images'][:2], f['st'], lf)
    with pytest.raises(ValueError, match='expected uint8'):
        DeviceRaySet.from_lightfield(f['images'][:, :, :-1], f['st'], lf)
    lfs.close()
    posed.close()
