"""`-m gpu`: training sets under the importance subsample rule (hr_rayset_set_image_importance, DeviceRaySet(subsample=[Importance...]))
against the fixtures the reference's own importance_subsample methods wrote (tests/golden/importance, tools/make_importance_golden.py)
and, for the shapes at which a kernel stage can go wrong, against the numpy statement of the rule in tests/importance_common.py on the
host build of hr_importance.h.  Pixel identity, colours and weights are exact; ray coordinates are held to the bars of
tests/fisheye_common.py (lens) or tests/camera_common.py (pinhole).  Nothing here provokes a fault: the refused calls are refused on
the host before anything is launched.

A workgroup of the compaction owns 1024 pixels and the scan of the workgroups' counts walks them in chunks of 256: 640 x 480 is 300
workgroups, so its scan crosses a chunk boundary."""
import ctypes as C

import numpy as np
import pytest
import torch

import camera_common as CC
import importance_common as IC
from hyperreel_amd import lib as _lib
from hyperreel_amd.data import DeviceRaySet, Importance, make_camera, make_lightfield
from hyperreel_amd.plan import hr_fisheye

pytestmark = pytest.mark.gpu

TILE, SCAN_CHUNK = 1024, 256


def _bits(t):
    return t.contiguous().view(torch.int32)


def _all_rows(s):
    return s.batch(0, 0, indices=torch.arange(len(s), dtype=torch.int64, device='cuda'))


def _cat(out):
    return torch.cat([out['coords'], out['rgb'], out['weight']], 1)


@pytest.mark.parametrize('name', IC.CASES)
def test_fixture_sets_are_the_references(name):
    f = IC.load(name)
    ref = f['all_inputs']
    s = IC.set_of(f)
    assert len(s) == ref.shape[0]
    limit = IC.dir_limit(f)
    coords64 = []
    for i in range(f['images'].shape[0]):
        kept = IC.kept_of(f, i)
        got = s.kept_pixels(i).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, kept), (name, i)
        info = s.image_info(i)
        assert info['count'] == len(kept)
        if f['num_take'][i]:
            assert info['is_list'] and info['prev'] == i - 1 and info['num_take'] == f['num_take'][i] and info['dir_z_below'] == (
                None if limit is None else float(np.float32(limit)))
            assert np.float32(info['threshold']).view(np.uint32) == f['threshold'][i].view(np.uint32), (name, i)
        else:
            assert not info['is_list'] and (info['every'], info['offset'], info['prev']) == (1, 0, -1)
        coords64.append(IC.image_rays64(f, i)[kept])
    out = _all_rows(s)
    rows = _cat(out).cpu().numpy()
    assert np.array_equal(rows[:, 8:11], ref[:, 8:11]) and np.array_equal(rows[:, 11], ref[:, 11]) and (rows[:, 11] == 1).all()
    assert np.array_equal(rows[:, 6:8], ref[:, 6:8])                       # camera id and time
    IC.check_coords(f, rows[:, :6].astype(np.float64), np.concatenate(coords64, 0), name)
    if limit is not None:                                                   # every row the set returns passes the test on its own column 5
        listed = np.concatenate([np.full(len(IC.kept_of(f, i)), bool(f['num_take'][i])) for i in range(f['images'].shape[0])])
        assert (rows[listed, 5] < np.float32(limit)).all()
    s.close()


def _pinhole(W, H, yaw=0.1):
    cy, sy = np.cos(yaw), np.sin(yaw)
    pose = np.array([[cy, 0, sy, 0.1], [0, 1, 0, -0.2], [-sy, 0, cy, 0.3]], np.float32)
    K = np.array([[0.8 * W, 0, W / 2 + 0.25], [0, 0.8 * W, H / 2 - 0.5], [0, 0, 1]], np.float32)
    return pose, K


def _pair_set(prev, cur, num_take, limit=None, yaw=0.1):
    """A set of two pinhole images: `prev` kept whole, `cur` under the importance rule against it.  Returns (set, threshold, kept) with
    the numpy rule's answer, the direction test on hr_camera.h's own float32 rays (its host build: the kernels' bits)."""
    H, W = cur.shape[:2]
    pose, K = _pinhole(W, H, yaw)
    s = DeviceRaySet(np.stack([prev, cur]), np.stack([pose, pose]), K, [0.0, 1.0], [0, 0], (W, H), subsample=[(1, 0), Importance(num_take, 0, limit)])
    d_z = None
    if limit is not None:
        cam = make_camera(pose, K, W, H, 0.0, 1.0)
        rays = np.empty((W * H, 6), np.float32)
        CC.host_lib().hc_pixel_rays(C.byref(cam), None, 0, W * H, rays.ctypes.data_as(C.c_void_p))
        d_z = rays[:, 5]
    threshold, kept = IC.select(IC.host_diff(cur, prev), num_take, d_z, limit)
    return s, threshold, kept


def _check_pair(prev, cur, num_take, limit=None, yaw=0.1, what=''):
    s, threshold, kept = _pair_set(prev, cur, num_take, limit, yaw)
    H, W = cur.shape[:2]
    info = s.image_info(1)
    print(f'{what}: {W} x {H}, num_take {num_take}, kept {len(kept)} (device {info["count"]}), threshold {float(threshold):.6g}', flush=True)
    assert np.float32(info['threshold']).view(np.uint32) == threshold.view(np.uint32), what
    assert info['count'] == len(kept) and len(s) == W * H + len(kept), what
    assert np.array_equal(s.kept_pixels(1).cpu().numpy(), kept), what
    if len(kept):
        idx = torch.arange(W * H, len(s), dtype=torch.int64, device='cuda')
        out = s.batch(0, 0, indices=idx)
        assert np.array_equal(out['rgb'].cpu().numpy(), cur.reshape(-1, 3)[kept].astype(np.float32) / np.float32(255)), what
        assert (out['weight'] == 1).all()
        if limit is not None:
            assert (out['coords'][:, 5] < float(np.float32(limit))).all()
    s.close()
    return kept


def test_one_pixel():
    prev, cur = np.array([[[3, 4, 5]]], np.uint8), np.array([[[200, 0, 9]]], np.uint8)
    assert len(_check_pair(prev, cur, 1, what='1 x 1')) == 0            # nothing is strictly above the largest


def test_odd_size_partial_last_workgroup():
    rng = np.random.default_rng(41)
    prev, cur = rng.integers(0, 256, (2, 47, 61, 3), dtype=np.uint8)
    assert (61 * 47) % TILE != 0 and 61 * 47 > 2 * TILE
    kept = _check_pair(prev, cur, 358, what='61 x 47')
    assert 300 < len(kept) <= 357 and kept.max() >= 2 * TILE            # some of them in the partial last workgroup
    _check_pair(prev, cur, 358, limit=-0.05, yaw=1.5, what='61 x 47 with the direction test')


def test_kept_pixels_only_in_the_last_partial_workgroup():
    rng = np.random.default_rng(42)
    prev = rng.integers(0, 256, (47, 61, 3), dtype=np.uint8)
    cur = prev.copy().reshape(-1, 3)
    where = np.sort(rng.choice(np.arange(2 * TILE + 5, 61 * 47), 40, replace=False))
    cur[where, 0] ^= 0x40
    kept = _check_pair(prev, cur.reshape(47, 61, 3), 100, what='last workgroup only')
    assert np.array_equal(kept, where)


def test_num_take_extremes():
    rng = np.random.default_rng(43)
    prev, cur = rng.integers(0, 256, (2, 47, 61, 3), dtype=np.uint8)
    n = 61 * 47
    diff = IC.host_diff(cur, prev)
    kept = _check_pair(prev, cur, n, what='num_take = W * H')          # the threshold is the minimum: all but the pixels equal to it
    assert len(kept) == int((diff > diff.min()).sum()) and len(kept) >= n - 8
    assert len(_check_pair(prev, cur, 1, what='num_take = 1')) == 0     # the threshold is the maximum


def test_plateau_straddling_the_rank():
    rng = np.random.default_rng(44)
    prev = rng.integers(0, 256, (47 * 61, 3), dtype=np.uint8)
    order = rng.permutation(61 * 47)
    plateau, above = order[:1000], order[1000:1200]
    prev[order[:1200]] = (10, 20, 30)                                    # the same bytes, so exactly the same diff
    cur = prev.copy()
    cur[plateau] = (10, 27, 30)                                          # 1000 equal diffs
    cur[above] = (10, 20, 60)                                            # 200 larger ones, equal among themselves too
    prev = prev.reshape(47, 61, 3)
    kept = _check_pair(prev, cur.reshape(47, 61, 3), 700, what='plateau')   # rank 700 from the top lies inside the plateau
    assert np.array_equal(kept, np.sort(above))
    kept = _check_pair(prev, cur.reshape(47, 61, 3), 200, what='plateau, rank on the upper level')   # the 200-th largest IS the upper level
    assert len(kept) == 0
    kept = _check_pair(prev, cur.reshape(47, 61, 3), 1201, what='plateau, rank just below it')        # threshold 0: both levels kept
    assert np.array_equal(kept, np.sort(order[:1200]))


def test_640_by_480_scan_crosses_its_chunk():
    rng = np.random.default_rng(45)
    prev, cur = rng.integers(0, 256, (2, 480, 640, 3), dtype=np.uint8)
    assert (640 * 480 + TILE - 1) // TILE > SCAN_CHUNK
    kept = _check_pair(prev, cur, 38400, limit=-0.05, yaw=1.5, what='640 x 480')
    assert (kept >= SCAN_CHUNK * TILE).any() and (kept < SCAN_CHUNK * TILE).any() and 0.2 < len(kept) / 38400 < 0.8


def test_building_twice_gives_the_same_lists():
    f = IC.load('immersive_small')
    a, b = IC.set_of(f), IC.set_of(f)
    assert len(a) == len(b)
    for i in range(f['images'].shape[0]):
        assert torch.equal(a.kept_pixels(i), b.kept_pixels(i))
        assert a.image_info(i) == b.image_info(i)
    assert torch.equal(_bits(_cat(_all_rows(a))), _bits(_cat(_all_rows(b))))
    a.close(); b.close()


def test_epoch_sample_and_graph():
    f = IC.load('static_background')                                     # whole, listed and one empty image
    s = IC.set_of(f)
    n = len(s)
    assert s.image_info(3)['count'] == 0 and s.image_info(3)['is_list']
    full = _cat(_all_rows(s))
    order = s.order(0, n, epoch=0)
    assert torch.equal(torch.sort(order).values, torch.arange(n, dtype=torch.int64, device='cuda'))
    bs = 1000
    parts = [_cat(s.batch(i, bs, epoch=0)) for i in range((n + bs - 1) // bs)]
    assert torch.equal(_bits(torch.cat(parts, 0)), _bits(full[order]))
    # draws with replacement are set elements, and their rows those elements' rows
    out = s.sample(512, step=3, seed=7, want_elements=True)
    el = out['elements']
    assert int(el.min()) >= 0 and int(el.max()) < n and int((el >= 2867).sum()) > 0
    assert torch.equal(_bits(_cat(out)), _bits(full[el]))
    # replayed from a captured graph into NaN-poisoned outputs: every output element is written
    out = {'coords': torch.empty((bs, s.ray_dim), device='cuda'), 'rgb': torch.empty((bs, 3), device='cuda'), 'weight': torch.empty((bs, 1), device='cuda')}
    side = torch.cuda.Stream()
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
        assert torch.equal(_bits(_cat(out)), _bits(full[order[2 * bs:3 * bs]]))
    s.close()


def test_refusals_leave_the_set_usable():
    L = _lib.load()
    f = IC.load('immersive_small')
    s = IC.set_of(f)
    before = _cat(_all_rows(s))
    W, H = int(f['img_wh'][0]), int(f['img_wh'][1])
    n = f['images'].shape[0]
    img = torch.from_numpy(np.array(f['images'][2])).cuda()
    ip = C.c_void_p(img.data_ptr())
    cam = make_camera(f['poses'][2], f['intrinsics'][2], W, H, 0.0, float(f['times'][2]))
    fe = hr_fisheye(*[float(k) for k in f['distortions'][2]])
    nan = float('nan')

    def refused(rc, word):
        msg = L.hr_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    call = L.hr_rayset_set_image_importance
    refused(call(s._h, 2, C.byref(cam), C.byref(fe), 2, 42, nan, ip), 'prev == i')
    refused(call(s._h, 2, C.byref(cam), C.byref(fe), n, 42, nan, ip), 'outside')
    refused(call(s._h, 2, C.byref(cam), C.byref(fe), -1, 42, nan, ip), 'outside')
    refused(call(s._h, 2, C.byref(cam), C.byref(fe), 1, 0, nan, ip), 'num_take 0')
    refused(call(s._h, 2, C.byref(cam), C.byref(fe), 1, 0, nan, ip), 'MINIMUM')
    refused(call(s._h, 2, C.byref(cam), C.byref(fe), 1, W * H + 1, nan, ip), 'num_take')
    refused(call(s._h, n, C.byref(cam), C.byref(fe), 1, 42, nan, ip), 'image')
    refused(call(s._h, 2, C.byref(cam), C.byref(fe), 1, 42, nan, None), 'null')
    refused(call(s._h, 2, C.byref(cam), C.byref(hr_fisheye(-0.5, 0.1)), 1, 42, nan, ip), 'not invertible')
    small = make_camera(f['poses'][2], f['intrinsics'][2], W - 1, H, 0.0, 0.0)
    refused(call(s._h, 2, C.byref(small), C.byref(fe), 1, 42, nan, ip), 'bad camera')
    # image 2 is the previous frame of the listed image 3: setting it again, by any rule, would leave that list stale
    refused(call(s._h, 2, C.byref(cam), C.byref(fe), 1, 42, nan, ip), 'load order')
    refused(L.hr_rayset_set_image_fisheye(s._h, 2, C.byref(cam), C.byref(fe), 1, 0, ip), 'load order')
    refused(L.hr_rayset_set_image(s._h, 0, C.byref(cam), 1, 0, ip), 'load order')
    refused(L.hr_rayset_image_pixels(s._h, 1, 0, s.image_info(1)['count'] + 1, ip, None), 'outside')
    assert torch.equal(_bits(_cat(_all_rows(s))), _bits(before))            # the refused calls changed nothing
    # the last image of the set is nobody's previous frame: it can be set again, under either rule
    last = n - 1
    cam_l = make_camera(f['poses'][last], f['intrinsics'][last], W, H, float(f['cam_ids'][last]), float(f['times'][last]))
    fe_l = hr_fisheye(*[float(k) for k in f['distortions'][last]])
    img_l = torch.from_numpy(np.array(f['images'][last])).cuda()
    assert call(s._h, last, C.byref(cam_l), C.byref(fe_l), last - 1, 42, nan, C.c_void_p(img_l.data_ptr())) == 0, L.hr_last_error()
    _, kept = IC.select(IC.host_diff(f['images'][last], f['images'][last - 1]), 42)
    assert np.array_equal(s.kept_pixels(last).cpu().numpy(), kept)
    assert int(L.hr_rayset_size(s._h)) == before.shape[0] - W * H + len(kept)
    assert L.hr_rayset_set_image_fisheye(s._h, last, C.byref(cam_l), C.byref(fe_l), 1, 0, C.c_void_p(img_l.data_ptr())) == 0, L.hr_last_error()
    s._size = int(L.hr_rayset_size(s._h))
    assert torch.equal(_bits(_cat(_all_rows(s))), _bits(before))
    s.close()
    # an image whose previous frame is not set yet, in a fresh set
    h = C.c_void_p()
    assert L.hr_rayset_create(3, W, H, 8, None, C.byref(h)) == 0
    refused(call(h, 1, C.byref(cam), C.byref(fe), 0, 42, nan, ip), 'not set yet')
    L.hr_rayset_destroy(h)
    # a light-field set
    lf = make_lightfield(W, H)
    assert L.hr_rayset_create_lightfield(2, C.byref(lf), C.byref(h)) == 0
    refused(call(h, 1, C.byref(cam), None, 0, 42, nan, ip), 'light-field')
    L.hr_rayset_destroy(h)
