"""The importance subsample rule without a GPU: hr_importance.h compiled for the host against torch's evaluation of the reference's
expression and against the fixtures the reference's own importance_subsample methods wrote (tools/make_importance_golden.py); the
numpy statement of select + mask + compaction that the GPU suite uses as its oracle, against the same fixtures; importance_rule; and
the refusals that need no device."""
import os

import numpy as np
import pytest
import torch

import importance_common as IC
from hyperreel_amd import data
from hyperreel_amd.data import DeviceRaySet, Importance


def _torch_diff(cur, prev):
    """the reference's line on ToTensor's floats (datasets/immersive.py:299), on the CPU where the reference runs it"""
    rgb = torch.from_numpy(cur.reshape(-1, 3)).to(torch.float32).div(255)
    last = torch.from_numpy(prev.reshape(-1, 3)).to(torch.float32).div(255)
    return torch.abs(rgb - last).mean(-1).numpy()


@pytest.mark.parametrize('name', IC.CASES)
def test_diff_equals_the_fixture_bit_for_bit(name):
    f = IC.load(name)
    seen = 0
    for i in range(f['images'].shape[0]):
        if f['num_take'][i] == 0:
            assert np.isnan(f['diff'][i]).all()
            continue
        got = IC.host_diff(f['images'][i], f['images'][i - 1])
        assert got.view(np.uint32).tolist() == f['diff'][i].view(np.uint32).tolist(), (name, i)
        assert np.array_equal(IC.host_keys(f['images'][i], f['images'][i - 1]), got.view(np.uint32))
        seen += 1
    assert seen >= 3


def test_channel_term_over_all_byte_pairs():
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    a, b = a.reshape(-1), b.reshape(-1)
    for ch in range(3):                                   # the term alone in each position of the sum
        cur, prev = np.zeros((65536, 3), np.uint8), np.zeros((65536, 3), np.uint8)
        cur[:, ch], prev[:, ch] = a, b
        got, ref = IC.host_diff(cur, prev), _torch_diff(cur, prev)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), ch
        x, y = a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255)
        assert np.array_equal(got, np.abs(x - y) / np.float32(3))      # ... and it is |a / 255 - b / 255| / 3 in float32


def test_diff_on_four_million_triples():
    rng = np.random.default_rng(31)
    n = 1 << 22
    cur, prev = rng.integers(0, 256, (n, 3), dtype=np.uint8), rng.integers(0, 256, (n, 3), dtype=np.uint8)
    prev[: n // 8] = cur[: n // 8]                          # identical pixels: exactly 0
    prev[n // 8: n // 4, 1:] = cur[n // 8: n // 4, 1:]       # one channel differs
    got, ref = IC.host_diff(cur, prev), _torch_diff(cur, prev)
    bad = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    print(f'{n} triples, {bad} differ', flush=True)
    assert bad == 0
    assert (got[: n // 8] == 0).all() and (got >= 0).all() and np.isfinite(got).all()
    order = np.argsort(got, kind='stable')                  # non-negative finite floats: unsigned order of the bits is float order
    assert (np.diff(got.view(np.uint32)[order].astype(np.int64)) >= 0).all()


@pytest.mark.parametrize('name', IC.CASES)
def test_numpy_rule_reproduces_the_reference(name):
    f = IC.load(name)
    limit = IC.dir_limit(f)
    n_pixels = int(f['img_wh'][0]) * int(f['img_wh'][1])
    rows = 0
    for i in range(f['images'].shape[0]):
        kept = IC.kept_of(f, i)
        if f['num_take'][i] == 0:
            assert np.array_equal(kept, np.arange(n_pixels))
        else:
            d_z = f['video_coords'][f['video_of'][i]][:, 5]
            threshold, got = IC.select(IC.host_diff(f['images'][i], f['images'][i - 1]), int(f['num_take'][i]), d_z, limit)
            assert threshold.view(np.uint32) == f['threshold'][i].view(np.uint32), (name, i)
            assert np.array_equal(got, kept), (name, i)
            assert len(kept) <= f['num_take'][i] - 1
            if limit is not None:
                assert (d_z[kept] < np.float32(limit)).all()
        # ... and all_inputs is those pixels' coords, colours and weight 1
        part = f['all_inputs'][rows:rows + len(kept)]
        assert np.array_equal(part[:, :7], f['video_coords'][f['video_of'][i]][kept])
        assert np.array_equal(part[:, 7], np.full(len(kept), np.float32(f['times'][i])))
        assert np.array_equal(part[:, 8:11], f['images'][i].reshape(-1, 3)[kept].astype(np.float32) / np.float32(255))
        assert (part[:, 11] == 1).all()
        rows += len(kept)
    assert rows == f['all_inputs'].shape[0]


def test_fixtures_hold_the_cases_they_are_for():
    f = IC.load('static_background')
    counts = np.diff(f['kept_rows'])
    assert counts[3] == 0 and counts[4] > 0                               # an empty image in the middle of the set
    assert (f['threshold'][1:] == 0).all() and int((f['diff'][1] == 0).sum()) > 2000     # threshold 0, ties in the thousands
    f = IC.load('immersive_small')
    dz = f['video_coords'][1][:, 5]
    assert 0.2 < float((dz < np.float32(-0.05)).mean()) < 0.8             # the limit's contour crosses camera 1's images
    for name in IC.CASES:
        f = IC.load(name)
        assert max(int((f['diff'][i] == f['threshold'][i]).sum()) for i in range(len(f['threshold']))) >= 2, name


@pytest.mark.parametrize('name', IC.CASES)
def test_importance_rule_reproduces_the_pattern(name):
    f = IC.load(name)
    rules = IC.rule_of(f)
    assert len(rules) == f['images'].shape[0]
    for i, r in enumerate(rules):
        if f['num_take'][i] == 0:
            assert r == (1, 0), (name, i)
        else:
            assert isinstance(r, Importance) and r == Importance(int(f['num_take'][i]), i - 1, IC.dir_limit(f)), (name, i)
    assert not any(isinstance(r, Importance) for r, first in zip(rules, f['first_of_video']) if first)


def test_importance_rule_shipped_config():
    """conf/experiment/dataset/immersive.yaml: 1280 x 960, steps 8 / 4, fractions 0.25 / 0.125"""
    rules = DeviceRaySet.importance_rule(list(range(10)) * 2, 1280 * 960, 8, 4, 0.25, 0.125, ([True] + [False] * 9) * 2)
    assert [isinstance(r, Importance) for r in rules[:10]] == [False, True, True, True, True, True, True, True, False, True]
    assert rules[4] == Importance(307200, 3, -0.05) and rules[5] == Importance(153600, 4, -0.05) and rules[10] == (1, 0)
    assert rules[15] == Importance(153600, 14, -0.05)
    assert DeviceRaySet.importance_rule([1], 100, 8, 4, 0.25, 0.125, [False], dir_z_below=None)[0].dir_z_below is None
    with pytest.raises(ValueError):
        DeviceRaySet.importance_rule([0, 1], 100, 8, 4, 0.25, 0.125, [True])


def test_refusals_without_a_device():
    img = np.zeros((2, 4, 5, 3), np.uint8)
    poses, K = np.tile(np.eye(4, dtype=np.float32)[:3], (2, 1, 1)), np.array([[4, 0, 2.5], [0, 4, 2], [0, 0, 1]], np.float32)
    for take, word in ((0, 'num_take 0'), (-3, 'num_take -3'), (21, 'num_take 21')):
        with pytest.raises(ValueError, match=word):
            DeviceRaySet(img, poses, K, None, None, (5, 4), subsample=[(1, 0), Importance(take)])
    with pytest.raises(ValueError, match='minimum'):          # why 0 is refused and not reproduced
        DeviceRaySet(img, poses, K, None, None, (5, 4), subsample=[(1, 0), Importance(0)])
    for prev in (1, 2, -1):
        with pytest.raises(ValueError, match='prev'):
            DeviceRaySet(img, poses, K, None, None, (5, 4), subsample=[(1, 0), Importance(3, prev)])
    with pytest.raises(ValueError, match='prev'):              # image 0 has no image before it
        DeviceRaySet(img, poses, K, None, None, (5, 4), subsample=[Importance(3), (1, 0)])
    lf = data.make_lightfield(5, 4)
    with pytest.raises(ValueError, match='light-field'):
        DeviceRaySet.from_lightfield(img, [(0, 0), (1, 0)], lf, subsample=[(1, 0), Importance(3)])
    # the names alone stay refused: the rule needs the images
    for rule in ('importance_subsample', 'random_subsample', 'test_subsample'):
        with pytest.raises(NotImplementedError, match=rule):
            DeviceRaySet(None, None, None, None, None, (4, 4), subsample=rule)
        with pytest.raises(NotImplementedError, match=rule):
            DeviceRaySet.video_rule([0, 1], rule=rule)
    assert 'importance_rule' in data.UNSUPPORTED_RULES['importance_subsample']


@pytest.mark.reference
@pytest.mark.parametrize('name', ['immersive_small'])
def test_fixture_regenerates_bit_for_bit(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_importance_golden', os.path.join(IC.HERE, '..', 'tools', 'make_importance_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    new, old = mod.make_case(name), IC.load(name)
    assert sorted(new) == sorted(old)
    for k in old:
        a, b = np.asarray(new[k]), old[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
