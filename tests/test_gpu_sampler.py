"""hr_rayset_sample on the device (DeviceRaySet.sample): the drawn elements against the host build of csrc/hr_sample_rng.h bit for bit, the
rows against hr_rayset_batch(indices = those elements) bit for bit, on a posed set (3 images of 16 x 12, one of them subsampled by the rule
(2, 1), 8-column rays with NDC) and a light-field set (2 x 2 views of 16 x 12); the step read from device memory; one captured launch
replayed while a torch op advances that word.  n: one row, less than a workgroup, more than one workgroup with a ragged tail."""
import ctypes as C

import numpy as np
import pytest
import torch

import sampler_common as SC
from hyperreel_amd import data as D
from hyperreel_amd import lib as _lib

pytestmark = pytest.mark.gpu

W, H = 16, 12
NS = [1, 96, 257]
KEYS = ('coords', 'rgb', 'weight')


@pytest.fixture(scope='module')
def hs():
    return SC.host_lib()


def _posed():
    rng = np.random.default_rng(5)
    images = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    poses = np.tile(np.eye(4, dtype=np.float32)[:3], (3, 1, 1))
    poses[:, :, 3] = [[0.0, 0.0, 1.0], [0.2, -0.1, 1.1], [-0.15, 0.1, 0.9]]
    K = np.array([[20.0, 0, W / 2], [0, 21.0, H / 2], [0, 0, 1]], np.float32)
    return D.DeviceRaySet(images, poses, K, [0.0, 0.5, 1.0], [0, 1, 2], (W, H), ndc=dict(fx=20.0, fy=21.0, near=0.5, width=W, height=H),
                          subsample=[(1, 0), (2, 1), (1, 0)])


def _lightfield():
    rng = np.random.default_rng(6)
    images = rng.integers(0, 256, (4, H, W, 3), dtype=np.uint8)
    st = [D.lightfield_coord(s, t, 2, 2) for t in range(2) for s in range(2)]
    return D.DeviceRaySet.from_lightfield(images, st, D.make_lightfield(W, H))


SETS = {'posed': (_posed, W * H * 2 + W * H // 2, 8), 'lightfield': (_lightfield, 4 * W * H, 6)}


@pytest.fixture(scope='module', params=list(SETS))
def rayset(request):
    make, size, ray_dim = SETS[request.param]
    s = make()
    assert len(s) == size and s.ray_dim == ray_dim
    yield s
    s.close()


def _poisoned(s, n, elements=True):
    out = {'coords': torch.full((n, s.ray_dim), float('nan'), device='cuda'), 'rgb': torch.full((n, 3), float('nan'), device='cuda'),
           'weight': torch.full((n, 1), float('nan'), device='cuda')}
    if elements:
        out['elements'] = torch.full((n,), -7, dtype=torch.int64, device='cuda')
    return out


def _same_bits(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in KEYS)


@pytest.mark.parametrize('n', NS)
def test_rows_are_the_host_sequence_and_what_batch_writes_for_it(rayset, hs, n):
    s = rayset
    for seed, step in [(0, 0), (3, 17), (2 ** 63 + 5, 2 ** 40 + 3)]:
        got = s.sample(n, step=step, seed=seed, out=_poisoned(s, n), want_elements=True)
        torch.cuda.synchronize()
        want = SC.host_elements(hs, len(s), seed, step, n)
        assert np.array_equal(got['elements'].cpu().numpy().astype(np.uint64), want), (seed, step)
        ref = s.batch(0, 0, indices=got['elements'], out=_poisoned(s, n, elements=False))
        torch.cuda.synchronize()
        assert _same_bits(got, ref)
        assert not any(torch.isnan(got[k]).any() for k in KEYS) and bool((got['weight'] == 1).all())
        # fresh tensors, without the elements: the same rows
        plain = s.sample(n, step=step, seed=seed)
        assert sorted(plain) == sorted(KEYS) and _same_bits(plain, got)
        # another stream
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other = s.sample(n, step=step, seed=seed, out=_poisoned(s, n), want_elements=True)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert _same_bits(other, got) and torch.equal(other['elements'], got['elements'])
    # a row depends on its index alone: the first rows of a longer call
    longer = s.sample(n + 300, step=17, seed=3, want_elements=True)
    short = s.sample(n, step=17, seed=3, want_elements=True)
    assert torch.equal(longer['elements'][:n], short['elements']) and all(torch.equal(longer[k][:n].view(torch.int32), short[k].view(torch.int32)) for k in KEYS)


def test_rows_from_a_pointer_off_the_vector_alignment(rayset):
    """coords 4 bytes off the 8 / 16-byte boundary: the scalar-store kernel, the same bits, nothing written outside"""
    s, n = rayset, 96
    flat = torch.full((n * s.ray_dim + 2,), float('nan'), device='cuda')
    out = {'coords': flat[1:1 + n * s.ray_dim].view(n, s.ray_dim), 'rgb': torch.empty((n, 3), device='cuda'), 'weight': torch.empty((n, 1), device='cuda')}
    assert out['coords'].data_ptr() % 8 == 4
    got = s.sample(n, step=2, seed=1, out=out)
    ref = s.sample(n, step=2, seed=1)
    torch.cuda.synchronize()
    assert _same_bits(got, ref) and torch.isnan(flat[0]) and torch.isnan(flat[-1])


@pytest.mark.parametrize('dtype', [torch.int64, torch.uint64])
def test_the_step_is_read_from_device_memory(rayset, dtype):
    s = rayset
    for step in (0, 5, 2 ** 40 + 3):
        word = torch.tensor([step], dtype=torch.int64, device='cuda').view(dtype)
        for n in NS:
            got = s.sample(n, step=123456, seed=9, step_tensor=word, out=_poisoned(s, n), want_elements=True)      # (`step` is not read then)
            ref = s.sample(n, step=step, seed=9, want_elements=True)
            torch.cuda.synchronize()
            assert torch.equal(got['elements'], ref['elements']) and _same_bits(got, ref)


def test_one_captured_launch_draws_a_new_batch_on_every_replay(rayset):
    s, n, first = rayset, 257, 41
    word = torch.tensor(first, dtype=torch.int64, device='cuda')
    out = _poisoned(s, n)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.sample(n, seed=4, step_tensor=word, out=out, want_elements=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.sample(n, seed=4, step_tensor=word, out=out, want_elements=True)
    for k in range(3):
        for key in KEYS:
            out[key].fill_(float('nan'))
        out['elements'].fill_(-7)
        graph.replay()
        ref = s.sample(n, step=first + k, seed=4, want_elements=True)
        torch.cuda.synchronize()
        assert torch.equal(out['elements'], ref['elements']) and _same_bits(out, ref), k
        word += 1                                          # a torch op between the replays
    assert int(word.item()) == first + 3


def test_refusals_and_the_empty_call(rayset):
    s = rayset
    L = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    buf = torch.full((8,), float('nan'), device='cuda')
    p = C.c_void_p(buf.data_ptr())
    assert L.hr_rayset_sample(s._h, 0, 0, 0, None, None, None, None, None, stream) == 0          # n == 0: nothing launched, nothing needed
    assert L.hr_rayset_sample(s._h, 0, 0, 0, None, p, None, None, None, stream) == 0
    assert L.hr_rayset_sample(s._h, -1, 0, 0, None, p, None, None, None, stream) != 0
    assert L.hr_rayset_sample(s._h, 1, 0, 0, None, None, None, None, None, stream) != 0 and b'every output is NULL' in L.hr_last_error()
    assert L.hr_rayset_sample(None, 1, 0, 0, None, p, None, None, None, stream) != 0
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()
    e = s.sample(0, want_elements=True)
    assert tuple(e['coords'].shape) == (0, s.ray_dim) and tuple(e['elements'].shape) == (0,)
    # one output alone (the others NULL)
    only = torch.full((5,), -7, dtype=torch.int64, device='cuda')
    assert L.hr_rayset_sample(s._h, 5, 1, 2, None, None, None, None, C.c_void_p(only.data_ptr()), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(only, s.sample(5, step=2, seed=1, want_elements=True)['elements'])
    with pytest.raises(ValueError, match='is on cpu'):
        s.sample(4, step_tensor=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match=r'out\[\'coords\'\]'):
        s.sample(4, out={'coords': torch.empty((5, s.ray_dim), device='cuda'), 'rgb': torch.empty((4, 3), device='cuda'), 'weight': torch.empty((4, 1), device='cuda')})
