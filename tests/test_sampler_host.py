"""The sampler with replacement and the capturable optimizer without a GPU: hyperreel_amd/csrc/hr_sample_rng.h compiled for the host against
a numpy restatement of Philox4x32-10 (Salmon et al., SC'11: two 32 x 32 -> 64 multiplies by 0xD2511F53 / 0xCD9E8D57 per round, the key
bumped by the golden-ratio / sqrt(3) Weyl constants between rounds, ten rounds) and of the multiply-high map, written here from that
definition; the sequences' independence of how a call is split; uniformity; the ctypes binding; the argument refusals of the Python
surface.  The kernel's indexing and stores are covered by tests/test_gpu_sampler.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import sampler_common as SC

SEEDS = [0, 1, 2 ** 63 + 5]
STEPS = [0, 1, 2 ** 32, 2 ** 40 + 3]
SIZES = [1, 2, 767, 65537, 2 ** 31 + 11]
ROWS = 4096
M32 = np.uint64(0xFFFFFFFF)


@pytest.fixture(scope='module')
def hs():
    return SC.host_lib()


def np_philox4x32_10(key, c0, c1, c2, c3):
    """key: Python int (64 bits); c0..c3: uint64 arrays holding 32-bit words -> four uint64 arrays of 32-bit words."""
    k0, k1 = key & 0xFFFFFFFF, key >> 32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0                    # (both factors below 2^32: the product fits 64 bits)
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def np_draws(seed, step, rows):
    j = np.asarray(rows, np.uint64)
    s = np.full(j.shape, step, np.uint64)
    w = np_philox4x32_10(seed, j & M32, j >> np.uint64(32), s & M32, s >> np.uint64(32))
    return (w[1] << np.uint64(32)) | w[0]


def np_elements(size, seed, step, rows):
    """floor(u * size / 2^64) in exact integer arithmetic (Python ints)."""
    return np.array([(int(u) * size) >> 64 for u in np_draws(seed, step, rows)], np.uint64)


def test_philox_known_answers(hs):
    """The known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 10): zero, all ones, digits of pi."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        out = np.zeros(4, np.uint32)
        hs.hs_philox(key[0] | key[1] << 32, ctr[0] | ctr[1] << 32, ctr[2] | ctr[3] << 32, out.ctypes.data_as(C.c_void_p))
        assert tuple(int(v) for v in out) == want
        got = np_philox4x32_10(key[0] | key[1] << 32, *[np.array([c], np.uint64) for c in ctr])
        assert tuple(int(v[0]) for v in got) == want


def test_header_equals_the_numpy_restatement(hs):
    rows = np.arange(ROWS, dtype=np.uint64)
    for seed in SEEDS:
        for step in STEPS:
            draws = np.empty(ROWS, np.uint64)
            hs.hs_draws(seed, step, 0, ROWS, draws.ctypes.data_as(C.c_void_p))
            ref = np_draws(seed, step, rows)
            assert np.array_equal(draws, ref), (seed, step)
            for size in SIZES:
                got = SC.host_elements(hs, size, seed, step, ROWS)
                want = np.array([(int(u) * size) >> 64 for u in ref], np.uint64)
                assert np.array_equal(got, want), (seed, step, size)
                assert int(got.max()) < size
                if size == 1:
                    assert not got.any()


def test_distinct_seed_step_pairs_give_distinct_sequences(hs):
    seqs = {(seed, step): SC.host_elements(hs, 65537, seed, step, ROWS) for seed in SEEDS for step in STEPS}
    keys = list(seqs)
    for a in range(len(keys)):
        for b in range(a + 1, len(keys)):
            same = float((seqs[keys[a]] == seqs[keys[b]]).mean())
            assert same < 0.01, (keys[a], keys[b], same)      # independent draws agree at 1 / 65537 of the rows


def test_a_row_depends_on_its_index_alone(hs):
    for seed, step, size in [(0, 0, 767), (2 ** 63 + 5, 2 ** 40 + 3, 2 ** 31 + 11)]:
        whole = SC.host_elements(hs, size, seed, step, ROWS)
        parts = [SC.host_elements(hs, size, seed, step, n, first) for first, n in ((0, 1), (1, 255), (256, 1), (257, 3000), (3257, ROWS - 3257))]
        assert np.array_equal(np.concatenate(parts), whole)
        assert np.array_equal(np_elements(size, seed, step, [ROWS - 1, 17, 0]), whole[[ROWS - 1, 17, 0]])


def test_draws_are_uniform(hs):
    """size 768, 65 536 draws, seeds 0..3 (fixed: the outcome is deterministic).  Every element drawn (the chance of a miss is
    768 * exp(-85.3) ~ 1e-34) and Pearson's statistic below the 1 - 1e-6 quantile of chi2(767): a sound generator fails once in a
    million seeds, a broken map (a bucket twice as likely) exceeds it by far."""
    from scipy import stats
    size, n = 768, 65536
    bar = float(stats.chi2.ppf(1.0 - 1e-6, size - 1))
    rows = np.arange(n, dtype=np.uint64)
    for seed in range(4):
        for name, e in (('header', SC.host_elements(hs, size, seed, 0, n)), ('numpy', np_elements(size, seed, 0, rows))):
            counts = np.bincount(e.astype(np.int64), minlength=size)
            assert counts.min() >= 1, (name, seed)
            expect = n / size
            chi2 = float(((counts - expect) ** 2 / expect).sum())
            print(f'{name} seed {seed}: chi2 {chi2:.1f} (bar {bar:.1f}, mean 767)')
            assert chi2 < bar, (name, seed, chi2, bar)


def test_lib_binds_both_symbols_with_the_documented_types():
    from hyperreel_amd import lib
    bound = {name: (res, args) for name, res, args in lib.SYMBOLS}
    V = C.c_void_p
    # (set, n, seed, step, step_dev, coords, rgb, weight, elements, stream)
    assert bound['hr_rayset_sample'] == (C.c_int, [V, C.c_int64, C.c_uint64, C.c_uint64, V, V, V, V, V, V])
    # (param, grad, exp_avg, exp_avg_sq, n, hp, lr_index, n_lr, lr_dev, step_dev, n_tensors, stream)
    assert bound['hr_adam_step_dev'] == (C.c_int, [V, V, V, V, V, V, V, C.c_int32, V, V, C.c_int32, V])
    L = lib.load()
    assert lib.ABI_VERSION == 27 and L.hr_abi_version() == 27         # additive: the version did not move
    # the refusals that need no device
    assert L.hr_rayset_sample(None, 4, 0, 0, None, None, None, None, None, None) != 0
    assert b'null set' in L.hr_last_error()
    assert L.hr_adam_step_dev(None, None, None, None, None, None, None, 0, None, None, 0, None) == 0        # nothing to step
    assert L.hr_adam_step_dev(None, None, None, None, None, None, None, 0, None, None, 1, None) != 0
    assert L.hr_adam_step_dev(None, None, None, None, None, None, None, 0, None, None, -1, None) != 0


def test_sample_refuses_a_bad_step_tensor_without_a_device():
    from hyperreel_amd.data import DeviceRaySet
    s = DeviceRaySet.__new__(DeviceRaySet)          # no device: the checks run before anything is allocated or launched
    s._h, s.device, s.ray_dim, s._size = None, torch.device('cpu'), 6, 100
    with pytest.raises(ValueError, match='int64 or uint64'):
        s.sample(4, step_tensor=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match='int64 or uint64'):
        s.sample(4, step_tensor=torch.zeros(1, dtype=torch.float32))
    with pytest.raises(ValueError, match='one element'):
        s.sample(4, step_tensor=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match='one element'):
        s.sample(4, step_tensor=torch.zeros((0,), dtype=torch.int64))
    with pytest.raises(TypeError, match='torch tensor'):
        s.sample(4, step_tensor=3)
    with pytest.raises(ValueError, match='n = -1'):
        s.sample(-1)
    s.device = torch.device('cuda', 0)
    with pytest.raises(ValueError, match='is on cpu'):
        s.sample(4, step_tensor=torch.zeros(1, dtype=torch.int64))


def test_capturable_adam_and_graphed_step_refusals_without_a_device():
    from hyperreel_amd.optim import HipAdam
    from hyperreel_amd.train import GraphedStep
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(RuntimeError, match='HIP device'):
        HipAdam([p], capturable=True)
    with pytest.raises(ValueError, match='invalid Adam'):
        HipAdam([p], lr=-1.0, capturable=True)
    plain = HipAdam([p], lr=1e-3)                      # the non-capturable form is constructed as before, without any device state
    assert plain.capturable is False and not hasattr(plain, 'step_tensor')
    assert sorted(plain.state_dict()['param_groups'][0]) == ['betas', 'eps', 'lr', 'params', 'weight_decay']
    plain.sync_hyperparameters()                       # a no-op there
    for opt in (plain, torch.optim.Adam([p], lr=1e-3)):
        with pytest.raises(TypeError, match='capturable=True'):
            GraphedStep(None, opt, None, 96, loss=None)
