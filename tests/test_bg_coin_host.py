"""hr_background_coin (hyperreel_amd/csrc/hr_sample_rng.h) compiled for the host: the per-step background coin the training kernels
flip under hr_train_set_background, and hyperreel_amd.train.background_coin, the library's exported copy of it."""
import numpy as np

import bg_coin_common as B

N = 65536


def test_the_coin_is_a_pure_function_of_seed_and_step():
    lib = B.host_lib()
    a, b = B.coins(lib, 0, 0, N), B.coins(lib, 0, 0, N)
    assert np.array_equal(a, b)
    assert np.array_equal(B.coins(lib, 0, 1000, 50), a[1000:1050])              # a step's coin does not depend on where the sequence starts
    for seed, step in ((0, 0), (7, 3), (2 ** 64 - 1, 2 ** 63 + 5), (123456789, 2 ** 40)):
        assert B.coins(lib, seed, step, 1)[0] == B.coins(lib, seed, step, 1)[0]
    # ... and depends on both: other seeds and the next steps give other sequences
    assert not np.array_equal(a[:256], B.coins(lib, 1, 0, 256)) and not np.array_equal(a[:256], a[1:257])
    assert not np.array_equal(a[:256], B.coins(lib, 2 ** 32, 0, 256))          # the seed's high word is part of the key


def test_the_coin_is_keyed_apart_from_the_samplers_rows():
    """The sampler's row j of step s uses the counter (j, s) with j < 2^63; the coin's counter carries a constant above that, so it is not
    the top bit of any row's first word -- in particular not row 0's, which it agrees with about half the time, as independent bits do
    (5 standard deviations of 65 536 fair comparisons: 640)."""
    lib = B.host_lib()
    assert lib.hb_domain() >= 2 ** 63
    for seed in (0, 7):
        coin, row0 = B.coins(lib, seed, 0, N), B.coins(lib, seed, 0, N, 'hb_sampler_first_bits')
        agree = int((coin == row0).sum())
        print(f'seed {seed}: the coin equals the top bit of the first word of row 0 at {agree} of {N} steps')
        assert abs(agree - N // 2) <= 640


def test_the_coin_is_fair_over_65536_steps_of_seed_0():
    """White at 32 768 +- 640 (5 standard deviations of 65 536 fair flips, sigma = 128) of steps 0 ... 65 535 of seed 0.  The function is
    fixed, so this is one number, not a chance: measured 32 739."""
    white = int(B.coins(B.host_lib(), 0, 0, N).sum())
    print(f'white at {white} of {N} steps')
    assert abs(white - 32768) <= 640


def test_the_python_background_coin_is_the_same_function():
    from hyperreel_amd.train import background_coin
    lib = B.host_lib()
    for seed in (0, 5, 2 ** 64 - 1):
        want = B.coins(lib, seed, 0, 512)
        assert [background_coin(seed, s) for s in range(512)] == want.tolist()
    assert background_coin(3, 2 ** 63 + 11) == bool(B.coins(lib, 3, 2 ** 63 + 11, 1)[0])
