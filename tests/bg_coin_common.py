"""Shared by tests/test_bg_coin_host.py and tests/test_gpu_bg_coin.py: the host build of hr_background_coin
(hyperreel_amd/csrc/hr_sample_rng.h, through tests/host_math/hr_bg_coin_host.cpp)."""
import ctypes as C
import os

import numpy as np

from helpers import build_host_lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'host_math', 'hr_bg_coin_host.cpp')
OUT = os.path.join(HERE, 'host_math', '_build', 'libhr_bg_coin_host.so')


def host_lib():
    build_host_lib(OUT, SRC, [SRC, os.path.join(HERE, '..', 'hyperreel_amd', 'csrc', 'hr_sample_rng.h')])
    lib = C.CDLL(OUT)
    for fn in (lib.hb_coins, lib.hb_sampler_first_bits):
        fn.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
        fn.restype = None
    lib.hb_domain.argtypes = []
    lib.hb_domain.restype = C.c_uint64
    return lib


def coins(lib, seed, first, n, fn='hb_coins'):
    out = np.empty(int(n), np.uint8)
    getattr(lib, fn)(int(seed), int(first), int(n), out.ctypes.data_as(C.c_void_p))
    return out.astype(bool)
