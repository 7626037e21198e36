"""Shared by tests/test_sampler_host.py and tests/test_gpu_sampler.py: the host build of hyperreel_amd/csrc/hr_sample_rng.h (the draw of
hr_rayset_sample) and the sequences it yields."""
import ctypes as C
import os

import numpy as np

from helpers import build_host_lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'host_math', 'hr_sample_rng_host.cpp')
OUT = os.path.join(HERE, 'host_math', '_build', 'libhr_sample_rng_host.so')


def host_lib():
    build_host_lib(OUT, SRC, [SRC, os.path.join(HERE, '..', 'hyperreel_amd', 'csrc', 'hr_sample_rng.h')])
    lib = C.CDLL(OUT)
    lib.hs_philox.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.hs_philox.restype = None
    lib.hs_draws.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.hs_draws.restype = None
    lib.hs_elements.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.hs_elements.restype = None
    return lib


def host_elements(lib, size, seed, step, n, first=0):
    """Set elements of rows [first, first + n) of (seed, step) over a set of `size` rays: (n) uint64."""
    out = np.empty(int(n), np.uint64)
    lib.hs_elements(int(size), int(seed), int(step), int(first), int(n), out.ctypes.data_as(C.c_void_p))
    return out
