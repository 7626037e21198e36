"""Shared by tests/test_lightfield_host.py and tests/test_gpu_lightfield.py: the light-field fixtures (tests/golden/lightfield/*.npz,
written by tools/make_lightfield_golden.py from the reference's own get_lightfield_rays / get_epi_rays), the host build of
hyperreel_amd/csrc/hr_lightfield.h, and the tolerance both suites hold the ray coordinates to.

The tolerance is not a constant of these files.  As for the NDC rays (tests/camera_common.py): per column group (origins,
directions), the bar is 4 x the largest distance between the reference's float32 rays and the float64 evaluation stored beside
them, over all committed fixtures -- two correct float32 evaluations of a divide or a normalise differ by a few ulp -- and never
looser than 1e-5 absolute.  That bar holds the directions (a normalise: torch sums the squares in another order, 1 ulp in about 1 %
of the elements).  Origins are asserted bit for bit: column 2 is `near`, a view's (s, t) * st_scale is the float32 product of two
scalars, and an EPI's s is one IEEE divide and one multiply on a linspace element that hr_linspace reproduces exactly -- nothing in
them depends on an order of operations.  The origins' bar is still computed and printed."""
import ctypes as C
import glob
import os

import numpy as np

from helpers import build_host_lib
from hyperreel_amd.plan import hr_lightfield

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'lightfield')
SRC = os.path.join(HERE, 'host_math', 'hr_lightfield_host.cpp')
OUT = os.path.join(HERE, 'host_math', '_build', 'libhr_lightfield_host.so')
CAP = 1e-5
VIEW_CASES = ['default_plane', 'stanford_like', 'one_wide']
EPI_CASES = ['epi', 'epi_one_row']
CASES = VIEW_CASES + EPI_CASES


def fixture_names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN, '*.npz')))


def load(name):
    with np.load(os.path.join(GOLDEN, f'{name}.npz')) as z:
        return {k: z[k] for k in z.files}


def reference_distances():
    """{'origins': d, 'directions': d}: the largest |reference float32 - float64| over all fixtures."""
    d = {'origins': 0.0, 'directions': 0.0}
    for name in fixture_names():
        f = load(name)
        diff = np.abs(f['rays'].astype(np.float64) - f['coords64'])
        d['origins'] = max(d['origins'], float(diff[:, :3].max()))
        d['directions'] = max(d['directions'], float(diff[:, 3:].max()))
    return d


def bars():
    return {k: min(4.0 * v, CAP) for k, v in reference_distances().items()}


def check_coords(got, ref, what):
    """got, ref: (n, 6) float32.  Prints the measured distances beside the bars, then asserts: origins (columns 0-2) exact, directions
    within bars()."""
    b = bars()
    if got.shape[0] == 0:
        return
    d_o, d_d = float(np.abs(got[:, :3] - ref[:, :3]).max()), float(np.abs(got[:, 3:6] - ref[:, 3:6]).max())
    bits = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    print(f'{what}: origins {d_o:.3e} (bar {b["origins"]:.3e}) directions {d_d:.3e} (bar {b["directions"]:.3e}); '
          f'{bits} of {got.size} floats differ in bits', flush=True)
    assert np.array_equal(got[:, :3].view(np.uint32), ref[:, :3].view(np.uint32)), what
    assert d_o <= b['origins'] and d_d <= b['directions'], what


def lightfield_of(f):
    from hyperreel_amd.data import make_lightfield
    return make_lightfield(int(f['width']), int(f['height']), float(f['aspect']), float(f['st_scale']), float(f['uv_scale']), float(f['near']),
                           float(f['far']))


def view_rows(f, i):
    n = int(f['width']) * int(f['height'])
    return i * n, (i + 1) * n


def host_lib():
    deps = [SRC, os.path.join(HERE, '..', 'hyperreel_amd', 'csrc', 'hr_lightfield.h'), os.path.join(HERE, '..', 'include', 'hyperreel_hip.h')]
    build_host_lib(OUT, SRC, deps)
    lib = C.CDLL(OUT)
    lib.hl_linspace.argtypes = [C.c_float, C.c_float, C.c_int, C.c_void_p]
    lib.hl_linspace.restype = None
    for fn in (lib.hl_view_rays, lib.hl_epi_rays):
        fn.argtypes = [C.POINTER(hr_lightfield), C.c_float, C.c_float, C.c_int64, C.c_int64, C.c_void_p]
        fn.restype = None
    return lib


def host_rays(lib, f, first=0, n=None):
    """hr_lightfield.h compiled for the host over a whole fixture: (rays, 6) float32 in the fixture's order; for an EPI, rows
    [first, first + n)."""
    lf = lightfield_of(f)
    size = int(f['width']) * int(f['height'])
    if str(f['kind']) == 'epi':
        n = size - first if n is None else n
        out = np.empty((n, 6), np.float32)
        lib.hl_epi_rays(C.byref(lf), float(f['v']), float(f['t']), first, n, out.ctypes.data_as(C.c_void_p))
        return out
    out = np.empty((len(f['st']), size, 6), np.float32)
    for i, (s, t) in enumerate(f['st']):
        lib.hl_view_rays(C.byref(lf), float(s), float(t), 0, size, out[i].ctypes.data_as(C.c_void_p))
    return out.reshape(-1, 6)
