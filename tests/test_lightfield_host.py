"""Two-plane light-field rays without a GPU: hyperreel_amd/csrc/hr_lightfield.h compiled for the host against the reference's own
get_lightfield_rays / get_epi_rays (tests/golden/lightfield, written by tools/make_lightfield_golden.py), hr_lightfield against its
ctypes mirror, the bound entry points, the host helpers that restate where the reference takes (s, t) from, and the refusals that
happen before anything touches a device.

The bar for ray coordinates is lightfield_common.bars(): 4 x the reference's own float32-to-float64 distance per column group over
the committed fixtures, capped at 1e-5 (measured: origins 1.4e-8 -> bar 5.4e-8, directions 6.9e-7 -> bar 2.7e-6).  The bar holds the
directions; origins (columns 0-2) are asserted bit for bit.  Every test prints what it measured."""
import ctypes as C
import os

import numpy as np
import pytest

import lightfield_common as LC
from helpers import build_host_lib
from hyperreel_amd import data, lib
from hyperreel_amd.plan import hr_lightfield

HERE = os.path.dirname(os.path.abspath(__file__))
LAYOUT_SRC = os.path.join(HERE, 'c_abi', 'lightfield_layout.c')
LAYOUT_OUT = os.path.join(HERE, 'c_abi', '_build', 'libhr_lightfield_layout.so')


@pytest.fixture(scope='module')
def hl():
    return LC.host_lib()


def test_fixtures_are_the_documented_cases():
    assert LC.fixture_names() == sorted(LC.CASES)
    for name in LC.CASES:
        f = LC.load(name)
        n = int(f['width']) * int(f['height']) * (len(f['st']) if str(f['kind']) == 'view' else 1)
        assert f['rays'].dtype == np.float32 and f['rays'].shape == (n, 6) and f['coords64'].shape == (n, 6)
    f = LC.load('default_plane')
    assert (float(f['near']), float(f['far']), float(f['st_scale']), float(f['uv_scale'])) == (-1.0, 0.0, 1.0, 1.0)
    assert int(f['width']) % 2 == 1 and int(f['height']) % 2 == 1 and int(f['width']) != int(f['height'])
    f = LC.load('stanford_like')
    assert float(f['st_scale']) == 0.125 and float(f['uv_scale']) != 1.0 and (float(f['near']), float(f['far'])) != (-1.0, 0.0)
    f = LC.load('epi')
    assert int(f['width']) != int(f['height'])
    assert int(LC.load('one_wide')['width']) == 1 and int(LC.load('epi_one_row')['height']) == 1


def test_the_bars_come_from_the_reference():
    d, b = LC.reference_distances(), LC.bars()
    print(f'reference float32 vs float64: {d}; bars: {b}', flush=True)
    for k in ('origins', 'directions'):
        assert 0.0 < d[k] < 2.5e-6 and b[k] == min(4.0 * d[k], 1e-5)


@pytest.mark.parametrize('name', LC.CASES)
def test_host_header_against_the_reference(hl, name):
    f = LC.load(name)
    got = LC.host_rays(hl, f)
    LC.check_coords(got, f['rays'], f'{name} (host build of hr_lightfield.h)')
    assert np.isfinite(got).all()


def test_linspace_ends_and_symmetry(hl):
    """Both ends exact, the list antisymmetric about its middle (the middle element of an odd list is stepped from the end and need
    not be exactly 0), one element = the start."""
    for n in (1, 2, 3, 23, 37, 64, 1024):
        a = np.empty(n, np.float32)
        hl.hl_linspace(-1.0, 1.0, n, a.ctypes.data_as(C.c_void_p))
        b = np.empty(n, np.float32)
        hl.hl_linspace(1.0, -1.0, n, b.ctypes.data_as(C.c_void_p))
        assert a[0] == -1.0 and b[0] == 1.0
        if n > 1:
            h = n // 2
            assert a[-1] == 1.0 and np.array_equal(a[:h], -a[::-1][:h]) and np.array_equal(b, -a) and (np.diff(a) > 0).all()
            assert np.abs(a - np.linspace(-1.0, 1.0, n)).max() <= 2.0 ** -24


def test_a_pixel_range_is_the_same_rows_of_the_view(hl):
    f = LC.load('stanford_like')
    lf = LC.lightfield_of(f)
    s, t = (float(v) for v in f['st'][3])
    n = int(f['width']) * int(f['height'])
    lo, hi = LC.view_rows(f, 3)
    full = LC.host_rays(hl, f)[lo:hi]
    for first, cnt in ((0, n), (5, 100), (n - 7, 7), (n, 0)):
        part = np.full((cnt, 6), np.nan, np.float32)
        hl.hl_view_rays(C.byref(lf), s, t, first, cnt, part.ctypes.data_as(C.c_void_p))
        assert np.array_equal(part.view(np.uint32), full[first:first + cnt].view(np.uint32))
    e = LC.load('epi')
    whole = LC.host_rays(hl, e)
    assert np.array_equal(LC.host_rays(hl, e, 40, 300).view(np.uint32), whole[40:340].view(np.uint32))


def test_hr_lightfield_layout_matches_c():
    build_host_lib(LAYOUT_OUT, LAYOUT_SRC, [LAYOUT_SRC, os.path.join(HERE, '..', 'include', 'hyperreel_hip.h')])
    m = C.CDLL(LAYOUT_OUT)
    m.hf_lightfield_offset.argtypes = [C.c_int]
    names = ['width', 'height', 'aspect', 'st_scale', 'uv_scale', 'near', 'far']
    assert [n for n, _ in hr_lightfield._fields_] == names
    assert m.hf_lightfield_sizeof() == C.sizeof(hr_lightfield) == 28
    for i, n in enumerate(names):
        assert m.hf_lightfield_offset(i) == getattr(hr_lightfield, n).offset == 4 * i
    assert m.hf_abi_version() == 27
    assert LC.host_lib().hl_sizeof_lightfield() == 28


def test_entry_points_are_bound_at_abi_27():
    assert lib.ABI_VERSION == 27
    bound = {name: (res, args) for name, res, args in lib.SYMBOLS}
    gen = (C.c_int, [C.POINTER(hr_lightfield), C.c_float, C.c_float, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p])
    assert bound['hr_generate_rays_lightfield'] == gen and bound['hr_generate_rays_epi'] == gen
    assert bound['hr_rayset_create_lightfield'] == (C.c_int, [C.c_int32, C.POINTER(hr_lightfield), C.POINTER(C.c_void_p)])
    assert bound['hr_rayset_set_view'] == (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_void_p])
    L = lib.load()                                          # raises when the library does not export one of them
    assert L.hr_abi_version() == 27
    with open(os.path.join(HERE, '..', 'include', 'hyperreel_hip.h')) as fh:
        header = fh.read()
    for name in ('hr_generate_rays_lightfield', 'hr_generate_rays_epi', 'hr_rayset_create_lightfield', 'hr_rayset_set_view'):
        assert f'int {name}(' in header
    assert 'exit()' in header                               # the note on prepare_train_data's leftover exit()


def test_host_helpers_give_the_reference_positions():
    """(s, t) as the fixtures recorded them from LightfieldDataset.get_coord and StanfordLightfieldDataset.normalize_coord: equal as
    Python floats, not merely close."""
    f = LC.load('default_plane')
    rows, cols = int(f['rows']), int(f['cols'])
    for (s_idx, t_idx), want in zip(f['st_idx'], f['st']):
        assert tuple(float(v) for v in data.lightfield_coord(int(s_idx), int(t_idx), rows, cols)) == tuple(want)
    assert [tuple(i) for i in f['st_idx']] == [(s, t) for t in range(rows) for s in range(cols)]       # t outer, s inner
    assert data.lightfield_coord(0, 0, 1, 1) == (0, 0) and data.lightfield_coord(1.5, 0, 1, 4) == (0.0, 0)
    o = LC.load('one_wide')
    assert [tuple(float(v) for v in data.lightfield_coord(int(s), int(t), int(o['rows']), int(o['cols']))) for s, t in o['st_idx']] \
        == [tuple(w) for w in o['st']]
    g = LC.load('stanford_like')
    cams = [tuple(c) for c in g['camera_coords']]
    cols = int(g['cols'])
    for (s_idx, t_idx), want in zip(g['st_idx'], g['st']):
        got = data.stanford_normalize_coord(cams[int(t_idx) * cols + int(s_idx)], cams)
        assert tuple(float(v) for v in got) == tuple(want)
    assert np.abs(g['st'][:, 0]).max() == 1.0 and np.abs(g['st'][:, 1]).max() < 1.0       # x spans [-1, 1]; y is divided by the rig's aspect


def test_make_lightfield():
    lf = data.make_lightfield(37, 23)
    assert (lf.width, lf.height, lf.st_scale, lf.uv_scale, lf.near, lf.far) == (37, 23, 1.0, 1.0, -1.0, 0.0)
    assert lf.aspect == np.float32(37.0 / 23.0)
    lf = data.make_lightfield(8, 4, aspect=1.5, st_scale=0.125, uv_scale=0.5, near=-2.0, far=1.0)
    assert (lf.aspect, lf.st_scale, lf.uv_scale, lf.near, lf.far) == (1.5, 0.125, 0.5, -2.0, 1.0)
    assert 'fisheye' in data.UNSUPPORTED_RULES


def test_refusals_happen_on_the_host():
    """Every invalid argument is HR_E_INVALID with a message before anything is launched or allocated: these calls pass without a
    device.  The buffer handed over is host memory and is never written."""
    L = lib.load()
    buf = np.full((64, 6), np.nan, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    good = data.make_lightfield(8, 8)

    def refused(rc, word):
        msg = L.hr_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    def lf(**kw):
        args = dict(width=8, height=8, aspect=1.0, st_scale=1.0, uv_scale=1.0, near=-1.0, far=0.0)
        args.update(kw)
        return data.make_lightfield(**args)

    for fn, who in ((L.hr_generate_rays_lightfield, 'hr_generate_rays_lightfield'), (L.hr_generate_rays_epi, 'hr_generate_rays_epi')):
        refused(fn(None, 0.0, 0.0, 0, 4, p, None), 'null')
        for bad in (lf(width=0), lf(height=0), lf(width=-3), lf(aspect=0.0)):
            refused(fn(C.byref(bad), 0.0, 0.0, 0, 4, p, None), 'bad hr_lightfield')
        for bad in (lf(aspect=float('nan')), lf(st_scale=float('inf')), lf(uv_scale=float('nan')), lf(near=float('-inf')), lf(far=float('nan'))):
            refused(fn(C.byref(bad), 0.0, 0.0, 0, 4, p, None), 'non-finite')
        refused(fn(C.byref(good), float('nan'), 0.0, 0, 4, p, None), 'non-finite')
        refused(fn(C.byref(good), 0.0, float('inf'), 0, 4, p, None), 'non-finite')
        refused(fn(C.byref(good), 0.0, 0.0, -1, 4, p, None), 'outside')
        refused(fn(C.byref(good), 0.0, 0.0, 0, -4, p, None), 'outside')
        refused(fn(C.byref(good), 0.0, 0.0, 62, 4, p, None), 'outside')
        refused(fn(C.byref(good), 0.0, 0.0, 65, 0, p, None), 'outside')
        refused(fn(C.byref(good), 0.0, 0.0, 0, 4, None, None), 'null output')
        assert who in L.hr_last_error().decode()
        assert fn(C.byref(good), 0.0, 0.0, 64, 0, None, None) == 0            # an empty range at the end: nothing to launch
        assert fn(C.byref(good), 0.0, 0.0, 3, 0, p, None) == 0
    h = C.c_void_p()
    refused(L.hr_rayset_create_lightfield(0, C.byref(good), C.byref(h)), '0 views')
    refused(L.hr_rayset_create_lightfield(2, None, C.byref(h)), 'null')
    refused(L.hr_rayset_create_lightfield(2, C.byref(lf(aspect=0.0)), C.byref(h)), 'bad hr_lightfield')
    refused(L.hr_rayset_create_lightfield(2, C.byref(good), None), 'null')
    assert not h.value
    refused(L.hr_rayset_set_view(None, 0, 0.0, 0.0, 1, 0, p), 'null')
    assert np.isnan(buf).all()
    with pytest.raises(NotImplementedError, match='fisheye'):
        data.DeviceRaySet.from_lightfield([], [], good, subsample='fisheye')
    with pytest.raises(TypeError, match='make_lightfield'):
        data.DeviceRaySet.from_lightfield([], [], dict(width=8, height=8))
