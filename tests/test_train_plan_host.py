"""CPU check of the host-side decisions of hyperreel_amd/csrc/hr_plan.h, compiled for the host (tests/host_math/hr_plan_host.cpp): the
plane-pair geometry hr_model_finalize packs by, the plane class, and the launch plan of the training step -- which kernels
hr_launch_train takes for a case, with what LDS, in how many passes.  The expectations are worked out by hand from the rules (texel =
density | appearance channels in groups of four; 150 KiB of dynamic LDS), not taken from the code."""
import pytest

from helpers import GridPlane, plan_lib, plane_geometry, train_branch, train_plan
from hyperreel_amd import config as C
from hyperreel_amd import plan
from train_dispatch_common import BRANCH, DETERMINISTIC, TWO_PASS_N, _assert_branch, _levels, _scene

CAP = 150 * 1024
FIELDS = ('cd4', 'ca4', 'tex', 'aw', 'ah', 'bw', 'bh', 'ax', 'ay', 'bx', 'app_off', 'app_real', 'app_real_off')


def _config(model, grid, z=None, **kw):
    cfg = C.model_config(model) if z is None else C.model_config(model, z_channels=z)
    return plan.compile_config(cfg, C.dataset_scalars(model), grid, **kw)


def _with(hc, **fields):
    """A copy of a compiled config with the given array fields replaced."""
    out = type(hc).from_buffer_copy(hc)
    for k, v in fields.items():
        for i, e in enumerate(v):
            getattr(out, k)[i] = e
    return out


@pytest.mark.parametrize('case', list(BRANCH))
def test_every_row_lands_on_its_branch(case):
    _assert_branch(case)


@pytest.mark.parametrize('case', DETERMINISTIC)
def test_the_deterministic_build_takes_the_atomics_kernel(case):
    got = _assert_branch(case, deterministic=True)
    assert got['phase_b'] == 'atomics' and got['passes'] == 0


def _rows(*rows):
    return [dict(zip(FIELDS, r)) for r in rows]


K = 12      # keyframes of the shipped keyframe models (asserted below)
# grid (28, 24, 20): plane j spans axes (0, 1), (0, 2), (1, 2); its line / time plane runs along axis 2, 1, 0
GEOMETRY = {
    # static [8, 4, 4]: texels of 8 + 8, 4 + 4, 4 + 4 floats; lines of 20, 24, 28 texels; appearance slots 0, 8, 12
    'static_844': (lambda: _config('donerf_sphere', [28, 24, 20]), 16, 16, True, _rows(
        (2, 2, 16, 28, 24, 1, 20, 0, 1, 2, 0, 8, 0), (1, 1, 8, 28, 20, 1, 24, 0, 2, 1, 8, 4, 8), (1, 1, 8, 24, 20, 1, 28, 1, 2, 0, 12, 4, 12))),
    # keyframe [8, 0, 0]: pairs 1 and 2 unused (tex 0); time planes K rows of 20, 24, 28 texels
    'keyframe_800': (lambda: _config('technicolor_z_plane', [28, 24, 20]), 8, 8, True, _rows(
        (2, 2, 16, 28, 24, 20, K, 0, 1, 2, 0, 8, 0), (0, 0, 0, 28, 20, 24, K, 0, 2, 1, 8, 0, 8), (0, 0, 0, 24, 20, 28, K, 1, 2, 0, 8, 0, 8))),
    # float16 texels come in whole octets: 8 density + 4 appearance = 12 halfs -> 16; 4 + 4 = 8 stays
    'fp16_rounded': (lambda: _with(_config('donerf_sphere', [28, 24, 20], grid_dtype='fp16'), n_den=[8, 4, 4], n_app=[4, 4, 4]), 12, 12, True, _rows(
        (2, 1, 16, 28, 24, 1, 20, 0, 1, 2, 0, 4, 0), (1, 1, 8, 28, 20, 1, 24, 0, 2, 1, 4, 4, 4), (1, 1, 8, 24, 20, 1, 28, 1, 2, 0, 8, 4, 8))),
    # a keyframe net skips a pair without density components for appearance too: pair 1 keeps no channels, basis_mat still has its 4
    # columns, and the geometry says that the two do not add up
    'keyframe_app_without_density': (lambda: _with(_config('technicolor_z_plane', [28, 24, 20]), n_app=[8, 4, 0]), 8, 12, False, _rows(
        (2, 2, 16, 28, 24, 20, K, 0, 1, 2, 0, 8, 0), (0, 0, 0, 28, 20, 24, K, 0, 2, 1, 8, 0, 8), (0, 0, 0, 24, 20, 28, K, 1, 2, 0, 8, 0, 8))),
}


@pytest.mark.parametrize('name', list(GEOMETRY))
def test_plane_geometry_equals_the_hand_derived_descriptors(name):
    make, ca_total, n_basis_cols, consistent, want = GEOMETRY[name]
    hc = make()
    if hc.video:
        assert hc.num_keyframes == K
    planes, ca, nb, ok = plane_geometry(hc)
    assert (ca, nb, ok) == (ca_total, n_basis_cols, consistent)
    for j in range(3):
        assert {k: getattr(planes[j], k) for k in FIELDS} == want[j], (name, j)
        assert planes[j].a is None and planes[j].b is None


def test_round_zp():
    lib = plan_lib()
    assert [lib.hp_round_zp(z) for z in (1, 8, 9, 64, 65, 200, 256)] == [8, 8, 16, 64, 128, 256, 256]


def test_the_cap_edge_of_a_static_net():
    """donerf_sphere (32 samples: 8 rays per trip), grid [12, 12, N]: decode matrices and their gradient 2 x 8 x 3 x 16, basis_mat's
    gradient 27 x 16, time taps 8 x 4 floats = 4928 B; lines 1 and 2: 12 texels x 8 floats each = 768 B; line 0: 64 B per texel.
    4928 + 768 + 64 N <= 153 600 holds up to N = 2311, with equality there."""
    hc = _config('donerf_sphere', [12, 12, 2400])
    at = lambda n: train_branch(_with(hc, grid=[12, 12, n]), 96)
    last = max(n for n in range(2200, 2401) if at(n)['phase_b'] == 'lines')
    assert last == 2311
    assert at(last)['lds_bytes'] == 4928 + 768 + 64 * last <= CAP < at(last + 1)['lds_bytes']
    assert (at(last)['passes'], at(last)['keyed']) == (1, False)
    assert at(last + 1)['phase_b'] == 'atomics' and at(last + 1)['passes'] == 0
    assert all(at(n)['phase_b'] == 'lines' for n in range(2200, last))
    assert at(2400)['phase_b'] == 'atomics'                                  # the lds_fallback row of the branch table
    assert _assert_branch('lds_fallback')['lds_bytes'] == at(2400)['lds_bytes'] == 4928 + 768 + 64 * 2400


@pytest.mark.parametrize('g0,g1', [(24, 20), (64, 64)])
def test_a_keyframe_net_splits_into_two_passes(g0, g1):
    """neural_3d_z_plane at 16 samples (16 rays per trip: 8128 B besides the windows), keyframe [8, 4, 4]: the window of a pair is two rows
    of its time plane -- 2 x N texels x 16 floats = 128 N B for pair 0 along the long axis, 64 B per texel of the other two axes for pairs 1
    and 2.  One pass while everything fits, two (pair 0, then pairs 1 + 2 adding to the first pass's point gradient) while pair 0 alone
    does, global atomics beyond."""
    hc = _config('neural_3d_z_plane', [g0, g1, 1000], z=16)
    assert list(hc.n_den[:3]) == [8, 4, 4] and hc.video and hc.num_keyframes == K
    base, small = 8128, 64 * (g0 + g1)
    at = lambda n: train_plan(_with(hc, grid=[g0, g1, n]), 48)
    one = (CAP - base - small) // 128              # the longest axis all three pairs fit with
    two = (CAP - base) // 128                      # ... pair 0 alone
    assert one < two
    for n in (one + 1, two):
        p = at(n)
        assert base + small + 128 * n > CAP
        assert (p.lines, p.keyed, p.passes, p.b_pc) == (1, 1, 2, 1), n
        assert list(p.pass_pairs) == [1, 6] and list(p.pass_add_dp) == [0, 1]
        assert list(p.pass_lds) == [base + 128 * n, base + small] and max(p.pass_lds) == p.lines_lds <= CAP
    p = at(one)
    assert (p.lines, p.passes, list(p.pass_pairs), list(p.pass_add_dp), p.lines_lds) == (1, 1, [7, 0], [0, 0], base + small + 128 * one)
    p = at(two + 1)
    assert (p.lines, p.passes, list(p.pass_pairs)) == (0, 0, [0, 0]) and p.lines_lds == base + 128 * (two + 1) > CAP
    if (g0, g1) == (24, 20):
        assert TWO_PASS_N == one + 1                                       # the branch table's row is the smallest such grid
        got = train_plan(_levels(_scene('two_pass'))[1], 48)
        assert (got.passes, list(got.pass_pairs), list(got.pass_lds)) == (2, [1, 6], list(at(TWO_PASS_N).pass_lds))


def test_the_train_class_is_generic_from_2_to_the_30_elements():
    """hr_bwd_slot addresses texel elements by 32-bit offsets: a plane of 2^30 elements or more takes the generic path.  Descriptors only."""
    lib = plan_lib()

    def planes(aw0):
        pl = (GridPlane * 3)()
        for j, (cd4, off) in enumerate([(2, 0), (1, 8), (1, 12)]):
            g = pl[j]
            g.cd4 = g.ca4 = cd4
            g.tex, g.app_off = 8 * cd4, off
            g.aw, g.ah, g.bw, g.bh = 64, 64, 1, 64
        pl[0].aw, pl[0].ah = aw0, 8192
        return pl
    assert 8192 * 8192 * 16 == 1 << 30
    assert lib.hp_plane_class(planes(8192), 16, 1) == 0 and lib.hp_plane_class(planes(8191), 16, 1) == 1
    assert lib.hp_plane_class(planes(8192), 16, 0) == 1                     # the render gathers' predicate does not look at the size
    big_line = planes(64)
    big_line[2].bh = 1 << 27                                                # 2^27 texels x 8 floats
    assert lib.hp_plane_class(big_line, 16, 1) == 0 and lib.hp_plane_class(big_line, 16, 0) == 1
    assert lib.hp_plane_class(planes(64), 16, 1) == 1 and lib.hp_plane_class(planes(64), 12, 1) == 0


# HrTrainTape's fields in workspace order with their planes of ns = n_rays x Z words: 1 + 1 + 1 + 3 + 1 + 1 + 18 + 3 + 1 = 30 words per sample
TAPE = (('ds', 1), ('src', 1), ('dfeat', 1), ('dpre', 3), ('ddc', 1), ('dts', 1), ('taps', 18), ('dp', 3), ('perm', 1))


def _tape_layout(ns, rows=False):
    import ctypes
    lib = plan_lib()
    lib.hp_tape_layout.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p]
    off = (ctypes.c_longlong * 9)()
    words = lib.hp_tape_layout(1 << 20, ns, int(rows), off)       # an address only: nothing is read or written
    return words, list(off)


@pytest.mark.parametrize('n_rays,z', [(1, 1), (3, 8), (95, 16), (48, 200)])
def test_the_tape_layout_equals_the_hand_derived_planes(n_rays, z):
    """hr_tape_bind cuts the workspace hr_train_backward allocates (HR_TAPE_WORDS floats per sample) into the planes above, 4-byte words."""
    ns = n_rays * z
    words, off = _tape_layout(ns)
    assert words == 30 == sum(p for _, p in TAPE)
    first = dict(ds=0, src=1, dfeat=2, dpre=3, ddc=6, dts=7, taps=8, dp=26, perm=29)      # first plane of each field, counted by hand
    spans = []
    for (name, planes), o in zip(TAPE, off):
        assert o == first[name] * ns * 4, name
        spans.append((o, o + planes * ns * 4, name))
    for i, (lo, hi, a) in enumerate(spans):
        assert 0 <= lo < hi <= 30 * ns * 4, a
        for lo2, hi2, b in spans[i + 1:]:
            assert hi <= lo2 or hi2 <= lo, (a, b)                     # pairwise disjoint
    assert max(hi for _, hi, _ in spans) == 30 * ns * 4                # the last byte of the allocation
    perm_lo, perm_hi, _ = spans[-1]
    assert perm_hi - perm_lo >= 4 * n_rays                             # the grouped ray order: n_rays ints
    # the coarse level of a cascade: ds, src, dts in the first three planes, nothing else bound
    words, off = _tape_layout(ns, rows=True)
    assert words == 30 and off == [0, 4 * ns, -1, -1, -1, 8 * ns, -1, -1, -1]


def _grad_pool(hc, elem, align):
    import ctypes
    lib = plan_lib()
    lib.hp_grad_pool.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    out = (ctypes.c_size_t * 13)()
    lib.hp_grad_pool(ctypes.byref(hc), elem, align, out)
    v = list(out)
    return dict(off_a=v[0:3], off_b=v[3:6], n_a=v[6:9], n_b=v[9:12], total=v[12])


def test_the_gradient_pool_of_a_static_844_net():
    """[8, 4, 4] on 28 x 24 x 20 (GEOMETRY['static_844']): planes of 28 x 24 x 16, 28 x 20 x 8 and 24 x 20 x 8 floats, lines of 20 x 16, 24 x 8 and
    28 x 8.  Float pool, 256-byte (64-float) starts: every size but the last line's 224 floats is a multiple of 64; that one is rounded to 256.
    Fixed-point pool: the same elements packed."""
    hc = _config('donerf_sphere', [28, 24, 20])
    n_a, n_b = [10752, 4480, 3840], [320, 192, 224]
    assert [28 * 24 * 16, 28 * 20 * 8, 24 * 20 * 8] == n_a and [20 * 16, 24 * 8, 28 * 8] == n_b
    assert all(n % 64 == 0 for n in n_a + n_b[:2]) and n_b[2] % 64 == 32
    packed = dict(off_a=[0, 11072, 15744], off_b=[10752, 15552, 19584], n_a=n_a, n_b=n_b, total=19808)
    assert _grad_pool(hc, 8, 8) == packed
    assert _grad_pool(hc, 4, 256) == dict(packed, total=19808 + 32)          # 79 360 bytes = 310 x 256
    assert (19808 + 32) * 4 == 310 * 256


def test_the_gradient_pool_of_a_net_with_empty_pairs():
    """Keyframe [8, 0, 0] on 27 x 23 x 19: pair 0 alone, plane 27 x 23 x 16 = 9936 floats (155.25 x 64 -> 9984 in the float pool), time plane
    12 rows x 19 x 16 = 3648 = 57 x 64; pairs 1 and 2 take nothing and keep offset 0."""
    hc = _config('technicolor_z_plane', [27, 23, 19])
    assert hc.num_keyframes == K and (27 * 23 * 16, K * 19 * 16) == (9936, 3648)
    want = dict(off_a=[0, 0, 0], off_b=[9936, 0, 0], n_a=[9936, 0, 0], n_b=[3648, 0, 0], total=13584)
    assert _grad_pool(hc, 8, 8) == want
    assert _grad_pool(hc, 4, 256) == dict(want, off_b=[9984, 0, 0], total=9984 + 3648)
