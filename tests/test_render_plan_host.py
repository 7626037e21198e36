"""CPU check of the render call's decisions in hyperreel_amd/csrc/hr_plan.h, compiled for the host (tests/host_math/hr_plan_host.cpp):
launch sizing, the sample kernel's LDS and instantiation, the create-time LDS bound, the sample stage's kinds and forms, the call's route,
live head columns, a frame's time tap, the frame kernel's plan.  The expectations are worked out by hand in the docstrings, not taken from the code."""
import ctypes

import numpy as np
import pytest

from helpers import (SAMPLE_KIND, Golden, SamplePlan, even_chunk, frame_plan, frame_time_tap, live_columns, math_lib, plan_lib, plane_geometry,
                     redo_list_cap, render_route, sample_form_plan, sample_lds_refused, sample_plan, sweep_cases)
from hyperreel_amd import config as C
from hyperreel_amd import plan

KIB = 1024
HEAD_FIELDS = ('f_z_vals', 'f_isect_sigma', 'f_offset_sigma', 'f_point_offset', 'f_color_scale', 'f_color_shift', 'f_spatial_flow',
               'f_color_scale_global', 'f_color_shift_global')


def _config(model, grid=(28, 24, 20), z=None, **kw):
    cfg = C.model_config(model) if z is None else C.model_config(model, z_channels=z)
    return plan.compile_config(cfg, C.dataset_scalars(model), list(grid), **kw)


def _copy(hc):
    return type(hc).from_buffer_copy(hc)


def _levels(case):
    """The levels of a sweep fixture's model as (name, hr_config, is the coarse level of a cascade)."""
    g = Golden(case)
    coarse, hc = plan.compile_model(g.cfg, g.dataset, g.grid, iteration=g.iteration)
    return ([('coarse', coarse, True)] if coarse is not None else []) + [('fine', hc, False)]


# ---------------------------------------------------------------- launch sizing
def test_even_chunk_splits_a_call_into_equal_launches():
    """Neural-3D's 1352 x 1014 = 1 370 928 rays on a 65 536-ray workspace: ceil(1 370 928 / 65 536) = 21 launches; 1 370 928 / 21 =
    65 282.3 -> 65 283 -> the next multiple of 64 is 65 344 (1021 x 64).  20 x 65 344 = 1 306 880, so the last launch holds 64 048 rays
    = 1000.75 x 64: not a multiple of 64.  A call that fits the workspace is one launch of the workspace's size; one ray more is two
    launches of ceil(65 537 / 2) = 32 769 -> 32 832 rays (the second holds 32 705)."""
    per = even_chunk(65536, 1370928)
    assert per == 65344 and -(-1370928 // per) == 21
    last = 1370928 - 20 * per
    assert last == 64048 and last % 64 != 0
    assert even_chunk(65536, 65536) == 65536 and even_chunk(65536, 1000) == 65536 and even_chunk(65536, 0) == 65536
    assert even_chunk(65536, 65537) == 32832 and 65537 - 32832 == 32705
    assert even_chunk(131072, 2228224) == 131072                   # 17 launches of the workspace's size exactly


@pytest.mark.parametrize('n,want', [(2228224, 139264), (1370928, 85696), (5483712, 342784), (1000, 1024), (0, 0), (1 << 27, 4194304)])
def test_redo_list_cap(n, want):
    """max(32 768, n / 16) rounded up to 64, never more than the rays rounded up to 64, never more than the 1 << 22 buffer:
    2 228 224 / 16 = 139 264 (a multiple of 64); 1 370 928 / 16 = 85 683 -> 85 696; 5 483 712 / 16 = 342 732 -> 342 784;
    1 000 rays: 32 768 > 1 000 -> 1 024; no rays: 0; 2^27 / 16 = 2^23 -> the buffer's 4 194 304."""
    assert redo_list_cap(n) == want


def test_default_chunk_and_wide_cap():
    """2^28 bytes of head per launch, 16 bytes per quad: DoNeRF (88 quads) 190 650 rays -> down to a multiple of 16 384: 180 224 -> the
    cap, 163 840; technicolor / immersive (120 quads) 139 810 -> 131 072; Neural-3D (240 quads) 69 905 -> 65 536; a cascade's 8 rows per
    ray of 24 quads: 87 381 -> 81 920; a 4096-quad head: 4 096 rays, the floor (below 16 384 nothing is rounded: 5 000 quads give 3 355 ->
    4 096).  The third pass's list: 8 192 entries, or the chunk when that is smaller."""
    lib = plan_lib()
    assert [lib.hp_default_chunk(nq, rows) for nq, rows in ((88, 1), (120, 1), (240, 1), (24, 8), (4096, 1), (5000, 1))] == \
        [163840, 131072, 65536, 81920, 4096, 4096]
    assert [lib.hp_wide_cap(c) for c in (64, 8192, 163840)] == [64, 8192, 8192]


# ---------------------------------------------------------------- the sample kernel's LDS
def test_sample_lds_bytes():
    """256 / ZP rays x rows x (4 nq + 4) floats, 256 / ZP x 3 x ca floats of decode matrices, 256 floats above 64 samples only:
    (nq 24, ca 16, ZP 32): 8 rays: 8 x 100 + 8 x 48 = 1 184 floats = 4 736 bytes.
    (nq 96, ca 16, ZP 128): 2 rays: 2 x 388 + 2 x 48 + 256 = 1 128 floats = 4 512 bytes.
    ZP 8, ca 16: 32 rays: 32 x (4 nq + 4) + 1 536 floats = 512 nq + 6 656 bytes: nq 115 -> 65 536 exactly, nq 116 -> 66 048."""
    lib = plan_lib()
    assert lib.hp_sample_lds_bytes(24, 16, 32, 1) == 4736
    assert lib.hp_sample_lds_bytes(96, 16, 128, 1) == 4512
    assert lib.hp_sample_lds_bytes(115, 16, 8, 1) == 65536 and lib.hp_sample_lds_bytes(116, 16, 8, 1) == 66048


def test_big_lds_starts_above_64_kib():
    """The opt-in for more than the default 64 KiB: 65 536 bytes (ZP 8, ca 16, nq 115) is not big, 66 048 (nq 116) is."""
    hc = _config('donerf_sphere', z=8)
    planes, ca, _, ok = plane_geometry(hc)
    assert ok and ca == 16
    got = {}
    for nq in (115, 116):
        out = SamplePlan()
        plan_lib().hp_sample_plan_raw(ctypes.byref(hc), planes, ca, nq, 1, ctypes.c_longlong(1000), 0, ctypes.byref(out))
        got[nq] = (out.zp, out.lds, out.big_lds, out.blocks)
    assert got == {115: (8, 65536, 0, 32), 116: (8, 66048, 1, 32)}            # 1000 rays in workgroups of 32: 32 workgroups


def _donerf_with_app(z, n_app):
    hc = _config('donerf_sphere', z=z)
    for j in range(3):
        hc.n_app[j] = n_app[j]
    return hc


@pytest.mark.parametrize('z,inside,outside', [(8, (128, 128, 124), (128, 128, 128)), (128, (2048, 2048, 2044), (2048, 2048, 2048))])
def test_create_time_lds_bound(z, inside, outside):
    """hr_model_create refuses what the bound it has always applied refuses: with rpb = 256 / ZP rays per workgroup,
        4 x (rpb x rows x (4 nq + 4) + rpb x 3 x ca + 256) > 160 KiB - 4 096 = 159 744 bytes.
    DoNeRF's head (11 live columns of 15) with hand-made appearance components (a static net: every pair is sampled, ca = their sum in
    fours):
      * 8 samples: ZP 8, rpb 32, nq = 22: 4 x (32 x 92 + 96 ca + 256) = 12 800 + 384 ca.  ca = 380 (128 + 128 + 124): 158 720, inside;
        ca = 384: 160 256, outside.  (The kernel itself asks for 1 024 bytes less at 64 samples or fewer -- 157 696 / 159 232 -- and the
        latter plus the 4 096 static bytes alone would pass: the bound's extra 1 KiB decides this pair.)
      * 128 samples: ZP 128, rpb 2, nq = 352: 4 x (2 x 1 412 + 6 ca + 256) = 12 320 + 24 ca.  ca = 6 140: 159 680, inside; ca = 6 144:
        159 776, outside.  (Above 64 samples the kernel's request is the bound's figure.)"""
    zp = 8 if z == 8 else 128
    rpb, nq = 256 // zp, (z * 11 + 3) // 4
    for n_app, refused in ((inside, False), (outside, True)):
        hc = _donerf_with_app(z, n_app)
        assert live_columns(hc)[1] == 11
        ca = sum(4 * ((a + 3) // 4) for a in n_app)
        bound = 4 * (rpb * (4 * nq + 4) + rpb * 3 * ca + 256)
        assert (bound > 160 * KIB - 4096) == refused
        got, request = sample_lds_refused(hc)
        assert got == refused
        assert request == bound - (0 if zp > 64 else 1024)


@pytest.mark.parametrize('n_app,request_bytes,refused', [((100, 100, 96), 157408, False), ((100, 100, 100), 159376, True)])
def test_create_time_lds_bound_of_an_mlp_shaded_model(n_app, request_bytes, refused):
    """The same bound, evaluated on the SHADE kind's largest form: the export form keeps all 27 rows of basis_mat (27 x ca floats) behind
    the plan's LDS.  DoNeRF's head at 8 samples (11 live columns, nq = 22, 32 rays per workgroup, no cross-wave scratch), shading set by
    hand to MLP_Fea: 4 x (32 x 92 + 96 ca) + 108 ca = 11 776 + 384 ca + 108 ca bytes, refused when that + 4 096 + 1 024 > 163 840, i.e.
    ca > 298.67.  ca = 296 (100 + 100 + 96): 11 776 + 492 x 296 = 157 408, + 5 120 = 162 528: accepted.  ca = 300: 11 776 + 147 600 =
    159 376, + 5 120 = 164 496: refused.  (The same components under RGB shading ask for 108 ca less and are both accepted.)"""
    hc = _donerf_with_app(8, n_app)
    ca = sum(n_app)
    assert live_columns(hc)[1] == 11 and all(a % 4 == 0 for a in n_app)
    assert sample_lds_refused(hc) == (False, 11776 + 384 * ca)
    hc.shading = plan.SHADING['MLP_Fea']
    assert 11776 + 384 * ca + 108 * ca == request_bytes and (request_bytes + 4096 + 1024 > 160 * KIB) == refused
    assert sample_lds_refused(hc) == (refused, request_bytes)
    # the request is the export form's plan
    assert sample_form_plan(hc, 'shade', exported=True)[0].lds == request_bytes


# ---------------------------------------------------------------- hr_sample_plan
def _want_class(hc, rows_emitted):
    """[8, 4, 4] on all three pairs -> 1, [8, 0, 0] -> 2, anything else -> 0 (float16 texels alike); never for a kernel that emits
    rows, never for a keyframe net with fewer than two keyframes.  (Every fixture's grid has at least two texels per axis.)"""
    if rows_emitted or (hc.video and hc.num_keyframes < 2):
        return 0
    return {((8, 4, 4), (8, 4, 4)): 1, ((8, 0, 0), (8, 0, 0)): 2}.get((tuple(hc.n_den), tuple(hc.n_app)), 0)


def _check_sample_plan(hc, rows_emitted=False):
    want = _want_class(hc, rows_emitted)
    for frame_lines in (False, True):
        p, inst = sample_plan(hc, rows_emitted=rows_emitted, frame_lines=frame_lines)
        # line taps: a static net's second factors are lines; a float32 keyframe net's are inside hr_render_frame
        lines = want != 0 and (not hc.video or (frame_lines and hc.num_keyframes >= 2 and hc.grid_dtype == 0))
        assert (p.pclass, p.all_lines) == (want, int(lines)), (frame_lines, p.pclass, p.all_lines)
        zp = max(8, 1 << (hc.z_channels - 1).bit_length())
        assert inst == (zp, int(hc.grid_dtype == 1), want, 2 if lines else 4)
        assert inst[2:] != (0, 2)                 # the generic gather has no line form


@pytest.mark.parametrize('case', sweep_cases())
def test_sample_plan_of_every_sweep_fixture(case):
    for _, hc, coarse in _levels(case):
        _check_sample_plan(hc, rows_emitted=coarse)


@pytest.mark.parametrize('model', C.MODEL_NAMES)
@pytest.mark.parametrize('grid_dtype', ['fp32', 'fp16'])
def test_sample_plan_of_every_benchmark_model(model, grid_dtype):
    """DoNeRF: [8, 4, 4] static -> class 1, lines.  technicolor: [8, 0, 0] keyframe -> class 2; Neural-3D and immersive: [8, 4, 4]
    keyframe -> class 1; time planes, so four taps, except inside hr_render_frame with float32 texels."""
    hc = _config(model, grid_dtype=grid_dtype)
    assert _want_class(hc, False) == {'donerf_sphere': 1, 'donerf_cylinder': 1, 'technicolor_z_plane': 2, 'neural_3d_z_plane': 1, 'immersive_sphere': 1}[model]
    _check_sample_plan(hc)


def test_sample_plan_special_cases():
    """A generic decomposition ([8, 8, 8], and [8, 4, 4] density with [4, 4, 4] appearance) is class 0; a keyframe net with ONE keyframe
    is class 0 (the class gathers clamp their taps to rows i, i + 1); a cascade's coarse level emits rows: class 0 whatever its planes."""
    for n_den, n_app in (((8, 8, 8), (8, 8, 8)), ((8, 4, 4), (4, 4, 4))):
        hc = _config('donerf_sphere')
        for j in range(3):
            hc.n_den[j], hc.n_app[j] = n_den[j], n_app[j]
        p, inst = sample_plan(hc)
        assert (p.pclass, p.all_lines, inst) == (0, 0, (32, 0, 0, 4))
    hc = _config('technicolor_z_plane')
    assert sample_plan(hc)[1] == (32, 0, 2, 4)
    hc.num_keyframes = 1
    p, inst = sample_plan(hc)
    assert (p.pclass, inst) == (0, (32, 0, 0, 4))
    assert sample_plan(hc, frame_lines=True)[1] == (32, 0, 0, 4)
    coarse = [hc0 for _, hc0, is_coarse in _levels('sweep/shiny_z_plane_cascaded') if is_coarse][0]
    assert tuple(coarse.n_den) == (8, 4, 4) and sample_plan(coarse)[1] == (8, 0, 1, 2)         # its planes alone would be class 1
    assert sample_plan(coarse, rows_emitted=True)[1] == (8, 0, 0, 4)


# ---------------------------------------------------------------- hr_sample_kind, hr_sample_form_plan
def test_sample_kind():
    """A density mode (whatever the shading) -> TIME_DENSITY; else RGBtLinear, RGBtFourier and RGBIdentity -> TIME, MLP_Fea and MLP ->
    SHADE, RGB and SH -> DECODE."""
    want = {'RGB': 'decode', 'SH': 'decode', 'MLP_Fea': 'shade', 'MLP': 'shade', 'RGBtLinear': 'time', 'RGBtFourier': 'time', 'RGBIdentity': 'time'}
    assert set(want) == set(plan.SHADING)
    for name, kind in want.items():
        assert plan_lib().hp_sample_kind(plan.SHADING[name], 0) == SAMPLE_KIND[kind], name
        assert plan_lib().hp_sample_kind(plan.SHADING[name], 1) == SAMPLE_KIND['time_density'], name


def test_form_plan_of_an_mlp_shaded_model():
    """DoNeRF ([8, 4, 4] static: its planes alone are class 1 with line taps) with the shading set to MLP_Fea.  The DECODE plan: 32 samples,
    8 rays per workgroup, nq = 32 x 11 / 4 = 88: 8 x (352 + 4) + 8 x 3 x 16 = 3 232 floats = 12 928 bytes.  Both SHADE forms take the
    generic gather, (32, float32, 0, 4); the import form asks for the same LDS, the export form for 27 x 16 x 4 = 1 728 bytes more, its
    block starting where the DECODE plan ends, at float 3 232."""
    hc = _config('donerf_sphere')
    hc.shading = plan.SHADING['MLP_Fea']
    for frame_lines in (False, True):
        dec, inst = sample_form_plan(hc, 'decode', n_rays=130, frame_lines=frame_lines)
        assert (dec.pclass, dec.all_lines, inst) == (1, 1, (32, 0, 1, 2))
        assert (dec.lds, dec.big_lds, dec.blocks, dec.x_off, dec.d_slots) == (12928, 0, 17, 0, 0)
        for exported in (False, True):
            p, inst = sample_form_plan(hc, 'shade', n_rays=130, maps=not exported, exported=exported, frame_lines=frame_lines)
            assert (p.zp, p.pclass, p.all_lines, inst) == (32, 0, 0, (32, 0, 0, 4))
            assert (p.lds, p.x_off) == ((12928 + 1728, 3232) if exported else (12928, 0))
            assert (p.big_lds, p.blocks, p.d_slots) == (0, 17, 0)
    # the DECODE forms are hr_sample_plan, with the maps or without
    for maps in (False, True):
        dec, inst = sample_form_plan(hc, 'decode', maps=maps)
        ref, ref_inst = sample_plan(hc)
        assert all(getattr(dec, k) == getattr(ref, k) for k, _ in SamplePlan._fields_) and inst == ref_inst


def test_form_plan_of_a_time_colour_model():
    """technicolor ([8, 0, 0] keyframe net) with RGBtFourier: the TIME form keeps class 2 and never takes the line form -- not inside
    hr_render_frame either, where the DECODE plan of the same planes does; (32, float32, 2, 4).  No block of its own: the LDS is the
    DECODE plan's (a decode matrix per ray was always counted)."""
    cfg = C.model_config('technicolor_z_plane', shading='RGBtFourier')
    hc = plan.compile_model(cfg, C.dataset_scalars('technicolor_z_plane'), [28, 24, 20])[1]
    assert hc.shading == plan.SHADING['RGBtFourier']
    for frame_lines in (False, True):
        dec, dec_inst = sample_form_plan(hc, 'decode', frame_lines=frame_lines)
        assert (dec.pclass, dec.all_lines, dec_inst) == (2, int(frame_lines), (32, 0, 2, 2 if frame_lines else 4))
        p, inst = sample_form_plan(hc, 'time', maps=True, frame_lines=frame_lines)
        assert (p.pclass, p.all_lines, inst) == (2, 0, (32, 0, 2, 4))
        assert (p.lds, p.big_lds, p.blocks, p.x_off, p.d_slots) == (dec.lds, dec.big_lds, dec.blocks, 0, 0)
        # with a density mode: class 2 keeps the row in the decode matrix's shape, 3 x 8 floats per ray behind the plan's LDS
        d, inst = sample_form_plan(hc, 'time_density', maps=True, frame_lines=frame_lines)
        assert (d.pclass, d.all_lines, inst) == (2, 0, (32, 0, 2, 4))
        assert (d.d_slots, d.x_off, d.lds) == (24, dec.lds // 4, dec.lds + 4 * 8 * 24)


# ---------------------------------------------------------------- hr_render_route
def test_render_route_table():
    """Which plan a call takes, from the facts alone.
      * the frame kernel: the image alone (no diagnostics, no maps) of a DECODE model where hr_frame_plan fits -- DoNeRF under
        HR_OPT_FRAME_KERNEL = 1; a call without rays takes the route too (and launches nothing).
      * the verified fast path: a verified model's image, with or without maps; not with diagnostics, not with an occupancy volume, not
        for 2^31 rays or more, not for no rays: those render launch by launch with the f16x3 tiles (tier 1).
      * a stale band: measured first (calibrate_first) unless the stream is being captured -- then tier 1 launches, nothing measured.
        After the measurement the caller asks again with what it left: still verified -> the fast path; given up -> tier 0.
      * an unverified model: launch by launch in its own arithmetic (tier 0), stale band or not.
      * SHADE, TIME, TIME_DENSITY: never the frame kernel, never the fast path, never a measurement -- whatever the other facts say."""
    hc = _config('donerf_sphere')
    fits = bool(frame_plan(hc, frame_mode=1).fits)
    assert fits and not frame_plan(hc, frame_mode=1, verified=True).fits
    R = render_route
    assert R(frame_fits=fits) == ('frame', 0, 0) and R(frame_fits=fits, n_rays=0) == ('frame', 0, 0)
    assert R(frame_fits=fits, maps=True) == ('chunked', 0, 0) and R(frame_fits=fits, fields=True) == ('chunked', 0, 0)
    assert R(frame_fits=False) == ('chunked', 0, 0)
    for kind in ('shade', 'time', 'time_density'):
        assert R(frame_fits=True, kind=kind) == ('chunked', 0, 0)
    V = dict(mlp_verified=True)
    assert R(**V) == ('verified', 0, 0) and R(**V, maps=True) == ('verified', 0, 0)
    assert R(**V, n_rays=1) == ('verified', 0, 0) and R(**V, n_rays=(1 << 31) - 1) == ('verified', 0, 0)
    assert R(**V, fields=True) == ('chunked', 1, 0) and R(**V, fields=True, maps=True) == ('chunked', 1, 0)
    assert R(**V, occupancy=True) == ('chunked', 1, 0)
    assert R(**V, n_rays=1 << 31) == ('chunked', 1, 0)
    assert R(**V, n_rays=0) == ('chunked', 1, 0)
    # a stale band
    assert R(**V, band_stale=True)[2] == 1 and R(**V, band_stale=True, maps=True)[2] == 1 and R(**V, band_stale=True, n_rays=0)[2] == 1
    assert R(**V, band_stale=True)[:2] == ('chunked', 1)               # (what the call would take without the measurement)
    assert R(mlp_verified=True, band_stale=False) == ('verified', 0, 0)
    assert R(mlp_verified=False, band_stale=False) == ('chunked', 0, 0)
    assert R(**V, band_stale=True, capturing=True) == ('chunked', 1, 0)
    for ineligible in (dict(fields=True), dict(occupancy=True), dict(n_rays=1 << 31)):          # nothing to measure for
        assert R(**V, band_stale=True, **ineligible) == ('chunked', 1, 0)
    assert R() == ('chunked', 0, 0) and R(band_stale=True) == ('chunked', 0, 0) and R(occupancy=True, maps=True) == ('chunked', 0, 0)
    for kind in ('shade', 'time', 'time_density'):
        for bits in range(64):
            fields, maps, occ, stale, cap, ff = ((bits >> i) & 1 for i in range(6))
            for n in (0, 130, 1 << 31):
                assert R(n_rays=n, fields=fields, maps=maps, kind=kind, mlp_verified=True, occupancy=occ, band_stale=stale, capturing=cap,
                         frame_fits=ff) == ('chunked', 1, 0)


# ---------------------------------------------------------------- hr_live_columns
def _read_channels(hc):
    """{field: channels the sample stage reads}, from the stage's own rules: sphere / cylinder read the radius (3) and, with a non-zero
    origin_scale, the origin (0-2); the deformable voxel grid alike with its normal scale; sphere_new / cylinder_new read the raw offset and
    radius (6, 7), the resize (3-5) with a non-zero resize OR origin scale (kept so that the field stays contiguous up to channel 7), the
    origin with a non-zero origin scale; the others read channel 0.  sigma: 1 channel.  point offset (3) and its sigma (1) with the stage
    on; colour scale / shift 3 each, a 9-channel global scale is a 3x3 matrix; spatial flow (3) with advection and the flow on."""
    t, z = hc.isect_type, set()
    if t in (plan.ISECT['sphere'], plan.ISECT['cylinder'], plan.ISECT['deformable_voxel_grid']):
        z = {3} | ({0, 1, 2} if (hc.dvg_normal_scale if t == plan.ISECT['deformable_voxel_grid'] else hc.origin_scale) != 0.0 else set())
    elif t in (plan.ISECT['sphere_new'], plan.ISECT['cylinder_new']):
        z = {6, 7} | ({3, 4, 5} if (hc.resize_scale != 0.0 or hc.origin_scale != 0.0) else set()) | ({0, 1, 2} if hc.origin_scale != 0.0 else set())
    else:
        z = {0}
    three = {0, 1, 2}
    return {'f_z_vals': z, 'f_isect_sigma': {0}, 'f_offset_sigma': {0} if hc.point_offset else None, 'f_point_offset': three if hc.point_offset else None,
            'f_color_scale': three, 'f_color_shift': three, 'f_spatial_flow': three if (hc.advect and hc.use_spatial_flow) else None,
            'f_color_scale_global': set(range(9)) if hc.f_color_scale_global.channels == 9 else three, 'f_color_shift_global': three}


def _check_live_columns(hc):
    col, p_live, k = live_columns(hc)
    read = _read_channels(hc)
    live = set()
    for name in HEAD_FIELDS:
        f = getattr(hc, name)
        if f.offset >= 0 and read[name] is not None:
            live |= {f.offset + ch for ch in read[name]}
    # the map: the live user columns, in order, onto 0 .. p_live - 1; nothing at or beyond preds_per_z
    assert [i for i in range(64) if col[i] >= 0] == sorted(live)
    assert [col[i] for i in sorted(live)] == list(range(len(live))) and p_live == len(live) == k.preds_per_z
    # every channel the stage reads sits, in the kernels' configuration, at the live column of the user's column
    for name in HEAD_FIELDS:
        f, kf = getattr(hc, name), getattr(k, name)
        if f.offset < 0 or read[name] is None:
            assert kf.offset == -1, name
            continue
        assert kf.channels == f.channels
        for ch in read[name]:
            assert kf.offset + ch == col[f.offset + ch], (name, ch)
    # prune off: every column kept where it is
    col, p_live, k = live_columns(hc, prune=False)
    assert col == list(range(hc.preds_per_z)) + [-1] * (64 - hc.preds_per_z) and p_live == hc.preds_per_z == k.preds_per_z
    for name in HEAD_FIELDS:
        if getattr(hc, name).offset >= 0 and read[name] is not None:
            assert getattr(k, name).offset == getattr(hc, name).offset
    return live_columns(hc)


@pytest.mark.parametrize('case', sweep_cases())
def test_live_columns_of_every_sweep_fixture(case):
    for _, hc, _ in _levels(case):
        _check_live_columns(hc)


def test_live_columns_hand_made():
    """DoNeRF's head: z_vals 4 | sigma 1 | point_sigma 1 | point_offset 3 | color_scale 3 | color_shift 3 = 15 columns.  origin_scale is 0:
    the origin (0-2) is dead, and so is point_sigma (the point_offset stage reads `sigma`) -- 11 live; z_vals' offset becomes col[3] - 3 = -3.
    With origin_scale 0.5 the origin is read: 14 live.
    A 3x3 color_transform_global keeps all 9 channels of the global scale field (a head of z 1 | scale_global 9 | shift_global 3 | one
    unread column: 13 live of 14, the shift's offset stays 10)."""
    hc = _config('donerf_sphere')
    assert hc.preds_per_z == 15 and hc.f_z_vals.offset == 0 and hc.origin_scale == 0.0
    col, p_live, k = _check_live_columns(hc)
    assert p_live == 11 and col[:4] == [-1, -1, -1, 0] and k.f_z_vals.offset == -3
    assert col[:15].count(-1) == 4
    hc.origin_scale = 0.5
    col, p_live, k = _check_live_columns(hc)
    assert p_live == 14 and col[:4] == [0, 1, 2, 3] and k.f_z_vals.offset == 0

    hc = _config('donerf_sphere')
    absent = plan._absent_field()
    for name in HEAD_FIELDS:
        setattr(hc, name, absent)
    hc.isect_type, hc.point_offset, hc.preds_per_z = plan.ISECT['z_plane'], 0, 14
    hc.f_z_vals.offset, hc.f_z_vals.channels = 0, 1
    hc.f_color_scale_global.offset, hc.f_color_scale_global.channels = 1, 9
    hc.f_color_shift_global.offset, hc.f_color_shift_global.channels = 10, 3
    col, p_live, k = _check_live_columns(hc)
    assert p_live == 13 and col[:14] == list(range(13)) + [-1]
    assert (k.f_color_scale_global.offset, k.f_color_shift_global.offset) == (1, 10)
    hc.f_color_scale_global.channels = 3                # a plain global scale: channels 4 .. 9 of the block are dead
    col, p_live, k = _check_live_columns(hc)
    assert p_live == 7 and k.f_color_shift_global.offset == 4


# ---------------------------------------------------------------- hr_frame_time_tap
def _keyframe_configs():
    out = []
    for case in sweep_cases():
        for level, hc, _ in _levels(case):
            if hc.video and hc.num_keyframes >= 2:
                out.append(pytest.param(hc, id=f'{case}-{level}'))
    return out


@pytest.mark.parametrize('hc', _keyframe_configs())
def test_frame_time_tap_equals_the_kernels_arithmetic(hc):
    """hr_render_frame's tap against hr_base_time, hr_normalize_time and hr_make_tap of hr_math.h (host build), bit for bit: at the
    keyframe times k / flow_fac and one ulp to either side (where the rounding to a keyframe flips), before 0, and after the last
    keyframe."""
    hm = math_lib()
    K = hc.num_keyframes
    key = np.arange(K, dtype=np.float32) * np.float32(hc.flow_inv_fac) if hc.advect else np.linspace(0, 1, K, dtype=np.float32)
    half = key[:-1] + np.diff(key) / np.float32(2)            # where the nearest keyframe changes
    times = np.concatenate([key, np.nextafter(key, np.float32(-np.inf)), np.nextafter(key, np.float32(np.inf)),
                            half, np.nextafter(half, np.float32(-np.inf)), np.nextafter(half, np.float32(np.inf)),
                            np.asarray([-1.0, -1e-3, np.nextafter(np.float32(0), np.float32(-1)), key[-1] + 1e-3, 1.0, 2.0, 100.0], np.float32)]).astype(np.float32)
    rows = set()
    for t in times:
        i0, i1, w0, w1 = ctypes.c_int(), ctypes.c_int(), ctypes.c_float(), ctypes.c_float()
        hm.hm_time_tap(ctypes.byref(hc), ctypes.c_float(t), ctypes.byref(i0), ctypes.byref(i1), ctypes.byref(w0), ctypes.byref(w1))
        got = frame_time_tap(hc, float(t))
        want = (i0.value, i1.value, w0.value, w1.value)
        assert np.asarray(got[2:], np.float32).tobytes() == np.asarray(want[2:], np.float32).tobytes() and got[:2] == want[:2], (float(t), got, want)
        assert 0 <= got[0] < K and 0 <= got[1] < K
        rows.add(got[0] if got[2] >= got[3] else got[1])
    if hc.advect:
        assert rows == set(range(K))             # the times reach every keyframe row


# ---------------------------------------------------------------- hr_frame_plan
# model -> (tile rays, head buffers, LDS bytes) where the frame kernel fits under HR_OPT_FRAME_KERNEL = 2; the first two also fit under 1
FRAME = {
    'donerf_sphere': (64, 1, 160448), 'donerf_cylinder': (64, 1, 160448),
    'technicolor_z_plane': (32, 2, 159424), 'immersive_sphere': (32, 2, 160960), 'neural_3d_z_plane': (32, 1, 158912),
}


@pytest.mark.parametrize('model', C.MODEL_NAMES)
def test_frame_plan_of_every_benchmark_model(model):
    """LDS = activations 2 x tile x 264 x 2 B | head buffers x tile x HS x 4 B | decode matrices | 32 B of counters | 40 floats of ones, with HS
    = the head row's floats rounded up to 4 mod 8.
      DoNeRF (static [8, 4, 4], 32 samples x 11 live columns = 352 -> HS 356; 11 output tiles; RGB: one matrix per sample wavefront):
        64-ray tiles, one buffer, 8 sample wavefronts: 67 584 + 91 136 + 8 x 3 x 16 x 4 + 192 = 160 448.  Fits under modes 1 and 2.
      The keyframe nets take the video gather: 32-ray tiles, mode 2 only (SH: a matrix per ray in flight).
        technicolor (480 -> HS 484, ca 8, 2 rays per pass): 33 792 + 2 x 61 952 + 8 x 2 x 3 x 8 x 4 + 192 = 159 424, two buffers.
        immersive (480 -> 484, ca 16): 33 792 + 123 904 + 3 072 + 192 = 160 960, two buffers.
        Neural-3D (64 samples: 960 -> 964, one ray per pass): 33 792 + 32 x 964 x 4 + 8 x 3 x 16 x 4 + 192 = 158 912, one buffer.
    640 000 rays on 256 compute units: 10 000 / 20 000 tiles, a workgroup per compute unit."""
    hc = _config(model)
    tile, nbuf, lds = FRAME[model]
    for mode in (0, 1, 2):
        for frame_lines in (False, True):
            p = frame_plan(hc, n_rays=640000, frame_mode=mode, frame_lines=frame_lines)
            fits = mode >= (1 if tile == 64 else 2)
            assert bool(p.fits) == fits, (mode, frame_lines)
            if not fits:
                continue
            assert (p.tile_rays, p.nbuf, p.lds, p.ns) == (tile, nbuf, lds, 8) and p.lds <= 160 * KIB
            assert p.nb == (2 if tile == 64 else 4) and p.zp == (64 if model == 'neural_3d_z_plane' else 32)
            assert p.pclass == (2 if model == 'technicolor_z_plane' else 1)
            assert p.head_stride % 8 == 4 and p.head_stride >= 4 * ((hc.z_channels * live_columns(hc)[1] + 3) // 4)
            assert p.m_copies == (1 if model.startswith('donerf') else 64 // p.zp)
            assert (p.n_tiles, p.grid) == (640000 // tile, 256)
    p = frame_plan(hc, n_rays=1000, frame_mode=2)
    assert (p.n_tiles, p.grid) == (-(-1000 // tile),) * 2            # fewer tiles than compute units: a workgroup per tile


def test_frame_plan_refusals_and_options():
    """DoNeRF fits the 64-ray form; what takes it away:
      * four sample wavefronts (HR_OPT_SAMPLE_WAVES = 4) still fit: 4 matrices less, 159 680 bytes; the input tile, 64 x 2 x (32 + 8) x
        2 B = 10 240, stays inside the first 4 x 2 rays' rows (8 x 356 x 4 = 11 392);
      * origin_scale != 0 keeps 14 columns: 448 head columns are 14 output tiles of the last Linear, more than the 12 a 64-ray tile's
        wavefronts hold: no fit under mode 1; mode 2 takes 32-ray tiles with two buffers (HS 452: 33 792 + 115 712 + 1 536 + 192 = 151 232);
      * a skip connection into the last Linear, the verified fast path, a cascade, the exact-fp32 MLP, a generic decomposition, mode 0,
        more than 2^36 rays: the two-kernel path."""
    hc = _config('donerf_sphere')
    p = frame_plan(hc, sample_waves=4)
    assert (p.fits, p.tile_rays, p.ns, p.lds) == (1, 64, 4, 159680)
    wide = _copy(hc)
    wide.origin_scale = 0.5
    assert live_columns(wide)[1] == 14
    assert not frame_plan(wide, frame_mode=1).fits
    p = frame_plan(wide, frame_mode=2)
    assert (p.fits, p.tile_rays, p.nbuf, p.nb, p.head_stride, p.lds) == (1, 32, 2, 4, 452, 151232)
    skip = _copy(hc)
    skip.mlp_skip_mask |= 1 << (hc.mlp_layers - 1)
    generic = _copy(hc)
    for j in range(3):
        generic.n_den[j] = generic.n_app[j] = 8
    for mode in (1, 2):
        assert not frame_plan(skip, frame_mode=mode).fits
        assert not frame_plan(generic, frame_mode=mode).fits
        assert not frame_plan(hc, frame_mode=mode, verified=True).fits
        assert not frame_plan(hc, frame_mode=mode, cascade=True).fits
        assert not frame_plan(hc, frame_mode=mode, split_mlp=False).fits
        assert not frame_plan(hc, frame_mode=mode, n_rays=(1 << 36) + 1).fits
        assert frame_plan(hc, frame_mode=mode).fits
    assert not frame_plan(hc, frame_mode=0).fits
    # 8 or 128 samples per ray: no instantiation of the frame kernel
    for z in (8, 128):
        assert not frame_plan(_config('donerf_sphere', z=z), frame_mode=2).fits
