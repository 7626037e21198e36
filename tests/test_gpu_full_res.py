"""`-m gpu`: one render() call at the frame sizes the reference ships, not the 800x800 frames of the rest of the suite.

Above 640 000 rays a call takes paths no smaller call reaches:
  * the verified fast path's list (csrc/hr_plan.h hr_redo_list_cap: max(32 768, n / 16) entries) outgrows the chunk's head workspace, so
    the second pass walks it in more than one slice -- Technicolor 2048x1088 (139 264 entries over a 131 072-ray workspace), Neural-3D
    1352x1014 (85 696 over 65 536), Neural-3D 2704x2028 (342 784: six slices);
  * hr_even_chunk() ends 1352x1014 in a launch that is not a multiple of 64 rays;
  * the persistent frame kernel (csrc/fused_impl.inc) deals 1.6 - 3.5 times the tiles of an 800x800 frame over its workgroups;
  * the viewer path (hr_generate_rays -> render -> hr_pack_display) meets non-square frames.
What is held: against the CPU restatement of the reference (oracle/torch_port.py) on a chosen subset of every frame, no ray over 1e-4; the
verified path over every ray, bit for bit; repeat calls, chunked calls, hipGraph replay and the frame kernel equal to the one-call image.
One family's grids are held at a time (_family); the oracle runs once per family."""
import math
import os

import numpy as np
import pytest
import torch

from helpers import even_chunk, redo_list_cap
from hyperreel_amd import config as C
from hyperreel_amd import scenes

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4
SUBSET = 131072
# (H, W) of one render() call, as the reference's configs ship them
FRAMES = {
    'technicolor_z_plane': (1088, 2048),    # conf/experiment/dataset/technicolor.yaml:8  img_wh: [2048, 1088]
    'neural_3d_z_plane': (1014, 1352),      # conf/experiment/dataset/neural_3d.yaml:9    img_wh: [1352, 1014]
    'immersive_sphere': (960, 1280),        # conf/experiment/dataset/immersive.yaml:8    img_wh: [1280, 960]
    'donerf_sphere': (1024, 1024),          # scripts/demo_donerf.sh:19  render_ray_chunk=1048576: one 2^20-ray call
}
N3D_FULL = (2028, 2704)                     # conf/experiment/dataset/neural_3d.yaml:8 (commented out): #img_wh: [2704, 2028]
KEYFRAME = ('technicolor_z_plane', 'neural_3d_z_plane', 'immersive_sphere')
FOV = 40.0                                  # scenes.benchmark_rays


def launch_starts(chunk, n):
    per = even_chunk(chunk, n)
    return list(range(per, n, per))


class _Family:
    """One family at its shipped frame size: weights at the final grid, the benchmark camera's rays, lazily built models per arithmetic and
    their images of the whole frame (each rendered once), the oracle on the checked subset."""

    def __init__(self, model):
        self.name = model
        self.H, self.W = FRAMES[model]
        self.cfg, self.ds = C.model_config(model), C.dataset_scalars(model)
        self.sd = scenes.make_state_dict(self.cfg, self.ds, None, seed=7, density='dense', app_scale=1.0)
        self.rays_np = scenes.benchmark_rays(model, self.H, self.W, frame=7)
        self.rays = torch.from_numpy(self.rays_np).cuda()
        self.n = self.rays.shape[0]
        self.t = float(self.rays_np[0, -1]) if model in KEYFRAME else None
        self.models, self.images = {}, {}
        self.redo, self.redo_overflowed = None, None
        self.ref = None

    def model(self, precision):
        if precision not in self.models:
            from gpu_common import make_render_fn
            self.models[precision] = make_render_fn(self.cfg, self.ds, self.sd, mlp_precision=precision).model
        return self.models[precision]

    def image(self, precision, frame=False):
        """The whole frame in one render() call (frame: through hr_render_frame)."""
        key = (precision, frame)
        if key not in self.images:
            m = self.model(precision)
            img = m.render(self.rays, frame_time=self.t if frame else None)['rgb'].clone()
            torch.cuda.synchronize()
            if precision == 'auto' and not frame:
                self.redo, self.redo_overflowed = m.redo_count(), m.redo_overflowed()
            self.images[key] = img
        return self.images[key]

    def subset(self):
        """Indices of the checked rays: +-2 about every launch boundary, the last 4 096 rays, 4 096 from 2^20 on, every ray where plain
        f16f8 and f16x3 differ by more than 1e-5 (the decisions the verified path's second pass repairs), the rest drawn with a fixed seed."""
        n = self.n
        must = [np.arange(max(n - 4096, 0), n)]
        for p in ('auto', 'f16x3', 'fp32', 'f16f8'):
            for b in launch_starts(self.model(p).chunk_rays(), n):
                must.append(np.arange(b - 2, min(b + 3, n)))
        if n > (1 << 20):
            must.append(np.arange((1 << 20) - 2, min((1 << 20) + 4094, n)))
        d = (self.image('f16f8') - self.image('f16x3')).abs().amax(-1)
        self.n_fast_diff = int((d > 1e-5).sum())
        must.append(torch.nonzero(d > 1e-5).flatten().cpu().numpy())
        idx = np.unique(np.concatenate(must)).astype(np.int64)
        if idx.size < SUBSET:
            rest = np.setdiff1d(np.arange(n, dtype=np.int64), idx, assume_unique=True)
            idx = np.union1d(idx, np.random.default_rng(11).choice(rest, SUBSET - idx.size, replace=False))
        return idx

    def oracle(self):
        if self.ref is None:
            from torch_port import TorchPort
            idx = self.subset()
            torch.set_num_threads(min(16, os.cpu_count() or 8))
            self.ref = (idx, np.asarray(TorchPort(self.cfg, self.ds, self.sd).render(self.rays_np[idx], chunk=16384)['rgb']))
        return self.ref


_cache = {}


def _family(model):
    if model not in _cache:
        _cache.clear()                       # one family's grids at a time (host and device)
        import gc
        gc.collect()
        torch.cuda.empty_cache()
        _cache[model] = _Family(model)
    return _cache[model]


def _render_into_nan(m, rays):
    # a ray that no wavefront wrote must not inherit a plausible value from whatever the allocator handed back
    out = torch.full((rays.shape[0], 3), float('nan'), dtype=torch.float32, device=rays.device)
    m.render(rays, out=out)
    torch.cuda.synchronize()
    return out


def _check_verified(what, n, auto, fast, safe, n_redo, overflowed, expect_listed):
    """`auto`'s image against the plain f16f8 (`fast`) and f16x3 (`safe`) images of the same weights and rays, over every ray."""
    is_fast = (auto == fast).all(-1)
    is_safe = (auto == safe).all(-1)
    assert bool((is_fast | is_safe).all()), f'{what}: {int((~(is_fast | is_safe)).sum())} pixels are neither arithmetic\'s'
    repaired = int((is_safe & ~is_fast).sum())
    assert repaired <= n_redo, f'{what}: {repaired} pixels are the f16x3 pixel only, {n_redo} rays were listed'
    d_ver = (auto - safe).abs().amax(-1)
    over = int((d_ver > RGB_TOL).sum())
    flips = int(((fast - safe).abs().amax(-1) > RGB_TOL).sum())
    assert over == 0, (f'{what}: {over} rays over 1e-4 from the f16x3 image (plain f16f8: {flips}); worst {float(d_ver.max()):.3e} at ray '
                       f'{int(d_ver.argmax())}; {n_redo} rays listed')
    assert not overflowed, f'{what}: the list overflowed ({n_redo} listed, {redo_list_cap(n)} entries)'
    assert n_redo <= 0.08 * n, f'{what}: {n_redo} rays listed'
    if expect_listed:
        assert n_redo > 0
    print(f'{what}: {n} rays, {n_redo} listed ({100.0 * n_redo / n:.3f} %, list {redo_list_cap(n)}), {repaired} repaired pixels, '
          f'plain f16f8 rays over the bar {flips}, worst after the second pass {float(d_ver.max()):.2e}')


# ---- 1. full-size frames against the oracle
@pytest.mark.parametrize('precision', ['auto', 'f16x3', 'fp32'])
@pytest.mark.parametrize('model', ['donerf_sphere', 'immersive_sphere', 'technicolor_z_plane', 'neural_3d_z_plane'])
def test_full_size_frame_against_the_oracle(model, precision):
    f = _family(model)
    idx, ref = f.oracle()
    idx_t = torch.from_numpy(idx).cuda()
    for frame in ((False, True) if f.t is not None else (False,)):
        rgb = f.image(precision, frame)
        what = f'{model} {f.W}x{f.H} / {precision}' + (' through hr_render_frame' if frame else '')
        assert rgb.shape == (f.n, 3) and bool(torch.isfinite(rgb).all()), what
        err = np.abs(rgb[idx_t].cpu().numpy() - ref).max(-1)
        over = int((err > RGB_TOL).sum())
        assert over == 0, f'{what}: {over} of {idx.size} rays over 1e-4 (worst {err.max():.3e} at ray {int(idx[err.argmax()])})'
        print(f'{what}: {idx.size} rays checked ({f.n_fast_diff} where f16f8 and f16x3 differ by > 1e-5), worst {err.max():.2e}')


# ---- 2. the verified path over every ray of the frame
@pytest.mark.parametrize('model', ['neural_3d_z_plane', 'technicolor_z_plane', 'immersive_sphere', 'donerf_sphere'])
def test_verified_path_over_every_ray_of_the_frame(model):
    f = _family(model)
    auto, fast, safe = f.image('auto'), f.image('f16f8'), f.image('f16x3')
    m = f.model('auto')
    assert m.mlp_verified() and not f.model('f16f8').mlp_verified()
    _check_verified(f'{model} {f.W}x{f.H}', f.n, auto, fast, safe, f.redo, f.redo_overflowed, model in ('donerf_sphere', 'neural_3d_z_plane'))
    # a repeat call reproduces the image (the list's counter was handed over to the next call clean)
    assert torch.equal(_render_into_nan(m, f.rays), auto)


# ---- 4c. the persistent frame kernel over the whole frame
@pytest.mark.parametrize('model', ['donerf_sphere', 'immersive_sphere', 'technicolor_z_plane', 'neural_3d_z_plane'])
def test_frame_kernel_full_size_every_word_twice(model):
    f = _family(model)
    two = f.image('f16x3')
    m = f.model('f16x3')
    m.set_execution(frame_kernel=2 if f.t is not None else True)
    try:
        assert m.frame_kernel_active()
        for _ in range(2):
            one = _render_into_nan(m, f.rays)
            assert torch.equal(one, two), f'{model}: {int((one != two).any(-1).sum())} rays differ from the two-kernel image'
    finally:
        m.set_execution(frame_kernel=False)


def test_neural_3d_full_resolution_verified_over_every_ray():
    """The commented-out full resolution of the Neural-3D config: 5 483 712 rays in one call, six slices of the list."""
    f = _family('neural_3d_z_plane')
    H, W = N3D_FULL
    rays = torch.from_numpy(scenes.benchmark_rays('neural_3d_z_plane', H, W, frame=7)).cuda()
    n = rays.shape[0]
    img = {}
    for p in ('auto', 'f16f8', 'f16x3'):
        f.model(p)._render_calls = 1000              # one call each: the frame as rendered, not re-rendered after a host re-decision
        img[p] = _render_into_nan(f.model(p), rays)
        if p == 'auto':
            n_redo, overflowed = f.model(p).redo_count(), f.model(p).redo_overflowed()
    assert bool(torch.isfinite(img['auto']).all())
    _check_verified(f'neural_3d_z_plane {W}x{H}', n, img['auto'], img['f16f8'], img['f16x3'], n_redo, overflowed, True)


# ---- 3. a populated multi-slice walk at the default chunk
def test_the_list_is_walked_in_slices_at_the_default_chunk():
    """Neural-3D 1352x1014 with the finalize default workspace (no reserve()): its list holds more entries than the workspace has rows, and
    every k-th ray leans 63 degrees off the planes' normal (listed by its conditioning alone, as in
    test_gpu_verified.py::test_the_list_is_walked_in_slices_of_the_workspace) so that the list fills to the middle of (chunk, cap)."""
    f = _family('neural_3d_z_plane')
    auto, fast, safe = f.model('auto'), f.model('f16f8'), f.model('f16x3')
    f.image('auto')
    n, n0, chunk, cap = f.n, f.redo, auto.chunk_rays(), redo_list_cap(f.n)
    assert chunk < cap, (chunk, cap)                 # the premise: more than one slice
    assert n0 < chunk, n0
    target = (chunk + cap) // 2
    k = int(math.ceil(n / (target - n0)))
    lean = np.arange(0, n, k)
    rays_np = f.rays_np.copy()
    d = np.array([0.6, 0.65, -0.4665], np.float32)
    rays_np[lean, 3:6] = d / np.linalg.norm(d)
    rays = torch.from_numpy(rays_np).cuda()
    for m in (auto, fast):
        m._render_calls = 1000                       # past the calls on which render() polls the sticky bits itself
    out = _render_into_nan(auto, rays)
    n_redo, overflowed = auto.redo_count(), auto.redo_overflowed()
    ref, cheap = safe.render(rays)['rgb'], fast.render(rays)['rgb']
    torch.cuda.synchronize()
    assert auto.mlp_verified(), auto.verify_info()
    assert chunk < n_redo <= cap and not overflowed, (f'{n_redo} listed (natural {n0}, {lean.size} leaning rays every {k}th), '
                                                      f'workspace {chunk}, list {cap}, overflowed {overflowed}')
    lean_t = torch.from_numpy(lean).cuda()
    moved = int((cheap[lean_t] != ref[lean_t]).any(-1).sum())
    assert torch.equal(out[lean_t], ref[lean_t]), f'{int((out[lean_t] != ref[lean_t]).any(-1).sum())} leaning rays differ from the f16x3 image'
    is_safe, is_fast = (out == ref).all(-1), (out == cheap).all(-1)
    assert bool((is_safe | is_fast).all()) and int((is_safe & ~is_fast).sum()) <= n_redo
    print(f'neural_3d_z_plane {f.W}x{f.H}: {n_redo} listed over {-(-n_redo // chunk)} slices of {chunk} (natural {n0}); {lean.size} leaning rays, '
          f'{moved} of them with an f16f8 pixel unlike the f16x3 one')
    # the next call starts from a clean list
    few = f.rays[:4096].contiguous()
    a2, s2 = auto.render(few)['rgb'], safe.render(few)['rgb']
    torch.cuda.synchronize()
    assert auto.redo_count() < few.shape[0] // 4 and float((a2 - s2).abs().max()) <= RGB_TOL


# ---- 5. the viewer path on non-square frames
def _camera(model, H, W):
    pose = scenes.look_at_pose((0.05, 0.03, 1.0), (0.0, 0.0, -1.0)) if 'z_plane' in model else scenes.look_at_pose((0.3, 0.0, 0.0), (1.0, 0.1, 0.05))
    focal = 0.5 * W / math.tan(0.5 * math.radians(FOV))
    K = np.asarray([[focal, 0, W / 2.0], [0, focal, H / 2.0], [0, 0, 1]], np.float32)
    return pose, K


def _to8b(rgb, H, W, transpose, flip):
    """The viewer's host path (utils/gui_utils.py:174-205, to8b utils/__init__.py:47), as test_gpu_zz_display.py restates it."""
    ref = rgb.reshape(H, W, 3)
    if transpose:
        ref = ref.transpose(1, 0, 2)
    if flip:
        ref = np.flip(ref, axis=0)
    return (255 * np.clip(np.ascontiguousarray(ref), 0, 1)).astype(np.uint8)


COMBOS = [(False, False), (True, False), (False, True), (True, True)]


@pytest.mark.parametrize('model', ['neural_3d_z_plane', 'technicolor_z_plane'])
def test_viewer_path_on_non_square_frames(model):
    f = _family(model)
    m = f.model('auto')
    H, W = f.H, f.W
    pose, K = _camera(model, H, W)
    ref = scenes.pinhole_rays(H, W, FOV, pose, cam_id=0, time=f.t)
    got = m.generate_rays(pose, K, W, H, f.t)
    torch.cuda.synchronize()
    got_np = got.cpu().numpy()
    assert got_np.shape == ref.shape and float(np.abs(got_np - ref).max()) <= 2e-7
    lo, hi = 3 * W + 17, (H - 5) * W + W // 3                     # starts and ends mid-row
    part = m.generate_rays(pose, K, W, H, f.t, pixel_range=(lo, hi)).cpu().numpy()
    assert part.shape == (hi - lo, ref.shape[1]) and np.array_equal(part, got_np[lo:hi])

    def frame():
        rgb = m.render_camera(pose, K, W, H, time=f.t)
        return [rgb] + [m.pack_display(rgb, H, W, tr, fl) for tr, fl in COMBOS]
    eager = [x.clone() for x in frame()]
    torch.cuda.synchronize()
    assert torch.equal(eager[0], m.render(got, frame_time=f.t)['rgb'])
    rgb_np = eager[0].cpu().numpy()
    for (tr, fl), px in zip(COMBOS, eager[1:]):
        assert px.shape == ((W, H, 4) if tr else (H, W, 4)) and px.dtype == torch.uint8
        px = px.cpu().numpy()
        assert np.array_equal(px[..., :3], _to8b(rgb_np, H, W, tr, fl)) and (px[..., 3] == 255).all(), (tr, fl)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        frame()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        outs = frame()
    for _ in range(2):
        outs[0].fill_(float('nan'))
        for o in outs[1:]:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for o, e in zip(outs, eager):
            assert torch.equal(o, e)


# ---- 4a / 4b. hipGraph replay and the reference's chunked calls of the 2.2 M-ray frame
def test_technicolor_frame_replays_from_a_hipgraph():
    f = _family('technicolor_z_plane')
    m = f.model('auto')
    eager = f.image('auto')
    assert m.mlp_verified() and redo_list_cap(f.n) > m.chunk_rays()          # two slices of the list in the captured plan
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.render(f.rays)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        out = m.render(f.rays)['rgb']
    for _ in range(3):
        out.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), f'{int((out != eager).any(-1).sum())} rays differ from the eager image'


def test_technicolor_frame_in_the_reference_chunks():
    """render_chunked with the reference's render_ray_chunk (scripts/demo_technicolor.sh): 1 048 576 + 1 048 576 + 131 072 rays.  Every
    call starts on a multiple of 64 rays, so the tiles -- and what each lists -- are those of the one call."""
    from hyperreel_amd.render import render_chunked
    f = _family('technicolor_z_plane')
    m = f.model('auto')
    one = f.image('auto')
    got = render_chunked(f.rays, lambda r: m.render(r), {}, 1048576)['rgb']
    torch.cuda.synchronize()
    assert got.shape == one.shape and torch.equal(got, one), f'{int((got != one).any(-1).sum())} rays differ from the one-call image'
