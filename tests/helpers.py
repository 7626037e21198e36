"""Shared test plumbing: golden fixtures -> (cfg, dataset scalars, regenerated weights, rays, expected)."""
import ctypes
import functools
import glob
import json
import os

import numpy as np

from hyperreel_amd import config as C
from hyperreel_amd import scenes
from hyperreel_amd.build import build_host_library

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def reference_facts():
    """What the reference's own configuration and construction code says, recorded by oracle/refgen/make_reference_facts.py."""
    with open(os.path.join(GOLDEN_DIR, 'reference_facts.json')) as f:
        return json.load(f)


def model_group_digest(cfg):
    """sha256 of a parsed model group in the canonical form reference_facts() records for the shipped YAML."""
    import hashlib
    return hashlib.sha256(json.dumps(C.to_plain(cfg), sort_keys=True).encode()).hexdigest()


def golden_cases():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, '*.npz')))


def initialiser_golden_cases():
    """golden_cases() without the fixtures whose MLP is scaled away from the initialiser (scenes.MLP_VARIANTS): the reduced-precision
    arithmetics that are opt-in by name (f16x2, plain f16f8, bf16x3) carry an error proportional to the weights and are not held to the
    1e-4 bar there -- 'auto' (which is), f16x3 and fp32 are."""
    return [c for c in golden_cases() if not c.endswith(('_hostile', '_stiff'))]


def sweep_cases():
    """One fixture per shipped model YAML the backend accepts (oracle/refgen/make_sweep.py)."""
    return sorted('sweep/' + os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, 'sweep', '*.npz')))


def sweep_coverage():
    with open(os.path.join(GOLDEN_DIR, 'sweep', 'coverage.json')) as f:
        return json.load(f)


class Golden:
    def __init__(self, case):
        z = np.load(os.path.join(GOLDEN_DIR, case + '.npz'))
        self.arrays = {k: z[k] for k in z.files if k != 'recipe'}
        self.recipe = json.loads(bytes(z['recipe']).decode())
        r = self.recipe
        if 'model_cfg' in r:        # sweep fixtures carry the parsed YAML group (no /root/reference on the GPU box)
            self.cfg = C.epoch_to_iter(C.to_cfg(r['model_cfg']), 4000)
        else:
            self.cfg = C.model_config(r['model'], z_channels=r['z_channels'])
        self.iteration = r.get('iter')          # training iteration of the activation / PE schedules (None: converged)
        self.dataset = r['dataset']
        self.grid = r['grid']
        self.rays = self.arrays['rays']
        if 'frame_idx' in self.arrays:          # rays of the 800x800 benchmark frame, stored as pixel indices (make_golden.py)
            at, frame = (int(v) for v in self.arrays['frame_at'])
            part = scenes.benchmark_rays(r['model'], 800, 800, frame=frame)[self.arrays['frame_idx']]
            self.rays = np.ascontiguousarray(np.concatenate([self.rays[:at], part, self.rays[at:]], 0), np.float32)
        self.rgb = self.arrays['rgb']
        self._sd = None

    @property
    def state_dict(self):
        if self._sd is None:
            r = self.recipe
            self._sd = scenes.make_state_dict(self.cfg, self.dataset, r['grid'], r['seed'], r['density'], r['app_scale'], r.get('mlp', 'default'))
            got = scenes.state_dict_checksum(self._sd)
            assert abs(got - r['checksum']) <= 1e-6 * max(1.0, abs(r['checksum'])), \
                f'regenerated weights differ from the ones the golden was made with ({got} vs {r["checksum"]})'
            for k in self.arrays:              # tensors the fixture stores in full (post-fit weights: oracle/refgen/make_golden.py, POSTFIT)
                if k.startswith('sd/'):
                    self._sd[k[3:]] = self.arrays[k]
        return self._sd


def linf(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)))) if np.size(a) else 0.0


def trainable_sweep_cases(cascades=False):
    """The sweep fixtures' single-level models, or with `cascades` the point_prediction ones (their coarse and fine stages are
    checked separately).  The training path differentiates every one of them (tests/test_train_host.py asks hr_train_unsupported), and
    oracle/torch_port.py restates them."""
    from hyperreel_amd import plan
    return [c for c in sweep_cases() if plan.is_cascade(Golden(c).cfg) == bool(cascades)]


class GradGolden:
    """Gradients of sum(rgb * G) from the REFERENCE'S OWN autograd in train mode (oracle/refgen/make_grad_golden.py): full arrays for
    small tensors, 16 seeded projections + the L2 norm for the MLP's large matrices."""

    def __init__(self, case, white):
        z = np.load(os.path.join(GOLDEN_DIR, 'grad', f'{case}_bg{int(white)}.npz'))
        self.recipe = json.loads(bytes(z['recipe']).decode())
        self.rgb = z['rgb']
        self.full = {k[5:]: z[k] for k in z.files if k.startswith('full/')}
        self.proj = {k[5:]: z[k] for k in z.files if k.startswith('proj/')}
        self.norm = {k[5:]: z[k] for k in z.files if k.startswith('norm/')}
        self.n_rays = int(self.recipe['n_rays'])
        self.G = np.random.default_rng(self.recipe['g_seed']).standard_normal((self.n_rays, 3)).astype(np.float32)

    def names(self):
        return sorted(set(self.full) | set(self.proj))

    def check(self, name, got, rel):
        """got: the gradient of tensor `name` (any shape with the same element order).  rel: tolerance relative to the reference
        gradient's largest element (full) / to its norm (projections: each is a N(0, |g|^2) combination of the elements)."""
        got = np.asarray(got, np.float64).ravel()
        if name in self.full:
            want = self.full[name].astype(np.float64).ravel()
            assert got.size == want.size, (name, got.size, want.size)
            scale = np.abs(want).max()
            err = np.abs(got - want).max()
            assert err <= rel * scale + 1e-9, f'{name}: |err| {err:.3e} vs max |g| {scale:.3e}'
        else:
            norm, size = self.norm[name]
            assert got.size == int(size), (name, got.size, size)
            seed = (sum(ord(c) * (i + 1) for i, c in enumerate(name)) * 2654435761 + got.size) % (2 ** 32)
            v = np.random.default_rng(seed).standard_normal((16, got.size)).astype(np.float32).astype(np.float64)
            err = np.abs(v @ got - self.proj[name]).max()
            assert err <= rel * norm * 4.0 + 1e-9, f'{name}: projection error {err:.3e} vs |g| {norm:.3e}'
            assert abs(np.linalg.norm(got) - norm) <= rel * norm + 1e-9, name


def port_leaves(port):
    """TorchPort tensors under the reference's parameter names (the keys of a gradient golden)."""
    out = {}
    net = 'model.color_model.net.'
    video = bool(port.o.video) if hasattr(port, 'o') else bool(getattr(port, 'video', False))
    a_name, b_name = ('plane_space', 'plane_time') if video else ('plane', 'line')
    for kind, ga, gb in (('density', port.d_a, port.d_b), ('app', port.a_a, port.a_b)):
        for j in range(3):
            out[f'{net}{kind}_{a_name}.{j}'] = ga[j]
            out[f'{net}{kind}_{b_name}.{j}'] = gb[j]
    out[net + 'basis_mat.weight'] = port.basis
    n = len(port.layers)
    for i, (w, b) in enumerate(port.layers):
        mid = f'{i}.0' if i < n - 1 else f'{i}'
        out[f'model.embedding_model.embeddings.0.net.layers.{mid}.weight'] = w
        out[f'model.embedding_model.embeddings.0.net.layers.{mid}.bias'] = b
    return out


class GridPlane(ctypes.Structure):          # mirrors HrGridPlane (hyperreel_amd/csrc/hr_grid.h)
    _fields_ = [('a', ctypes.c_void_p), ('b', ctypes.c_void_p)] + [(k, ctypes.c_int) for k in
                ('tex', 'aw', 'ah', 'bw', 'bh', 'cd4', 'ca4', 'ax', 'ay', 'bx', 'app_off', 'app_real', 'app_real_off')]


class TrainPlan(ctypes.Structure):          # mirrors HrTrainPlan (hyperreel_amd/csrc/hr_plan.h)
    _fields_ = [(k, ctypes.c_int) for k in ('zp', 'thread_per_ray', 'rays_per_group', 'a_pc', 'a_nb')] + [('a_blocks', ctypes.c_uint), ('a_lds', ctypes.c_size_t)] + \
               [(k, ctypes.c_int) for k in ('backward', 'taps', 'lines', 'keyed', 'b_pc', 'passes')] + \
               [('pass_pairs', ctypes.c_uint * 2), ('pass_add_dp', ctypes.c_int * 2), ('pass_lds', ctypes.c_size_t * 2), ('lines_lds', ctypes.c_size_t),
                ('lines_blocks', ctypes.c_uint), ('bucket_lds', ctypes.c_size_t), ('atomics_rpb', ctypes.c_int), ('atomics_blocks', ctypes.c_uint),
                ('atomics_lds', ctypes.c_size_t), ('tail_blocks', ctypes.c_uint)]


class SamplePlan(ctypes.Structure):         # mirrors HrSamplePlan (hyperreel_amd/csrc/hr_plan.h)
    _fields_ = [(k, ctypes.c_int) for k in ('zp', 'pclass', 'all_lines', 'big_lds')] + [('blocks', ctypes.c_uint), ('lds', ctypes.c_size_t)]


class SampleFormPlan(ctypes.Structure):     # mirrors HrSampleFormPlan: HrSamplePlan and the form's own block
    _fields_ = SamplePlan._fields_ + [('x_off', ctypes.c_int), ('d_slots', ctypes.c_int)]


class FramePlan(ctypes.Structure):          # mirrors HrFramePlan (hyperreel_amd/csrc/hr_plan.h)
    _fields_ = [(k, ctypes.c_int) for k in ('fits', 'zp', 'pclass', 'tile_rays', 'ns', 'nb', 'nbuf', 'm_copies', 'head_stride', 'n_tiles', 'grid')] + \
               [('lds', ctypes.c_size_t)]


class TimeTap(ctypes.Structure):            # mirrors HrTimeTap (hyperreel_amd/csrc/hr_plan.h)
    _fields_ = [('i0', ctypes.c_int), ('i1', ctypes.c_int), ('w0', ctypes.c_float), ('w1', ctypes.c_float)]


PLANE_CLASS = ['generic', '8,4,4', '8,0,0']          # hr_plane_class
REDO_BUFFER = 1 << 22                                # entries of the verified path's list buffer (hr_model_reserve)


@functools.lru_cache(maxsize=None)
def plan_lib():
    """Host build of hyperreel_amd/csrc/hr_plan.h (tests/host_math/hr_plan_host.cpp): the library's own geometry and dispatch decisions."""
    here = os.path.dirname(os.path.abspath(__file__))
    src = os.path.join(here, 'host_math', 'hr_plan_host.cpp')
    deps = [src, os.path.join(here, '..', 'include', 'hyperreel_hip.h')] + [os.path.join(here, '..', 'hyperreel_amd', 'csrc', f) for f in ('hr_plan.h', 'hr_grid.h', 'hr_train.h', 'hr_math.h')]
    lib = ctypes.CDLL(build_host_lib(os.path.join(here, 'host_math', '_build', 'libhr_plan_host.so'), src, deps))
    assert lib.hp_sizeof_plane() == ctypes.sizeof(GridPlane) and lib.hp_sizeof_plan() == ctypes.sizeof(TrainPlan)
    assert lib.hp_sizeof_sample_plan() == ctypes.sizeof(SamplePlan) and lib.hp_sizeof_frame_plan() == ctypes.sizeof(FramePlan)
    assert lib.hp_sizeof_time_tap() == ctypes.sizeof(TimeTap)
    lib.hp_default_chunk.restype = lib.hp_even_chunk.restype = ctypes.c_longlong
    lib.hp_default_chunk.argtypes = [ctypes.c_longlong, ctypes.c_int]
    lib.hp_even_chunk.argtypes = [ctypes.c_longlong, ctypes.c_longlong]
    lib.hp_redo_list_cap.argtypes = [ctypes.c_longlong, ctypes.c_int]
    lib.hp_wide_cap.argtypes = [ctypes.c_longlong]
    lib.hp_sample_lds_bytes.restype = ctypes.c_size_t
    lib.hp_frame_time_tap.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]
    lib.hp_calib_sample.argtypes = [ctypes.c_longlong, ctypes.c_void_p]
    lib.hp_band_margins.argtypes = [ctypes.c_float] * 4 + [ctypes.c_void_p]
    lib.hp_listed_frac.restype = ctypes.c_float
    lib.hp_listed_frac.argtypes = [ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_uint]
    lib.hp_verify_fallback.argtypes = [ctypes.c_float, ctypes.c_float]
    return lib


@functools.lru_cache(maxsize=None)
def math_lib():
    """Host build of hyperreel_amd/csrc/hr_math.h (tests/host_math/hr_math_host.cpp): the formulas the kernels call."""
    here = os.path.dirname(os.path.abspath(__file__))
    src = os.path.join(here, 'host_math', 'hr_math_host.cpp')
    deps = [src, os.path.join(here, '..', 'hyperreel_amd', 'csrc', 'hr_math.h'), os.path.join(here, '..', 'include', 'hyperreel_hip.h')]
    lib = ctypes.CDLL(build_host_lib(os.path.join(here, 'host_math', '_build', 'libhr_math_host.so'), src, deps))
    lib.hm_normalize_time.restype = ctypes.c_float
    lib.hm_normalize_time.argtypes = [ctypes.c_void_p, ctypes.c_float]
    lib.hm_time_tap.argtypes = [ctypes.c_void_p, ctypes.c_float] + [ctypes.c_void_p] * 4
    return lib


@functools.lru_cache(maxsize=None)
def train_lib():
    """Host build of hyperreel_amd/csrc/hr_train.h (tests/host_math/hr_train_host.cpp): the training path's per-ray / per-sample phases."""
    here = os.path.dirname(os.path.abspath(__file__))
    src = os.path.join(here, 'host_math', 'hr_train_host.cpp')
    deps = [src, os.path.join(here, '..', 'include', 'hyperreel_hip.h')] + [os.path.join(here, '..', 'hyperreel_amd', 'csrc', f) for f in ('hr_train.h', 'hr_mask.h', 'hr_math.h', 'hr_grid.h', 'hr_plan.h')]
    lib = ctypes.CDLL(build_host_lib(os.path.join(here, 'host_math', '_build', 'libhr_train_host.so'), src, deps))
    lib.ht_unsupported.restype = ctypes.c_char_p
    assert lib.ht_sizeof_plane() == ctypes.sizeof(GridPlane)
    return lib


def even_chunk(chunk, n):
    """hr_even_chunk: rays per launch of a call of n rays on a workspace of `chunk` rays."""
    return plan_lib().hp_even_chunk(chunk, n)


def redo_list_cap(n, buffer_cap=REDO_BUFFER):
    """hr_redo_list_cap: entries of the verified path's list one call of n rays may fill."""
    return plan_lib().hp_redo_list_cap(n, buffer_cap)


def live_columns(hc, prune=True):
    """hr_live_columns of a compiled config: (user column -> live column or -1, for all 64 slots; p_live; the kernels' config)."""
    col, p_live, kcfg = (ctypes.c_int * 64)(), ctypes.c_int(), type(hc)()
    plan_lib().hp_live_columns(ctypes.byref(hc), int(bool(prune)), col, ctypes.byref(p_live), ctypes.byref(kcfg))
    return list(col), p_live.value, kcfg


def live_head_columns(hc):
    """Per-sample head columns the path reads, as booleans over the user's preds_per_z columns.  The library drops the others from
    the last Linear; `hr_render_fields` reports them as 0."""
    return [c >= 0 for c in live_columns(hc)[0][:hc.preds_per_z]]


def sample_lds_refused(hc):
    """(hr_model_create refuses a level of `hc` for the sample kernel's LDS, the kernel's request in bytes)."""
    n = ctypes.c_size_t()
    return bool(plan_lib().hp_sample_lds_refused(ctypes.byref(hc), ctypes.byref(n))), n.value


def sample_plan(hc, n_rays=4096, rows_emitted=False, frame_lines=False):
    """hr_sample_plan for a model of `hc` (frame_lines: inside hr_render_frame) and the instantiation (ZP, HALF, PC, NB) it launches."""
    out, inst = SamplePlan(), (ctypes.c_int * 4)()
    plan_lib().hp_sample_plan(ctypes.byref(hc), ctypes.c_longlong(n_rays), int(bool(rows_emitted)), int(bool(frame_lines)), ctypes.byref(out), inst)
    return out, tuple(inst)


SAMPLE_KIND = {'decode': 0, 'shade': 1, 'time': 2, 'time_density': 3}        # HrSampleKind
ROUTE = {'frame': 0, 'verified': 1, 'chunked': 2}                             # HrRoute


def sample_form_plan(hc, kind, n_rays=4096, maps=False, exported=False, frame_lines=False):
    """hr_sample_form_plan for a launch of form (kind, maps, exported) on a model of `hc`, and the instantiation hr_sample_dispatch names."""
    out, inst = SampleFormPlan(), (ctypes.c_int * 4)()
    assert plan_lib().hp_sizeof_sample_form_plan() == ctypes.sizeof(SampleFormPlan)
    plan_lib().hp_sample_form_plan(ctypes.byref(hc), ctypes.c_longlong(n_rays), int(bool(frame_lines)), SAMPLE_KIND[kind], int(bool(maps)),
                                   int(bool(exported)), ctypes.byref(out), inst)
    return out, tuple(inst)


def render_route(n_rays=640000, fields=False, maps=False, kind='decode', mlp_verified=False, occupancy=False, band_stale=False, capturing=False,
                 frame_fits=False):
    """hr_render_route of the facts given: (route name, tier, calibrate_first)."""
    out = (ctypes.c_int * 3)()
    plan_lib().hp_render_route(ctypes.c_longlong(n_rays), int(fields), int(maps), SAMPLE_KIND[kind], int(mlp_verified), int(occupancy), int(band_stale),
                               int(capturing), int(frame_fits), out)
    return {v: k for k, v in ROUTE.items()}[out[0]], out[1], out[2]


def frame_plan(hc, n_rays=640000, frame_mode=1, sample_waves=0, cascade=False, verified=False, split_mlp=True, frame_lines=False):
    """hr_frame_plan for a model of `hc` on 256 compute units with a split MLP arithmetic (HR_OPT_FRAME_KERNEL = frame_mode)."""
    out = FramePlan()
    plan_lib().hp_frame_plan(ctypes.byref(hc), ctypes.c_longlong(n_rays), frame_mode, sample_waves, int(bool(cascade)), int(bool(verified)),
                             int(bool(split_mlp)), int(bool(frame_lines)), ctypes.byref(out))
    return out


def frame_time_tap(hc, t):
    """hr_frame_time_tap: (i0, i1, w0, w1) of a frame at time t."""
    out = TimeTap()
    plan_lib().hp_frame_time_tap(ctypes.byref(hc), ctypes.c_float(t), ctypes.byref(out))
    return out.i0, out.i1, out.w0, out.w1


def mlp_choice(hc, act_max, cascade_level=False, range_supported=True):
    """hr_mlp_choice for a compiled config and the calibration's maxima (one per Linear; the rest 0):
    (active_precision, verified, needs_calibration, status)."""
    a, out = (ctypes.c_float * 8)(*act_max), (ctypes.c_int * 4)()
    plan_lib().hp_mlp_choice(ctypes.byref(hc), int(bool(cascade_level)), int(bool(range_supported)), a, out)
    return out[0], out[1], bool(out[2]), out[3]


def mlp_limits():
    """(HR_F16_CALIBRATION_LIMIT, HR_BAND_FLOOR, HR_VERIFY_LISTED_LIMIT, HR_VERIFY_RGB_LIMIT) as float32."""
    out = (ctypes.c_float * 4)()
    plan_lib().hp_mlp_limits(out)
    return tuple(np.float32(v) for v in out)


def calib_sample(n):
    """hr_calib_sample: (stride, rays kept) of n calibration rays handed over by the caller."""
    out = (ctypes.c_longlong * 2)()
    plan_lib().hp_calib_sample(n, out)
    return out[0], out[1]


def band_margins(d_zc, d_dist_n, d_geo_n, d_off):
    """hr_band_margins: (band, band_q, band_off) as float32 from the largest differences measured."""
    out = (ctypes.c_float * 3)()
    plan_lib().hp_band_margins(d_zc, d_dist_n, d_geo_n, d_off, out)
    return tuple(np.float32(v) for v in out)


def listed_frac(calibrated, n, n_used, listed):
    """hr_listed_frac: hr_verify_info::listed_frac (calibrated: 1 = synthetic rays, 2 = the caller's)."""
    return np.float32(plan_lib().hp_listed_frac(calibrated, n, n_used, listed))


def verify_fallback(frac, max_d_rgb):
    """hr_verify_fallback: 0 = the fast path stays, 1 = too many rays listed, 2 = the images are too far apart."""
    return plan_lib().hp_verify_fallback(frac, max_d_rgb)


def plane_geometry(hc):
    """hr_plane_geometry of a compiled config: (HrGridPlane[3] without texel pointers, ca_total, n_basis_cols, consistent)."""
    planes, ca, nb = (GridPlane * 3)(), ctypes.c_int(), ctypes.c_int()
    ok = plan_lib().hp_plane_geometry(ctypes.byref(hc), planes, ctypes.byref(ca), ctypes.byref(nb))
    return planes, ca.value, nb.value, bool(ok)


def train_plan(hc, n_rays=96, deterministic=False):
    """hr_train_plan for a backward step of n_rays rays on a model of `hc` whose tape has taps (what hr_train_backward provides)."""
    out = TrainPlan()
    plan_lib().hp_train_plan(ctypes.byref(hc), ctypes.c_longlong(n_rays), int(bool(deterministic)), ctypes.byref(out))
    return out


def train_branch(hc, n_rays=96, deterministic=False):
    """The kernels hr_launch_train (csrc/train_kernel.hip) picks for a compiled config -- for a cascade, its fine level --: what the
    library's own hr_train_plan (csrc/hr_plan.h, compiled for the host) answers, as a dict:
      zp               z_channels rounded up to a power of two (8 ... 256)
      thread_per_ray   phase A is hr_train_kernel<zp> (zp > 64: no taps on the tape), else hr_train_lanes_kernel<zp, nb, pc>
      rays_per_group   rays of one phase-A workgroup (lanes) or wavefront (thread per ray)
      plane_class      '8,4,4' | '8,0,0' | 'generic': hr_plane_class, the PC of the lanes kernel
      nb               the lanes kernel's NB (2: compiled for static nets only)
      video, keyed     keyframe net; phase B keeps two time-plane rows per pair (KEYED) instead of whole lines
      phase_b          'lines' (hr_train_gather_bwd_lines_kernel, window in LDS) | 'atomics' (hr_train_gather_bwd_kernel)
      phase_b_class    PC of the lines kernel ('generic' without taps)
      passes           lines kernel launches (2: pair 0, then pairs 1 + 2); 0 with 'atomics'
      lds_bytes        the largest dynamic LDS request of the lines kernel considered (cap: 150 KiB)
    The lines path also needs the runtime to grant the LDS request (hr_lds_opt_in), which a gfx950 workgroup's 160 KiB always does."""
    p = train_plan(hc, n_rays, deterministic)
    return dict(zp=p.zp, thread_per_ray=bool(p.thread_per_ray), rays_per_group=p.rays_per_group, plane_class=PLANE_CLASS[p.a_pc], nb=p.a_nb,
                video=bool(hc.video), keyed=bool(p.keyed), phase_b='lines' if p.lines else 'atomics', phase_b_class=PLANE_CLASS[p.b_pc],
                passes=p.passes, lds_bytes=p.lines_lds)


def build_host_lib(out, src, deps):
    """g++ -shared of a host restatement: the package's own builder (flock, atomic rename), at the -O1 the tests' restatements are held to"""
    return build_host_library(out, src, deps, opt='-O1')
