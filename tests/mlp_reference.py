"""The sample-prediction MLP (K1) on its own terms: a float64 evaluation of BaseMLP.forward (nlf/nets/mlp.py:159-172, restated in
oracle/hyperreel_oracle.py:_run_mlp -- cat([input, x]) on skip layers, LeakyReLU with slope float32(0.01)) from the fp32 features the
oracle's _param_pe(rays) returns.  numpy / torch CPU only: tests/test_mlp_reference_host.py checks it without a GPU,
tests/test_gpu_mlp_structure.py holds the kernels to it.

Three forms, each a rounding rule for the weights and one for the layer inputs:
  exact       no rounding
  stored(a)   the weights are what arithmetic `a` keeps of them -- the rules of csrc/hr_mlp_pack.h restated with torch's CPU casts, never
              read back from the packer: v = w * 2^s, s = 14 - exponent(max |w| of the layer) clamped to [-14, 40] (exact, undone
              afterwards; 0 for bf16x3 / fp32); f16x3 keeps f16(v) + f16(v - f16(v)), bf16x3 the same with bf16 halves, f16x2 f16(v)
              alone, f16f8 f16(v) + e4m3((v - f16(v)) * 64) / 64 on the hidden k-steps (hr_pack_kseg) and both f16 halves on the input
              k-steps, fp32 v.  Layer inputs unrounded.
  dropped(a)  stored(a) with every layer input rounded to ONE element of the arithmetic (f16, bf16): a kernel whose activation-side
              correction product is gone -- the smallest wrong kernel the tolerances must catch.

The unit of error is max |delta| / max |reference| over the live head columns of every ray.  Tolerances come from the reference alone:
  E_ref32 = |fp32 numpy chain - exact|, E_drop(a) = |dropped(a) - stored(a)|
  T(fp32) = 8 E_ref32;  T(f16x3, bf16x3, f16x2) = E_drop / 64 + 8 E_ref32;  T(f16f8) = E_drop / 4 + 8 E_ref32
(two correct fp32 summation orders differ by a few E_ref32; a three-product kernel differs from stored(a) by truncating its inputs to two
halves and by fp32 accumulation; f16f8's correction products carry e4m3's four significant bits, ~16 x under E_drop; a lost correction is
at least E_drop / sqrt 2).
T(f16f8) was E_drop / 8 and is E_drop / 4 for a cause that is not the kernels' arithmetic: the fp8 images of a layer's output are scaled
from the CALIBRATION's largest activation of that layer (hr_f8_exponent, 16 x headroom), and e4m3 keeps four significant bits over the 15
octaves below that only.  hr_model_finalize calibrates on synthetic rays with uniformly random directions; with a two-plane
parameterisation whose coordinates reach the MLP as they are (mlp_in 4, 12, 20: identity columns), the synthetic rays that graze the
planes put the calibrated maxima ~1000 x above what rays towards the planes produce, their images fall into e4m3's subnormals and the
correction product x8 w_lo8 keeps one or two bits: 1.04 - 1.25 of E_drop / 8 + 8 E_ref32 on those cases, 0.29 - 0.33 of it on the same
rays once hr_model_calibrate has seen them (every other case: 0.25 - 0.34 either way).  Case.tight_f16f8 is the bound after calibration.

A case is a config, a state dict from scenes.make_state_dict on a tiny grid and 193 rays (three 64-ray tiles and one ray)."""
import contextlib
import functools

import numpy as np
import torch

from helpers import live_columns
from hyperreel_amd import config as C
from hyperreel_amd import plan, scenes

F32, F64 = np.float32, np.float64
ARITHMETICS = ('fp32', 'bf16x3', 'f16x3', 'f16x2', 'f16f8')
SPLIT = ARITHMETICS[1:]
GRID_SIZE = [9, 8, 7]
N_RAYS = 193
SLOPE = F64(F32(0.01))
EMB = scenes.EMB


@contextlib.contextmanager
def one_thread():
    """The matrices here are small: thread pools of numpy's BLAS and of torch that size themselves by the machine's cores spend their time
    waiting for each other (a factor 15 on these chains).  Restored on exit."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        try:
            from threadpoolctl import threadpool_limits
        except ImportError:
            yield
            return
        with threadpool_limits(limits=1):
            yield
    finally:
        torch.set_num_threads(n)


# ---------------------------------------------------------------- roundings
def _t32(x):
    return torch.from_numpy(np.ascontiguousarray(x, F32))


def round_to(x, dtype):
    """float64 array rounded once (to nearest even) to one element of `dtype`, back as float64"""
    return torch.from_numpy(np.ascontiguousarray(x, F64)).to(dtype).double().numpy()


def element_type(a):
    return torch.bfloat16 if a == 'bf16x3' else torch.float16


def two_halves(x, dtype):
    """(hi, lo) = (r(x), r(x - r(x))) of fp32 values, as float64"""
    v = _t32(x)
    hi = v.to(dtype)
    lo = (v - hi.float()).to(dtype)
    return hi.double().numpy(), lo.double().numpy()


def four_bits(x):
    """x rounded to four significant bits (e4m3's, inside its block-scaled range)"""
    m, e = np.frexp(np.asarray(x, F64))
    return np.ldexp(np.round(m * 16.0) / 16.0, e)


def weight_shift(w):
    """s of the fp16 modes' packed weights w * 2^s (hr_weight_shift): the layer's largest |w| lands in [2^13, 2^14)"""
    mx = float(np.abs(w).max()) if w.size else 0.0
    if not (mx > 0.0 and np.isfinite(mx)):
        return 0
    return min(40, max(-14, 14 - int(np.frexp(mx)[1])))


def stored_parts(w, a, n_input_cols):
    """What arithmetic `a` keeps of a layer's torch matrix w (out, in), in the packed unit: (s, hi, lo) as float64 with
    stored = (hi + lo) * 2^-s.  n_input_cols: the leading columns that are input features (the whole first layer, the cat'ed input of a
    skip layer) -- f16f8 keeps both f16 halves there and the fp8 image of the residual on the hidden columns."""
    w = np.ascontiguousarray(w, F32)
    if a == 'fp32':
        return 0, w.astype(F64), np.zeros(w.shape, F64)
    if a == 'bf16x3':
        hi, lo = two_halves(w, torch.bfloat16)
        return 0, hi, lo
    s = weight_shift(w)
    v = _t32(w) * F32(2.0 ** s)
    hi = v.half()
    res = v - hi.float()
    if a == 'f16x2':
        lo = torch.zeros_like(res).double()
    elif a == 'f16x3':
        lo = res.half().double()
    elif a == 'f16f8':
        lo = torch.clamp(res * 64.0, -448.0, 448.0).to(torch.float8_e4m3fn).double() / 64.0
        lo[:, :n_input_cols] = res.half().double()[:, :n_input_cols]
    else:
        raise KeyError(a)
    return s, hi.double().numpy(), lo.numpy()


def stored_weights(w, a, n_input_cols):
    s, hi, lo = stored_parts(w, a, n_input_cols)
    return (hi + lo) * 2.0 ** -s


# ---------------------------------------------------------------- the chain
def chain(features, layers, skips, weights, inputs=None):
    """BaseMLP.forward in float64.  weights(w, n_input_cols) -> the (out, in) matrix used; inputs(x): rounding of every layer input."""
    inp = x = np.asarray(features, F64)
    for i, (w, b) in enumerate(layers):
        if i in skips:
            x = np.concatenate([inp, x], -1)
        n_input_cols = x.shape[1] if i == 0 else (inp.shape[1] if i in skips else 0)
        xin = x if inputs is None else inputs(x)
        x = xin @ weights(w, n_input_cols).T + np.asarray(b, F64)
        if i < len(layers) - 1:
            x = np.where(x >= 0, x, x * SLOPE)
    return x


def chain32(features, layers, skips):
    """the fp32 numpy chain (a peer of the kernels, not a reference): oracle/hyperreel_oracle.py:_run_mlp"""
    from hyperreel_oracle import HyperReelOracle
    return HyperReelOracle._run_mlp(np.asarray(features, F32), len(layers) - 2, list(skips), layers)


def model(features, layers, skips, a):
    """A numpy model of arithmetic `a` as the kernels run it: fp32 activations split into two halves, the products the kernel issues
    (hi hi + hi lo + lo hi; f16x2 without the weights' low half; f16f8 with four-bit operands in the two correction products of the hidden
    k-steps), summed in fp32 from the scaled bias, times 2^-s."""
    if a == 'fp32':
        return chain32(features, layers, skips).astype(F64)
    dt = element_type(a)
    inp = x = np.asarray(features, F32)
    for i, (w, b) in enumerate(layers):
        if i in skips:
            x = np.concatenate([inp, x], -1)
        k_in = x.shape[1] if i == 0 else (inp.shape[1] if i in skips else 0)
        s, wh, wl = stored_parts(w, a, k_in)
        xh, xl = two_halves(x, dt)
        f = lambda m: m.astype(F32)
        acc = f(xh) @ f(wh).T + f(np.asarray(b, F64) * 2.0 ** s)
        if a == 'f16f8':
            acc = acc + f(xh[:, :k_in]) @ f(wl[:, :k_in]).T + f(xl[:, :k_in]) @ f(wh[:, :k_in]).T
            acc = acc + f(four_bits(x[:, k_in:])) @ f(wl[:, k_in:]).T + f(four_bits(xl[:, k_in:])) @ f(four_bits(wh[:, k_in:])).T
        else:
            acc = acc + f(xh) @ f(wl).T + f(xl) @ f(wh).T
        x = (acc * F32(2.0 ** -s)).astype(F32)
        if i < len(layers) - 1:
            x = np.maximum(x, x * F32(0.01)).astype(F32)
    return x.astype(F64)


def err(x, ref, mask=None):
    """max |x - ref| / max |ref| over the columns of `mask`"""
    x, ref = np.asarray(x, F64), np.asarray(ref, F64)
    if mask is not None:
        x, ref = x[:, mask], ref[:, mask]
    return float(np.abs(x - ref).max() / np.abs(ref).max())


# ---------------------------------------------------------------- a case
class Case:
    """A config, its dataset scalars, a state dict on the tiny grid and rays; the references and tolerances, computed once."""

    def __init__(self, name, cfg, dataset, rays, mlp='default', seed=11, sd=None):
        self.name, self.cfg, self.dataset, self.mlp = name, cfg, dataset, mlp
        self.rays = np.ascontiguousarray(rays, F32)
        self.sd = sd if sd is not None else scenes.make_state_dict(cfg, dataset, GRID_SIZE, seed=seed, density='dense', app_scale=1.0, mlp=mlp)
        pred = cfg['embedding']['embeddings']['ray_prediction_0']
        self.hidden = int(pred['net']['hidden_channels'])
        self.depth = int(pred['net']['depth'])
        self.skips = [s for s in pred['net'].get('skips', []) if 0 < s < self.depth]
        self.arithmetics = ARITHMETICS if self.hidden == 256 else ('fp32',)
        self._cache = {}

    def _memo(self, key, make):
        if key not in self._cache:
            with one_thread():
                self._cache[key] = make()
        return self._cache[key]

    @property
    def oracle(self):
        from hyperreel_oracle import HyperReelOracle
        return self._memo('oracle', lambda: HyperReelOracle(self.cfg, self.dataset, self.sd))

    @property
    def layers(self):
        return self.oracle.layers

    @property
    def features(self):
        """the fp32 features the oracle's _param_pe returns: where the kernels' own operation starts"""
        return self._memo('features', lambda: self.oracle._param_pe(self.rays))

    def hc(self, precision='fp32'):
        return plan.compile_config(self.cfg, self.dataset, GRID_SIZE, mlp_precision=precision)

    def live_mask(self, prune=True):
        """booleans over the Z * P_user head columns of a ray: the ones the path computes"""
        def make():
            hc = self.hc()
            col = live_columns(hc, prune)[0][:hc.preds_per_z]
            return np.tile(np.asarray([c >= 0 for c in col]), hc.z_channels)
        return self._memo(('live', bool(prune)), make)

    def exact(self):
        return self._memo('exact', lambda: chain(self.features, self.layers, self.skips, lambda w, k: np.asarray(w, F64)))

    def stored(self, a):
        return self._memo(('stored', a), lambda: chain(self.features, self.layers, self.skips, lambda w, k: stored_weights(w, a, k)))

    def dropped(self, a):
        dt = element_type(a)
        return self._memo(('dropped', a), lambda: chain(self.features, self.layers, self.skips, lambda w, k: stored_weights(w, a, k),
                                                        inputs=lambda x: round_to(x, dt)))

    def chain32(self):
        return self._memo('chain32', lambda: chain32(self.features, self.layers, self.skips))

    def model(self, a):
        return self._memo(('model', a), lambda: model(self.features, self.layers, self.skips, a))

    def e_ref32(self, prune=True):
        return err(self.chain32(), self.exact(), self.live_mask(prune))

    def e_drop(self, a, prune=True):
        return err(self.dropped(a), self.stored(a), self.live_mask(prune))

    def tolerance(self, a, prune=True):
        if a == 'fp32':
            return 8.0 * self.e_ref32(prune)
        return self.e_drop(a, prune) / (4.0 if a == 'f16f8' else 64.0) + 8.0 * self.e_ref32(prune)

    def tight_f16f8(self, prune=True):
        """f16f8 with fp8 exponents calibrated on the case's own rays (hr_model_calibrate): E_drop / 8 + 8 E_ref32"""
        return self.e_drop('f16f8', prune) / 8.0 + 8.0 * self.e_ref32(prune)


# ---------------------------------------------------------------- the structure grid
def _pred(cfg):
    return cfg.embedding.embeddings.ray_prediction_0


def _net(cfg, **kw):
    _pred(cfg).net.update(**kw)


def _ray_param(cfg, param, pe):
    g = _pred(cfg).params.ray
    g['param'] = C.to_cfg(param)
    if pe is None:
        g.pop('pe', None)
    else:
        g['pe'] = C.to_cfg(pe)


def _windowed(n, exclude=False, mult=2.0):
    return {'type': 'windowed', 'freq_multiplier': mult, 'n_freqs': n, 'wait_iters': 0, 'max_freq_epoch': 0, 'exclude_identity': exclude}


_TWO_PLANE = {'n_dims': 4, 'fn': 'two_plane'}
_PLUECKER = {'n_dims': 6, 'fn': 'pluecker', 'direction_multiplier': 1.0, 'moment_multiplier': 1.0}

# name: (base model, z_channels or None, edit(cfg), rays kind, expected mlp_in).  One factor at a time around DoNeRF's static net:
# depth 6, skip [3], mlp_in 18 (Pluecker, one windowed frequency), Z = 32 with 11 live head columns = 352 = exactly 11 tiles.
STRUCTURES = {
    'base': ('donerf_sphere', None, lambda c: None, 'ball', 18),
    # depth: no hidden-to-hidden layer / exactly one / HR_MAX_LAYERS
    'depth2': ('donerf_sphere', None, lambda c: _net(c, depth=2, skips=[]), 'ball', 18),
    'depth3': ('donerf_sphere', None, lambda c: _net(c, depth=3, skips=[1]), 'ball', 18),
    'depth8': ('donerf_sphere', None, lambda c: _net(c, depth=8), 'ball', 18),
    # skips: none / into layer 1 / into the last Linear / into every layer at HR_MAX_LAYERS
    'skips_none': ('donerf_sphere', None, lambda c: _net(c, skips=[]), 'ball', 18),
    'skip_1': ('donerf_sphere', None, lambda c: _net(c, skips=[1]), 'ball', 18),
    'skip_last': ('donerf_sphere', None, lambda c: _net(c, skips=[5]), 'ball', 18),
    'skips_all_depth8': ('donerf_sphere', None, lambda c: _net(c, depth=8, skips=[1, 2, 3, 4, 5, 6, 7]), 'ball', 18),
    # mlp_in: k0p is padded to a multiple of 16 -- 4 and 12 under one k-step, 16 exactly one, 20 one over, 64 the maximum
    'in4': ('donerf_sphere', None, lambda c: _ray_param(c, _TWO_PLANE, None), 'front', 4),
    'in12': ('donerf_sphere', None, lambda c: _ray_param(c, _TWO_PLANE, _windowed(1)), 'front', 12),
    'in16': ('donerf_sphere', None, lambda c: _ray_param(c, _TWO_PLANE, _windowed(2, exclude=True)), 'front', 16),
    'in20': ('donerf_sphere', None, lambda c: _ray_param(c, _TWO_PLANE, _windowed(2)), 'front', 20),
    'in64': ('donerf_sphere', None, lambda c: _ray_param(c, _TWO_PLANE, _windowed(8, exclude=True, mult=1.4)), 'front', 64),
    'basic_pe': ('donerf_sphere', None, lambda c: _ray_param(c, _PLUECKER, {'type': 'basic', 'n_freqs': 2, 'freq_multiplier': 2.0}), 'ball', 30),
    # n_out = Z * P_live: under one 32-column tile / 12 tiles / 12 tiles and one column / the keyframe family's 960 columns, whose
    # second parameter group is the time column (mlp_in 18 + 5)
    'out_22': ('donerf_sphere', 2, lambda c: None, 'ball', 18),
    'out_374': ('donerf_sphere', 34, lambda c: None, 'ball', 18),
    'out_385': ('donerf_sphere', 35, lambda c: None, 'ball', 18),
    'out_960_time_group': ('neural_3d_z_plane', None, lambda c: None, 'front_video', 23),
    # the exact-fp32 kernel's other widths, with a skip
    'width64': ('donerf_sphere', None, lambda c: _net(c, hidden_channels=64), 'ball', 18),
    'width128': ('donerf_sphere', None, lambda c: _net(c, hidden_channels=128), 'ball', 18),
    # the windowed encoding's largest frequency at the f16f8 kernels' limit (2^4 = 16, hr_mlp_fast_sincos_ok) and beyond it (2^8), on
    # coordinates of order 3: arguments of ~48 and ~768 rad.  (Eight frequencies on Pluecker's six coordinates would be 96 features,
    # beyond HR_MAX_MLP_IN = 64: the case beyond the limit is the two-plane group's four coordinates, 64 features, on rays whose plane
    # coordinates are of order 3 -- the same arguments.)
    'pe_limit_16': ('donerf_sphere', None, lambda c: _ray_param(c, _PLUECKER, _windowed(4)), 'far_ball', 54),
    'pe_beyond_256': ('donerf_sphere', None, lambda c: _ray_param(c, _TWO_PLANE, _windowed(8, exclude=True)), 'far_front', 64),
}
GRID = [n for n in STRUCTURES if not n.startswith(('width', 'pe_'))]
WIDTHS = ['width64', 'width128']
N_OUT = ['out_22', 'base', 'out_374', 'out_385', 'out_960_time_group']      # the cases that run again with HR_PRUNE=0 (both column maps)
INITS = ['default', 'hostile']


def _rays(kind, n=N_RAYS):
    if kind == 'ball':
        return scenes.random_rays(n, 17)
    if kind == 'far_ball':              # origins ~3 from the centre: Pluecker moments of order 3
        return scenes.random_rays(n, 19, pos_mean=(2.2, -1.5, 1.5), pos_std=0.2)
    front = dict(pos_mean=(0.0, 0.0, 1.0), pos_std=0.15, dir_mean=(0.0, 0.0, -1.2), dir_std=0.3)
    if kind == 'front':
        return scenes.random_rays(n, 18, **front)
    if kind == 'front_video':
        return scenes.random_rays(n, 18, True, **dict(front, dir_std=0.5))
    if kind == 'far_front':             # two-plane coordinates of order 3
        return scenes.random_rays(n, 20, **dict(front, pos_mean=(3.0, -2.5, 1.0), pos_std=0.3))
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def get_case(name, init='default'):
    base, z, edit, kind, mlp_in = STRUCTURES[name]
    cfg = C.model_config(base, z_channels=z)
    edit(cfg)
    case = Case(f'{name}-{init}', cfg, C.dataset_scalars(base), _rays(kind), mlp=init)
    assert case.features.shape == (N_RAYS, mlp_in), (name, case.features.shape)
    return case


# ---------------------------------------------------------------- the exact cases
EXACT_DEPTHS = (2, 6, 8)
EXACT_SKIPS = ('none', 'three', 'all')


def _draw(shape, seed, high):
    return np.random.default_rng(seed).integers(0, high, size=shape)


@functools.lru_cache(maxsize=None)
def get_exact_case(depth, skips):
    """Inputs no arithmetic rounds: identity parameterisation without PE (the features are the ray columns, integers 0..3), every weight
    row two entries of 1 at columns drawn per (layer, row), biases 0 or 1.  Every pre-activation is a non-negative integer (LeakyReLU
    is the identity) of at most 4 * 2^depth - 1 <= 1023: one f16, two bf16 halves; every low half of a weight and every fp8 image of a
    residual is 0; the fp32 accumulators (at most 2^10 * 2^14 in the packed unit) are exact."""
    sk = {'none': [], 'three': [3], 'all': list(range(1, depth))}[skips]
    cfg = C.model_config('donerf_sphere')
    _net(cfg, depth=depth, skips=sk)
    _ray_param(cfg, {'n_dims': 6, 'fn': 'identity'}, None)
    ds = C.dataset_scalars('donerf_sphere')
    sd = scenes.make_state_dict(cfg, ds, GRID_SIZE, seed=5, density='dense', app_scale=1.0)
    for i, (n_out, n_in) in enumerate(scenes.mlp_layer_shapes(cfg)):
        mid = '.0' if i < depth - 1 else ''
        w = np.zeros((n_out, n_in), F32)
        first = _draw(n_out, 1000 + 10 * i, n_in)
        second = (first + 1 + _draw(n_out, 1001 + 10 * i, n_in - 1)) % n_in        # a different column
        w[np.arange(n_out), first] = 1.0
        w[np.arange(n_out), second] = 1.0
        sd[f'{EMB}0.net.layers.{i}{mid}.weight'] = w
        sd[f'{EMB}0.net.layers.{i}{mid}.bias'] = _draw(n_out, 1002 + 10 * i, 2).astype(F32)
    rays = np.concatenate([_draw((N_RAYS, 3), 7, 4), 1 + _draw((N_RAYS, 3), 8, 3)], -1).astype(F32)
    return Case(f'exact-depth{depth}-{skips}', cfg, ds, rays, sd=sd)


def exact_precondition(case):
    """Every layer input and pre-activation of the case, as the float64 chain sees them: (all are non-negative integers, the largest)."""
    seen = []

    def spy(x):
        seen.append(x)
        return x
    seen.append(chain(case.features, case.layers, case.skips, lambda w, k: np.asarray(w, F64), inputs=spy))
    ok = all((v >= 0).all() and np.array_equal(v, np.round(v)) for v in seen)
    return ok, max(float(v.max()) for v in seen)

