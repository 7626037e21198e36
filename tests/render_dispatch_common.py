"""Shared by tests/test_render_dispatch_host.py and tests/test_gpu_render_dispatch.py: one small case per instantiation of the render
sample stage's kernels (hr_sample_dispatch, csrc/hr_plan.h), the scenes and references behind the cases, and the check that a case lands
on the instantiation its row claims -- answered by the library's own hr_sample_form_plan through helpers.sample_form_plan.

  hr_sample_kernel / hr_sample_maps_kernel <ZP, HALF, PC, NB>    DECODE rows: 6 ZP x 2 HALF x 5 (PC, NB); a row claims both kernels
  hr_sample_time_kernel <ZP, HALF, PC, TD>                       TIME rows: 6 x 2 x 3 PC x TD {1, 3}
  hr_sample_shade_export_kernel / _import_kernel <ZP, HALF>      SHADE rows: ZP <= 64 x 2; a row claims both kernels

Every Z is no power of two (idle lanes, the sort's padding), 49 rays leave every workgroup but a one-ray one partly filled, and the
'dense' scene is thinned (scenes.scale_density) until the compositing weight reaches the last sample indices: at density 1 the first
quarter of the indices holds at least 0.88 of it and the back half none, so the second to fourth wavefronts of a ray above 64 samples
would compute nothing a comparison sees."""
import functools
from types import SimpleNamespace

import numpy as np

from helpers import SAMPLE_KIND, plan_lib, sample_form_plan, sample_plan
from hyperreel_amd import config as C
from hyperreel_amd import plan, scenes

Z_OF = {8: 7, 16: 12, 32: 24, 64: 48, 128: 96, 256: 200}          # ZP -> z_channels
DTYPE = ('fp32', 'fp16')                                           # HALF 0, 1
PAIRS = [(0, 4), (1, 2), (1, 4), (2, 2), (2, 4)]                   # (PC, NB): the generic gather has no line form
GRID, N_RAYS, SEED, RAY_SEED = [24, 20, 16], 49, 4, 2
DENSITY_SCALE = 0.1
ODD = dict(n_lamb_sigma=[5, 0, 3], n_lamb_sh=[9, 0, 2])            # no plane class: the generic gather on a keyframe net

# (PC, NB) -> (model, edits of color.net)
DECODE_RECIPE = {(0, 4): ('donerf_sphere', dict(n_lamb_sigma=[8, 8, 8], n_lamb_sh=[8, 8, 8])),
                 (1, 2): ('donerf_sphere', {}),
                 (1, 4): ('immersive_sphere', {}),
                 (2, 2): ('donerf_sphere', dict(n_lamb_sigma=[8, 0, 0], n_lamb_sh=[8, 0, 0])),
                 (2, 4): ('technicolor_z_plane', {})}
# TD 1, per PC: the recipes a row rotates through (model, shading, edits)
TIME_RECIPE = {0: [('technicolor_z_plane', 'RGBtLinear', ODD), ('technicolor_z_plane', 'RGBtFourier', ODD)],
               1: [('immersive_sphere', 'RGBtLinear', {}), ('donerf_sphere', 'RGBIdentity', {})],
               2: [('technicolor_z_plane', 'RGBtFourier', {})]}
# TD 3, per PC: the model; the shading and the density mode rotate (RGBIdentity exists on the static net only, which has no density mode:
# it appears under TD 1)
DENSITY_MODEL = {0: ('technicolor_z_plane', ODD), 1: ('immersive_sphere', {}), 2: ('technicolor_z_plane', {})}
DENSITY_SHADING = ['RGB', 'SH', 'RGBtLinear', 'RGBtFourier']
DENSITY_MODE = ['DensityFourier', 'DensityLinear']

# A density mode's pre-activation is sum_j basis_j(t) (basis_mat_density . components)_j: on a 'dense' scene (components > 0) its sign over most of
# the volume is the luck of the seed's basis_mat_density, and relu empties the rest.  Per row, the factor of scenes.scale_density -- a negative one
# turns the sign -- from the ladder +-(0.1 0.2 0.3 0.5 1 2 4) that spreads the reference's weights best (tests/test_render_dispatch_host.py holds
# every row to the conditions).  z_channels -> (fp32 PC 0, 1, 2, fp16 PC 0, 1, 2)
DENSITY_MODE_SCALE = {
    7: (-2.0, 1.0, 4.0, -4.0, -4.0, 2.0),
    12: (-1.0, 2.0, -0.5, -2.0, 4.0, 2.0),
    24: (-4.0, 1.0, -1.0, -1.0, 4.0, -4.0),
    48: (-0.5, 1.0, -4.0, -2.0, 1.0, -0.5),
    96: (-2.0, -4.0, 0.5, -1.0, 0.5, 1.0),
    200: (2.0, 1.0, -1.0, -2.0, 1.0, 2.0),
}


def _rows():
    rows, n_den = {}, 0
    for zi, (zp, z) in enumerate(Z_OF.items()):
        for half, dt in enumerate(DTYPE):
            n_time = zi + half                           # both texel formats and every sample count meet every recipe of a class
            for pc, nb in PAIRS:
                model, edits = DECODE_RECIPE[(pc, nb)]
                rows[f'decode_z{z}_{dt}_pc{pc}_nb{nb}'] = dict(kind='decode', inst=(zp, half, pc, nb), model=model, z=z, edits=edits)
            for pc in (0, 1, 2):
                model, shading, edits = TIME_RECIPE[pc][n_time % len(TIME_RECIPE[pc])]
                rows[f'time_z{z}_{dt}_pc{pc}_td1'] = dict(kind='time', inst=(zp, half, pc, 1), model=model, z=z, edits=edits, shading=shading)
                model, edits = DENSITY_MODEL[pc]
                rows[f'time_z{z}_{dt}_pc{pc}_td3'] = dict(kind='time_density', inst=(zp, half, pc, 3), model=model, z=z, edits=edits,
                                                          shading=DENSITY_SHADING[n_den % 4], density_mode=DENSITY_MODE[(n_den // 4 + n_den) % 2],
                                                          density_scale=DENSITY_MODE_SCALE[z][3 * half + pc])
                n_den += 1
            if zp <= 64:
                rows[f'shade_z{z}_{dt}'] = dict(kind='shade', inst=(zp, half), model='donerf_sphere', z=z, edits={},
                                                shading='MLP' if (half + zi) % 2 else 'MLP_Fea')
    return rows


ROWS = _rows()
KINDS = ('decode', 'time', 'time_density', 'shade')


def rows_of(*kinds):
    return [n for n, r in ROWS.items() if r['kind'] in kinds]


def compiled_sets():
    """The instantiations the library compiles, from the rule stated in csrc/hr_plan.h (hr_sample_dispatch and the launchers' `if constexpr`):
    the five (PC, NB) pairs per ZP and texel format; NB 4 only for the time kernel, per TD; PC 0 / NB 4 and ZP <= 64 for the shade kernels."""
    base = [(zp, h, pc, nb) for zp in Z_OF for h in (0, 1) for pc, nb in PAIRS]
    shade = [(zp, h) for zp, h, pc, nb in base if (pc, nb) == (0, 4) and zp <= 64]
    return {'hr_sample_kernel': set(base), 'hr_sample_maps_kernel': set(base),
            'hr_sample_time_kernel': {(zp, h, pc, td) for zp, h, pc, nb in base if nb == 4 for td in (1, 3)},
            'hr_sample_shade_export_kernel': set(shade), 'hr_sample_shade_import_kernel': set(shade)}


def claimed_sets():
    out = {k: set() for k in compiled_sets()}
    for name, r in ROWS.items():
        kernels = {'decode': ('hr_sample_kernel', 'hr_sample_maps_kernel'), 'time': ('hr_sample_time_kernel',), 'time_density': ('hr_sample_time_kernel',),
                   'shade': ('hr_sample_shade_export_kernel', 'hr_sample_shade_import_kernel')}[r['kind']]
        for k in kernels:
            assert r['inst'] not in out[k], name                  # one row per instantiation
            out[k].add(r['inst'])
    return out


def round_grids_to_half(sd):
    from test_gpu_parity import _round_grids_to_half
    return _round_grids_to_half(sd)


@functools.lru_cache(maxsize=None)
def _scene_of(model, z, edits, shading, density_mode, density_scale):
    cfg, ds = C.model_config(model, z_channels=z, shading=shading, density_mode=density_mode), C.dataset_scalars(model)
    cfg.color.net.update({k: list(v) for k, v in edits})
    sd = scenes.scale_density(scenes.make_state_dict(cfg, ds, GRID, seed=SEED, density='dense', app_scale=1.0), density_scale)
    video = cfg.color.net.type == 'tensor_vm_split_time'
    if 'z_plane' in model:                               # as tests/train_dispatch_common.py::_scene
        rays = scenes.random_rays(N_RAYS, RAY_SEED, video, pos_mean=(0, 0, 1.0), pos_std=0.15, dir_mean=(0, 0, -1.2), dir_std=0.5)
    else:
        rays = scenes.random_rays(N_RAYS, RAY_SEED, video)
    return SimpleNamespace(cfg=cfg, dataset=ds, state_dict=sd, grid=GRID, video=video, rays=np.ascontiguousarray(rays, np.float32))


def _key(r):
    return r['model'], r['z'], tuple(sorted((k, tuple(v)) for k, v in r['edits'].items())), r.get('shading'), r.get('density_mode'), r.get('density_scale', DENSITY_SCALE)


def scene(name):
    """The row's model and seeded scene (shared by the rows of both texel formats) and its 49 rays."""
    return _scene_of(*_key(ROWS[name]))


def level(name):
    """The row's compiled config: its texel format, the float32 MLP (the head is the oracle's chain; the call renders launch by launch)."""
    sc = scene(name)
    return plan.compile_model(sc.cfg, sc.dataset, sc.grid, grid_dtype=DTYPE[ROWS[name]['inst'][1]], mlp_precision='fp32')[1]


@functools.lru_cache(maxsize=None)
def _reference_of(key, kind, half):
    sc = _scene_of(*key)
    sd = round_grids_to_half(sc.state_dict) if half else sc.state_dict
    if kind == 'decode':
        import os
        import sys
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'oracle'))
        from hyperreel_oracle import HyperReelOracle
        ref = HyperReelOracle(sc.cfg, sc.dataset, sd).render(sc.rays, keep='all')
        out = {k: np.asarray(ref[k]) for k in ('rgb', 'render_weights', 'distances')}
    elif kind == 'shade':
        from shading_oracle import shade_port
        out = shade_port(sc.cfg, sc.dataset, sd).fields(sc.rays)
    else:
        from time_decode_oracle import time_port
        out = time_port(sc.cfg, sc.dataset, sd).fields(sc.rays)
    out['distances'] = out['distances'].reshape(out['render_weights'].shape)
    for v in out.values():
        v.setflags(write=False)
    return out


def reference(name, half=None):
    """{'rgb', 'render_weights', 'distances'} of the row's scene from the reference restatement of its kind, computed once and read-only:
    HyperReelOracle (decode), time_decode_oracle.time_port (time), shading_oracle.shade_port (shade).  A float16 row's scene is the
    half-rounded one; half=False asks for the float32 scene's all the same."""
    r = ROWS[name]
    return _reference_of(_key(r), r['kind'], bool(r['inst'][1]) if half is None else bool(half))


def assert_instantiation(name):
    """The row lands on the instantiation it claims, in every form its kernels are launched in."""
    r, hc = ROWS[name], level(name)
    kind = r['kind']
    td = hc.time_decode
    got_kind = plan_lib().hp_sample_kind(hc.shading, int(td is not None and td.density_mode != 0))
    assert got_kind == SAMPLE_KIND[kind], (name, got_kind)
    assert hc.z_channels == r['z'] and hc.mlp_precision == plan.MLP_PRECISION['fp32'], name
    if kind == 'decode':
        assert sample_plan(hc, N_RAYS)[1] == r['inst'], (name, sample_plan(hc, N_RAYS)[1])
        for maps in (False, True):
            assert sample_form_plan(hc, kind, N_RAYS, maps=maps)[1] == r['inst'], (name, maps)
    elif kind == 'shade':
        zp, half = r['inst']
        assert zp <= 64
        for form in (dict(exported=True), dict(maps=True)):
            assert sample_form_plan(hc, kind, N_RAYS, **form)[1] == (zp, half, 0, 4), (name, form)
    else:
        zp, half, pc, tdv = r['inst']
        assert tdv == (3 if kind == 'time_density' else 1)
        assert sample_form_plan(hc, kind, N_RAYS, maps=True)[1] == (zp, half, pc, 4), (name, sample_form_plan(hc, kind, N_RAYS, maps=True)[1])
    return hc


def workgroup_edge(name):
    """A ray index at a workgroup's edge: the last ray of the first workgroup that has a successor (256 / ZP rays per workgroup)."""
    rpb = 256 // ROWS[name]['inst'][0]
    return rpb - 1 if rpb > 1 else 24
