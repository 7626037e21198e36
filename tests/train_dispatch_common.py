"""Shared by tests/test_train_plan_host.py and tests/test_gpu_train_dispatch.py: one small case per branch hr_launch_train can take
(csrc/train_kernel.hip), the scenes behind the cases, and the check that a case lands on the branch its row claims -- answered by the
library's own hr_train_plan (csrc/hr_plan.h) through helpers.train_branch."""
import functools
from types import SimpleNamespace

import numpy as np

from helpers import Golden, train_branch
from hyperreel_amd import config as C
from hyperreel_amd import plan, scenes

# branch -> case.  Fixtures of tests/golden/sweep (94 to 96 rays on a 28 x 24 x 20 grid), then seeded scenes.  The expectations are what
# helpers.train_branch must report for the case: a later change to a fixture or to the dispatch must not silently empty a row.
LANES, PER_RAY = dict(thread_per_ray=False), dict(thread_per_ray=True)
BRANCH = {
    'shiny_z_plane_tiny': dict(LANES, zp=8, z=8, plane_class='8,4,4', nb=2, video=False, phase_b='lines', mlp=(128, 4)),
    'technicolor_z_plane_tiny': dict(LANES, zp=8, z=8, plane_class='8,0,0', nb=4, video=True, keyed=True, phase_b='lines'),
    'shiny_z_plane_small': dict(LANES, zp=16, z=16, plane_class='8,4,4', nb=2, video=False, phase_b='lines'),
    'stanford_z_plane_small': dict(LANES, zp=16, z=16, plane_class='8,0,0', nb=4, video=False, phase_b='lines'),
    'technicolor_z_plane_small': dict(LANES, zp=16, z=16, plane_class='8,0,0', nb=4, video=True, keyed=True, phase_b='lines'),
    'neural_3d_z_plane_world': dict(LANES, zp=64, z=48, plane_class='8,4,4', nb=4, video=True, keyed=True, phase_b='lines'),
    'catacaustics_z_plane': dict(LANES, zp=64, z=64, plane_class='8,0,0', nb=4, video=False, phase_b='lines'),
    'immersive_z_plane': dict(LANES, zp=32, z=32, plane_class='8,0,0', video=False, phase_b='lines', views=5),
    'catacaustics_voxel': dict(PER_RAY, zp=128, z=96, n_den=[8, 8, 8], video=False, phase_b='lines', phase_b_class='generic'),
    'technicolor_z_plane_no_sample': dict(PER_RAY, zp=128, z=128, video=True, keyed=True, phase_b='atomics', mlp=(0, 0)),
    'neural_3d_z_plane_static': dict(PER_RAY, zp=256, z=256, n_den=[8, 0, 0], video=False, phase_b='lines', phase_b_class='generic'),
    # cascades: coarse rows, point MLP, fine stage
    'shiny_z_plane_cascaded': dict(LANES, cascade=True, zp=32, plane_class='8,4,4', video=False, mlp=(0, 0)),
    'shiny_z_plane_feedback': dict(LANES, cascade=True, zp=32, plane_class='8,0,0', video=False),
    'shiny_z_tensorf_cascaded': dict(PER_RAY, cascade=True, zp=128, n_den=[8, 8, 8], video=False),
    'technicolor_cascaded': dict(LANES, cascade=True, zp=32, plane_class='8,0,0', video=True, keyed=True, phase_b='lines'),
    # no fixture has [8, 4, 4] above 64 samples, or a keyframe net whose small sample count is not a power of two
    'seeded_donerf_sphere_z96': dict(PER_RAY, zp=128, z=96, n_den=[8, 4, 4], video=False, phase_b='lines'),
    'seeded_donerf_cylinder_z200': dict(PER_RAY, zp=256, z=200, n_den=[8, 4, 4], video=False, phase_b='lines'),
    'seeded_technicolor_z_plane_z12': dict(LANES, zp=16, z=12, plane_class='8,0,0', video=True, keyed=True, phase_b='lines'),
    # the per-ray colour transforms on the thread-per-ray kernel (no fixture has one above 64 samples): the per-camera colour table, and
    # the 3x3 from the head (`color_transform_global`)
    'seeded_immersive_z_plane_z96': dict(PER_RAY, zp=128, z=96, video=False, phase_b='lines', views=5),
    'seeded_color_transform_global_head_z96': dict(PER_RAY, zp=128, z=96, video=False, phase_b='lines', head_matrix=True),
    # pair 0's line alone is 2400 texels x 16 channels x 4 B = 150 KiB, the cap of hr_launch_gather_bwd_lines: the default build's fall-back
    'lds_fallback': dict(LANES, zp=32, z=32, plane_class='8,4,4', video=False, phase_b='atomics', over_cap=True),
    # a keyframe net whose rows of all three pairs exceed the cap together (128 B x 1115 + 64 B x (24 + 20) + 8128 B = 153 664 B against
    # 153 600): pair 0 in one pass, pairs 1 + 2 in a second that adds to the point gradient of the first
    'two_pass': dict(LANES, zp=16, z=16, plane_class='8,4,4', nb=4, video=True, keyed=True, phase_b='lines', phase_b_class='8,4,4', passes=2),
}
TWO_PASS_N = 1115
# the rows the deterministic build is run on as well (64-bit fixed-point sums, the global-atomics kernel for everything)
DETERMINISTIC = ['shiny_z_plane_tiny', 'stanford_z_plane_small', 'catacaustics_voxel', 'neural_3d_z_plane_static', 'immersive_z_plane',
                 'technicolor_cascaded']
SEEDED = {'seeded_donerf_sphere_z96': ('donerf_sphere', 96), 'seeded_donerf_cylinder_z200': ('donerf_cylinder', 200),
          'seeded_technicolor_z_plane_z12': ('technicolor_z_plane', 12)}
# ... and from a fixture's config instead of a model YAML's, both z_channels keys set
SEEDED_FIXTURE = {'seeded_immersive_z_plane_z96': ('sweep/immersive_z_plane', 96),
                  'seeded_color_transform_global_head_z96': ('sweep/variant_color_transform_global_head', 96)}


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name in SEEDED:                                   # as tests/test_train_host.py::test_backward_at_other_sample_counts
        model, z = SEEDED[name]
        cfg, ds, grid = C.model_config(model, z_channels=z), C.dataset_scalars(model), [24, 20, 16]
        sd = scenes.make_state_dict(cfg, ds, grid, seed=4, density='dense', app_scale=1.0)
        video = cfg.color.net.type == 'tensor_vm_split_time'
        if 'z_plane' in model:
            rays = scenes.random_rays(48, 2, video, pos_mean=(0, 0, 1.0), pos_std=0.15, dir_mean=(0, 0, -1.2), dir_std=0.5)
        else:
            rays = scenes.random_rays(48, 2, video)
        return SimpleNamespace(cfg=cfg, dataset=ds, state_dict=sd, iteration=None, grid=grid, rays=np.ascontiguousarray(rays, np.float32))
    if name in SEEDED_FIXTURE:
        fixture, z = SEEDED_FIXTURE[name]
        g = Golden(fixture)
        cfg, ds, grid = g.cfg, g.dataset, [24, 20, 16]
        cfg.embedding.embeddings.ray_prediction_0.z_channels = cfg.embedding.embeddings.ray_intersect_0.z_channels = z
        sd = scenes.make_state_dict(cfg, ds, grid, seed=4, density='dense', app_scale=1.0)
        timed = g.rays.shape[1] > 6                      # camera id and time columns
        if 'z_plane' in fixture:
            rays = scenes.random_rays(48, 2, timed, pos_mean=(0, 0, 1.0), pos_std=0.15, dir_mean=(0, 0, -1.2), dir_std=0.5)
        else:
            rays = scenes.random_rays(48, 2, timed)
        if ds.get('val_all', False):                     # every camera of the colour table
            rays[:, 6] = np.arange(48) % ds['total_images_per_frame']
        return SimpleNamespace(cfg=cfg, dataset=ds, state_dict=sd, iteration=g.iteration, grid=grid, rays=np.ascontiguousarray(rays, np.float32))
    if name == 'lds_fallback':
        cfg, ds, grid = C.model_config('donerf_sphere'), C.dataset_scalars('donerf_sphere'), [12, 12, 2400]
        sd = scenes.make_state_dict(cfg, ds, grid, seed=4, density='dense', app_scale=1.0)
        # smooth lines: the fp32 rounding of a coordinate on a 1 / 2400 texel must not move the features
        for kind in ('density', 'app'):
            for j in range(3):
                key = f'model.color_model.net.{kind}_line.{j}'
                _, ch, n, _ = sd[key].shape
                u = (np.arange(n, dtype=np.float64) + 0.5) / n
                sd[key] = (0.5 + 0.4 * np.sin(2 * np.pi * 3 * u[None, :] + np.arange(ch)[:, None])).astype(np.float32).reshape(1, ch, n, 1)
        rays = scenes.random_rays(96, 2, False)
        return SimpleNamespace(cfg=cfg, dataset=ds, state_dict=sd, iteration=None, grid=grid, rays=np.ascontiguousarray(rays, np.float32))
    if name == 'two_pass':
        model, grid = 'neural_3d_z_plane', [24, 20, TWO_PASS_N]
        cfg, ds = C.model_config(model, z_channels=16), C.dataset_scalars(model)
        sd = scenes.make_state_dict(cfg, ds, grid, seed=4, density='dense', app_scale=1.0)
        # smooth along the long axis, as the lines of lds_fallback: every tensor that has it (space planes 1 and 2, time plane 0)
        for key in [k for k in sd if '_plane_' in k and TWO_PASS_N in sd[k].shape]:
            shape = sd[key].shape
            ax = shape.index(TWO_PASS_N)
            u = ((np.arange(TWO_PASS_N, dtype=np.float64) + 0.5) / TWO_PASS_N).reshape([-1 if i == ax else 1 for i in range(4)])
            ch = np.arange(shape[1], dtype=np.float64).reshape(1, -1, 1, 1)
            other = np.arange(shape[5 - ax], dtype=np.float64).reshape([-1 if i == 5 - ax else 1 for i in range(4)])
            sd[key] = (0.5 + 0.4 * np.sin(2 * np.pi * 3 * u + ch + 0.7 * other)).astype(np.float32)
        rays = scenes.random_rays(48, 2, True, pos_mean=(0, 0, 1.0), pos_std=0.15, dir_mean=(0, 0, -1.2), dir_std=0.5)
        return SimpleNamespace(cfg=cfg, dataset=ds, state_dict=sd, iteration=None, grid=grid, rays=np.ascontiguousarray(rays, np.float32))
    g = Golden('sweep/' + name)
    assert 94 <= g.rays.shape[0] <= 96 and list(g.grid) == [28, 24, 20], name
    return SimpleNamespace(cfg=g.cfg, dataset=g.dataset, state_dict=g.state_dict, iteration=g.iteration, grid=list(g.grid),
                           rays=np.ascontiguousarray(g.rays, np.float32))


def _levels(sc):
    return plan.compile_model(sc.cfg, sc.dataset, sc.grid, iteration=sc.iteration)


def _assert_branch(name, n_rays=None, deterministic=False):
    """The case lands on the branch its row claims."""
    sc = _scene(name)
    coarse, hc = _levels(sc)
    want = dict(BRANCH[name])
    got = train_branch(hc, sc.rays.shape[0] if n_rays is None else n_rays, deterministic=deterministic)
    assert (coarse is not None) == bool(want.pop('cascade', False)), name
    lvl0 = coarse if coarse is not None else hc
    if 'mlp' in want:
        assert (lvl0.mlp_hidden if lvl0.mlp_layers else 0, lvl0.mlp_layers) == want.pop('mlp'), name
    if 'z' in want:
        assert hc.z_channels == want.pop('z'), name
    if 'n_den' in want:
        assert list(hc.n_den) == want.pop('n_den'), name
    if 'views' in want:
        assert hc.color_table_views == want.pop('views'), name
    if want.pop('head_matrix', False):
        assert hc.f_color_scale_global.offset >= 0 and hc.f_color_scale_global.channels == 9, name
    if want.pop('over_cap', False):
        assert got['lds_bytes'] > 150 * 1024 and not got['keyed'], (name, got)
    if deterministic:                                    # train_det_kernel.hip: the global-atomics kernel for everything
        want['phase_b'] = 'atomics'
    for k, v in want.items():
        assert got[k] == v, (name, k, got)
    return got
