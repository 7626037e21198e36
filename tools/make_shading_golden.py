"""Generates tests/golden/shading/*.npz for the MLP shading modes (shadingMode MLP_Fea / MLP) by running the REFERENCE ITSELF
(imported in-process through oracle/refgen/ref_shim.py) on seeded inputs.  Run where the reference tree exists:

    python tools/make_shading_golden.py [name ...]

TEST INFRASTRUCTURE ONLY.  Two kinds of file:

  whole-model  a shipped model YAML plus an edit (CASES), the reference built from it on a 28 x 24 x 20 grid and loaded with
               scenes.make_state_dict's seeded scene emptied over the lower half of the x axis (scenes.carve_half_space: rays that stay
               there have no live sample), run on the sweep's rays, 26 more random ones and 8 that stay on one side (130 in all).
               Stored: rays, the reference's rgb and render_weights, rgb64 (the same model on a float64 copy: how far one correct
               float32 evaluation lies from the exact value) and the recipe in the sweep fixtures' format -- the scene is regenerated
               from the seed (`checksum` pins it; `density_scale` and `carve_x` repeat what was done to it).
  unit_*       the reference's MLPRender_Fea / MLPRender module alone on 300 seeded (f, v) rows, |f| up to 4: f, v, the module's
               state_dict, rgb (float32) and rgb64.

The conditions tests/test_gpu_shade*.py rely on are asserted here when a file is written and again by the tests (check_whole,
check_unit): no NaN, at least half of the channels in (0.05, 0.95), a ray without and a ray with only live samples, the live fraction of the 1e-3 threshold case in (0.1, 0.9),
max |rgb32 - rgb64| <= 2.5e-5 for whole models."""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'oracle', 'refgen'))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, 'tests', 'golden', 'shading')
GRID = [28, 24, 20]


def _net(cfg):
    return cfg.color.net


def _mlp(mode, **kw):
    def edit(cfg):
        n = _net(cfg)
        n.shadingMode = mode
        n.data_dim_color = 27
        for k, v in kw.items():
            n[k] = v
    return edit


def _chain(*edits):
    def edit(cfg):
        for e in edits:
            e(cfg)
    return edit


def _global_head(cfg):
    import make_sweep
    make_sweep._v_color_transform_global_head(cfg)


E_SEED = 321

# name: (base YAML, edit[, options]).  Options: seed (default 300 + position), density_scale (scenes.scale_density: the dense scene
# thinned, so that the transmittance does not underflow before the last sample and the tail of a ray stays above a 1e-3 threshold)
CASES = {
    'a_donerf_fea_default': ('donerf_sphere', _mlp('MLP_Fea')),
    'b_donerf_fea_pe2_c64': ('donerf_sphere', _mlp('MLP_Fea', fea_pe=2, view_pe=2, featureC=64)),
    'c_donerf_fea_c40': ('donerf_sphere', _mlp('MLP_Fea', fea_pe=1, view_pe=3, featureC=40)),
    'c_donerf_fea_nofeape': ('donerf_sphere', _mlp('MLP_Fea', fea_pe=0, view_pe=4, featureC=64)),
    'd_donerf_mlp_pe0': ('donerf_sphere', _mlp('MLP', view_pe=0, featureC=64)),
    'd_donerf_mlp_pe6': ('donerf_sphere', _mlp('MLP', view_pe=6)),
    'e_technicolor_fea': ('technicolor_z_plane', _mlp('MLP_Fea', fea_pe=2, view_pe=2, featureC=64), dict(density_scale=0.2, seed=E_SEED)),
    'f_immersive_fea': ('immersive_sphere', _mlp('MLP_Fea', fea_pe=2, view_pe=2, featureC=64)),
    'g_donerf_white_bg': ('donerf_sphere', _mlp('MLP_Fea', fea_pe=2, view_pe=2, featureC=64, white_bg=1)),
    'g_technicolor_thresh': ('technicolor_z_plane', _mlp('MLP_Fea', fea_pe=2, view_pe=2, featureC=64, rm_weight_mask_thre=1e-3), dict(density_scale=0.2)),
    # (the sweep's base for the 3 x 3 global transform, catacaustics_distance, spreads its 64 distances over (-far, far) and masks the
    #  negative half: no ray of it keeps every sample.  catacaustics_cylinder carries the same head on a cylinder intersection)
    'g_catacaustics_global': ('catacaustics_cylinder', _chain(_global_head, _mlp('MLP_Fea', fea_pe=2, view_pe=2, featureC=64)), dict(density_scale=0.2)),
}

# name: (module, constructor arguments)
UNITS = {
    'unit_fea_default': ('MLPRender_Fea', dict(viewpe=6, feape=6, featureC=128)),
    'unit_fea_pe2_c64': ('MLPRender_Fea', dict(viewpe=2, feape=2, featureC=64)),
    'unit_fea_c40': ('MLPRender_Fea', dict(viewpe=3, feape=1, featureC=40)),
    'unit_fea_nofeape': ('MLPRender_Fea', dict(viewpe=4, feape=0, featureC=64)),
    'unit_mlp_pe0': ('MLPRender', dict(viewpe=0, featureC=64)),
    'unit_mlp_pe6': ('MLPRender', dict(viewpe=6, featureC=128)),
    'unit_fea_c256': ('MLPRender_Fea', dict(viewpe=1, feape=1, featureC=256)),
    'unit_mlp_c1': ('MLPRender', dict(viewpe=2, featureC=1)),
}


def live_stats(weights, thresh):
    live = weights > thresh
    return float(live.mean()), int((~live.any(1)).sum()), int(live.all(1).sum())


def check_whole(name, a, recipe):
    """The conditions on a whole-model fixture (the tool when it writes, the tests when they read)."""
    rgb, rgb64, w = a['rgb'], a['rgb64'], a['render_weights']
    assert not np.isnan(rgb).any() and not np.isnan(rgb64).any(), name
    mid = float(((rgb > 0.05) & (rgb < 0.95)).mean())
    assert mid >= 0.5, f'{name}: only {mid:.2f} of the channels in (0.05, 0.95)'
    thresh = float(recipe['model_cfg']['color']['net'].get('rm_weight_mask_thre', 1e-4))
    frac, none_live, all_live = live_stats(w, thresh)
    assert none_live >= 1 and all_live >= 1, f'{name}: {none_live} rays without, {all_live} rays with only live samples'
    if abs(thresh - 1e-3) < 1e-9:
        assert 0.1 < frac < 0.9, f'{name}: live fraction {frac:.3f}'
    dev = float(np.abs(rgb.astype(np.float64) - rgb64).max())
    assert dev <= 2.5e-5, f'{name}: max |rgb32 - rgb64| {dev:.3e}'
    return mid, frac, none_live, all_live, dev


def check_unit(name, a):
    rgb, rgb64 = a['rgb'], a['rgb64']
    assert not np.isnan(rgb).any() and not np.isnan(rgb64).any(), name
    mid = float(((rgb > 0.05) & (rgb < 0.95)).mean())
    assert mid >= 0.5, f'{name}: only {mid:.2f} of the channels in (0.05, 0.95)'
    return mid, float(np.abs(rgb.astype(np.float64) - rgb64).max())


CARVE_X = 0.5        # scenes.carve_half_space: the scene is empty where x lies in the lower half of its axis


def shading_rays(cfg, seed):
    """The sweep's 96 rays, 26 more random ones and 8 that stay on one side of the carved scene (4 on the empty side: no live sample;
    4 on the other): 130 in all -- a third workgroup tile of the 64-ray kernels, an odd tail."""
    import make_sweep
    from hyperreel_amd import scenes
    r = make_sweep.sweep_rays(cfg, seed)
    video = r.shape[1] == 8
    z_plane = 'z_plane' in [e for e in cfg.embedding.embeddings.values() if e.get('type') == 'ray_intersect'][0].intersect.type
    more = scenes.random_rays(26, seed + 7, video)
    if z_plane:
        more = scenes.random_rays(26, seed + 7, video, pos_mean=(0, 0, 1.0), pos_std=0.15, dir_mean=(0, 0, -1.2), dir_std=0.5)
        side = [[sx * 0.5, 0.1, 1.0, sx * d, 0.02, -1.0] for sx in (-1.0, 1.0) for d in (0.0, 0.05, 0.1, 0.15)]
    else:
        side = [[sx * 0.5, 0.05, -0.1, sx * 1.0, dy, dz] for sx in (-1.0, 1.0) for dy, dz in ((0.0, 0.0), (0.2, 0.1), (-0.3, 0.2), (0.1, -0.4))]
    side = np.asarray(side, np.float32)
    side[:, 3:6] /= np.linalg.norm(side[:, 3:6], axis=1, keepdims=True)
    if video:
        side = np.concatenate([side, np.zeros((8, 1), np.float32), np.linspace(0.0, 0.9, 8, dtype=np.float32)[:, None]], -1)
    more = np.concatenate([more, side.astype(np.float32)], 0)
    if more.shape[1] < r.shape[1]:
        more = np.concatenate([more, np.zeros((more.shape[0], r.shape[1] - more.shape[1]), np.float32)], -1)
    return np.ascontiguousarray(np.concatenate([r, more], 0), np.float32)


def run_whole(name, base, edit, seed, density_scale=1.0):
    import make_sweep
    import ref_shim
    from hyperreel_amd import config as C
    from hyperreel_amd import plan, scenes
    ds = make_sweep.dataset_for(base)
    raw = C.load_model_yaml(f'{ref_shim.REF}/conf/experiment/model/{base}.yaml')
    raw.color.net.grid_size = C.to_cfg({'start': list(GRID), 'end': list(GRID)})
    edit(raw)
    raw = C.to_cfg(C.to_plain(raw))
    model_cfg = C.epoch_to_iter(C.to_cfg(C.to_plain(raw)), 4000)
    plan.compile_model(model_cfg, ds, GRID)

    def overrides(cfg):
        cfg.color.net.grid_size = ref_shim.to_attr({'start': list(GRID), 'end': list(GRID)})
        edit(cfg)
        isect = [e for e in cfg.embedding.embeddings.values() if e.get('type') == 'ray_intersect'][0].intersect
        for k, v in list(isect.items()):                  # plain dicts written by an edit -> attr dicts
            isect[k] = ref_shim.to_attr(v)

    fn = ref_shim.build_reference(ref_shim.load_model_cfg(base, overrides), ds)
    sd = scenes.make_state_dict(model_cfg, ds, GRID, seed, 'dense', 1.0)
    checksum = scenes.state_dict_checksum(sd)
    sd = scenes.carve_half_space(scenes.scale_density(sd, density_scale), CARVE_X)
    own = dict(fn.state_dict())
    with torch.no_grad():
        for k, v in sd.items():
            if k.endswith('gridSize'):
                continue
            assert tuple(own[k].shape) == tuple(v.shape), (name, k, own[k].shape, v.shape)
            own[k].copy_(torch.from_numpy(v))
    missing = [k for k in own if k not in sd and 'dummy_layer' not in k]
    assert not missing, (name, missing)
    rays = shading_rays(model_cfg, seed)
    out = ref_shim.run_reference(fn, torch.from_numpy(rays), fields=['render_weights'])
    fn64 = copy.deepcopy(fn).double()
    out64 = ref_shim.run_reference(fn64, torch.from_numpy(rays).double())
    recipe = {'case': 'shading/' + name, 'model': base, 'model_cfg': C.to_plain(raw), 'z_channels': None, 'grid': GRID, 'seed': seed,
              'density': 'dense', 'app_scale': 1.0, 'dataset': ds, 'checksum': checksum, 'carve_x': CARVE_X,
              'density_scale': density_scale}
    arrays = {'rays': rays, 'rgb': out['rgb'].numpy().astype(np.float32), 'rgb64': out64['rgb'].numpy().astype(np.float64),
              'render_weights': out['render_weights'].numpy().astype(np.float32)}
    thresh = float(recipe['model_cfg']['color']['net'].get('rm_weight_mask_thre', 1e-4))
    print(f'{name:28s} most live samples on a ray {int((arrays["render_weights"] > thresh).sum(1).max())} of {arrays["render_weights"].shape[1]}, max |rgb32 - rgb64| {np.abs(arrays["rgb"] - arrays["rgb64"]).max():.3e}', flush=True)
    stats = check_whole(name, arrays, recipe)
    np.savez_compressed(os.path.join(OUT, name + '.npz'), recipe=np.frombuffer(json.dumps(recipe).encode(), dtype=np.uint8), **arrays)
    print(f'{name:28s} {rays.shape[0]} rays, mid {stats[0]:.2f}, live {stats[1]:.3f}, rays none/all live {stats[2]}/{stats[3]}, '
          f'max |rgb32 - rgb64| {stats[4]:.3e}')
    return [k[len('model.'):] for k in own if 'renderModule' in k]


def run_unit(name, module, kwargs, seed):
    import ref_shim
    ref_shim.install()
    with ref_shim.cpu_mode():
        from nlf.nets import tensorf_base
        torch.manual_seed(seed)
        net = getattr(tensorf_base, module)(27, **kwargs)
    rng = np.random.default_rng(seed)
    with torch.no_grad():                        # the last Linear x 4, as scenes.make_state_dict scales it: colours off 0.5, not saturated
        net.mlp[4].weight.mul_(4.0)
    n = 300
    f = ((rng.random((n, 27), dtype=np.float32) * 2 - 1) * rng.choice(np.asarray([0.05, 0.5, 2.0, 4.0], np.float32), (n, 1))).astype(np.float32)
    v = rng.standard_normal((n, 3), dtype=np.float32)
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    with torch.no_grad():
        rgb = net(None, torch.from_numpy(v), torch.from_numpy(f), {}).numpy().astype(np.float32)
        rgb64 = copy.deepcopy(net).double()(None, torch.from_numpy(v).double(), torch.from_numpy(f).double(), {}).numpy()
    arrays = {'f': f, 'v': v, 'rgb': rgb, 'rgb64': rgb64}
    for k, t in net.state_dict().items():
        arrays['sd/' + k] = t.numpy().astype(np.float32)
    recipe = {'module': module, 'kwargs': kwargs, 'seed': seed}
    mid, dev = check_unit(name, arrays)
    np.savez_compressed(os.path.join(OUT, name + '.npz'), recipe=np.frombuffer(json.dumps(recipe).encode(), dtype=np.uint8), **arrays)
    print(f'{name:28s} {n} rows, width {net.in_mlpC}, mid {mid:.2f}, max |rgb32 - rgb64| {dev:.3e}')


def main(only=None):
    torch.set_num_threads(1)
    os.makedirs(OUT, exist_ok=True)
    keys = None
    failed = []
    for i, (name, case) in enumerate(CASES.items()):
        if only and name not in only:
            continue
        opts = dict(case[2]) if len(case) > 2 else {}
        try:
            keys = run_whole(name, case[0], case[1], opts.pop('seed', 300 + i), **opts)
        except AssertionError as e:               # the other cases still run; the tool fails at the end
            failed.append(str(e))
            print('FAILED', e, flush=True)
    for i, (name, (module, kwargs)) in enumerate(UNITS.items()):
        if only and name not in only:
            continue
        run_unit(name, module, kwargs, 400 + i)
    if keys is not None:                         # the reference's state_dict keys of the colour network: names only
        with open(os.path.join(OUT, 'render_module_keys.json'), 'w') as fjson:
            json.dump(sorted(keys), fjson, indent=1)
    assert not failed, failed


if __name__ == '__main__':
    main(sys.argv[1:] or None)
