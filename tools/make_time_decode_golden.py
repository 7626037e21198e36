"""Generates tests/golden/time_decode/*.npz for the keyframe net's time-dependent decode modes (shadingMode RGBtLinear / RGBtFourier /
RGBIdentity, densityMode DensityLinear / DensityFourier) by running the REFERENCE ITSELF (imported in-process through
oracle/refgen/ref_shim.py) on seeded inputs.  Run where the reference tree exists:

    python tools/make_time_decode_golden.py [name ...]

TEST INFRASTRUCTURE ONLY.  Whole-model files in the layout of tools/make_shading_golden.py (whose recipe, scene and ray functions this
tool calls): a shipped model YAML plus an edit (CASES), the reference built from it on a 28 x 24 x 20 grid and loaded with
scenes.make_state_dict's seeded scene, thinned (scenes.scale_density) and emptied over the lower half of the x axis
(scenes.carve_half_space), run on shading_rays' 130 rays.  The times of the 8 rays that stay on one side, and of 4 of the random rays,
are set so that the set holds t = 0, a t on a keyframe exactly (time_offset == 0), offsets of both signs and a t close to 1.
Stored: rays, the reference's rgb and render_weights, rgb64 (the same model on a float64 copy), the recipe, and for the Density* cases
`sigma_pre` -- the density before its activation at every sample the reference evaluates, recorded from the reference's own
DensityLinearRender / DensityFourierRender -- and `sd/...basis_mat_density.weight` in full (below).

A Density* scene: the seeded basis_mat_density has weights of both signs on every row, and under the shipped `fea2denseAct: relu` no ray
of it keeps every sample.  density_matrix() therefore makes the row of the basis' CONSTANT function (Linear: row 0; Fourier: cos 0,
row 1) positive and scales the time-dependent rows by `den_amp`: most rays stay dense, and rays whose time swings the sum below zero
lose samples to the relu.  The matrix is a function of the seeded draw, stored in full (helpers.Golden's `sd/` keys) like the post-fit
weights of the parity fixtures.

Gradient fixtures (tests/golden/time_decode/grad/<case>_bg<0|1>.npz, run_grad): the three colour modes in the reference's train mode.

The conditions tests/test_gpu_time_decode.py relies on are asserted here when a file is written and again by the tests (check_case): no
NaN, at least half of the colour channels in (0.05, 0.95), a ray without and a ray with only live samples, for Density* cases at
least 10 % of `sigma_pre` negative and at least 10 % positive, max |rgb32 - rgb64| <= 2.5e-5."""
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
sys.path.insert(0, HERE)

import make_shading_golden as S          # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'time_decode')
GRID = S.GRID
NET = 'model.color_model.net.'
CAP = 8                                   # plan.TIME_MAX_FPK


def _mode(shading=None, density=None, fpk=None, fpk_default=4, **kw):
    """The YAML edit of a case: the toggles, data_dim_color as the reference sets it (3 nb: tensorf_dynamic.py:62-65), other net keys."""
    def edit(cfg):
        n = cfg.color.net
        if fpk is not None:
            n.frames_per_keyframe = fpk
        if density is not None:
            n.densityMode = density
        if shading is not None:
            n.shadingMode = shading
            f = fpk if fpk is not None else fpk_default
            n.data_dim_color = {'RGBtLinear': 6, 'RGBtFourier': 3 * (2 * f + 1), 'RGBIdentity': 3}[shading]
        for k, v in kw.items():
            n[k] = v
    return edit


# name: (base YAML, edit, options).  Options: seed, density_scale (scenes.scale_density), den_amp (density_matrix), special (time_rays).
# Seeds and amplitudes: the first of a short scan at which the reference alone meets check_case's conditions.
# The shipped video datasets have 50 frames and 12 keyframes: frames_per_keyframe defaults to 50 // 12 = 4.
CASES = {
    'a_technicolor_rgbt_linear': ('technicolor_z_plane', _mode('RGBtLinear'), dict(density_scale=0.2)),
    'b_technicolor_rgbt_fourier': ('technicolor_z_plane', _mode('RGBtFourier'), dict(density_scale=0.2)),               # 27 rows, SH's count
    'b_technicolor_rgbt_fourier_fpk1': ('technicolor_z_plane', _mode('RGBtFourier', fpk=1), dict(density_scale=0.2)),   # 9 rows
    'b_technicolor_rgbt_fourier_fpk5': ('technicolor_z_plane', _mode('RGBtFourier', fpk=5), dict(density_scale=0.2, seed=513)),   # 33 rows
    'b_technicolor_rgbt_fourier_cap': ('technicolor_z_plane', _mode('RGBtFourier', fpk=CAP), dict(density_scale=0.2, seed=513)),  # 51 rows
    'c_technicolor_density_linear': ('technicolor_z_plane', _mode(density='DensityLinear'), dict(density_scale=0.2, seed=505, den_amp=5.0)),
    'c_technicolor_density_fourier': ('technicolor_z_plane', _mode(density='DensityFourier'), dict(density_scale=0.2, seed=505)),
    'd_technicolor_both_fourier': ('technicolor_z_plane', _mode('RGBtFourier', 'DensityFourier'), dict(density_scale=0.2, seed=505)),
    'e_neural_3d_both_fourier': ('neural_3d_z_plane', _mode('RGBtFourier', 'DensityFourier'), dict(density_scale=0.2, seed=532, den_amp=3.0, special=(89, 90, 92))),
    'f_immersive_rgbt_fourier': ('immersive_sphere', _mode('RGBtFourier'), dict(density_scale=0.2, seed=503)),
    'g_donerf_rgb_identity': ('donerf_sphere', _mode('RGBIdentity'), dict()),
    'h_technicolor_linear_white_bg': ('technicolor_z_plane', _mode('RGBtLinear', 'DensityLinear', white_bg=1), dict(density_scale=0.2, seed=507, den_amp=6.0)),
    'h_technicolor_fourier_thresh': ('technicolor_z_plane', _mode('RGBtFourier', rm_weight_mask_thre=1e-3), dict(density_scale=0.2, seed=513)),
}


def keyframe_time(dataset, k):
    """A float32 time whose offset from its keyframe is exactly zero: k * float32(1 / fac), what get_base_time returns for it
    (utils/flow_utils.py:10-35)."""
    fac = dataset['num_keyframes'] * (dataset['num_frames'] - 1) / dataset['num_frames']
    return np.float32(np.float32(k) * np.float32(1.0 / fac))


def time_rays(cfg, dataset, seed, special=True):
    """shading_rays with chosen times on the rays that stay on one side (the last 8: 4 on the empty side, then 4 on the dense side)
    and on 4 of the random rays before them.  special: which of the sweep's 8 hand-made rays (88..95: parallel to a plane, through the
    origin ...) are replaced by random ones (False: all, a tuple: those) -- under neural_3d's contraction rays 89, 90 and 92 sit on a
    comparison that the reference's own float32 and float64 evaluations decide differently (a colour difference of 0.97 with `Density`
    too), which says nothing about a decode mode; the other five stay."""
    from hyperreel_amd import scenes
    rays = S.shading_rays(cfg, seed)
    if special is not True:            # False: all eight replaced; a tuple: those of them
        idx = list(range(88, 96)) if special is False else list(special)
        rays[idx] = scenes.random_rays(8, seed + 11, rays.shape[1] == 8, pos_mean=(0, 0, 1.0), pos_std=0.15, dir_mean=(0, 0, -1.2), dir_std=0.5)[:len(idx)]
    if rays.shape[1] != 8:
        return rays
    tk = keyframe_time(dataset, 3)
    dense_side = [0.0, tk, np.float32(tk - np.float32(0.03)), 0.999]        # t = 0; on a keyframe; a negative offset; close to 1
    empty_side = [np.float32(tk + np.float32(0.03)), 0.25, 0.6, 0.97]
    rays[-8:-4, -1] = np.asarray(empty_side, np.float32)
    rays[-4:, -1] = np.asarray(dense_side, np.float32)
    rays[-12:-8, -1] = np.asarray([tk, np.float32(tk + np.float32(0.03)), 0.0, 0.985], np.float32)
    return rays


def density_matrix(w, mode, amp):
    """The Density* scene's basis_mat_density from the seeded draw `w` (rows, cols): the constant function's row made positive, the
    other rows scaled by `amp`."""
    w = w.copy()
    const = 0 if mode == 'DensityLinear' else 1
    for r in range(w.shape[0]):
        w[r] = np.abs(w[r]) if r == const else (w[r] * np.float32(amp)).astype(np.float32)
    return w.astype(np.float32)


def check_case(name, a, recipe):
    """The conditions on a fixture (the tool when it writes, the tests when they read)."""
    stats = S.check_whole(name, a, recipe)
    if recipe['model_cfg']['color']['net'].get('densityMode', 'Density') != 'Density':
        pre = a['sigma_pre']
        neg, pos = float((pre < 0).mean()), float((pre > 0).mean())
        assert neg >= 0.1 and pos >= 0.1, f'{name}: density pre-activations negative {neg:.3f}, positive {pos:.3f}'
        return stats + (neg, pos)
    return stats


def run_case(name, base, edit, seed, density_scale=1.0, den_amp=1.5, special=True):
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
        for k, v in list(isect.items()):
            isect[k] = ref_shim.to_attr(v)

    fn = ref_shim.build_reference(ref_shim.load_model_cfg(base, overrides), ds)
    sd = scenes.make_state_dict(model_cfg, ds, GRID, seed, 'dense', 1.0)
    checksum = scenes.state_dict_checksum(sd)
    sd = scenes.carve_half_space(scenes.scale_density(sd, density_scale), S.CARVE_X)
    dmode = model_cfg.color.net.get('densityMode', 'Density')
    full = {}
    if dmode != 'Density':
        key = NET + 'basis_mat_density.weight'
        sd[key] = full['sd/' + key] = density_matrix(sd[key], dmode, den_amp)
    own = dict(fn.state_dict())
    with torch.no_grad():
        for k, v in sd.items():
            if k.endswith('gridSize'):
                continue
            assert tuple(own[k].shape) == tuple(v.shape), (name, k, own[k].shape, v.shape)
            own[k].copy_(torch.from_numpy(v))
    missing = [k for k in own if k not in sd and 'dummy_layer' not in k]
    assert not missing, (name, missing)
    rays = time_rays(model_cfg, ds, seed, special)

    # the density before its activation, from the reference's own reduction over the time basis
    from nlf.nets import tensorf_dynamic
    recorded = []
    originals = {n: getattr(tensorf_dynamic, n) for n in ('DensityLinearRender', 'DensityFourierRender')}

    def recording(f):
        def g(features, kwargs):
            out = f(features, kwargs)
            recorded.append(out.detach().reshape(-1).numpy().astype(np.float32))
            return out
        return g

    for n, f in originals.items():
        setattr(tensorf_dynamic, n, recording(f))
    try:
        out = ref_shim.run_reference(fn, torch.from_numpy(rays), fields=['render_weights'])
    finally:
        for n, f in originals.items():
            setattr(tensorf_dynamic, n, f)
    fn64 = copy.deepcopy(fn).double()
    out64 = ref_shim.run_reference(fn64, torch.from_numpy(rays).double())
    recipe = {'case': 'time_decode/' + name, 'model': base, 'model_cfg': C.to_plain(raw), 'z_channels': None, 'grid': GRID, 'seed': seed,
              'density': 'dense', 'app_scale': 1.0, 'dataset': ds, 'checksum': checksum, 'carve_x': S.CARVE_X,
              'density_scale': density_scale, 'den_amp': den_amp, 'special_rays': special if isinstance(special, bool) else list(special)}
    arrays = {'rays': rays, 'rgb': out['rgb'].numpy().astype(np.float32), 'rgb64': out64['rgb'].numpy().astype(np.float64),
              'render_weights': out['render_weights'].numpy().astype(np.float32), **full}
    if dmode != 'Density':
        arrays['sigma_pre'] = np.concatenate(recorded) if recorded else np.zeros((0,), np.float32)
    stats = check_case(name, arrays, recipe)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, name + '.npz'), recipe=np.frombuffer(json.dumps(recipe).encode(), dtype=np.uint8), **arrays)
    print(f'{name:36s} {rays.shape[0]} rays, basis_mat {tuple(sd[NET + "basis_mat.weight"].shape)}, mid {stats[0]:.2f}, live {stats[1]:.3f}, '
          f'rays none/all live {stats[2]}/{stats[3]}, max |rgb32 - rgb64| {stats[4]:.3e}'
          + (f', density pre-activation neg/pos {stats[5]:.2f}/{stats[6]:.2f}' if len(stats) > 5 else ''), flush=True)


# Gradient fixtures (the GradGolden layout of oracle/refgen/make_grad_golden.py, whose projections() this calls): the reference in TRAIN
# mode on the case's scene and rays, loss = sum(rgb * G) for a seeded G, both background draws; the full gradient of a tensor of at most
# 20 000 elements (basis_mat among them), 16 seeded projections and the norm of a larger one.
GRAD_CASES = ('a_technicolor_rgbt_linear', 'b_technicolor_rgbt_fourier', 'g_donerf_rgb_identity')
GRAD_OUT = os.path.join(OUT, 'grad')


def run_grad(name):
    import make_grad_golden as GG
    import ref_shim
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from helpers import Golden
    from hyperreel_amd import scenes
    g = Golden('time_decode/' + name)
    base, edit = CASES[name][0], CASES[name][1]

    def overrides(cfg):
        cfg.color.net.grid_size = ref_shim.to_attr({'start': list(GRID), 'end': list(GRID)})
        edit(cfg)
        isect = [e for e in cfg.embedding.embeddings.values() if e.get('type') == 'ray_intersect'][0].intersect
        for k, v in list(isect.items()):
            isect[k] = ref_shim.to_attr(v)

    fn = ref_shim.build_reference(ref_shim.load_model_cfg(base, overrides), g.dataset)
    sd = scenes.carve_half_space(scenes.scale_density(g.state_dict, g.recipe['density_scale']), g.recipe['carve_x'])
    own = dict(fn.state_dict())
    with torch.no_grad():
        for k, v in sd.items():
            if not k.endswith('gridSize'):
                own[k].copy_(torch.from_numpy(v))
    fn.train()
    n = min(GG.N_RAYS, g.rays.shape[0])
    rays = torch.from_numpy(np.ascontiguousarray(g.rays[:n], np.float32))
    G = torch.from_numpy(np.random.default_rng(3).standard_normal((n, 3)).astype(np.float32))
    os.makedirs(GRAD_OUT, exist_ok=True)
    for white in (0, 1):
        for p in fn.parameters():
            p.grad = None
        real_rand = torch.rand
        torch.rand = lambda *a, **k: torch.full((1,), 0.1 if white else 0.9)      # the background draw of this step
        try:
            with ref_shim.cpu_mode():
                rgb = fn(rays)['rgb']
        finally:
            torch.rand = real_rand
        (rgb * G).sum().backward()
        payload = {'rgb': rgb.detach().numpy().astype(np.float32),
                   'recipe': np.frombuffer(json.dumps({'case': 'time_decode/' + name, 'n_rays': n, 'white': white, 'g_seed': 3}).encode(), dtype=np.uint8)}
        for pname, p in fn.named_parameters():
            if p.grad is None or 'dummy' in pname:
                continue
            gr = p.grad.detach().numpy().astype(np.float32)
            if gr.size <= GG.FULL_MAX:
                payload['full/' + pname] = gr
            else:
                payload['proj/' + pname] = GG.projections(pname, gr)
                payload['norm/' + pname] = np.asarray([np.linalg.norm(gr.astype(np.float64)), float(gr.size)])
        bm = payload['full/model.color_model.net.basis_mat.weight']
        assert np.isfinite(payload['rgb']).all() and (np.abs(bm).max(1) > 0).sum() >= bm.shape[0] - 3, name      # every row of basis_mat but the three of sin(0) has a gradient
        path = os.path.join(GRAD_OUT, f'{name}_bg{white}.npz')
        np.savez_compressed(path, **payload)
        print(f'grad {name} bg{white}: {n} rays, basis_mat gradient {bm.shape} max {np.abs(bm).max():.3e}, {os.path.getsize(path) / 1024:.0f} KiB', flush=True)


def main(only=None):
    torch.set_num_threads(1)
    failed = []
    for i, (name, case) in enumerate(CASES.items()):
        if only and name not in only:
            continue
        opts = dict(case[2])
        try:
            run_case(name, case[0], case[1], opts.pop('seed', 500 + i), **opts)
        except AssertionError as e:               # the other cases still run; the tool fails at the end
            failed.append(str(e))
            print('FAILED', e, flush=True)
    assert not failed, failed
    for name in GRAD_CASES:
        if not only or name in only or 'grad' in only:
            run_grad(name)


if __name__ == '__main__':
    main(sys.argv[1:] or None)
