"""A/B of K1 builds inside ONE lease: hr_stage_mlp over 4 x 131 072 DoNeRF rays, each library in its own process, rounds interleaved.
python tools/k1_ab.py product a b ...   (names of tools/_bin/libhr_<name>.so, e.g. from tools/build_k1_variants.py; `product` = the in-tree library)
Times K1 alone (131 072 rays per launch, HIP events on the launch stream) for the DoNeRF model."""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(lib):
    sys.path.insert(0, ROOT)
    import ctypes
    import torch
    from hyperreel_amd import lib as hl
    if lib != 'product':
        hl.LIB_PATH = os.path.join(ROOT, 'tools', '_bin', f'libhr_{lib}.so')
        assert os.path.exists(hl.LIB_PATH), hl.LIB_PATH
    from hyperreel_amd import config as C, scenes
    from hyperreel_amd.render import build_render_fn
    cfg, ds = C.model_config('donerf_sphere'), C.dataset_scalars('donerf_sphere')
    sd = scenes.make_state_dict(cfg, ds, [64, 64, 64], seed=7, density='dense', app_scale=1.0)
    f = build_render_fn(cfg, dataset=ds, grid_size=[64, 64, 64], mlp_precision='f16f8')
    f.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    h = f.model.native()
    rays = torch.from_numpy(scenes.benchmark_rays('donerf_sphere', 800, 800, frame=7)[:131072 * 4]).cuda()
    L = hl.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        for o in range(4):
            hl.check(L.hr_stage_mlp(h, ctypes.c_void_p(rays.data_ptr() + o * 131072 * rays.shape[1] * 4), 131072, st), 'hr_stage_mlp')
    for _ in range(60):          # the clock ramp of an idle GPU
        run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(30):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); run(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / 4)
    ts.sort()
    print(json.dumps({'variant': lib, 'ms_per_launch_min': round(ts[0], 4), 'p50': round(ts[len(ts) // 2], 4)}))


if len(sys.argv) > 2 and sys.argv[1] == '--child':
    child(sys.argv[2])
else:
    names = sys.argv[1:]
    res = {n: [] for n in names}
    for rnd in range(3):
        for n in names:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', n], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            if r.returncode: print(n, 'rc', r.returncode, r.stderr[-400:], flush=True)
            ln = next((l for l in r.stdout.splitlines() if l.startswith('{')), None)
            if ln:
                res[n].append(json.loads(ln)['p50'])
    for n in names:
        print(n, res[n], flush=True)
