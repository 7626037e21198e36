"""Records what hyperreel_amd/plan.py compiles, as tests/golden/plan/config_digests.json: one line per (model, dataset scalars, compile
arguments) of a corpus.  An accepted entry is the sha256 of the coarse hr_config's bytes (empty without a cascade), the rendering level's,
and its `shade_mlp` and `time_decode` descriptors (a marker where one is None); a refused entry is '<ExceptionType>: <message>'.

    python tools/make_plan_digests.py            # rewrites the file
    python tools/make_plan_digests.py --check    # exit status 1 where the file and the code differ, with the keys

TEST INFRASTRUCTURE ONLY.  The file is generated on the commit BEFORE a change to plan.py and committed with it;
tests/test_plan_digests_host.py recomputes every entry.  Where a change moves hr_config's bytes on purpose, regenerating shows in the
file's diff which models changed.

The corpus (corpus()):
  fixture/   every golden and sweep fixture through compile_model at the fixture's own iteration, x mlp_precision auto / fp32 / f16f8v,
             x grid_dtype fp32 / fp16
  iter/      every sweep fixture whose name carries `iter` or `ease`, at the iterations None, 0, 2000, 6000 and 10**7; the same through
             an enclosing at_iteration and through compile_config(iteration=...)
  aabb/      an `aabb=` override on a static and on a keyframe model
  mode/      config.model_config on a static and a keyframe family: each shadingMode x densityMode x frames_per_keyframe, the
             combinations the compiler refuses included"""
import functools
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from hyperreel_amd import config as CFG                     # noqa: E402
from hyperreel_amd import plan                              # noqa: E402
import helpers                                              # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'plan', 'config_digests.json')
PRECISIONS = ('auto', 'fp32', 'f16f8v')
GRID_DTYPES = ('fp32', 'fp16')
ITERATIONS = (None, 0, 2000, 6000, 10**7)
FAMILIES = ('donerf_sphere', 'technicolor_z_plane')         # a static and a keyframe family
BOX = [[-1.5, -1.0, -0.5], [1.0, 1.5, 2.0]]
GRID = [28, 24, 20]
NONE = b'\x00none\x00'


@functools.lru_cache(maxsize=None)
def fixture(case):
    return helpers.Golden(case)


def _mode(name, shading, density, fpk):
    kw = dict(shading=shading)
    if density is not None:
        kw['density_mode'] = density
    if fpk is not None:
        kw['frames_per_keyframe'] = fpk
    return plan.compile_model(CFG.model_config(name, **kw), CFG.dataset_scalars(name), GRID)


def _single(case, it, how):
    """A single-level fixture through compile_config: under an enclosing at_iteration, or with its own `iteration` (inside another)."""
    g = fixture(case)
    if how == 'with':
        with plan.at_iteration(it):
            return None, plan.compile_config(g.cfg, g.dataset, g.grid)
    with plan.at_iteration(123):
        return None, plan.compile_config(g.cfg, g.dataset, g.grid, iteration=it)


def corpus():
    """-> {key: function returning (coarse hr_config or None, hr_config)}"""
    out = {}
    for case in helpers.golden_cases() + helpers.sweep_cases():
        for p in PRECISIONS:
            for gd in GRID_DTYPES:
                out[f'fixture/{case}/{p}/{gd}'] = lambda case=case, p=p, gd=gd: plan.compile_model(
                    fixture(case).cfg, fixture(case).dataset, fixture(case).grid, p, gd, iteration=fixture(case).iteration)
    for case in helpers.sweep_cases():
        if 'iter' not in case and 'ease' not in case:
            continue
        for it in ITERATIONS:
            out[f'iter/{case}/{it}'] = lambda case=case, it=it: plan.compile_model(
                fixture(case).cfg, fixture(case).dataset, fixture(case).grid, iteration=it)
            for how in ('with', 'arg'):
                out[f'iter/{case}/{it}/{how}'] = lambda case=case, it=it, how=how: _single(case, it, how)
    for name in FAMILIES:
        out[f'aabb/{name}'] = lambda name=name: plan.compile_model(CFG.model_config(name), CFG.dataset_scalars(name), GRID, aabb=BOX)
        out[f'aabb/{name}/iter2000'] = lambda name=name: plan.compile_model(
            CFG.epoch_to_iter(CFG.model_config(name), 4000), CFG.dataset_scalars(name), GRID, iteration=2000, aabb=BOX)
        for shading in plan.SHADING:
            for density in (None,) + tuple(plan.DENSITY_MODE):
                for fpk in (None, 1, 4, 8):
                    out[f'mode/{name}/{shading}/{density}/fpk{fpk}'] = lambda name=name, shading=shading, density=density, fpk=fpk: _mode(
                        name, shading, density, fpk)
    return out


def digest(fn):
    try:
        coarse, hc = fn()
    except Exception as e:                                  # a refusal is an entry: its type and whole message
        return f'{type(e).__name__}: {e}'
    h = hashlib.sha256()
    h.update(b'' if coarse is None else bytes(coarse))
    h.update(bytes(hc))
    for d in (hc.shade_mlp, hc.time_decode):
        h.update(NONE if d is None else bytes(d))
    return h.hexdigest()


def recorded():
    with open(OUT) as f:
        return json.load(f)


def main():
    got = {k: digest(fn) for k, fn in corpus().items()}
    if '--check' in sys.argv[1:]:
        want = recorded()
        bad = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
        print('\n'.join(bad) if bad else f'{len(got)} entries match')
        return 1 if bad else 0
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, 'w') as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write('\n')
    refused = sum(1 for v in got.values() if ': ' in v)
    print(f'{len(got)} entries ({refused} refused) -> {os.path.relpath(OUT, ROOT)}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
