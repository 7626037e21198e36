"""plan.py compiles every model of a recorded corpus to the bytes it compiled to when tests/golden/plan/config_digests.json was written
(tools/make_plan_digests.py, whose corpus and digest this file calls): the fixtures' models across the MLP arithmetics and grid types, the
scheduled models across training iterations, aabb overrides, and the shading / density modes of the built-in families -- with the
refusals among them, whose type and whole message are the entry.  No GPU."""
import functools
import importlib.util
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def tool():
    spec = importlib.util.spec_from_file_location('make_plan_digests', os.path.join(HERE, '..', 'tools', 'make_plan_digests.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def corpus():
    return tool().corpus()


def groups():
    """The corpus by everything before a key's last two parts: a fixture with its six (arithmetic, grid type) entries, a family's mode"""
    out = {}
    for k in corpus():
        out.setdefault(k.rsplit('/', 2)[0], []).append(k)
    return out


def test_the_file_and_the_corpus_list_the_same_entries():
    want = tool().recorded()
    assert sorted(want) == sorted(corpus())
    assert len(want) >= 480 + 30 + 2 + 100
    refused = [k for k, v in want.items() if ': ' in v]
    assert any(k.startswith('fixture/') for k in refused) and any(k.startswith('mode/') for k in refused)
    assert all(len(v) == 64 for k, v in want.items() if k not in refused)


@pytest.mark.parametrize('group', sorted(groups()))
def test_compiles_to_the_recorded_bytes(group):
    want, fns = tool().recorded(), corpus()
    for k in groups()[group]:
        assert tool().digest(fns[k]) == want[k], k
