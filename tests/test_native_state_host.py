"""The host layer's two rules, without a device: lib.call (the binding's single entry) on symbols that need none, and
models.native_action (create / upload / re-configure / keep an hr_model) as a table over keys that real models produce."""
import ctypes
import glob
import os
import types

import pytest
import torch

from helpers import Golden
from hyperreel_amd import config as C
from hyperreel_amd import lib
from hyperreel_amd.models import CONFIG, CREATE, KEEP, UPLOAD, HipLightfieldModel, native_action

PKG = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'hyperreel_amd')


# ---- native_action ------------------------------------------------------------------------------------------------------------------
def _donerf():
    return HipLightfieldModel(C.model_config('donerf_sphere'), dataset=C.dataset_scalars('donerf_sphere'), grid_size=[8, 8, 8])


def _golden(case):
    g = Golden(case)
    return HipLightfieldModel(g.cfg, dataset=g.dataset, grid_size=g.grid), g


def _key(m, values_travel=False):
    """What the model would hand native_action now (no handle is held on the host, so it is compiled afresh every time)."""
    return m._want(values_travel)[0]


def _touch(m):
    with torch.no_grad():                                                # an in-place update as an optimizer makes it: the version moves, the
        next(iter(m.color_model.net.parameters())).mul_(1.0)             # address stays (through `.data` the version would stand still)


def _new_box(m):
    net = m.color_model.net
    net.aabb = net.aabb.clone() * 0.5                                    # what shrink does: a fresh buffer with another box


def test_no_handle_creates():
    assert native_action(None, _key(_donerf())) is CREATE
    assert native_action(None, _key(_donerf(), True), values_travel=True) is CREATE


def test_keys_of_an_untouched_model_keep_the_handle():
    m = _donerf()
    held = _key(m)
    assert _key(m) == held
    assert native_action(held, _key(m)) is KEEP


def test_parameter_changes_upload_and_creation_inputs_create():
    m = _donerf()
    held = _key(m)
    _touch(m)
    want = _key(m)
    assert want.param_key != held.param_key and want[1:] == held[1:]
    assert native_action(held, want) is UPLOAD
    m.invalidate()                                                       # invalidate() is for the handle's key: the model's own is whole
    assert _key(m) == want
    assert native_action(want._replace(param_key=None), want) is UPLOAD  # ... and an invalidated handle uploads

    m = _donerf()
    held = _key(m)
    m.color_model.net.init_svd_volume([9, 9, 9])                         # parameter key and grid
    want = _key(m)
    assert want.grid == [9, 9, 9] and want.param_key != held.param_key
    assert native_action(held, want) is CREATE

    m = _donerf()
    held = _key(m)
    m.mlp_precision = 'bf16x3'                                           # the precision code the handle is created with
    want = _key(m)
    assert want.made[0] != held.made[0] and want.grid == held.grid
    assert native_action(held, want) is CREATE

    m = _donerf()
    held = _key(m)
    _new_box(m)
    want = _key(m)
    assert want.box_key != held.box_key and want.made[2] != held.made[2]
    assert native_action(held, want) is CREATE


def test_cur_iter_moves_the_configuration_only_where_a_schedule_is_active():
    m = _donerf()                                                        # no schedule: any iteration compiles to the same bytes
    held = _key(m)
    m.set_iter(5)
    assert _key(m) == held and native_action(held, _key(m)) is KEEP

    m, g = _golden('sweep/variant_ease_iter2000')                        # single level, inside its EaseValue window
    held = _key(m)
    m.set_iter(g.iteration)
    want = _key(m)
    assert want.blob != held.blob and want._replace(blob=held.blob) == held and not want.cascade
    assert native_action(held, want) is CONFIG
    m.set_iter(10_000_000)                                               # converged again: the bytes of a model never told an iteration
    assert native_action(held, _key(m)) is KEEP


def test_a_cascade_is_created_again_once_where_a_single_level_is_reconfigured():
    m, g = _golden('sweep/technicolor_cascaded')
    held = _key(m)
    assert held.cascade
    m.set_iter(1000)
    want = _key(m)
    assert want.blob != held.blob and want.blob == bytes(m._compile(m.grid_size)[1]) + bytes(m._compile(m.grid_size)[0])
    assert native_action(held, want) is CREATE                           # hr_model_update_config does not take cascades
    _touch(m)                                                            # parameters AND schedule: one action, the strongest
    want = _key(m)
    assert want.param_key != held.param_key and want.blob != held.blob
    assert native_action(held, want) is CREATE
    assert native_action(held, want._replace(blob=held.blob)) is UPLOAD  # (the parameters alone would have uploaded)


def test_a_training_step_ignores_the_parameter_key_but_not_the_box():
    m = _donerf()
    held = _key(m)
    _touch(m)
    want = _key(m, values_travel=True)
    assert want.param_key is None
    assert native_action(held, want, values_travel=True) is KEEP
    assert native_action(held, _key(m), values_travel=False) is UPLOAD
    _new_box(m)
    assert native_action(held, _key(m, values_travel=True), values_travel=True) is CREATE
    m, g = _golden('sweep/variant_ease_iter2000')                        # the schedule still reaches a training step's handle
    held = _key(m)
    m.set_iter(g.iteration)
    assert native_action(held, _key(m, values_travel=True), values_travel=True) is CONFIG


def test_the_state_object_starts_whole_and_the_old_names_read_it():
    m = _donerf()
    assert m._native is None and m._hc is None and m._coarse_hc is None and m._render_calls == 0
    assert m.held_config() is None
    assert m.wanted_config() == _key(m).blob == bytes(m._compile(m.grid_size)[1])
    m._render_calls = 1000                                               # tools set it to get past the polled calls
    assert m._render_calls == 1000


# ---- lib.call -----------------------------------------------------------------------------------------------------------------------
def test_call_returns_values_and_checks_statuses():
    L = lib.load()
    for seed, step in [(0, 0), (1, 2), (7, 3), (2 ** 64 - 1, 5), (11, 2 ** 40)]:
        assert lib.call('hr_train_background_coin', seed, step) == L.hr_train_background_coin(seed, step)
    coins = {lib.call('hr_train_background_coin', 3, s) for s in range(64)}
    assert coins == {0, 1}                                               # a coin of 1 is an answer, not a failing status
    assert lib.call('hr_abi_version') == lib.ABI_VERSION
    lo, hi, lo2, hi2 = (ctypes.c_int64(-1) for _ in range(4))
    assert L.hr_shard_range(1001, 2, 8, ctypes.byref(lo), ctypes.byref(hi)) == 0
    assert lib.call('hr_shard_range', 1001, 2, 8, ctypes.byref(lo2), ctypes.byref(hi2)) is None
    assert (lo2.value, hi2.value) == (lo.value, hi.value) == (251, 125)        # (first ray, count) of rank 2
    with pytest.raises(RuntimeError, match='hr_shard_range failed'):
        lib.call('hr_shard_range', 1001, 8, 8, ctypes.byref(lo2), ctypes.byref(hi2))


def test_call_hands_tensors_over_as_their_own_pointers(monkeypatch):
    seen = []

    def fake(*args):
        seen.append(args)
        return 0
    fake.restype = ctypes.c_int
    monkeypatch.setattr(lib, '_lib', types.SimpleNamespace(hr_fake=fake))
    x = torch.arange(24, dtype=torch.float32).reshape(4, 6)
    view = x[:, 2:]                                                      # row-strided: what HipLinear and HipMLP pass on purpose
    assert not view.is_contiguous()
    assert lib.call('hr_fake', x, None, torch.empty(0), view, 7, 0.5, b'name') is None
    assert seen == [(x.data_ptr(), None, None, view.data_ptr(), 7, 0.5, b'name')]
    assert view.data_ptr() == x.data_ptr() + 8                           # the view's own address: nothing was copied


def test_call_raises_with_the_symbol_and_the_library_text():
    x = torch.zeros(4)
    with pytest.raises(RuntimeError) as e:
        lib.call('hr_plane_reg_forward', x, 1, 0, 4, x, None)            # refused before any launch (tests/c_abi/abi_check.c)
    text = lib.load().hr_last_error().decode()
    assert text and 'hr_plane_reg_forward failed' in str(e.value) and text in str(e.value)
    assert not isinstance(e.value, lib.HipRangeError)
    with pytest.raises(lib.HipRangeError, match='hr_x failed'):
        lib.check(lib.HR_E_RANGE, 'hr_x')
    assert lib.HR_E_RANGE == -5


# ---- the package's source -----------------------------------------------------------------------------------------------------------
def _sources():
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(PKG, '*.py')))}


def test_the_package_calls_the_library_in_one_way():
    src = _sources()
    assert len(src) > 10
    assert [n for n, s in src.items() if '_lib.check(' in s] == []       # (lib.py itself says check(...))
    assert [n for n, s in src.items() if 'cuda_stream' in s] == ['lib.py']
    assert "getattr(self, '_" not in src['models.py']
    assert [n for n, s in src.items() if 'from .lib import' in s] == []  # through the module attribute: tests wrap lib.call
