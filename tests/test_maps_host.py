"""hr_maps (include/hyperreel_hip.h) against its ctypes mirror, and the Python surface of render(maps=...) that needs no GPU."""
import ctypes as C
import os

import pytest

from helpers import build_host_lib
from hyperreel_amd import lib, plan

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'c_abi', 'maps_layout.c')
OUT = os.path.join(HERE, 'c_abi', '_build', 'libhr_maps_layout.so')


@pytest.fixture(scope='module')
def ml():
    build_host_lib(OUT, SRC, [SRC, os.path.join(HERE, '..', 'include', 'hyperreel_hip.h')])
    m = C.CDLL(OUT)
    m.hm_maps_offset.argtypes = [C.c_int]
    return m


def test_hr_maps_layout_matches_c(ml):
    assert ml.hm_maps_sizeof() == C.sizeof(plan.hr_maps)
    names = [n for n, _ in plan.hr_maps._fields_]
    assert names == ['distances_dev', 'points_dev', 'acc_dev']
    for i, n in enumerate(names):
        assert ml.hm_maps_offset(i) == getattr(plan.hr_maps, n).offset, n


def test_maps_entry_points_are_bound_at_abi_27():
    assert lib.ABI_VERSION == 27
    bound = {name: args for name, _, args in lib.SYMBOLS}
    assert bound['hr_render_maps'][-2] is C.POINTER(plan.hr_maps)
    assert bound['hr_render_frame_maps'][3] is C.c_float
    assert bound['hr_render_frame_maps'][-2] is C.POINTER(plan.hr_maps)


def test_fast_fields_request_selection():
    """Which forward(fields=...) requests the opt-in fast_fields path serves (no GPU: only the model's compiled configuration)."""
    from hyperreel_amd import config
    from hyperreel_amd.models import HipLightfieldModel
    cfg = config.model_config('donerf_sphere')
    m = HipLightfieldModel(cfg, dataset=config.dataset_scalars('donerf'), fast_fields=True)
    assert m.fast_fields
    assert m._fast_field_maps(['distances', 'points'], {}) == ('distances', 'points')
    assert m._fast_field_maps(['points', 'not_a_field'], {}) == ('points',)          # unknown keys are skipped, as the reference's loop does
    assert m._fast_field_maps(['distances', 'render_weights'], {}) is None          # a per-sample output
    assert m._fast_field_maps(['distances', 'viewdirs'], {}) is None
    assert m._fast_field_maps(['distances'], {'no_over_fields': ['distances']}) is None
    assert m._fast_field_maps(['distances'], {'pred_weights_fields': ['distances']}) is None
    assert not HipLightfieldModel(cfg, dataset=config.dataset_scalars('donerf')).fast_fields
