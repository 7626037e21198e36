"""Every refusal of plan.compile_config and plan.compile_cascade, by name: one row per `raise`, reached through the public front door
(plan.compile_model) from a base model and one mutation of its YAML group or dataset scalars.  The exception's type and its WHOLE message
are compared, so no refusal changes its wording -- nor, in the rows where two would apply (COMPETING), its precedence.  No GPU.

Two refusals cannot be reached from the public entry points and have no row: compile_config's "... with a point_prediction cascade"
(a configuration with a point_prediction stage is refused as an unknown embedding first, and compile_cascade refuses the modes before it
compiles a level) and compile_cascade's 'more than 4 point_prediction inputs' (the inputs are a mapping over four known names, and an
unknown name is refused first)."""
import copy

import pytest

from hyperreel_amd import config as CFG
from hyperreel_amd import plan
from helpers import Golden

GRID = [28, 24, 20]
NIE, VE = NotImplementedError, ValueError


def _base(name, **kw):
    if name == 'cascade':
        g = Golden('sweep/technicolor_cascaded')
        return copy.deepcopy(g.cfg), copy.deepcopy(g.dataset)
    return CFG.model_config(name, **kw), CFG.dataset_scalars(name)


class M:
    """The parts of a model group a mutation reaches for"""

    def __init__(self, cfg, ds):
        self.cfg, self.ds, self.args = cfg, ds, {}
        self.E = cfg.embedding.embeddings
        self.pred = self.E.ray_prediction_0
        self.ray = self.pred.params.ray
        self.out = self.pred.outputs
        self.ic = self.E.ray_intersect_0.intersect
        self.net = cfg.color.net
        self.pp = self.E.get('point_prediction_0')

    def reorder(self, *keys):
        """the embeddings named first, in that order, then the rest"""
        items = [(k, self.E[k]) for k in keys] + [(k, v) for k, v in self.E.items() if k not in keys]
        self.E.clear()
        self.E.update(items)

    def stage(self, name, **kw):
        self.E[name] = CFG.to_cfg(dict(type=name, **kw))

    def see(self, field):
        self.E.extract_fields.fields.append(field)

    def z(self, n):
        self.pred.z_channels = self.E.ray_intersect_0.z_channels = n


def _set(obj, **kw):
    for k, v in kw.items():
        obj[k] = CFG.to_cfg(v)


def _groups(m, n):
    for i in range(n):
        m.pred.params[f'g{i}'] = CFG.to_cfg({'start': 0, 'end': 1, 'param': {'fn': 'identity'}})


def _voxel(m, **kw):
    _set(m.ic, type='voxel_grid', **kw)


def _deformable(m, **kw):
    _set(m.ic, type='deformable_voxel_grid', use_dataset_bounds=False, **kw)


def _color_table(m, **kw):
    m.stage('color_transform', **kw)
    m.ds['val_all'] = True
    m.ds['total_images_per_frame'] = 4


def _donerf_contract(m):
    _set(m.ic, contract={'type': 'donerf', 'contract_samples': True, 'distance_activation': 'sigmoid'})


ORDER = "embedding order ['ray_prediction', 'point_offset', 'ray_intersect'] (expected prediction, intersect[, advect][, offset])"
LAYOUT = ("cascade layout ['ray_prediction', 'ray_intersect', 'point_prediction', 'advect_points', 'point_offset', 'add_point_outputs', "
          "'extract_fields'] (expected ray_prediction, ray_intersect, point_prediction, ray_intersect, ...)")
MLP_PE = ("shadingMode 'MLP_PE': the reference cannot run it (MLPRender_PE's first Linear expects more inputs than its forward "
          "concatenates)")
SCOPE = 'is outside the hot-path scope'
D, T, CASC = 'donerf_sphere', 'technicolor_z_plane', 'cascade'

# (id, base model, mutation, exception type, whole message)
CONFIG = [
    ('param_fn', D, lambda m: _set(m.cfg.param, fn='pluecker'), NIE, "model.param.fn other than 'identity'"),
    ('embedding_type', D, lambda m: _set(m.cfg.embedding, type='ray'), NIE, 'embedding type ray'),
    ('embedding_stage', D, lambda m: m.stage('foo'), NIE, f"embedding 'foo' {SCOPE}"),
    ('embedding_order', D, lambda m: m.reorder('ray_prediction_0', 'point_offset_0'), NIE, ORDER),
    ('ray_outputs', D, lambda m: _set(m.pred, ray_outputs={'x': 1}), NIE, 'ray_outputs'),
    ('rays_name', D, lambda m: _set(m.pred, rays_name='r'), NIE, 'rays_name'),
    ('groups', D, lambda m: _groups(m, 4), NIE, 'more than 4 parameter groups'),
    ('param_unknown', D, lambda m: _set(m.ray.param, fn='spherical'), NIE, f"ray param 'spherical' {SCOPE}"),
    ('use_local_param', D, lambda m: _set(m.ray.param, use_local_param=True), NIE, 'use_local_param'),
    ('pluecker_columns', D, lambda m: _set(m.ray, end=5), VE, 'pluecker needs 6 ray columns'),
    ('two_plane_columns', T, lambda m: _set(m.ray, end=5), VE, 'two_plane needs 6 ray columns'),
    ('identity_columns', D, lambda m: _set(m.ray, end=9, param={'fn': 'identity'}), NIE, 'identity param with more than 8 columns'),
    ('pe_type', D, lambda m: _set(m.ray.pe, type='gaussian'), NIE, f"pe 'gaussian' {SCOPE}"),
    ('pe_window_iters', D, lambda m: _set(m.ray.pe, window_iters=5), NIE, f'windowed PE with explicit window_iters / ceil {SCOPE}'),
    ('pe_ceil', D, lambda m: _set(m.ray.pe, type='basic', ceil=True), NIE, f'windowed PE with explicit window_iters / ceil {SCOPE}'),
    ('pe_freqs', D, lambda m: _set(m.ray.pe, n_freqs=9), NIE, 'windowed PE with more than 8 frequencies'),
    ('mlp_in', D, lambda m: _set(m.ray.pe, n_freqs=8), NIE, 'MLP input of 102 features (max 64)'),
    ('net_type', D, lambda m: _set(m.pred.net, type='tiny'), NIE, f"net 'tiny' {SCOPE} (BaseMLP, ZeroMLP)"),
    ('net_key', D, lambda m: _set(m.pred.net, pad_to=8), NIE, 'net.pad_to'),
    ('net_activation', D, lambda m: _set(m.pred.net, layer_activation='relu'), NIE, 'MLP activations other than leaky_relu / identity'),
    ('net_bias', D, lambda m: _set(m.pred.net, bias=False), NIE, 'bias-free MLP'),
    ('net_skip_0', D, lambda m: _set(m.pred.net, skips=[0]), NIE, 'skip connection into layer 0'),
    ('z_channels', D, lambda m: m.z(257), NIE, 'z_channels 257 > 256'),
    ('no_z_vals', D, lambda m: m.out.pop('z_vals'), NIE, 'model without a z_vals head'),
    ('color_scale_alone', D, lambda m: m.out.pop('color_shift'), VE, 'color_scale without color_shift'),
    ('color_transform_head', T, lambda m: (m.out.pop('color_scale'), _set(m.out, color_transform={'channels': 9})), NIE,
     f"head 'color_transform' {SCOPE}"),
    ('color_scale_global_alone', T, lambda m: _set(m.out, color_scale_global={'channels': 3}), VE,
     'color_scale_global without color_shift_global'),
    ('color_transform_global_alone', T, lambda m: _set(m.out, color_transform_global={'channels': 9}), VE,
     'color_transform_global without color_shift_global'),
    ('color_transform_global_channels', T,
     lambda m: _set(m.out, color_transform_global={'channels': 6}, color_shift_global={'channels': 3}), VE,
     'color_transform_global needs 9 channels'),
    ('color_channels', D, lambda m: _set(m.out.color_scale, channels=4), VE, 'color_scale needs 3 channels'),
    ('color_global_channels', T, lambda m: _set(m.out, color_scale_global={'channels': 3}, color_shift_global={'channels': 9}), VE,
     'color_shift_global needs 3 channels'),
    ('weights_shift', T, lambda m: (_set(m.out, weights_shift={'channels': 1}), m.see('weights_shift')), NIE,
     f"head 'weights_shift' {SCOPE}"),
    ('color_table_renamed', T, lambda m: _color_table(m, out_transform_field='x'), NIE, 'color_transform with renamed output fields'),
    ('color_table_next_to_head', T, lambda m: (_color_table(m), _set(m.out, color_shift_global={'channels': 3})), NIE,
     'color_transform next to a color_shift_global head'),
    ('z_channels_disagree', D, lambda m: _set(m.E.ray_intersect_0, z_channels=16), VE,
     'ray_prediction and ray_intersect disagree on z_channels'),
    ('intersect_type', D, lambda m: _set(m.ic, type='plane'), NIE, f"intersect 'plane' {SCOPE} (SURVEY 8f-1)"),
    ('intersect_z_vals', D, lambda m: _set(m.ic, type='z_plane'), VE, "intersect 'z_plane' needs 1 z_vals channels, the head has 4"),
    ('intersect_key', D, lambda m: _set(m.ic, dropout=0.5), NIE, 'intersect.dropout'),
    ('intersect_key_last', D, lambda m: _set(m.ic, max_axis=True), NIE, 'intersect.max_axis'),
    ('intersect_num_repeat', D, lambda m: _set(m.ic, num_repeat=2), NIE, 'intersect.num_repeat'),
    ('intersect_sigma_channels', D, lambda m: _set(m.ic, in_density_field='point_offset'), NIE,
     'intersect density field with more than one channel'),
    ('contract_type', D, lambda m: _set(m.ic.contract, type='foo'), NIE, f"contract 'foo' {SCOPE}"),
    ('contract_stop_iters', D, lambda m: _set(m.ic.contract, stop_iters=5), NIE, 'contract.stop_iters'),
    ('mipnerf_distance_activation', D, lambda m: _set(m.ic.contract, distance_activation='sigmoid'), NIE,
     f'contract.distance_activation {SCOPE}'),
    ('donerf_distance_activation', D, _donerf_contract, NIE, f'contract.distance_activation {SCOPE}'),
    ('voxel_thirds', T, lambda m: _voxel(m), VE, 'voxel_grid needs z_channels divisible by 3'),
    ('voxel_bounds', T, lambda m: (m.z(30), _voxel(m, use_dataset_bounds=True), m.ic.pop('initial')), VE,
     'voxel_grid with use_dataset_bounds reads dataset.bbox_min / bbox_max'),
    ('deformable_bounds', D, lambda m: _set(m.ic, type='deformable_voxel_grid'), NIE,
     'deformable_voxel_grid with use_dataset_bounds (reads the dataset point cloud)'),
    ('deformable_normals', D, lambda m: _deformable(m, start_normal=[]), VE,
     'deformable_voxel_grid needs 1..3 start normals dividing z_channels'),
    ('deformable_normals_divide', D, lambda m: _deformable(m), VE, 'deformable_voxel_grid needs 1..3 start normals dividing z_channels'),
    ('deformable_z_scale', D, lambda m: (m.z(30), _deformable(m, z_scale=[1.0])), NIE,
     'deformable_voxel_grid.z_scale with more than one axis (the reference cannot broadcast it)'),
    ('angular_flow', T, lambda m: _set(m.E.flow_0, use_angular_flow=True), NIE, 'angular flow'),
    ('flow_head', T, lambda m: m.out.pop('spatial_flow'), VE, 'advect_points needs a spatial_flow head'),
    ('offset_key', D, lambda m: _set(m.E.point_offset_0, dropout=0.5), NIE, 'point_offset.dropout'),
    ('offset_head', D, lambda m: m.out.pop('point_offset'), VE, 'point_offset needs a point_offset head'),
    ('offset_sigma_channels', D, lambda m: _set(m.E.point_offset_0, in_density_field='color_scale'), NIE,
     'offset density field with more than one channel'),
    ('color_model', D, lambda m: _set(m.cfg.color, type='x'), NIE, 'color model x'),
    ('colour_net', D, lambda m: _set(m.net, type='tensor_vm'), NIE, f"colour net 'tensor_vm' {SCOPE}"),
    ('net_filter', D, lambda m: _set(m.net, filter={}), NIE, 'net.filter (apply_filter_weights)'),
    ('shading_mlp_pe', D, lambda m: _set(m.net, shadingMode='MLP_PE'), NIE, MLP_PE),
    ('shading_unknown', D, lambda m: _set(m.net, shadingMode='foo'), NIE,
     f"shadingMode 'foo' {SCOPE} (RGB, SH, MLP_Fea, MLP, RGBtLinear, RGBtFourier, RGBIdentity)"),
    ('shading_mlp_samples', D, lambda m: (m.z(96), _set(m.net, shadingMode='MLP_Fea', data_dim_color=27)), NIE,
     "shadingMode 'MLP_Fea' with z_channels 96 > 64"),
    ('density_act', D, lambda m: _set(m.net, fea2denseAct='exp'), NIE, 'fea2denseAct exp'),
    ('video_without_advect', T, lambda m: m.E.pop('flow_0'), NIE, 'video net without an advect_points stage (base_times)'),
    ('precision_width', D, lambda m: (_set(m.pred.net, hidden_channels=128), m.args.update(mlp_precision='f16x3')), NIE,
     'f16x3 MLP needs hidden_channels == 256'),
    ('grid_dtype', D, lambda m: m.args.update(grid_dtype='bf16'), VE, "grid_dtype must be one of ['fp16', 'fp32'] (got 'bf16')"),
]

CASCADE = [
    ('shading_mlp', CASC, lambda m: _set(m.net, shadingMode='MLP'), NIE, "shadingMode 'MLP' with a point_prediction cascade"),
    ('time_modes', CASC, lambda m: _set(m.net, densityMode='DensityLinear'), NIE,
     "shadingMode 'SH' / densityMode 'DensityLinear' with a point_prediction cascade"),
    ('identity_mode', CASC, lambda m: _set(m.net, shadingMode='RGBIdentity'), NIE,
     "shadingMode 'RGBIdentity' / densityMode 'Density' with a point_prediction cascade"),
    ('layout', CASC, lambda m: m.E.pop('ray_intersect_1'), NIE, LAYOUT),
    ('filter', CASC, lambda m: _set(m.pp, filter=True), NIE, 'point_prediction.filter'),
    ('renamed', CASC, lambda m: _set(m.pp, points_name='p'), NIE, 'point_prediction with renamed rays / points'),
    ('residual', CASC, lambda m: _set(m.pp.outputs.z_vals, residual=True), NIE, 'residual point_prediction outputs'),
    ('in_z', CASC, lambda m: _set(m.pp, in_z_channels=4), VE, 'point_prediction in_z_channels 4 / out_z_channels 32 vs 8 coarse samples'),
    ('out_z', CASC, lambda m: _set(m.pp, out_z_channels=36), VE, 'point_prediction in_z_channels 8 / out_z_channels 36 vs 8 coarse samples'),
    ('input_name', CASC, lambda m: _set(m.pp.inputs, normals=3), NIE, "point_prediction input 'normals'"),
    ('input_columns', CASC, lambda m: _set(m.pp.inputs, points=4), VE, "point_prediction input 'points': 4 columns"),
    ('row_width', CASC, lambda m: _set(m.pp, inputs={'points': 3, 'viewdirs': 3, 'origins': 3}), NIE,
     'point_prediction rows wider than 8 columns'),
    ('param_fn', CASC, lambda m: _set(m.pp.params.ray.param, fn='pluecker'), NIE, 'point_prediction params other than identity'),
    ('param_end', CASC, lambda m: _set(m.pp.params.time, end=9), VE, 'point_prediction param reads beyond the input row'),
]

# two refusals apply; the one raised is the one the compiler reaches first
COMPETING = [
    ('stage_before_order', D, lambda m: (m.stage('foo'), m.reorder('ray_prediction_0', 'point_offset_0')), NIE, f"embedding 'foo' {SCOPE}"),
    ('color_scale_before_weights_shift', T,
     lambda m: (m.out.pop('color_shift'), _set(m.out, weights_shift={'channels': 1}), m.see('weights_shift')), VE,
     'color_scale without color_shift'),
    ('param_fn_before_embedding_type', D, lambda m: (_set(m.cfg.param, fn='pluecker'), _set(m.cfg.embedding, type='ray')), NIE,
     "model.param.fn other than 'identity'"),
    ('z_channels_before_disagreement', D, lambda m: _set(m.pred, z_channels=257), NIE, 'z_channels 257 > 256'),
    ('ray_outputs_before_net_type', D, lambda m: (_set(m.pred, ray_outputs={'x': 1}), _set(m.pred.net, type='tiny')), NIE, 'ray_outputs'),
    ('intersect_type_before_key', D, lambda m: _set(m.ic, type='plane', dropout=0.5), NIE, f"intersect 'plane' {SCOPE} (SURVEY 8f-1)"),
    ('intersect_keys_in_order', D, lambda m: _set(m.ic, max_axis=True, weight_fn='x'), NIE, 'intersect.weight_fn'),
    ('contract_type_before_stop_iters', D, lambda m: _set(m.ic.contract, type='foo', stop_iters=5), NIE, f"contract 'foo' {SCOPE}"),
    ('head_before_intersect', D, lambda m: (m.out.pop('color_shift'), _set(m.ic, type='plane')), VE, 'color_scale without color_shift'),
    ('intersect_before_offset', D, lambda m: (_set(m.ic, num_repeat=2), m.out.pop('point_offset')), NIE, 'intersect.num_repeat'),
    ('offset_before_colour_net', D, lambda m: (m.out.pop('point_offset'), _set(m.net, type='tensor_vm')), VE,
     'point_offset needs a point_offset head'),
    ('mlp_pe_before_density_act', D, lambda m: _set(m.net, shadingMode='MLP_PE', fea2denseAct='exp'), NIE, MLP_PE),
    ('shading_mlp_before_samples', D, lambda m: (m.z(96), _set(m.net, shadingMode='MLP_Fea', data_dim_color=3)), NIE,
     "shadingMode 'MLP_Fea' with data_dim_color 3: the colour network's kernels take 27 appearance features"),
    ('precision_before_grid_dtype', D,
     lambda m: (_set(m.pred.net, hidden_channels=128), m.args.update(mlp_precision='f16x3', grid_dtype='bf16')), NIE,
     'f16x3 MLP needs hidden_channels == 256'),
    ('colour_net_before_grid_dtype', D, lambda m: (_set(m.net, fea2denseAct='exp'), m.args.update(grid_dtype='bf16')), NIE,
     'fea2denseAct exp'),
    ('cascade_shading_before_layout', CASC, lambda m: (_set(m.net, shadingMode='MLP'), m.E.pop('ray_intersect_1')), NIE,
     "shadingMode 'MLP' with a point_prediction cascade"),
    ('cascade_layout_before_filter', CASC, lambda m: (m.E.pop('ray_intersect_1'), _set(m.pp, filter=True)), NIE, LAYOUT),
    ('cascade_row_before_coarse_level', CASC,
     lambda m: (_set(m.pp, inputs={'points': 3, 'viewdirs': 3, 'origins': 3}), _set(m.pred.net, type='tiny')), NIE,
     'point_prediction rows wider than 8 columns'),
    ('cascade_coarse_level_before_param', CASC, lambda m: (_set(m.pred.net, type='tiny'), _set(m.pp.params.time, end=9)), NIE,
     f"net 'tiny' {SCOPE} (BaseMLP, ZeroMLP)"),
]


def _rows(table):
    return [pytest.param(*row[1:], id=row[0]) for row in table]


def _check(base, mutate, exc, message):
    m = M(*_base(base))
    mutate(m)
    with pytest.raises(exc) as e:
        plan.compile_model(m.cfg, m.ds, GRID, **m.args)
    assert type(e.value) is exc and str(e.value) == message


def test_the_bases_compile():
    for base in (D, T, CASC):
        m = M(*_base(base))
        assert plan.compile_model(m.cfg, m.ds, GRID)[1].z_channels == 32


@pytest.mark.parametrize('base,mutate,exc,message', _rows(CONFIG))
def test_compile_config_refuses(base, mutate, exc, message):
    _check(base, mutate, exc, message)


@pytest.mark.parametrize('base,mutate,exc,message', _rows(CASCADE))
def test_compile_cascade_refuses(base, mutate, exc, message):
    _check(base, mutate, exc, message)


@pytest.mark.parametrize('base,mutate,exc,message', _rows(COMPETING))
def test_the_first_of_two_refusals_stays_the_first(base, mutate, exc, message):
    _check(base, mutate, exc, message)


def test_one_row_per_refusal():
    """60 of compile_config's 61 and 12 of compile_cascade's 13 (the module docstring names the two without a row), the contracts'
    distance_activation twice, and the second arm of four conditions that refuse with one message"""
    assert len({r[0] for r in CONFIG}) == len(CONFIG) == 60 + 2 + 4
    assert len({r[0] for r in CASCADE}) == len(CASCADE) == 12 + 2
    assert len(COMPETING) >= 5
