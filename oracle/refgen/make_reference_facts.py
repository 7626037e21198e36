"""Generates tests/golden/reference_facts.json: what the CPU tests compare against the REFERENCE'S OWN configuration and
construction code (imported in-process through ref_shim.py), recorded once so that the tests need no reference tree.  Per model group:

  yaml_sha256        digest of the shipped YAML group (conf/experiment/model/<name>.yaml) as parsed by
                     hyperreel_amd.config.load_model_yaml, in the canonical form of yaml_digest() (the content itself is not stored);
  state_dict_shapes  name -> shape of every tensor of the reference's LightfieldModel (nlf/models/models.py) built from that YAML
                     the way INRSystem builds it (nlf/__init__.py:355-364), i.e. the checkpoint keys;
  aabb               that model's scene box buffer (color_model.net.aabb), the one non-grid value a checkpoint load changes;
  growth             the grid schedule that model's TensorVMSplit derives (N_voxel_list, upsamp_list, update_AlphaMask_list, gridSize);

and `transform_color_all`: what utils/tensorf_utils.py:283-306 does with a per-sample (B, Z, 9) colour-transform head.

    python oracle/refgen/make_reference_facts.py

TEST INFRASTRUCTURE ONLY.
"""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import ref_shim  # noqa: E402
from hyperreel_amd import config as C  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'reference_facts.json')


def yaml_digest(cfg):
    """sha256 of a parsed model group: sorted-key JSON of its plain form (the tests digest C.model_config(name) the same way)."""
    return hashlib.sha256(json.dumps(C.to_plain(cfg), sort_keys=True).encode()).hexdigest()


def transform_color_all_facts(B=5):
    with ref_shim.cpu_mode():
        from utils.tensorf_utils import transform_color_all
    out = {'B': B}
    for Z in (1, 2, 32):
        try:
            r = transform_color_all(torch.rand(B, Z, 3), torch.rand(B, Z, 9), torch.rand(B, Z, 3))
            out[f'Z{Z}'] = {'shape': list(r.shape)}
        except RuntimeError:
            out[f'Z{Z}'] = {'raises': 'RuntimeError'}
    return out


def main():
    ref_shim.install()
    with ref_shim.cpu_mode():
        from nlf.models.models import model_dict
    models = {}
    for name in C.MODEL_NAMES:
        ds = C.dataset_scalars(name)
        yml = yaml_digest(C.load_model_yaml(f'{ref_shim.REF}/conf/experiment/model/{name}.yaml'))
        with ref_shim.cpu_mode():
            ref = model_dict['lightfield'](ref_shim.load_model_cfg(name), system=ref_shim.make_system(ds))
        net = ref_shim.build_reference(ref_shim.load_model_cfg(name), ds).model.color_model.net
        models[name] = {
            'yaml_sha256': yml,
            'state_dict_shapes': {k: list(v.shape) for k, v in ref.state_dict().items()},
            'aabb': ref.state_dict()['color_model.net.aabb'].tolist(),
            'growth': {'N_voxel_list': [int(v) for v in net.N_voxel_list], 'upsamp_list': [int(v) for v in net.upsamp_list],
                       'update_AlphaMask_list': [int(v) for v in net.update_AlphaMask_list],
                       'gridSize': [int(v) for v in net.gridSize.tolist()]},
        }
    facts = {'models': models, 'transform_color_all': transform_color_all_facts()}
    with open(OUT, 'w') as f:
        json.dump(facts, f, indent=1, sort_keys=True)
        f.write('\n')
    print(OUT)


if __name__ == '__main__':
    main()
