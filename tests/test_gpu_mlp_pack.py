"""The two callers of csrc/hr_mlp_pack.h seen through the kernels: the host routine (hr_pack_mlp_layer, run by pack_mlp at finalize) and
the device pack kernel (hr_pack_split_bf16_kernel, run by hr_mlp_train_forward every step) must fill the same bf16 tiles."""
import numpy as np
import pytest
import torch

from helpers import Golden

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', ['technicolor_z_plane_small', 'donerf_sphere_small'])
def test_device_packed_tiles_give_the_host_packed_head_bit_for_bit(case):
    """mlp_precision='bf16x3' forced (not the verified path: tier 0 is the host-packed bf16 tiles), a ray count that is no multiple of
    the 64-ray tile.  The raw head of hr_mlp_train_forward on the model's own parameter tensors against the head export of
    hr_render_fields: both launches run hr_mlp_tile<256, 2, 4> on bf16 tiles (the training form only adds the tap stores), so the two
    heads differ only if the two packers do.  Equality, not a tolerance."""
    from gpu_common import make_render_fn
    from hyperreel_amd import train as T
    g = Golden(case)
    fn = make_render_fn(g.cfg, g.dataset, g.state_dict, mlp_precision='bf16x3', iteration=g.iteration)
    m = fn.model
    rays = torch.from_numpy(np.ascontiguousarray(np.concatenate([g.rays, g.rays[:37]], 0), np.float32)).cuda()
    assert rays.shape[0] % 64 != 0 and rays.shape[0] > 64
    fn.eval()
    with torch.no_grad():
        host = m.render(rays, want=('head',))['head'].clone()
    assert m.mlp_precision_active() == 'bf16x3'
    fn.train()
    h, hc = m.native(), m._hc
    pred = m.embedding_model.embeddings[0]
    n_out = hc.z_channels * hc.preds_per_z
    with torch.no_grad():
        dev = T.mlp_forward_fused(h, rays, T.ray_features(h, rays, hc.mlp_in), pred.net, hc.mlp_skip_mask, n_out)
    torch.cuda.synchronize()
    host, dev = host.reshape(rays.shape[0], n_out), dev.reshape(rays.shape[0], n_out)
    assert bool(torch.isfinite(host).all()) and float(host.abs().max()) > 0
    differ = int((host.view(torch.int32) != dev.view(torch.int32)).sum())
    print(f'{case}: {differ} of {host.numel()} head words differ, max |d| {float((host - dev).abs().max()):.3e}', flush=True)
    assert differ == 0
