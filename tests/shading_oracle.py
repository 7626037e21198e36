"""float64 torch restatement of the per-sample colour networks of shadingMode MLP_Fea / MLP (nlf/nets/tensorf_base.py:38-69,
106-135; utils/tensorf_utils.py:232-239), written from the definition -- what tests/test_shade_host.py holds against the fixtures'
rgb64 and the host header, and tests/test_gpu_shade_unit.py's one-hot cases against the device.

  positional_encoding(p, F): q[..., i * F + j] = p[..., i] * 2^j;  cat[sin(q), cos(q)]
  MLP_Fea: in = [f, v, PE(f, fea_pe), PE(v, view_pe)]      MLP: in = [f, v, PE(v, view_pe)]      (a PE with F == 0 is left out)
  rgb = sigmoid(L4(relu(L2(relu(L0(in))))))"""
import torch


def positional_encoding(p, freqs):
    q = (p[..., None] * (2.0 ** torch.arange(freqs, dtype=p.dtype, device=p.device))).reshape(p.shape[:-1] + (freqs * p.shape[-1],))
    return torch.cat([torch.sin(q), torch.cos(q)], -1)


def encode(mode, view_pe, fea_pe, f, v):
    """(n, width) input rows of the network, in the dtype of f."""
    parts = [f, v]
    if mode == 'MLP_Fea' and fea_pe > 0:
        parts.append(positional_encoding(f, fea_pe))
    if view_pe > 0:
        parts.append(positional_encoding(v, view_pe))
    return torch.cat(parts, -1)


def width(mode, view_pe, fea_pe):
    return 27 + 3 + 2 * 3 * view_pe + (2 * 27 * fea_pe if mode == 'MLP_Fea' else 0)


def shade(mode, view_pe, fea_pe, weights, f, v):
    """weights: {'mlp.{0,2,4}.{weight,bias}': array}; f (n, 27), v (n, 3) -> rgb (n, 3), all in float64."""
    t = lambda a: torch.as_tensor(a).double()
    x = encode(mode, view_pe, fea_pe, t(f), t(v))
    h = torch.relu(x @ t(weights['mlp.0.weight']).T + t(weights['mlp.0.bias']))
    h = torch.relu(h @ t(weights['mlp.2.weight']).T + t(weights['mlp.2.bias']))
    return torch.sigmoid(h @ t(weights['mlp.4.weight']).T + t(weights['mlp.4.bias'])).numpy()


def unit_descriptor(recipe):
    """(mode, view_pe, fea_pe, featureC) of a unit fixture's recipe (tools/make_shading_golden.py)."""
    kw = recipe['kwargs']
    mode = 'MLP_Fea' if recipe['module'] == 'MLPRender_Fea' else 'MLP'
    return mode, int(kw['viewpe']), int(kw.get('feape', 0)), int(kw['featureC'])


def shade_port(cfg, dataset, state_dict):
    """time_decode_oracle.composite_port for a model with shadingMode MLP_Fea / MLP: TorchPort (built as the SH model the 27-row basis_mat
    fits) up to the weights and the 27 appearance features of a live sample, then shade() above on them and the ray's direction."""
    import copy
    from time_decode_oracle import composite_port
    net = cfg['color']['net']
    mode, view_pe, fea_pe = net['shadingMode'], int(net.get('view_pe', 6)), int(net.get('fea_pe', 6))
    pre = 'model.color_model.net.renderModule.'
    weights = {k[len(pre):]: v for k, v in state_dict.items() if k.startswith(pre)}
    as_sh = copy.deepcopy(cfg)
    as_sh['color']['net']['shadingMode'] = 'SH'

    def colour(port, feat, t, off, viewdirs):
        return torch.from_numpy(shade(mode, view_pe, fea_pe, weights, feat.detach().numpy(), viewdirs.detach().numpy()))

    return composite_port(as_sh, dataset, state_dict, colour=colour)
