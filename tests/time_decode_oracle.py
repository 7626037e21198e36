"""Float64 restatement of the keyframe net's time-dependent decode modes, written from their definition (utils/tensorf_utils.py:346-456
of the reference) for tests/test_time_decode_host.py.  TEST INFRASTRUCTURE ONLY.

  basis(Linear)  = [1, t]
  basis(Fourier) = [t, cos(2 pi f s) f = 0 .. fpk - 1, sin(2 pi f s) f = 0 .. fpk - 1],  s = time_offset * K (F - 1) / F
  colour c       = relu(sum_j basis_j * feature[c nb + j] + 0.5)            RGBIdentity: |feature[c] + 0.5|
  density        = sum_j basis_j * feature_d[j]"""
import numpy as np


def nb(fourier, fpk):
    return 2 * fpk + 1 if fourier else 2


def scale(num_keyframes, num_frames):
    return num_keyframes * (num_frames - 1) / num_frames


def base_time(t, num_keyframes, num_frames):
    """get_base_time (utils/flow_utils.py:10-35) without jitter."""
    fac = scale(num_keyframes, num_frames)
    return np.round(np.clip(np.asarray(t, np.float64) * fac, 0.0, num_keyframes - 1.0) - 1e-5) / fac


def basis(fourier, fpk, t, time_offset, fac):
    """(n, nb) float64."""
    t = np.asarray(t, np.float64).reshape(-1, 1)
    if not fourier:
        return np.concatenate([np.ones_like(t), t], 1)
    s = np.asarray(time_offset, np.float64).reshape(-1, 1) * float(fac)
    f = np.arange(fpk, dtype=np.float64)[None]
    return np.concatenate([t, np.cos(2.0 * np.pi * f * s), np.sin(2.0 * np.pi * f * s)], 1)


def fold(fourier, fpk, t, time_offset, fac, weight):
    """weight (rows = groups * nb, cols) -> (n, groups, cols): sum_j basis_j * weight[g nb + j] -- the ray's decode matrix (groups 3) or
    density row (groups 1)."""
    b = basis(fourier, fpk, t, time_offset, fac)
    w = np.asarray(weight, np.float64).reshape(-1, b.shape[1], weight.shape[1])
    return np.einsum('nj,gjc->ngc', b, w)


def colour(mode, fpk, t, time_offset, fac, features):
    """features (n, 3 nb) (RGBIdentity: (n, 3)) -> (n, 3) float64."""
    x = np.asarray(features, np.float64)
    if mode == 'RGBIdentity':
        return np.abs(x + 0.5)
    b = basis(mode == 'RGBtFourier', fpk, t, time_offset, fac)
    return np.maximum((b[:, None, :] * x.reshape(x.shape[0], 3, -1)).sum(-1) + 0.5, 0.0)


def density(mode, fpk, t, time_offset, fac, features):
    """features (n, nb) -> (n,) float64, before the activation."""
    b = basis(mode == 'DensityFourier', fpk, t, time_offset, fac)
    return (b * np.asarray(features, np.float64)).sum(-1)


def time_port(cfg, dataset, state_dict):
    """oracle/torch_port.py's TorchPort (the restatement torch.autograd differentiates) for a colour mode it does not know: built as the
    RGB model the tensors fit (its decode is `features = basis_mat . components`, any row count), with `color` restated here for
    RGBtLinear / RGBtFourier / RGBIdentity from the definition above -- everything before the colour (intersection, points, density,
    weights) is TorchPort's own.  color(x, rays, ...) takes the rays for their times."""
    import copy
    import os
    import sys
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'oracle'))
    from torch_port import TorchPort
    net = cfg['color']['net']
    mode = net['shadingMode']
    K, Fr = int(dataset['num_keyframes']), int(dataset['num_frames'])
    fpk = int(net['frames_per_keyframe']) if 'frames_per_keyframe' in net else Fr // max(K, 1)
    as_rgb = copy.deepcopy(cfg)
    as_rgb['color']['net']['shadingMode'] = 'RGB'

    class TimePort(TorchPort):
        def color(self, x, rays, train=False, white_bg=None):
            o = self.o
            pts = x['points']
            B, Z = pts.shape[:2]
            dist = x['distances'].reshape(B, Z)
            deltas = torch.cat([dist[:, 1:] - dist[:, :-1], torch.full((B, 1), 1e10)], 1)
            valid = ~(((self.aabb[0] > pts) | (pts > self.aabb[1])).any(-1)) & (dist > 0)
            pn = (pts - self.aabb[0]) * self.inv_size - 1
            if o.video:
                pn = torch.cat([pn, (x['base_times'] * o.tsf + o.tpo) * 2 - 1], -1)
            sigma = torch.zeros(B, Z)
            if valid.any():
                f = self._feat(self.d_a, self.d_b, pn[valid]).sum(0)
                sigma[valid] = F.relu(f) if o.act == 'relu' else (f.abs() if o.act == 'relu_abs' else F.softplus(f + float(o.density_shift)))
            alpha = 1.0 - torch.exp(-sigma * (deltas * float(o.distance_scale)))
            T = torch.cumprod(torch.cat([torch.ones(B, 1), 1.0 - alpha + 1e-10], -1), -1)
            weight = alpha * T[:, :-1]
            app = weight > float(o.thr)
            rgb = torch.zeros(B, Z, 3)
            if app.any():
                feat = F.linear(self._feat(self.a_a, self.a_b, pn[app]).T, self.basis)
                if mode == 'RGBIdentity':
                    col = torch.abs(feat + 0.5)
                else:
                    t = rays[:, -1:].expand(B, Z)[app][:, None]
                    if mode == 'RGBtLinear':
                        b = torch.cat([torch.ones_like(t), t], -1)
                    else:
                        s = (rays[:, -1:] - x['base_times'].reshape(B, Z)[:, :1]).expand(B, Z)[app][:, None] * (K * (Fr - 1) / Fr)
                        fr = torch.arange(fpk, dtype=t.dtype)[None]
                        b = torch.cat([t, torch.cos(s * fr * 2 * np.pi), torch.sin(s * fr * 2 * np.pi)], -1)
                    col = torch.relu((b[:, None] * feat.view(-1, 3, b.shape[1])).sum(-1) + 0.5)
                rgb[app] = col
            if 'color_scale' in x:
                rgb = rgb * (x['color_scale'] + 1.0) + x['color_shift']
            out = (weight[..., None] * rgb).sum(-2)
            if o.white_bg if white_bg is None else white_bg:
                out = out + (1.0 - weight.sum(-1)[:, None])
            return out if train else out.clamp(0, 1)

    return TimePort(as_rgb, dataset, state_dict)
