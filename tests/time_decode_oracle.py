"""Float64 restatement of the keyframe net's time-dependent decode modes, written from their definition (utils/tensorf_utils.py:346-456
of the reference) for tests/test_time_decode_host.py, and the whole-model restatement built on it (time_port, at the bottom) that
the training tests differentiate and tests/test_gpu_render_dispatch.py renders every instantiation of the time kernel against.  TEST
INFRASTRUCTURE ONLY.

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


def basis_t(fourier, fpk, t, time_offset, fac):
    """basis() on torch tensors (n, 1) -> (n, nb), in their dtype: what autograd differentiates."""
    import torch
    if not fourier:
        return torch.cat([torch.ones_like(t), t], -1)
    s = time_offset * float(fac)
    f = torch.arange(fpk, dtype=t.dtype)[None]
    return torch.cat([t, torch.cos(s * f * 2 * np.pi), torch.sin(s * f * 2 * np.pi)], -1)


def composite_port(cfg, dataset, state_dict, density=None, colour=None):
    """oracle/torch_port.py's TorchPort (the restatement torch.autograd differentiates) with the two per-sample functions a mode replaces
    handed in -- everything else (intersection, points, grid features, weights, per-sample and per-ray colour transforms, background,
    clamp) is TorchPort's own statements:
      density(port, comps (C, n), t (n, 1), off (n, 1)) -> (n,) before the activation      None: comps.sum(0), every other model's
      colour(port, feat (n, rows of basis_mat), t, off, viewdirs (n, 3)) -> (n, 3)         None: TorchPort's RGB / SH
    t: the sample's ray time, off: t minus the ray's keyframe time (zeros on a static net).  `cfg` is what HyperReelOracle is built from: a
    shading it knows (RGB, or SH with 27 rows) and the plain density.  color(x, rays, ...) takes the rays for their times; fields(rays)
    returns what the device tests compare."""
    import os
    import sys
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'oracle'))
    from hyperreel_oracle import C0, C1, C2
    from torch_port import TorchPort

    class Port(TorchPort):
        def composite(self, x, rays, train=False, white_bg=None):
            o = self.o
            pts = x['points']
            B, Z = pts.shape[:2]
            dist = x['distances'].reshape(B, Z)
            deltas = torch.cat([dist[:, 1:] - dist[:, :-1], torch.full((B, 1), 1e10)], 1)
            valid = ~(((self.aabb[0] > pts) | (pts > self.aabb[1])).any(-1)) & (dist > 0)
            pn = (pts - self.aabb[0]) * self.inv_size - 1
            t = rays[:, -1:].expand(B, Z)
            off = torch.zeros(B, Z)
            if o.video:
                pn = torch.cat([pn, (x['base_times'] * o.tsf + o.tpo) * 2 - 1], -1)
                off = t - x['base_times'].reshape(B, Z)
            sigma, pre = torch.zeros(B, Z), torch.zeros(B, Z)
            if valid.any():
                comps = self._feat(self.d_a, self.d_b, pn[valid])
                f = comps.sum(0) if density is None else density(self, comps, t[valid][:, None], off[valid][:, None])
                pre[valid] = f
                sigma[valid] = F.relu(f) if o.act == 'relu' else (f.abs() if o.act == 'relu_abs' else F.softplus(f + float(o.density_shift)))
            alpha = 1.0 - torch.exp(-sigma * (deltas * float(o.distance_scale)))
            T = torch.cumprod(torch.cat([torch.ones(B, 1), 1.0 - alpha + 1e-10], -1), -1)
            weight = alpha * T[:, :-1]
            app = weight > float(o.thr)
            rgb = torch.zeros(B, Z, 3)
            if app.any():
                feat = F.linear(self._feat(self.a_a, self.a_b, pn[app]).T, self.basis)
                d = x['viewdirs'][app]
                if colour is not None:
                    col = colour(self, feat, t[app][:, None], off[app][:, None], d)
                elif o.shading == 'RGB':
                    col = torch.sigmoid(feat)
                else:
                    xx, yy, zz = d[:, 0], d[:, 1], d[:, 2]
                    sh = torch.stack([torch.full_like(xx, C0), -C1 * yy, C1 * zz, -C1 * xx, C2[0] * xx * yy, C2[1] * yy * zz,
                                      C2[2] * (2.0 * zz * zz - xx * xx - yy * yy), C2[3] * xx * zz, C2[4] * (xx * xx - yy * yy)], -1)
                    col = torch.relu((sh[:, None] * feat.view(-1, 3, 9)).sum(-1) + 0.5)
                rgb[app] = col.to(rgb.dtype)
            if 'color_scale' in x:
                rgb = rgb * (x['color_scale'] + 1.0) + x['color_shift']
            out = (weight[..., None] * rgb).sum(-2)
            if o.white_bg if white_bg is None else white_bg:
                out = out + (1.0 - weight.sum(-1)[:, None])
            if 'color_scale_global' in x:
                out = out * (x['color_scale_global'][:, 0, :] + 1.0) + x['color_shift_global'][:, 0, :]
            elif 'color_transform_global' in x:
                M = x['color_transform_global'].reshape(B, -1, 3, 3)[:, 0]
                out = out + (M * out[:, None, :]).sum(-1) + x['color_shift_global'].reshape(B, -1, 3)[:, 0]
            return (out if train else out.clamp(0, 1)), weight, pre, valid

        def color(self, x, rays, train=False, white_bg=None):
            return self.composite(x, rays, train, white_bg)[0]

        @torch.no_grad()
        def fields(self, rays):
            """{'rgb' (B, 3), 'render_weights' (B, Z), 'distances' (B, Z), 'sigma_pre' (B, Z): the density before its activation, 'valid' (B, Z): where it was
            evaluated} as numpy arrays."""
            rays = torch.from_numpy(np.ascontiguousarray(rays, np.float32))
            x = self.embed(rays)
            rgb, weight, pre, valid = self.composite(x, rays)
            return {'rgb': rgb.numpy(), 'render_weights': weight.numpy(), 'distances': x['distances'].reshape(weight.shape).numpy(),
                    'sigma_pre': pre.numpy(), 'valid': valid.numpy()}

    return Port(cfg, dataset, state_dict)


def time_port(cfg, dataset, state_dict):
    """composite_port for a model with a time-dependent decode mode: built as the RGB / SH model the tensors fit (its decode is `features =
    basis_mat . components`, any row count) with the plain density, the colour restated here for RGBtLinear / RGBtFourier / RGBIdentity
    and the density for DensityLinear / DensityFourier -- `sum_j basis_j * (basis_mat_density . components)_j`, density() above on
    tensors -- from the definitions at the top of the file."""
    import copy
    import torch
    import torch.nn.functional as F
    net = cfg['color']['net']
    mode, dmode = net['shadingMode'], net.get('densityMode', 'Density')
    K, Fr = int(dataset['num_keyframes']), int(dataset['num_frames'])
    fpk = int(net['frames_per_keyframe']) if 'frames_per_keyframe' in net else Fr // max(K, 1)
    fac = scale(K, Fr)
    plain = copy.deepcopy(cfg)
    plain['color']['net']['densityMode'] = 'Density'
    if mode not in ('RGB', 'SH'):
        plain['color']['net']['shadingMode'] = 'RGB'

    def colour(port, feat, t, off, viewdirs):
        if mode == 'RGBIdentity':
            return torch.abs(feat + 0.5)
        b = basis_t(mode == 'RGBtFourier', fpk, t, off, fac)
        return torch.relu((b[:, None] * feat.view(-1, 3, b.shape[1])).sum(-1) + 0.5)

    def dens(port, comps, t, off):
        w = torch.from_numpy(np.ascontiguousarray(state_dict['model.color_model.net.basis_mat_density.weight'], np.float32))
        return (basis_t(dmode == 'DensityFourier', fpk, t, off, fac) * F.linear(comps.T, w)).sum(-1)

    return composite_port(plain, dataset, state_dict, density=None if dmode == 'Density' else dens, colour=None if mode in ('RGB', 'SH') else colour)
