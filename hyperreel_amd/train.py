"""Training step on the HIP device.

What INRSystem.training_step (nlf/__init__.py:634-709) gets from torch.autograd for the reference, split the way the
hardware wants it:
  * ray parameterisation + positional encoding: hr_train_features (no parameters, no gradient);
  * the sample-prediction MLP: `HipLinear`, a torch.autograd.Function over hr_linear_forward / hr_linear_backward -- every
    Linear (+ LeakyReLU) and its dgrad / wgrad / bias gradient as split-precision MFMA GEMMs (csrc/train_gemm_kernel.hip)
    on the reference-named nn.Linear parameters, exactly BaseMLP.forward (nlf/nets/mlp.py:159-172); torch only concatenates
    the skip layer's input;
  * everything after the MLP (head activations, intersection, sort, contraction, offsets / flow, VM gather, density,
    compositing, colour): one hand-written HIP forward and one backward kernel behind `SampleStage`, a
    torch.autograd.Function over the C ABI (hr_train_forward / hr_train_backward).
Gradients arrive on the reference's own parameters (planes, lines, basis_mat, MLP weights), so the reference's optimizers,
schedulers and regularizers apply unchanged.  There is no CPU path: the tensors must live on the HIP device.
`GraphedStep` records the whole step -- the batch draw, forward, loss, backward and Adam -- once and replays it.
"""
import ctypes as C

import torch

from . import lib as _lib


def _tensors_struct(groups, basis, table=None):
    """groups: 4 lists of 3 tensors (density a, density b, app a, app b) -> hr_train_tensors."""
    t = _lib.hr_train_tensors()
    for name, grp in zip(('density_a', 'density_b', 'app_a', 'app_b'), groups):
        arr = getattr(t, name)
        for j in range(3):
            arr[j] = grp[j].data_ptr() if grp[j].numel() > 0 else None
    t.basis = basis.data_ptr() if basis.numel() > 0 else None
    t.color_table = table.data_ptr() if table is not None and table.numel() > 0 else None
    return t


class SampleStage(torch.autograd.Function):
    """rgb = f(head; planes, lines, basis_mat), not clamped (training mode, tensorf_no_sample.py:246).
    Inputs after `white_bg`: basis_mat.weight, then the 12 grid tensors in the order density a[0..2], density b[0..2],
    app a[0..2], app b[0..2] (a = plane | plane_space, b = line | plane_time), then -- only for models with a per-camera
    colour table (ColorTransformEmbedding, read with dataset.val_all) -- its `color_embedding`."""

    poison_outputs = False # tests: gradient buffers start as NaN instead of uninitialised memory

    @staticmethod
    def run(ctx, fields_z, handle, rays, head, white_bg, basis, tensors):
        """The forward of both stages -> (rgb, fields): fields is None, or with fields_z = z_channels the forward's own per-sample
        (distances, points, render_weights) (hr_train_forward_fields)."""
        grids, table = tensors[:12], (tensors[12] if len(tensors) > 12 else None)
        dev = rays.device
        if dev.type != 'cuda' or head.device != dev:
            raise RuntimeError('SampleStage runs on the HIP device; there is no CPU path')
        rays, head = rays.contiguous().float(), head.contiguous().float()
        vals = [g.detach().contiguous() for g in grids]
        groups = [vals[0:3], vals[3:6], vals[6:9], vals[9:12]]
        params = _tensors_struct(groups, basis.detach().contiguous(), None if table is None else table.detach().contiguous())
        B = rays.shape[0]
        rgb = torch.empty((B, 3), dtype=torch.float32, device=dev)
        fields = None
        if fields_z:
            # the forward's own per-sample values: what a field-consuming regulariser reads, without a second pass through the inference kernels
            from .plan import hr_fields
            Z = int(fields_z)
            f = hr_fields()
            fields = tuple(torch.zeros(shape, dtype=torch.float32, device=dev) for shape in ((B, Z), (B, Z, 3), (B, Z)))
            f.distances_dev, f.points_dev, f.weights_dev = (t.data_ptr() for t in fields)
            _lib.call('hr_train_forward_fields', handle, C.byref(params), rays, head, B, int(bool(white_bg)), rgb, C.byref(f), _lib.stream(dev), device=dev)
        else:
            _lib.call('hr_train_forward', handle, C.byref(params), rays, head, B, int(bool(white_bg)), rgb, _lib.stream(dev), device=dev)
        ctx.handle, ctx.white_bg = handle, int(bool(white_bg))
        ctx.has_table = table is not None
        ctx.save_for_backward(rays, head, basis, *tensors)
        return rgb, fields

    @staticmethod
    def forward(ctx, handle, rays, head, white_bg, basis, *tensors):
        return SampleStage.run(ctx, None, handle, rays, head, white_bg, basis, tensors)[0]

    @staticmethod
    def backward(ctx, d_rgb):
        rays, head, basis, *tensors = ctx.saved_tensors
        grids, table = tensors[:12], (tensors[12] if ctx.has_table else None)
        dev = rays.device
        d_rgb = d_rgb.contiguous().float()
        d_head = torch.empty_like(head)
        # hr_train_backward writes every element of every gradient tensor (the re-layout of the packed texel gradients covers the whole
        # (C, H, W) tensors; basis_mat's and the colour table's accumulators are cleared by the library on the stream): no zero fill here --
        # thirteen fills of 48 MB per step otherwise.  `poison_outputs` (tests) fills them with NaN instead, which must not survive.
        fresh = (lambda t: torch.full_like(t, float('nan'), memory_format=torch.contiguous_format)) if SampleStage.poison_outputs else \
            (lambda t: torch.empty_like(t, memory_format=torch.contiguous_format))
        g_grids = [fresh(g) for g in grids]
        g_basis = fresh(basis)
        g_table = None if table is None else fresh(table)
        gt = _tensors_struct([g_grids[0:3], g_grids[3:6], g_grids[6:9], g_grids[9:12]], g_basis, g_table)
        if g_basis.numel() == 0:
            raise RuntimeError('basis_mat has no columns')
        _lib.call('hr_train_backward', ctx.handle, rays, head, d_rgb, rays.shape[0], ctx.white_bg, d_head, C.byref(gt), _lib.stream(dev), device=dev)
        return (None, None, d_head, None, g_basis, *g_grids) + (() if table is None else (g_table,))


class SampleStageFields(torch.autograd.Function):
    """SampleStage that also returns its forward's per-sample fields: apply(z_channels, <SampleStage's arguments>) ->
    (rgb, distances (B, Z), points (B, Z, 3), render_weights (B, Z)); the three fields carry no gradient."""

    @staticmethod
    def forward(ctx, z_channels, *args):
        rgb, fields = SampleStage.run(ctx, z_channels, *args[:5], args[5:])
        ctx.mark_non_differentiable(*fields)
        return (rgb, *fields)

    @staticmethod
    def backward(ctx, d_rgb, *_):
        return (None, *SampleStage.backward(ctx, d_rgb))


class CoarseRows(torch.autograd.Function):
    """Coarse level of a point_prediction cascade (nlf/embedding/point.py:137-203): raw head of the ray MLP (B, Zc * Pc) ->
    the point MLP's input rows (B * Zc, row_dim), and the gradient back (hr_train_rows_forward / _backward)."""

    @staticmethod
    def forward(ctx, handle, rays, head, n_rows_per_ray, row_dim):
        dev = rays.device
        if dev.type != 'cuda' or head.device != dev:
            raise RuntimeError('CoarseRows runs on the HIP device; there is no CPU path')
        rays, head = rays.contiguous().float(), head.contiguous().float()
        rows = torch.empty((rays.shape[0] * int(n_rows_per_ray), int(row_dim)), dtype=torch.float32, device=dev)
        _lib.call('hr_train_rows_forward', handle, rays, head, rays.shape[0], rows, _lib.stream(dev), device=dev)
        ctx.handle = handle
        ctx.save_for_backward(rays, head)
        ctx.shape = tuple(rows.shape)
        return rows

    @staticmethod
    def backward(ctx, d_rows):
        rays, head = ctx.saved_tensors
        dev = rays.device
        d_rows = d_rows.contiguous().float()
        scratch = torch.empty(ctx.shape, dtype=torch.float32, device=dev)
        d_head = torch.empty_like(head)
        _lib.call('hr_train_rows_backward', ctx.handle, rays, head, d_rows, rays.shape[0], scratch, d_head, _lib.stream(dev), device=dev)
        return None, None, d_head, None, None


def row_features(hc, rows):
    """Input of a cascade's point MLP: the identity parameterisation + positional encoding of its rows (nlf/pe.py:53-66,
    210-221), the arithmetic of hr_ray_features in torch ops because the rows carry a gradient (their point columns)."""
    cols = []
    for g in range(hc.n_groups):
        pg = hc.groups[g]
        if pg.fn != 0:
            raise NotImplementedError('point_prediction with a non-identity parameterisation of its inputs')
        x = rows[:, pg.start:pg.end]
        out = [x] if (pg.pe_type in (0, 2) or not pg.pe_exclude_identity) else []
        if pg.pe_type == 1:                                   # windowed: [sin(all), cos(all)] per frequency
            f = 1.0
            for j in range(pg.pe_n_freqs):
                f = f * pg.pe_freq_mult
                w = float(pg.pe_weight[j])
                out += [w * torch.sin(pg.pe_base_mult * f * x), w * torch.cos(pg.pe_base_mult * f * x)]
        elif pg.pe_type == 2:                                 # basic: [x, sin(f_j x_i) (i-major), cos(f_j x_i)]
            fr = torch.tensor([pg.pe_freq_mult ** (j + 1) for j in range(pg.pe_n_freqs)], dtype=x.dtype, device=x.device)
            cur = (fr[None, None] * x[..., None]).reshape(x.shape[0], -1)
            out += [torch.sin(cur), torch.cos(cur)]
        cols.append(torch.cat(out, -1))
    return torch.cat(cols, -1)


def ray_features(handle, rays, mlp_in):
    """rays (B, ray_dim) -> MLP input (B, mlp_in): RayParam + positional encoding on the device."""
    rays = rays.contiguous().float()
    out = torch.empty((rays.shape[0], int(mlp_in)), dtype=torch.float32, device=rays.device)
    _lib.call('hr_train_features', handle, rays, rays.shape[0], out, _lib.stream(rays.device), device=rays.device)
    return out


class HipLinear(torch.autograd.Function):
    """y = LeakyReLU_slope(x W^T + b) (slope < 0: no activation) and its backward on the matrix cores
    (hr_linear_forward / hr_linear_backward: three bf16 MFMA products per fp32 GEMM, fp32 accumulation)."""

    @staticmethod
    def forward(ctx, x, weight, bias, slope):
        dev = x.device
        if dev.type != 'cuda' or weight.device != dev:
            raise RuntimeError('HipLinear runs on the HIP device; there is no CPU path')
        x = x.float()
        if x.stride(-1) != 1:
            x = x.contiguous()
        w, b = weight.detach().contiguous().float(), bias.detach().contiguous().float()
        rows, fin, fout = x.shape[0], x.shape[1], w.shape[0]
        y = torch.empty((rows, fout), dtype=torch.float32, device=dev)
        _lib.call('hr_linear_forward', x, x.stride(0), rows, fin, w, b, fout, float(slope), y, fout, _lib.stream(dev), device=dev)
        ctx.slope = float(slope)
        ctx.save_for_backward(x, w, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        dev = x.device
        dy = dy.contiguous().float()
        rows, fin, fout = x.shape[0], x.shape[1], w.shape[0]
        dx = torch.empty((rows, fin), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w)
        db = torch.empty((fout,), dtype=torch.float32, device=dev)
        ws = torch.empty((max(int(_lib.call('hr_linear_workspace', rows, fin, fout)) // 4, 1),), dtype=torch.float32, device=dev)
        _lib.call('hr_linear_backward', x, x.stride(0), w, y if ctx.slope >= 0 else None, fout, dy, fout, rows, fin, fout, ctx.slope, dx, fin, dw, db,
                  ws, _lib.stream(dev), device=dev)
        return dx, dw, db, None


class HipMLP(torch.autograd.Function):
    """BaseMLP.forward (nlf/nets/mlp.py:159-172) of the ray MLP as ONE launch (hr_mlp_train_forward: the render path's six-layer MFMA
    kernel on the current parameter values, which also leaves every hidden layer's output in HBM), and its backward layer by layer on
    the matrix cores (hr_linear_backward, as HipLinear).  Inputs: the model handle, rays, the MLP's input features (for layer 0's
    weight gradient), the skip mask, then weight_0, bias_0, weight_1, ... as the reference names them."""

    @staticmethod
    def forward(ctx, handle, rays, feats, skip_mask, n_out, *params):
        dev = rays.device
        nl = len(params) // 2
        ws = [p.detach().contiguous().float() for p in params[0::2]]
        bs = [p.detach().contiguous().float() for p in params[1::2]]
        n, fin = rays.shape[0], feats.shape[1]
        hidden = ws[0].shape[0]
        # x[l]: the input of layer l.  x[0] = feats; x[l] = the output of layer l - 1, behind a copy of feats where layer l is a skip layer
        xs = [feats]
        acts, lds, offs = [], [], []
        for l in range(1, nl):
            skip = (skip_mask >> l) & 1
            # a skip layer's input row is [feats | hidden]; two pad columns in FRONT of it keep the hidden part (what the kernels read
            # and write in 16-byte pieces) on a 16-byte boundary
            lead = (fin + ((-fin) % 4)) if skip else 0
            buf = torch.empty((n, lead + hidden), dtype=torch.float32, device=dev)
            x = buf[:, lead - fin:] if skip else buf
            if skip:
                x[:, :fin] = feats
            xs.append(x)
            acts.append(buf); lds.append(lead + hidden); offs.append(lead)
        head = torch.empty((n, int(n_out)), dtype=torch.float32, device=dev)
        PV = C.c_void_p * nl
        wv, bv = PV(*[w.data_ptr() for w in ws]), PV(*[b.data_ptr() for b in bs])
        av = PV(*([a.data_ptr() for a in acts] + [0]))
        ldv = (C.c_int64 * nl)(*(lds + [0]))
        offv = (C.c_int32 * nl)(*(offs + [0]))
        _lib.call('hr_mlp_train_forward', handle, wv, bv, rays, n, av, ldv, offv, head, _lib.stream(dev), device=dev)
        ctx.skip_mask, ctx.nl, ctx.fin, ctx.hidden = int(skip_mask), nl, fin, hidden
        ctx.save_for_backward(*xs, *ws)
        return head

    @staticmethod
    def backward(ctx, dhead):
        nl, fin, hidden = ctx.nl, ctx.fin, ctx.hidden
        xs, ws = ctx.saved_tensors[:nl], ctx.saved_tensors[nl:]
        dev = dhead.device
        dy = dhead.contiguous().float()
        dy_ptr, ld_dy = dy.data_ptr(), dy.shape[1]
        grads = [None] * (2 * nl)
        rows = xs[0].shape[0]
        keep = []
        with torch.cuda.device(dev):
            for l in range(nl - 1, -1, -1):
                x, w = xs[l], ws[l]
                fout, fin_l = w.shape[0], w.shape[1]
                last = (l == nl - 1)
                # y of layer l (the LeakyReLU mask) = the hidden part of x[l + 1]
                if last:
                    y_ptr, ldy = 0, fout
                else:
                    nxt = xs[l + 1]
                    y_ptr, ldy = nxt.data_ptr() + 4 * (nxt.shape[1] - hidden), nxt.stride(0)
                dx = None
                if l > 0:                               # same row shape as x[l]: the hidden columns of dx stay 16-byte aligned
                    lead = x.stride(0) - hidden
                    dxb = torch.empty((rows, lead + hidden), dtype=torch.float32, device=dev)
                    dx = dxb[:, lead + hidden - fin_l:]
                dw = torch.empty_like(w)
                db = torch.empty((fout,), dtype=torch.float32, device=dev)
                wsb = torch.empty((max(int(_lib.call('hr_linear_workspace', rows, fin_l, fout)) // 4, 1),), dtype=torch.float32, device=dev)
                _lib.call('hr_linear_backward', x, x.stride(0), w, C.c_void_p(y_ptr), ldy, C.c_void_p(dy_ptr), ld_dy, rows, fin_l, fout,
                          -1.0 if last else 0.01, dx, dx.stride(0) if dx is not None else fin_l, dw, db, wsb, _lib.stream(dev))
                grads[2 * l], grads[2 * l + 1] = dw, db
                keep.append((dx, wsb))
                if dx is not None:                      # upstream of layer l - 1: the hidden columns of dx (a skip layer's first fin columns belong to the input)
                    dy_ptr, ld_dy = dx.data_ptr() + 4 * (fin_l - hidden), dx.stride(0)
        return (None, None, None, None, None, *grads)


def mlp_forward_fused(handle, rays, feats, net, skip_mask, n_out):
    """mlp_forward below through HipMLP: one forward launch.  The caller checks that the model qualifies (hidden width 256, no cascade)."""
    n = len(net.layers)
    params = []
    for i, layer in enumerate(net.layers):
        lin = layer[0] if i < n - 1 else layer
        params += [lin.weight, lin.bias]
    return HipMLP.apply(handle, rays, feats, int(skip_mask), int(n_out), *params)


def mlp_forward(net, x, skip_mask):
    """BaseMLP.forward (nlf/nets/mlp.py:159-172) on the reference-named parameters: Linear + LeakyReLU(0.01), the
    input concatenated in front of the activations at the skip layers, no activation after the last Linear."""
    inp = x
    n = len(net.layers)
    for i, layer in enumerate(net.layers):
        lin = layer[0] if i < n - 1 else layer
        if (skip_mask >> i) & 1:
            x = torch.cat([inp, x], -1)
        x = HipLinear.apply(x, lin.weight, lin.bias, 0.01 if i < n - 1 else -1.0)
    return x


def grid_parameters(net):
    """The 12 grid tensors of a HostTensorVM in SampleStage's order."""
    if net.video:
        groups = (net.density_plane_space, net.density_plane_time, net.app_plane_space, net.app_plane_time)
    else:
        groups = (net.density_plane, net.density_line, net.app_plane, net.app_line)
    return [p for grp in groups for p in grp]


class PlaneReg(torch.autograd.Function):
    """(1, C, H, W) plane -> [sum of squared vertical differences, sum of squared horizontal differences, sum |x|] in one
    pass (hr_plane_reg_forward); the backward is one elementwise kernel driven by the upstream gradient on the device."""

    @staticmethod
    def forward(ctx, plane):
        if plane.device.type != 'cuda':
            raise RuntimeError('PlaneReg runs on the HIP device; there is no CPU path')
        x = plane.detach().contiguous().float()
        _, c, h, w = x.shape
        sums = torch.zeros(3, dtype=torch.float32, device=x.device)
        _lib.call('hr_plane_reg_forward', x, c, h, w, sums, _lib.stream(x.device), device=x.device)
        ctx.save_for_backward(x)
        return sums

    @staticmethod
    def backward(ctx, d_sums):
        (x,) = ctx.saved_tensors
        _, c, h, w = x.shape
        coef = d_sums.contiguous().float()
        grad = torch.empty_like(x)
        _lib.call('hr_plane_reg_backward', x, c, h, w, coef, grad, _lib.stream(x.device), device=x.device)
        return grad


def tv_loss(plane, weight=1.0):
    """TVLoss.forward (nlf/regularizers/tensorf.py:19-31) of one plane."""
    b, c, h, w = plane.shape
    s = PlaneReg.apply(plane)
    return weight * 2 * (s[0] / (c * (h - 1) * w) + s[1] / (c * h * (w - 1))) / b


def l1_mean(plane):
    """torch.mean(torch.abs(plane)) (density_L1, nlf/nets/tensorf_base.py:1024-1035)."""
    return PlaneReg.apply(plane)[2] / plane.numel()


def background_coin(seed, step):
    """True when training step `step` of `seed` composites over white under Model.set_background_coin / GraphedStep(white_bg='coin'): the
    library's own hr_background_coin (csrc/hr_sample_rng.h), evaluated on the host."""
    m = 0xFFFFFFFFFFFFFFFF
    return bool(_lib.call('hr_train_background_coin', int(seed) & m, int(step) & m))


class HipTensoRFRegularizer:
    """The reference's TensoRF regulariser (nlf/regularizers/tensorf.py:35-96 on BaseRegularizer, nlf/regularizers/base.py:146-168) as ONE
    device call per step (hr_tensorf_reg): value and gradient of density_L1, TV_loss_density and TV_loss_app over every plane and line
    `net._reg_planes()` names, the gradient added into the parameters' .grad.

        reg = HipTensoRFRegularizer(model, cfg, steps_per_epoch)
        reg.set_iter(i); reg.sync()         # host: this iteration's three weights; device: written when they changed
        loss.backward(); value = reg.accumulate()

    cfg: the reference's regulariser group (conf/experiment/regularizers/tensorf/*.yaml: update_AlphaMask_list, lr_decay_target_ratio,
    n_iters, total_num_tv_iters, L1_weight_initial, L1_weight_rest, TV_weight_density, TV_weight_app; optional wait_iters, stop_iters,
    warmup_iters, and `weight`: a float or {type: exponential_decay, start, decay, num_epochs}).  steps_per_epoch: the reference's
    len(train_dataset) // cur_batch_size.

    What changes with the iteration lives in three floats on the device -- what the step multiplies L1, density TV and appearance TV by,
    loss_weight() included -- so a recorded step that calls accumulate() follows set_iter() / sync() on every replay.  As the reference:
    TV is weighted by the CONSTANT cfg.TV_weight_* (the decayed copies only gate `> 0`, which they stay); with both TV weights positive
    the density TV term counts TWICE (`loss_tv = loss_tv + ...; total_loss += loss_tv`, tensorf.py:79-87); the L1 weight switches when
    set_iter sees cur_iter == update_AlphaMask_list[0], and stays.  TV_weight_density <= 0 < TV_weight_app, where the reference raises
    NameError (loss_tv is unbound), is refused here."""

    SLOT_L1, SLOT_TV_DENSITY, SLOT_TV_APP = 0, 1, 2

    def __init__(self, model, cfg, steps_per_epoch):
        import numpy as np
        get = lambda k, d: cfg[k] if k in cfg else d
        self.model, self.cfg, self.steps_per_epoch = model, cfg, int(steps_per_epoch)
        self.weight = get('weight', 0.0)
        self.wait_iters, self.warmup_iters, self.stop_iters = get('wait_iters', 0), get('warmup_iters', 0), get('stop_iters', float('inf'))
        self.update_AlphaMask_list = list(cfg['update_AlphaMask_list'])
        self.total_num_tv_iters = cfg['total_num_tv_iters'] if 'total_num_tv_iters' in cfg else \
            int(np.round((np.log(1e-4) / np.log(cfg['lr_decay_target_ratio'])) * cfg['n_iters']))
        self.L1_reg_weight = cfg['L1_weight_initial']
        self.TV_weight_density, self.TV_weight_app = cfg['TV_weight_density'], cfg['TV_weight_app']
        if self.TV_weight_app > 0 and not self.TV_weight_density > 0:
            raise ValueError('HipTensoRFRegularizer: TV_weight_density <= 0 with TV_weight_app > 0 -- the reference raises NameError on this '
                             'combination (tensorf.py:86 reads loss_tv, which only the density branch binds); set TV_weight_density > 0 or TV_weight_app to 0')
        if not isinstance(self.weight, float) and not (hasattr(self.weight, 'keys') and self.weight['type'] == 'exponential_decay'):
            raise ValueError(f'HipTensoRFRegularizer: weight must be a float or an exponential_decay group, not {self.weight!r}')
        self.cur_iter = 0 - self.wait_iters
        self.weights = self._weights()
        self._dev = self._synced = self._plan = self._plan_key = self._grad_key = None

    # -- host: the reference's schedule, expression for expression
    def loss_weight(self):
        """base.py:154-165."""
        import numpy as np
        if isinstance(self.weight, float):
            return self.weight
        weight_num_iters = self.weight['num_epochs'] * self.steps_per_epoch
        exponent = self.cur_iter / weight_num_iters
        return self.weight['start'] * np.power(self.weight['decay'], exponent)

    def warming_up(self):
        return self.cur_iter < self.warmup_iters

    def _weights(self):
        """(L1, density TV, appearance TV): what multiplies the three unweighted terms in `loss(...) * loss_weight()` (base.py:146-152,
        tensorf.py:57-89), as Python floats (doubles)."""
        if self.cur_iter < 0 or self.cur_iter >= self.stop_iters:
            return (0.0, 0.0, 0.0)
        lw = float(self.loss_weight())
        l1 = self.L1_reg_weight if self.L1_reg_weight > 0 else 0.0
        tvd = tva = 0.0
        if not self.cur_iter > self.total_num_tv_iters:
            if self.TV_weight_density > 0:
                tvd = self.TV_weight_density
            if self.TV_weight_app > 0:
                tva = self.TV_weight_app
                tvd = tvd + tvd                    # loss_tv carries the density term into the second `total_loss + loss_tv`
        return (l1 * lw, tvd * lw, tva * lw)

    def set_iter(self, i):
        self.cur_iter = i - self.wait_iters
        if len(self.update_AlphaMask_list) > 0 and self.cur_iter == self.update_AlphaMask_list[0]:
            self.L1_reg_weight = self.cfg['L1_weight_rest']
        self.weights = self._weights()

    def terms(self):
        """The descriptor table without pointers: [(parameter, kh, kw, kl, slot_h, slot_w, slot_l)] over net._reg_planes(), with the skip
        rules of density_L1 / TV_loss_density / TV_loss_app (models.py) and the reference's static factors formed in double."""
        net = self.model.color_model.net
        da, db, aa = net._reg_planes()
        out = []
        for i in range(3):
            has_l1 = da[i].shape[1] != 0
            tv_d = not (da[i].shape[1] == 0 or (net.video and db[i].shape[1] == 0))
            tv_a = not ((aa[i].shape[1] == 0) if not net.video else (da[i].shape[1] == 0 or db[i].shape[1] == 0))
            for p, l1, tv in ((da[i], has_l1, self.SLOT_TV_DENSITY if tv_d else -1), (db[i], has_l1, -1), (aa[i], False, self.SLOT_TV_APP if tv_a else -1)):
                if not l1 and tv < 0:
                    continue
                b, c, h, w = p.shape
                if b != 1:
                    raise ValueError(f'HipTensoRFRegularizer: a plane of batch size {b}')
                if tv >= 0 and c > 0 and (h < 2 or w < 2):
                    raise ValueError(f'HipTensoRFRegularizer: total variation of a {h} x {w} plane (the reference divides by a zero count)')
                kh = 1e-2 * 2 / (c * (h - 1) * w) if tv >= 0 and c > 0 else 0.0
                kw = 1e-2 * 2 / (c * h * (w - 1)) if tv >= 0 and c > 0 else 0.0
                kl = 1.0 / (c * h * w) if l1 and c > 0 else 0.0
                out.append((p, kh, kw, kl, tv, tv, self.SLOT_L1 if l1 else -1))
        return out

    # -- device
    def sync(self):
        """Writes the three weights to the device floats accumulate() reads, ordered on the current stream, when they changed since the
        last call.  Not inside a capture (a recorded copy would replay one value).  The device holds float32."""
        w = tuple(float(v) for v in self.weights)
        if self._dev is not None and w == self._synced:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('HipTensoRFRegularizer.sync inside a graph capture: call it before each replay instead')
        if self._dev is None:
            dev = next(self.model.parameters()).device
            if dev.type != 'cuda':
                raise RuntimeError('HipTensoRFRegularizer runs on the HIP device; there is no CPU path')
            self._dev = torch.zeros(_lib.HR_REG_SLOTS, dtype=torch.float32, device=dev)
            self._loss = torch.zeros(1 + _lib.HR_REG_SLOTS, dtype=torch.float32, device=dev)
        self._dev.copy_(torch.tensor(w, dtype=torch.float32))
        self._synced = w

    def _table(self, terms):
        arr = (_lib.hr_reg_tensor * max(len(terms), 1))()
        for e, (p, kh, kw, kl, sh, sw, sl) in zip(arr, terms):
            e.plane_dev, e.grad_dev = p.data_ptr() or None, p.grad.data_ptr() or None
            e.channels, e.h, e.w = p.shape[1], p.shape[2], p.shape[3]
            e.kh, e.kw, e.kl, e.slot_h, e.slot_w, e.slot_l = kh, kw, kl, sh, sw, sl
        return arr

    def accumulate(self):
        """The one hr_tensorf_reg call, on the current stream: adds the regulariser's gradient into every listed parameter's .grad (a
        zero gradient first where it is None; nothing is added while warming_up(), as the reference leaves the term out of `loss`) and
        returns the weighted value `loss(...) * loss_weight()` as a detached device scalar -- the same tensor every call.  `terms_value`
        holds the three unweighted terms of the last call.  The descriptor table is rebuilt when the model's parameters were replaced
        (shrink, upsample_volume_grid, load_state_dict)."""
        if self._dev is None:
            self.sync()
        terms = self.terms()
        for p, *_ in terms:
            if not p.is_contiguous() or p.dtype != torch.float32:
                raise RuntimeError('HipTensoRFRegularizer: planes must be contiguous float32')
            if p.grad is None:
                p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
            elif not p.grad.is_contiguous():
                p.grad = p.grad.contiguous()
        key = tuple((id(p), p.data_ptr(), tuple(p.shape)) for p, *_ in terms)
        gkey = tuple(p.grad.data_ptr() for p, *_ in terms)
        dev = self._dev.device
        with torch.cuda.device(dev):
            if self._plan is None or key != self._plan_key:
                self.close()
                h = C.c_void_p()
                _lib.call('hr_reg_plan_create', self._table(terms), len(terms), C.byref(h))
                self._plan, self._plan_key, self._grad_key = h, key, gkey
            elif gkey != self._grad_key:
                _lib.call('hr_reg_plan_update', self._plan, self._table(terms), len(terms))
                self._grad_key = gkey
            _lib.call('hr_tensorf_reg', self._plan, self._dev, self._loss, 0 if self.warming_up() else 1, _lib.stream(dev))
        return self._loss[0]

    @property
    def terms_value(self):
        """(density_L1, TV_loss_density, TV_loss_app) of the last accumulate(), unweighted: a view of the device result."""
        return self._loss[1:]

    def close(self):
        if self._plan is not None:
            _lib.call('hr_reg_plan_destroy', self._plan)
            self._plan = self._plan_key = self._grad_key = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


KEEP = object()         # GraphedStep.recapture: leave the setting as it is


class GraphedStep:
    """The whole training step as ONE replayed graph (torch.cuda.graph over the library's launches):

        gs = GraphedStep(model, optimizer, rayset, batch_size, loss=HipImageLoss('mse'), seed=0, white_bg=None, regularizer=None, warmup=3)
        out = gs.step()        # one replay: {'loss', 'sse'} as device tensors, no host synchronisation

    One iteration is  rayset.sample(batch_size, step_tensor=optimizer.step_tensor, seed=seed, out=fixed buffers)  ->
    model.forward_train  ->  loss.step_loss  ->  + regularizer(model) when given (tv_loss / l1_mean terms)  ->
    zero_grad(set_to_none=True)  ->  backward  ->  optimizer.step().  What changes from step to step lives on the device: the
    optimizer's step count, which is also the sampler's step, and the learning rates (`optimizer.sync_hyperparameters()`, called by
    step() before the replay).

    regularizer: a callable of the model whose result is added to the loss before backward() -- recorded with the Python floats it
    used -- or a HipTensoRFRegularizer: its accumulate() runs after backward() and its value is added to the returned `loss`; step()
    calls its set_iter(iteration) and sync() before the replay, so every replay trains with the reference's weights of its own iteration.
    The iteration is the optimizer's count, read from the device when the step is (re)recorded and counted on the host from there.

    Construction runs `warmup` (>= 1) iterations eagerly on a side stream -- GENUINE training steps: they update the parameters and
    advance the count, and they are what sizes the library's lazily grown workspaces and allocates the moments -- and then records one
    iteration on a single stream (no parallel branches), which is not executed.  After construction `warmup` steps have been taken.

    optimizer: HipAdam(capturable=True) holding every trainable parameter of the model.  white_bg: True / False -- the background of
    every step; None -- the configuration's `white_bg and not black_bg`; 'coin' -- the reference's per-step draw
    (tensorf_no_sample.py:236), taken on the device from the optimizer's step count: step s is white iff background_coin(bg_seed, s)
    (or always / never for a white_bg / black_bg configuration).  'coin' binds the model (Model.set_background_coin) until close() or
    a recapture(white_bg=...) with another setting.
    step() returns the SAME two tensors every time (the graph's outputs: `loss` is the differentiated total, `sse` the squared-error
    sum of train/psnr); clone what must outlive the next replay.

    Anything that replaces parameters or changes the compiled configuration -- set_iter inside a schedule window or across a grid
    growth, upsample_volume_grid, load_state_dict, a new optimizer state -- makes the recording stale: step() raises and names
    recapture().  Cascade models (point_prediction) are refused."""

    def __init__(self, model, optimizer, rayset, batch_size, loss, seed=0, white_bg=None, regularizer=None, warmup=3, bg_seed=0):
        from .optim import HipAdam
        if not isinstance(optimizer, HipAdam) or not optimizer.capturable:
            raise TypeError('GraphedStep needs a HipAdam(capturable=True) optimizer: the step count and the learning rates of any other one live on '
                            'the host, and a recorded step would repeat them')
        if not hasattr(loss, 'step_loss'):
            raise TypeError('GraphedStep: loss must be a hyperreel_amd.losses.HipImageLoss')
        if int(batch_size) < 1 or int(warmup) < 1:
            raise ValueError('GraphedStep: batch_size >= 1 and warmup >= 1 (the first eager step sizes the workspaces and allocates the moments)')
        if model._compile(model.grid_size)[0] is not None:
            raise NotImplementedError('GraphedStep: point_prediction cascades re-create their native model when a schedule moves; use the eager loop')
        self.model, self.optimizer, self.rayset, self.loss = model, optimizer, rayset, loss
        self.batch_size, self.seed, self.regularizer = int(batch_size), int(seed), regularizer
        self.bg_seed = int(bg_seed)
        self.white_bg = self._background(white_bg)
        dev = rayset.device
        self.batch = {'coords': torch.empty((self.batch_size, rayset.ray_dim), dtype=torch.float32, device=dev),
                      'rgb': torch.empty((self.batch_size, 3), dtype=torch.float32, device=dev),
                      'weight': torch.empty((self.batch_size, 1), dtype=torch.float32, device=dev)}
        self.graph = None
        self.recapture(warmup=warmup)

    def _background(self, white_bg):
        if isinstance(white_bg, str):
            if white_bg != 'coin':
                raise ValueError(f"GraphedStep: white_bg must be True, False, None or 'coin', not {white_bg!r}")
            return 'coin'
        net_cfg = self.model.cfg['color']['net']
        return (bool(net_cfg.get('white_bg', False)) and not bool(net_cfg.get('black_bg', False))) if white_bg is None else bool(white_bg)

    def close(self):
        """Drops the recording and, for white_bg='coin', unbinds the model's background from the step count."""
        self.graph = self._out = None
        if self.white_bg == 'coin':
            self.model.set_background_coin(step_tensor=None)

    def _iteration(self):
        b = self.rayset.sample(self.batch_size, step_tensor=self.optimizer.step_tensor, seed=self.seed, out=self.batch)
        rgb = self.model.forward_train(b['coords'], white_bg=False if self.white_bg == 'coin' else self.white_bg)
        loss, sse = self.loss.step_loss(rgb, b['rgb'], b['weight'])
        device_reg = isinstance(self.regularizer, HipTensoRFRegularizer)
        if self.regularizer is not None and not device_reg:
            loss = loss + self.regularizer(self.model)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        total = loss.detach()
        if device_reg:                                       # value and gradient in one call, behind autograd's gradients
            value = self.regularizer.accumulate()
            if not self.regularizer.warming_up():            # (the reference logs a warming-up term and leaves it out of `loss`)
                total = total + value
        self.optimizer.step()
        return total, sse

    def _before_step(self):
        """What the host owes the device before iteration `self._host_step` runs: the learning rates and the regulariser's weights."""
        self.optimizer.sync_hyperparameters()
        if isinstance(self.regularizer, HipTensoRFRegularizer):
            self.regularizer.set_iter(self._host_step)
            self.regularizer.sync()

    def _fingerprint(self):
        """What the recording holds pointers to: the parameters, their moments, and the compiled configuration."""
        ps = tuple((id(p), p.data_ptr(), tuple(p.shape)) for p in self.model.parameters())
        st = self.optimizer.state
        ms = tuple((st[p]['exp_avg'].data_ptr(), st[p]['exp_avg_sq'].data_ptr()) if p in st and 'exp_avg' in st[p] else None
                   for g in self.optimizer.param_groups for p in g['params'])
        return ps, ms, self.model.held_config()

    def recapture(self, optimizer=None, warmup=1, white_bg=KEEP, bg_seed=None):
        """Runs `warmup` eager iterations (genuine steps; >= 1 whenever parameters were replaced: the native model and the moments are
        rebuilt by an eager step) and records the iteration again.  optimizer: the new HipAdam(capturable=True) when the parameters were
        replaced (its count starts where its state says: 0 for a fresh one).  white_bg / bg_seed: another background setting."""
        from .optim import HipAdam
        if optimizer is not None:
            if not isinstance(optimizer, HipAdam) or not optimizer.capturable:
                raise TypeError('GraphedStep.recapture needs a HipAdam(capturable=True) optimizer')
            self.optimizer = optimizer
        held = {id(p) for g in self.optimizer.param_groups for p in g['params']}
        missing = [n for n, p in self.model.named_parameters() if p.requires_grad and id(p) not in held]
        if missing:
            raise ValueError(f'GraphedStep: the optimizer does not hold {missing[:3]}{" ..." if len(missing) > 3 else ""} -- after parameters were '
                             'replaced, build a new HipAdam(capturable=True) over model.parameters() and pass it to recapture(optimizer=...)')
        self.graph = None
        self._out = None
        if white_bg is not KEEP:
            self.white_bg = self._background(white_bg)
        if bg_seed is not None:
            self.bg_seed = int(bg_seed)
        # (binds to the optimizer this recording steps; any other setting leaves the white_bg argument in charge)
        self.model.set_background_coin(self.bg_seed, self.optimizer.step_tensor if self.white_bg == 'coin' else None)
        dev = self.rayset.device
        self._host_step = self.optimizer.steps_done()        # the host's mirror of the device count: the regulariser's iteration
        with torch.cuda.device(dev):
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(int(warmup)):
                    self._before_step()
                    self._iteration()
                    self._host_step += 1
            torch.cuda.current_stream(dev).wait_stream(side)
            self.optimizer.zero_grad(set_to_none=True)
            self._before_step()
            self._reg_warming_up = self.regularizer.warming_up() if isinstance(self.regularizer, HipTensoRFRegularizer) else None
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):                   # one stream: the recording has no parallel branches
                loss, sse = self._iteration()
        self.graph, self._out = graph, {'loss': loss, 'sse': sse}
        self._cur_iter = self.model.cur_iter
        self._key = self._fingerprint()

    def step(self):
        """One replay.  Returns {'loss', 'sse'}: device tensors, overwritten by the next replay."""
        m = self.model
        if m.cur_iter != self._cur_iter:                     # set_iter since the recording: do the compiled constants still hold?
            if m.wanted_config() != m.held_config():
                raise RuntimeError(f'GraphedStep: set_iter({m.cur_iter}) changed the compiled configuration the recorded step was built from '
                                   f'(recorded at {self._cur_iter}); call gs.recapture()')
            self._cur_iter = m.cur_iter
        if self.graph is None or self._fingerprint() != self._key:
            raise RuntimeError('GraphedStep: parameters, optimizer state or the native model were replaced since the step was recorded (grid '
                               'growth, upsample_volume_grid, load_state_dict ...); call gs.recapture() -- with a new optimizer over the new parameters')
        self._before_step()
        if self._reg_warming_up is not None and self.regularizer.warming_up() != self._reg_warming_up:
            raise RuntimeError(f'GraphedStep: the regulariser left its warm-up at iteration {self._host_step}: the recorded step adds no '
                               'regulariser gradient; call gs.recapture()')
        self.graph.replay()
        self.model.invalidate()                              # the replay stepped the parameters without moving their versions
        self._host_step += 1
        return self._out
