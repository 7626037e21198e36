"""Host-side mirror of the reference's model objects for the forward-render path.

`HipLightfieldModel` stands where `LightfieldModel` (nlf/models/models.py:104-138) stands
in the reference: it is built from the same `experiment.model` YAML group and the same
`system` object, exposes the attributes `INRSystem` touches (`set_iter`,
`embedding_model`, `color_model.net`, nlf/__init__.py:449-479,608-614) and owns
nn.Parameters under exactly the reference's state_dict keys, so
reference checkpoints load by name.  The modules hold weights only -- all arithmetic
happens in libhyperreel_hip.so, which receives the tensors through hr_model_upload.
"""
import collections
import ctypes as C
import math
import weakref

import torch
from torch import nn

from . import lib as _lib
from .config import n_to_reso, to_plain
from .data import make_camera, make_fisheye, make_ndc
from .plan import (MLP_PRECISION, compile_model, fast_sincos_ok, frames_per_keyframe, hr_fields, hr_lightfield, hr_maps, shading_mlp, shading_width,
                   time_basis_size, upload_names)

_MLP_PRECISION_NAME = {code: name for name, code in MLP_PRECISION.items()}      # HR_OPT_MLP_PRECISION_ACTIVE -> 'f16x3' ...

MAT_MODE = [[0, 1], [0, 2], [1, 2]]
VEC_MODE = [2, 1, 0]
MAT_MODE_TIME = [[2, 3], [1, 3], [0, 3]]


def dataset_scalars_from_system(system):
    """The five `system.dm.train_dataset` reads of the hot path."""
    td = system.dm.train_dataset
    get = (lambda k, d=None: td[k] if isinstance(td, dict) and k in td else getattr(td, k, d))
    ds = {'near': get('near', 0.0), 'far': get('far', 1.0), 'depth_range': list(get('depth_range', [0.0, 1.0])),
          'num_keyframes': get('num_keyframes', 1), 'num_frames': get('num_frames', 1)}
    # read by single stages only: voxel_grid bounds (voxel.py:27-29), the per-camera colour table (point.py:576-577)
    for k in ('bbox_min', 'bbox_max', 'total_images_per_frame', 'val_all'):
        v = get(k)
        if v is not None:
            ds[k] = [float(t) for t in v] if k.startswith('bbox') else v
    return ds


class _Dummy(nn.Module):
    """RayParam / PE modules of the reference carry an unused nn.Linear(1,1) `dummy_layer`
    (nlf/param.py:479, nlf/pe.py:165); kept so strict state_dict loading works."""

    def __init__(self):
        super().__init__()
        self.dummy_layer = nn.Linear(1, 1)


class _Empty(nn.Module):
    pass


class _ZeroNet(nn.Module):
    """ZeroMLP (nlf/nets/mlp.py:14-33): an unused nn.Linear(1, 1), kept for strict state_dict loading."""

    def __init__(self):
        super().__init__()
        self.layer = nn.Linear(1, 1)


class HostMLP(nn.Module):
    """Parameter container shaped like BaseMLP (nlf/nets/mlp.py:127-154)."""

    def __init__(self, shapes):
        super().__init__()
        self.layers = nn.ModuleList()
        for i, (o, n_in) in enumerate(shapes):
            lin = nn.Linear(n_in, o)
            self.layers.append(nn.Sequential(lin, nn.Identity()) if i < len(shapes) - 1 else lin)


class HostRayPrediction(nn.Module):
    def __init__(self, pred_cfg, shapes):
        super().__init__()
        self.params = nn.ModuleList([_Dummy() for _ in pred_cfg['params']])
        self.pes = nn.ModuleList([_Dummy() if 'pe' in p else _Empty() for p in pred_cfg['params'].values()])
        self.net = HostMLP(shapes) if shapes else _ZeroNet()


class HostColorTransform(nn.Module):
    """ColorTransformEmbedding (nlf/embedding/point.py:558-602): one [3x3 | shift] row per camera."""

    def __init__(self, num_views):
        super().__init__()
        self.color_embedding = nn.Parameter(torch.zeros((int(num_views), 12)))


class HostEmbedding(nn.Module):
    def __init__(self, cfg, shapes, dataset=None):
        super().__init__()
        mods = []
        for e in cfg['embedding']['embeddings'].values():
            if e['type'] == 'ray_prediction':
                mods.append(HostRayPrediction(e, shapes))
            elif e['type'] == 'point_prediction':         # cascades: a second MLP, same container shape
                from .scenes import point_mlp_layer_shapes
                mods.append(HostRayPrediction(e, point_mlp_layer_shapes(e)))
            elif e['type'] == 'color_transform':
                mods.append(HostColorTransform((dataset or {}).get('total_images_per_frame', 1)))
            else:
                mods.append(_Empty())
        self.embeddings = nn.ModuleList(mods)


class HostRenderModule(nn.Module):
    """Parameter container shaped like MLPRender_Fea / MLPRender (nlf/nets/tensorf_base.py:38-69, 106-135): `mlp` is a Sequential with
    Linears at indices 0, 2 and 4, initialised as there (nn.Linear's default, the last bias 0).  The function runs in the library
    (csrc/shade_kernel.hip)."""

    def __init__(self, in_mlpC, featureC):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(in_mlpC, featureC), nn.ReLU(inplace=True), nn.Linear(featureC, featureC), nn.ReLU(inplace=True),
                                 nn.Linear(featureC, 3))
        nn.init.constant_(self.mlp[-1].bias, 0)


class HostTensorVM(nn.Module):
    """Parameter container shaped like TensorVMSplit (nlf/nets/tensorf_base.py:895-991) or
    TensorVMKeyframeTime (nlf/nets/tensorf_dynamic.py:108-244)."""

    def __init__(self, net_cfg, grid_size, num_keyframes, num_frames=None):
        super().__init__()
        self.video = net_cfg['type'] == 'tensor_vm_split_time'
        self.n_den = list(net_cfg.get('n_lamb_sigma', [8, 8, 8]))
        self.n_app = list(net_cfg.get('n_lamb_sh', [24, 24, 24]))
        self.app_dim = int(net_cfg.get('data_dim_color', 27))
        self.num_keyframes = int(num_keyframes)
        self.act = net_cfg.get('fea2denseAct', 'softplus')
        self.alpha_mask_thres = float(net_cfg.get('alpha_mask_thre', 0.001))         # tensorf_base.py:206-208
        self.update_alpha_mask_list = [int(v) for v in net_cfg.get('update_AlphaMask_list', [])]
        self._owner = None                       # weakref to the HipLightfieldModel (set by it): native handle for getDenseAlpha
        # growth schedule of the grids (tensorf_base.py:150-198): log-linear between the start and end resolutions
        self.upsamp_list = [int(v) for v in net_cfg.get('upsamp_list', [])]
        n_up = len(self.upsamp_list) + 1
        steps = lambda a, b: torch.round(torch.exp(torch.linspace(math.log(a), math.log(b), n_up))).long().tolist()[1:]
        self.use_grid_size_upsample = 'grid_size' in net_cfg
        if self.use_grid_size_upsample:
            gs, ge = list(net_cfg['grid_size']['start']), list(net_cfg['grid_size']['end'])
            self.N_voxel_list = [steps(gs[i], ge[i]) for i in range(3)]
        elif 'N_voxel_init' in net_cfg and 'N_voxel_final' in net_cfg:
            self.N_voxel_list = steps(net_cfg['N_voxel_init'], net_cfg['N_voxel_final'])
        else:
            self.N_voxel_list = []
        self.register_buffer('aabb', torch.tensor(to_plain(net_cfg['aabb']), dtype=torch.float32))
        self.register_buffer('gridSize', torch.tensor([int(v) for v in grid_size], dtype=torch.long))
        self.basis_mat = nn.Linear(sum(self.n_app), self.app_dim, bias=False)
        shade = shading_mlp(net_cfg)
        if shade is not None:                    # MLP_Fea / MLP: the reference's renderModule (tensorf_base.py:38-69, 106-135, 252-262)
            self.renderModule = HostRenderModule(shading_width(net_cfg['shadingMode'], shade), shade.feature_c)
        if self.video:
            # densityMode DensityLinear / DensityFourier: one row per function of the time basis (tensorf_dynamic.py:69-74, 122-124)
            self.density_mode = net_cfg.get('densityMode', 'Density')
            rows = 1
            if self.density_mode != 'Density':
                rows = time_basis_size(self.density_mode, frames_per_keyframe(net_cfg, {'num_frames': num_frames or 1, 'num_keyframes': num_keyframes}))
            self.basis_mat_density = nn.Linear(sum(self.n_den), rows, bias=False)
        self.init_svd_volume(grid_size)

    def _dens(self, shape):
        if self.act == 'softplus':
            return 0.1 * torch.randn(shape)
        return 1e-2 * torch.rand(shape).clamp(1e-2, 1e8)

    def init_svd_volume(self, grid_size, device=None):
        """(Re)allocates the planes for `grid_size` with the reference's initialisers."""
        N = [int(v) for v in grid_size]
        device = device if device is not None else self.aabb.device
        self.gridSize = torch.tensor(N, dtype=torch.long, device=device)
        mk = lambda fn, shapes: nn.ParameterList([nn.Parameter(fn(s).to(device)) for s in shapes])
        app = lambda s: 0.1 * torch.randn(s)
        plane = lambda n: [(1, n[i], N[MAT_MODE[i][1]], N[MAT_MODE[i][0]]) for i in range(3)]
        if self.video:
            time = lambda n: [(1, n[i], self.num_keyframes, N[MAT_MODE_TIME[i][0]]) for i in range(3)]
            self.density_plane_space = mk(self._dens, plane(self.n_den))
            self.density_plane_time = mk(self._dens, time(self.n_den))
            self.app_plane_space = mk(app, plane(self.n_app))
            self.app_plane_time = mk(app, time(self.n_app))
        else:
            line = lambda n: [(1, n[i], N[VEC_MODE[i]], 1) for i in range(3)]
            self.density_plane = mk(self._dens, plane(self.n_den))
            self.density_line = mk(self._dens, line(self.n_den))
            self.app_plane = mk(app, plane(self.n_app))
            self.app_line = mk(app, line(self.n_app))

    def set_iter(self, i):
        """TensorBase.set_iter (tensorf_base.py:510-552): in training mode, at the iterations of update_AlphaMask_list the
        occupancy mask is rebuilt (at most 200^3) and, the first time, the grids are shrunk to it; at the iterations of
        upsamp_list the grids grow to the next resolution of N_voxel_list / grid_size."""
        self.cur_iter = i
        if not self.training:
            return
        if i in self.update_alpha_mask_list:
            reso = tuple(int(v) for v in self.gridSize.tolist())
            if reso[0] > 200:
                reso = (200, 200, 200)
            new_aabb = self.updateAlphaMask(reso)
            if i == self.update_alpha_mask_list[0]:
                self.shrink(new_aabb)
        if i in self.upsamp_list and self.N_voxel_list:
            if self.use_grid_size_upsample:
                reso = [self.N_voxel_list[a].pop(0) for a in range(3)]
            else:
                reso = n_to_reso(self.N_voxel_list.pop(0), self.aabb.detach().cpu().tolist())
            self.upsample_volume_grid(reso)

    # -- occupancy / grid management of the training loop (TensorBase.set_iter, nlf/nets/tensorf_base.py:510-530) -------
    @torch.no_grad()
    def getDenseAlpha(self, grid_size):
        """TensorBase.getDenseAlpha (tensorf_base.py:381-401) / TensorVMKeyframeTime.getDenseAlpha (tensorf_dynamic.py:499-536):
        alpha = 1 - exp(-sigma * 0.01) on a dense (n0, n1, n2) lattice of the box (keyframe nets: the maximum over the
        frames), points the current mask rejects get 0.  One HIP launch (hr_dense_alpha) on the owner's native model."""
        owner = self._owner() if self._owner is not None else None
        if owner is None:
            raise RuntimeError('getDenseAlpha needs the owning HipLightfieldModel (its native handle)')
        if getattr(self, 'density_mode', 'Density') != 'Density':
            raise NotImplementedError(f'getDenseAlpha / updateAlphaMask with densityMode {self.density_mode}: the density modes are inference only')
        h = owner.native()
        n = [int(v) for v in grid_size]
        dev = self.aabb.device
        out = torch.empty(n, dtype=torch.float32, device=dev)
        vol = getattr(self, 'alpha_volume', None)
        box = self.alpha_aabb.detach().cpu().reshape(-1).tolist() if vol is not None else [0.0] * 6
        pn = [vol.shape[2], vol.shape[1], vol.shape[0]] if vol is not None else [0, 0, 0]
        _lib.call('hr_dense_alpha', h, (C.c_int32 * 3)(*n), 0.01, int(owner.dataset.get('num_frames', 1)), None if vol is None else vol.contiguous(),
                  (C.c_int32 * 3)(*pn), (C.c_float * 6)(*box), out, _lib.stream(dev), device=dev)
        return out

    @torch.no_grad()
    def updateAlphaMask(self, grid_size=(200, 200, 200)):
        """TensorBase.updateAlphaMask (tensorf_base.py:403-429): dense alpha -> 3x3x3 max-pool -> threshold -> the mask
        volume (stored like AlphaGridMask does, utils/tensorf_utils.py:459-475) and the bounding box of what is left."""
        import torch.nn.functional as F
        n = [int(v) for v in grid_size]
        alpha = self.getDenseAlpha(n)
        dev = alpha.device
        samples = torch.stack(torch.meshgrid(torch.linspace(0, 1, n[0]), torch.linspace(0, 1, n[1]), torch.linspace(0, 1, n[2]),
                                             indexing='ij'), -1).to(dev)
        dense_xyz = self.aabb[0] * (1 - samples) + self.aabb[1] * samples
        dense_xyz = dense_xyz.transpose(0, 2).contiguous()
        alpha = alpha.clamp(0, 1).transpose(0, 2).contiguous()[None, None]
        alpha = F.max_pool3d(alpha, kernel_size=3, padding=1, stride=1).view(n[::-1])
        thres = float(self.alpha_mask_thres)
        alpha = (alpha >= thres).to(torch.float32)
        self.register_buffer('alpha_volume', alpha, persistent=False)            # (n2, n1, n0)
        self.register_buffer('alpha_aabb', self.aabb.clone(), persistent=False)
        valid = dense_xyz[alpha > 0.5]
        return torch.stack((valid.amin(0), valid.amax(0)))

    @torch.no_grad()
    def shrink(self, new_aabb):
        """TensorVMSplit.shrink (tensorf_base.py:1191-1232) / TensorVMKeyframeTime.shrink (tensorf_dynamic.py:444-497):
        crops every plane and line to the texels that cover `new_aabb` and moves the box to those texels."""
        new_aabb = new_aabb.to(self.aabb)
        grid = self.gridSize.to(self.aabb.device)
        units = (self.aabb[1] - self.aabb[0]) / (grid - 1)
        t_l, b_r = (new_aabb[0] - self.aabb[0]) / units, (new_aabb[1] - self.aabb[0]) / units
        t_l, b_r = torch.round(torch.round(t_l)).long(), torch.round(b_r).long() + 1
        b_r = torch.stack([b_r, grid]).amin(0)
        tl, br = t_l.tolist(), b_r.tolist()
        P = lambda t: nn.Parameter(t.contiguous())
        for i in range(3):
            m0, m1 = MAT_MODE[i]
            if self.video:
                t0 = MAT_MODE_TIME[i][0]
                for space, time in ((self.density_plane_space, self.density_plane_time), (self.app_plane_space, self.app_plane_time)):
                    space[i] = P(space[i].data[..., tl[m1]:br[m1], tl[m0]:br[m0]])
                    time[i] = P(time[i].data[..., :, tl[t0]:br[t0]])
            else:
                v = VEC_MODE[i]
                for plane, line in ((self.density_plane, self.density_line), (self.app_plane, self.app_line)):
                    line[i] = P(line[i].data[..., tl[v]:br[v], :])
                    plane[i] = P(plane[i].data[..., tl[m1]:br[m1], tl[m0]:br[m0]])
        mask_grid = torch.tensor([self.alpha_volume.shape[2], self.alpha_volume.shape[1], self.alpha_volume.shape[0]], device=grid.device)
        if not torch.all(mask_grid == grid):
            t_l_r, b_r_r = t_l / (grid - 1), (b_r - 1) / (grid - 1)
            correct = torch.zeros_like(new_aabb)
            correct[0] = (1 - t_l_r) * self.aabb[0] + t_l_r * self.aabb[1]
            correct[1] = (1 - b_r_r) * self.aabb[0] + b_r_r * self.aabb[1]
            new_aabb = correct
        self.aabb = new_aabb.clone()                 # a fresh buffer: the owner sees a new box and rebuilds its native model
        self.gridSize = (b_r - t_l).to(self.gridSize)

    # -- regularizers, as the reference's TensoRF regularizer calls them (nlf/regularizers/tensorf.py:57-92) ----------
    def _reg_planes(self):
        if self.video:
            return self.density_plane_space, self.density_plane_time, self.app_plane_space
        return self.density_plane, self.density_line, self.app_plane

    def density_L1(self):
        """tensorf_base.py:1024-1035 / tensorf_dynamic.py:246-259."""
        from .train import l1_mean
        da, db, _ = self._reg_planes()
        total = 0
        for i in range(3):
            if da[i].shape[1] == 0:
                continue
            total = total + l1_mean(da[i]) + l1_mean(db[i])
        return total

    def TV_loss_density(self, reg):
        """tensorf_base.py:1037-1046 / tensorf_dynamic.py:261-272; `reg` is the reference's TVLoss module (only its weight
        is read: the differences are computed by hr_plane_reg_forward)."""
        from .train import tv_loss
        da, db, _ = self._reg_planes()
        total = 0
        for i in range(3):
            if da[i].shape[1] == 0 or (self.video and db[i].shape[1] == 0):
                continue
            total = total + tv_loss(da[i], getattr(reg, 'TVLoss_weight', 1)) * 1e-2
        return total

    def TV_loss_app(self, reg):
        """tensorf_base.py:1048-1057 / tensorf_dynamic.py:274-285."""
        from .train import tv_loss
        da, db, aa = self._reg_planes()
        total = 0
        for i in range(3):
            if (aa[i].shape[1] == 0) if not self.video else (da[i].shape[1] == 0 or db[i].shape[1] == 0):
                continue
            total = total + tv_loss(aa[i], getattr(reg, 'TVLoss_weight', 1)) * 1e-2
        return total

    @torch.no_grad()
    def upsample_volume_grid(self, res_target):
        """TensorVMSplit.upsample_volume_grid (nlf/nets/tensorf_base.py:1152-1188) /
        TensorVMKeyframeTime.upsample_volume_grid (nlf/nets/tensorf_dynamic.py:395-441): every plane and line is
        resized bilinearly (align_corners=True) to the new grid by hr_upsample_plane; planes of a video net whose density
        plane has no components are re-created as zeros, as in the reference.  Parameters must live on the HIP device."""
        N = [int(v) for v in res_target]

        def resize(p, h2, w2):
            src = p.data.contiguous().float()
            if src.device.type != 'cuda':
                raise RuntimeError('upsample_volume_grid runs on the HIP device; there is no CPU path')
            _, c, h, w = src.shape
            dst = torch.empty((1, c, h2, w2), dtype=torch.float32, device=src.device)
            _lib.call('hr_upsample_plane', src, c, h, w, dst, h2, w2, _lib.stream(src.device), device=src.device)
            return nn.Parameter(dst)

        for i in range(3):
            m0, m1 = MAT_MODE[i]
            if self.video:
                t0 = MAT_MODE_TIME[i][0]
                empty = self.density_plane_space[i].shape[1] == 0
                for space, time in ((self.app_plane_space, self.app_plane_time), (self.density_plane_space, self.density_plane_time)):
                    if empty:
                        space[i] = nn.Parameter(space[i].data.new_zeros(1, space[i].shape[1], N[m1], N[m0]))
                        time[i] = nn.Parameter(time[i].data.new_zeros(1, time[i].shape[1], self.num_keyframes, N[t0]))
                    else:
                        space[i] = resize(space[i], N[m1], N[m0])
                        time[i] = resize(time[i], self.num_keyframes, N[t0])
            else:
                for plane, line in ((self.app_plane, self.app_line), (self.density_plane, self.density_line)):
                    if plane[i].shape[1] > 0:
                        plane[i] = resize(plane[i], N[m1], N[m0])
                    if line[i].shape[1] > 0:
                        line[i] = resize(line[i], N[VEC_MODE[i]], 1)
        self.gridSize = torch.tensor(N, dtype=torch.long, device=self.gridSize.device)


class HostColorModel(nn.Module):
    def __init__(self, net_cfg, grid_size, num_keyframes, num_frames=None):
        super().__init__()
        self.net = HostTensorVM(net_cfg, grid_size, num_keyframes, num_frames)

    def set_iter(self, i):
        self.net.set_iter(i)


KEEP, CONFIG, UPLOAD, CREATE = 'keep', 'config', 'upload', 'create'        # what native_action asks for, weakest first

# What an hr_model was made from (held) or would be made from now (want).  param_key: HipLightfieldModel._param_key(), None = stale;
# box_key: (data_ptr, version) of the net's aabb buffer; made: (mlp_precision code, grid_dtype code, compiled aabb), which with the grid
# is fixed at creation; blob: config_blob of the compiled configuration; cascade: whether it has a coarse level.
NativeKey = collections.namedtuple('NativeKey', ['param_key', 'grid', 'box_key', 'made', 'blob', 'cascade'])


def config_blob(coarse, hc):
    """The bytes of a compiled configuration: what tells two of them apart."""
    return bytes(hc) + (bytes(coarse) if coarse is not None else b'')


def native_action(held, want, values_travel=False):
    """The rule for an hr_model's life: held (None: no handle) against want -> KEEP | CONFIG (hr_model_update_config) | UPLOAD (every
    tensor again, then finalize; the configuration after it where that moved too) | CREATE (a new handle, then the upload).
    values_travel: a training step hands the parameter values to the kernels itself -- the parameter key is not looked at, a new grid
    or box is what makes the handle stale."""
    if held is None:
        return CREATE
    if values_travel:
        stale = (held.grid, held.box_key) != (want.grid, want.box_key)
    else:
        stale = held.param_key != want.param_key
    moved = held.blob != want.blob                         # cur_iter moved a schedule, or what was uploaded compiles differently
    if (stale and (held.grid, held.made) != (want.grid, want.made)) or (moved and want.cascade):
        return CREATE                                      # (hr_model_update_config does not take cascades: two nested configurations)
    if stale:
        return UPLOAD
    return CONFIG if moved else KEEP


class _Native:
    """Everything a HipLightfieldModel knows about its hr_model."""

    def __init__(self):
        self.handle = None
        self.key = None            # NativeKey of what the handle holds
        self.hc = self.coarse = None   # the compiled configuration behind key.blob (coarse: a cascade's first level)
        self.iter = None           # cur_iter that configuration was compiled at
        self.occ_key = None        # the occupancy volume handed to it (_sync_occupancy)


class HipLightfieldModel(nn.Module):
    """Drop-in for model_dict['lightfield'] (nlf/models/models.py:141-143)."""

    def __init__(self, cfg, **kwargs):
        super().__init__()
        from .scenes import mlp_layer_shapes
        self.cfg = cfg
        system = kwargs.get('system')
        self.dataset = kwargs['dataset'] if 'dataset' in kwargs else dataset_scalars_from_system(system)
        # arithmetic of the MLP GEMMs: 'auto' (= 'f16x3' where its fp16 range is proven at finalize, else 'bf16x3') | 'f16x3' | 'bf16x3' | 'f16f8' | 'f16x2' | 'fp32' (plan.compile_config)
        self.mlp_precision = kwargs.get('mlp_precision', 'auto')
        self.grid_dtype = kwargs.get('grid_dtype', 'fp32')     # 'fp16': half-precision texels (viewer path)
        # execution plan of render() (hr_model_set_option): frame kernel on/off, its sample wavefronts (None: library default)
        # opt-in occupancy early-reject (hr_model_set_occupancy): samples the colour net's AlphaGridMask rejects are neither
        # gathered nor composited -- the reference's own test at tensorf_no_sample.py:171-177, which it ships disabled
        self.use_occupancy = bool(kwargs.get('use_occupancy', False))
        self.frame_kernel = self._frame_mode(kwargs.get('frame_kernel', False))
        self.sample_waves = kwargs.get('sample_waves')
        self.train_deterministic = bool(kwargs.get('train_deterministic', False))
        self.train_fused_mlp = bool(kwargs.get('train_fused_mlp', False))
        # opt-in: an eval-mode forward whose requested fields are only 'distances' / 'points' (weighted sums) is served by render(maps=...):
        # O(B) memory on hr_render's plan, instead of the per-sample diagnostics path (_forward_fields)
        self.fast_fields = bool(kwargs.get('fast_fields', False))
        net = cfg['color']['net']
        if 'grid_size' in kwargs and kwargs['grid_size'] is not None:
            grid = list(kwargs['grid_size'])
        elif 'grid_size' in net:                                   # tensorf_base.py:150-154
            grid = list(net['grid_size']['start'])
        else:
            grid = n_to_reso(net['N_voxel_init'], to_plain(net['aabb']))
        self.param = _Dummy()
        self.embedding_model = HostEmbedding(cfg, mlp_layer_shapes(cfg), self.dataset)
        self.color_model = HostColorModel(net, grid, self.dataset['num_keyframes'], self.dataset.get('num_frames'))
        self.color_model.net._owner = weakref.ref(self)
        self.cur_iter = None           # training iteration of the activation / PE schedules; None = converged (see set_iter)
        self._n = _Native()
        self._render_calls = 0         # render() calls of this handle's overflow guard (_overflow_guard)
        self._reserve = None           # rays per chunk asked for by reserve()
        self._bg_coin = None           # (seed, step tensor) of set_background_coin
        self._box_host = (None, None)  # (box key, the aabb buffer on the host)
        self._grid_size_host = None    # (gridSize tensor, its version, its values)
        self._f8_cannot_calibrate = self._warned_detached_fields = False
        # fail on configurations outside the supported path now, not at the first render
        coarse, hc = self._compile(grid)
        if self.mlp_precision in ('f16f8', 'f16f8v') and not all(fast_sincos_ok(c) for c in (coarse, hc) if c is not None):
            import warnings
            warnings.warn(f"hyperreel_amd: mlp_precision {self.mlp_precision!r} was requested, but a windowed positional encoding of this model reaches "
                          "base_multiplier * freq_multiplier ** n_freqs > 16, beyond what the f16f8 kernels' v_sin / v_cos hold: the MLP runs f16x3 "
                          "(mlp_precision_active() reports it)")

    def upsample_volume_grid(self, res_target):
        """Grows the feature grids like the reference's training loop does (nlf/__init__.py upsampling hooks ->
        color_model.net.upsample_volume_grid); the native model is rebuilt for the new size at the next render."""
        self.color_model.net.upsample_volume_grid(res_target)
        self.invalidate()

    # the names the state went by (tests and tools read them)
    _native = property(lambda self: self._n.handle)
    _hc = property(lambda self: self._n.hc)
    _coarse_hc = property(lambda self: self._n.coarse)

    def invalidate(self):
        """The next native() uploads every tensor again, whatever their versions say."""
        if self._n.key is not None:
            self._n.key = self._n.key._replace(param_key=None)

    def _box_key(self):
        box = self.color_model.net.aabb
        return (box.data_ptr(), box._version)

    def _compile(self, grid):
        """-> (coarse hr_config or None, hr_config of the level that renders), schedules evaluated at cur_iter."""
        # the box is the net's buffer, not the YAML's value: `shrink` replaces it during training and checkpoints carry it
        key = self._box_key()
        if self._box_host[0] != key:        # one device->host copy per change of the box, not per call
            self._box_host = (key, self.color_model.net.aabb.detach().cpu().numpy())
        aabb = self._box_host[1]
        return compile_model(self.cfg, self.dataset, grid, self.mlp_precision, self.grid_dtype, iteration=self.cur_iter, aabb=aabb)

    # -- reference surface ---------------------------------------------------------
    def set_iter(self, i):
        """LightfieldModel.set_iter (what INRSystem.set_train_iter calls every step, nlf/__init__.py:608-614): the EaseValue
        activations (nlf/activations.py:462-496) and WindowedPE weights (nlf/pe.py:166-208) of the model are evaluated at
        training iteration `i`.  Render / test call it with 1e7 (nlf/__init__.py:582-583), where every weight is 1; a model
        that was never told an iteration is in that converged state too.  Only constants of the compiled configuration
        change: the next call swaps them in with hr_model_update_config, no weights are re-packed."""
        self.cur_iter = i
        self.color_model.set_iter(i)

    @property
    def grid_size(self):
        # gridSize is a buffer and lives on the device with the model: read it back only when it changed (forward_train asks every step --
        # a device-to-host copy there stalls the host behind the queue and cannot be captured into a graph)
        # The cache holds the TENSOR it read (shrink / upsample_volume_grid / load_state_dict replace gridSize by fresh tensors whose _version is 0
        # again and whose storage the allocator may hand out at a freed tensor's address: identity, not data_ptr, is the key -- ADVICE r4)
        gs = self.color_model.net.gridSize
        cached = self._grid_size_host
        if cached is None or cached[0] is not gs or cached[1] != gs._version:
            cached = self._grid_size_host = (gs, gs._version, [int(v) for v in gs.tolist()])
        return list(cached[2])

    def load_state_dict(self, state_dict, strict=True):
        """Accepts reference checkpoints: strips a leading `render_fn.model.` / `model.`,
        re-allocates the planes when the checkpoint's gridSize differs and reshapes plane
        tensors (nlf/__init__.py:433-479)."""
        sd = {}
        for k, v in state_dict.items():
            for pre in ('render_fn.model.', 'model.'):
                if k.startswith(pre):
                    k = k[len(pre):]
                    break
            sd[k] = v
        # the alpha mask a trained checkpoint carries (nlf/__init__.py:437-447,472-479) is kept but not read: the colour
        # net's forward never consults it (`if self.alphaMask is not None and False`, tensorf_no_sample.py:171)
        mask = {k: sd.pop(k) for k in list(sd) if 'alpha_aabb' in k or 'alpha_volume' in k}
        if mask:
            net = self.color_model.net
            net.alpha_mask_state = mask
            # the occupancy early-reject (use_occupancy) reads net.alpha_volume / net.alpha_aabb: materialise them from the checkpoint's
            # AlphaGridMask (alphaMask.alpha_volume (1, 1, D, H, W) or flat, alphaMask.alpha_aabb; tensorf_base.py:1139-1168)
            vol = next((v for k, v in mask.items() if k.endswith('alpha_volume')), None)
            box = next((v for k, v in mask.items() if k.endswith('alpha_aabb')), None)
            if vol is not None and box is not None:
                vol = vol.detach().float()
                if vol.dim() == 5:
                    vol = vol[0, 0]
                if vol.dim() == 3:
                    dev = net.aabb.device
                    net.register_buffer('alpha_volume', vol.to(dev).contiguous(), persistent=False)
                    net.register_buffer('alpha_aabb', box.detach().float().reshape(2, 3).to(dev), persistent=False)
        gs = sd.get('color_model.net.gridSize')
        if gs is not None and [int(x) for x in gs.tolist()] != self.grid_size:
            self.color_model.net.init_svd_volume([int(x) for x in gs.tolist()])
        own = self.state_dict()
        for k in list(sd.keys()):
            if k in own and torch.is_tensor(sd[k]) and sd[k].shape != own[k].shape and sd[k].numel() == own[k].numel():
                sd[k] = sd[k].view(own[k].shape)
        self.invalidate()
        return super().load_state_dict(sd, strict=strict)

    # -- native side -------------------------------------------------------------------
    def _tensors(self, coarse, hc):
        own = dict(self.named_parameters())
        types = [e['type'] for e in self.cfg['embedding']['embeddings'].values()]
        idx = {'idx': types.index('ray_prediction'),
               'pp_idx': types.index('point_prediction') if 'point_prediction' in types else -1,
               'ct_idx': types.index('color_transform') if 'color_transform' in types else -1}
        return [(abi, own[key.format(**idx)]) for abi, key in upload_names(hc, coarse)]

    def _param_key(self):
        # cheap fingerprint of everything the native model was built from: in-place
        # updates bump ._version, re-allocations change data_ptr/shape
        net = self.color_model.net
        return (self.mlp_precision, self.grid_dtype, net.aabb.data_ptr(), net.aabb._version) + \
            tuple((p.data_ptr(), p._version, tuple(p.shape)) for p in self.parameters())

    def _want(self, values_travel):
        """-> (NativeKey of what the model is now, coarse, hc).  The configuration is compiled only when something it is compiled from
        moved: while native_action keeps the handle on the cheap keys alone and cur_iter stands, it compiles to what is held."""
        n = self._n
        grid, box_key = self.grid_size, self._box_key()
        param_key = None if values_travel else self._param_key()
        if n.key is not None and n.iter == self.cur_iter:
            same = n.key._replace(param_key=param_key, grid=grid, box_key=box_key)
            if native_action(n.key, same, values_travel) is KEEP:
                return same, n.coarse, n.hc
        coarse, hc = self._compile(grid)
        made = (hc.mlp_precision, hc.grid_dtype, tuple(hc.aabb))
        return NativeKey(param_key, grid, box_key, made, config_blob(coarse, hc), coarse is not None), coarse, hc

    def held_config(self):
        """The bytes of the configuration the native handle holds (None: no handle yet)."""
        return None if self._n.key is None else self._n.key.blob

    def wanted_config(self):
        """The bytes cur_iter compiles to now."""
        return config_blob(*self._compile(self.grid_size))

    def native(self, values_travel=False):
        """Returns the hr_model handle, brought to what native_action asks for: created, its weights (re)uploaded if any parameter
        changed, the constants of cur_iter's schedules swapped in.  values_travel: forward_train's call (see native_action)."""
        n = self._n
        want, coarse, hc = self._want(values_travel)
        action = native_action(n.key if n.handle is not None else None, want, values_travel)
        if action is not KEEP:
            dev = next(self.parameters()).device
            if dev.type != 'cuda':
                raise RuntimeError('HipLightfieldModel must live on a HIP device (model.cuda()); there is no CPU path')
            with torch.cuda.device(dev):
                if action is CREATE:
                    self._create(want, coarse, hc, values_travel)
                if action is not CONFIG:
                    torch.cuda.current_stream().synchronize()
                    for abi, t in self._tensors(coarse, hc):
                        t = t.detach().contiguous().float()
                        _lib.call('hr_model_upload', n.handle, abi.encode(), t, t.numel() * 4)
                    _lib.call('hr_model_finalize', n.handle)
                    n.key = want._replace(param_key=self._param_key(), blob=n.key.blob)
                if n.key.blob != want.blob:          # CONFIG, or an upload into a handle that still held another iteration's constants
                    _lib.call('hr_model_update_config', n.handle, C.byref(hc), _lib.stream(dev))
                    n.key = n.key._replace(blob=want.blob)
        n.hc, n.coarse, n.iter = hc, coarse, self.cur_iter
        return n.handle

    def _create(self, want, coarse, hc, values_travel):
        n = self._n
        if n.handle is not None:
            _lib.call('hr_model_destroy', n.handle)
            if native_action(n.key, want._replace(blob=n.key.blob), values_travel) is not CREATE:
                self._render_calls = 0                 # re-created for a cascade's schedule alone: its overflow guard polls from the start
            n.handle = n.key = None
        h = C.c_void_p()
        if coarse is None:
            _lib.call('hr_model_create', C.byref(hc), C.byref(h))
        else:
            _lib.call('hr_model_create_cascade', C.byref(coarse), C.byref(hc), C.byref(h))
        n.handle, n.key = h, want._replace(param_key=None)
        n.occ_key = None                       # a fresh handle holds no occupancy volume
        if getattr(hc, 'shade_mlp', None) is not None:         # MLP shading modes: the colour network's descriptor, before any upload
            _lib.call('hr_model_set_shading_mlp', h, C.byref(hc.shade_mlp))
        if getattr(hc, 'time_decode', None) is not None:       # RGBt* / Density* modes: the time basis' descriptor, before any upload
            _lib.call('hr_model_set_time_decode', h, C.byref(hc.time_decode))
        self._apply_options()
        if self._reserve:
            _lib.call('hr_model_reserve', h, self._reserve)

    def _sync_occupancy(self):
        """Hands the colour net's current mask volume to the native model (or clears it)."""
        net = self.color_model.net
        vol = getattr(net, 'alpha_volume', None) if self.use_occupancy else None
        key = None if vol is None else (vol.data_ptr(), vol._version, tuple(vol.shape), net.alpha_aabb.data_ptr(), net.alpha_aabb._version)
        if key == self._n.occ_key or self._native is None:
            return
        dev = next(self.parameters()).device
        if vol is None:
            _lib.call('hr_model_set_occupancy', self._native, None, None, None, _lib.stream(dev), device=dev)
        else:
            v = vol.detach().contiguous().float().to(dev)
            n = (C.c_int32 * 3)(v.shape[2], v.shape[1], v.shape[0])
            box = (C.c_float * 6)(*net.alpha_aabb.detach().cpu().reshape(-1).tolist())
            _lib.call('hr_model_set_occupancy', self._native, v, n, box, _lib.stream(dev), device=dev)
        self._n.occ_key = key

    def set_occupancy(self, enable=True):
        """Turns the occupancy early-reject of render() on or off (needs a mask: updateAlphaMask or a checkpoint's)."""
        if enable and getattr(self.color_model.net, 'alpha_volume', None) is None:
            raise RuntimeError('set_occupancy(True): the colour net has no alpha mask volume (run updateAlphaMask, or load a checkpoint that carries one)')
        self.use_occupancy = bool(enable)
        if self._native is not None:
            self._sync_occupancy()

    def _apply_options(self):
        _lib.call('hr_model_set_option', self._native, _lib.HR_OPT_FRAME_KERNEL, int(self.frame_kernel))
        if self.sample_waves is not None:
            _lib.call('hr_model_set_option', self._native, _lib.HR_OPT_SAMPLE_WAVES, int(self.sample_waves))
        _lib.call('hr_model_set_option', self._native, _lib.HR_OPT_TRAIN_DETERMINISTIC, int(self.train_deterministic))
        bg = self._bg_coin
        if bg is not None and not self._black_bg():
            _lib.call('hr_train_set_background', self._native, 1, bg[0], bg[1])
        else:
            _lib.call('hr_train_set_background', self._native, 0, 0, None)

    def _black_bg(self):
        return bool(self.cfg['color']['net'].get('black_bg', False))

    def set_background_coin(self, seed=0, step_tensor=None):
        """Binds the training step's background to the device (hr_train_set_background): with `step_tensor` -- one int64 on the HIP device,
        HipAdam(capturable=True).step_tensor -- forward_train and its backward ignore their white_bg argument and composite step s =
        step_tensor's value over white iff hyperreel_amd.train.background_coin(seed, s), read when the kernels run: the reference's
        per-step draw (tensorf_no_sample.py:236) in a form a replayed graph follows.  As there, a white_bg configuration is white at
        every step and a black_bg one black.  step_tensor=None unbinds: the white_bg argument decides again.  The binding survives a
        re-created native model."""
        if step_tensor is None:
            self._bg_coin = None
        else:
            if step_tensor.dtype != torch.int64 or step_tensor.numel() != 1 or step_tensor.device.type != 'cuda':
                raise TypeError('set_background_coin: step_tensor must be one int64 on the HIP device (HipAdam(capturable=True).step_tensor)')
            self._bg_coin = (int(seed) & 0xFFFFFFFFFFFFFFFF, step_tensor)
        if self._native is not None:
            self._apply_options()

    @staticmethod
    def _frame_mode(v):
        """HR_OPT_FRAME_KERNEL: False / 0 = two kernels (default), True / 1 = the frame kernel for the static nets it fits on 64-ray tiles,
        2 = wherever it fits"""
        return 2 if (v == 2 and v is not True) else int(bool(v))

    def set_train_deterministic(self, enable=True):
        """HR_OPT_TRAIN_DETERMINISTIC: the training step's gradient sums as 64-bit fixed point through integer atomics -- two runs of the
        same step agree bit for bit (the default, fp32 atomics, is faster and reproducible to rounding only)."""
        self.train_deterministic = bool(enable)
        if self._native is not None:
            self._apply_options()

    def set_execution(self, frame_kernel=None, sample_waves=None):
        """Chooses how render() is laid out on the device (images are bit-identical under every setting):
        frame_kernel False = the two-kernel path through the HBM workspace (default), True = the persistent frame kernel for the static
        nets (64-ray tiles), 2 = wherever the model fits it; sample_waves 4 | 8.
        The frame kernel is a one-pass plan: a model on the verified fast path (mlp_precision 'auto' / 'f16f8v', two passes over the HBM
        workspace) keeps the two-kernel path whatever is asked for here -- choose mlp_precision 'f16x3' (or plain 'f16f8') with it."""
        if frame_kernel is not None:
            self.frame_kernel = self._frame_mode(frame_kernel)
        if sample_waves is not None:
            self.sample_waves = int(sample_waves)
        if self._native is not None:
            self._apply_options()
            if self.frame_kernel and self.mlp_verified():
                import warnings
                warnings.warn("hyperreel_amd: frame_kernel was requested for a model on the verified fast path (mlp_precision 'auto' resolved to "
                              "f16f8 + verification), which is a two-pass plan: the request has no effect; use mlp_precision='f16x3' with it")

    def frame_kernel_active(self):
        """True when render() of this model runs as the single persistent frame kernel (head tile in LDS)."""
        return bool(self._get_option(_lib.HR_OPT_FRAME_KERNEL_ACTIVE))

    def chunk_rays(self):
        """Rays per launch of the head workspace (hr_model_reserve / the finalize default): the most hr_stage_* accept."""
        return self._get_option(_lib.HR_OPT_CHUNK_RAYS)

    def _get_option(self, opt):
        v = C.c_int32(0)
        _lib.call('hr_model_get_option', self.native(), opt, C.byref(v))
        return int(v.value)

    def mlp_precision_active(self):
        """The arithmetic the MLP kernels run ('auto' resolved by the library's activation-range calibration)."""
        return _MLP_PRECISION_NAME[self._get_option(_lib.HR_OPT_MLP_PRECISION_ACTIVE)]

    def mlp_verified(self):
        """True when render() runs the verified fast path: f16f8 first, then the rays with a comparison at risk again with the f16x3 tiles
        (HR_MLP_F16F8V; what 'auto' resolves to for a plain ray MLP with at most 64 samples per ray)."""
        return bool(self._get_option(_lib.HR_OPT_MLP_VERIFIED))

    def redo_count(self):
        """Rays the last render() listed for its second pass (synchronises)."""
        return self._get_option(_lib.HR_OPT_REDO_COUNT)

    def wide_count(self):
        """Rays the last render() passed on to its third pass (bf16x3 tiles) because an activation left the IEEE-half range (synchronises)."""
        return self._get_option(_lib.HR_OPT_WIDE_COUNT)

    def redo_overflowed(self):
        """Sticky: a render() listed more rays than a call's list holds (max(32768, B / 16)); the excess kept their first-pass pixels
        (_overflow_guard then re-decides the arithmetic on those rays and renders the batch again)."""
        return bool(self._get_option(_lib.HR_OPT_REDO_OVERFLOW))

    def verify_info(self):
        """hr_model_verify_info as a dict: the band of the verified fast path for THIS model and the f16f8-vs-f16x3 measurement on the
        calibration rays it was derived from (band = max(floor, 4 x the largest difference of a distance / length / point))."""
        v = _lib.hr_verify_info()
        _lib.call('hr_model_verify_info', self.native(), C.byref(v))
        return {k: getattr(v, k) for k, _ in v._fields_}

    def mlp_overflowed(self):
        """True when an fp16-split kernel saw an activation at the IEEE-half range on a rendered ray (sticky; synchronises)."""
        return bool(self._get_option(_lib.HR_OPT_MLP_OVERFLOW))

    def mlp_f8_saturated(self):
        """mlp_precision 'f16f8': True when a hidden activation of a rendered ray was beyond the range of its fp8 image (sticky; synchronises).
        Nothing overflowed -- that ray's correction products were computed from saturated images; `calibrate(rays)` moves the exponents."""
        return bool(self._get_option(_lib.HR_OPT_MLP_F8_SATURATED))

    def calibrate(self, rays):
        """Re-decides the MLP arithmetic on the caller's rays (hr_model_calibrate); returns the per-layer activation maxima."""
        self.native()
        rays = self._check_rays(rays)
        out = (C.c_float * 8)()
        _lib.call('hr_model_calibrate', self.native(), rays, rays.shape[0], out, _lib.stream(rays.device), device=rays.device)
        return [float(v) for v in out[:int(self._hc.mlp_layers)]]

    def reserve(self, rays_per_chunk):
        """Sizes the native workspace; remembered, so that a handle that is re-created (grid growth, cascade schedules) gets it again."""
        self._reserve = int(rays_per_chunk)
        _lib.call('hr_model_reserve', self.native(), self._reserve)

    def device_bytes(self):
        return int(_lib.call('hr_model_device_bytes', self.native()))

    def __del__(self):
        try:
            if self._native is not None:
                _lib.call('hr_model_destroy', self._native)
                self._n.handle = None
                self._render_calls = 0
        except Exception:
            pass

    # -- rendering ---------------------------------------------------------------------
    def _check_rays(self, rays):
        hc = self._hc
        if rays.device.type != 'cuda':
            raise RuntimeError('rays must be on the HIP device; there is no CPU path')
        if rays.dim() != 2 or rays.shape[1] < hc.ray_dim:
            raise ValueError(f'rays must be (B,{hc.ray_dim}), got {tuple(rays.shape)}')
        # the C ABI takes no row stride: extra columns are cut (6-column nets ignore camera id / time, rendering.py)
        return rays[:, :hc.ray_dim].contiguous().float()

    MAP_COLUMNS = {'distances': 1, 'points': 3, 'acc': 1}

    def render(self, rays, want=(), out=None, frame_time=None, maps=(), maps_out=None):
        """rays (B, 6|8) on the HIP device -> dict with 'rgb' (B,3) and any of
        'distances' (B,Z), 'points' (B,Z,3), 'sigma' (B,Z), 'render_weights' (B,Z),
        'head' (B,Z*P) listed in `want`.  out: an existing (B,3) float32 device tensor to render into.
        frame_time: the caller's statement that every ray carries this time (one frame of a keyframe net): hr_render_frame, which reads
        one row of each time plane instead of blending two (images agree with the general path to ~1e-6, not bit for bit).
        maps: per-ray maps from the same launches as the image (hr_render_maps; 'rgb' is bit for bit the one without them):
        'distances' (B,1) = sum_k w_k d_k (depth), 'points' (B,3) = sum_k w_k p_k (expected point), 'acc' (B,1) = sum_k w_k (opacity) --
        the reference's fields=['distances', 'points'] and acc_map.  maps_out: {name: existing contiguous float32 device tensor} to
        render those maps into (a captured graph's fixed buffers).  `want` and `maps` are exclusive."""
        h = self.native()
        self._sync_occupancy()
        rays = self._check_rays(rays)
        B = rays.shape[0]
        hc = self._hc
        Z = hc.z_channels
        maps = tuple(maps)
        if want and maps:
            raise ValueError('render(): `want` (per-sample diagnostics) and `maps` (per-ray maps) cannot be combined')
        unknown = [k for k in maps if k not in self.MAP_COLUMNS]
        if unknown:
            raise ValueError(f'render(): unknown maps {unknown}; available: {sorted(self.MAP_COLUMNS)}')
        if maps_out and set(maps_out) - set(maps):
            raise ValueError('render(): maps_out holds buffers for maps that were not requested')
        if out is not None and (out.shape != (B, 3) or out.dtype != torch.float32 or out.device != rays.device or not out.is_contiguous()):
            raise ValueError('out must be a contiguous (B, 3) float32 tensor on the rays\' device')
        out = {'rgb': out if out is not None else torch.empty((B, 3), dtype=torch.float32, device=rays.device)}
        mp = None
        if maps:
            mp = hr_maps()
            slots = {'distances': 'distances_dev', 'points': 'points_dev', 'acc': 'acc_dev'}
            for k in maps:
                t = (maps_out or {}).get(k)
                shape = (B, self.MAP_COLUMNS[k])
                if t is None:
                    t = torch.empty(shape, dtype=torch.float32, device=rays.device)
                elif t.shape != shape or t.dtype != torch.float32 or t.device != rays.device or not t.is_contiguous():
                    raise ValueError(f'maps_out[{k!r}] must be a contiguous {shape} float32 tensor on the rays\' device')
                out[k] = t
                setattr(mp, slots[k], t.data_ptr())
        stream, rgb = _lib.stream(rays.device), out['rgb']
        with torch.cuda.device(rays.device):
            if not want:
                for attempt in (0, 1):
                    if frame_time is not None and mp is not None:
                        _lib.call('hr_render_frame_maps', h, rays, B, float(frame_time), rgb, C.byref(mp), stream)
                    elif frame_time is not None:
                        _lib.call('hr_render_frame', h, rays, B, float(frame_time), rgb, stream)
                    elif mp is not None:
                        _lib.call('hr_render_maps', h, rays, B, rgb, C.byref(mp), stream)
                    else:
                        _lib.call('hr_render', h, rays, B, rgb, stream)
                    if attempt == 1 or not self._overflow_guard(rays):
                        break
                return out
            f = hr_fields()
            shapes = {'distances': (B, Z), 'points': (B, Z, 3), 'sigma': (B, Z), 'render_weights': (B, Z),
                      'head': (B, Z * hc.preds_per_z)}
            slots = {'distances': 'distances_dev', 'points': 'points_dev', 'sigma': 'sigma_dev',
                     'render_weights': 'weights_dev', 'head': 'head_dev'}
            for k in want:
                out[k] = torch.zeros(shapes[k], dtype=torch.float32, device=rays.device)
                setattr(f, slots[k], out[k].data_ptr())
            _lib.call('hr_render_fields', h, rays, B, rgb, C.byref(f), stream)
        return out

    def _overflow_guard(self, rays):
        """The fp16 split arithmetic ('auto' -> f16x3) was chosen on CALIBRATION rays (hr_model_finalize: synthetic origins in and around
        the scene box); real cameras may stand further out, and activations beyond the IEEE-half range would render inf / NaN where the
        reference's fp32 BaseMLP (nlf/nets/mlp.py:159-172) does not.  The kernels raise a sticky bit when that happens; it is read here
        on the model's first 16 render calls and every 256th after (one 4-byte read behind a synchronise; never inside a stream
        capture).  If set: the arithmetic is re-decided on the offending rays -- 'auto' re-packs as bf16x3 (fp32 exponent range), a forced
        fp16 mode raises HipRangeError -- and the caller renders the batch again.  Returns True when it did so."""
        n = self._render_calls = self._render_calls + 1
        if not (n <= 16 or n % 256 == 0) or torch.cuda.is_current_stream_capturing():
            return False
        active = self.mlp_precision_active()
        if active not in ('f16x3', 'f16x2', 'f16f8'):
            return False
        import warnings
        if self.mlp_overflowed():
            warnings.warn('hyperreel_amd: an MLP activation reached the IEEE-half range on rendered rays (the fp16 split arithmetic had been chosen '
                          'on calibration rays); re-deciding the arithmetic on these rays and rendering the batch again')
            try:
                self.calibrate(rays)
            except RuntimeError as e:
                # a point_prediction cascade cannot be calibrated on the caller's rays (the point MLP's rows are internal: hr_model_calibrate
                # refuses): 'auto' re-creates the native model with the fp32-range split, a forced fp16 mode is refused by name
                if 'cascades' not in str(e):
                    raise
                if self.mlp_precision != 'auto':
                    raise _lib.HipRangeError(f'mlp_precision {self.mlp_precision!r} overflowed the IEEE-half range on rendered rays of a point_prediction '
                                             'cascade; use mlp_precision="auto" or "bf16x3"') from e
                self.mlp_precision = 'bf16x3'
                self.invalidate()
                self.native()
            return True
        if active == 'f16f8' and self.mlp_verified() and self.redo_overflowed():
            # verified fast path: more than a sixteenth of the batch had a comparison inside its margin -- rays unlike the calibration's (which
            # gives the fast path up above a twentieth).  The excess kept their unverified pixels: measure the band on THESE rays (the library
            # falls back to f16x3 when they list too many) and render again; a model that still overflows leaves the fast path for good
            warnings.warn('hyperreel_amd: the verified fast path listed more rays than a call holds; re-calibrating on these rays and rendering the batch again')
            self.calibrate(rays)
            if self.mlp_verified() and self.verify_info()['listed_frac'] > 0.05:
                self.mlp_precision = 'f16x3'
                self.invalidate()
                self.native()
            return True
        if active == 'f16f8' and self.mlp_f8_saturated():
            # f16f8: the fp8 images of a layer's output are scaled from the calibration's largest activation of that layer.  Beyond 16x that they
            # saturate (finite, less accurate).  Where the model can be calibrated on the caller's rays, do so and render again; a cascade's
            # point MLP sees internal rows (hr_model_calibrate refuses it): say so once and carry on
            if self._f8_cannot_calibrate:
                return False
            try:
                self.calibrate(rays)
            except RuntimeError as e:
                if 'cascades' not in str(e):
                    raise
                self._f8_cannot_calibrate = True
                warnings.warn('hyperreel_amd: mlp_precision f16f8 saturated the fp8 image of an activation on rendered rays and this model (a cascade) '
                              'cannot be re-calibrated on them: those rays carry less accurate correction products (mlp_precision f16x3 has none)')
                return False
            warnings.warn('hyperreel_amd: mlp_precision f16f8 saturated the fp8 image of an activation on rendered rays; moved the exponents to these '
                          'rays and rendering the batch again')
            return True
        return False

    def generate_rays(self, pose, K, width, height, time=None, cam_id=0.0, pixel_range=None, device=None, ndc=None, fisheye=None):
        """get_coords_from_camera (datasets/base.py:485-518) on the device: 3x4 camera-to-world
        `pose`, 3x3 intrinsics `K` -> rays (n, 6|8) for pixels [lo, hi) of the row-major image
        (whole image by default).  80 bytes cross the PCIe bus instead of the ray list.
        ndc: dict(fx, fy, near, width, height) or an hr_ndc -- the DATASET's to_ndc arguments (datasets/technicolor.py:355-358),
        for nets trained on use_ndc datasets: the rays then pass through get_ndc_rays_fx_fy (hr_generate_rays_ndc).
        fisheye: (k1, k2) or an hr_fisheye -- the camera's radial distortion, for the rays of an Immersive camera's own pixels
        (datasets/immersive.py:514-523; hr_generate_rays_fisheye).  None: a pinhole camera, the call and the bits of before."""
        self.native()
        dev = torch.device(device) if device is not None else next(self.parameters()).device
        lo, hi = (0, int(width) * int(height)) if pixel_range is None else (int(pixel_range[0]), int(pixel_range[1]))
        cam = make_camera(pose, K, width, height, cam_id, 0.0 if time is None else time)
        fe, nd = make_fisheye(fisheye), make_ndc(ndc)
        rd = self._hc.ray_dim
        rays = torch.empty((hi - lo, rd), dtype=torch.float32, device=dev)
        # NULL for both optional pointers: hr_generate_rays itself
        _lib.call('hr_generate_rays_fisheye', C.byref(cam), C.byref(fe) if fe is not None else None, C.byref(nd) if nd is not None else None,
                  rd, lo, hi - lo, rays, _lib.stream(dev), device=dev)
        return rays

    def render_camera(self, pose, K, width, height, time=None, cam_id=0.0, pixel_range=None, ndc=None, fisheye=None):
        """The viewer's frame path (utils/gui_utils.py:139-212, nlf/__init__.py:754-807) without
        its host round trips: pose -> rays -> rgb, all on the device and on the current stream."""
        return self.render(self.generate_rays(pose, K, width, height, time, cam_id, pixel_range, ndc=ndc, fisheye=fisheye), frame_time=time)['rgb']

    def _lightfield_rays(self, epi, a, b, lightfield, pixel_range, device):
        if not isinstance(lightfield, hr_lightfield):
            raise TypeError('lightfield must be an hr_lightfield (data.make_lightfield)')
        self.native()
        if self._hc.ray_dim != 6:
            raise ValueError(f'two-plane light-field rays have 6 columns; this model takes {self._hc.ray_dim}')
        dev = torch.device(device) if device is not None else next(self.parameters()).device
        lo, hi = (0, int(lightfield.width) * int(lightfield.height)) if pixel_range is None else (int(pixel_range[0]), int(pixel_range[1]))
        if hi < lo:
            raise ValueError(f'pixel_range {pixel_range} is reversed')
        rays = torch.empty((hi - lo, 6), dtype=torch.float32, device=dev)
        _lib.call('hr_generate_rays_epi' if epi else 'hr_generate_rays_lightfield', C.byref(lightfield), float(a), float(b), lo, hi - lo, rays,
                  _lib.stream(dev), device=dev)
        return rays

    def generate_lightfield_rays(self, s, t, lightfield, pixel_range=None, device=None):
        """get_lightfield_rays (utils/ray_utils.py:14-45) on the device: rays (n, 6) for pixels [lo, hi) of the row-major U x V view at
        camera-plane position (s, t) (whole view by default); lightfield: data.make_lightfield(...).  28 bytes cross the PCIe bus
        instead of the ray list (datasets/stanford.py:120)."""
        return self._lightfield_rays(False, s, t, lightfield, pixel_range, device)

    def render_lightfield_view(self, s, t, lightfield, pixel_range=None):
        """render(generate_lightfield_rays(...))['rgb'], bit for bit; image-parallel ranks pass their own pixel_range."""
        return self.render(self.generate_lightfield_rays(s, t, lightfield, pixel_range))['rgb']

    def generate_epi_rays(self, v, t, lightfield, pixel_range=None, device=None):
        """get_epi_rays (utils/ray_utils.py:47-78) on the device: the epipolar slice (u, s) at a fixed (v, t), rays (U * S, 6) with
        lightfield.width = U and lightfield.height = S (nlf/visualizers/epipolar.py:106)."""
        return self._lightfield_rays(True, v, t, lightfield, pixel_range, device)

    def render_epi(self, v, t, lightfield, pixel_range=None):
        """render(generate_epi_rays(...))['rgb'], bit for bit."""
        return self.render(self.generate_epi_rays(v, t, lightfield, pixel_range))['rgb']

    def evaluate(self, rays, gt, h, w, frame_time=None, ssim=True, lpips=None):
        """Render a frame and score it against its ground truth without leaving the device until the four sums are read: what
        validation_image does on the host (nlf/__init__.py:976-980, metrics.py:25-35).  rays: the frame's h*w rays; gt: (h*w, 3)
        on the HIP device.  Returns (rgb, {'mse', 'psnr', 'ssim'}); rgb is the unchanged render() call's, bit for bit.
        lpips: an hyperreel_amd.lpips.Lpips; the result gains 'lpips', the distance of the same frame (metrics.py:54-58), enqueued
        before the first read-back.  LPIPS does not add across image tiles (receptive fields cross the cuts): on image-parallel ranks
        gather the frame and score it on one rank."""
        from . import metrics
        rgb = self.render(rays, frame_time=frame_time)['rgb']
        sums = metrics.image_scores(rgb, gt, h, w, ssim=ssim)
        if lpips is None:
            return rgb, metrics.scores_to_metrics(sums, h, w)
        dist = lpips.lpips_scores(rgb, gt, h, w)
        m = metrics.scores_to_metrics(sums, h, w)
        m['lpips'] = float(dist[5])
        return rgb, m

    def pack_display(self, rgb, height, width, transpose=False, flip=False, rgba8=True):
        """The viewer's hand-over (utils/gui_utils.py:174-205) on the device: rgb (H*W, 3) as rendered -> the displayed
        buffer, transposed / flipped as NeRFGUI does on the host, as 8-bit RGBA (to8b, utils/__init__.py:47) or fp32 RGB."""
        oh, ow = (width, height) if transpose else (height, width)
        rgb = rgb.contiguous().float()
        if rgb.device.type != 'cuda' or rgb.numel() != height * width * 3:
            raise ValueError('rgb must be a (H*W, 3) tensor on the HIP device')
        out = torch.empty((oh, ow, 4), dtype=torch.uint8, device=rgb.device) if rgba8 else \
            torch.empty((oh, ow, 3), dtype=torch.float32, device=rgb.device)
        _lib.call('hr_pack_display', rgb, int(height), int(width), int(bool(transpose)), int(bool(flip)), int(bool(rgba8)), out,
                  _lib.stream(rgb.device), device=rgb.device)
        return out

    def forward_train(self, rays, white_bg=None, want_fields=False):
        """One differentiable forward of the training step (nlf/__init__.py:634-709 calls `self(coords)` in train mode):
        rgb (B, 3) WITHOUT the eval-mode clamp, with autograd history to the MLP, the planes / lines and basis_mat.
        white_bg: this step's background; default = the reference's draw `white_bg or rand() < 0.5` unless black_bg
        (tensorf_no_sample.py:236).  The activation schedules are the converged ones (see set_iter).
        want_fields: also return {'distances', 'points', 'render_weights', 'head'} of THIS forward (detached; hr_train_forward_fields)."""
        from . import train as T
        mode = self.cfg['color']['net'].get('shadingMode', 'MLP_PE')
        if shading_mlp(self.cfg['color']['net']) is not None:
            raise NotImplementedError(f'training with shadingMode {mode}: the colour network is inference only')
        if self.cfg['color']['net'].get('densityMode', 'Density') != 'Density':
            raise NotImplementedError(f"training with densityMode {self.cfg['color']['net']['densityMode']}: the density modes are inference only")
        h, hc = self.native(values_travel=True), self._hc
        rays = self._check_rays(rays)
        net_cfg = self.cfg['color']['net']
        if self._bg_coin is not None:         # set_background_coin: the device decides (a black_bg configuration stays black)
            white_bg = False
        elif white_bg is None:
            white_bg = (bool(net_cfg.get('white_bg', False)) or bool(torch.rand(()) < 0.5)) and not bool(net_cfg.get('black_bg', False))
        types = [e['type'] for e in self.cfg['embedding']['embeddings'].values()]
        pred = self.embedding_model.embeddings[types.index('ray_prediction')]
        lvl0 = self._coarse_hc if self._coarse_hc is not None else hc       # the level the ray MLP belongs to
        if lvl0.mlp_layers == 0:                                # ZeroMLP, nlf/nets/mlp.py:14-33
            head = torch.zeros((rays.shape[0], lvl0.z_channels * lvl0.preds_per_z), dtype=torch.float32, device=rays.device)
        else:
            feats = T.ray_features(h, rays, lvl0.mlp_in)
            if self.train_fused_mlp and self._coarse_hc is None and lvl0.mlp_hidden == 256 and lvl0.mlp_layers >= 2 and not self.train_deterministic:
                # opt-in: one launch for the six layers (hr_mlp_train_forward: bf16 split arithmetic, head within 7e-6 of max |head|).  Not
                # the default: a pre-activation within that error of zero takes the other branch of the LeakyReLU, and the reference's
                # gradient (its autograd goldens, 1e-3 of a tensor's largest entry) is only met by the layer-by-layer forward, whose
                # GEMMs carry 24 mantissa bits (HipLinear); DESIGN 11
                head = T.mlp_forward_fused(h, rays, feats, pred.net, lvl0.mlp_skip_mask, lvl0.z_channels * lvl0.preds_per_z)
            else:
                head = T.mlp_forward(pred.net, feats, lvl0.mlp_skip_mask)
        if self._coarse_hc is not None:                         # point_prediction cascade (point.py:137-203)
            rows = T.CoarseRows.apply(h, rays, head, lvl0.z_channels, hc.casc_row_dim)
            point = self.embedding_model.embeddings[types.index('point_prediction')]
            head = T.mlp_forward(point.net, T.row_features(hc, rows), hc.mlp_skip_mask).reshape(rays.shape[0], -1)
        vm = self.color_model.net
        extra = ()
        if hc.color_table_views > 0:                            # ColorTransformEmbedding's table (point.py:558-602)
            extra = (self.embedding_model.embeddings[types.index('color_transform')].color_embedding,)
        args = (h, rays, head, white_bg, vm.basis_mat.weight, *T.grid_parameters(vm), *extra)
        if want_fields:
            rgb, distances, points, weights = T.SampleStageFields.apply(hc.z_channels, *args)
            return rgb, {'distances': distances, 'points': points, 'render_weights': weights, 'head': head.detach()}
        return T.SampleStage.apply(*args)

    def forward(self, rays, render_kwargs=None):
        """LightfieldModel.forward (models.py:135-138).  In train mode with autograd enabled this is the
        differentiable path (forward_train); otherwise the inference renderer."""
        render_kwargs = render_kwargs or {}
        fields = list(render_kwargs.get('fields', []))
        if self.training and torch.is_grad_enabled() and not fields:
            return {'rgb': self.forward_train(rays)}
        if not fields:
            return {'rgb': self.render(rays)['rgb']}
        if self.fast_fields and not self.training:
            maps = self._fast_field_maps(fields, render_kwargs)
            if maps is not None:
                r = self.render(rays, maps=maps)
                return {k: r[k] for k in ['rgb', *maps]}
        if self.training and torch.is_grad_enabled() and self._hc.z_channels <= 64:
            # INRSystem.training_step passes the regularizers' field list on the main forward (nlf/__init__.py:658-690): the colour
            # stays differentiable (training arithmetic: no eval-mode clamp, the per-step background draw) and the requested fields are
            # the per-sample values of the SAME forward pass (hr_train_forward_fields), detached -- no second, inference pass and no
            # re-upload of the weights.  A regulariser that needs d(field)/d(parameters) is outside the training path (SURVEY 8f-4
            # covers the colour loss and the plane regularisers).
            rgb, r = self.forward_train(rays, want_fields=True)
            r['rgb'] = rgb.detach()
            return self._detached_fields(self._forward_fields(rays, render_kwargs, r), rgb,
                                         ' are DETACHED values of the training forward -- a regulariser that needs their gradient contributes none '
                                         '(differentiable: rgb, and the plane regularisers of hyperreel_amd.train)')
        out = self._forward_fields(rays, render_kwargs)
        if self.training and torch.is_grad_enabled():
            # INRSystem.training_step passes the regularizers' field list on the main forward (nlf/__init__.py:634-709):
            # the colour must stay differentiable.  rgb comes from the training arithmetic (no eval-mode clamp, the
            # per-step background draw); the requested fields are the inference kernel's values, detached -- a
            # regulariser that needs d(field)/d(parameters) is outside the training path (SURVEY 8f-4 covers the colour loss
            # and the plane regularisers).
            return self._detached_fields(out, self.forward_train(rays),
                                         ' come from the inference kernels and are DETACHED -- a regulariser that needs their gradient contributes none '
                                         '(differentiable: rgb, and the plane regularisers of hyperreel_amd.train); every such step also re-uploads the '
                                         'weights for the inference pass')
        return out

    def _detached_fields(self, out, rgb, how):
        """forward's train-mode answer to a field list: the fields detached, `rgb` the differentiable colour; warns once, `how` saying
        where the fields come from."""
        out = {k: v.detach() for k, v in out.items()}
        if not self._warned_detached_fields:
            import warnings
            self._warned_detached_fields = True
            warnings.warn('HipLightfieldModel.forward in train mode: the fields ' + ', '.join(sorted(k for k in out if k != 'rgb')) + how,
                          RuntimeWarning, stacklevel=3)
        out['rgb'] = rgb
        return out

    # -- diagnostics surface (visualizers only) ------------------------------------------
    def _head_fields(self, rays, head):
        hc = self._hc
        B, Z, P = rays.shape[0], hc.z_channels, hc.preds_per_z
        h = head.view(B, Z, P)
        out = {}

        def act(f, x):
            y = x * f.act.inner + f.act.shift
            if f.act.type == 1:
                y = torch.sigmoid(y)
            elif f.act.type == 2:
                y = torch.tanh(y)
            return y * f.act.outer + f.act.add

        for name, f in (('color_scale', hc.f_color_scale), ('color_shift', hc.f_color_shift)):
            if f.offset >= 0:
                out[name] = act(f, h[..., f.offset:f.offset + f.channels]).reshape(B, -1)
        return out

    def embed(self, rays, render_kwargs=None):
        """LightfieldModel.embed (models.py:131-133): the flattened fields handed to the
        colour net (extract_fields lists of the YAMLs).  Diagnostics path."""
        return self._embed_from(rays, self.render(rays, want=('distances', 'points', 'head')))

    def _embed_from(self, rays, r):
        rays = self._check_rays(rays)
        B, Z = rays.shape[0], self._hc.z_channels
        x = {'points': r['points'].reshape(B, -1), 'distances': r['distances'],
             'viewdirs': rays[:, None, 3:6].expand(B, Z, 3).reshape(B, -1),
             'weights': torch.ones_like(r['distances'])}
        x.update(self._head_fields(rays, r['head']))
        if self._hc.advect:
            t = rays[:, -1:]
            fac, inv = self._hc.flow_fac, self._hc.flow_inv_fac
            base = torch.round((t * fac).clamp(0.0, self._hc.flow_kmax) - 1e-5) * inv
            x['base_times'] = base.expand(B, Z).contiguous()
            x['time_offset'] = (t - base).expand(B, Z).contiguous()
            x['times'] = t.expand(B, Z).contiguous()
        return x

    def _field_names(self):
        """The keys _forward_fields can produce for this model (others are skipped, as the reference's loop over x skips them)."""
        hc = self._hc
        if hc is None:                                  # no native model yet: the configuration it will be built from
            hc = self._compile(self.grid_size)[1]
        names = {'render_weights', 'points', 'distances', 'viewdirs', 'weights'}
        names |= {n for n, f in (('color_scale', hc.f_color_scale), ('color_shift', hc.f_color_shift)) if f.offset >= 0}
        if hc.advect:
            names |= {'base_times', 'time_offset', 'times'}
        return names

    def _fast_field_maps(self, fields, render_kwargs):
        """fast_fields: the maps that serve `fields` when every producible requested key is a weighted sum of 'distances' / 'points'
        (none of them in no_over_fields); None: the request needs the per-sample path."""
        if render_kwargs.get('pred_weights_fields'):
            return None
        no_over = set(render_kwargs.get('no_over_fields', []))
        keys = [k for k in dict.fromkeys(fields) if k in self._field_names()]
        if any(k not in ('distances', 'points') or k in no_over for k in keys):
            return None
        return tuple(keys)

    def _forward_fields(self, rays, render_kwargs, r=None):
        """render_kwargs `fields` / `no_over_fields` (tensorf_no_sample.py:254-278).  r: per-sample values already at hand (the training
        forward's own); default: one pass of the inference kernels."""
        fields = list(render_kwargs.get('fields', []))
        no_over = list(render_kwargs.get('no_over_fields', []))
        if render_kwargs.get('pred_weights_fields'):
            raise NotImplementedError('pred_weights_fields')
        if r is None:
            r = self.render(rays, want=('distances', 'points', 'render_weights', 'head'))
        x = self._embed_from(rays, r)
        B, Z = r['render_weights'].shape
        out = {'rgb': r['rgb']}
        w = r['render_weights']
        for key in fields:
            if key == 'render_weights':
                out[key] = w
            elif key in x:
                v = x[key]
                out[key] = v.view(B, -1) if key in no_over else torch.sum(w[..., None] * v.view(B, Z, -1), -2)
        return out


model_dict = {'lightfield': HipLightfieldModel, 'lightfield_hip': HipLightfieldModel}
