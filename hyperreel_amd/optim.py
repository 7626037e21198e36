"""The optimizer of the training loop on the HIP device.

The reference builds `torch.optim.Adam(parameters, lr=..., eps=1e-8, weight_decay=..., betas=(0.9, 0.99))` per parameter group
(utils/__init__.py:49-76, get_optimizer; nlf/__init__.py:504-530, configure_optimizers) and Lightning steps it after every
`training_step`.  `HipAdam` is that optimizer with the same constructor, the same state names (`step`, `exp_avg`, `exp_avg_sq`: its
`state_dict()` loads into `torch.optim.Adam` and back) and the same arithmetic, whose `step()` is ONE launch of `hr_adam_step` over every
parameter of every group -- one pass over memory instead of the eleven of torch's default foreach form.

`HipAdam(..., capturable=True)` keeps what changes from step to step in device memory -- ONE int64 count of the steps done (`step_tensor`) and one
float learning rate per parameter group -- and steps through `hr_adam_step_dev`, which reads them when the kernel runs: `step()` touches no host
state and may be recorded by `torch.cuda.graph` (one eager step first: the moments are allocated by the first step).  `group['lr']` stays the
Python float the reference's schedulers set (LambdaLR(exp_decay), utils/__init__.py:78-125); `sync_hyperparameters()` carries it to the device.
betas, eps and weight_decay are kernel arguments: a recorded step keeps the values it was recorded with."""
import ctypes as C

import torch

from . import lib as _lib


class HipAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=False):
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0) or not (0.0 <= betas[1] < 1.0):
            raise ValueError('invalid Adam hyper-parameter')
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.capturable = bool(capturable)      # (an attribute, not a group default: the state_dict of either form has torch.optim.Adam's keys only)
        if self.capturable:
            devs = {p.device for g in self.param_groups for p in g['params']}
            if len(devs) != 1 or next(iter(devs)).type != 'cuda':
                raise RuntimeError('HipAdam(capturable=True) keeps its step count and learning rates on the HIP device: all parameters on one such device '
                                   f'(got {sorted(str(d) for d in devs)}); there is no CPU path')
            dev = next(iter(devs))
            self.step_tensor = torch.zeros((), dtype=torch.int64, device=dev)            # steps done; advanced by hr_adam_step_dev on the device
            self._lr_dev = torch.zeros((len(self.param_groups),), dtype=torch.float32, device=dev)
            self._lr_host = None                                                       # what _lr_dev holds (None: nothing yet)
            self.sync_hyperparameters()

    def add_param_group(self, param_group):
        if getattr(self, 'capturable', False):
            raise RuntimeError('HipAdam(capturable=True): parameter groups are fixed at construction (one device learning rate per group)')
        super().add_param_group(param_group)

    def sync_hyperparameters(self):
        """capturable: copies every group's current `lr` to the device floats the step reads, ordered on the current stream; nothing is
        enqueued when no lr changed since the last call.  Not inside a capture (a recorded copy would replay one value).  The device holds
        float32: the step uses float(float32(lr))."""
        if not self.capturable:
            return
        lrs = [float(g['lr']) for g in self.param_groups]
        if lrs == self._lr_host:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('HipAdam.sync_hyperparameters inside a graph capture: call it before each replay instead')
        self._lr_dev.copy_(torch.tensor(lrs, dtype=torch.float32))
        self._lr_host = lrs

    def steps_done(self):
        """capturable: the device count as a Python int (synchronises)."""
        return int(self.step_tensor.item())

    def state_dict(self):
        """torch.optim.Adam's names.  capturable: `step` of every parameter that has moments is materialised from the device count
        (synchronises) -- the result loads into HipAdam(capturable=False) and torch.optim.Adam."""
        sd = super().state_dict()
        if self.capturable:
            t = float(self.steps_done())
            sd['state'] = {k: dict(v, step=torch.tensor(t, dtype=torch.float32)) for k, v in sd['state'].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if self.capturable:
            if len(self.param_groups) != self._lr_dev.numel():
                raise RuntimeError('HipAdam(capturable=True): the loaded state has another number of parameter groups')
            steps = {float(st.pop('step')) for st in self.state.values() if 'step' in st}
            if len(steps) > 1:
                raise RuntimeError(f'HipAdam(capturable=True) keeps ONE step count; the loaded state holds {sorted(steps)}')
            self.step_tensor.fill_(int(steps.pop()) if steps else 0)
            self._lr_host = None
            self.sync_hyperparameters()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        dev = self.step_tensor.device if self.capturable else None
        # validate EVERYTHING before any state is touched: a raise must not leave some parameters' step counts advanced
        for group in self.param_groups:
            if group.get('amsgrad', False) or group.get('maximize', False):
                raise RuntimeError('HipAdam implements plain Adam: amsgrad / maximize are not supported (use torch.optim.Adam for those groups)')
            for p in group['params']:
                if p.grad is None:
                    continue
                if p.device.type != 'cuda':
                    raise RuntimeError('HipAdam steps parameters on the HIP device; there is no CPU path')
                if p.dtype != torch.float32 or p.grad.dtype != torch.float32 or p.grad.is_sparse or not p.is_contiguous():
                    raise RuntimeError('HipAdam: contiguous float32 parameters with dense float32 gradients')
                if dev is None:
                    dev = p.device
                elif p.device != dev:
                    raise RuntimeError('HipAdam: all parameters of one optimizer on one device')
        # one row per parameter that has a gradient: (p, gradient, its state, group index); the capturable form keeps no host count
        rows = []
        for gi, group in enumerate(self.param_groups):
            for p in group['params']:
                if p.grad is None:
                    continue
                st = self.state[p]
                if len(st) == 0:
                    if not self.capturable:
                        st['step'] = torch.tensor(0.0, dtype=torch.float32)               # (host, as torch.optim.Adam keeps it when not capturable)
                    elif torch.cuda.is_current_stream_capturing():
                        raise RuntimeError('HipAdam(capturable=True): take one eager step before the capture (the first step allocates the moments)')
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if not self.capturable:
                    st['step'] += 1
                rows.append((p, p.grad if p.grad.is_contiguous() else p.grad.contiguous(), st, gi))
        if not rows:
            return loss
        k, groups = len(rows), self.param_groups
        ptrs = [(C.c_void_p * k)(*(t.data_ptr() for t in col)) for col in zip(*((p, g, st['exp_avg'], st['exp_avg_sq']) for p, g, st, _ in rows))]
        ns = (C.c_int64 * k)(*(p.numel() for p, *_ in rows))
        if self.capturable:     # betas, eps, weight_decay per row; lr and the count are read on the device
            hp = [float(v) for *_, gi in rows for v in (*groups[gi]['betas'], groups[gi]['eps'], groups[gi]['weight_decay'])]
            _lib.call('hr_adam_step_dev', *ptrs, ns, (C.c_double * len(hp))(*hp), (C.c_int32 * k)(*(gi for *_, gi in rows)), len(groups),
                      self._lr_dev, self.step_tensor, k, _lib.stream(dev), device=dev)
        else:
            hp = [float(v) for _, _, st, gi in rows for v in (groups[gi]['lr'], *groups[gi]['betas'], groups[gi]['eps'], groups[gi]['weight_decay'], st['step'])]
            _lib.call('hr_adam_step', *ptrs, ns, (C.c_double * len(hp))(*hp), k, _lib.stream(dev), device=dev)
        # the launch wrote the parameters behind torch's back: whoever keys on their versions (the model's native handle) must see a step
        torch.autograd.graph.increment_version([p for p, *_ in rows])
        return loss
