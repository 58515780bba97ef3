"""The reference's optimizer and learning-rate schedule (run_train.py:79-92, config/base.yaml:9-25) on the HIP engine.

`AdamW` / `Adam` are drop-in `torch.optim.Optimizer`s with torch's constructor signatures, defaults, param-group keys and state layout
(`state[p] = {"step", "exp_avg", "exp_avg_sq"}`, `step` a CPU float32 scalar tensor), so checkpoints move freely between them and
`torch.optim.AdamW` / `torch.optim.Adam`.  `step()` is `pp_adam_multi_tensor` (csrc/pp_optim.hip): two launches over every parameter
with a gradient — the update, then the re-split of the trained weights whose f16x3 operand the engine caches (ops.device_split_targets),
so the next forward finds those operands current and launches no split of its own.

`WarmupCosineLR` is the reference's schedule (utils/lr_scheduler.py:306-356 with its warm-up factor, :409-433), written from the
formula; it drives any torch optimizer."""
import math

import numpy as np
import torch

from . import _lib, ops

_STEP_DTYPE = np.dtype(_lib.PpAdamStep)     # one record per tensor and step, filled in field order (`recs` of step())
assert _STEP_DTYPE.itemsize == 40


def _check_param(p):
    if not isinstance(p, torch.Tensor):
        raise TypeError(f"picopose_amd.optim: parameters must be tensors, got {type(p).__name__}")
    if p.dtype != torch.float32:
        raise TypeError(f"picopose_amd.optim: parameters must be float32, got {p.dtype} (there is no fallback to torch's optimizer)")
    if not p.is_contiguous():
        raise ValueError(f"picopose_amd.optim: parameters must be contiguous, got shape {tuple(p.shape)} strides {p.stride()}")
    if not p.is_cuda:
        raise ValueError("picopose_amd.optim: parameters must live on the GPU (the step is a HIP kernel)")


class _FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam's algorithm (`_single_tensor_adam`, fp32) as one fused multi-tensor HIP step."""

    def __init__(self, params, lr, betas, eps, weight_decay, amsgrad, *, foreach, maximize, capturable, differentiable, fused,
                 decoupled_weight_decay):
        if isinstance(lr, torch.Tensor):
            if lr.numel() != 1:
                raise ValueError("Tensor lr must be 1-element")
            lr = float(lr)
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        betas = tuple(float(b) for b in betas)
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if amsgrad:
            raise ValueError("picopose_amd.optim: amsgrad=True is not implemented (the reference does not use it)")
        if maximize:
            raise ValueError("picopose_amd.optim: maximize=True is not implemented")
        if capturable or differentiable:
            raise ValueError("picopose_amd.optim: capturable / differentiable steps are not implemented")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        super().__init__(params, defaults)
        self._table_key = None
        self._workspace = None
        self._ring = [None, None]      # two pinned PpAdamStep slots, each with the event of its last upload
        self._slot = 0

    def add_param_group(self, param_group):
        ps = param_group["params"]
        for p in ([ps] if isinstance(ps, torch.Tensor) else list(ps)):
            _check_param(p)
        super().add_param_group(param_group)

    def _decoupled(self, group):
        return bool(group.get("decoupled_weight_decay", False))

    def _pinned_slot(self, nbytes):
        k = self._slot
        self._slot ^= 1
        ent = self._ring[k]
        if ent is not None:
            ent[1].synchronize()       # the upload issued from this slot two steps ago has left it
        if ent is None or ent[0].numel() < nbytes:
            ent = self._ring[k] = [torch.empty(nbytes, dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
        return ent

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        params, grads, recs = [], [], []
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize") or group.get("capturable") or group.get("differentiable"):
                raise ValueError("picopose_amd.optim: amsgrad / maximize / capturable / differentiable param groups are not implemented")
            lr = float(group["lr"])
            beta1, beta2 = (float(b) for b in group["betas"])
            wd = float(group["weight_decay"])
            decoupled = self._decoupled(group)
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                if g.is_sparse:
                    raise TypeError("picopose_amd.optim: sparse gradients are not supported")
                if g.dtype != torch.float32 or g.device != p.device:
                    raise TypeError(f"picopose_amd.optim: the gradient must be float32 on {p.device}, got {g.dtype} on {g.device}")
                g = g.contiguous()
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                for k in ("exp_avg", "exp_avg_sq"):     # (a loaded checkpoint: same device and dtype already, by Optimizer.load_state_dict)
                    t = state[k]
                    if t.device != p.device or t.dtype != torch.float32 or not t.is_contiguous() or t.shape != p.shape:
                        state[k] = t.to(device=p.device, dtype=torch.float32).reshape(p.shape).contiguous()
                st = state["step"]
                if st.device.type != "cpu" or st.dtype != torch.float32:
                    st = state["step"] = st.detach().to("cpu", torch.float32)
                st += 1
                step = float(st)
                # the scalars of _single_tensor_adam, formed in double and handed to the kernel as fp32 (as torch's scalar kernels do)
                if wd != 0.0:
                    mode, decay = (1, 1.0 - lr * wd) if decoupled else (2, wd)
                else:
                    mode, decay = 0, 0.0
                inv_bc2 = 1.0 / (1.0 - beta2 ** step) ** 0.5     # (ATen divides by a scalar b as x * fp32(1 / b), 1 / b in double)
                recs.append((g.data_ptr(), -(lr / (1.0 - beta1 ** step)), inv_bc2, decay, 1.0 - beta1, beta2, 1.0 - beta2,
                             float(group["eps"]), mode))
                params.append(p)
                grads.append(g)
        if not params:
            return loss
        dev = params[0].device
        if any(p.device != dev for p in params):
            raise ValueError("picopose_amd.optim: all parameters of one optimizer must be on the same GPU")
        with torch.cuda.device(dev):
            stamp = self._launch(params, recs)
        torch.autograd.graph.increment_version(params)   # the Packed caches and the split cache are keyed on _version
        stamp()
        return loss

    def _launch(self, params, recs):
        targets, stamp = ops.device_split_targets(params)
        hl = {i: (h, s2) for i, h, s2 in targets}
        n = len(params)
        tensors = (_lib.PpAdamTensor * n)()
        key = []
        for i, p in enumerate(params):
            st = self.state[p]
            h, s2 = hl.get(i, (None, None))
            t = tensors[i]
            t.p, t.m, t.v, t.n = p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()
            t.hl, t.scale2 = _lib.address(h), _lib.address(s2)
            key.append((t.p, t.m, t.v, t.n, t.hl, t.scale2))
        key = (params[0].device, tuple(key))
        rebuild = key != self._table_key
        if rebuild:
            need = _lib.workspace_bytes("pp_adam_workspace_bytes", tensors, n)
            if self._workspace is None or self._workspace.numel() < need or self._workspace.device != params[0].device:
                self._workspace = torch.empty(need, dtype=torch.uint8, device=params[0].device)
        # the per-step records: pinned, uploaded on the current stream (two slots: the host never overwrites a copy in flight)
        nbytes = n * _STEP_DTYPE.itemsize
        host, ev = self._pinned_slot(nbytes)
        np.frombuffer(host.numpy(), dtype=_STEP_DTYPE, count=n)[:] = np.array(recs, dtype=_STEP_DTYPE)
        steps = torch.empty(nbytes, dtype=torch.uint8, device=params[0].device)
        steps.copy_(host[:nbytes], non_blocking=True)
        ev.record()
        _lib.call("pp_adam_multi_tensor", tensors, n, steps, ops.terms(), int(rebuild), self._workspace, self._workspace.numel())
        self._table_key = key
        return stamp


class AdamW(_FusedAdam):
    """torch.optim.AdamW (decoupled weight decay) — the reference's optimizer (run_train.py:80-81)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize, capturable=capturable,
                         differentiable=differentiable, fused=fused, decoupled_weight_decay=True)

    def _decoupled(self, group):
        return True

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group["decoupled_weight_decay"] = True


class Adam(_FusedAdam):
    """torch.optim.Adam (L2 weight decay folded into the gradient unless decoupled_weight_decay=True) — run_train.py:82-83."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize, capturable=capturable,
                         differentiable=differentiable, fused=fused, decoupled_weight_decay=decoupled_weight_decay)


def build_optimizer(cfg_optimizer, params):
    """The `type` switch of run_train.py:79-85 on `cfg.optimizer` (a mapping or an attribute object with type, lr, betas, eps,
    weight_decay): "AdamW" or "Adam".  The reference's third branch passes betas / eps to `optim.SGD`, which rejects them (TypeError), so
    no configuration can reach it; it is not reproduced here — any other type raises ValueError."""
    get = (lambda k: cfg_optimizer[k]) if isinstance(cfg_optimizer, dict) else (lambda k: getattr(cfg_optimizer, k))
    kind = get("type")
    cls = {"AdamW": AdamW, "Adam": Adam}.get(kind)
    if cls is None:
        raise ValueError(f"optimizer type {kind!r}: only 'AdamW' and 'Adam' are supported (the reference's SGD branch cannot run)")
    return cls(params, lr=get("lr"), betas=tuple(get("betas")), eps=get("eps"), weight_decay=get("weight_decay"))


def _warmup_factor(method, it, warmup_iters, warmup_factor):
    """utils/lr_scheduler.py:409-433: 1 from `warmup_iters` on; before it `warmup_factor` (constant) or the linear ramp from
    `warmup_factor` to 1."""
    if it >= warmup_iters or warmup_iters == 0:
        return 1.0
    if method == "constant":
        return warmup_factor
    if method == "linear":
        a = it / warmup_iters
        return warmup_factor * (1 - a) + a
    raise ValueError(f"Unknown warmup method: {method}")


class WarmupCosineLR(torch.optim.lr_scheduler.LRScheduler):
    """The reference's schedule (utils/lr_scheduler.py:306-356): lr = base_lr * w(it) * c(it) with the warm-up factor w above and
    c = cos(pi * cycle_factor * it / max_iters), mapped to 0.5 (1 + c) when cycle_factor > 0.5.  start_cos_after_warmup=True: the
    warm-up factor alone up to `warmup_iters`, then the cosine over (it - warmup_iters) / max(1, max_iters - warmup_iters), without the
    warm-up factor."""

    def __init__(self, optimizer, max_iters, cycle_factor=1.0, warmup_factor=0.001, warmup_iters=1000, warmup_method="linear",
                 start_cos_after_warmup=False, last_epoch=-1):
        self.max_iters = max_iters
        self.cycle_factor = cycle_factor
        self.warmup_factor = warmup_factor
        self.warmup_iters = warmup_iters
        self.warmup_method = warmup_method
        self.start_cos_after_warmup = start_cos_after_warmup
        super().__init__(optimizer, last_epoch)

    def _factor(self, it):
        w = _warmup_factor(self.warmup_method, it, self.warmup_iters, self.warmup_factor)
        if self.start_cos_after_warmup:
            if it <= self.warmup_iters:
                return w
            c = math.cos(math.pi * self.cycle_factor * (it - self.warmup_iters) / max(1, self.max_iters - self.warmup_iters))
        else:
            c = math.cos(math.pi * self.cycle_factor * it / self.max_iters)
        if self.cycle_factor > 0.5:
            c = 0.5 * (1.0 + c)
        return c if self.start_cos_after_warmup else w * c

    def get_lr(self):
        f = self._factor(self.last_epoch)
        return [base_lr * f for base_lr in self.base_lrs]

    def _get_closed_form_lr(self):
        return self.get_lr()
