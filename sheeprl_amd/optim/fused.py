"""Optimizers.

* :class:`FusedAdam` — Adam with a single multi-tensor HIP kernel per step on
  GPU; exact Adam math (PyTorch semantics) on CPU.
  States are kept in fp32 even for bf16 params (master-state Adam) so that
  bf16-true training matches the reference's quality.
* :class:`RMSpropTF` — TensorFlow-style RMSprop (eps inside the sqrt,
  square_avg initialized to ones); parity: sheeprl/optim/rmsprop_tf.py:14-156
  (reference uses it for Dreamer-V1).
"""

from __future__ import annotations

from typing import Iterable

import torch
from torch import Tensor

from sheeprl_amd.ops._ext import require_ext, use_hip


def _reinstall_fp32_state(opt: torch.optim.Optimizer, state_dict: dict) -> None:
    """Undo ``Optimizer.load_state_dict``'s cast of tensor state to the
    parameter dtype: re-install every saved tensor as float32 on the
    parameter's device, bit-identical to what was saved.  The HIP kernels read
    these buffers as ``float*``; a bf16 copy would be half the size."""
    saved_ids = [i for g in state_dict["param_groups"] for i in g["params"]]
    params = [p for g in opt.param_groups for p in g["params"]]
    for i, p in zip(saved_ids, params):
        saved = state_dict["state"].get(i)
        if saved is None:
            continue
        st = opt.state[p]
        for k, v in saved.items():
            if isinstance(v, Tensor) and v.is_floating_point():
                st[k] = v.detach().to(device=p.device, dtype=torch.float32, copy=True)


def _require_fp32(opt_name: str, tensors) -> None:
    for t in tensors:
        if t is not None and t.dtype is not torch.float32:
            raise RuntimeError(
                f"{opt_name}: optimizer state must be float32 for the HIP kernels, got {t.dtype}. "
                "State is kept in fp32 for every parameter dtype; something cast it "
                "(torch's Optimizer.load_state_dict does, use this class's own)."
            )


class FusedAdam(torch.optim.Optimizer):
    _ADAM_CHUNK = 4096  # elements per block; must match kAdamChunk in the HIP kernel

    def __init__(
        self,
        params: Iterable,
        lr: float = 1e-3,
        betas: tuple = (0.9, 0.999),
        eps: float = 1e-8,
        weight_decay: float = 0.0,
    ) -> None:
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._zeroes_grads_in_kernel = False
        self._mt_cache = {}
        # host mirror of each group's device step counter: id(group) -> value
        # the counter holds after the last launch issued from here
        self._step_host = {}

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        _reinstall_fp32_state(self, state_dict)
        # the groups are new dicts and the state tensors new storage
        self._mt_cache = {}
        self._step_host = {}

    def _device_step(self, group, params, step: int) -> Tensor:
        """The group's device-side step counter (bias correction reads it in
        the kernel, so a captured step replays with advancing counts).  It is
        stored as ``step_t`` in the state of the first parameter that had
        state when it was created, never in an uninitialised state dict, and
        is found again by scanning the group, so a parameter whose gradient
        is missing cannot disturb it.  Allocated once: the address is stable."""
        dev = params[0].device
        state = self.state
        holder = None
        for p in group["params"]:
            if p in state and "step_t" in state[p]:
                holder = p
                break
        if holder is not None and state[holder]["step_t"].device != dev:
            del state[holder]["step_t"]
            holder = None
        key = id(group)
        if holder is None:
            step_t = torch.zeros(1, dtype=torch.float32, device=dev)
            step_t.fill_(float(step - 1))
            state[params[0]]["step_t"] = step_t
        else:
            step_t = state[holder]["step_t"]
            # every launch from here advances counter and host step together;
            # they part only when the set of stepping parameters changed
            if self._step_host.get(key, step - 1) != step - 1:
                step_t.fill_(float(step - 1))
        self._step_host[key] = step
        return step_t

    def zero_grad(self, set_to_none: bool = True) -> None:
        # on GPU the multi-tensor kernel zeroes each grad in place right after
        # consuming it, so the training loop's zero_grad is a no-op (keeping
        # grad buffers alive also keeps their addresses stable for the cached
        # chunk table and for hipGraph capture)
        if self._zeroes_grads_in_kernel:
            return
        super().zero_grad(set_to_none=set_to_none)

    def _chunk_table(self, group, params, grads, exp_avgs, exp_avg_sqs):
        """Build (or reuse) the device-side pointer/chunk table for one launch."""
        dev = params[0].device
        ptr_sig = [p.data_ptr() for p in params] + [g.data_ptr() for g in grads]
        cache = self._mt_cache
        key = id(group)
        ent = cache.get(key)
        if ent is not None and ent["sig"] == ptr_sig:
            return ent
        ptrs, sizes, ctid, coff = [], [], [], []
        for k, (p, g, m, v) in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs)):
            ptrs.append([p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()])
            n = p.numel()
            sizes.append(n)
            for off in range(0, n, self._ADAM_CHUNK):
                ctid.append(k)
                coff.append(off)
        ent = {
            "sig": ptr_sig,
            "ptrs": torch.tensor(ptrs, dtype=torch.int64, device=dev),
            "sizes": torch.tensor(sizes, dtype=torch.int64, device=dev),
            "ctid": torch.tensor(ctid, dtype=torch.int32, device=dev),
            "coff": torch.tensor(coff, dtype=torch.int64, device=dev),
        }
        cache[key] = ent
        return ent

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # re-derived every step from the path actually taken: only the
        # multi-tensor kernel zeroes grads in place, so a single group (or
        # step) falling back to the dev/eager path must re-enable the training
        # loop's zero_grad or gradients would accumulate across steps
        all_groups_zeroed_in_kernel = True
        for group in self.param_groups:
            params, grads, exp_avgs, exp_avg_sqs = [], [], [], []
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p, dtype=torch.float32)
                    state["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32)
                state["step"] += 1
                params.append(p)
                grads.append(p.grad)
                exp_avgs.append(state["exp_avg"])
                exp_avg_sqs.append(state["exp_avg_sq"])
            if not params:
                continue
            beta1, beta2 = group["betas"]
            # torch.optim.Adam semantics: each parameter is bias-corrected with
            # its own step count.  Normally every parameter stepping now shares
            # one count and the shared-counter paths below apply; a parameter
            # that joined late (its first gradients were None) sends the group
            # to the per-parameter path at the bottom
            steps = [self.state[p]["step"] for p in params]
            step = steps[0]
            uniform = all(s == step for s in steps)
            bc1 = 1 - beta1**step
            bc2 = 1 - beta2**step
            def _dense_same_layout(p, g):
                # elementwise update only needs p/g/m/v to share one dense
                # memory layout — channels_last conv weights qualify
                return (
                    p.dtype == params[0].dtype
                    and g.stride() == p.stride()
                    and (p.is_contiguous() or p.is_contiguous(memory_format=torch.channels_last))
                )

            if uniform and use_hip(params[0]) and all(_dense_same_layout(p, g) for p, g in zip(params, grads)):
                # device-side step counter: bias correction is computed in the
                # kernel from a device scalar so the step is hipGraph-capturable;
                # chunk table makes the whole group ONE kernel launch
                step_t = self._device_step(group, params, step)
                _require_fp32("FusedAdam", exp_avgs + exp_avg_sqs + [step_t])
                ent = self._chunk_table(group, params, grads, exp_avgs, exp_avg_sqs)
                require_ext().adam_step_mt(
                    ent["ptrs"], ent["sizes"], ent["ctid"], ent["coff"],
                    step_t, params[0], True,
                    group["lr"], beta1, beta2, group["eps"], group["weight_decay"],
                    True,
                )
            elif uniform and use_hip(params[0]) and all(
                # the dev kernel walks p flat and contiguous()-copies g: both
                # must be standard-contiguous or the orders diverge
                p.is_contiguous() and g.is_contiguous() for p, g in zip(params, grads)
            ):
                step_t = self._device_step(group, params, step)
                _require_fp32("FusedAdam", exp_avgs + exp_avg_sqs + [step_t])
                all_groups_zeroed_in_kernel = False
                require_ext().adam_step_dev(
                    params,
                    grads,
                    exp_avgs,
                    exp_avg_sqs,
                    step_t,
                    group["lr"],
                    beta1,
                    beta2,
                    group["eps"],
                    group["weight_decay"],
                )
            elif uniform and all(p.dtype == torch.float32 and g.dtype == torch.float32 for p, g in zip(params, grads)):
                # foreach eager path (CPU / non-HIP): one C++ multi-tensor op
                # per stage instead of a Python loop per parameter — the loop
                # measured ~3 ms/step on the CPU SAC wall-clock benchmark
                all_groups_zeroed_in_kernel = False
                if group["weight_decay"] != 0:
                    grads = torch._foreach_add(grads, params, alpha=group["weight_decay"])
                torch._foreach_mul_(exp_avgs, beta1)
                torch._foreach_add_(exp_avgs, grads, alpha=1 - beta1)
                torch._foreach_mul_(exp_avg_sqs, beta2)
                torch._foreach_addcmul_(exp_avg_sqs, grads, grads, value=1 - beta2)
                denom = torch._foreach_div(exp_avg_sqs, bc2)
                torch._foreach_sqrt_(denom)
                torch._foreach_add_(denom, group["eps"])
                upd = torch._foreach_div(exp_avgs, bc1)
                torch._foreach_div_(upd, denom)
                torch._foreach_add_(params, upd, alpha=-group["lr"])
            else:
                all_groups_zeroed_in_kernel = False
                for p, g, m, v, s in zip(params, grads, exp_avgs, exp_avg_sqs, steps):
                    gf = g.float()
                    if group["weight_decay"] != 0:
                        gf = gf.add(p.float(), alpha=group["weight_decay"])
                    m.mul_(beta1).add_(gf, alpha=1 - beta1)
                    v.mul_(beta2).addcmul_(gf, gf, value=1 - beta2)
                    denom = (v / (1 - beta2**s)).sqrt_().add_(group["eps"])
                    upd = (m / (1 - beta1**s)) / denom
                    p.add_((-group["lr"] * upd).to(p.dtype))
        self._zeroes_grads_in_kernel = all_groups_zeroed_in_kernel
        return loss


def make_optimizer(params: Iterable, opt_cfg) -> torch.optim.Optimizer:
    """Build the optimizer named by an algo config's ``optimizer`` block.

    Parity: the reference selects the optimizer class per module via its
    ``configs/optim/{adam,rmsprop,sgd}.yaml`` Hydra group
    (sheeprl/configs/optim/adam.yaml:2, rmsprop.yaml:2); here the same choice
    is the ``name`` field of each algo's ``optimizer`` block
    (adam | rmsprop_tf | sgd).  Unknown names fail loudly.
    """
    name = str(opt_cfg.get("name", "adam")).lower()
    lr = float(opt_cfg.lr)
    wd = float(opt_cfg.get("weight_decay", 0.0) or 0.0)  # configs may carry null
    if name in ("adam", "fused_adam", "adamw"):
        return FusedAdam(
            params, lr=lr,
            betas=tuple(opt_cfg.get("betas", (0.9, 0.999))),
            eps=float(opt_cfg.get("eps", 1e-8)),
            weight_decay=wd,
        )
    if name in ("rmsprop", "rmsprop_tf", "rmsproptf"):
        return RMSpropTF(
            params, lr=lr,
            alpha=float(opt_cfg.get("alpha", 0.9)),
            eps=float(opt_cfg.get("eps", 1e-10)),
            weight_decay=wd,
            momentum=float(opt_cfg.get("momentum", 0.0)),
            centered=bool(opt_cfg.get("centered", False)),
        )
    if name == "sgd":
        return torch.optim.SGD(
            params, lr=lr,
            momentum=float(opt_cfg.get("momentum", 0.0)),
            weight_decay=wd,
            nesterov=bool(opt_cfg.get("nesterov", False)),
        )
    raise ValueError(f"unknown optimizer name {name!r} (expected adam | rmsprop_tf | sgd)")


class RMSpropTF(torch.optim.Optimizer):
    """TF-style RMSprop: v <- rho v + (1-rho) g^2; update = g / sqrt(v + eps)
    (eps INSIDE the sqrt), square_avg initialized to ONES, momentum optional.
    """

    _CHUNK = 4096  # must match kAdamChunk in the HIP kernel

    def __init__(
        self,
        params: Iterable,
        lr: float = 1e-2,
        alpha: float = 0.9,
        eps: float = 1e-10,
        weight_decay: float = 0.0,
        momentum: float = 0.0,
        centered: bool = False,
    ) -> None:
        defaults = dict(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum, centered=centered)
        super().__init__(params, defaults)
        self._mt_cache = {}

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        _reinstall_fp32_state(self, state_dict)
        self._mt_cache = {}

    def _chunk_table(self, group, params, grads, sqs, mbs, gas):
        dev = params[0].device
        ptr_sig = [p.data_ptr() for p in params] + [g.data_ptr() for g in grads]
        ent = self._mt_cache.get(id(group))
        if ent is not None and ent["sig"] == ptr_sig:
            return ent
        ptrs, sizes, ctid, coff = [], [], [], []
        for k, (p, g, sq, mb, ga) in enumerate(zip(params, grads, sqs, mbs, gas)):
            ptrs.append([p.data_ptr(), g.data_ptr(), sq.data_ptr(),
                         mb.data_ptr() if mb is not None else 0,
                         ga.data_ptr() if ga is not None else 0])
            n = p.numel()
            sizes.append(n)
            for off in range(0, n, self._CHUNK):
                ctid.append(k)
                coff.append(off)
        ent = {
            "sig": ptr_sig,
            "ptrs": torch.tensor(ptrs, dtype=torch.int64, device=dev),
            "sizes": torch.tensor(sizes, dtype=torch.int64, device=dev),
            "ctid": torch.tensor(ctid, dtype=torch.int32, device=dev),
            "coff": torch.tensor(coff, dtype=torch.int64, device=dev),
        }
        self._mt_cache[id(group)] = ent
        return ent

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            # one-launch multi-tensor HIP path (same chunk-table scheme as
            # FusedAdam)
            mt = [p for p in group["params"] if p.grad is not None]
            if mt and use_hip(mt[0]) and all(
                # elementwise: p/g/state only need to share one dense layout
                # (state is *_like(p)), so channels_last conv weights qualify
                p.dtype == mt[0].dtype
                and p.grad.stride() == p.stride()
                and (p.is_contiguous() or p.is_contiguous(memory_format=torch.channels_last))
                for p in mt
            ):
                sqs, mbs, gas = [], [], []
                for p in mt:
                    state = self.state[p]
                    if len(state) == 0:
                        state["square_avg"] = torch.ones_like(p, dtype=torch.float32)
                        if group["momentum"] > 0:
                            state["momentum_buffer"] = torch.zeros_like(p, dtype=torch.float32)
                        if group["centered"]:
                            state["grad_avg"] = torch.zeros_like(p, dtype=torch.float32)
                    sqs.append(state["square_avg"])
                    mbs.append(state.get("momentum_buffer"))
                    gas.append(state.get("grad_avg"))
                _require_fp32("RMSpropTF", sqs + mbs + gas)
                ent = self._chunk_table(group, mt, [p.grad for p in mt], sqs, mbs, gas)
                require_ext().rmsprop_step_mt(
                    ent["ptrs"], ent["sizes"], ent["ctid"], ent["coff"], mt[0],
                    group["lr"], group["alpha"], group["eps"], group["weight_decay"],
                    group["momentum"], bool(group["centered"]), False,
                )
                continue
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad.float()
                state = self.state[p]
                if len(state) == 0:
                    state["square_avg"] = torch.ones_like(p, dtype=torch.float32)
                    if group["momentum"] > 0:
                        state["momentum_buffer"] = torch.zeros_like(p, dtype=torch.float32)
                    if group["centered"]:
                        state["grad_avg"] = torch.zeros_like(p, dtype=torch.float32)
                if group["weight_decay"] != 0:
                    g = g.add(p.float(), alpha=group["weight_decay"])
                sq = state["square_avg"]
                one_minus_alpha = 1.0 - group["alpha"]
                sq.add_(g.pow(2) - sq, alpha=one_minus_alpha)
                if group["centered"]:
                    ga = state["grad_avg"]
                    ga.add_(g - ga, alpha=one_minus_alpha)
                    avg = sq.addcmul(ga, ga, value=-1).add_(group["eps"]).sqrt_()
                else:
                    avg = sq.add(group["eps"]).sqrt_()
                if group["momentum"] > 0:
                    buf = state["momentum_buffer"]
                    buf.mul_(group["momentum"]).addcdiv_(g, avg)
                    p.add_((-group["lr"] * buf).to(p.dtype))
                else:
                    p.add_((-group["lr"] * g / avg).to(p.dtype))
        return loss
