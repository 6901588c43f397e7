"""models/optimizer.py:9-24 `get_optimizer`: Adam(lr) for cfg.TRAIN.OPTIMIZER == 'adam'
(the reference's SGD branch reads cfg keys that do not exist, so only Adam is live).

`HipAdam` / `HipSGD` are the opt-in HIP implementation of the stage: torch's update rules, one kernel launch per
parameter group through hp_optim_adam_multi / hp_optim_sgd_multi.  They subclass torch's classes, so `param_groups` and the
state keys (`step`, `exp_avg`, `exp_avg_sq`; `momentum_buffer`) are torch's and a `state_dict()` of either loads into the other.
Selected by cfg.TRAIN.OPTIMIZER == "adam_hip" / "sgd_hip" or by HP_OPTIMIZER_IMPL=hip; the default is torch's optimizer.
"""
import ctypes as C
import math
import os

import torch
from torch import optim

from ._lib import OptimAdamRec, OptimSgdRec


def _env_on(name: str, default: str = "0") -> bool:
    """An on / off environment switch: anything but "" and "0" is on (no int(): a stray value never raises at import)."""
    return os.environ.get(name, default) not in ("", "0")


def hip_optimizer_selected() -> bool:
    """HP_OPTIMIZER_IMPL=hip: `get_optimizer` returns the HIP classes for "adam" and "sgd" as well ("torch" names the default)."""
    return _env_on("HP_OPTIMIZER_IMPL") and os.environ["HP_OPTIMIZER_IMPL"].strip().lower() != "torch"


def _refuse(what: str):
    raise ValueError(f"{what} is not built in the HIP optimizer (use torch.optim for it)")


class _HipMultiTensor:
    """What HipAdam and HipSGD share: the checks of a group's parameters, the record table and the workspace."""

    _REC = None          # ctypes mirror of the record
    _WS_BYTES = None     # name of the workspace query
    _REFUSED = ()        # group options that are not built

    def _hp_check_group(self, group):
        for name in self._REFUSED:   # a loaded state_dict may carry them
            if group.get(name):
                _refuse(f"{name}=True")

    def _hp_live_params(self, group):
        """The group's parameters that have a gradient, checked; their device."""
        from ._lib import HiddenPoseHipError

        ps = [p for p in group["params"] if p.grad is not None]
        for p in ps:
            if p.grad.is_sparse:
                _refuse("a sparse gradient")
            if p.dtype != torch.float32 or p.grad.dtype != torch.float32:
                _refuse(f"a {p.dtype} parameter (gradient {p.grad.dtype}); fp32 only:")
            if not p.is_cuda:
                raise HiddenPoseHipError(f"{type(self).__name__}: parameter on {p.device}; this package has no CPU path")
            if p.device != ps[0].device:
                _refuse("a parameter group on several devices")
            if not p.is_contiguous():
                _refuse("a non-contiguous parameter")
        return ps

    def _hp_table(self, gi: int, count: int):
        """(record array, workspace tensor, its bytes) of group `gi`, kept between steps and grown when `count` does."""
        from . import _lib

        cache = self.__dict__.setdefault("_hp_cache", {})
        ent = cache.get(gi)
        if ent is None or ent[0] < count:
            cap = max(count, 2 * ent[0] if ent else 0)
            ent = (cap, (self._REC * cap)(), int(getattr(_lib.lib(), self._WS_BYTES)(cap)), {})
            cache[gi] = ent
        return ent

    @staticmethod
    def _hp_workspace(ent, dev):
        ws = ent[3].get(dev)
        if ws is None:
            ws = ent[3][dev] = torch.empty(ent[2], dtype=torch.uint8, device=dev)
        return ws

    @staticmethod
    def _hp_grad(p):
        g = p.grad
        return g if g.is_contiguous() else g.contiguous()

    def _hp_steps_to_host(self):
        """A `step` written by torch's fused / capturable optimizers lives on the device: bring it to the host once."""
        for st in self.state.values():
            s = st.get("step")
            if torch.is_tensor(s) and s.is_cuda:
                st["step"] = s.detach().to("cpu", torch.float32)
            elif s is not None and not torch.is_tensor(s):
                st["step"] = torch.tensor(float(s), dtype=torch.float32)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:   # which torch implementation wrote the state says nothing about this one
            group["foreach"] = False
            if "fused" in group:
                group["fused"] = None
        self._hp_steps_to_host()


class HipAdam(_HipMultiTensor, optim.Adam):
    """torch.optim.Adam (L2 weight decay) with the update in one HIP launch per parameter group."""

    _REC, _WS_BYTES = OptimAdamRec, "hp_optim_adam_multi_workspace_bytes"
    _REFUSED = ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None):
        for name, v in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable), ("differentiable", differentiable),
                        ("foreach", foreach), ("fused", fused)):
            if v:
                _refuse(f"{name}=True")
        if torch.is_tensor(lr):
            _refuse("a tensor lr")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)

    @torch.no_grad()
    def step(self, closure=None):
        from . import _lib

        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = _lib.lib()
        for gi, group in enumerate(self.param_groups):
            self._hp_check_group(group)
            ps = self._hp_live_params(group)
            if not ps:
                continue
            lr, (b1, b2) = float(group["lr"]), group["betas"]
            ent = self._hp_table(gi, len(ps))
            recs, scal, keep = ent[1], {}, []
            for i, p in enumerate(ps):
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                elif st["step"].is_cuda:
                    st["step"] = st["step"].detach().to("cpu", torch.float32)
                st["step"] += 1
                t = st["step"].item()
                sc = scal.get(t)
                if sc is None:   # in double from THIS tensor's step count, rounded once
                    sc = scal[t] = (lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t))
                g = self._hp_grad(p)
                keep.append(g)
                r = recs[i]
                r.p, r.g, r.m, r.v, r.n = p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()
                r.lr_over_bc1, r.inv_sqrt_bc2 = sc
            dev = ps[0].device
            with torch.cuda.device(dev):
                ws = self._hp_workspace(ent, dev)
                _lib.check(L.hp_optim_adam_multi(C.addressof(recs), len(ps), b1, b2, group["eps"], group["weight_decay"],
                                                 ws.data_ptr(), ent[2], _lib.current_stream_handle(dev)), "hp_optim_adam_multi")
        return loss


class HipSGD(_HipMultiTensor, optim.SGD):
    """torch.optim.SGD (momentum, dampening, Nesterov, weight decay) with the update in one HIP launch per parameter group."""

    _REC, _WS_BYTES = OptimSgdRec, "hp_optim_sgd_multi_workspace_bytes"
    _REFUSED = ("maximize", "differentiable")

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None):
        for name, v in (("maximize", maximize), ("differentiable", differentiable), ("foreach", foreach), ("fused", fused)):
            if v:
                _refuse(f"{name}=True")
        if torch.is_tensor(lr):
            _refuse("a tensor lr")
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                         foreach=False)

    @torch.no_grad()
    def step(self, closure=None):
        from . import _lib

        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = _lib.lib()
        for gi, group in enumerate(self.param_groups):
            self._hp_check_group(group)
            ps = self._hp_live_params(group)
            if not ps:
                continue
            mu = float(group["momentum"])
            ent = self._hp_table(gi, len(ps))
            recs, keep = ent[1], []
            for i, p in enumerate(ps):
                g = self._hp_grad(p)
                keep.append(g)
                r = recs[i]
                r.p, r.g, r.n, r.buf, r.first_step = p.data_ptr(), g.data_ptr(), p.numel(), None, 0
                if mu != 0.0:
                    st = self.state[p]
                    buf = st.get("momentum_buffer")
                    if buf is None:
                        buf = st["momentum_buffer"] = torch.empty_like(p, memory_format=torch.preserve_format)
                        r.first_step = 1
                    r.buf = buf.data_ptr()
            dev = ps[0].device
            with torch.cuda.device(dev):
                ws = self._hp_workspace(ent, dev)
                _lib.check(L.hp_optim_sgd_multi(C.addressof(recs), len(ps), float(group["lr"]), mu, float(group["dampening"]),
                                                float(group["weight_decay"]), 1 if group["nesterov"] else 0, ws.data_ptr(), ent[2],
                                                _lib.current_stream_handle(dev)), "hp_optim_sgd_multi")
        return loss


def get_optimizer(cfg, model):
    name = cfg.TRAIN.OPTIMIZER
    hip = hip_optimizer_selected()
    if name == "adam_hip" or (hip and name == "adam"):
        return HipAdam(list(model.parameters()), lr=cfg.TRAIN.LR)
    if name == "sgd_hip" or (hip and name == "sgd"):
        return HipSGD(list(model.parameters()), lr=cfg.TRAIN.LR, momentum=getattr(cfg.TRAIN, "MOMENTUM", 0.9),
                      weight_decay=getattr(cfg.TRAIN, "WD", 0.0), nesterov=getattr(cfg.TRAIN, "NESTEROV", False))
    if cfg.TRAIN.OPTIMIZER == "adam":
        params = list(model.parameters())
        # same update rule and state_dict layout; on the GPU the single fused kernel replaces ~50 multi-tensor launches
        fused = bool(params) and all(p.is_cuda for p in params) and __import__("os").environ.get("HP_ADAM_FUSED", "1") != "0"
        return optim.Adam(params, lr=cfg.TRAIN.LR, fused=fused)
    if cfg.TRAIN.OPTIMIZER == "sgd":
        return optim.SGD(model.parameters(), lr=cfg.TRAIN.LR, momentum=getattr(cfg.TRAIN, "MOMENTUM", 0.9),
                         weight_decay=getattr(cfg.TRAIN, "WD", 0.0), nesterov=getattr(cfg.TRAIN, "NESTEROV", False))
    return None
