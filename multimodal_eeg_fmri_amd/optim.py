"""Flat parameter bucket + fused clip/AdamW (``mm_sumsq`` + ``mm_adamw_clip``, or ``mm_adamw_clip_ema`` when an
exponential moving average of the weights is kept: same launch, one more read and one more write stream).

Replaces the reference's ``clip_grad_norm_(max_norm=1.0)`` + ``torch.optim.AdamW.step()``
pair (run_training_lite.py:487-488, _test_bridge.py:784-786) with two kernel
launches over one contiguous fp32 buffer."""
from __future__ import annotations

import contextlib

import torch

from . import _hip, ops


def check_ema_decay(ema_decay, who: str):
    """``ema_decay`` is 0 (no average) or a decay in (0, 1): ValueError otherwise"""
    if not 0.0 <= float(ema_decay) < 1.0:
        raise ValueError(f"{who}: ema_decay must be in [0, 1) (got {ema_decay}); 0 = no averaged weights")


class FlatBucket:
    """All trainable parameters (and their gradients / Adam moments) as single
    contiguous fp32 buffers; ``param.data`` and ``param._mm_grad`` are views, so
    kernels accumulate gradients in place and one collective covers the step.
    ``ema=True``: ``self.ema`` is one more flat fp32 buffer, a copy of ``self.p`` made after the parameters were copied
    in - the averaged weights that ``mm_adamw_clip_ema`` maintains (None otherwise)."""

    def __init__(self, params, ema: bool = False):
        self.params = [p for p in params if p.requires_grad]
        n = sum(p.numel() for p in self.params)
        dev = self.params[0].device
        self.n = n
        self.p = torch.empty(n, dtype=torch.float32, device=dev)
        self.g = torch.zeros(n, dtype=torch.float32, device=dev)
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        self.state = torch.zeros(8 + 1024, dtype=torch.float32, device=dev)   # MM_OPT_STATE_FLOATS
        off = 0
        for p in self.params:
            k = p.numel()
            self.p[off:off + k].copy_(p.detach().reshape(-1))
            p.data = self.p[off:off + k].view(p.shape)
            p._mm_grad = self.g[off:off + k].view(p.shape)
            off += k
        self.ema = self.p.clone() if ema else None

    def zero_grad(self):
        self.g.zero_()
        for p in self.params:
            p.grad = None

    @contextlib.contextmanager
    def swapped(self):
        """exchange the contents of ``p`` and ``ema`` in place (pointers and parameter views stay valid; copies are
        exact) and exchange them back on exit"""
        def exchange():
            with torch.no_grad():
                tmp = self.p.clone()
                self.p.copy_(self.ema)
                self.ema.copy_(tmp)
            ops.weights_changed()
        exchange()
        try:
            yield self
        finally:
            exchange()

    def absorb_autograd_grads(self):
        """parameters whose gradient came back through autograd (not a kernel sink)"""
        for p in self.params:
            if p.grad is not None:
                p._mm_grad.add_(p.grad)
                p.grad = None


class FusedAdamW:
    """torch.optim.AdamW-like surface (``param_groups[0]['lr']``, ``zero_grad``, ``step``)
    with the global-norm clip folded in (``max_grad_norm`` <= 0 disables it).
    ``ema_decay`` in (0, 1): ``step()`` also keeps an exponential moving average of the weights (``bucket.ema``), in the
    update kernel itself: ``ema += (1 - d) * (p - ema)`` after every step, ``d = min(ema_decay, (1 + t) / (10 + t))`` at
    step count t with ``ema_warmup`` (the usual warm-up of the decay, so that the first steps are not averaged with the
    initialisation for long), ``d = ema_decay`` without.  0 (default): no average, the launches are unchanged."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01,
                 max_grad_norm: float = 0.0, ema_decay: float = 0.0, ema_warmup: bool = True):
        check_ema_decay(ema_decay, "FusedAdamW")
        self.ema_decay, self.ema_warmup = float(ema_decay), bool(ema_warmup)
        self._averaged = False
        self._all = list(params)                  # torch's state_dict numbers EVERY param of the group
        self.bucket = FlatBucket(self._all, ema=self.ema_decay > 0)
        self.param_groups = [{"lr": lr, "params": self.bucket.params}]
        self.betas, self.eps, self.weight_decay, self.max_grad_norm = betas, eps, weight_decay, max_grad_norm
        ops.weights_changed()

    def zero_grad(self, set_to_none: bool = True):
        self.bucket.zero_grad()

    def step(self):
        b = self.bucket
        b.absorb_autograd_grads()
        b.state[2] = float(self.param_groups[0]["lr"])
        if self._averaged:
            raise RuntimeError("FusedAdamW.step inside averaged(): the parameters hold the averaged weights")
        _hip.call("mm_sumsq", b.g, b.state, b.n)
        if b.ema is None:
            _hip.call("mm_adamw_clip", b.p, b.g, b.m, b.v, b.state, b.n, self.betas[0], self.betas[1],
                      self.eps, self.weight_decay, float(self.max_grad_norm), 1.0, 0, None)
        else:
            _hip.call("mm_adamw_clip_ema", b.p, b.g, b.m, b.v, b.state, b.n, self.betas[0], self.betas[1],
                      self.eps, self.weight_decay, float(self.max_grad_norm), 1.0, 0, None,
                      b.ema, self.ema_decay, int(self.ema_warmup))
        ops.weights_changed()

    # -- averaged weights
    def _need_ema(self, who: str):
        if self.bucket.ema is None:
            raise RuntimeError(f"FusedAdamW.{who}: built without ema_decay, there are no averaged weights")

    @torch.no_grad()
    def sync_ema(self):
        """set the average to the live weights"""
        self._need_ema("sync_ema")
        self.bucket.ema.copy_(self.bucket.p)

    @contextlib.contextmanager
    def averaged(self):
        """inside, the parameters hold the averaged weights (the contents of ``bucket.p`` and ``bucket.ema`` are
        exchanged in place, so parameter views and captured pointers stay valid); the live bits return on exit.
        ``step()`` inside raises RuntimeError."""
        self._need_ema("averaged")
        if self._averaged:
            raise RuntimeError("FusedAdamW.averaged: already inside averaged()")
        with self.bucket.swapped():
            self._averaged = True
            try:
                yield self
            finally:
                self._averaged = False

    # -- checkpoint drop-in: the dict layout of torch.optim.AdamW.state_dict(), so a
    # FlexibleTrainer checkpoint (EEG notebook cell 23: 'optimizer_state_dict') moves both ways.
    def _slices(self):
        off = 0
        index = {id(p): i for i, p in enumerate(self._all)}
        for p in self.bucket.params:
            k = p.numel()
            yield index[id(p)], p, slice(off, off + k)
            off += k

    def state_dict(self):
        b = self.bucket
        step = float(b.state[0].item())
        state = {i: {"step": torch.tensor(step), "exp_avg": b.m[sl].view(p.shape).clone(),
                     "exp_avg_sq": b.v[sl].view(p.shape).clone()} for i, p, sl in self._slices()}
        group = {"lr": self.param_groups[0]["lr"], "betas": tuple(self.betas), "eps": self.eps,
                 "weight_decay": self.weight_decay, "amsgrad": False, "maximize": False, "foreach": None,
                 "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": True,
                 "params": list(range(len(self._all)))}
        sd = {"state": state, "param_groups": [group]}
        if b.ema is not None:                     # one extra top-level key, only when averaging is on
            sd["ema"] = {"decay": self.ema_decay, "warmup": self.ema_warmup, "shadow": b.ema.clone()}
        return sd

    def load_state_dict(self, sd):
        group = sd["param_groups"][0]
        if len(group["params"]) != len(self._all):
            raise ValueError("loaded state dict contains a parameter group that doesn't match the size of "
                             "optimizer's group")
        if group.get("amsgrad"):
            raise ValueError("FusedAdamW has no amsgrad state")
        b = self.bucket
        ema = sd.get("ema")
        # (a torch.optim.AdamW state dict has no "ema": the average is then left as it is - `sync_ema` after loading the
        # weights starts it from them)
        if ema is not None and b.ema is None:
            raise ValueError("FusedAdamW: the state dict carries averaged weights, this optimizer was built without ema_decay")
        if ema is not None and tuple(ema["shadow"].shape) != (b.n,):
            raise ValueError(f"FusedAdamW: ema.shadow has {tuple(ema['shadow'].shape)} elements, the bucket {b.n}")
        self.param_groups[0]["lr"] = group["lr"]
        self.betas, self.eps, self.weight_decay = tuple(group["betas"]), group["eps"], group["weight_decay"]
        steps = set()
        b.m.zero_(); b.v.zero_()
        for i, p, sl in self._slices():
            st = sd["state"].get(i)
            if st is None:
                continue
            b.m[sl].copy_(st["exp_avg"].reshape(-1))
            b.v[sl].copy_(st["exp_avg_sq"].reshape(-1))
            steps.add(float(st["step"]))
        if len(steps) > 1:
            raise ValueError("FusedAdamW keeps one step counter; the loaded per-parameter steps differ")
        b.state[0] = steps.pop() if steps else 0.0
        if ema is not None:
            b.ema.copy_(ema["shadow"])

    @property
    def last_grad_norm(self) -> float:
        return float(self.bucket.state[4])
