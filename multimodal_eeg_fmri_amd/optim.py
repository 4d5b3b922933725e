"""Flat parameter bucket + fused clip/AdamW.  `adamw_update` is the one host call of a step, for `FusedAdamW` and the
bridge trainer alike: ``mm_sumsq`` + ``mm_adamw_clip``, or ``mm_adamw_clip_ema`` when an exponential moving average of the
weights is kept (same launch, one more read and one more write stream); with parameter groups - learning-rate multipliers
and weight decays per segment of the bucket, `segment_table` - ``mm_adamw_clip_groups`` / ``mm_adamw_clip_groups_ema``.
The four entry points are instances of one kernel body.

Replaces the reference's ``clip_grad_norm_(max_norm=1.0)`` + ``torch.optim.AdamW.step()``
pair (run_training_lite.py:487-488, _test_bridge.py:784-786) with two kernel
launches over one contiguous fp32 buffer."""
from __future__ import annotations

import contextlib
import math

import torch

from . import _hip, ops


def check_ema_decay(ema_decay, who: str):
    """``ema_decay`` is 0 (no average) or a decay in (0, 1): ValueError otherwise"""
    if not 0.0 <= float(ema_decay) < 1.0:
        raise ValueError(f"{who}: ema_decay must be in [0, 1) (got {ema_decay}); 0 = no averaged weights")


MAX_SEGMENTS = 1024                               # MM_OPT_MAX_SEGMENTS


def check_lr_scale(value, who: str) -> float:
    """a learning-rate multiplier is a finite number >= 0 (0 holds the weights still while the moments move):
    ValueError otherwise"""
    try:
        x = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: lr_scale must be a number (got {value!r})") from None
    if not math.isfinite(x) or x < 0.0:
        raise ValueError(f"{who}: lr_scale must be finite and >= 0 (got {value})")
    return x


def segment_table(entries, who: str = "segment_table", tags: bool = False):
    """The host side of the segment table of ``mm_adamw_clip_groups``.  ``entries``: ``(numel, lr_scale, weight_decay)``
    or ``(numel, lr_scale, weight_decay, tag)`` per parameter, in bucket order.  Neighbours with equal
    ``(lr_scale, weight_decay, tag)`` merge into one segment (a tag keeps two ranges apart whose values are equal now
    but are changed separately later); entries of no elements vanish.  Returns ``(seg_end, seg_lr_mult, seg_wd)``:
    lists of equal length 1 .. ``MAX_SEGMENTS``, the ends strictly increasing and the last one the bucket's size
    (``tags=True``: and the list of the segments' tags).
    ValueError: a multiplier that is negative, NaN or infinite, a weight decay that is, a negative size, no element at
    all, or more than ``MAX_SEGMENTS`` segments."""
    ends, mults, wds, seg_tags = [], [], [], []
    off = 0
    for e in entries:
        k, scale, wd = int(e[0]), check_lr_scale(e[1], who), float(e[2])
        tag = e[3] if len(e) > 3 else None
        if k < 0:
            raise ValueError(f"{who}: a parameter of {k} elements")
        if not math.isfinite(wd) or wd < 0.0:
            raise ValueError(f"{who}: weight_decay must be finite and >= 0 (got {e[2]})")
        if k == 0:
            continue
        off += k
        if ends and (mults[-1], wds[-1], seg_tags[-1]) == (scale, wd, tag):
            ends[-1] = off
        else:
            ends.append(off); mults.append(scale); wds.append(wd); seg_tags.append(tag)
    if not ends:
        raise ValueError(f"{who}: no elements")
    if len(ends) > MAX_SEGMENTS:
        raise ValueError(f"{who}: {len(ends)} segments, the update kernel takes at most {MAX_SEGMENTS} (order the parameters "
                         "so that equal (lr_scale, weight_decay) are neighbours)")
    return (ends, mults, wds, seg_tags) if tags else (ends, mults, wds)


class SegmentTable:
    """``segment_table``'s lists as the device arrays ``mm_adamw_clip_groups`` reads: ``end`` int64, ``mult`` and ``wd``
    fp32, ``n_seg`` values each.  The arrays are written in place (`write`), so a captured launch that holds their
    pointers serves later values; the number of segments of a table is fixed."""

    def __init__(self, ends, mults, wds, device):
        self.n_seg = len(ends)
        self.ends, self.mults, self.wds = list(ends), list(mults), list(wds)
        self.end = torch.tensor(self.ends, dtype=torch.int64, device=device)
        self.mult = torch.tensor(self.mults, dtype=torch.float32, device=device)
        self.wd = torch.tensor(self.wds, dtype=torch.float32, device=device)

    @property
    def uniform(self) -> bool:
        """multiplier 1 everywhere and one weight decay: the step of the plain kernel"""
        return all(m == 1.0 for m in self.mults) and len(set(self.wds)) == 1

    def write(self, mults=None, wds=None):
        """new multipliers and / or decays for the same segments, copied into the device arrays"""
        for new, host, devt in ((mults, self.mults, self.mult), (wds, self.wds, self.wd)):
            if new is None:
                continue
            if len(new) != self.n_seg:
                raise ValueError(f"SegmentTable.write: {len(new)} values for {self.n_seg} segments")
            host[:] = [float(x) for x in new]
            devt.copy_(torch.tensor(host, dtype=torch.float32))


def adamw_update(b, betas, eps, max_norm, grad_scale, zero_grad, seed_epoch, decay, ema_decay=0.0, ema_warmup=True):
    """The two launches of a step on FlatBucket ``b``: ``mm_sumsq``, then the one matching entry point of the update
    kernel.  ``decay``: a scalar weight decay (``mm_adamw_clip``) or a SegmentTable in its place (``mm_adamw_clip_groups``);
    ``_ema`` - the weight average rides along in the same launch - exactly when ``b.ema`` exists."""
    _hip.call("mm_sumsq", b.g, b.state, b.n)
    grouped, averaged = isinstance(decay, SegmentTable), b.ema is not None
    args = [b.p, b.g, b.m, b.v, b.state, b.n, betas[0], betas[1], eps]
    args += [] if grouped else [float(decay)]
    args += [float(max_norm), float(grad_scale), int(zero_grad), seed_epoch]
    args += [decay.end, decay.mult, decay.wd, decay.n_seg] if grouped else []
    args += [b.ema, float(ema_decay), int(ema_warmup)] if averaged else []
    _hip.call("mm_adamw_clip" + "_groups" * grouped + "_ema" * averaged, *args)


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
    initialisation for long), ``d = ema_decay`` without.  0 (default): no average, the launches are unchanged.
    ``params``: parameters, or torch-style groups ``[{"params": a}, {"params": b, "lr_scale": 0.1, "weight_decay": 0.0}]``.
    ``param_groups[i]["lr"]`` is the BASE learning rate, one value shared by all groups (``step()`` raises ValueError when
    they disagree; a scheduler that sets every group to the same value keeps the ratios); ``lr_scale`` (default 1, finite,
    >= 0) multiplies it for the group, ``weight_decay`` defaults to the constructor's.  The bucket is laid out in group
    order, neighbours with equal ``(lr_scale, weight_decay)`` share one segment of the table (`segment_table`); one
    segment of multiplier 1 - a plain parameter list - launches ``mm_adamw_clip[_ema]`` as ever, anything else
    ``mm_adamw_clip_groups[_ema]``.  The norm that is clipped is over all groups."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01,
                 max_grad_norm: float = 0.0, ema_decay: float = 0.0, ema_warmup: bool = True):
        check_ema_decay(ema_decay, "FusedAdamW")
        self.ema_decay, self.ema_warmup = float(ema_decay), bool(ema_warmup)
        self._averaged = False
        params = list(params)
        groups = params if params and isinstance(params[0], dict) else [{"params": params}]
        self._group_all = []                      # every param of each group: torch's state_dict numbers them ALL
        self.param_groups = []
        for gr in groups:
            unknown = set(gr) - {"params", "lr", "lr_scale", "weight_decay"}
            if unknown:
                raise ValueError(f"FusedAdamW: a parameter group has the keys {sorted(unknown)}; betas and eps are shared, "
                                 "a group sets lr_scale and weight_decay")
            ps = list(gr["params"])
            self._group_all.append(ps)
            self.param_groups.append({"lr": gr.get("lr", lr), "params": [p for p in ps if p.requires_grad],
                                      "lr_scale": check_lr_scale(gr.get("lr_scale", 1.0), "FusedAdamW"),
                                      "weight_decay": gr.get("weight_decay", weight_decay)})
        self._all = [p for ps in self._group_all for p in ps]
        if len({id(p) for p in self._all}) != len(self._all):
            raise ValueError("FusedAdamW: some parameters appear in more than one parameter group")
        self.bucket = FlatBucket(self._all, ema=self.ema_decay > 0)
        self.betas, self.eps, self.max_grad_norm = betas, eps, max_grad_norm
        self._table = None                        # SegmentTable of the last step that needed one
        self._host_table()                        # (more than MAX_SEGMENTS segments: ValueError here, not at step 1)
        ops.weights_changed()

    @property
    def weight_decay(self):
        """the weight decay of group 0 - of every parameter when ``params`` was a plain list"""
        return self.param_groups[0]["weight_decay"]

    @weight_decay.setter
    def weight_decay(self, value):
        self.param_groups[0]["weight_decay"] = value

    def zero_grad(self, set_to_none: bool = True):
        self.bucket.zero_grad()

    def _host_table(self):
        return segment_table([(p.numel(), gr["lr_scale"], gr["weight_decay"]) for gr in self.param_groups
                              for p in gr["params"]], "FusedAdamW")

    def step(self):
        b = self.bucket
        b.absorb_autograd_grads()
        lrs = {float(gr["lr"]) for gr in self.param_groups}
        if len(lrs) != 1:
            raise ValueError(f"FusedAdamW.step: the groups' 'lr' is the shared base learning rate, they hold {sorted(lrs)}; "
                             "give a group its own rate with 'lr_scale'")
        b.state[2] = lrs.pop()
        if self._averaged:
            raise RuntimeError("FusedAdamW.step inside averaged(): the parameters hold the averaged weights")
        ends, mults, wds = self._host_table()     # (read every step: the groups' values may be changed between steps)
        decay = wds[0]                            # one segment of multiplier 1: the plain kernel
        if not (len(ends) == 1 and mults[0] == 1.0):
            decay = self._table
            if decay is None or decay.ends != ends:
                decay = self._table = SegmentTable(ends, mults, wds, b.p.device)
            elif (decay.mults, decay.wds) != (mults, wds):
                decay.write(mults, wds)
        adamw_update(b, self.betas, self.eps, self.max_grad_norm, 1.0, 0, None, decay, self.ema_decay, self.ema_warmup)
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
        groups, first = [], 0
        for gr, ps in zip(self.param_groups, self._group_all):
            groups.append({"lr": gr["lr"], "betas": tuple(self.betas), "eps": self.eps,
                           "weight_decay": gr["weight_decay"], "amsgrad": False, "maximize": False, "foreach": None,
                           "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": True,
                           "params": list(range(first, first + len(ps)))})
            if len(self.param_groups) > 1 or gr["lr_scale"] != 1.0:    # (a plain parameter list keeps its container)
                groups[-1]["lr_scale"] = gr["lr_scale"]
            first += len(ps)
        sd = {"state": state, "param_groups": groups}
        if b.ema is not None:                     # one extra top-level key, only when averaging is on
            sd["ema"] = {"decay": self.ema_decay, "warmup": self.ema_warmup, "shadow": b.ema.clone()}
        return sd

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        if len(groups) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups")
        if any(len(g["params"]) != len(ps) for g, ps in zip(groups, self._group_all)):
            raise ValueError("loaded state dict contains a parameter group that doesn't match the size of "
                             "optimizer's group")
        if any(g.get("amsgrad") for g in groups):
            raise ValueError("FusedAdamW has no amsgrad state")
        if any((tuple(g["betas"]), g["eps"]) != (tuple(groups[0]["betas"]), groups[0]["eps"]) for g in groups):
            raise ValueError("FusedAdamW shares betas and eps between its parameter groups; the loaded groups' differ")
        scales = [check_lr_scale(g.get("lr_scale", mine["lr_scale"]), "FusedAdamW.load_state_dict")
                  for g, mine in zip(groups, self.param_groups)]
        group = groups[0]
        b = self.bucket
        ema = sd.get("ema")
        # (a torch.optim.AdamW state dict has no "ema": the average is then left as it is - `sync_ema` after loading the
        # weights starts it from them)
        if ema is not None and b.ema is None:
            raise ValueError("FusedAdamW: the state dict carries averaged weights, this optimizer was built without ema_decay")
        if ema is not None and tuple(ema["shadow"].shape) != (b.n,):
            raise ValueError(f"FusedAdamW: ema.shadow has {tuple(ema['shadow'].shape)} elements, the bucket {b.n}")
        for mine, g, scale in zip(self.param_groups, groups, scales):
            mine["lr"], mine["weight_decay"], mine["lr_scale"] = g["lr"], g["weight_decay"], scale
        self.betas, self.eps = tuple(group["betas"]), group["eps"]
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
