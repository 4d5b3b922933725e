"""Checkpoint, resume and the epoch loop of the contrastive bridge trainer (`BridgeTrainer`).

The file is the container of the reference's loops and of `FlexibleTrainer.save_checkpoint` -
``{epoch, model_state_dict, optimizer_state_dict, scheduler_state_dict, metrics}`` - plus one key,
``bridge_trainer_state``, that holds what the reference's containers cannot express and an exact resume needs:

* ``model_state_dict``: the trainer's unchanged ``nn.Module.state_dict()`` (CPU copies);
* ``optimizer_state_dict``: the layout of ``torch.optim.AdamW.state_dict()`` over
  ``[p for p in trainer.parameters() if p.requires_grad]`` in ``parameters()`` order (the flat bucket is laid out by
  layer group, so its slices are mapped back to that order); the frozen half of the bridge has no entry;
* ``bridge_trainer_state``: the optimizer words (step count, lr, ...), the hyperparameters, the EEG branch kind, the
  model's shapes, the head count of every transformer block, the world size, the bucket layout, the dropout stream,
  the state of `fit`, - only for a trainer with an augmenter - ``augment``: its parameters and the step index
  (``fmri_augment``: the same for a volume augmenter; ``eeg_time_augment``: for a temporal EEG augmenter, whose step index
  is ``augment``'s), -
  only for a trainer of the pairwise sigmoid loss - ``loss`` = ``"sigmoid"`` (absent: InfoNCE), and - only for a trainer
  built with ``neighbour_radius > 0`` - ``neighbour_radius`` (absent: 0, no ignored neighbours), and - only for a trainer
  built with ``classify=True`` - ``classify`` = ``{ce_weight, num_classes, class_weight}``, and - only for a trainer with
  a cross-batch memory (``bank_size > 0``) - ``bank`` = ``{size, warmup, grouped, state, rows, ids}``: the ring's words,
  rows and group ids (``rows`` / ``ids`` None before the first training step; with ``key_encoder=True`` one more field,
  ``key_encoder`` = True: the rows are the key encoder's), and - only for a trainer that keeps
  averaged weights (``ema_decay > 0``) - ``ema`` = ``{decay, warmup, shadow}``: ``shadow`` is the flat fp32 average of
  the bucket (``bucket_n`` elements, bucket order), and - only for a trainer with parameter groups (a learning-rate
  multiplier other than 1, ``no_decay=True`` or a frozen encoder) - ``param_groups`` = ``{components, multipliers,
  no_decay, freeze, seg_end, seg_wd}``: the multipliers by component and the update kernel's segment table.
  ``model_state_dict`` always holds the live weights.

The step itself is untouched: saving and loading are copies, `fit` only calls `train_step` and `embed`.

Reference behaviour: the epoch loop with schedule, evaluation, early stop and best-state restore
(run_training_lite.py:465-520); best-state copy / restore (_test_bridge.py:876-892); loading ``model_state_dict`` or
a bare state dict (_test_bridge.py:499-504).
"""
from __future__ import annotations

import contextlib
import math
import os
import tempfile
from typing import Callable, Optional, Union

import torch

from . import dp, ops
from .bridge_staging import AUGMENTERS
from .enhanced_models_v4 import TemporalTransformerBlock

FORMAT = 1
CONTAINER_KEYS = ("epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "metrics",
                  "bridge_trainer_state")


class _LRWord(dict):
    """``param_groups[0]`` of the optimizer the schedule steps: setting ``"lr"`` writes the trainer's LR word"""

    def __init__(self, trainer):
        super().__init__(lr=float(trainer.lr))
        self._trainer = trainer

    def __setitem__(self, key, value):
        super().__setitem__(key, value)
        if key == "lr":
            self._trainer.set_lr(float(value))


class _LROptimizer:
    def __init__(self, trainer):
        self.param_groups = [_LRWord(trainer)]


def _cpu(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to("cpu", copy=True)


def monitor_value(metrics: dict, monitor: Union[str, Callable[[dict], float]]) -> float:
    """``"mean_R@1"``: the mean of R@1 over both retrieval directions; ``"<direction>.<key>"`` (e.g.
    ``"fmri_to_eeg.mrr"``): one entry of `retrieval_metrics`; a callable: ``monitor(metrics)``"""
    if callable(monitor):
        return float(monitor(metrics))
    if monitor == "mean_R@1":
        return 0.5 * (metrics["eeg_to_fmri"]["R@1"] + metrics["fmri_to_eeg"]["R@1"])
    d, _, k = monitor.partition(".")
    return float(metrics[d][k] if k else metrics[d])


class TrainerCheckpointMixin:
    """`BridgeTrainer`'s checkpoint / resume / `fit` surface (the trainer's attributes are used directly)."""

    # ------------------------------------------------------------------ layout
    def optimizer_param_map(self):
        """[(index in the AdamW layout, name, parameter, slice of the flat bucket)]: the trainable parameters in
        ``parameters()`` order, each with its range of ``bucket.p / m / v`` (the bucket is in layer-group order)"""
        offs, o = {}, 0
        for p in self.bucket.params:
            offs[id(p)] = slice(o, o + p.numel())
            o += p.numel()
        names = {id(p): n for n, p in self.named_parameters()}
        trainable = [p for p in self.parameters() if p.requires_grad]
        if {id(p) for p in trainable} != set(offs):
            raise RuntimeError("BridgeTrainer: the trainable parameters and the flat bucket disagree")
        return [(i, names[id(p)], p, offs[id(p)]) for i, p in enumerate(trainable)]

    def _block_heads(self) -> list:
        """[[module name, heads]] of every transformer block: 128 wide with 4 or 8 heads has the same shapes"""
        return [[n, int(m.nhead)] for n, m in self.named_modules() if isinstance(m, TemporalTransformerBlock)]

    def _layout(self) -> dict:
        return {"eeg_kind": self._eeg_kind,
                "heads": self._block_heads(),
                "shapes": {k: list(v.shape) for k, v in self.state_dict().items()},
                "bucket_n": int(self.bucket.n),
                "groups": [[n, r, int(lo), int(hi)] for n, r, lo, hi in self.groups],
                "world": int(self.world)}

    # ------------------------------------------------------------------ dropout stream
    def _dropout_stream_state(self) -> dict:
        """Graph mode with a captured step: the seeds were fixed when the capture began (its two warm-up steps draw
        first), so the counter at that point + the device epoch word the replays mix in.  Otherwise: the counter."""
        c = self._cap
        if self.mode == "graph" and c is not None and "seed_step" in c:
            return {"kind": "graph", "base": int(c["seed_base"]), "step": int(c["seed_step"]),
                    "epoch_word": int(c["epoch"].item())}
        return {"kind": "counter", "base": int(ops._seed_state["base"]), "step": int(ops._seed_state["step"]),
                "epoch_word": None}

    def _drop_capture(self):
        """forget the captured step (the next graph-mode `train_step` captures anew); its epoch word is uninstalled"""
        c = self._cap
        if c is None:
            return
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        if ops.EP() is c["epoch"]:
            ops.set_seed_epoch(None)
        self._cap = None
        self._works = []
        self.capture_mode = None

    def checkpoint_classify(self) -> Optional[dict]:
        """``bridge_trainer_state["classify"]``: None unless the trainer was built with classify=True"""
        if not getattr(self, "classify", False):
            return None
        cw = self._class_weight
        return {"ce_weight": float(self.ce_weight), "num_classes": int(self.num_classes),
                "class_weight": None if cw is None else [float(v) for v in cw.detach().cpu()]}

    def checkpoint_bank(self) -> Optional[dict]:
        """``bridge_trainer_state["bank"]``: None unless the trainer was built with bank_size > 0"""
        if not getattr(self, "_bank_size", 0):
            return None
        bank = self._bank
        out = {"size": int(self._bank_size), "warmup": int(self._bank_warmup), "grouped": self._bank_grouped,
               "state": [0, 0, 0, 0] if bank is None else [int(v) for v in bank.state.detach().cpu()],
               "rows": None if bank is None else _cpu(bank.bank), "ids": None if bank is None else _cpu(bank.gid)}
        if getattr(self, "_key_encoder", False):                   # (absent without a key encoder: the container is unchanged)
            out["key_encoder"] = True
        return out

    def checkpoint_fmri_branch(self) -> Optional[dict]:
        """``bridge_trainer_state["fmri_branch"]``: None unless the fMRI branch records more than the shapes say (a sequence
        encoder: its kind and frame count)"""
        branch = getattr(self, "_fmri", None)
        if branch is None or branch.checkpoint_tag is None:
            return None
        return {"kind": branch.kind, **branch.checkpoint_tag(self.fmri_encoder)}

    def checkpoint_ema(self) -> Optional[dict]:
        """``bridge_trainer_state["ema"]``: None unless the trainer was built with ema_decay > 0"""
        ema = getattr(self.bucket, "ema", None)
        if ema is None:
            return None
        return {"decay": float(self.ema_decay), "warmup": bool(self.ema_warmup), "shadow": _cpu(ema)}

    def checkpoint_param_groups(self) -> Optional[dict]:
        """``bridge_trainer_state["param_groups"]``: None while every learning-rate multiplier is 1, ``no_decay`` is off and
        nothing is frozen"""
        scales = getattr(self, "_lr_scale", None)
        if scales is None:
            return None
        frozen, no_decay = list(getattr(self, "_frozen", ())), bool(getattr(self, "no_decay", False))
        if all(v == 1.0 for v in scales.values()) and not no_decay and not frozen:
            return None
        t = self._table
        return {"components": list(self.COMPONENTS), "multipliers": [float(scales[c]) for c in self.COMPONENTS],
                "no_decay": no_decay, "freeze": frozen, "seg_end": [int(e) for e in t.ends],
                "seg_wd": [float(w) for w in t.wds]}

    # ------------------------------------------------------------------ state
    def checkpoint_state(self, epoch: Optional[int] = None, metrics: Optional[dict] = None, scheduler=None) -> dict:
        """the checkpoint container (CPU tensors, dicts, lists and Python scalars: loads with ``weights_only=True``)"""
        if getattr(self, "_ema_active", False):        # model_state_dict always holds the live weights
            raise RuntimeError("checkpoint_state inside ema_weights(): the parameters hold the averaged weights; leave "
                               "the context first")
        b = self.bucket
        words = _cpu(b.state)
        step = float(words[0])
        state = {}
        for i, _, p, sl in self.optimizer_param_map():
            state[i] = {"step": torch.tensor(step, dtype=torch.float32),
                        "exp_avg": _cpu(b.m[sl]).view(p.shape), "exp_avg_sq": _cpu(b.v[sl]).view(p.shape)}
        group = {"lr": float(self.lr), "betas": (float(self.betas[0]), float(self.betas[1])), "eps": float(self.eps),
                 "weight_decay": float(self.weight_decay), "amsgrad": False, "maximize": False, "foreach": None,
                 "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": True,
                 "params": list(range(len(state)))}
        bts = {"format": FORMAT, "optimizer_words": words, "step": step, "lr": float(self.lr),
               "hyper": {"betas": [float(self.betas[0]), float(self.betas[1])], "eps": float(self.eps),
                         "weight_decay": float(self.weight_decay), "grad_clip": float(self.grad_clip)},
               "dropout": self._dropout_stream_state(), "fit": getattr(self, "_fit_state", None)}
        bts.update(self._layout())
        for a in AUGMENTERS:                                       # (absent without that augmenter: the container is unchanged)
            if getattr(self, a.attr, None) is not None:
                bts[a.attr] = dict(getattr(self, a.attr).params(), step=int(getattr(self, a.counter)))
        if getattr(self, "loss", "infonce") != "infonce":          # (absent for the default loss: the container is unchanged)
            bts["loss"] = self.loss
        if getattr(self, "neighbour_radius", 0):                   # (absent at radius 0: the container is unchanged)
            bts["neighbour_radius"] = int(self.neighbour_radius)
        if self.checkpoint_classify() is not None:                 # (absent without classify: the container is unchanged)
            bts["classify"] = self.checkpoint_classify()
        if self.checkpoint_bank() is not None:                     # (absent without a bank: the container is unchanged)
            bts["bank"] = self.checkpoint_bank()
        if self.checkpoint_ema() is not None:                      # (absent without averaged weights: the container is unchanged)
            bts["ema"] = self.checkpoint_ema()
        if self.checkpoint_fmri_branch() is not None:              # (absent for the volume and tabular branches: the container is unchanged)
            bts["fmri_branch"] = self.checkpoint_fmri_branch()
        if self.checkpoint_param_groups() is not None:             # (absent at the defaults: the container is unchanged)
            bts["param_groups"] = self.checkpoint_param_groups()
        return {"epoch": epoch, "model_state_dict": {k: _cpu(v) for k, v in self.state_dict().items()},
                "optimizer_state_dict": {"state": state, "param_groups": [group]},
                "scheduler_state_dict": scheduler.state_dict() if scheduler is not None else None,
                "metrics": metrics, "bridge_trainer_state": bts}

    def _check_compatible(self, sd: dict):
        """ValueError naming the first field that differs; touches nothing"""
        missing = [k for k in CONTAINER_KEYS if k not in sd]
        if missing:
            raise ValueError(f"load_checkpoint_state: not a BridgeTrainer checkpoint (missing {missing})")
        bts = sd["bridge_trainer_state"]
        if bts.get("format") != FORMAT:
            raise ValueError(f"load_checkpoint_state: format {bts.get('format')} (this trainer reads {FORMAT})")
        mine = self._layout()

        def same(*fields):
            for field in fields:
                if bts.get(field) != mine[field]:
                    raise ValueError(f"load_checkpoint_state: {field} differs: checkpoint {bts.get(field)!r}, "
                                     f"trainer {mine[field]!r}")
        same("eeg_kind", "world")
        mine_fb, theirs_fb = self.checkpoint_fmri_branch(), bts.get("fmri_branch")
        if mine_fb != theirs_fb:                                   # before the shapes: lag_pool.* exists in one branch only
            words = lambda fb: "one fMRI item per pair (volume or tabular)" if fb is None else \
                ", ".join(f"{k}={v!r}" for k, v in fb.items())     # noqa: E731
            raise ValueError(f"load_checkpoint_state: fmri_branch differs: checkpoint [{words(theirs_fb)}], trainer "
                             f"[{words(mine_fb)}]")
        loss, theirs_loss = getattr(self, "loss", "infonce"), bts.get("loss", "infonce")
        if loss != theirs_loss:                                    # before the shapes: logit_bias exists under one loss only
            raise ValueError(f"load_checkpoint_state: loss differs: checkpoint {theirs_loss!r}, trainer {loss!r}")
        radius, theirs_radius = int(getattr(self, "neighbour_radius", 0)), int(bts.get("neighbour_radius", 0))
        if radius != theirs_radius:                                # the same weights under another loss: not a resume
            raise ValueError(f"load_checkpoint_state: neighbour_radius differs: checkpoint {theirs_radius}, trainer {radius}")
        mine_cls = self.checkpoint_classify()
        theirs_cls = bts.get("classify")
        if (mine_cls is None) != (theirs_cls is None):             # before the shapes and the bucket layout, which differ too
            raise ValueError(f"load_checkpoint_state: classify differs: the checkpoint was written "
                             f"{'with' if theirs_cls is not None else 'without'} classify=True, this trainer was built "
                             f"{'with' if mine_cls is not None else 'without'} it")
        if mine_cls is not None:
            for field in ("num_classes", "ce_weight", "class_weight"):
                if theirs_cls.get(field) != mine_cls[field]:
                    raise ValueError(f"load_checkpoint_state: classify.{field} differs: checkpoint "
                                     f"{theirs_cls.get(field)!r}, trainer {mine_cls[field]!r}")
        size, theirs_bank = getattr(self, "_bank_size", 0), bts.get("bank")
        if (size > 0) != (theirs_bank is not None):
            raise ValueError(f"load_checkpoint_state: bank differs: the checkpoint was written "
                             f"{'with' if theirs_bank is not None else 'without'} a cross-batch memory, this trainer was built "
                             f"{'with' if size > 0 else 'without'} one")
        if theirs_bank is not None:
            for field, mine_v in (("size", size), ("warmup", int(self._bank_warmup))):
                if theirs_bank.get(field) != mine_v:
                    raise ValueError(f"load_checkpoint_state: bank.{field} differs: checkpoint {theirs_bank.get(field)!r}, "
                                     f"trainer {mine_v!r}")
            mine_key = bool(getattr(self, "_key_encoder", False))
            if bool(theirs_bank.get("key_encoder", False)) != mine_key:
                raise ValueError(f"load_checkpoint_state: bank.key_encoder differs: the checkpoint's bank holds the rows of "
                                 f"{'a key encoder' if not mine_key else 'the online encoders'}, this trainer was built "
                                 f"{'with' if mine_key else 'without'} key_encoder=True")
            rows, N2 = theirs_bank.get("rows"), 2 * self.head.bridge.bridge_dim
            if rows is not None and (tuple(rows.shape) != (size, N2) or tuple(theirs_bank["ids"].shape) != (size,)):
                raise ValueError(f"load_checkpoint_state: bank.rows differ: checkpoint {tuple(rows.shape)}, trainer {(size, N2)}")
        mine_ema, theirs_ema = getattr(self.bucket, "ema", None), bts.get("ema")
        if (mine_ema is None) != (theirs_ema is None):
            raise ValueError(f"load_checkpoint_state: ema differs: the checkpoint was written "
                             f"{'with' if theirs_ema is not None else 'without'} averaged weights, this trainer was built "
                             f"{'with' if mine_ema is not None else 'without'} ema_decay")
        if theirs_ema is not None:
            for field, mine_v in (("decay", float(self.ema_decay)), ("warmup", bool(self.ema_warmup))):
                if theirs_ema.get(field) != mine_v:
                    raise ValueError(f"load_checkpoint_state: ema.{field} differs: checkpoint {theirs_ema.get(field)!r}, "
                                     f"trainer {mine_v!r}")
            shadow = theirs_ema.get("shadow")
            if shadow is None or tuple(shadow.shape) != (int(self.bucket.n),) or shadow.dtype != torch.float32:
                raise ValueError(f"load_checkpoint_state: ema.shadow differs: the trainer's bucket has {int(self.bucket.n)} "
                                 "fp32 elements")
        # parameter groups: before the bucket layout, which a frozen encoder changes too
        theirs_pg = bts.get("param_groups") or {}
        for field, mine_v in (("no_decay", bool(getattr(self, "no_decay", False))), ("freeze", list(getattr(self, "_frozen", ())))):
            theirs_v = theirs_pg.get(field, type(mine_v)())
            if theirs_v != mine_v:
                raise ValueError(f"load_checkpoint_state: {field} differs: checkpoint {theirs_v!r}, trainer {mine_v!r}")
        if theirs_pg:
            if list(theirs_pg.get("components", ())) != list(self.COMPONENTS) or len(theirs_pg.get("multipliers", ())) != len(self.COMPONENTS):
                raise ValueError(f"load_checkpoint_state: param_groups.components differ: checkpoint "
                                 f"{theirs_pg.get('components')!r}, trainer {list(self.COMPONENTS)!r}")
            if list(theirs_pg.get("seg_end", ())) != list(self._table.ends) or len(theirs_pg.get("seg_wd", ())) != self._table.n_seg:
                raise ValueError(f"load_checkpoint_state: param_groups.seg_end differs: checkpoint {theirs_pg.get('seg_end')!r}, "
                                 f"trainer {self._table.ends!r}")
        # a checkpoint written before the head counts were recorded comes from a trainer whose blocks all had 4 heads
        heads = bts.get("heads", [[n, 4] for n, _ in mine["heads"]])
        if heads != mine["heads"]:
            raise ValueError(f"load_checkpoint_state: heads differ: checkpoint {heads!r}, trainer {mine['heads']!r}")
        theirs = bts.get("shapes", {})
        for k, shp in mine["shapes"].items():
            if theirs.get(k) != shp:
                raise ValueError(f"load_checkpoint_state: shapes differ at {k}: checkpoint {theirs.get(k)}, trainer {shp}")
        if set(theirs) != set(mine["shapes"]):
            raise ValueError(f"load_checkpoint_state: shapes differ: extra keys {sorted(set(theirs) - set(mine['shapes']))}")
        same("bucket_n", "groups")
        steps = {}                                                 # augmenters that share a counter hold one step index
        for a in AUGMENTERS:
            aug, theirs = getattr(self, a.attr, None), bts.get(a.attr)
            if (aug is None) != (theirs is None):
                raise ValueError(f"load_checkpoint_state: {a.attr} differs: the checkpoint was written "
                                 f"{'with' if theirs is not None else 'without'} {a.ckpt_noun}, this trainer has "
                                 f"{'none' if aug is None else 'one'}")
            if aug is None:
                continue
            mine_aug = aug.params()
            if {k: theirs.get(k) for k in mine_aug} != mine_aug:
                raise ValueError(f"load_checkpoint_state: {a.attr} differs: checkpoint {theirs!r}, trainer {mine_aug!r}")
            first = steps.setdefault(a.counter, theirs["step"])
            if int(first) != int(theirs["step"]):
                raise ValueError(f"load_checkpoint_state: {a.attr} differs: the two EEG augmenters share one step index, the "
                                 f"checkpoint holds {first!r} and {theirs['step']!r}")
        msd = sd["model_state_dict"]
        for k, shp in mine["shapes"].items():
            if k not in msd or list(msd[k].shape) != shp:
                raise ValueError(f"load_checkpoint_state: model_state_dict differs at {k}")
        osd = sd["optimizer_state_dict"]
        pmap = self.optimizer_param_map()
        if len(osd["param_groups"]) != 1 or len(osd["param_groups"][0]["params"]) != len(pmap):
            raise ValueError("load_checkpoint_state: optimizer_state_dict has a different parameter group")
        for i, name, p, _ in pmap:
            st = osd["state"].get(i)
            if st is None or tuple(st["exp_avg"].shape) != tuple(p.shape) or tuple(st["exp_avg_sq"].shape) != tuple(p.shape):
                raise ValueError(f"load_checkpoint_state: optimizer state differs at parameter {i} ({name})")
        if tuple(bts["optimizer_words"].shape) != tuple(self.bucket.state.shape):
            raise ValueError("load_checkpoint_state: optimizer_words differ in size")

    @torch.no_grad()
    def _copy_model_state(self, msd: dict):
        """in place: parameters are views of ``bucket.p`` and captured graphs hold the pointers"""
        for k, t in self.state_dict(keep_vars=True).items():
            t.copy_(msd[k])

    @torch.no_grad()
    def load_checkpoint_state(self, sd: dict) -> None:
        """continue bit for bit from `checkpoint_state`: parameters, BatchNorm buffers, Adam moments, optimizer words,
        hyperparameters and the dropout stream, all copied in place.  Any captured step is dropped; the next
        graph-mode `train_step` captures again with the checkpoint's seeds and epoch word.  The process-global dropout
        counter (``ops._seed_state``) is set from the checkpoint.  A checkpoint of another EEG branch, loss, shape, bucket
        layout, world size, cross-batch memory (presence, size, warm-up), averaged weights (presence, decay, warm-up),
        ``no_decay`` or ``freeze`` raises ValueError before anything is touched; the learning-rate multipliers are restored.  The average (``ema.shadow``) is copied into ``bucket.ema`` in place."""
        if getattr(self, "_ema_active", False):
            raise RuntimeError("load_checkpoint_state inside ema_weights(): leave the context first")
        self._check_compatible(sd)
        bts = sd["bridge_trainer_state"]
        b = self.bucket
        self._drop_capture()
        self._copy_model_state(sd["model_state_dict"])
        st = sd["optimizer_state_dict"]["state"]
        for i, _, _, sl in self.optimizer_param_map():
            b.m[sl].copy_(st[i]["exp_avg"].reshape(-1))
            b.v[sl].copy_(st[i]["exp_avg_sq"].reshape(-1))
        b.state.copy_(bts["optimizer_words"])
        b.g.zero_()
        h = bts["hyper"]
        self.betas, self.eps = (h["betas"][0], h["betas"][1]), h["eps"]
        self.weight_decay, self.grad_clip = h["weight_decay"], h["grad_clip"]
        self.lr = float(bts["lr"])
        if getattr(self, "_table", None) is not None:              # the multipliers and decays, restored like the lr word
            pg = bts.get("param_groups")
            mult = dict(zip(pg["components"], pg["multipliers"])) if pg else {c: 1.0 for c in self.COMPONENTS}
            self._lr_scale.update({c: float(v) for c, v in mult.items()})
            self._table.write(mults=[self._lr_scale[c] for c in self._seg_component],
                              wds=pg["seg_wd"] if pg else self._table_lists()[2])
            self._grouped = self._grouped or not self._table.uniform   # (the capture was dropped above)
        d = bts["dropout"]
        ops._seed_state["base"] = int(d["base"])
        ops._seed_state["step"] = int(d["step"])
        self._pending_epoch_word = d["epoch_word"] if d["kind"] == "graph" else None
        for a in AUGMENTERS:
            if a.attr in bts:
                setattr(self, a.counter, int(bts[a.attr]["step"]))
        if "bank" in bts:
            self._load_bank(bts["bank"])
        if "ema" in bts:
            b.ema.copy_(bts["ema"]["shadow"])
        ops.weights_changed()

    def _load_bank(self, ck: dict):
        """the ring's words, rows and ids, in place when the storage exists (allocated here otherwise)"""
        self._bank_grouped = ck["grouped"]
        self._bank_pushes = int(ck["state"][2])
        if ck["rows"] is None:                                     # written before the first training step: an empty bank
            if self._bank is not None:
                self._bank.reset()
            return
        if self._bank is None:
            self._bank = ops.ClipBank(self._bank_size, self.head.bridge.bridge_dim, True, self._scal.device)
        bank = self._bank
        bank.grouped = bool(ck["grouped"])
        bank.bank.copy_(ck["rows"])
        bank.gid.copy_(ck["ids"])
        bank.state.copy_(torch.tensor(ck["state"], dtype=torch.int32))

    # ------------------------------------------------------------------ files
    def _barrier(self):
        if dp.world_size(self.group) > 1:
            import torch.distributed as dist
            dist.barrier(group=dp._control_group(self.group))

    def save_checkpoint(self, path: str, epoch: int, metrics: Optional[dict] = None, scheduler=None) -> None:
        """write `checkpoint_state` to ``path`` atomically (a temporary file in the same directory, then
        ``os.replace``).  Under data parallelism this is collective: rank 0 writes (parameters and moments are the
        same on every rank; the BatchNorm running statistics saved are rank 0's), then all ranks meet at a barrier."""
        if dp.rank(self.group) == 0:
            ck = self.checkpoint_state(epoch, metrics, scheduler)
            d = os.path.dirname(os.path.abspath(path))
            fd, tmp = tempfile.mkstemp(prefix="." + os.path.basename(path) + ".", suffix=".tmp", dir=d)
            try:
                with os.fdopen(fd, "wb") as f:
                    torch.save(ck, f)
                    f.flush()
                    os.fsync(f.fileno())
                os.replace(tmp, path)
            except BaseException:
                if os.path.exists(tmp):
                    os.unlink(tmp)
                raise
        self._barrier()

    def load_checkpoint(self, path: str, scheduler=None):
        """-> (epoch, metrics).  A `save_checkpoint` file restores everything (`load_checkpoint_state`); a
        reference-style container without ``bridge_trainer_state`` or a bare state dict restores the model only.
        ``scheduler``: receives ``scheduler_state_dict`` when the file has one.  A model-only file carries no average:
        a trainer that keeps one starts it anew from the loaded weights (`sync_ema`)."""
        ck = torch.load(path, map_location="cpu", weights_only=True)
        averaging = getattr(self.bucket, "ema", None) is not None
        if "model_state_dict" not in ck:                       # a bare state dict (_test_bridge.py:499-504)
            self.load_state_dict(ck)
            if averaging:
                self.sync_ema()
            ops.weights_changed()
            return None, None
        if "bridge_trainer_state" in ck:
            self.load_checkpoint_state(ck)
        else:
            self.load_state_dict(ck["model_state_dict"])
            if averaging:
                self.sync_ema()
            ops.weights_changed()
        if scheduler is not None and ck.get("scheduler_state_dict") is not None:
            scheduler.load_state_dict(ck["scheduler_state_dict"])
        return ck.get("epoch"), ck.get("metrics")

    # ------------------------------------------------------------------ epoch loop
    def _best_copy(self):
        """(live parameters, buffers, averaged parameters or None): the average travels with the weights it belongs to"""
        ema = getattr(self.bucket, "ema", None)
        return self.bucket.p.clone(), [t.clone() for t in self.buffers()], None if ema is None else ema.clone()

    def _best_copy_from(self, ck: dict):
        """`_best_copy` from a ``best.pt`` container"""
        msd = ck["model_state_dict"]
        names = {id(p): n for n, p in self.named_parameters()}
        dev = self.bucket.p.device
        p = torch.cat([msd[names[id(q)]].reshape(-1) for q in self.bucket.params]).to(dev)
        ema = ck.get("bridge_trainer_state", {}).get("ema")
        return p, [msd[n].to(dev) for n, _ in self.named_buffers()], None if ema is None else ema["shadow"].to(dev)

    @torch.no_grad()
    def _restore_best(self, best):
        p, bufs, ema = best
        self.bucket.p.copy_(p)
        for t, s in zip(self.buffers(), bufs):
            t.copy_(s)
        if ema is not None:
            self.bucket.ema.copy_(ema)
        ops.weights_changed()

    def _validate(self, val, monitor, batch_size, use_ema: bool = False, radius: int = 0):
        from .bridge_utils import retrieval_metrics
        s0 = ops._seed_state["step"]
        with (self.ema_weights() if use_ema else contextlib.nullcontext()):
            ze, zf = self.embed(val[0], val[1], batch_size)
            metrics = retrieval_metrics(ze, zf, groups=val[2] if len(val) > 2 else None, radius=radius)
            if len(val) > 3 and val[3] is not None:       # class labels: the reference's evaluate_bridge metrics as well
                metrics["classification"] = self.evaluate_classification(val[0], val[1], val[3], batch_size)
        assert ops._seed_state["step"] == s0, "validation drew dropout seeds"
        return metrics, monitor_value(metrics, monitor)

    def fit(self, train, epochs: int, *, val=None, warmup_epochs: int = 3, min_lr: float = 1e-6,
            monitor: Union[str, Callable[[dict], float]] = "mean_R@1", mode: str = "max", patience: int = 15,
            min_delta: float = 1e-3, eval_every: int = 1, checkpoint_dir: Optional[str] = None, resume: bool = False,
            val_batch_size: int = 256, validate_with: Optional[str] = None, val_radius: int = 0):
        """The reference's epoch loop (run_training_lite.py:465-520) on the contrastive step -> per-epoch history.

        ``train``: an iterable of (eeg, fmri) or (eeg, fmri, groups) batches re-iterated every epoch, or ``epoch ->
        iterable`` (1-based).  Every batch goes through `train_step` (``groups``: subject ids, pairs of one subject are
        positives of each other); in graph mode keep one batch shape and one kind (a new shape, or a switch between
        grouped and ungrouped batches, captures the step again).
        Schedule: `CosineAnnealingWarmup(warmup_epochs, epochs, min_lr)` from the trainer's current lr, stepped after each
        epoch's training as the reference does (epoch 1 runs at the base rate, epoch e > 1 at ``_lr_at(e - 1)``).
        A classify trainer takes (eeg, fmri, groups_or_None, labels) batches; ``val = (eeg, fmri, groups_or_None, labels)``
        adds ``metrics["classification"]`` (`evaluate_classification`), e.g. ``monitor="classification.Accuracy"``.
        ``val = (eeg, fmri[, groups])``: every ``eval_every`` epochs (and after the last) `embed` + `retrieval_metrics`
        (grouped ranks with ``groups``; ``val_radius`` = R > 0: ``groups`` are timeline ids and a pair within R of the
        query's id is ignored by the validation ranks, `retrieval_metrics(radius=R)` - what a trainer built with
        ``neighbour_radius=R`` should be selected on; it is an argument like the others, not part of a checkpoint, so
        ``resume=True`` needs the same value again); the
        monitored value (``monitor_value``; ``mode`` "max" or "min") drives `EarlyStopping(patience, min_delta)` and the
        best state: on a strict improvement a device copy of the parameters and buffers is kept (and ``best.pt`` written
        when ``checkpoint_dir`` is set); the best model is restored in place at the end (the optimizer state is not,
        as in the reference).  ``last.pt`` is written after every epoch; ``resume=True`` continues from it at the
        epoch boundary (the same ``train``, ``val`` and arguments must be given).
        ``validate_with``: "ema" - validation, early stopping and the best-epoch decision use the averaged weights
        (`ema_weights()`; the default on a trainer built with ``ema_decay > 0``, ValueError on one without) - or "live"
        (the default otherwise).  The best state kept, written and restored is the live weights AND their average;
        ``model_state_dict`` of ``best.pt`` / ``last.pt`` is always the live weights (`ema_state_dict()` exports the average).
        Data parallel: rank 0 validates and broadcasts the metrics, the monitored value and its decisions; every rank
        acts on them.  Pass the same ``val`` on every rank (only rank 0 reads it)."""
        from .crossmodal_v4_enhancements import CosineAnnealingWarmup, EarlyStopping
        if epochs < 1 or warmup_epochs < 0 or warmup_epochs >= epochs:
            raise ValueError(f"fit: need 0 <= warmup_epochs < epochs (got {warmup_epochs}, {epochs})")
        if eval_every < 1:
            raise ValueError("fit: eval_every must be >= 1")
        if mode not in ("max", "min"):
            raise ValueError("fit: mode is 'max' or 'min'")
        if resume and checkpoint_dir is None:
            raise ValueError("fit: resume=True needs checkpoint_dir")
        averaging = getattr(self.bucket, "ema", None) is not None
        if validate_with is None:
            validate_with = "ema" if averaging else "live"
        if validate_with not in ("ema", "live"):
            raise ValueError(f"fit: validate_with is 'ema' or 'live' (got {validate_with!r})")
        if validate_with == "ema" and not averaging:
            raise ValueError("fit: validate_with='ema' needs a trainer built with ema_decay > 0")
        use_ema = validate_with == "ema"
        val_radius = int(val_radius)
        if val_radius < 0:
            raise ValueError(f"fit: val_radius must be >= 0 (got {val_radius})")
        if val_radius > 0 and (val is None or len(val) < 3 or val[2] is None):
            raise ValueError(f"fit: val_radius={val_radius} needs val = (eeg, fmri, groups) with timeline ids")
        if checkpoint_dir is not None and dp.rank(self.group) == 0:
            os.makedirs(checkpoint_dir, exist_ok=True)
        last = os.path.join(checkpoint_dir, "last.pt") if checkpoint_dir else None
        best_path = os.path.join(checkpoint_dir, "best.pt") if checkpoint_dir else None
        sched = CosineAnnealingWarmup(_LROptimizer(self), warmup_epochs, epochs, min_lr)
        stopper = EarlyStopping(patience, min_delta, mode)
        history, best_score, best_epoch, best, start, stopped = [], None, None, None, 1, False
        if resume and os.path.exists(last):
            ck = torch.load(last, map_location="cpu", weights_only=True)
            fs = ck.get("bridge_trainer_state", {}).get("fit")
            if fs is None:
                raise ValueError(f"fit: {last} was not written by fit")
            self.load_checkpoint_state(ck)
            ss = ck["scheduler_state_dict"]
            sched.current_epoch, sched.base_lr = ss["current_epoch"], ss["base_lr"]
            stopper.counter, stopper.best_score, stopper.should_stop = fs["stopper"]
            history, best_score, best_epoch, stopped = list(fs["history"]), fs["best_score"], fs["best_epoch"], fs["stopped"]
            start = ck["epoch"] + 1
            if best_epoch is not None:
                best = self._best_copy_from(torch.load(best_path, map_location="cpu", weights_only=True))
        dev = self.bucket.p.device
        try:
            for epoch in range(start, epochs + 1):
                if stopped:
                    break
                lr = float(self.lr)
                total = torch.zeros((), dtype=torch.float64, device=dev)
                n = 0
                for batch in (train(epoch) if callable(train) else train):
                    total += self.train_step(*batch)["loss"]
                    n += 1
                sched.step()
                entry = {"epoch": epoch, "lr": lr, "steps": n, "train_loss": total.item() / max(n, 1),
                         "val": None, "monitor": None, "improved": False, "stop": False}
                if val is not None and (epoch % eval_every == 0 or epoch == epochs):
                    entry.update(self._decide(val, monitor, mode, val_batch_size, stopper, best_score, use_ema, val_radius))
                    if entry["improved"]:
                        best_score, best_epoch = entry["monitor"], epoch
                        best = self._best_copy()
                    stopped = entry["stop"]
                history.append(entry)
                self._fit_state = {"history": history, "best_score": best_score, "best_epoch": best_epoch,
                                   "stopped": stopped, "epochs": epochs,
                                   "stopper": [stopper.counter, stopper.best_score, stopper.should_stop]}
                if checkpoint_dir is not None:
                    if entry["improved"]:
                        self.save_checkpoint(best_path, epoch, entry["val"], sched)
                    self.save_checkpoint(last, epoch, entry["val"], sched)
        finally:
            self._fit_state = None
        if best is not None:
            self._restore_best(best)
        return history

    def _decide(self, val, monitor, mode, batch_size, stopper, best_score, use_ema: bool = False, radius: int = 0) -> dict:
        """rank 0 validates (``use_ema``: with the averaged weights); every rank takes rank 0's metrics, monitored value,
        improvement and stop"""
        metrics = score = None
        if dp.rank(self.group) == 0:
            metrics, score = self._validate(val, monitor, batch_size, use_ema, radius)
        if dp.world_size(self.group) > 1:
            import torch.distributed as dist
            ctrl = dp._control_group(self.group)
            box = [metrics, score]
            dist.broadcast_object_list(box, src=dist.get_global_rank(ctrl, 0), group=ctrl)
            metrics, score = box
        improved = not math.isnan(score) and (best_score is None or (score > best_score if mode == "max" else score < best_score))
        stop = bool(stopper(score))
        if dp.world_size(self.group) > 1:
            import torch.distributed as dist
            ctrl = dp._control_group(self.group)
            flags = torch.tensor([int(improved), int(stop)], dtype=torch.int64)
            dist.broadcast(flags, src=dist.get_global_rank(ctrl, 0), group=ctrl)
            improved, stop = bool(flags[0]), bool(flags[1])
            stopper.should_stop = stop
        return {"val": metrics, "monitor": score, "improved": improved, "stop": stop}
