"""Data-parallel contrastive EEG<->fMRI bridge trainer (north-star hot path).

One process per GPU (``torch.distributed`` backend ``nccl`` == RCCL over xGMI).
Per step and per rank: EEG temporal encoder + fMRI voxel encoder forward on the
local (EEG-epoch, fMRI-volume) pairs, projection heads, one all-gather of the
packed L2-normalised embeddings (global contrastive negatives), fused
similarity/InfoNCE forward+backward on this rank's rows of the gathered batch
(every rank evaluates all rows, so no reduce-scatter of column gradients is
issued), encoder backward, the all-reduce of the flat fp32 gradient bucket in
one piece per FINISHED LAYER GROUP (``groups``: the fMRI encoder as soon as its
shorter backward is done; transformer stack + heads, then conv blocks 3-2, as
soon as their handed-over weight-gradient sums have been flushed on the side
stream; only conv block 1 - 0.1 MB - after the chain), each an asynchronous
collective the optimizer alone waits for, and the fused clip+AdamW on the flat
parameter bucket.  At world size > 1 the whole step, collectives included, is
ONE hipGraph when the backend's collectives can be captured (RCCL) - all ranks
agree on that outcome before any replay (``dp.agree_on_capture``) - else three
graph segments around two eager collectives (``capture_mode`` says which).
BatchNorm statistics stay per-rank (the reference has no SyncBN; SURVEY.md
section 8e).

The reference has no such trainer (its loops are run_training_lite.py:474-489
and _test_bridge.py:775-788: zero_grad / forward / backward / clip 1.0 / AdamW);
this keeps that step structure.
"""
from __future__ import annotations

import contextlib
import os
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import _hip, dp, ops, optim
from .autograd import GradBag, bridge_cls_bwd, contrastive_embed_bwd, contrastive_embed_bwd_da, deferred, ffn_rows_bwd_fused
from .bridge_branches import input_layout, select_eeg, select_fmri, step_schedule
from .bridge_checkpoint import TrainerCheckpointMixin
from .bridge_staging import TrainerStagingMixin
from .bridge_utils import EEGfMRIContrastiveBridge, retrieval_metrics
from .enhanced_models_v4 import EnhancedERPEncoder
from .fmri_utils import fMRIVolumeEncoder3D
from .optim import FlatBucket, check_ema_decay


class BridgeTrainer(TrainerCheckpointMixin, TrainerStagingMixin, nn.Module):
    def __init__(self, eeg_channels: int = 64, hidden_dim: int = 128, fmri_dim: int = 64,
                 bridge_dim: int = 128, dropout: float = 0.3, lr: float = 1e-4,
                 weight_decay: float = 1e-4, grad_clip: float = 1.0, betas=(0.9, 0.999),
                 eps: float = 1e-8, group=None, device="cuda", mode: str = "graph", eeg_encoder: Optional[nn.Module] = None,
                 num_heads: int = 4, num_layers: int = 2, augment=None, loss: str = "infonce",
                 classify: bool = False, ce_weight: float = 1.0, class_weight=None, num_classes: int = 2,
                 fmri_encoder: Optional[nn.Module] = None, bank_size: int = 0, bank_warmup: int = 0, fmri_augment=None,
                 ema_decay: float = 0.0, ema_warmup: bool = True, lr_scale=None, no_decay: bool = False, freeze=(),
                 eeg_time_augment=None, key_encoder: bool = False, neighbour_radius: int = 0):
        """``eeg_encoder``: the EEG branch when it is not the default ``EnhancedERPEncoder(eeg_channels, hidden_dim,
        num_layers, num_heads, dropout)`` - an ``EnhancedPowerEncoder`` (enhanced_models_v4.py:196-285) or a
        ``MultiScaleSTFTPowerEncoder`` (BASELINE config #5: raw EEG -> multi-scale STFT power -> a4); it must end in
        ``hidden_dim`` features.  The attention kernels run head dims ``hidden_dim / num_heads`` of 16, 24, ..., 64
        (checked at the first step, not here: a trainer built on the CPU to read weights takes any shape).
        ``augment``: an ``EEGTransforms`` (crossmodal_eeg_scr.py) - every `train_step` then augments its EEG batch on the
        device (noise + channel drop, csrc/augment.hip), drawing step index 0, 1, 2, ... from the trainer's own counter and
        this process's rank; `evaluate`, `embed`, `evaluate_retrieval`, `explain`, `perturb` and `forward` never augment.
        ``loss``: "infonce" (default: the symmetric InfoNCE, mm_clip_loss_own_rows*) or "sigmoid" (the pairwise sigmoid
        loss, mm_sigmoid_loss_own_rows: no softmax normaliser, so its signal does not depend on the number of in-batch
        negatives; one more trained scalar, ``head.logit_bias``).
        ``classify``: also train the bridge's classification branch (cross attention, fusion, classifier) on class labels
        with ``ce_weight`` x the (``class_weight``-ed, (num_classes,) floats) cross-entropy: `train_step(..., labels=)`,
        three more launches per step (mm_bridge_cls_fwd, mm_bridge_cls_bwd).  ``num_classes`` sizes
        the bridge's classifier on any trainer (`predict`).
        ``fmri_encoder``: None (default) = the voxel encoder ``fMRIVolumeEncoder3D(1, fmri_dim)`` on (B, 1, D, H, W)
        volumes; an ``fMRITabularEncoder`` = the reference's own fMRI input, ROI activation statistics and flattened
        connectivity as one (B, activation_dim + connectivity_dim) tensor ``[activation | connectivity]`` - the branch is
        then two launches per step (mm_fmri_tab_fwd, mm_fmri_tab_bwd), train-mode batches of
        2..256 rows; its ``hidden_dim`` must equal ``fmri_dim``.  Everything else - losses, groups, classify, augment,
        embed / evaluate / retrieval / predict / explain, checkpoints, `fit`, the packed host-fed path - is the same.
        An ``fMRISequenceEncoder3D(frames=F, out_dim=fmri_dim)`` = F fMRI frames per EEG epoch, (B, F, D, H, W): every
        frame through one shared voxel encoder (the B * F volumes are one batch, BatchNorm statistics over all of them),
        then a learned attention pool over the frames (mm_lagpool_fwd, mm_lagpool_bwd) - the voxel
        branch's launches plus one each way; `explain` adds ``fmri_frames`` and ``lag_weights``, `perturb` knocks out
        frames (``("rows", 1)``, default) or blocks of all frames; no ``fmri_augment``.
        ``bank_size`` = K > 0: a cross-batch memory of the last K pairs' embeddings (Wang et al., "Cross-Batch Memory for
        Embedding Learning") - every `train_step` scores its rows against the batch AND the valid
        bank rows (mm_clip_bank_loss in place of mm_clip_loss_own_rows*: more negatives, and with ``groups=`` more
        positives, at no encoder pass), then pushes its own embeddings (mm_clip_bank_push).  Bank rows are constants: no
        loss, no gradient.  ``bank_warmup`` = w: the first w steps fill the bank without using it - they launch the in-batch
        loss (and the push), so they are a default trainer's steps to the bit; in graph mode the step is captured once more
        when the warm-up ends.  The storage is
        allocated at the first step, before any capture; the number of valid rows lives on the device, so a captured step
        is never captured again for it.  Whether the bank carries group ids is fixed by the first training step (a later
        switch between ``groups=None`` and ``groups=...`` raises ValueError; `reset_bank` lifts that).  InfoNCE only, one
        process only.  `evaluate`, `embed`, `evaluate_retrieval`, `predict`, `explain`, `perturb` and `forward` never read or write
        the bank: they keep the in-batch loss.  0 (default): no bank, the step is unchanged.
        ``fmri_augment``: a ``VolumeTransforms`` (fmri_utils.py; voxel encoder only) - every `train_step` then augments its
        fMRI batch on the device (flip, shift, scale, noise, erase; csrc/volume_augment.hip), drawing
        step index 0, 1, 2, ... from a counter of its own (`fmri_augment_step`) and this process's rank; in graph mode the
        two launches write the captured step's static fMRI buffer.  The entry points that never augment the EEG never
        augment the volumes either.  None (default): the step issues the launches it always did.
        ``ema_decay`` = d in (0, 1): an exponential moving average of every trained parameter (``bucket.ema``, one more
        flat fp32 buffer), kept by the update kernel itself - the step launches mm_adamw_clip_ema in place of
        mm_adamw_clip: no new launch, no graph node, no collective (every rank computes the same bits), in all three
        modes.  After step t the decay is ``min(d, (1 + t) / (10 + t))`` with ``ema_warmup`` (default), d without
        (DESIGN.md section 5s).  `ema_weights()` evaluates with the average, `fit` validates with it, checkpoints carry it,
        `ema_state_dict()` exports it.  Only parameters are averaged: BatchNorm running statistics and the other buffers
        are running averages already, so the averaged weights run with the LIVE buffers.  0 (default): no average; the
        trainer takes exactly the code path, launches and checkpoint container it has without the keyword.
        Parameter groups - the reference's transfer recipe, pretrained encoders frozen and then
        fine-tuned below the heads' rate.  The components are ``"eeg_encoder"``, ``"fmri_encoder"`` and ``"head"`` (the
        bridge's trained parameters, ``logit_scale`` and ``logit_bias``); an unknown name raises ValueError.
        ``lr_scale`` = ``{"eeg_encoder": 0.1, ...}``: a multiplier of the learning rate per component (finite, >= 0;
        missing components: 1).  `set_lr` / `fit`'s schedule move the base rate only, the ratios stay; `set_lr_scale`
        rewrites a multiplier between steps (device memory the captured step reads: no new capture), `lr_scales` reads
        them.  0 holds a component still while its Adam moments and BatchNorm statistics keep moving (torch's
        ``lr=0`` group) - the held-then-released stage.
        ``no_decay=True``: every trained parameter with ``ndim <= 1`` - biases, LayerNorm / BatchNorm gains and biases,
        ``logit_scale``, ``logit_bias``, fusion logits and temperatures - gets weight decay 0.
        Both go into the update kernel as a segment table over the flat bucket (mm_adamw_clip_groups[_ema] in place of
        mm_adamw_clip[_ema]: no new launch; the clipped norm stays the whole bucket's); the table is the same on every
        rank, so both work at any world size.  A table of multiplier 1 and one decay launches the plain kernel.
        ``freeze`` = ``("fmri_encoder",)`` and / or ``"eeg_encoder"``: the reference's ``requires_grad_(False)`` +
        ``eval()`` of a pretrained encoder.  The component's parameters leave the bucket, its forward runs in eval form
        inside the step (frozen BatchNorm, no dropout seed drawn, nothing updated), and its backward is not issued in
        any mode.  Fixed at construction; ``"head"`` cannot be frozen (ValueError); one process only
        (NotImplementedError at world size > 1).
        ``eeg_time_augment``: an ``EEGTimeTransforms`` (crossmodal_eeg_scr.py) - every `train_step` then shifts, scales,
        inverts and masks its EEG batch along the time axis on the device (mm_stage_inputs_taug).
        Alone it replaces the step's one staging launch by one launch; together with ``augment=`` the two share the
        staging launch (after the plan launch) and therefore the step index (`augment_step`).  The entry points that never
        augment never shift either.  None (default): the step issues the launches it always did.
        ``key_encoder=True``: a momentum key encoder for the bank (He et al., "Momentum Contrast").
        Needs ``bank_size > 0``, ``ema_decay > 0``, ``loss="infonce"`` and one process (ValueError otherwise).  Every
        `train_step` then embeds its (staged, augmented) batch a second time with the AVERAGED weights - unregistered twins
        of the trained encoders and of the two projection heads whose parameters are views into ``bucket.ema`` and whose
        buffers are the online modules' own, run in the eval form (nothing saved, no seed drawn, no running statistic
        written; a frozen encoder has no twin: its online features are the key features).  These rows are the keys of the
        batch and what the bank receives (mm_clip_key_loss in place of mm_clip_bank_loss, then mm_clip_bank_push of the
        keys); gradients flow through the online rows - the queries - only.  Each encoder's key pass is issued in front
        of its online pass on that branch's stream: it reads the BatchNorm running statistics as they stood before this
        step's update, and step t's keys come from the average after step t - 1.  During ``bank_warmup`` the same kernel
        runs with no valid bank row (decided on the device): the step is captured once.  False (default): unchanged.
        ``neighbour_radius`` = R > 0: the ``groups=`` ids are positions on a timeline (`bridge_utils.timeline_ids`) and a
        pair whose id is within R of the query's, and not equal to it, is IGNORED by the contrastive loss - out of the
        softmax normaliser, out of the positive set, exactly zero gradient (mm_clip_loss_own_rows_masked /
        mm_sigmoid_loss_own_rows_masked in place of the grouped launch): consecutive epochs of a
        recording, which share most of their input, stop being pushed apart.  `train_step`, `forward` and `evaluate`
        then need ``groups=`` (ValueError otherwise); no bank and no key encoder (ValueError: their kernels have no
        ignore relation).  `evaluate_retrieval` by default still ranks neighbours; with ``radius=`` it does not (pass
        ``radius=trainer.neighbour_radius``; `fit(val_radius=)` for validation).  0 (default): unchanged."""
        super().__init__()
        self.neighbour_radius = int(neighbour_radius)
        if self.neighbour_radius < 0:
            raise ValueError(f"BridgeTrainer: neighbour_radius must be >= 0 (got {neighbour_radius})")
        if self.neighbour_radius and (bank_size > 0 or key_encoder):
            raise ValueError(f"BridgeTrainer: neighbour_radius={self.neighbour_radius} cannot be combined with bank_size > 0 or "
                             "key_encoder=True: the bank kernels (mm_clip_bank_loss, mm_clip_key_loss) have no ignore "
                             "relation yet, so a neighbour in the bank would still be a negative")
        self._frozen = self._check_freeze(freeze, group)
        self._lr_scale = self._check_lr_scale(lr_scale)
        self.no_decay = bool(no_decay)
        check_ema_decay(ema_decay, "BridgeTrainer")
        self.ema_decay, self.ema_warmup = float(ema_decay), bool(ema_warmup)
        self._ema_active = False                      # inside `ema_weights()`: the parameters hold the averaged weights
        if key_encoder:                               # each missing partner by name, before any allocation
            if not bank_size > 0:
                raise ValueError("BridgeTrainer: key_encoder=True needs bank_size > 0 (the key encoder fills the cross-batch "
                                 "bank; without one there is nothing for its rows to be keys of)")
            if not ema_decay > 0:
                raise ValueError("BridgeTrainer: key_encoder=True needs ema_decay > 0 (the key encoder runs on the averaged "
                                 "weights, bucket.ema)")
            if loss != "infonce":
                raise ValueError(f"BridgeTrainer: key_encoder=True needs loss='infonce' (got {loss!r}: the pairwise sigmoid "
                                 "loss has no bank for a key encoder to fill)")
            if group is not None and dp.world_size(group) > 1:
                raise ValueError("BridgeTrainer: key_encoder=True needs a world size of 1 (the bank it fills is one "
                                 f"process's; got a process group of {dp.world_size(group)})")
        if bank_size < 0 or bank_warmup < 0:
            raise ValueError(f"BridgeTrainer: bank_size and bank_warmup must be >= 0 (got {bank_size}, {bank_warmup})")
        if bank_size > 0:
            if loss == "sigmoid":
                raise ValueError("BridgeTrainer: bank_size > 0 needs loss='infonce' (the pairwise sigmoid loss is the other "
                                 "remedy for few in-batch negatives, not a partner of the bank)")
            if group is not None and dp.world_size(group) > 1:
                raise NotImplementedError("BridgeTrainer: bank_size > 0 with a process group of world size > 1 is not "
                                          "supported yet (intended: every rank pushes the gathered rows of all ranks)")
            ops.clip_bank_check(1, bank_size, bridge_dim, bank_warmup, "BridgeTrainer(bank_size=)")
        self._key_encoder = bool(key_encoder)
        self._key = None                              # the key encoder's unregistered twins (`_build_key_modules`)
        self._key_rows = None                         # the running step's key embeddings (B, 2N): `_seg_forward` -> `_seg_loss`
        self._bank_size, self._bank_warmup = int(bank_size), int(bank_warmup)
        self._bank = None                             # ops.ClipBank, allocated at the first training step (before any capture)
        self._bank_grouped = None                     # fixed by the first training step: do the bank rows carry group ids
        self._bank_pushes = 0                         # host mirror of the bank's `pushes` word (one push per training step)
        # the running step launches a loss that reads the bank: pushes >= warmup - a key trainer always (mm_clip_key_loss
        # gates on the device alone; there are no in-batch bits to keep, the keys are not the queries)
        self._bank_live = bank_warmup == 0 or self._key_encoder
        self._fmri = select_fmri(fmri_encoder, fmri_dim)      # the fMRI branch's entry of `bridge_branches.FMRI_BRANCHES`
        self._fmri_kind = self._fmri.kind
        self.classify, self.ce_weight, self.num_classes = bool(classify), float(ce_weight), int(num_classes)
        cw = None
        if class_weight is not None:
            if not classify:
                raise ValueError("BridgeTrainer: class_weight needs classify=True")
            cw = torch.as_tensor(class_weight, dtype=torch.float32).reshape(-1)
            if cw.numel() != self.num_classes or bool((cw < 0).any()):
                raise ValueError(f"BridgeTrainer: class_weight must be {self.num_classes} non-negative floats (got {cw.tolist()})")
        if classify:
            if self.ce_weight < 0:
                raise ValueError(f"BridgeTrainer: ce_weight must be >= 0 (got {ce_weight})")
            if group is not None and dp.world_size(group) > 1:
                raise NotImplementedError("BridgeTrainer: classify=True with a process group of world size > 1 is not "
                                          "supported yet (intended: the mean over ranks of each rank's weighted mean)")
            ops.bridge_cls_check(bridge_dim, 4, self.num_classes, "BridgeTrainer(classify=True)")   # (the bridge has 4 heads)
        if augment is not None:
            from .crossmodal_eeg_scr import EEGTransforms
            if not isinstance(augment, EEGTransforms):
                raise TypeError(f"BridgeTrainer: augment must be an EEGTransforms (got {type(augment).__name__})")
        self.augment = augment
        if eeg_time_augment is not None:
            from .crossmodal_eeg_scr import EEGTimeTransforms
            if not isinstance(eeg_time_augment, EEGTimeTransforms):
                raise TypeError(f"BridgeTrainer: eeg_time_augment must be an EEGTimeTransforms (got {type(eeg_time_augment).__name__})")
        self.eeg_time_augment = eeg_time_augment
        self._aug_step = 0                            # step index the next train_step's EEG augmentation draws with (both augmenters)
        if fmri_augment is not None:
            from .fmri_utils import VolumeTransforms
            if not isinstance(fmri_augment, VolumeTransforms):
                raise TypeError(f"BridgeTrainer: fmri_augment must be a VolumeTransforms (got {type(fmri_augment).__name__})")
            if not self._fmri.augmentable:
                raise ValueError(f"BridgeTrainer: fmri_augment augments (B, 1, D, H, W) volumes; {self._fmri.not_augmentable_why}")
        self.fmri_augment = fmri_augment
        self._fmri_aug_step = 0                       # step index the next train_step's volume augmentation draws with
        self.eeg_encoder = (EnhancedERPEncoder(eeg_channels, hidden_dim, num_layers, num_heads, dropout)
                            if eeg_encoder is None else eeg_encoder)
        self._eeg = select_eeg(self.eeg_encoder)              # the EEG branch's entry of `bridge_branches.EEG_BRANCHES`
        self._eeg_kind = self._eeg.kind               # (the checkpoint's "eeg_kind")
        self.fmri_encoder = fMRIVolumeEncoder3D(1, fmri_dim, dropout=dropout) if fmri_encoder is None else fmri_encoder
        self.head = EEGfMRIContrastiveBridge(hidden_dim, fmri_dim, bridge_dim, dropout, loss=loss, num_classes=num_classes)
        self.loss = loss
        self.to(device)
        self._class_weight = None if cw is None else cw.to(device)     # (not a buffer: the state dict keeps its keys)
        self._cls_ticket = None                       # int32 word of mm_bridge_cls_fwd, allocated at the first labelled step
        self.group = group
        self.two_streams = True
        self.mode = mode
        self._cap = None
        self._pending_epoch_word = None               # dropout epoch word for the next capture (load_checkpoint_state)
        self._fit_state = None                        # early-stopping / best-metric state while `fit` runs
        self._weight_list = None                      # recorded by the first manual step
        self._arena_need = None                       # floats of scratch one step uses (None: clear all)
        self.stamps = None                            # int64[16] device buffer when phase stamps are wanted
        self.force_segments = False                   # rehearsal: run the N > 1 segmented step even at world 1
        self._side_stream = None                      # created on first use (the host logic also constructs on CPU)
        self.schedule = None                          # the `StepSchedule` of the last issued (or captured) step: for inspection only
        self._bags = []                               # the last steps' gradient bags (they keep descriptor tables alive)
        self.lr, self.weight_decay, self.grad_clip = lr, weight_decay, grad_clip
        self.betas, self.eps = betas, eps
        br = self.head.bridge
        # only what the step touches is trained: without ``classify`` the classifier / cross-attention half of the
        # bridge stays out of the bucket
        is_proj = lambda name: name.startswith("eeg_proj") or name.startswith("fmri_proj")  # noqa: E731
        for name, p in br.named_parameters():
            if not is_proj(name) and not classify:
                p.requires_grad_(False)
        # bucket order = the order in which gradients are NOT yet final, i.e. the reverse of when each layer group's
        # all-reduce can start (`step_schedule`): conv block 1 (last kernel of the chain) | conv blocks 2-3 (final once
        # the second hand-over has been flushed) | transformer stack + encoder head + projection heads + logit scale
        # (first hand-over) | fMRI encoder (its own, shorter backward).  Each group is one contiguous range of the
        # flat bucket, the fMRI encoder's the tail [fmri_lo, n).
        # (classification branch: the parameters whose size is no multiple of 4 floats go last, so that the matrices
        # before them keep the alignment the projection heads' weights have)
        cls_params = [p for name, p in br.named_parameters() if p.requires_grad and not is_proj(name)]
        cls_params.sort(key=lambda p: p.numel() % 4 != 0)
        head_params = [p for name, p in br.named_parameters() if p.requires_grad and is_proj(name)] + cls_params + [self.head.logit_scale]
        if loss == "sigmoid":
            head_params.append(self.head.logit_bias)
        # a frozen encoder (the reference's requires_grad_(False) + eval()): out of the bucket, eval form for good
        for name in self._frozen:
            getattr(self, name).requires_grad_(False).eval()
        if "eeg_encoder" in self._frozen:             # no EEG backward, no hand-over: the heads' gradients are final on the chain
            layout = [("heads", "main", head_params)]
        else:
            layout = self._eeg.layout(self.eeg_encoder, head_params)
        layout.append(("fmri encoder", "fmri", list(self.fmri_encoder.parameters())))
        self.bucket = FlatBucket([p for _, _, ps in layout for p in ps], ema=self.ema_decay > 0)
        self.groups = []                            # (name, ready point, lo, hi) over the flat bucket, in bucket order
        off = 0
        for name, ready, ps in layout:
            k = sum(p.numel() for p in ps if p.requires_grad)
            self.groups.append((name, ready, off, off + k))
            off += k
        assert off == self.bucket.n
        self.fmri_lo = self.groups[-1][2]
        # parameter groups: which component every bucket parameter belongs to, and the segment table of the update kernel
        # (device arrays, allocated here - before any capture - and rewritten in place by `set_lr_scale`)
        comp = {id(p): "head" for p in head_params}
        comp.update({id(p): "eeg_encoder" for p in self.eeg_encoder.parameters()})
        comp.update({id(p): "fmri_encoder" for p in self.fmri_encoder.parameters()})
        self._param_component = [comp[id(p)] for p in self.bucket.params]
        self._seg_component = self._segment_components()
        self._table = optim.SegmentTable(*self._table_lists(), device=self.bucket.p.device)
        # which update kernel the step launches: the plain one while the table is uniform (multiplier 1, one decay).  Fixed
        # here for the captured step; `set_lr_scale` away from a uniform table switches it once (and drops the capture)
        self._grouped = not self._table.uniform
        self._works = []                              # asynchronous all-reduces of the running step (waited for by the optimizer)
        self.capture_mode = None                      # "one graph" | "one graph + captured RCCL collectives" | "3 segments + 2 eager collectives"
        self.bucket.state[2] = lr
        # {loss, top-1 e->f, top-1 f->e, d loss / d logit_scale} (sigmoid: + d loss / d logit_bias) of the last step:
        # owned by this trainer (plain stores of the loss kernel), so the tensors a step returns are overwritten only
        # by THIS trainer's next step - keep a value with .item() / .clone()
        # classify: + {ce, rows classified right, sum of row weights, ce_weight * ce} (mm_bridge_cls_fwd) and the total
        # loss (mm_bridge_cls_bwd), after the contrastive loss's words
        self._scal_cls = 5 if loss == "sigmoid" else 4
        self._scal = torch.zeros(self._scal_cls + (5 if classify else 0), device=device)
        if self._key_encoder:
            self._build_key_modules()
        ops.weights_changed()

    @property
    def _side(self):
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream()
        return self._side_stream

    @property
    def world(self):
        import torch.distributed as dist
        return dist.get_world_size(self.group) if self.group is not None else 1

    @property
    def bank_size(self) -> int:
        """rows of the cross-batch memory (0: none)"""
        return self._bank_size

    @property
    def bank_filled(self) -> int:
        """valid rows of the bank right now.  Reads a device word: SYNCHRONISES with the stream (not for the step loop)."""
        return 0 if self._bank is None else int(self._bank.state[1].item())

    def reset_bank(self):
        """empty the bank (its state words are zeroed on the device; the rows stay and are never read) and let the next
        training step choose anew whether the bank carries group ids"""
        if self._bank is not None:
            self._bank.reset()
        self._bank_grouped = None
        self._bank_pushes = 0

    def _bank_prepare(self, B: int, grouped: bool, who: str):
        """a bank trainer's checks and allocations of a training step, before its first launch (or its capture)"""
        ops.clip_bank_check(B, self._bank_size, self.head.bridge.bridge_dim, self._bank_warmup, f"{who} (bank_size={self._bank_size})")
        if self._bank_grouped is not None and self._bank_grouped != grouped:
            raise ValueError(f"{who}: the bank was filled {'with' if self._bank_grouped else 'without'} group ids and this step "
                             f"comes {'with' if grouped else 'without'} them: the ids of the bank's rows would be undefined "
                             "(reset_bank() empties the bank and lifts this)")
        if self._bank is None:
            self._bank = ops.ClipBank(self._bank_size, self.head.bridge.bridge_dim, True, self._scal.device)
        self._bank_grouped = self._bank.grouped = grouped
        # the device gates on `pushes >= warmup` as well; the host decides which loss the step launches: before that the
        # in-batch kernels, whose bits a default trainer has (mm_clip_bank_loss at n = 0 agrees with them to rounding only,
        # and rounding does not stay small behind AdamW's g / (|g| + eps))
        self._bank_live = self._key_encoder or self._bank_pushes >= self._bank_warmup
        self._bank_pushes += 1

    # ------------------------------------------------------------------ momentum key encoder
    def _build_key_modules(self):
        """structural twins of the trained encoders and of the two projection heads: every parameter a view into
        ``bucket.ema`` at the online parameter's offset (a parameter outside the bucket: the online storage itself), every
        buffer the online module's own tensor (BatchNorm running statistics, positional tables: read-only in the eval
        form).  Kept in a plain dict - NOT registered: absent from parameters(), state_dict(), the bucket, the gradient
        groups and checkpoints.  A frozen encoder has no twin."""
        import copy
        import types
        b = self.bucket
        where, off = {}, 0
        for p in b.params:
            where[id(p)] = off
            off += p.numel()

        def twin(online: nn.Module) -> nn.Module:
            t = copy.deepcopy(online).eval()
            for mo, mt in zip(online.modules(), t.modules()):
                for name, p in mo._parameters.items():
                    if p is None:
                        continue
                    tp = mt._parameters[name]
                    tp.requires_grad_(False)
                    o = where.get(id(p))
                    tp.data = p.data if o is None else b.ema[o:o + p.numel()].view(p.shape)
                for name, buf in mo._buffers.items():
                    mt._buffers[name] = buf
            return t
        br = self.head.bridge
        key = {name: twin(getattr(self, name)) for name in ("eeg_encoder", "fmri_encoder") if name not in self._frozen}
        key["bridge"] = types.SimpleNamespace(eeg_proj=twin(br.eeg_proj), fmri_proj=twin(br.fmri_proj),
                                              bridge_dim=br.bridge_dim, drop_p=br.drop_p)
        self._key = key

    def _key_embed(self, kfe, kff):
        """the twin heads on the two encoders' key features -> the key rows (B, 2N) = [ke | kf]; eval form"""
        return ops.contrastive_embed_impl(self._key["bridge"], kfe, kff, False)[0]

    @property
    def augment_step(self) -> int:
        """the step index the next `train_step` augments with (0 after construction; restored by a checkpoint)"""
        return self._aug_step

    @property
    def fmri_augment_step(self) -> int:
        """the step index the next `train_step` augments its fMRI batch with (0 after construction; restored by a checkpoint)"""
        return self._fmri_aug_step

    def set_lr(self, lr: float):
        self.lr = lr
        self.bucket.state[2] = lr

    # ------------------------------------------------------------------ parameter groups
    COMPONENTS = ("eeg_encoder", "fmri_encoder", "head")

    @classmethod
    def _check_component(cls, name, who: str) -> str:
        if name not in cls.COMPONENTS:
            raise ValueError(f"BridgeTrainer: {who} names the component {name!r}; the components are {cls.COMPONENTS}")
        return name

    @classmethod
    def _check_freeze(cls, freeze, group) -> tuple:
        names = (freeze,) if isinstance(freeze, str) else tuple(freeze)
        for name in names:
            if cls._check_component(name, "freeze") == "head":
                raise ValueError("BridgeTrainer: freeze=('head',) would leave nothing the contrastive loss trains; freeze the "
                                 "encoders, hold the head with lr_scale={'head': 0.0}")
        if names and group is not None and dp.world_size(group) > 1:
            raise NotImplementedError("BridgeTrainer: freeze= with a process group of world size > 1 is not supported yet "
                                      "(intended: the gradient groups of the remaining parameters, reduced as now)")
        return tuple(n for n in cls.COMPONENTS if n in names)

    @classmethod
    def _check_lr_scale(cls, lr_scale) -> dict:
        scales = {name: 1.0 for name in cls.COMPONENTS}
        for name, value in (lr_scale or {}).items():
            scales[cls._check_component(name, "lr_scale")] = optim.check_lr_scale(value, f"BridgeTrainer(lr_scale[{name!r}])")
        return scales

    def _table_entries(self):
        """(numel, multiplier, weight decay, component) of every bucket parameter, in bucket order"""
        wd = float(self.weight_decay)
        return [(p.numel(), self._lr_scale[c], 0.0 if self.no_decay and p.ndim <= 1 else wd, c)
                for p, c in zip(self.bucket.params, self._param_component)]

    def _table_lists(self):
        return optim.segment_table(self._table_entries(), "BridgeTrainer")

    def _segment_components(self) -> list:
        """the component of every segment of the table (segments never span two components: `segment_table`'s tag)"""
        return optim.segment_table(self._table_entries(), "BridgeTrainer", tags=True)[3]

    @property
    def lr_scales(self) -> dict:
        """``{component: multiplier of the learning rate}`` (a frozen component's is kept but unused)"""
        return dict(self._lr_scale)

    def set_lr_scale(self, name: str, value: float):
        """rewrite one component's learning-rate multiplier: a copy into the segment table on the device, outside the
        captured step, the way `set_lr` writes the rate itself - the next step uses it, nothing is captured again.
        (Only a trainer whose table was uniform - it launches the plain kernel - switches to the per-segment kernel at the
        first multiplier that differs, once: its captured step is dropped and the next graph step captures anew.)"""
        self._check_component(name, "set_lr_scale")
        self._lr_scale[name] = optim.check_lr_scale(value, f"set_lr_scale({name!r})")
        self._table.write(mults=[self._lr_scale[c] for c in self._seg_component])
        if not self._grouped and not self._table.uniform:
            self._grouped = True
            self._drop_capture()

    def train(self, mode: bool = True):
        """a frozen encoder stays in eval form"""
        super().train(mode)
        for name in getattr(self, "_frozen", ()):
            getattr(self, name).eval()
        return self

    # ------------------------------------------------------------------ averaged weights
    def _need_ema(self, who: str):
        if self.bucket.ema is None:
            raise RuntimeError(f"{who}: this trainer was built without ema_decay, there are no averaged weights")

    def _no_step_on_average(self, who: str):
        if self._ema_active:
            raise RuntimeError(f"{who} inside ema_weights(): the parameters hold the averaged weights; leave the context first")

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside, every trained parameter holds its exponential moving average: `evaluate`, `embed`,
        `evaluate_retrieval`, `predict`, `evaluate_classification`, `explain`, `perturb`, `temporal_attention` and
        `forward` see the averaged weights.  The contents of ``bucket.p`` and ``bucket.ema`` are exchanged in place (two
        bucket-sized copies each way, exact), so parameter views and a captured graph's pointers stay valid, and the
        prepared weight images are invalidated on both edges; on exit the live weights have their old bits and training
        goes on as if nothing had happened.  BatchNorm running statistics and the other buffers are not averaged (they
        are running averages already): the averaged weights run with the live buffers.  `train_step` /
        `train_step_packed` inside raise RuntimeError before any launch.  Not re-entrant."""
        self._need_ema("ema_weights")
        if self._ema_active:
            raise RuntimeError("ema_weights: already inside ema_weights()")
        with self.bucket.swapped():
            self._ema_active = True
            try:
                yield self
            finally:
                self._ema_active = False

    @torch.no_grad()
    def sync_ema(self):
        """set the average to the live weights (after weights were loaded by other means than a trainer checkpoint)"""
        self._need_ema("sync_ema")
        self._no_step_on_average("sync_ema")
        self.bucket.ema.copy_(self.bucket.p)

    def ema_state_dict(self) -> dict:
        """the model ``state_dict()`` with the averaged weights, as CPU copies: the trained parameters are the average,
        the frozen parameters and the buffers (BatchNorm statistics: live, not averaged) are what ``state_dict()`` holds.
        For export into the reference's modules."""
        self._need_ema("ema_state_dict")
        with self.ema_weights():
            return {k: v.detach().to("cpu", copy=True) for k, v in self.state_dict().items()}

    def forward(self, eeg: torch.Tensor, fmri: torch.Tensor, groups: Optional[torch.Tensor] = None):
        """the two encoders are independent until the heads: they run on two HIP
        streams (autograd replays each backward on its forward stream), so the
        many sub-chip kernels of one branch overlap the other's latency.
        ``groups``: (B,) integer ids, pairs with equal ids are positives of each other (ops.clip_loss)."""
        gid = self._need_groups(ops.group_ids(groups, eeg.shape[0], eeg.device, "BridgeTrainer"), "forward")
        fe, ff = self._encode(eeg, fmri)
        if not self.neighbour_radius:
            return self.head(fe, ff, self.group, gid)
        return self.head(fe, ff, self.group, gid, self.neighbour_radius)

    # ------------------------------------------------------------------ step
    def _labels(self, labels, B: int, device, who: str):
        """`ops.class_labels` plus the rule that a classify trainer's step takes labels and no other trainer's does"""
        if self.classify and labels is None:
            raise ValueError(f"{who}: this trainer was built with classify=True and needs labels=")
        if labels is not None and not self.classify:
            raise ValueError(f"{who}: labels= needs a trainer built with classify=True")
        return ops.class_labels(labels, B, self.num_classes, device, who)

    def _need_groups(self, gid, who: str):
        """``gid`` - or, for a trainer with ``neighbour_radius > 0`` called without ``groups=``, ``ValueError``: the ids
        are the timeline positions the radius is measured on"""
        if self.neighbour_radius and gid is None:
            raise ValueError(f"{who}: this trainer was built with neighbour_radius={self.neighbour_radius} and needs groups= "
                             "(the pairs' timeline ids, bridge_utils.timeline_ids)")
        return gid

    def _check_fmri(self, shape, training: bool, who: str):
        """the fMRI batch's shape, before the first launch of a step (or of its capture): ``ValueError`` otherwise"""
        self._fmri.check(self.fmri_encoder, shape, training, who)

    def _result(self, scal) -> Dict[str, torch.Tensor]:
        """the dict a step returns: views of the trainer's result words"""
        out = {"loss": scal[0], "top1_e2f": scal[1], "top1_f2e": scal[2]}
        if self.classify:
            o = self._scal_cls
            out.update(loss=scal[o + 4], contrastive_loss=scal[0], ce_loss=scal[o], cls_correct=scal[o + 1])
        return out

    def train_step(self, eeg: torch.Tensor, fmri: torch.Tensor, groups: Optional[torch.Tensor] = None,
                   labels: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """zero_grad -> forward -> backward -> (all-reduce) -> clip + AdamW.

        ``mode``: "graph" (default) replays the step from hipGraphs captured on
        first use (one graph at world 1; three segments around the two
        collectives otherwise); "manual" runs the same autograd-free tape eagerly;
        "autograd" goes through the public nn.Module / torch.autograd surface.
        ``groups``: (B,) integer ids (e.g. subjects; ``ops.group_ids``): pairs with equal ids are positives of each
        other (mm_clip_loss_own_rows_grouped).  In graph mode a grouped step is its own capture, as a new shape is.
        ``labels``: (B,) integer class labels (``ops.class_labels``), required by - and only taken by - a trainer built
        with ``classify=True``: the step then also trains the classification branch and returns ``contrastive_loss``,
        ``ce_loss``, ``cls_correct`` and ``loss`` = contrastive_loss + ce_weight * ce_loss."""
        self._no_step_on_average("train_step")
        self._check_fmri(fmri.shape, "fmri_encoder" not in self._frozen, "train_step")   # before the first launch of the step (or of its capture)
        if self._fmri.capture_words is not None and fmri.is_cuda:
            self._fmri.capture_words(self.fmri_encoder, fmri.device)   # the forward launch's words exist before any capture
            if self._key is not None and "fmri_encoder" in self._key:
                self._fmri.capture_words(self._key["fmri_encoder"], fmri.device)
        gid = self._need_groups(ops.group_ids(groups, eeg.shape[0], None if self.mode == "graph" else eeg.device, "train_step"),
                                "train_step")
        lab = self._labels(labels, eeg.shape[0], None if self.mode == "graph" else eeg.device, "train_step")
        if self._bank_size:
            self._bank_prepare(eeg.shape[0], gid is not None, "train_step")
        if lab is not None and self._cls_ticket is None:       # this trainer's own word, allocated before any capture
            self._cls_ticket = torch.zeros(1, dtype=torch.int32, device=self._scal.device)
        if self.eeg_time_augment is not None:
            self.eeg_time_augment.check(eeg.shape, self.augment, "train_step (eeg_time_augment)")
        aug_step = self._take_step("_aug_step")
        if aug_step is not None and self.mode != "graph":
            eeg = self._augmented_eeg(eeg, aug_step)
        if self.fmri_augment is not None:
            self.fmri_augment.check(fmri.shape, "train_step (fmri_augment)")
        fmri_aug_step = self._take_step("_fmri_aug_step")
        if fmri_aug_step is not None and self.mode != "graph":
            fmri = self.fmri_augment.batch(fmri, fmri_aug_step, dp.rank(self.group))
        if self.mode == "autograd":
            return self._step_autograd(eeg, fmri, gid, lab)
        if self.mode == "manual":
            with torch.no_grad():
                return self._step_manual(eeg, fmri, gid, lab)
        return self._step_graph(eeg, fmri, gid, aug_step, lab, fmri_aug_step)

    def _encode(self, eeg, fmri):
        """both encoders through their nn.Module surface: independent until the heads, so on two HIP streams"""
        if not self.two_streams:
            return self.eeg_encoder(eeg), self.fmri_encoder(fmri)
        main = torch.cuda.current_stream()
        self._side.wait_stream(main)
        with torch.cuda.stream(self._side):
            ff = self.fmri_encoder(fmri)
        fe = self.eeg_encoder(eeg)
        main.wait_stream(self._side)
        ff.record_stream(main)
        return fe, ff

    def _encode_with_keys(self, eeg, fmri):
        """`_encode`, and for a key trainer the key rows of the same batch (else None).  Each twin's eval pass runs BEFORE
        the online forward (it reads the running statistics this step's forward updates); a frozen encoder's online
        features are its key features.  Nothing of the key pass is on the tape."""
        if not self._key_encoder:
            return self._encode(eeg, fmri), None
        with torch.no_grad():
            kfe = self._eeg.forward(self._key["eeg_encoder"], eeg, None, False)[0] if "eeg_encoder" in self._key else None
            kff = self._fmri.forward(self._key["fmri_encoder"], fmri, False)[0] if "fmri_encoder" in self._key else None
        fe, ff = self._encode(eeg, fmri)
        with torch.no_grad():
            keys = self._key_embed(fe.detach() if kfe is None else kfe, ff.detach() if kff is None else kff)
        return (fe, ff), keys

    def _forward_classify(self, eeg, fmri, gid, lab):
        """the classify step's forward from the existing differentiable pieces (the independent path the tape is
        compared with): projection heads, F.normalize, the contrastive loss, `ops.bridge_cls_rows` (bridge_forward's
        train branch on the projected rows) and the weighted cross-entropy.  Seeds are drawn in the tape's order."""
        from . import small_autograd as sa
        br = self.head.bridge
        (fe, ff), keys = self._encode_with_keys(eeg, fmri)
        p = br.drop_p if self.training else 0.0
        ep = sa.proj_head(fe, br.eeg_proj, p)
        fp = sa.proj_head(ff, br.fmri_proj, p)
        ze = torch.nn.functional.normalize(ep, dim=1, eps=1e-12)
        zf = torch.nn.functional.normalize(fp, dim=1, eps=1e-12)
        logits, fw, aw = ops.bridge_cls_rows(br, ep, fp)
        lc, acc_e, acc_f = self._loss_autograd(ze, zf, gid, True, keys)
        ce = ops.weighted_cross_entropy(logits, lab.long(), self._class_weight)
        return lc, acc_e, acc_f, ce, logits

    def _loss_autograd(self, ze, zf, gid, training: bool, keys=None):
        """-> (loss, acc_e, acc_f): the trainer's contrastive loss on the differentiable surface, `_seg_loss`'s choice.
        A bank trainer's training step (``training``; everything else keeps the in-batch loss) scores against the bank
        (`ClipBankLossFn`: the bank is a constant of the tape), then pushes its own rows - detached: nothing of it is on
        the tape.  ``keys``: a key trainer's key rows (`_encode_with_keys`) - the batch's keys and what is pushed"""
        if self.neighbour_radius:                      # (no bank: refused at construction)
            if self.loss == "sigmoid":
                return ops.sigmoid_loss(ze, zf, self.head.logit_scale, self.head.logit_bias, self.group, gid, self.neighbour_radius)
            return ops.clip_loss(ze, zf, self.head.logit_scale, self.group, gid, self.neighbour_radius)
        if self.loss == "sigmoid":
            return ops.sigmoid_loss(ze, zf, self.head.logit_scale, self.head.logit_bias, self.group, gid)
        if not (training and self._bank_size):
            return ops.clip_loss(ze, zf, self.head.logit_scale, self.group, gid)
        if keys is not None:
            out = ops.clip_loss_key(ze, zf, keys, self.head.logit_scale, self._bank, gid, self._bank_warmup)
            with torch.no_grad():
                ops.clip_bank_push(keys, gid, self._bank)
            return out
        if self._bank_live:
            out = ops.clip_loss_bank(ze, zf, self.head.logit_scale, self._bank, gid, self._bank_warmup)
        else:                                          # a warm-up step: the in-batch loss, the bank only fills
            out = ops.clip_loss(ze, zf, self.head.logit_scale, self.group, gid)
        with torch.no_grad():
            ops.clip_bank_push(ops._packed_pair(ze, zf).detach().float().contiguous(), gid, self._bank)
        return out

    def _step_autograd(self, eeg, fmri, gid=None, lab=None):
        b = self.bucket
        b.zero_grad()
        out = {}
        if lab is not None:
            lc, acc_e, acc_f, ce, logits = self._forward_classify(eeg, fmri, gid, lab)
            loss = lc + self.ce_weight * ce
            out = {"contrastive_loss": lc.detach(), "ce_loss": ce.detach(),
                   "cls_correct": (logits.detach().argmax(dim=1) == lab).sum().float()}
        else:
            feats, keys = self._encode_with_keys(eeg, fmri)
            loss, acc_e, acc_f = self._loss_autograd(*self.head.embed(*feats), gid, True, keys)
        loss.backward()
        b.absorb_autograd_grads()
        self._seg_optimizer()
        return {"loss": loss.detach(), "top1_e2f": acc_e, "top1_f2e": acc_f, **out}

    # ---- the segments of the autograd-free tape ------------------------------
    STAMP_NAMES = ("step start", "weights prepared", "EEG fwd done", "fMRI fwd start", "fMRI fwd done",
                   "heads fwd done", "loss done", "heads bwd done", "EEG bwd done", "fMRI bwd start",
                   "fMRI bwd done", "grad reductions done", "AdamW done", "side stream done",
                   "EEG key pass done", "fMRI key pass done")     # (the last two: key_encoder=True only)

    def _stamp(self, i):
        if self.stamps is not None:
            _hip.call("mm_debug_stamp", self.stamps, i)

    def _seg_forward(self, eeg, fmri, xb=None, lab=None):
        """``xb``: the EEG batch already packed (B, T, Cp) bf16 (the captured step reads its static packed buffer, which
        the trainer fills outside the graph together with the input copies).  ``lab``: int32 device class labels (a
        classify trainer's step): the classification branch's forward follows the projection heads'."""
        self._stamp(0)
        # one memset of what the step's accumulators actually use (high-water mark of the first
        # step + slack); the gradient bucket is cleared by the previous step's AdamW kernel
        if self._weight_list is not None:
            # every bf16 weight image of the step AND the clearing of its accumulators: one launch
            ops.arena.begin(eeg.device, clear=self._arena_need, defer_zero=True)
            ops.weights.prepare_all(self._weight_list, zero=ops.arena.zero_range())
        else:
            ops.arena.begin(eeg.device, clear=self._arena_need)
        self._stamp(1)
        main = torch.cuda.current_stream()
        self._side.wait_stream(main)                 # fork point: recorded before any encoder kernel
        # The longer branch is issued FIRST: a hipGraph replay writes its kernel packets in capture order at
        # ~4.6 us per node, and the branch captured second cannot start before the host has written every packet
        # of the first (profiles/README.md).  That is the EEG chain at 32^3 voxels, the fMRI branch at config #4's
        # 64 x 64 x 48 (`step_schedule`; which row-wise backward the saved blocks take bears on the backward only).
        def schedule(fused_rows):
            return step_schedule(self._eeg_kind, self._fmri_kind, self._frozen, tuple(fmri.shape[1:]), fused_rows, os.environ)
        sched = schedule(False)
        # key_encoder: each trained encoder's twin runs its eval form IN FRONT of the online pass, on that branch's own
        # stream - stream order alone makes it read the BatchNorm running statistics as they stood before this step's
        # update.  A frozen encoder has no twin: its online pass is the eval form, its features are the key features.
        key = self._key or {}
        kf = {}

        def fmri_branch():
            with torch.cuda.stream(self._side):
                self._stamp(3)                           # (frozen: the eval form, nothing saved, no seed drawn)
                if "fmri_encoder" in key:
                    kf["fmri"] = self._fmri.forward(key["fmri_encoder"], fmri, False)[0]
                    self._stamp(15)
                out = self._fmri.forward(self.fmri_encoder, fmri, sched.fmri_live)
                self._stamp(4)
            return out
        if sched.fmri_first:
            ff, sv_f = fmri_branch()
        if "eeg_encoder" in key:
            kf["eeg"] = self._eeg.forward(key["eeg_encoder"], eeg, xb, False)[0]
            self._stamp(14)
        fe, sv_e = self._eeg.forward(self.eeg_encoder, eeg, xb, sched.eeg_live)
        self._stamp(2)
        if not sched.fmri_first:
            ff, sv_f = fmri_branch()
        main.wait_stream(self._side)
        z, sv_h = ops.contrastive_embed_impl(self.head.bridge, fe, ff, True)
        if self._key_encoder:
            self._key_rows = self._key_embed(kf.get("eeg", fe), kf.get("fmri", ff))
        sv_c = None
        if lab is not None:
            o = self._scal_cls
            sv_c = ops.bridge_cls_forward_impl(self.head.bridge, sv_h, True, lab, self._class_weight, self.ce_weight,
                                               loss_out=self._scal[o:o + 4], ticket=self._cls_ticket)[3]
        self._stamp(5)
        # the backward's schedule travels with what the forward saved (across a graph-segment boundary too): the same
        # pure function, asked again now that the saved blocks say which row-wise backward they take
        self.schedule = sched = schedule(sched.eeg_live and ffn_rows_bwd_fused(sv_e.get("blocks")))
        return z, (sv_e, sv_f, sv_h, sv_c, sched)

    def _seg_loss(self, z_all, scal, dz, gid_all=None):
        """symmetric InfoNCE of this rank's rows against the gathered batch, gradient w.r.t. ITS rows only
        (``mm_clip_loss_own_rows``: every rank evaluates all rows of the gathered batch, so no reduce-scatter
        of column gradients is needed).  ``scal`` = the trainer's own 4-float result buffer, ``dz`` (B, 2N): both written with plain stores.
        ``gid_all``: the gathered int32 group ids -> the grouped loss (``mm_clip_loss_own_rows_grouped``).
        ``loss="sigmoid"``: the pairwise sigmoid loss on the same inputs (``mm_sigmoid_loss_own_rows``), ``scal`` 5 floats.
        ``bank_size > 0``: the loss against the batch and the valid bank rows (``mm_clip_bank_loss``), then the push of the
        step's rows (``mm_clip_bank_push``) behind it on the same stream.
        ``neighbour_radius > 0``: the masked form of either loss (``mm_clip_loss_own_rows_masked``,
        ``mm_sigmoid_loss_own_rows_masked``) in place of the grouped launch."""
        ls = self.head.logit_scale.detach().reshape(1)
        B, row0 = dz.shape[0], dp.rank(self.group) * dz.shape[0]
        if self.neighbour_radius:                      # (no bank: refused at construction)
            if self.loss == "sigmoid":
                ops.sigmoid_loss_own_rows(z_all, gid_all, ls, self.head.logit_bias.detach().reshape(1), scal, dz, B, row0,
                                          self.neighbour_radius)
            else:
                ops.clip_loss_own_rows(z_all, gid_all, ls, scal, dz, B, row0, self.neighbour_radius)
        elif self.loss == "sigmoid":
            ops.sigmoid_loss_own_rows(z_all, gid_all, ls, self.head.logit_bias.detach().reshape(1), scal, dz, B, row0)
        elif self._key_encoder:                        # the keys of the batch and the rows pushed are the key encoder's
            ops.clip_key_loss(z_all, self._key_rows, gid_all, self._bank, ls, scal, dz, self._bank_warmup)
            ops.clip_bank_push(self._key_rows, gid_all, self._bank)
        elif self._bank_size:
            if self._bank_live:
                ops.clip_bank_loss(z_all, gid_all, self._bank, ls, scal, dz, self._bank_warmup)
            else:                                      # a warm-up step: the in-batch loss, the bank only fills
                ops.clip_loss_own_rows(z_all, gid_all, ls, scal, dz, B, row0)
            ops.clip_bank_push(z_all, gid_all, self._bank)
        else:
            ops.clip_loss_own_rows(z_all, gid_all, ls, scal, dz, B, row0)
        self._stamp(6)

    def _reduce_group(self, ready: str):
        """all-reduce (asynchronous: the issuing stream does not wait) every bucket range whose gradients are final at
        ``ready``; the handles are waited for by `_seg_optimizer`.  Host issue order = collective order on every rank."""
        for name, rdy, lo, hi in self.groups:
            if rdy == ready and hi > lo:
                self._works.append(dp.allreduce_sum_(self.bucket.g[lo:hi], self.group, async_op=True))

    def _seg_backward(self, saved, dz, scal, reduce: bool = False):
        """``reduce``: all-reduce every layer group of the gradient bucket as soon as it is final - the fMRI encoder's
        after that branch's backward, the transformer stack's and conv blocks 3-2's after their handed-over sums were
        flushed on the side stream (all three hidden beside the EEG chain), conv block 1's after the chain"""
        sv_e, sv_f, sv_h, sv_c, sched = saved
        self._works = []
        pending = list(sched.reduce_order) if reduce else []

        def reduce_ready(ready):                 # the schedule's next collective, once ``ready``'s gradients are final
            if pending and pending[0][0] == ready:
                self._reduce_group(pending.pop(0)[0])
        bag = GradBag()
        with deferred(bag, dz.device):           # ONE batched reduction after both branches joined
            # d loss / d logit_scale (scal[3]) rides in the same batched reduction launch
            bag.defer(scal.data_ptr() + 12, self.head.logit_scale._mm_grad.view(1), 1, 1, 1, keep=scal)
            if self.loss == "sigmoid":           # and d loss / d logit_bias (scal[4])
                bag.defer(scal.data_ptr() + 16, self.head.logit_bias._mm_grad.view(1), 1, 1, 1, keep=scal)
            if sv_c is None:
                dfe, dff = contrastive_embed_bwd(bag, sv_h, dz)
            else:                                # the classification branch's two launches, then the heads' with its da
                o = self._scal_cls
                da = bridge_cls_bwd(bag, sv_c, loss_in=scal[0:1], loss_total=scal[o + 4:o + 5])
                dfe, dff = contrastive_embed_bwd_da(bag, sv_h, dz, da)
            self._stamp(7)
            main = torch.cuda.current_stream()
            self._side.wait_stream(main)
            handed = []                          # (`step_schedule`: why, and when, the chain hands its sums to the side stream)

            def split():
                if not sched.hand:
                    return
                ev = torch.cuda.Event()
                handed.append((bag.hand_over(), ev))
                ev.record()
            # second hand-over: the weight gradients of conv blocks 3 and 2 (k = 3, 5) leave the chain too;
            # block 1's (the last kernel of the chain) stays, and its slot sum runs on this stream BEFORE
            # the join below instead of after it
            def split_convs():
                split()
                bag.defer_conv_wgrads = False
            bag.defer_conv_wgrads = sched.handed_convs >= 2

            def conv3_done():
                bag.defer_conv_wgrads = sched.handed_convs >= 1

            def fmri_branch():
                with torch.cuda.stream(self._side):
                    self._stamp(9)
                    bag_f = GradBag()                    # the fMRI branch flushes its own reductions on ITS stream,
                    with deferred(bag_f, dz.device):     # hidden beside the rest of the EEG backward
                        if sched.fmri_live:              # (frozen: no backward launch of this encoder)
                            self._fmri.backward(bag_f, sv_f, dff)
                    self._stamp(10)
                    reduce_ready("fmri")
                    for i, (hb, ev) in enumerate(handed):
                        self._side.wait_event(ev)
                        hb.flush(dz.device)
                        reduce_ready(f"handed{i}")
                    self._stamp(13)
                return bag_f
            if not sched.hand:
                bag_f = fmri_branch()
            finish = None
            if sched.eeg_live:                   # (frozen: no backward launch of this encoder); longer chain first (see _seg_forward)
                finish = self._eeg.backward(bag, sv_e, dfe, after_blocks=split, after_conv2=split_convs, after_conv3=conv3_done)
            bag.flush(dz.device)
            if finish is not None:
                finish()
            self._stamp(8)
            if sched.hand:
                bag_f = fmri_branch()
            for ready, stream in pending:        # what only the chain's end makes final (the collectives run in host issue order)
                with torch.cuda.stream(self._side) if stream == "side" else contextlib.nullcontext():
                    self._reduce_group(ready)
            main.wait_stream(self._side)
        self._stamp(11)
        self._bags = self._bags[-12:] + [bag, bag_f] + [hb for hb, _ in handed]   # keep descriptor tables alive

    def _seg_optimizer(self, reduced: bool = False):
        """``reduced``: the backward issued the per-group all-reduces (wait for them); else ONE all-reduce of the whole bucket"""
        if reduced:
            for w in self._works:
                dp.wait(w)
            self._works = []
        else:
            dp.allreduce_sum_(self.bucket.g, self.group)
        self._seg_adamw()

    def _seg_adamw(self):
        # parameter groups: the segment table in place of the scalar decay; with bucket.ema the weight average rides along
        optim.adamw_update(self.bucket, self.betas, self.eps, self.grad_clip, 1.0 / self.world, 1, ops.EP(),
                           self._table if self._grouped else self.weight_decay, self.ema_decay, self.ema_warmup)
        ops.weights_changed()
        if self._arena_need is None:
            self._arena_need = (ops.arena.high * 5 // 4 + 4095) // 4096 * 4096
        ops.arena.end()
        self._stamp(12)

    def _step_manual(self, eeg, fmri, gid=None, lab=None):
        recording = self._weight_list is None
        if recording:                                 # first step: note every weight image the tape asks for
            ops.weights.start_recording()
        try:
            return self._step_manual_body(eeg, fmri, gid, lab)
        finally:
            if recording:
                self._weight_list = ops.weights.stop_recording()

    def _step_manual_body(self, eeg, fmri, gid=None, lab=None):
        gid_all = None if gid is None else dp.gather_embeddings(gid.view(-1, 1), self.group).view(-1)
        z, saved = self._seg_forward(eeg, fmri, lab=lab)
        z_all = dp.gather_embeddings(z, self.group)
        scal, dz = self._scal, ops._empty(tuple(z.shape), torch.float32, z)
        self._seg_loss(z_all, scal, dz, gid_all)
        early = dp.active(self.group)
        self._seg_backward(saved, dz, scal, reduce=early)
        self._seg_optimizer(reduced=early)
        return self._result(scal)

    # ---- hipGraph capture ------------------------------------------------------
    def _capture(self, eeg, fmri, gid=None, lab=None):
        dev = eeg.device
        if self._cls_ticket is not None:
            self._cls_ticket.zero_()                      # (a launch that died mid-count would have left it non-zero)
        if self._fmri.capture_words is not None:
            self._fmri.capture_words(self.fmri_encoder, dev).zero_()
        world = self.world
        c = {"epoch": torch.zeros(1, dtype=torch.int32, device=dev)}
        # the step's static inputs are views of ONE flat buffer `c["in"]` (`bridge_branches.input_layout`), so that a
        # host-fed loop fills them with a single copy (`train_step_packed`)
        Bx, Cx, Tx = eeg.shape
        c["grouped"] = gid is not None
        c["labelled"] = lab is not None
        c["bank_live"] = self._bank_live              # which loss the recorded step launches (a bank trainer's warm-up)
        n_e, n_f, n_g, n_l = input_layout(self._eeg, eeg.shape, fmri.numel(), c["grouped"], c["labelled"])
        c["in"] = torch.empty(n_e + n_f + n_g + n_l, dtype=torch.uint8, device=dev)
        c["fmri"] = c["in"][n_e:n_e + n_f].view(torch.float32).view(fmri.shape)
        c["fmri"].copy_(fmri)
        c["gid"] = c["gid_all"] = None
        if c["grouped"]:
            c["gid"] = c["in"][n_e + n_f:n_e + n_f + n_g].view(torch.int32)
            c["gid"].copy_(gid)
        c["lab"] = None
        if c["labelled"]:
            c["lab"] = c["in"][n_e + n_f + n_g:].view(torch.int32)
            c["lab"].copy_(lab)
        if self._eeg.raw_input:
            c["eeg"], c["xb"] = c["in"][:n_e].view(torch.float32).view(eeg.shape), None
            c["eeg"].copy_(eeg)
        else:
            c["eeg"] = eeg.clone()                      # (shape carrier / in-place loader target; the graph reads c["xb"])
            c["xb"] = c["in"][:n_e].view(torch.bfloat16).view(Bx, Tx, ops.cpad(Cx))
            _hip.call("mm_pack_nct_bf16", c["eeg"], c["xb"], Bx, Cx, Tx, c["xb"].shape[2])
        ops.set_seed_epoch(c["epoch"])
        # warm-up outside capture (lazy inits, allocator priming) on a snapshot of the
        # training state, so that the first replay is really step 1
        b = self.bucket
        snap = [t.clone() for t in (b.p, b.m, b.v, b.state)]
        bufs = [t for t in self.buffers() if t is not None]
        if b.ema is not None:                         # the warm-up steps average: the shadow is part of the training state
            bufs.append(b.ema)
        if self._bank is not None:                    # the warm-up steps push: the bank is part of the training state
            bufs += self._bank.tensors()
        snap_bufs = [t.clone() for t in bufs]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(2):
                self._step_manual(c["eeg"], c["fmri"], c["gid"], c["lab"])
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        with torch.no_grad():
            for t, sv in zip((b.p, b.m, b.v, b.state), snap):
                t.copy_(sv)
            for t, sv in zip(bufs, snap_bufs):
                t.copy_(sv)
        ops.weights_changed()                                     # weight-image kernels must be recorded
        c["pool"] = torch.cuda.graph_pool_handle()
        graphs = []

        # A process group's watchdog thread polls the events of its finished collectives (hipEventQuery) for a while after
        # they are done; under a GLOBAL-mode capture that call is refused and the watchdog ends the process ("operation
        # not permitted when stream is capturing" - seen once in the aborted-capture rehearsal, where the communicator
        # check runs right before the segments are recorded).  Every capture of a distributed job is therefore
        # thread-local: only this thread's calls are policed.
        dist_alive = torch.distributed.is_available() and torch.distributed.is_initialized()

        def record(fn, mode=None):
            mode = mode or ("thread_local" if dist_alive else "global")
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=c["pool"], capture_error_mode=mode), torch.no_grad():
                fn()
            graphs.append(g)

        B = eeg.shape[0]
        N2 = 2 * self.head.bridge.bridge_dim
        c["scal"] = self._scal
        dist_step = not (world == 1 and not (self.force_segments and self.group is not None))
        # a grouped step gathers its ids when it issues collectives (world > 1, or MM_DP_FORCE); else they are the local ones
        c["gid_gather"] = c["grouped"] and dist_step and dp.active(self.group)
        if c["grouped"]:
            c["gid_all"] = torch.empty(world * B, dtype=torch.int32, device=dev) if c["gid_gather"] else c["gid"]
        if not dist_step:
            def whole():
                z, saved = self._seg_forward(c["eeg"], c["fmri"], xb=c["xb"], lab=c["lab"])
                c["z"] = z
                c["dz"] = ops._empty(tuple(z.shape), torch.float32, z)
                self._seg_loss(z, c["scal"], c["dz"], c["gid_all"])
                self._seg_backward(saved, c["dz"], c["scal"])
                self._grad_probe()
                self._seg_adamw()
            record(whole)
            self.capture_mode = "one graph"
        elif dp.CAPTURABLE and os.environ.get("MM_DP_CAPTURE", "1") != "0" and self._capture_with_collectives(c, record, graphs, B, N2, world, dev):
            self.capture_mode = "one graph + captured RCCL collectives"
        else:
            self.capture_mode = "3 segments + 2 eager collectives"
            def seg1():
                c["z"], c["saved"] = self._seg_forward(c["eeg"], c["fmri"], xb=c["xb"], lab=c["lab"])
                c["dz"] = ops._empty((B, N2), torch.float32, c["z"])
            record(seg1)
            c["z_all"] = torch.empty(world * B, N2, device=dev)

            def seg2():
                self._seg_loss(c["z_all"], c["scal"], c["dz"], c["gid_all"])
                self._seg_backward(c["saved"], c["dz"], c["scal"])
            record(seg2)

            def seg3():
                self._grad_probe()
                self._seg_adamw()
            record(seg3)
        c["graphs"] = graphs
        self._cap = c

    def _grad_probe(self):
        """``self.grad_probe`` (a flat fp32 tensor the size of the bucket, set by a test BEFORE the first graph step):
        the step copies its finished gradients there just before clip + AdamW clears them - one more node, the
        arithmetic untouched - so that a replayed step's gradients can be compared with the oracle's"""
        probe = getattr(self, "grad_probe", None)
        if probe is not None:
            probe.copy_(self.bucket.g)

    def _capture_with_collectives(self, c, record, graphs, B, N2, world, dev) -> bool:
        """the N > 1 step as ONE hipGraph: the all-gather of the embeddings and the all-reduce of every layer group of the
        gradient bucket (side branch / chain, `_seg_backward`) are graph nodes (no replay gaps, no host in the step).
        Every rank then reports its outcome and ALL take the same form (`dp.agree_on_capture`): the graph when every rank
        captured it, else the three segments on every rank (returns False, nothing recorded).  A recorded collective has
        not run, so dropping the graphs leaves the ranks in step; when the abort came after collectives had been recorded,
        or only on some ranks, the communicator must first pass `dp.check_communicator`."""
        c["z_all"] = torch.empty(world * B, N2, device=dev)
        # the communicator must exist before the capture starts (its lazy initialisation is not capturable)
        dp.all_gather_into(c["z_all"], torch.zeros(B, N2, device=dev), self.group)
        dp.wait(dp.allreduce_sum_(torch.zeros(8, device=dev), self.group, async_op=True))
        torch.cuda.synchronize()

        def whole_dp():
            self._gather_group_ids(c)
            z, saved = self._seg_forward(c["eeg"], c["fmri"], xb=c["xb"], lab=c["lab"])
            c["z"] = z
            c["dz"] = ops._empty((B, N2), torch.float32, z)
            dp.all_gather_into(c["z_all"], z, self.group)
            self._seg_loss(c["z_all"], c["scal"], c["dz"], c["gid_all"])
            self._seg_backward(saved, c["dz"], c["scal"], reduce=True)
            for w in self._works:
                dp.wait(w)
            self._works = []
            self._grad_probe()
            self._seg_adamw()
        issued0 = dp.issued
        err = None
        try:
            # thread-local capture mode: the process group's watchdog thread polls its events while this thread captures
            record(whole_dp, mode="thread_local")
        except Exception as e:  # noqa: BLE001 - any refusal (RCCL, the caching allocator, a host sync)
            # keep the text only: the traceback holds `record`'s frame and with it the half-built graph object, and a
            # graph destroyed by the cyclic collector DURING the next capture ends the process (~CUDAGraph: "operation
            # not permitted when stream is capturing")
            err = f"{type(e).__name__}: {e}"
            e.__traceback__ = None
            del e
        verdict = dp.agree_on_capture(err is None, dp.issued - issued0, self.group)
        if verdict == "captured":
            return True
        import gc
        import warnings
        warnings.warn(f"collectives not captured into the step's hipGraph on every rank (this rank: "
                      f"{'captured' if err is None else err}; group verdict {verdict}); "
                      "all ranks use three graph segments around two eager collectives")
        if err is None:
            graphs.pop()                                          # this rank's graph is dropped with the others'
        c.pop("z", None), c.pop("dz", None)
        gc.collect()                                              # every graph of the attempt is gone before the segments are recorded
        torch.cuda.synchronize()
        c["pool"] = torch.cuda.graph_pool_handle()                # (the attempt's memory pool went with its last graph)
        self._works = []
        if verdict == "segments-after-abort":
            dp.check_communicator(self.group, dev)
        ops.arena.end()
        ops.weights_changed()
        return False

    def _gather_group_ids(self, c):
        """the all-gather of a grouped step's ids: issued at the start of the step on the side stream (off the EEG chain;
        the fMRI branch that follows it there is joined before the loss), skipped when the step issues no collectives"""
        if not c["gid_gather"]:
            return
        self._side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._side):
            dp.all_gather_into(c["gid_all"].view(-1, 1), c["gid"].view(-1, 1), self.group)

    def _step_graph(self, eeg, fmri, gid=None, aug_step=None, lab=None, fmri_aug_step=None):
        """``aug_step`` / ``fmri_aug_step``: the step index of the EEG / volume augmentation (trainers with that augmenter).
        The capture and its two warm-up steps see the batch as it came; what a replay reads is staged below, augmented."""
        if (self._cap is None or self._cap["eeg"].shape != eeg.shape or self._cap["fmri"].shape != fmri.shape
                or self._cap["grouped"] != (gid is not None) or self._cap["labelled"] != (lab is not None)
                or self._cap["bank_live"] != self._bank_live):
            step0, base0 = ops._seed_state["step"], ops._seed_state["base"]
            self._capture(eeg, fmri, gid, lab)
            # the dropout seeds of this capture were drawn from here on (checkpoint_state)
            self._cap["seed_step"], self._cap["seed_base"] = step0, base0
            if self._pending_epoch_word is not None:      # resumed: the replays go on from the saved epoch word
                self._cap["epoch"].fill_(self._pending_epoch_word)
                self._pending_epoch_word = None
        c = self._cap
        self._stage(c, eeg, fmri, aug_step, fmri_aug_step)
        if gid is not None and gid.data_ptr() != c["gid"].data_ptr():
            c["gid"].copy_(gid)
        if lab is not None and lab.data_ptr() != c["lab"].data_ptr():
            c["lab"].copy_(lab)
        return self._replay()

    def _replay(self):
        c = self._cap
        g = c["graphs"]
        if len(g) == 1:
            g[0].replay()
        else:
            if c["gid_gather"]:
                dp.all_gather_into(c["gid_all"].view(-1, 1), c["gid"].view(-1, 1), self.group)
            g[0].replay()                                              # forward
            dp.all_gather_into(c["z_all"], c["z"], self.group)
            g[1].replay()                                              # loss on the gathered batch + backward
            dp.allreduce_sum_(self.bucket.g, self.group)
            g[2].replay()                                              # clip + AdamW
        return self._result(c["scal"])

    # ---- host-fed input path ---------------------------------------------------
    def pack_host_batch(self, eeg: torch.Tensor, fmri: torch.Tensor, out: Optional[torch.Tensor] = None,
                        groups: Optional[torch.Tensor] = None) -> torch.Tensor:
        """CPU side of the host-fed loop (a data loader's job, off the step's critical path): one (EEG, fMRI) batch as
        ONE flat pinned byte buffer in the layout of the step's static inputs - the EEG epochs already in the first
        convolution's operand format (channels-last (B, T, Cp) bf16, zero-padded channels: half the bytes of fp32, and
        no pack launch on the device; raw fp32 for the STFT front-end) followed by the fp32 volumes.  Round-to-nearest-
        even on the host = what mm_pack_nct_bf16 does on the device: the step's arithmetic is bit-identical.
        ``groups``: a grouped batch's (B,) ids, appended as int32 (the layout of a grouped capture's inputs).
        Reference counterpart: the ``.to(device)`` of each batch, run_training_lite.py:480-481."""
        self._no_packed_augment("pack_host_batch")
        gid = ops.group_ids(groups.detach().cpu() if groups is not None else None, eeg.shape[0], None, "pack_host_batch")
        eeg, fmri = eeg.detach().cpu().float(), fmri.detach().cpu().float().contiguous()
        if self._eeg.raw_input:
            e_bytes = eeg.contiguous().view(-1).view(torch.uint8)
        else:
            B, C, T = eeg.shape
            xb = torch.zeros(B, T, ops.cpad(C), dtype=torch.bfloat16)
            xb[:, :, :C] = eeg.permute(0, 2, 1)
            e_bytes = xb.view(-1).view(torch.uint8)
        n_e, n_f, n_g, _ = input_layout(self._eeg, eeg.shape, fmri.numel(), gid is not None)
        n = n_e + n_f + n_g
        if out is None:
            out = torch.empty(n, dtype=torch.uint8).pin_memory()
        out[:n_e].copy_(e_bytes)
        out[n_e:n_e + n_f].copy_(fmri.view(-1).view(torch.uint8))
        if gid is not None:
            out[n_e + n_f:n].copy_(gid.view(torch.uint8))
        return out

    def train_step_packed(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """one graph-replayed step on a batch that is already in the packed layout of `pack_host_batch` and on the device
        (a staging buffer an H2D copy filled): ONE device-to-device copy into the static inputs, then the replay"""
        self._no_packed_augment("train_step_packed")
        self._no_step_on_average("train_step_packed")
        if self._cap is None:
            raise RuntimeError("train_step_packed: run one train_step(eeg, fmri) first (it captures the step and fixes the shapes)")
        c = self._cap
        if self._bank_size:
            if c["bank_live"] != (self._key_encoder or self._bank_pushes >= self._bank_warmup):
                raise RuntimeError("train_step_packed: the bank's warm-up has ended and the captured step is the warm-up's; run "
                                   "one train_step(eeg, fmri) (it captures the step that reads the bank)")
            self._bank_pushes += 1
        if flat.dtype != torch.uint8 or flat.numel() != c["in"].numel() or not flat.is_cuda:
            raise ValueError(f"train_step_packed: expected a device uint8 buffer of {c['in'].numel()} bytes")
        c["in"].copy_(flat, non_blocking=True)
        return self._replay()

    def host_feeder(self, depth: int = 3) -> "HostFeeder":
        """the loop that feeds `train_step_packed` from pinned host buffers (see `HostFeeder`)"""
        self._no_packed_augment("host_feeder")
        return HostFeeder(self, depth)

    def time_collectives(self, batch: int, iters: int = 50) -> Dict[str, float]:
        """microseconds per call of every collective one step issues, each alone at its message size (HIP events on the
        current stream around ``iters`` back-to-back calls; collective: every rank of the group must call it).  What the
        step pays is less: all but the all-gather and the last group run beside the backward."""
        if not dp.active(self.group):
            return {}
        dev = self.bucket.g.device
        N2 = 2 * self.head.bridge.bridge_dim
        z = torch.zeros(batch, N2, device=dev)
        z_all = torch.empty(self.world * batch, N2, device=dev)
        cases = [(f"all_gather embeddings ({batch}x{N2} fp32 per rank)", lambda: dp.all_gather_into(z_all, z, self.group))]
        for name, _, lo, hi in self.groups:
            buf = torch.zeros(hi - lo, device=dev)
            cases.append((f"all_reduce {name} ({(hi - lo) * 4 / 1e6:.2f} MB)",
                          lambda buf=buf: dp.wait(dp.allreduce_sum_(buf, self.group, async_op=True))))
        out = {}
        for name, fn in cases:
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[name] = a.elapsed_time(b) / iters * 1e3
        return out

    def input_buffers(self):
        """the static (eeg, fmri) tensors the captured step reads, or None before the first graph step:
        a loader that writes the next batch straight into them saves the two device copies per step"""
        return None if self._cap is None else (self._cap["eeg"], self._cap["fmri"])

    @contextlib.contextmanager
    def _eval_scope(self):
        """the eval form of every module inside; on exit each module's own train / eval flag is what it was (a frozen
        or hand-set sub-module stays as it is)"""
        modes = [(m, m.training) for m in self.modules()]
        self.eval()
        ops.weights_changed()                      # graph replays bypass the python-side version counter
        try:
            yield
        finally:
            for m, mode in modes:
                m.training = mode

    @torch.no_grad()
    def evaluate(self, eeg, fmri, groups=None, labels=None):
        """eval-mode loss and in-batch top-1 of one batch (``groups``, ``labels``: as in `train_step`; with labels also
        ``contrastive_loss``, ``ce_loss`` and ``cls_correct``, and ``loss`` is their weighted sum)"""
        lab = self._labels(labels, eeg.shape[0], eeg.device, "evaluate")
        self._check_fmri(fmri.shape, False, "evaluate")
        with self._eval_scope():
            if lab is None:
                loss, acc_e, acc_f = self.forward(eeg, fmri, groups)
                return {"loss": loss, "top1_e2f": acc_e, "top1_f2e": acc_f}
            gid = self._need_groups(ops.group_ids(groups, eeg.shape[0], eeg.device, "evaluate"), "evaluate")
            br = self.head.bridge
            fe, ff = self._encode(eeg, fmri)
            z, sv_h = ops.contrastive_embed_impl(br, fe, ff, False)
            cls = ops.bridge_cls_forward_impl(br, sv_h, False, lab, self._class_weight, self.ce_weight)[3]["loss"]
            N = br.bridge_dim
            lc, acc_e, acc_f = self._loss_autograd(z[:, :N], z[:, N:], gid, False)
            return {"loss": lc + cls[3], "top1_e2f": acc_e, "top1_f2e": acc_f, "contrastive_loss": lc, "ce_loss": cls[0],
                    "cls_correct": cls[1]}

    @torch.no_grad()
    def predict(self, eeg, fmri, batch_size: int = 256) -> Dict[str, torch.Tensor]:
        """the bridge classifier's eval-mode outputs for paired inputs (host or device, ``batch_size`` pairs at a time):
        ``logits`` (N, C), ``probs`` = softmax, ``pred`` = argmax (int64), ``fusion_weights`` (N, 2), ``attn_weights``
        (N, 2; head-averaged) on the trainer's device - the encoders, mm_proj_heads_fwd and mm_bridge_cls_fwd.  Never
        augments, draws no dropout seed, restores the train / eval state; on a trainer without ``classify`` the branch
        is the untrained initialisation."""
        if eeg.shape[0] != fmri.shape[0]:
            raise ValueError(f"predict: {eeg.shape[0]} EEG epochs but {fmri.shape[0]} fMRI volumes")
        if batch_size < 1:
            raise ValueError("predict: batch_size must be >= 1")
        dev = self._scal.device
        br = self.head.bridge
        with self._eval_scope():
            outs = []
            for x, y in zip(self._chunks(eeg, batch_size, dev), self._chunks(fmri, batch_size, dev)):
                self._check_fmri(y.shape, False, "predict")
                fe, ff = self._encode(x, y)
                _, sv_h = ops.contrastive_embed_impl(br, fe, ff, False)
                outs.append(ops.bridge_cls_forward_impl(br, sv_h, False)[:3])
        logits, fw, aw = (torch.cat(t) for t in zip(*outs))
        return {"logits": logits, "probs": torch.softmax(logits, dim=1), "pred": logits.argmax(dim=1),
                "fusion_weights": fw, "attn_weights": aw}

    def evaluate_classification(self, eeg, fmri, labels, batch_size: int = 256) -> dict:
        """`predict`, then the reference's ``evaluate_bridge`` metric dict (`fmri_utils.classification_metrics`: Accuracy,
        weighted F1 / Precision / Recall, and for two classes the AUC of class 1, 0.5 where undefined)"""
        from .fmri_utils import classification_metrics
        lab = ops.class_labels(labels.detach().cpu() if isinstance(labels, torch.Tensor) else labels, eeg.shape[0],
                               self.num_classes, None, "evaluate_classification")
        out = self.predict(eeg, fmri, batch_size)
        return classification_metrics(lab.numpy(), out["pred"].cpu().numpy(), out["probs"].cpu().numpy(), self.num_classes)

    @staticmethod
    def _chunks(x: torch.Tensor, batch_size: int, device):
        for i in range(0, x.shape[0], batch_size):
            yield x[i:i + batch_size].to(device, non_blocking=True)

    @torch.no_grad()
    def embed(self, eeg: Optional[torch.Tensor] = None, fmri: Optional[torch.Tensor] = None, batch_size: int = 256):
        """L2-normalised eval-mode embeddings of one or both modalities: ``ze`` (N_eeg, bridge_dim) and / or ``zf``
        (N_fmri, bridge_dim) fp32 on this trainer's device (None for a modality not given).  Host or device input,
        encoded ``batch_size`` items at a time; the projection head is the paired path's kernel with this modality's
        head in both halves, so a row is the same bits as in the paired eval embedding of the same batch.  Restores the
        train / eval state; draws no dropout seeds."""
        if eeg is None and fmri is None:
            raise ValueError("embed: give eeg and / or fmri")
        if batch_size < 1:
            raise ValueError("embed: batch_size must be >= 1")
        dev = self._scal.device
        br = self.head.bridge
        with self._eval_scope():
            ze = zf = None
            if eeg is not None:
                ze = torch.cat([ops.proj_embed_one(br, self.eeg_encoder(x), "eeg")
                                for x in self._chunks(eeg, batch_size, dev)])
            if fmri is not None:
                zf = torch.cat([ops.proj_embed_one(br, self.fmri_encoder(x), "fmri")
                                for x in self._chunks(fmri, batch_size, dev)])
        return ze, zf

    @torch.no_grad()
    def temporal_attention(self, eeg: torch.Tensor, method: str = "rollout", layer: Optional[int] = None,
                           batch_size: int = 256) -> Dict[str, torch.Tensor]:
        """Which time steps the EEG encoder's transformer stack attends to (``ops.encoder_attention``): ``method``
        "rollout" (attention rollout over all layers to the mean-pooled feature) or "received" (the attention every step
        receives in layer ``layer``, default the last).  Host or device input, ``batch_size`` epochs at a time like
        ``embed``.  -> {"tokens": (N, L)} and, where the token-to-sample map is fixed (ERP: pooled pairs, power: identity;
        not the overlapping STFT frames), "time": (N, T); fp32 on the trainer's device.  Forward kernels only, in their
        eval form (frozen BatchNorm, no dropout, no seed drawn) whatever the train / eval flags are: parameters,
        BatchNorm buffers, the dropout seed counter, the gradient bucket and a captured graph stay as they were.  An
        EEG encoder without transformer layers raises ValueError."""
        if batch_size < 1:
            raise ValueError("temporal_attention: batch_size must be >= 1")
        ops.weights_changed()                      # graph replays bypass the python-side version counter
        parts = [ops.encoder_temporal_attention(self.eeg_encoder, x, method, layer)
                 for x in self._chunks(eeg, batch_size, self._scal.device)]
        return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}

    @torch.no_grad()
    def evaluate_retrieval(self, eeg, fmri, batch_size: int = 256, ks=(1, 5, 10), k: int = 0, groups=None, radius: int = 0):
        """held-out gallery retrieval: ``embed`` both modalities, then ``retrieval_metrics`` (pair i is the positive of
        query i, both directions; with ``groups`` (N,) every pair of the query's group, the best-placed one ranked).
        k > 0 adds ``topk``: {"eeg_to_fmri": (idx, score), "fmri_to_eeg": (idx, score)}, each (N, k).
        ``radius`` > 0 (needs ``groups``, timeline ids): a pair within ``radius`` of the query's id, not equal to it, is
        ignored - it does not count against the rank and never appears in ``topk`` (``retrieval_metrics(radius=)``,
        mm_retrieval_masked).  The default 0 ranks neighbours as before, whatever the trainer's ``neighbour_radius``:
        pass ``radius=trainer.neighbour_radius`` to evaluate the way the trainer trains.  Single process only: a sharded
        gallery is not supported."""
        if self.world > 1:
            raise ValueError("evaluate_retrieval: the gallery is not sharded; run it on one process (world size 1)")
        if eeg.shape[0] != fmri.shape[0]:
            raise ValueError(f"evaluate_retrieval: {eeg.shape[0]} EEG epochs but {fmri.shape[0]} fMRI volumes")
        radius = int(radius)
        if radius < 0:
            raise ValueError(f"evaluate_retrieval: radius must be >= 0 (got {radius})")
        if radius > 0 and groups is None:
            raise ValueError(f"evaluate_retrieval: radius={radius} needs groups= (timeline ids, bridge_utils.timeline_ids)")
        ops.group_ids(groups, eeg.shape[0], None, "evaluate_retrieval")      # bad ids fail before the encoders run
        ze, zf = self.embed(eeg, fmri, batch_size)
        out = retrieval_metrics(ze, zf, ks, groups, radius)
        if k > 0 and radius > 0:
            _, ie, se = ops.retrieval(ze, zf, k=k, ranks=False, q_groups=groups, g_groups=groups, radius=radius)
            _, if_, sf = ops.retrieval(zf, ze, k=k, ranks=False, q_groups=groups, g_groups=groups, radius=radius)
            out["topk"] = {"eeg_to_fmri": (ie, se), "fmri_to_eeg": (if_, sf)}
        elif k > 0:
            _, ie, se = ops.retrieval(ze, zf, k=k, ranks=False)
            _, if_, sf = ops.retrieval(zf, ze, k=k, ranks=False)
            out["topk"] = {"eeg_to_fmri": (ie, se), "fmri_to_eeg": (if_, sf)}
        return out

    def explain(self, eeg: torch.Tensor, fmri: torch.Tensor, method: str = "integrated_gradients", n_steps: int = 50,
                baseline: str = "zero", chunk_steps: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """Which channels, time points and voxels make EEG epoch i match volume i: attributes each pair's eval-mode
        cosine similarity ``ze_i . zf_i`` - the matching score the contrastive step optimises (dropout off, frozen
        BatchNorm, projection heads followed by the L2 normalisation) - to the raw EEG and the raw volume.
        ``method``: "integrated_gradients" (``n_steps`` interpolation points from the ``baseline`` "zero" or "mean" = the
        batch mean, batched by ``ops.integrated_gradients``; ``chunk_steps`` overrides its memory rule), "gradient"
        (|d score / d input|) or "gradient_x_input".
        -> {"eeg": (B, C, T), "eeg_channels": (B, C) = the mean over time, "fmri": (B, 1, D, H, W), "scores": (B,)}, fp32
        on the trainer's device; with a tabular fMRI encoder "fmri" is (B, A + C) and "fmri_activation" (B, A) /
        "fmri_connectivity" (B, C) are views of it; with a sequence encoder "fmri" is (B, F, D, H, W), "fmri_frames" (B, F)
        its sum over each frame's voxels and "lag_weights" (B, F) the encoder's `lag_weights` of the batch.
        The training state is left as it was, bit for bit: parameters, Adam moments, optimizer
        words, BatchNorm buffers, the gradient bucket, the dropout seed counter and a captured graph (no seed is drawn in
        eval mode; the gradient bucket, into which the backward kernels add their parameter gradients, is restored).
        Costs and side effects to know: the existing module-level backward functions are reused whole, so every chunk also
        runs their weight-gradient kernels - work that attribution does not need - and those kernels add into the trainer's
        gradient bucket: the bit-for-bit guarantee rests on `explain` cloning the bucket before and copying it back after
        (one bucket-sized copy each way).  Every module's own train / eval flag is put back individually.  With
        ``chunk_steps=None`` the engine measures one step's memory with ``torch.cuda.reset_peak_memory_stats``, which
        resets the caller's peak-memory statistics of this device (`ops.integrated_gradients`)."""
        if method not in ops.XAI_MODES:
            raise ValueError(f"explain: method must be one of {sorted(ops.XAI_MODES)}, got {method!r}")
        if baseline not in ("zero", "mean"):
            raise ValueError(f"explain: baseline must be 'zero' or 'mean', got {baseline!r}")
        ig = method == "integrated_gradients"
        eeg, fmri, bases, accs, scores = self._pair_gradients(eeg, fmri, int(n_steps) if ig else 1,
                                                              baseline if ig else None, chunk_steps)
        steps = int(n_steps) if ig else 1
        attr_e, chan = ops.xai_finish(eeg, bases[0], accs[0], steps, method, channels=True)
        attr_f, _ = ops.xai_finish(fmri, bases[1], accs[1], steps, method)
        out = {"eeg": attr_e, "eeg_channels": chan, "fmri": attr_f, "scores": scores}
        if self._fmri.explain_views is not None:
            out.update(self._fmri.explain_views(self.fmri_encoder, attr_f, fmri))
        return out

    def _pair_gradients(self, eeg, fmri, steps: int, baseline: Optional[str], chunk_steps: Optional[int] = None):
        """the signed sums behind `explain`: -> (eeg, fmri on the device, [baseline or None] x 2, [sum over the ``steps``
        interpolation points of d (ze_i . zf_i) / d eeg, ... / d fmri], scores (B,) at the inputs).  ``baseline`` None:
        ONE evaluation at the inputs themselves (the plain gradient)."""
        if eeg.shape[0] != fmri.shape[0]:
            raise ValueError(f"explain: {eeg.shape[0]} EEG epochs but {fmri.shape[0]} fMRI volumes")
        if steps < 1:
            raise ValueError("explain: n_steps must be >= 1")
        self._check_fmri(fmri.shape, False, "explain")
        dev = self._scal.device
        eeg = eeg.detach().to(dev).float().contiguous()
        fmri = fmri.detach().to(dev).float().contiguous()
        B = eeg.shape[0]
        if baseline is None:
            steps, path, bases = 1, [eeg, fmri], [None, None]          # one step from the input itself = the input
        elif baseline == "mean":
            path = bases = [eeg.mean(dim=0, keepdim=True), fmri.mean(dim=0, keepdim=True)]
        else:
            path = bases = [None, None]
        scores = {}

        def forward(e, f):
            ze, zf = self.head.embed(self.eeg_encoder(e), self.fmri_encoder(f))
            return ops._packed_pair(ze, zf)

        def seed(z, s0, k):
            score, g = ops.xai_pair_score(z)
            if s0 + k == steps:                               # the last step is the input itself (alpha = 1)
                scores["at_input"] = score[-B:].clone()
            return g
        saved_seed = dict(ops._seed_state)
        g0 = self.bucket.g.clone()                            # the backward kernels add parameter gradients into the bucket
        try:
            with self._eval_scope():
                accs, _ = ops.integrated_gradients(forward, [eeg, fmri], path, steps, seed,
                                                   chunk_steps=1 if baseline is None else chunk_steps)
                if baseline is not None and steps == 1:           # a single step is the BASELINE (alpha = 0), not the input:
                    with torch.enable_grad(), ops.attribution_mode():      # the scores at the inputs, through the same kernels
                        z = forward(eeg.clone().requires_grad_(True), fmri.clone().requires_grad_(True))
                    scores["at_input"] = ops.xai_pair_score(z, want_seed=False)[0]
                    ops._release_tape(z)
                    del z
        finally:
            self.bucket.g.copy_(g0)
            ops._seed_state.update(saved_seed)
            ops.weights_changed()
        return eeg, fmri, bases, accs, scores["at_input"]

    def _perturb_units(self, modality: str, units):
        """the (kind, size) of `ops.perturb_scores` for `perturb`'s ``eeg_units`` / ``fmri_units``"""
        if modality == "eeg":
            if units == "channels":
                return ("rows", 1)
            allowed, what = ("windows",), "'channels' or ('windows', w)"
        else:
            if units is None:
                return self._fmri.perturb_default
            allowed, what = self._fmri.perturb_kinds, self._fmri.perturb_what
        if not isinstance(units, (tuple, list)) or len(units) != 2 or units[0] not in allowed:
            raise ValueError(f"perturb: {modality}_units must be {what}, got {units!r}")
        return (units[0], units[1])

    def perturb(self, eeg: torch.Tensor, fmri: torch.Tensor, method: str = "occlusion", eeg_units="channels", fmri_units=None,
                baseline: str = "zero", n_permutations: int = 16, seed: int = 0, permutations=None,
                chunk_masks: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """Does the match of pair i survive without this electrode, this time window, this block of the volume:
        perturbation attribution of the score `explain` attributes - the eval-mode cosine similarity ``ze_i . zf_i`` - from
        forward scores alone (`ops.perturb_scores`: the masked copies of the batch go through the encoder as a few large
        batches, csrc/perturb.hip).
        ``eeg_units``: "channels" or ("windows", w) = w time points of all channels; ``fmri_units``: ("blocks", s) = s^3
        voxels of a volume (default s = 8), for a tabular encoder ("windows", w) = w features (default 1), for a sequence
        encoder ("rows", 1) = one frame (default) or ("blocks", s) = s^3 voxels of all frames.  A knocked-out
        unit is replaced by the ``baseline``: "zero", or "mean" = the batch mean (as in `explain`).
        ``method``: "occlusion" - drop[b][u] = score_full[b] - score(unit u replaced): U evaluations per modality plus
        the full one; "shapley" - permutation-sampled Shapley values of the game whose players are the units:
        ``n_permutations`` = P permutations per modality from ``torch.randperm`` on a CPU generator seeded with ``seed``
        (EEG drawn first; all samples share them), or ``permutations`` = {"eeg": (P, U) long, "fmri": ...} in place of
        the draw (a modality not named is drawn); P (U - 1) + 2 evaluations per modality.  Each modality is perturbed
        with the OTHER intact, and that one is embedded once.
        -> {"eeg": (B, U_e), "fmri": (B, U_f), "scores": (B,)} fp32 on the trainer's device; Shapley adds
        "empty_scores": {"eeg": (B,), "fmri": (B,)}, the score with every unit of that modality replaced, so that
        sum_u phi[b][u] = scores[b] - empty_scores[b] up to rounding (efficiency).
        A drop is the difference of two bf16-operand scores: differences at the level of the scores' own error are noise
        (DESIGN.md 5p).  The encoders run the forward `explain` differentiates (eval mode with autograd on), so "scores"
        are `explain`'s and both methods attribute the same number; that forward keeps what a backward would need, which
        is dropped after every chunk and counted by the memory rule.  `embed`'s ``no_grad`` forward differs from it by
        bf16 rounding.  ``chunk_masks``: masks per batch; None = the memory rule of `ops.perturb_scores` (it resets this
        device's peak-memory statistics).  Changes nothing on the trainer and draws no dropout seed; every module's
        train / eval flag is put back; a captured graph goes on replaying.  No collectives: any rank may call it on
        its own data."""
        if method not in ("occlusion", "shapley"):
            raise ValueError(f"perturb: method must be 'occlusion' or 'shapley', got {method!r}")
        if baseline not in ("zero", "mean"):
            raise ValueError(f"perturb: baseline must be 'zero' or 'mean', got {baseline!r}")
        if eeg.shape[0] != fmri.shape[0]:
            raise ValueError(f"perturb: {eeg.shape[0]} EEG epochs but {fmri.shape[0]} fMRI volumes")
        self._check_fmri(fmri.shape, False, "perturb")
        units = {"eeg": self._perturb_units("eeg", eeg_units), "fmri": self._perturb_units("fmri", fmri_units)}
        # the sample shape each modality's units are cut from (a frame sequence's frames are the rows of (F, D * H * W))
        cut = {"eeg": tuple(eeg.shape[1:]), "fmri": tuple(fmri.shape[1:])}
        if self._fmri.perturb_shape is not None:
            cut["fmri"] = self._fmri.perturb_shape(units["fmri"][0], cut["fmri"])
        n_units = {k: ops.perturb_units(units[k][0], cut[k], units[k][1]) for k in ("eeg", "fmri")}
        masks, pos = {}, {}
        if method == "occlusion":
            for k, U in n_units.items():
                masks[k] = 1 - torch.eye(U, dtype=torch.int32)
        else:
            given = dict(permutations or {})
            if set(given) - {"eeg", "fmri"}:
                raise ValueError(f"perturb: permutations has keys {sorted(given)}; 'eeg' and / or 'fmri' are known")
            if not given.keys() >= {"eeg", "fmri"} and n_permutations < 1:
                raise ValueError("perturb: n_permutations must be >= 1")
            gen = torch.Generator().manual_seed(int(seed))
            for k, U in n_units.items():                                   # EEG first
                perm = given[k] if k in given else torch.stack([torch.randperm(U, generator=gen) for _ in range(int(n_permutations))])
                if isinstance(perm, torch.Tensor) and perm.dim() == 2 and perm.shape[1] != U:
                    raise ValueError(f"perturb: permutations[{k!r}] is {tuple(perm.shape)} but there are {U} units")
                prefix, pos[k] = ops.shapley_masks(perm)
                masks[k] = torch.cat([torch.zeros(1, U, dtype=torch.int32), prefix])      # the empty coalition first
        dev = self._scal.device
        shape = {"eeg": tuple(eeg.shape[1:]), "fmri": tuple(fmri.shape[1:])}
        x = {"eeg": eeg.detach().to(dev).float().contiguous(), "fmri": fmri.detach().to(dev).float().contiguous()}
        x = {k: t.view(t.shape[0], *cut[k]) for k, t in x.items()}
        base = {k: (t.mean(dim=0, keepdim=True) if baseline == "mean" else None) for k, t in x.items()}
        enc = {"eeg": self.eeg_encoder, "fmri": self.fmri_encoder}
        br = self.head.bridge

        def embed_rows(k, rows):
            # the forward `explain` differentiates - autograd on, the input asking for a gradient - so that both methods
            # attribute the same number; the `no_grad` forward of `embed` folds BatchNorm into the convolution kernels and
            # differs from it by bf16 rounding.  No backward follows: the tape is dropped at once.
            with torch.enable_grad(), ops.attribution_mode():
                f = enc[k](rows.detach().view(-1, *shape[k]).requires_grad_(True))
            z = ops.proj_embed_one(br, f, k)
            ops._release_tape(f)
            return z
        with self._eval_scope(), torch.no_grad():
            z = {k: embed_rows(k, x[k]) for k in ("eeg", "fmri")}
            out = {"scores": ops.perturb_pair_scores(z["eeg"], z["fmri"])[0]}
            empty = {}
            for k, other in (("eeg", "fmri"), ("fmri", "eeg")):
                v = ops.perturb_scores(lambda rows: ops.perturb_pair_scores(embed_rows(k, rows), z[other]),
                                       x[k], base[k], masks[k], units[k], chunk_masks)
                if method == "occlusion":
                    out[k] = (out["scores"].unsqueeze(0) - v).t().contiguous()
                else:
                    empty[k] = v[0].clone()
                    out[k] = ops.perturb_shapley(v[1:] if n_units[k] > 1 else None, empty[k], out["scores"], pos[k])
            if method == "shapley":
                out["empty_scores"] = empty
        return out


class HostFeeder:
    """Feeds `BridgeTrainer.train_step_packed` from packed pinned host buffers (`pack_host_batch`), one H2D copy per
    batch on a copy stream into a ring of ``depth`` staging buffers, overlapped with the steps before it.

    The ordering between the copy stream and the step's stream is kept by the HOST: `step()` blocks on the event its
    batch's copy recorded (issued a whole step earlier), `upload()` on the event recorded after the step that last read
    the staging buffer (``depth - 1`` steps earlier).  Neither queue ever holds a barrier for the other: with
    hipStreamWaitEvent in both directions the same loop lost 8 % to the two cross-queue waits per step, ordered from the
    host it loses 1 % (0.786 vs 0.779 ms, profiles/r04_h2d_probe.txt) - the host has the time, a step costs it 0.25 ms.

        feeder = trainer.host_feeder()
        feeder.upload(packed[0])
        for i in range(n):
            if i + 1 < n:
                feeder.upload(packed[i + 1])      # returns at once; the pinned buffer is free again when the event it returns is done
            out = feeder.step()

    Reference counterpart: the per-batch ``.to(device)`` + step of run_training_lite.py:474-489."""

    def __init__(self, trainer: BridgeTrainer, depth: int = 3):
        if trainer._cap is None:
            raise RuntimeError("HostFeeder: run one train_step(eeg, fmri) first (it captures the step and fixes the shapes)")
        if depth < 2:
            raise ValueError("HostFeeder: at least two staging buffers")
        n = trainer._cap["in"].numel()
        dev = trainer._cap["in"].device
        self.trainer, self.depth, self.nbytes = trainer, depth, n
        self.ring = [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(depth)]
        self.copy_stream = torch.cuda.Stream(device=dev)
        self.ready = [torch.cuda.Event() for _ in range(depth)]
        self.done = [torch.cuda.Event() for _ in range(depth)]
        self.uploaded = 0
        self.stepped = 0

    def upload(self, packed: torch.Tensor) -> "torch.cuda.Event":
        """start the H2D copy of the next batch; ``packed``: a pinned uint8 buffer from `pack_host_batch`.  Returns the
        event that marks the copy's end (until then the pinned buffer must not be rewritten)."""
        if packed.dtype != torch.uint8 or packed.numel() != self.nbytes or packed.is_cuda:
            raise ValueError(f"HostFeeder.upload: expected a host uint8 buffer of {self.nbytes} bytes")
        if self.uploaded - self.stepped >= self.depth:
            raise RuntimeError(f"HostFeeder.upload: {self.depth} batches are already waiting for their step")
        b = self.uploaded % self.depth
        if self.uploaded >= self.depth:
            self.done[b].synchronize()                    # the step that read this staging buffer has finished with it
        with torch.cuda.stream(self.copy_stream):
            self.ring[b].copy_(packed, non_blocking=True)
            self.ready[b].record(self.copy_stream)
        self.uploaded += 1
        return self.ready[b]

    def step(self) -> Dict[str, torch.Tensor]:
        """one training step on the oldest uploaded batch"""
        if self.stepped >= self.uploaded:
            raise RuntimeError("HostFeeder.step: nothing uploaded")
        b = self.stepped % self.depth
        self.ready[b].synchronize()                       # host-side: no barrier packet on the step's queue
        out = self.trainer.train_step_packed(self.ring[b])
        self.done[b].record()
        self.stepped += 1
        return out


def synthetic_pairs(batch: int, eeg_channels: int = 64, samples: int = 1024, vol=(32, 32, 32),
                    seed: int = 1234, device="cuda", latent: int = 16):
    """pairs share a 16-d latent so retrieval is learnable:
    EEG = A_e z broadcast over time + N(0,1), fMRI = A_f z reshaped + N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    gm = torch.Generator().manual_seed(99)
    A_e = torch.randn(eeg_channels, latent, generator=gm)
    A_f = torch.randn(vol[0] * vol[1] * vol[2], latent, generator=gm) / latent ** 0.5
    z = torch.randn(batch, latent, generator=g)
    eeg = (z @ A_e.t()).unsqueeze(-1) * 0.5 + torch.randn(batch, eeg_channels, samples, generator=g)
    fmri = (z @ A_f.t()).view(batch, 1, *vol) + torch.randn(batch, 1, *vol, generator=g)
    return eeg.to(device), fmri.to(device)


def synthetic_subject_pairs(subjects: int, per_subject: int, eeg_channels: int = 64, samples: int = 1024, vol=(32, 32, 32),
                            seed: int = 1234, device="cuda", latent: int = 16, epoch_noise: float = 0.5):
    """``synthetic_pairs`` with the structure of real recordings: several EEG epochs per subject, one fMRI volume per
    subject.  Subject s has one latent z_s and one volume A_f z_s + N(0,1), repeated for every pair of the subject;
    each EEG epoch is built from z_s + ``epoch_noise`` N(0,1) as in ``synthetic_pairs``.  Pairs are subject-major.
    -> (eeg (S*E, C, T), fmri (S*E, 1, *vol), groups int32 (S*E,) = the subject index), all on ``device``."""
    if subjects < 1 or per_subject < 1:
        raise ValueError("synthetic_subject_pairs: need subjects >= 1 and per_subject >= 1")
    g = torch.Generator().manual_seed(seed)
    gm = torch.Generator().manual_seed(99)
    A_e = torch.randn(eeg_channels, latent, generator=gm)
    A_f = torch.randn(vol[0] * vol[1] * vol[2], latent, generator=gm) / latent ** 0.5
    z = torch.randn(subjects, latent, generator=g)
    fmri_s = (z @ A_f.t()).view(subjects, 1, *vol) + torch.randn(subjects, 1, *vol, generator=g)
    groups = torch.arange(subjects).repeat_interleave(per_subject)
    z_ep = z[groups] + epoch_noise * torch.randn(subjects * per_subject, latent, generator=g)
    eeg = (z_ep @ A_e.t()).unsqueeze(-1) * 0.5 + torch.randn(subjects * per_subject, eeg_channels, samples, generator=g)
    fmri = fmri_s[groups]
    return eeg.to(device), fmri.to(device), groups.to(torch.int32).to(device)


def synthetic_sequence_pairs(batch: int, frames: int, peak: int, eeg_channels: int = 64, samples: int = 1024, vol=(32, 32, 32),
                             seed: int = 1234, device="cuda", latent: int = 16):
    """``synthetic_pairs`` whose fMRI is a sequence of ``frames`` volumes (batch, frames, *vol) with a planted lag: only
    frame ``peak`` carries the shared latent (A_f z + N(0, 1)), every other frame is N(0, 1) noise - what a lag pool must
    find.  The EEG, the maps and the latents are `synthetic_pairs`' for the same seed."""
    if frames < 1 or not 0 <= peak < frames:
        raise ValueError(f"synthetic_sequence_pairs: need frames >= 1 and 0 <= peak < frames (got {frames}, {peak})")
    g = torch.Generator().manual_seed(seed)
    gm = torch.Generator().manual_seed(99)
    A_e = torch.randn(eeg_channels, latent, generator=gm)
    A_f = torch.randn(vol[0] * vol[1] * vol[2], latent, generator=gm) / latent ** 0.5
    z = torch.randn(batch, latent, generator=g)
    eeg = (z @ A_e.t()).unsqueeze(-1) * 0.5 + torch.randn(batch, eeg_channels, samples, generator=g)
    fmri = torch.randn(batch, frames, *vol, generator=g)
    fmri[:, peak] += (z @ A_f.t()).view(batch, *vol)
    return eeg.to(device), fmri.to(device)


def _tabular_maps(activation_dim: int, connectivity_dim: int, eeg_channels: int, latent: int):
    gm = torch.Generator().manual_seed(99)
    A_e = torch.randn(eeg_channels, latent, generator=gm)
    A_f = torch.randn(activation_dim + connectivity_dim, latent, generator=gm) / latent ** 0.5
    return A_e, A_f


def synthetic_tabular_pairs(batch: int, eeg_channels: int = 64, samples: int = 1024, activation_dim: int = 100,
                            connectivity_dim: int = 200, seed: int = 1234, device="cuda", latent: int = 16):
    """``synthetic_pairs`` with the reference's tabular fMRI input: EEG = A_e z broadcast over time + N(0,1), fMRI =
    A_f z + N(0,1) as one (batch, activation_dim + connectivity_dim) row ``[activation | connectivity]``."""
    g = torch.Generator().manual_seed(seed)
    A_e, A_f = _tabular_maps(activation_dim, connectivity_dim, eeg_channels, latent)
    z = torch.randn(batch, latent, generator=g)
    eeg = (z @ A_e.t()).unsqueeze(-1) * 0.5 + torch.randn(batch, eeg_channels, samples, generator=g)
    fmri = z @ A_f.t() + torch.randn(batch, activation_dim + connectivity_dim, generator=g)
    return eeg.to(device), fmri.to(device)


def synthetic_tabular_subject_pairs(subjects: int, per_subject: int, eeg_channels: int = 64, samples: int = 1024,
                                    activation_dim: int = 100, connectivity_dim: int = 200, seed: int = 1234, device="cuda",
                                    latent: int = 16, epoch_noise: float = 0.5):
    """``synthetic_subject_pairs`` with tabular fMRI rows: one latent and one fMRI row per subject, repeated for each of its
    EEG epochs; pairs are subject-major.  -> (eeg (S*E, C, T), fmri (S*E, A + C), groups int32 (S*E,))."""
    if subjects < 1 or per_subject < 1:
        raise ValueError("synthetic_tabular_subject_pairs: need subjects >= 1 and per_subject >= 1")
    g = torch.Generator().manual_seed(seed)
    A_e, A_f = _tabular_maps(activation_dim, connectivity_dim, eeg_channels, latent)
    z = torch.randn(subjects, latent, generator=g)
    fmri_s = z @ A_f.t() + torch.randn(subjects, activation_dim + connectivity_dim, generator=g)
    groups = torch.arange(subjects).repeat_interleave(per_subject)
    z_ep = z[groups] + epoch_noise * torch.randn(subjects * per_subject, latent, generator=g)
    eeg = (z_ep @ A_e.t()).unsqueeze(-1) * 0.5 + torch.randn(subjects * per_subject, eeg_channels, samples, generator=g)
    return eeg.to(device), fmri_s[groups].to(device), groups.to(torch.int32).to(device)
