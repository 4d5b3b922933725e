"""Training-side classes of the reference's EEG notebook (``EEG_CODE/CrossModal_EEG_scr.ipynb``) on the
MI355X HIP path: ``PerFoldNormalizer`` (cell 19), ``FocalLoss`` (cell 20), ``ImprovedTriModalFusionNet`` /
``ImprovedSmartFusionNet`` (cells 21-22), ``FlexibleTrainer`` (cell 23) and ``collate_trimodal`` (cell 24); the
single-modality baselines ``ERPOnlyNet`` / ``PWOnlyNet`` with ``ERPEncoder`` / ``PowerEncoder`` / ``BaseEEGModel`` and
``evaluate_late_fusion``; ``InterpretabilityAnalyzer`` (channel ablation, channel Shapley values and
integrated gradients).

SURVEY.md §8 (f).1 / (f).3: same names, constructor arguments, batch conventions and checkpoint
container (``epoch / model_state_dict / optimizer_state_dict / scheduler_state_dict / metrics``) as
the notebook, so ``best_trimodal_fold*.pt`` files move between the two.  Model forward/backward, the
losses and the optimizer step run in the HIP kernels; there is no CPU path.
"""
from __future__ import annotations

import logging
import numbers
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from . import augment_stream as AS, ops
from .bridge_utils import ImprovedTriModalFusionNet, WeightedCrossEntropy
from .crossmodal_v4_enhancements import EnhancedSmartFusionNetV4, get_fusion_weights_from_model
from .optim import FusedAdamW


class PerFoldNormalizer:
    """global mean / std over every value of the training subjects' entries (keys are tuples whose
    first element is the subject), applied to all entries (cell 19)."""

    def __init__(self):
        self.stats = {}

    def fit_on_indices(self, data_dict, train_indices, subject_array):
        train_subjects = set(np.asarray(subject_array)[train_indices])
        vals = [np.asarray(v).flatten() for k, v in data_dict.items() if k[0] in train_subjects]
        flat = np.concatenate(vals)
        self.stats["mean"] = np.mean(flat)
        self.stats["std"] = np.std(flat) + 1e-8

    def transform(self, data_dict):
        return {k: (v - self.stats["mean"]) / self.stats["std"] for k, v in data_dict.items()}


class FocalLoss(nn.Module):
    """alpha (1 - p_t)^gamma CE (cell 20), one kernel forward + gradient."""

    def __init__(self, alpha: float = 0.25, gamma: float = 2.0, reduction: str = "mean"):
        super().__init__()
        self.alpha, self.gamma, self.reduction = alpha, gamma, reduction

    def forward(self, inputs, targets):
        red = self.reduction if self.reduction in ("mean", "sum") else "none"
        return ops.focal_loss(inputs, targets, self.alpha, self.gamma, red)


class ImprovedSmartFusionNet(nn.Module):
    """two-modality checkpoint wrapper (cell 22): keys carry the ``model.`` prefix;
    ``return_feats`` -> dict(logits, gates, fused_feats)."""

    def __init__(self, in_pw_dim, in_erp_dim, fusion_dim=128, num_classes=2, dropout=0.4,
                 num_transformer_layers=2, num_heads=4, use_cross_attention=True):
        super().__init__()
        self.model = EnhancedSmartFusionNetV4(erp_channels=in_erp_dim, pw_channels=in_pw_dim, hidden_dim=fusion_dim,
                                              num_classes=num_classes, dropout=dropout,
                                              num_transformer_layers=num_transformer_layers, num_heads=num_heads,
                                              use_cross_attention=use_cross_attention)
        self.use_cross_attention = use_cross_attention
        self.fusion_weight_history = []

    def forward(self, erp, pw, return_feats=False):
        if return_feats:
            logits, gates, fused = self.model(erp, pw, return_fusion_weights=True, return_fused_feats=True)
            return {"logits": logits, "gates": gates, "fused_feats": fused}
        return self.model(erp, pw)

    def get_fusion_weights(self):
        return get_fusion_weights_from_model(self.model)

    def track_fusion_weights(self):
        w = self.get_fusion_weights()
        if w:
            self.fusion_weight_history.append(w)

    def get_weight_history(self):
        return self.fusion_weight_history


class BaseEEGModel(nn.Module):
    """(cell 5) the common forward signature of the notebook's four models"""

    def forward(self, erp: Optional[torch.Tensor] = None, pw: Optional[torch.Tensor] = None,
                return_feats: bool = False) -> torch.Tensor:
        raise NotImplementedError


class PowerEncoder(nn.Module):
    """(cell 8) three Conv1d(k=3)-BatchNorm1d-ReLU blocks at 32 / 64 / 128 channels, MaxPool1d(2) after the first two, a
    1 x 1 projection to ``out_dim`` and dropout: (B, C, T) -> (B, T / 4, out_dim) fp32.  T % 4 == 0 (the kernels pool even
    lengths; MaxPool1d's floor on an odd length is not served), out_dim a multiple of 16 up to 512."""

    def __init__(self, in_channels: int, out_dim: int = 128, dropout: float = 0.2):
        super().__init__()
        self.conv1 = nn.Conv1d(in_channels, 32, kernel_size=3, padding=1)
        self.bn1 = nn.BatchNorm1d(32)
        self.conv2 = nn.Conv1d(32, 64, kernel_size=3, padding=1)
        self.bn2 = nn.BatchNorm1d(64)
        self.conv3 = nn.Conv1d(64, 128, kernel_size=3, padding=1)
        self.bn3 = nn.BatchNorm1d(128)
        self.proj = nn.Conv1d(128, out_dim, kernel_size=1)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.eeg_step_encoder_forward(self, x, "pw")


class PWOnlyNet(BaseEEGModel):
    """(cell 9) the power-only baseline: PowerEncoder -> max over time -> Linear-BatchNorm1d-GELU-Dropout(0.5)-Linear.
    The projection, its dropout and the max run as one launch (csrc/timepool.hip); ``return_feats`` is accepted and
    ignored, as in the notebook."""

    def __init__(self, in_channels: int, pw_out: int = 128, hidden: int = 64, n_classes: int = 2):
        super().__init__()
        self.pw_enc = PowerEncoder(in_channels=in_channels, out_dim=pw_out)
        self.pool = nn.AdaptiveMaxPool1d(1)
        self.head = nn.Sequential(
            nn.Flatten(),
            nn.Linear(pw_out, hidden),
            nn.BatchNorm1d(hidden),
            nn.GELU(),
            nn.Dropout(0.5),
            nn.Linear(hidden, n_classes)
        )

    def forward(self, erp: Optional[torch.Tensor] = None, pw: torch.Tensor = None,
                return_feats: bool = False) -> torch.Tensor:
        return ops.eeg_baseline_forward(self, pw, "pw")


class ERPEncoder(nn.Module):
    """(cell 12) Conv1d(k=7 / 5 / 3)-BatchNorm1d-ReLU blocks at 32 / 64 / 128 channels, MaxPool1d(2) after the first two and
    a 1 x 1 projection of every time step: (B, C, T) -> (B, T / 4, out_dim) fp32.  Its ``dropout`` module is never applied
    (as in the notebook).  T % 4 == 0, out_dim a multiple of 16 up to 512."""

    def __init__(self, in_channels: int = 18, out_dim: int = 128, dropout: float = 0.2):
        super().__init__()
        self.out_dim = out_dim
        self.conv1 = nn.Conv1d(in_channels, 32, kernel_size=7, padding=3)
        self.bn1 = nn.BatchNorm1d(32)
        self.conv2 = nn.Conv1d(32, 64, kernel_size=5, padding=2)
        self.bn2 = nn.BatchNorm1d(64)
        self.conv3 = nn.Conv1d(64, 128, kernel_size=3, padding=1)
        self.bn3 = nn.BatchNorm1d(128)
        self.pool = nn.MaxPool1d(2)
        self.step_proj = nn.Conv1d(128, out_dim, kernel_size=1)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.eeg_step_encoder_forward(self, x, "erp")


class ERPOnlyNet(BaseEEGModel):
    """(cell 13) the ERP-only baseline: ERPEncoder -> AdaptiveAvgPool1d(4) -> Flatten -> Linear-BatchNorm1d-GELU-
    Dropout(0.5)-Linear.  A (B, T, C) batch with T > C is transposed first.  The time bins are averaged before the
    projection (csrc/timepool.hip: the same function, 4 projected rows per sample)."""

    def __init__(self, in_dim: int, erp_out: int = 128, hidden: int = 64, n_classes: int = 2):
        super().__init__()
        self.erp_enc = ERPEncoder(in_channels=in_dim, out_dim=erp_out)
        self.pool = nn.AdaptiveAvgPool1d(4)
        self.head = nn.Sequential(
            nn.Flatten(),
            nn.Linear(erp_out * 4, hidden),
            nn.BatchNorm1d(hidden),
            nn.GELU(),
            nn.Dropout(0.5),
            nn.Linear(hidden, n_classes)
        )

    def forward(self, erp: torch.Tensor, pw: Optional[torch.Tensor] = None,
                return_feats: bool = False) -> torch.Tensor:
        if erp is not None and erp.dim() == 3 and erp.shape[1] > erp.shape[2]:
            erp = erp.permute(0, 2, 1).contiguous()
        return ops.eeg_baseline_forward(self, erp, "erp")


def evaluate_late_fusion(roc_all: Dict) -> Dict:
    """(cell 34, without its printing) per fold, the mean of the ERP-only and power-only class probabilities decides;
    ``roc_all[model][fold] = (y_true, probabilities (n, classes), ...)`` -> the means over the folds of the fused
    accuracy and weighted F1 and of either baseline's own accuracy"""
    from .fmri_utils import classification_metrics
    accs, f1s = [], []
    for erp_fold, pw_fold in zip(roc_all["erponly"], roc_all["pwonly"]):
        y_true = np.asarray(erp_fold[0])
        fused = (np.asarray(erp_fold[1]) + np.asarray(pw_fold[1])) / 2.0
        m = classification_metrics(y_true, np.argmax(fused, axis=1))
        accs.append(m["Accuracy"])
        f1s.append(m["F1"])

    def own(folds):
        return [float(np.mean(np.asarray(f[0]) == np.argmax(np.asarray(f[1]), axis=1))) for f in folds]

    return {"late_fusion_acc": np.mean(accs), "late_fusion_f1": np.mean(f1s),
            "erp_acc": np.mean(own(roc_all["erponly"])), "pw_acc": np.mean(own(roc_all["pwonly"]))}


class EEGTransforms(AS.StepCounter):
    """The notebook's augmenter (cell 18; handed to the training datasets as ``transform=``): with probability ``p``
    Gaussian noise of ``noise_factor * x.std()``, then with probability ``p`` ``max(1, int(0.1 * C))`` random channels
    zeroed.  Same positional signature; ``p_noise`` / ``p_drop`` (default ``p``) and ``drop_fraction`` split what the
    notebook ties together.

    The random stream is this package's own (augment_stream.py), a pure function of (seed, step, rank, sample,
    element): ``batch`` on a device tensor runs the two HIP launches of ``ops.eeg_augment``, on a CPU tensor the same
    stream in numpy - the same decisions and dropped channels, the noise equal to fp32 rounding.  `BridgeTrainer(augment=)`
    augments each training step's EEG batch on the device; ``__call__`` is the per-sample dataset form."""

    def __init__(self, p: float = 0.3, noise_factor: float = 0.05, *, p_noise: Optional[float] = None,
                 p_drop: Optional[float] = None, drop_fraction: float = 0.1, seed: int = 0):
        self.p = p
        self.p_noise = p if p_noise is None else p_noise
        self.p_drop = p if p_drop is None else p_drop
        self.noise_factor, self.drop_fraction, self.seed = noise_factor, drop_fraction, int(seed)
        for name in ("p", "p_noise", "p_drop"):
            v = getattr(self, name)
            if not (isinstance(v, numbers.Real) and 0.0 <= v <= 1.0):
                raise ValueError(f"EEGTransforms: {name} must lie in [0, 1] (got {v!r})")
        if not (isinstance(noise_factor, numbers.Real) and 0.0 <= noise_factor < float("inf")):
            raise ValueError(f"EEGTransforms: noise_factor must be a finite number >= 0 (got {noise_factor!r})")
        if not (isinstance(drop_fraction, numbers.Real) and 0.0 < drop_fraction <= 1.0):
            raise ValueError(f"EEGTransforms: drop_fraction must lie in (0, 1] (got {drop_fraction!r})")

    def n_drop(self, channels: int) -> int:
        return max(1, int(self.drop_fraction * channels))

    def params(self) -> dict:
        """what two augmenters must share to draw the same stream (the trainer's checkpoint carries it)"""
        return {"seed": self.seed, "p_noise": float(self.p_noise), "p_drop": float(self.p_drop),
                "noise_factor": float(self.noise_factor), "drop_fraction": float(self.drop_fraction)}

    def kernel_args(self, channels: int) -> dict:
        return dict(p_noise=float(self.p_noise), p_drop=float(self.p_drop), noise_factor=float(self.noise_factor),
                    n_drop=self.n_drop(channels), seed=self.seed)

    def batch(self, x: torch.Tensor, step: int, rank: int = 0) -> torch.Tensor:
        """the augmented copy of a (B, C, T) batch at step index ``step`` on rank ``rank``"""
        if x.dim() != 3:
            raise ValueError(f"EEGTransforms.batch: expected a (B, C, T) batch, got shape {tuple(x.shape)}")
        if x.is_cuda:
            return ops.eeg_augment(x, step=step, rank=rank, **self.kernel_args(x.shape[1]))
        return self._batch_cpu(x, step, rank)

    def _fields_cpu(self, a: np.ndarray, step: int, rank: int):
        """the draws of a step for the fp32 batch ``a`` (B, C, T), in numpy -> (noise scale fp32 (B,): noise_factor * std_b,
        0 where the noise is off; z fp64 (B, C, T): the unit Gaussian field, None when no sample takes noise; dropped bool
        (B, C))"""
        B, C, T = a.shape
        n_drop = self.n_drop(C)
        s = dict(zip(ops.AUG_PURPOSES, ops.augment_streams(self.seed, step, rank)))
        h = AS.sample_draws("eeg", self.seed, step, rank, B)
        noise_on, drop_on = AS.decide(h["noise_decision"], self.p_noise), AS.decide(h["drop_decision"], self.p_drop)
        scale, z = np.zeros(B, dtype=np.float32), None
        if noise_on.any():
            std = a.astype(np.float64).std(axis=(1, 2), ddof=1).astype(np.float32)
            scale = np.where(noise_on, np.float32(self.noise_factor) * std, np.float32(0)).astype(np.float32)
            half = (T + 1) // 2
            z = AS.gauss_field(s["gauss_a"], s["gauss_b"], 0, B * C * half).reshape(B, C, 2 * half)[:, :, :T]
        dropped = np.zeros((B, C), dtype=bool)
        if drop_on.any():
            keys = AS.aug_hash(s["channel_keys"], np.arange(B * C, dtype=np.uint64)).reshape(B, C)
            order = np.argsort(keys, axis=1, kind="stable")          # ties by channel index
            ranks = np.empty_like(order)
            np.put_along_axis(ranks, order, np.broadcast_to(np.arange(C), (B, C)), axis=1)
            dropped = drop_on[:, None] & (ranks < n_drop)
        return scale, z, dropped

    def _batch_cpu(self, x: torch.Tensor, step: int, rank: int) -> torch.Tensor:
        B, C, T = x.shape
        ops.eeg_augment_check(B, C, T, self.n_drop(C), "EEGTransforms")
        a = x.detach().to(torch.float32).contiguous().numpy()
        scale, z, dropped = self._fields_cpu(a, step, rank)
        out = a.copy()
        if z is not None:
            noisy = (a.astype(np.float64) + z * scale.astype(np.float64)[:, None, None]).astype(np.float32)
            out = np.where((scale != 0)[:, None, None], noisy, a)
        out[dropped] = 0.0
        return torch.from_numpy(np.ascontiguousarray(out)).to(x.dtype)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """the notebook's per-sample form: one (C, ...) sample -> a new tensor (dimension 0 is the channels, as in the
        notebook: a flat feature vector drops single values); the call counter is the step index"""
        if x.dim() < 1:
            raise ValueError(f"EEGTransforms: expected a (channels, ...) sample, got shape {tuple(x.shape)}")
        return self.batch(x.reshape(1, x.shape[0], -1), self.next_step()).reshape(x.shape)


class EEGTimeTransforms(AS.StepCounter):
    """Temporal augmenter of (B, C, T) EEG batches (this package's own; the reference has none - DESIGN.md 5u).  Per sample,
    each with its own probability: an integer time shift ``s`` in ``[-max_shift, max_shift]`` (``out[t] = x[t - s]``,
    zeros where there is no source), an amplitude scale by ``1 + scale_range * (2u - 1)``, a polarity inversion, and one
    window of ``max(1, int(mask_fraction * T))`` samples zeroed on every channel.  A probability of 0 or 1 is valid.

    The random stream is augment_stream.py's on purposes of its own (``ops.eeg_time_augment_streams``), a pure function of
    (seed, step, rank, sample).  ``batch`` on a device tensor is ONE HIP launch (mm_stage_inputs_taug), on a CPU tensor the
    same stream in numpy - the same decisions, shifts, gains and windows.  With ``base=`` an ``EEGTransforms`` its noise
    and channel drop ride in the same launch: the noise is indexed by the output position and scaled by the original
    sample's standard deviation, and an element without a source takes none.  `BridgeTrainer(eeg_time_augment=)`
    augments each training step's EEG batch on the device; ``__call__`` is the per-sample dataset form."""

    def __init__(self, p_shift: float = 0.5, max_shift: int = 16, p_scale: float = 0.3, scale_range: float = 0.1,
                 p_invert: float = 0.0, p_mask: float = 0.3, mask_fraction: float = 0.1, seed: int = 0):
        real = lambda v: isinstance(v, numbers.Real) and not isinstance(v, bool)  # noqa: E731
        for name, v in (("p_shift", p_shift), ("p_scale", p_scale), ("p_invert", p_invert), ("p_mask", p_mask)):
            if not (real(v) and 0.0 <= v <= 1.0):
                raise ValueError(f"EEGTimeTransforms: {name} must lie in [0, 1] (got {v!r})")
        if not (isinstance(max_shift, numbers.Integral) and not isinstance(max_shift, bool) and max_shift >= 0):
            raise ValueError(f"EEGTimeTransforms: max_shift must be an integer >= 0 (got {max_shift!r})")
        if not (real(scale_range) and 0.0 <= scale_range < 1.0):
            raise ValueError(f"EEGTimeTransforms: scale_range must lie in [0, 1) (got {scale_range!r})")
        if not (real(mask_fraction) and 0.0 < mask_fraction <= 1.0):
            raise ValueError(f"EEGTimeTransforms: mask_fraction must lie in (0, 1] (got {mask_fraction!r})")
        self.p_shift, self.p_scale, self.p_invert, self.p_mask = p_shift, p_scale, p_invert, p_mask
        self.max_shift, self.scale_range, self.mask_fraction, self.seed = int(max_shift), scale_range, mask_fraction, int(seed)

    def mask_len(self, T: int) -> int:
        return max(1, int(self.mask_fraction * T))

    def params(self) -> dict:
        """what two augmenters must share to draw the same stream (the trainer's checkpoint carries it)"""
        return {"seed": self.seed, "p_shift": float(self.p_shift), "max_shift": self.max_shift, "p_scale": float(self.p_scale),
                "scale_range": float(self.scale_range), "p_invert": float(self.p_invert), "p_mask": float(self.p_mask),
                "mask_fraction": float(self.mask_fraction)}

    def kernel_args(self, T: int) -> dict:
        """``time_args`` of ``ops.eeg_time_augment`` for epochs of ``T`` samples (which size the masked window)"""
        kw = self.params()
        del kw["mask_fraction"]
        kw["mask_len"] = self.mask_len(T)
        return kw

    def check(self, shape, base: Optional[EEGTransforms] = None, who: str = "EEGTimeTransforms") -> dict:
        """``ops.eeg_time_augment_check`` of a (B, C, T) batch under this augmenter's settings, with ``base`` riding along
        (``ValueError`` before anything runs) -> `kernel_args(T)`"""
        B, C, T = (int(v) for v in shape)
        kw = self.kernel_args(T)
        ops.eeg_time_augment_check(B, C, T, n_drop=None if base is None else base.n_drop(C), who=who,
                                   **{k: v for k, v in kw.items() if k != "seed"})
        return kw

    def batch(self, x: torch.Tensor, step: int, rank: int = 0, base: Optional[EEGTransforms] = None) -> torch.Tensor:
        """the augmented copy of a (B, C, T) batch at step index ``step`` on rank ``rank``; ``base``: an ``EEGTransforms``
        whose noise and channel drop (drawn at the same step index) go into the same pass"""
        if x.dim() != 3:
            raise ValueError(f"EEGTimeTransforms.batch: expected a (B, C, T) batch, got shape {tuple(x.shape)}")
        if base is not None and not isinstance(base, EEGTransforms):
            raise TypeError(f"EEGTimeTransforms.batch: base must be an EEGTransforms (got {type(base).__name__})")
        kw = self.check(x.shape, base)
        if x.is_cuda:
            return ops.eeg_time_augment(x, time_args=kw, base_args=None if base is None else base.kernel_args(x.shape[1]),
                                        step=step, rank=rank).to(x.dtype)
        return self._batch_cpu(x, step, rank, base)

    def draws(self, B: int, T: int, step: int, rank: int = 0) -> dict:
        """the per-sample draws of a step, on the host (numpy; what mm_stage_inputs_taug writes into its time plan):
        {"flags": {shift, scale, invert, mask: bool (B,)}, "shift": int (B,), "gain": fp32 (B,), "mask_start": int (B,),
        "mask_len": int (B,) (0 when off)}"""
        h = AS.sample_draws("eeg_time", self.seed, step, rank, B)
        flags = {k: AS.decide(h[k + "_decision"], getattr(self, "p_" + k)) for k in ops.EEG_TIME_AUG_FLAGS}
        shift = (AS.uniform(h["shift_amount"], 2 * self.max_shift + 1) - self.max_shift) * flags["shift"]
        factor = np.where(flags["scale"], AS.scale_factor(self.scale_range, h["scale_u"]), np.float32(1.0))
        gain = np.where(flags["invert"], -factor, factor).astype(np.float32)
        L = self.mask_len(T)
        return {"flags": flags, "shift": shift, "gain": gain, "mask_start": AS.uniform(h["mask_start"], T - L + 1) * flags["mask"],
                "mask_len": L * flags["mask"].astype(np.int64)}

    def _batch_cpu(self, x: torch.Tensor, step: int, rank: int, base: Optional[EEGTransforms]) -> torch.Tensor:
        B, C, T = x.shape
        a = x.detach().to(torch.float32).contiguous().numpy()
        d = self.draws(B, T, step, rank)
        scale, z, dropped = (np.zeros(B, dtype=np.float32), None, np.zeros((B, C), dtype=bool)) if base is None \
            else base._fields_cpu(a, step, rank)
        out = np.zeros_like(a)
        for b in range(B):
            sh = int(d["shift"][b])
            dst, frm = slice(max(sh, 0), T + min(sh, 0)), slice(max(-sh, 0), T + min(-sh, 0))   # out[t] = x[t - sh]
            v = a[b, :, frm]
            if scale[b] != 0:                                     # the noise field sits at the OUTPUT positions
                v = (v.astype(np.float64) + z[b, :, dst] * float(scale[b])).astype(np.float32)
            if d["flags"]["scale"][b] or d["flags"]["invert"][b]:
                v = v * d["gain"][b]                              # (one fp32 product)
            out[b, :, dst] = v
            out[b, dropped[b], :] = 0.0
            out[b, :, int(d["mask_start"][b]):int(d["mask_start"][b]) + int(d["mask_len"][b])] = 0.0
        return torch.from_numpy(np.ascontiguousarray(out)).to(x.dtype)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """the per-sample dataset form: one (C, T) epoch -> a new tensor; the call counter is the step index"""
        if x.dim() != 2:
            raise ValueError(f"EEGTimeTransforms: expected a (C, T) sample, got shape {tuple(x.shape)}")
        return self.batch(x.reshape(1, *x.shape), self.next_step()).reshape(x.shape)


def _channels_first(x):
    """(B, T, C) with T > C -> (B, C, T): the notebook's orientation fix for ERP / power inputs."""
    if x is not None and x.dim() == 3 and x.shape[1] > x.shape[2]:
        return x.transpose(1, 2)
    return x


def collate_trimodal(batch):
    """(cell 24) 5-tuples (erp, pw, conn, subject, y) or 4-tuples (erp, pw, subject, y)."""
    n = len(batch[0])
    if n not in (4, 5):
        raise ValueError(f"Unexpected batch element length: {n}")
    cols = list(zip(*batch))
    erps, pws = _channels_first(torch.stack(cols[0])), _channels_first(torch.stack(cols[1]))
    conns = torch.stack(cols[2]) if n == 5 else None
    return (erps, pws, conns, torch.tensor(cols[-2], dtype=torch.long), torch.tensor(cols[-1], dtype=torch.long))


class _PlateauLR:
    """``ReduceLROnPlateau(mode='min', factor, patience)`` with torch's defaults (rel threshold 1e-4, no
    cooldown, min_lr 0, eps 1e-8) over a FusedAdamW, with the same ``state_dict`` field names."""

    def __init__(self, optimizer, factor=0.5, patience=5, threshold=1e-4, eps=1e-8):
        self.optimizer, self.factor, self.patience, self.threshold, self.eps = optimizer, factor, patience, threshold, eps
        self.best, self.num_bad_epochs, self.last_epoch = float("inf"), 0, 0

    def step(self, metric):
        metric = float(metric)
        self.last_epoch += 1
        if metric < self.best * (1.0 - self.threshold):
            self.best, self.num_bad_epochs = metric, 0
        else:
            self.num_bad_epochs += 1
        if self.num_bad_epochs > self.patience:
            for g in self.optimizer.param_groups:
                new = g["lr"] * self.factor
                if g["lr"] - new > self.eps:
                    g["lr"] = new
            self.num_bad_epochs = 0

    def state_dict(self):
        return {"factor": self.factor, "patience": self.patience, "threshold": self.threshold, "eps": self.eps,
                "best": self.best, "num_bad_epochs": self.num_bad_epochs, "last_epoch": self.last_epoch,
                "mode": "min", "threshold_mode": "rel", "cooldown": 0, "cooldown_counter": 0, "min_lrs": [0.0]}

    def load_state_dict(self, sd):
        for k in ("factor", "patience", "threshold", "eps", "best", "num_bad_epochs", "last_epoch"):
            if k in sd:
                setattr(self, k, sd[k])


class FlexibleTrainer:
    """(cell 23) one model + criterion + AdamW + ReduceLROnPlateau(0.5, 5); ``modality`` selects how a
    batch is unpacked and which inputs the model receives."""

    def __init__(self, model: nn.Module, device: Optional[torch.device] = None, lr: float = 1e-5,
                 weight_decay: float = 1e-5, modality: str = "fusion", class_weights: Optional[torch.Tensor] = None,
                 use_focal_loss: bool = False, logger: Optional[logging.Logger] = None):
        self.device = device or torch.device("cuda")
        self.model = model.to(self.device)
        self.modality = modality
        self.logger = logger or logging.getLogger(__name__)
        if use_focal_loss:
            self.criterion = FocalLoss(alpha=0.25, gamma=2.0)
        else:
            self.criterion = WeightedCrossEntropy(None if class_weights is None else class_weights.to(self.device))
            self.criterion.to(self.device)
        self.opt = FusedAdamW(self.model.parameters(), lr=lr, weight_decay=weight_decay)
        self.scheduler = _PlateauLR(self.opt, factor=0.5, patience=5)
        self.fusion_weights_history = []

    def _forward_model(self, erp=None, pw=None, conn=None):
        if self.modality == "trimodal":
            return self.model(erp=erp, pw=pw, conn=conn)
        if self.modality == "fusion":
            return self.model(erp=erp, pw=pw)
        if self.modality == "erponly":
            return self.model(erp=erp)
        if self.modality == "pwonly":
            return self.model(pw=pw)
        raise ValueError(f"Unknown modality: {self.modality}")

    def _unpack_batch(self, batch):
        if len(batch) == 5:
            erp, pw, conn, subj, y = batch
        elif len(batch) == 4:
            (erp, pw, subj, y), conn = batch, None
        elif len(batch) == 3:
            if self.modality == "erponly":
                (erp, subj, y), pw, conn = batch, None, None
            else:
                (pw, subj, y), erp, conn = batch, None, None
        else:
            raise ValueError(f"Batch format mismatch. Got length {len(batch)}")
        return _channels_first(erp), _channels_first(pw), conn, subj, y

    def _to_device(self, *xs):
        return [x.to(self.device) if x is not None else None for x in xs]

    def _logits(self, erp, pw, conn, return_feats):
        if isinstance(self.model, ImprovedTriModalFusionNet):
            return self.model(erp=erp, pw=pw, conn=conn, return_feats=return_feats)
        if isinstance(self.model, ImprovedSmartFusionNet):
            return self.model(erp=erp, pw=pw, return_feats=return_feats)
        return self._forward_model(erp, pw, conn)

    def train_one_epoch(self, loader, grad_clip=None):
        self.model.train()
        self.opt.max_grad_norm = float(grad_clip) if grad_clip else 0.0
        total, n = 0.0, 0
        for batch in loader:
            erp, pw, conn, _, y = self._unpack_batch(batch)
            erp, pw, conn = self._to_device(erp, pw, conn)
            self.opt.zero_grad()
            loss = self.criterion(self._logits(erp, pw, conn, False), y.to(self.device).long())
            loss.backward()
            self.opt.step()
            total += loss.item()
            n += 1
        return total / max(n, 1)

    @torch.no_grad()
    def evaluate(self, loader, n_classes: int):
        from .fmri_utils import classification_metrics
        self.model.eval()
        preds, targets, probs, gates, feats, subjects = [], [], [], [], [], []
        for batch in loader:
            erp, pw, conn, subj, y = self._unpack_batch(batch)
            erp, pw, conn = self._to_device(erp, pw, conn)
            out = self._logits(erp, pw, conn, True)
            if isinstance(out, dict):
                logits = out["logits"]
                if out.get("gates") is not None:
                    gates.append(out["gates"].float().cpu().numpy())
                if out.get("fused_feats") is not None:
                    feats.append(out["fused_feats"].float().cpu().numpy())
            else:
                logits = out
            p = torch.softmax(logits.float(), dim=1).cpu().numpy()
            probs.extend(p)
            preds.extend(np.argmax(p, axis=1))
            targets.extend(y.cpu().numpy())
            subjects.extend(subj.cpu().numpy())
        targets, preds = np.array(targets), np.array(preds)
        probs = np.array(probs) if len(probs) else np.zeros((len(preds), n_classes))
        metrics = classification_metrics(targets, preds) if len(targets) else \
            {"Accuracy": 0.0, "F1": 0.0, "Precision": 0.0, "Recall": 0.0}
        return metrics, targets, probs, feats, gates, subjects

    def track_fusion_weights(self):
        if hasattr(self.model, "get_fusion_weights"):
            self.fusion_weights_history.append(self.model.get_fusion_weights())

    def get_fusion_weights(self):
        return self.model.get_fusion_weights() if hasattr(self.model, "get_fusion_weights") else None

    def save_checkpoint(self, path: str, epoch: int, metrics: Dict):
        torch.save({"epoch": epoch, "model_state_dict": self.model.state_dict(),
                    "optimizer_state_dict": self.opt.state_dict(),
                    "scheduler_state_dict": self.scheduler.state_dict(), "metrics": metrics}, path)
        self.logger.info("Checkpoint saved to %s", path)

    def load_checkpoint(self, path: str):
        ck = torch.load(path, map_location=self.device, weights_only=False)
        self.model.load_state_dict(ck["model_state_dict"])
        ops.weights_changed()
        self.opt.load_state_dict(ck["optimizer_state_dict"])
        self.scheduler.load_state_dict(ck["scheduler_state_dict"])
        self.logger.info("Checkpoint loaded from %s", path)
        return ck["epoch"], ck["metrics"]


class InterpretabilityAnalyzer:
    """The notebook's ``InterpretabilityAnalyzer`` (cell "ADVANCED INTERPRETABILITY") on the batched perturbation engine
    (`ops.perturb_scores`, csrc/perturb.hip).  The model is called as the notebook calls it,
    ``model(erp, pw[, conn])``; the score of a sample is ``softmax(logits)[target_class]``, the softmax taken by torch.
    The notebook runs one clone and one forward per zeroed channel and fetches every mean with ``.item()``; here the
    zeroed copies of a batch are rows of a few large batches and one tensor per batch goes to the host.
    ``chunk_masks`` (attribute): masks per forward; None = the engine's memory rule.  ``compute_shap`` (shap's
    DeepExplainer) is not ported."""

    def __init__(self, model, device, channel_names=None):
        self.model = model.eval().to(device)
        self.device = device
        self.channels = channel_names or [f"Ch{i}" for i in range(18)]
        self.chunk_masks = None

    def _forward_func(self, *inputs):
        if len(inputs) == 3:
            return self.model(inputs[0], inputs[1], inputs[2])
        return self.model(inputs[0], inputs[1])

    def _to_device(self, erp, pw, conn):
        put = lambda t: None if t is None else t.detach().to(self.device).float().contiguous()      # noqa: E731
        return put(erp), put(pw), put(conn)

    def _target(self, target_class, B: int) -> torch.Tensor:
        """(B,) int64 on the device: one class for every row, or one class per row"""
        if isinstance(target_class, torch.Tensor):
            t = target_class.detach().to(self.device).long().reshape(-1)
            if t.numel() == 1:
                t = t.expand(B)
            if t.numel() != B:
                raise ValueError(f"target_class: {t.numel()} classes for {B} rows")
            return t.contiguous()
        return torch.full((B,), int(target_class), dtype=torch.long, device=self.device)

    def _games(self, erp, pw, conn, target, baseline: str, masks_of):
        """-> (p_full (B,), {"erp": (M_e, B), "pw": (M_p, B)}): the class probability at the inputs and under every mask
        ``masks_of(C)`` of each modality's channels, the other modality (and conn) intact"""
        if baseline not in ("zero", "mean"):
            raise ValueError(f"baseline must be 'zero' or 'mean', got {baseline!r}")
        self.model.eval()
        B = erp.shape[0]

        def prob(e, p, c):
            k = e.shape[0] // B
            logits = self._forward_func(e, p, c) if c is not None else self._forward_func(e, p)
            return torch.softmax(logits.float(), dim=1).gather(1, target.repeat(k).unsqueeze(1)).squeeze(1)

        def tiled(t, rows):                                       # the intact inputs, once per mask of the chunk
            return None if t is None else t.repeat((rows.shape[0] // B,) + (1,) * (t.dim() - 1))
        with torch.no_grad():
            full = prob(erp, pw, conn)
            scores = {}
            for name, x in (("erp", erp), ("pw", pw)):
                if x.dim() != 3:
                    raise ValueError(f"{name}: expected (B, C, T), got {tuple(x.shape)}")
                base = x.mean(dim=0, keepdim=True) if baseline == "mean" else None
                if name == "erp":
                    rows_fn = lambda rows: prob(rows, tiled(pw, rows), tiled(conn, rows))      # noqa: E731
                else:
                    rows_fn = lambda rows: prob(tiled(erp, rows), rows, tiled(conn, rows))     # noqa: E731
                scores[name] = ops.perturb_scores(rows_fn, x, base, masks_of(name, x.shape[1]), ("rows", 1), self.chunk_masks)
        return full, scores

    def channel_drops(self, erp, pw, conn=None, target_class=1, baseline="zero"):
        """-> {"erp": (B, C_e), "pw": (B, C_p)} fp32 on the device: per sample, the probability of ``target_class`` (an
        int, or a tensor of one class per row) at the inputs minus the same with ONE channel replaced by the baseline
        ("zero", or "mean" = the batch mean) - the notebook's quantity before its mean over the batch."""
        erp, pw, conn = self._to_device(erp, pw, conn)
        target = self._target(target_class, erp.shape[0])
        full, s = self._games(erp, pw, conn, target, baseline, lambda name, C: 1 - torch.eye(C, dtype=torch.int32))
        return {k: (full.unsqueeze(0) - v).t().contiguous() for k, v in s.items()}

    def compute_channel_importance(self, dataloader):
        """Measure importance of each channel by zeroing it out -> (importance_erp, importance_pw), numpy arrays of
        ``len(channel_names)`` values.  Batches of 5 items are (erp, pw, conn, subjects, labels), any other batch is
        (erp, pw, subjects, labels).  The notebook's arithmetic, kept to the letter: per batch the MEAN over the batch of
        ``softmax(logits)[:, 1]`` at the input minus the same with one channel zeroed is added up, for every ERP and
        every PW channel, and at the end the sum of those batch means is divided by the number of SAMPLES, not of
        batches - so the result scales with 1 / batch size.  That is what the notebook computes.  `channel_drops` has
        the per-sample drops without that division."""
        importance_erp = np.zeros(len(self.channels))
        importance_pw = np.zeros(len(self.channels))
        n_samples = 0
        for batch in dataloader:
            if len(batch) == 5:
                erp, pw, conn = batch[0], batch[1], batch[2]
            else:
                erp, pw, conn = batch[0], batch[1], None
            if max(erp.shape[1], pw.shape[1]) > len(self.channels):
                raise ValueError(f"{max(erp.shape[1], pw.shape[1])} channels but {len(self.channels)} channel names")
            drops = self.channel_drops(erp, pw, conn, target_class=1, baseline="zero")
            means = torch.cat([drops["erp"].mean(dim=0), drops["pw"].mean(dim=0)]).cpu().numpy()      # one transfer per batch
            importance_erp[:erp.shape[1]] += means[:erp.shape[1]]
            importance_pw[:pw.shape[1]] += means[erp.shape[1]:]
            n_samples += erp.shape[0]
        return importance_erp / n_samples, importance_pw / n_samples

    def compute_channel_shapley(self, erp, pw, conn=None, target_class=1, n_permutations=16, seed=0, baseline="zero"):
        """Permutation-sampled Shapley values of the channels -> {"erp": (B, C_e), "pw": (B, C_p)} fp32 on the device.
        TWO games, not one joint game: the players of the first are the ERP channels with PW (and conn) intact, those of
        the second the PW channels with ERP intact; a coalition's value is the probability of ``target_class`` with the
        channels outside it replaced by the baseline.  Per modality sum_c phi[b][c] = p(inputs) - p(all its channels
        replaced) up to rounding.  ``n_permutations`` permutations per game from ``torch.randperm`` on a CPU generator
        seeded with ``seed`` (ERP drawn first; all samples share them); P (C - 1) + 2 evaluations per game."""
        if n_permutations < 1:
            raise ValueError("n_permutations must be >= 1")
        erp, pw, conn = self._to_device(erp, pw, conn)
        target = self._target(target_class, erp.shape[0])
        gen = torch.Generator().manual_seed(int(seed))
        pos = {}

        def masks_of(name, C):
            perm = torch.stack([torch.randperm(C, generator=gen) for _ in range(int(n_permutations))])
            prefix, pos[name] = ops.shapley_masks(perm)
            return torch.cat([torch.zeros(1, C, dtype=torch.int32), prefix])             # the empty coalition first
        full, s = self._games(erp, pw, conn, target, baseline, masks_of)
        return {k: ops.perturb_shapley(v[1:] if v.shape[0] > 1 else None, v[0].clone(), full, pos[k]) for k, v in s.items()}

    def compute_integrated_gradients(self, erp, pw, conn=None, target_class=1, steps=50):
        """-> (attr_erp, attr_pw[, attr_conn]) numpy arrays from `eeg_xai_analysis.IntegratedGradients` with ``steps``
        points and the zero baseline, the model called (erp, pw[, conn]) as everywhere in this class.  These are the
        ABSOLUTE values |(x - baseline) * mean_s grad| on ``np.linspace(0, 1, steps)``, that module's convention - NOT what
        the notebook's captum call returns (signed attributions at Gauss-Legendre points); captum is not a dependency
        (DESIGN.md section 7)."""
        from .eeg_xai_analysis import IntegratedGradients
        # that class calls model(pw, erp[, conn]): handing it (erp=pw, pw=erp) makes the call model(erp, pw[, conn])
        out = IntegratedGradients(self.model, self.device, n_steps=steps).compute(pw, erp, conn, target_class=target_class)
        return (out["pw"], out["erp"]) + ((out["conn"],) if conn is not None else ())
