"""The reference's fMRI notebook (``fMRI_CODE/CrossModal_fmri_scr.ipynb``) on the MI355X HIP path: its transformer
encoders and the three models built on them (cells "# ENCODER BLOCKS", "class fMRIActivationOnly", "# FUSION MODEL"),
``fMRISubjectDataHandler`` and ``run_fmri_loso_evaluation`` (leave-one-subject-out), and the notebook's k-fold
``run_experiment``.

These classes share their NAMES with the MLP family of ``fmri_utils.py`` (== ``run_fmri_v11.py``) and differ in
signature and ``state_dict``: ``ActivationEncoder(num_layers, in_dim, hidden_dim, dropout)`` here is
``Linear(in_dim -> H)``, an ``nn.TransformerEncoder`` of post-norm layers (nhead 4, dim_feedforward 4H) on a sequence
of length ONE, and ``LayerNorm(H)``; ``fMRIFusionNet`` adds ``cross_attn``.  This is the model behind the fMRI numbers
BASELINE.md quotes.  The ``nn.TransformerEncoder`` / ``nn.MultiheadAttention`` modules are parameter CONTAINERS only, so
that a notebook checkpoint loads strictly (73 tensors for the fusion net at two layers); ``forward`` never calls them.
Both encoders of a fusion net run as ONE forward launch and TWO backward launches (csrc/fmri_tx.hip, DESIGN.md
section 5n); the rest is composed from the small fp32 kernels (``small_autograd``).

With one key the attention softmax is identically 1, so a layer's query / key rows of ``in_proj`` (and ``cross_attn``'s)
never reach the output; their gradients are written as exact zeros.
"""
from __future__ import annotations

import logging

import numpy as np
import torch
import torch.nn as nn

from . import fmri_utils as FU
from . import ops
from .fmri_utils import (SEED, collate_fmri, evaluate, fMRIDataset, load_activation_features,   # noqa: F401
                         load_connectivity_features, train_epoch)

logger = logging.getLogger(__name__)


class ActivationEncoder(nn.Module):
    """(B, in_dim) -> (B, hidden_dim); ``hidden_dim`` in {32, 64, 128}, 1 <= ``num_layers`` <= 8, any ``in_dim`` >= 1.
    ``state_dict``: ``project.*``, ``transformer.layers.<i>.*`` (12 tensors a layer), ``norm.*`` as in the notebook."""

    def __init__(self, num_layers, in_dim, hidden_dim, dropout):
        super().__init__()
        ops.tab_tx_check(hidden_dim, num_layers, [in_dim], dropout, who=type(self).__name__)
        self.project = nn.Linear(in_dim, hidden_dim)
        encoder_layer = nn.TransformerEncoderLayer(d_model=hidden_dim, nhead=4, dim_feedforward=hidden_dim * 4,
                                                   dropout=dropout, batch_first=True)
        self.transformer = nn.TransformerEncoder(encoder_layer, num_layers=num_layers)
        self.norm = nn.LayerNorm(hidden_dim)
        self.in_dim, self.hidden_dim, self.num_layers, self.drop_p = int(in_dim), int(hidden_dim), int(num_layers), float(dropout)

    def forward(self, x):
        from . import small_autograd as sa
        return sa.tab_tx([self], [x], self.training)[0]


class ConnectivityEncoder(ActivationEncoder):
    pass


def _head(hidden_dim, dropout, out_dim):
    return nn.Sequential(nn.Linear(hidden_dim, hidden_dim // 2), nn.ReLU(), nn.Dropout(dropout), nn.Linear(hidden_dim // 2, out_dim))


def _run_head(m, feat):
    from . import small_autograd as sa
    p = m.drop_p if m.training else 0.0
    output = sa.linear(sa.linear(feat, m.head[0], "relu", p), m.head[3])
    return output.squeeze(-1) if m.task == "regression" else output


class _SingleBranch(nn.Module):
    _encoder_cls = ActivationEncoder

    def __init__(self, in_dim: int, hidden_dim: int = 64, num_classes: int = 2, dropout: float = 0.4,
                 task: str = "classification", num_layers: int = 2):
        super().__init__()
        if task not in ("classification", "regression"):
            raise ValueError(f"{type(self).__name__}: task must be 'classification' or 'regression', got {task!r}")
        self.task = task
        self.encoder = self._encoder_cls(num_layers, in_dim, hidden_dim, dropout)
        self.head = _head(hidden_dim, dropout, num_classes if task == "classification" else 1)
        self.drop_p = float(dropout)


class fMRIActivationOnly(_SingleBranch):
    """activation features only; ``connectivity`` is accepted and ignored, so the three models share the epoch loops"""

    def forward(self, activation, connectivity=None):
        return _run_head(self, self.encoder(activation))


class fMRIConnectivityOnly(_SingleBranch):
    """connectivity features only; with ``connectivity`` None the first argument is encoded (the notebook's rule for a
    caller that passes the features positionally)"""
    _encoder_cls = ConnectivityEncoder

    def forward(self, activation=None, connectivity=None):
        x = activation if connectivity is None and activation is not None else connectivity
        return _run_head(self, self.encoder(x))


class fMRIFusionNet(nn.Module):
    """both encoders (one launch), cross attention with query = activation feature and key = value = connectivity feature
    (one key: the output is out_proj(dropout_head(Wv c + bv)), whatever the query), the softmax-weighted concat
    [w_a * act | w_c * attended], ``fusion`` Linear-BatchNorm1d-ReLU-Dropout and ``head``."""

    def __init__(self, activation_dim: int, connectivity_dim: int, hidden_dim: int = 64, num_classes: int = 2,
                 dropout: float = 0.3, num_transformer_layers: int = 2, num_heads: int = 4, task: str = "classification"):
        super().__init__()
        if task not in ("classification", "regression"):
            raise ValueError(f"fMRIFusionNet: task must be 'classification' or 'regression', got {task!r}")
        if num_heads < 1 or num_heads > 16 or hidden_dim % num_heads:
            raise ValueError(f"fMRIFusionNet: num_heads must divide hidden_dim and be at most 16, got {num_heads}")
        self.task = task
        self.activation_encoder = ActivationEncoder(num_transformer_layers, activation_dim, hidden_dim, dropout)
        self.connectivity_encoder = ConnectivityEncoder(num_transformer_layers, connectivity_dim, hidden_dim, dropout)
        self.cross_attn = nn.MultiheadAttention(hidden_dim, num_heads=num_heads, dropout=dropout, batch_first=True)
        self.fusion = nn.Sequential(nn.Linear(hidden_dim * 2, hidden_dim), nn.BatchNorm1d(hidden_dim), nn.ReLU(), nn.Dropout(dropout))
        self.activation_weight = nn.Parameter(torch.ones(1) * 0.5)
        self.connectivity_weight = nn.Parameter(torch.ones(1) * 0.5)
        self.head = _head(hidden_dim, dropout, num_classes if task == "classification" else 1)
        self.drop_p = float(dropout)

    def forward(self, activation, connectivity, return_features=False):
        from . import small_autograd as sa
        tr = self.training
        if tr and activation.shape[0] < 2:
            raise ValueError(f"fMRIFusionNet: train mode (BatchNorm1d batch statistics) takes B >= 2 rows, got {activation.shape[0]}")
        p = self.drop_p if tr else 0.0
        act_feat, conn_feat = sa.tab_tx([self.activation_encoder, self.connectivity_encoder], [activation, connectivity], tr)
        attn_out, _ = sa.mha_1xk(self.cross_attn, [conn_feat], tr)
        combined = sa.Softmax2ConcatFn.apply(act_feat, attn_out, self.activation_weight, self.connectivity_weight)
        fused = sa.linear_bn_act(combined, self.fusion[0], self.fusion[1], "relu", p, frozen=not tr)
        output = _run_head(self, fused)
        return (output, fused) if return_features else output

    get_fusion_weights = FU.fMRIFusionNet.get_fusion_weights


MODEL_CLASSES = {"fusion": fMRIFusionNet, "activation_only": fMRIActivationOnly, "connectivity_only": fMRIConnectivityOnly}


def load_labels(label_path, subject_list, binary: bool = True):
    """({subject: class label}, {subject: score} or None) from the first of labels.csv / outcomes.csv /
    subjects_labels.csv / ../labels.csv that exists (notebook cell "DATA LOADING"); the score column is one of Score /
    Value / Continuous.  No label file: random dummy labels, as there."""
    import pandas as pd
    from pathlib import Path
    label_path = Path(label_path)
    candidates = [label_path / "labels.csv", label_path / "outcomes.csv", label_path / "subjects_labels.csv",
                  label_path.parent / "labels.csv"]
    label_file = next((f for f in candidates if f.exists()), None)
    if label_file is None:
        logger.warning("No fMRI label file found. Using dummy labels.")
        return ({s: int(np.random.randint(0, 2)) for s in subject_list}, {s: float(np.random.randn()) for s in subject_list})
    df = pd.read_csv(label_file)
    subj_col = next((c for c in FU._SUBJECT_COLS + ("subject_id",) if c in df.columns), None)
    label_col = next((c for c in FU._LABEL_COLS if c in df.columns), None)
    reg_col = next((c for c in ("Score", "score", "Value", "value", "Continuous", "continuous") if c in df.columns), None)
    if not subj_col or not label_col:
        raise ValueError(f"Could not identify subject or label columns in {label_file}: {df.columns.tolist()}")
    wanted = set(subject_list)
    class_labels, reg_labels = {}, {}
    for _, row in df.iterrows():
        subj = int(row[subj_col])
        if subj not in wanted:
            continue
        label = row[label_col]
        if binary:
            label = (1 if label.lower() in ("good", "positive", "yes", "1") else 0) if isinstance(label, str) else int(label)
        class_labels[subj] = label
        if reg_col:
            reg_labels[subj] = float(row[reg_col])
    return class_labels, (reg_labels or None)


class fMRISubjectDataHandler:
    """label loading, feature aggregation and per-subject splits for the leave-one-subject-out evaluation (notebook cell
    "fMRI SUBJECT DATA HANDLER").  ``config``: an ``fmri_utils.fMRIConfig``-like attribute bag."""

    def __init__(self, config):
        self.config = config
        self.activation_features, self.connectivity_features = {}, {}
        self.class_labels, self.reg_labels = {}, {}
        self.subject_ids, self.subject_labels = [], {}

    def load_all(self):
        c = self.config
        self.activation_features = load_activation_features(c.data_dir, c.subject_list, activation_types=c.activation_types,
                                                            agg_method=c.agg_method)
        self.connectivity_features = load_connectivity_features(c.data_dir, c.subject_list, connectivity_types=c.connectivity_types)
        self.class_labels, self.reg_labels = load_labels(c.label_path, c.subject_list)
        common = set(self.activation_features) & set(self.connectivity_features) & set(self.class_labels)
        self.subject_ids = sorted(common)
        self.subject_labels = {s: self.class_labels[s] for s in self.subject_ids}
        logger.info("fMRISubjectDataHandler: %d subjects with complete data", len(self.subject_ids))

    def build_dataset(self):
        return fMRIDataset(self.activation_features, self.connectivity_features, self.class_labels, self.reg_labels)

    def get_subject_ids_and_labels(self):
        return np.array(self.subject_ids), np.array([self.subject_labels[s] for s in self.subject_ids])

    def get_subject_split_indices(self, dataset, held_out_subjects):
        """(train indices, test indices) of ``dataset.samples`` for a held-out set of subjects"""
        held = set(int(s) for s in held_out_subjects)
        train_idx = [i for i, s in enumerate(dataset.samples) if int(s["subject"]) not in held]
        test_idx = [i for i, s in enumerate(dataset.samples) if int(s["subject"]) in held]
        return train_idx, test_idx


def subject_vote(y_pred) -> int:
    """the subject-level label of the notebook: ``int(np.round(np.mean(y_pred)))`` - numpy rounds half to even, so a 1:1
    tie between classes 0 and 1 votes 0"""
    return int(np.round(np.mean(y_pred)))


LOSO_COLUMNS = ["subject_id", "true_label", "predicted_label", "confidence", "n_samples", "sample_accuracy", "correct"]


def _make_model(model_name, activation_dim, connectivity_dim, num_classes, config, task):
    if model_name not in MODEL_CLASSES:
        raise ValueError(f"Unknown model_name: {model_name}")
    kw = dict(hidden_dim=config.hidden_dim, num_classes=num_classes, dropout=config.dropout, task=task)
    if model_name == "fusion":
        return fMRIFusionNet(activation_dim=activation_dim, connectivity_dim=connectivity_dim, **kw)
    return MODEL_CLASSES[model_name](in_dim=activation_dim if model_name == "activation_only" else connectivity_dim, **kw)


def run_fmri_loso_evaluation(handler: fMRISubjectDataHandler, config, model_name: str = "fusion",
                             task: str = "classification", device=None, verbose: bool = True):
    """Leave-one-subject-out (notebook cell "LEAVE-ONE-SUBJECT-OUT EVALUATION"): for every subject a fresh model is
    trained on the others with AdamW + ReduceLROnPlateau(0.5, 5) on the TRAINING loss, the best-training-loss state is
    restored (early stop after ``config.patience`` epochs without improvement) and the held-out subject is scored.
    Returns a DataFrame with one row per subject (`LOSO_COLUMNS`).  The optimizer is ``optim.FusedAdamW``."""
    import copy
    import pandas as pd
    from sklearn.metrics import accuracy_score
    from sklearn.utils.class_weight import compute_class_weight
    from torch.utils.data import DataLoader, Subset
    from .bridge_utils import WeightedCrossEntropy
    from .crossmodal_eeg_scr import _PlateauLR
    from .optim import FusedAdamW
    say = print if verbose else (lambda *a, **k: None)
    device = device or torch.device("cuda")
    dataset = handler.build_dataset()
    subj_ids, _ = handler.get_subject_ids_and_labels()
    sample = dataset[0]
    activation_dim, connectivity_dim = sample[0].shape[0], sample[1].shape[0]
    num_classes = len(np.unique(np.array([s["class_label"] for s in dataset.samples])))
    rows = []
    for fold_idx, held_out in enumerate(subj_ids, 1):
        train_idx, test_idx = handler.get_subject_split_indices(dataset, [held_out])
        if not test_idx:
            continue
        train_loader = DataLoader(Subset(dataset, train_idx), batch_size=config.batch_size, shuffle=True, collate_fn=collate_fmri)
        test_loader = DataLoader(Subset(dataset, test_idx), batch_size=config.batch_size, shuffle=False, collate_fn=collate_fmri)
        if task == "classification":
            y_train = np.array([dataset.samples[i]["class_label"] for i in train_idx])
            cw = compute_class_weight("balanced", classes=np.unique(y_train), y=y_train)
            criterion = WeightedCrossEntropy(torch.tensor(cw, dtype=torch.float32)).to(device)
        else:
            criterion = nn.MSELoss()
        model = _make_model(model_name, activation_dim, connectivity_dim, num_classes, config, task).to(device)
        optimizer = FusedAdamW(model.parameters(), lr=config.learning_rate, weight_decay=config.weight_decay)
        scheduler = _PlateauLR(optimizer, factor=0.5, patience=5)
        best_loss, best_state, patience_counter = float("inf"), None, 0
        for epoch in range(1, config.num_epochs + 1):
            train_loss = train_epoch(model, train_loader, optimizer, criterion, device, task, config.grad_clip)
            scheduler.step(train_loss)
            if train_loss < best_loss:
                best_loss, best_state, patience_counter = train_loss, copy.deepcopy(model.state_dict()), 0
            else:
                patience_counter += 1
            if patience_counter >= config.patience:
                break
        if best_state:
            model.load_state_dict(best_state)
            ops.weights_changed()
        _, y_true, y_out = evaluate(model, test_loader, device, task, num_classes)
        true_label = int(handler.subject_labels[held_out])
        if task == "classification":
            y_probs = np.array(y_out)
            y_pred = np.argmax(y_probs, axis=1)
            sample_acc = accuracy_score(np.array(y_true), y_pred)
            pred_label = subject_vote(y_pred)
            confidence = float(np.mean(y_probs[:, pred_label]))
        else:
            sample_acc, pred_label, confidence = 0.0, float(np.mean(np.array(y_out))), 0.0
        rows.append({"subject_id": int(held_out), "true_label": true_label, "predicted_label": pred_label,
                     "confidence": confidence, "n_samples": len(y_true), "sample_accuracy": sample_acc,
                     "correct": int(true_label == pred_label)})
        say(f"LOSO {fold_idx}/{len(subj_ids)} sub-{held_out}: true={true_label}, pred={pred_label}, conf={confidence:.3f}")
    df = pd.DataFrame(rows, columns=LOSO_COLUMNS)
    if len(df) and task == "classification":
        say(f"LOSO subject-level accuracy: {accuracy_score(df['true_label'], df['predicted_label']):.4f} over {len(df)} subjects")
    return df


def run_experiment(dataset, config, task="classification", **kwargs):
    """the notebook's k-fold protocol (cell "MAIN EXPERIMENT": the same loop as ``fmri_utils.run_experiment``) with the
    three transformer models of this module -> (results, fusion_weights_all)"""
    return FU.run_experiment(dataset, config, task, model_classes=MODEL_CLASSES, **kwargs)
