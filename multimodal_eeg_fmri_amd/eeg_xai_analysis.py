"""Attribution for the EEG fusion classifiers on the HIP path (the reference's EEG_CODE/eeg_xai_analysis.py).

Same classes, constructors, method signatures and result dictionaries as the reference module:
``GradientSaliency``, ``IntegratedGradients``, ``SHAPExplainer``, ``ChannelImportanceExtractor``, ``EEGExplainer``
and the channel-name / brain-region tables.  Every model call - forward and backward - runs in the HIP kernels;
integrated gradients goes through ``ops.integrated_gradients``: the interpolation steps as batches of S_c * B rows
instead of one forward/backward and one numpy round trip per step.  Results are numpy arrays of the input shapes.
The plotting helpers and the report writer are not part of this package.

Reference behaviour kept on purpose:
* the model is called as ``model(pw, erp[, conn])`` - power first;
* with ``target_class=None`` integrated gradients attributes the class predicted at its FIRST interpolation step,
  alpha = 0, i.e. at the baseline;
* ``conn`` is not interpolated; its attribution is ``|conn * mean over steps of d logit / d conn|``;
* the ``'mean'`` baseline is the mean over the batch given to ``compute``.
"""
from __future__ import annotations

import warnings
from collections import defaultdict
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import ops

# ------------------------------------------------------------------ channel tables (10-20 / 10-10 systems)
STANDARD_10_20_19 = ["Fp1", "Fp2", "F7", "F3", "Fz", "F4", "F8", "T3", "C3", "Cz", "C4", "T4", "T5", "P3", "Pz", "P4", "T6",
                     "O1", "O2"]
STANDARD_10_20_21 = STANDARD_10_20_19 + ["A1", "A2"]
EXTENDED_10_10_32 = ["Fp1", "Fp2", "F7", "F3", "Fz", "F4", "F8", "FC5", "FC1", "FC2", "FC6", "T7", "C3", "Cz", "C4", "T8",
                     "CP5", "CP1", "CP2", "CP6", "P7", "P3", "Pz", "P4", "P8", "PO3", "PO4", "O1", "Oz", "O2", "AF3", "AF4"]
BRAIN_REGIONS = {
    "Frontal": ["Fp1", "Fp2", "Fpz", "F7", "F3", "Fz", "F4", "F8", "AF3", "AF4"],
    "Central": ["C3", "Cz", "C4", "FC1", "FC2", "FC5", "FC6"],
    "Temporal": ["T3", "T4", "T5", "T6", "T7", "T8", "P7", "P8"],
    "Parietal": ["P3", "Pz", "P4", "CP1", "CP2", "CP5", "CP6"],
    "Occipital": ["O1", "Oz", "O2", "PO3", "PO4"],
}


def _default_device(device):
    return device or torch.device("cuda" if torch.cuda.is_available() else "cpu")


def _target_seed(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """one-hot rows: the gradient ``logits.backward`` starts from in the reference"""
    return torch.zeros_like(logits).scatter_(1, target.view(-1, 1), 1.0)


def _as_target(target_class, batch: int, device) -> Optional[torch.Tensor]:
    if target_class is None:
        return None
    t = torch.as_tensor(target_class, device=device).long().reshape(-1)
    return t.expand(batch).contiguous() if t.numel() == 1 else t


class _Attributor:
    def __init__(self, model, device=None):
        self.model = model
        self.device = _default_device(device)
        self.model.to(self.device)
        self.model.eval()

    def _forward(self, pw, erp, conn=None):
        return self.model(pw, erp, conn) if conn is not None else self.model(pw, erp)

    def _run(self, erp, pw, conn, target_class, baselines, n_steps, chunk_steps=None):
        """-> (erp, pw, conn on the device, accumulators [erp, pw(, conn)]): the sum over the interpolation steps of the
        gradient of the target logit (one step, no baseline = the plain gradient at the input)"""
        self.model.eval()
        erp = erp.detach().to(self.device).float()
        pw = pw.detach().to(self.device).float()
        conn = None if conn is None else conn.detach().to(self.device).float()
        fixed = {"target": _as_target(target_class, erp.shape[0], self.device)}

        def forward(erp_i, pw_i, *c):
            return self._forward(pw_i, erp_i, c[0] if c else None)

        def seed(logits, s0, steps):
            if fixed["target"] is None:                   # the first step's prediction (alpha = 0 when interpolating)
                fixed["target"] = logits[:erp.shape[0]].argmax(dim=1)
            return _target_seed(logits, fixed["target"].repeat(steps))
        accs, _ = ops.integrated_gradients(forward, [erp, pw], baselines, n_steps, seed,
                                           constants=[] if conn is None else [conn], chunk_steps=chunk_steps)
        self.last_target = fixed["target"]
        return erp, pw, conn, accs


class GradientSaliency(_Attributor):
    """|d logit_target / d input| and its product with |input| (reference :88-152)."""

    def __init__(self, model: torch.nn.Module, device: torch.device = None):
        super().__init__(model, device)

    def _attribute(self, erp, pw, conn, target_class, method) -> Dict[str, np.ndarray]:
        # one "interpolation" step with the input as its own baseline: x + 0 * (x - x) = x
        erp_d, pw_d, conn_d, accs = self._run(erp, pw, conn, target_class, [erp, pw], 1, chunk_steps=1)
        out = {"erp": ops.xai_finish(erp_d, None, accs[0], 1, method)[0].cpu().numpy(),
               "pw": ops.xai_finish(pw_d, None, accs[1], 1, method)[0].cpu().numpy()}
        if conn_d is not None:
            out["conn"] = ops.xai_finish(conn_d, None, accs[2], 1, method)[0].cpu().numpy()
        return out

    def vanilla_gradient(self, erp: torch.Tensor, pw: torch.Tensor, conn: torch.Tensor = None,
                         target_class: int = None) -> Dict[str, np.ndarray]:
        return self._attribute(erp, pw, conn, target_class, "gradient")

    def gradient_x_input(self, erp: torch.Tensor, pw: torch.Tensor, conn: torch.Tensor = None,
                         target_class: int = None) -> Dict[str, np.ndarray]:
        return self._attribute(erp, pw, conn, target_class, "gradient_x_input")


class IntegratedGradients(_Attributor):
    """|(x - baseline) * mean over n_steps of d logit_target / d x(alpha)| (reference :155-236), the steps batched."""

    def __init__(self, model: torch.nn.Module, device: torch.device = None, n_steps: int = 50):
        super().__init__(model, device)
        self.n_steps = n_steps
        self.chunk_steps = None                   # None: ops.ig_chunk_steps (the memory rule) decides

    def compute(self, erp: torch.Tensor, pw: torch.Tensor, conn: torch.Tensor = None, target_class: int = None,
                baseline: str = "zero") -> Dict[str, np.ndarray]:
        if baseline == "zero":
            bases = [None, None]
        else:                                      # as in the reference, anything else is the batch mean
            bases = [erp.detach().to(self.device).float().mean(dim=0, keepdim=True),
                     pw.detach().to(self.device).float().mean(dim=0, keepdim=True)]
        erp_d, pw_d, conn_d, accs = self._run(erp, pw, conn, target_class, bases, self.n_steps, self.chunk_steps)
        m = "integrated_gradients"
        out = {"erp": ops.xai_finish(erp_d, bases[0], accs[0], self.n_steps, m)[0].cpu().numpy(),
               "pw": ops.xai_finish(pw_d, bases[1], accs[1], self.n_steps, m)[0].cpu().numpy()}
        if conn_d is not None:
            out["conn"] = ops.xai_finish(conn_d, None, accs[2], self.n_steps, m)[0].cpu().numpy()
        return out


class SHAPExplainer:
    """KernelSHAP wrapper (reference :243-365).  ``shap`` is an optional dependency: without it the constructor
    warns and ``compute_shap_values`` raises, as the reference does."""

    def __init__(self, model: torch.nn.Module, background_data: Dict[str, torch.Tensor], device: torch.device = None):
        self.model = model
        self.device = _default_device(device)
        self.background = background_data
        self.model.to(self.device)
        self.model.eval()
        self._shap_available = self._check_shap()

    def _check_shap(self) -> bool:
        try:
            import shap
        except ImportError:
            warnings.warn("SHAP not installed. Run: pip install shap")
            return False
        self.shap = shap
        return True

    def _logits_of_flat(self, flat, with_conn: bool):
        n_erp = int(np.prod(self.erp_shape[1:]))
        n_pw = int(np.prod(self.pw_shape[1:]))
        t = torch.as_tensor(np.asarray(flat), dtype=torch.float32, device=self.device)
        erp = t[:, :n_erp].reshape(-1, *self.erp_shape[1:]).contiguous()
        pw = t[:, n_erp:n_erp + n_pw].reshape(-1, *self.pw_shape[1:]).contiguous()
        with torch.no_grad():
            if with_conn:
                logits = self.model(pw, erp, t[:, n_erp + n_pw:].contiguous())
            else:
                logits = self.model(pw, erp)
        return logits.cpu().numpy()

    def _model_wrapper_trimodal(self, inputs):
        return self._logits_of_flat(inputs, True)

    def _model_wrapper_bimodal(self, inputs):
        return self._logits_of_flat(inputs, False)

    def compute_shap_values(self, erp: torch.Tensor, pw: torch.Tensor, conn: torch.Tensor = None,
                            n_background: int = 100) -> Dict[str, np.ndarray]:
        if not self._shap_available:
            raise RuntimeError("SHAP not available. Install with: pip install shap")
        self.erp_shape, self.pw_shape = erp.shape, pw.shape
        names = ["erp", "pw"] + (["conn"] if conn is not None else [])
        test = np.concatenate([t.cpu().numpy().reshape(t.shape[0], -1) for t in ([erp, pw] + ([conn] if conn is not None else []))], axis=1)
        background = np.concatenate([self.background[k][:n_background].cpu().numpy().reshape(n_background, -1) for k in names], axis=1)
        wrapper = self._model_wrapper_trimodal if conn is not None else self._model_wrapper_bimodal
        values = self.shap.KernelExplainer(wrapper, background).shap_values(test, nsamples=100)
        sv = values[1] if isinstance(values, list) else values          # the positive class
        n_erp, n_pw = int(np.prod(erp.shape[1:])), int(np.prod(pw.shape[1:]))
        out = {"erp": np.abs(sv[:, :n_erp]).reshape(-1, *erp.shape[1:]),
               "pw": np.abs(sv[:, n_erp:n_erp + n_pw]).reshape(-1, *pw.shape[1:])}
        if conn is not None:
            out["conn"] = np.abs(sv[:, n_erp + n_pw:])
        return out


class ChannelImportanceExtractor:
    """attribution maps -> per-channel, per-pair and per-region importance with 10-20 names (reference :372-491)"""

    def __init__(self, channel_names: List[str] = None, n_channels: int = None):
        if channel_names is not None:
            self.channel_names = channel_names
            self.n_channels = len(channel_names)
        elif n_channels is not None:
            self.n_channels = n_channels
            tables = {19: STANDARD_10_20_19, 21: STANDARD_10_20_21, 32: EXTENDED_10_10_32}
            self.channel_names = tables.get(n_channels) or [f"Ch{i + 1}" for i in range(n_channels)]
        else:
            raise ValueError("Must provide either channel_names or n_channels")

    def extract_channel_importance(self, attribution: np.ndarray, modality: str = "erp") -> Dict[str, float]:
        """(batch, channels, time) - or (batch, channels * k) flattened - -> {channel: share}, shares summing to 1"""
        if attribution.ndim == 2:
            n, f = attribution.shape
            attribution = attribution.reshape(n, self.n_channels, f // self.n_channels)
        imp = attribution.mean(axis=2).mean(axis=0)
        imp = imp / (imp.sum() + 1e-8)
        return {name: float(v) for name, v in zip(self.channel_names, imp)}

    def extract_connectivity_importance(self, attribution: np.ndarray) -> Dict[Tuple[str, str], float]:
        """connectivity attributions (batch, metrics * pairs) -> {(ch_i, ch_j), i < j: share}; pairs in row-major
        upper-triangle order, averaged over metrics and samples, normalised to sum 1"""
        n = attribution.shape[0]
        flat = attribution.reshape(n, -1)
        n_pairs = self.n_channels * (self.n_channels - 1) // 2
        per_pair = flat.reshape(n, flat.shape[1] // n_pairs, n_pairs).mean(axis=1).mean(axis=0)
        pairs = [(self.channel_names[i], self.channel_names[j])
                 for i in range(self.n_channels) for j in range(i + 1, self.n_channels)]
        raw = {pair: float(v) for pair, v in zip(pairs, per_pair)}
        total = sum(raw.values()) + 1e-8
        return {pair: v / total for pair, v in raw.items()}

    def get_region_importance(self, channel_importance: Dict[str, float]) -> Dict[str, float]:
        """mean importance of the channels present in each brain region (0.0 for a region without any)"""
        out = {}
        for region, members in BRAIN_REGIONS.items():
            found = [channel_importance[ch] for ch in members if ch in channel_importance]
            out[region] = float(np.mean(found)) if found else 0.0
        return out

    def get_top_channels(self, channel_importance: Dict[str, float], k: int = 5) -> List[Tuple[str, float]]:
        return sorted(channel_importance.items(), key=lambda kv: kv[1], reverse=True)[:k]

    def get_top_connections(self, conn_importance: Dict[Tuple[str, str], float], k: int = 10) -> List[Tuple[Tuple[str, str], float]]:
        return sorted(conn_importance.items(), key=lambda kv: kv[1], reverse=True)[:k]


def attention_connectivity_importance(encoder, x: torch.Tensor, edge_index: torch.Tensor, channel_names: List[str],
                                      edge_attr: Optional[torch.Tensor] = None) -> Dict[Tuple[str, str], float]:
    """which electrode pairs a ``GNNConnectivityEncoder`` attends to: {(source name, target name): share}.  The
    eval-mode attention alpha[target <- source] of the GATv2 layers (the softmax the kernels save, no dropout),
    averaged over batch, heads and layers; self-loops left out, the copies of a duplicated edge summed; normalised to
    sum 1 as ``ChannelImportanceExtractor.extract_connectivity_importance`` does, so ``get_top_connections`` takes it."""
    if len(channel_names) != encoder.num_nodes:
        raise ValueError(f"attention_connectivity_importance: {len(channel_names)} channel names for {encoder.num_nodes} nodes")
    was_training = encoder.training
    encoder.eval()
    try:
        with torch.no_grad():
            alphas: List[torch.Tensor] = []
            ops.gnn_conn_encoder_forward(encoder, x, edge_index, edge_attr, attn_sink=alphas)
            graph = ops.gat_graph(edge_index, encoder.num_nodes)
            pairs, _ = ops.gat_attention_output(graph, alphas[0])
            mean = torch.stack([ops.gat_attention_output(graph, a)[1].mean(dim=(0, 2)) for a in alphas]).mean(dim=0)
    finally:
        encoder.train(was_training)
    raw: Dict[Tuple[str, str], float] = defaultdict(float)
    for (s, t), v in zip(pairs.t().tolist(), mean.tolist()):
        if s != t:
            raw[(channel_names[s], channel_names[t])] += v
    total = sum(raw.values()) + 1e-8
    return {pair: v / total for pair, v in raw.items()}


def temporal_attention_importance(model, erp: Optional[torch.Tensor] = None, pw: Optional[torch.Tensor] = None,
                                  method: str = "rollout", top_k: int = 10) -> Dict[str, Dict[str, object]]:
    """which time steps the EEG transformer encoders attend to: {"erp": {...}, "pw": {...}} for the modalities given.
    ``model`` is a fusion net with ``erp_encoder`` / ``pw_encoder`` (EnhancedTriModalFusionNet, the V4 nets) or a bare
    encoder (its input goes in ``erp`` for an EnhancedERPEncoder, in ``pw`` otherwise).  Per modality: "tokens" (B, L)
    from ``encoder.temporal_attention(x, method)`` ("rollout" / "received") and "time" (B, T) where the encoder
    defines it, as numpy, and "top_steps": the ``top_k`` steps of the batch-mean importance ("time" when there is one,
    else "tokens") as [(index, value), ...], largest first.  Eval-mode semantics; the train / eval flags are not
    touched.  A model without a transformer encoder (the Lite nets, the notebook baselines) raises ValueError."""
    pairs = []
    if hasattr(model, "erp_encoder") or hasattr(model, "pw_encoder"):
        if erp is not None:
            pairs.append(("erp", getattr(model, "erp_encoder", None), erp))
        if pw is not None:
            pairs.append(("pw", getattr(model, "pw_encoder", None), pw))
    else:
        kind = ops._attention_encoder(model)[0]             # ValueError for anything that is not a transformer encoder
        name = "erp" if kind == "erp" else "pw"
        pairs.append((name, model, erp if name == "erp" else pw))
    if not pairs or any(x is None for _, _, x in pairs):
        raise ValueError("temporal_attention_importance: give erp= and / or pw= inputs for the model's encoders")
    out: Dict[str, Dict[str, object]] = {}
    for name, enc, x in pairs:
        if enc is None:
            raise ValueError(f"temporal_attention_importance: {type(model).__name__} has no {name}_encoder")
        res = ops.encoder_temporal_attention(enc, x, method)
        entry: Dict[str, object] = {k: v.detach().float().cpu().numpy() for k, v in res.items()}
        steps = entry.get("time", entry["tokens"]).mean(axis=0)
        order = np.argsort(-steps, kind="stable")[:max(int(top_k), 0)]
        entry["top_steps"] = [(int(i), float(steps[i])) for i in order]
        out[name] = entry
    return out


class EEGExplainer:
    """several attribution methods + channel-level summaries behind one object (reference :498-693)"""

    def __init__(self, model: torch.nn.Module, channel_names: List[str] = None, n_channels: int = None,
                 device: torch.device = None):
        self.model = model
        self.device = _default_device(device)
        self.model.to(self.device)
        self.model.eval()
        self.gradient_saliency = GradientSaliency(model, device)
        self.integrated_gradients = IntegratedGradients(model, device)
        self.channel_extractor = None
        self.channel_names = channel_names
        self.n_channels = n_channels
        self.results_history = []

    def _init_channel_extractor(self, sample_erp: torch.Tensor):
        if self.channel_extractor is None:
            n_ch = sample_erp.shape[1] if sample_erp.dim() == 3 else sample_erp.shape[0]
            self.channel_extractor = ChannelImportanceExtractor(channel_names=self.channel_names,
                                                                n_channels=self.n_channels or n_ch)

    def analyze_sample(self, erp: torch.Tensor, pw: torch.Tensor, conn: torch.Tensor = None, target_class: int = None,
                       methods: List[str] = ["gradient", "integrated_gradients"]) -> Dict:
        """'gradient' = gradient x input, 'integrated_gradients' = zero-baseline IG; unknown method names are skipped"""
        self._init_channel_extractor(erp)
        results = {"attributions": {}, "channel_importance": {}, "region_importance": {}, "top_channels": {},
                   "prediction": None}
        with torch.no_grad():
            e, p = erp.to(self.device), pw.to(self.device)
            logits = self.model(p, e, conn.to(self.device)) if conn is not None else self.model(p, e)
            results["prediction"] = {"class": logits.argmax(dim=1).cpu().numpy(),
                                     "probabilities": torch.softmax(logits.float().cpu(), dim=1).numpy()}
        ex = self.channel_extractor
        for method in methods:
            if method == "gradient":
                attr = self.gradient_saliency.gradient_x_input(erp, pw, conn, target_class)
            elif method == "integrated_gradients":
                attr = self.integrated_gradients.compute(erp, pw, conn, target_class)
            else:
                continue
            results["attributions"][method] = attr
            ch, reg, top = {}, {}, {}
            for modality in ("erp", "pw"):
                if modality in attr:
                    ch[modality] = ex.extract_channel_importance(attr[modality], modality)
                    reg[modality] = ex.get_region_importance(ch[modality])
                    top[modality] = ex.get_top_channels(ch[modality], k=5)
            if "conn" in attr:
                ch["connectivity"] = ex.extract_connectivity_importance(attr["conn"])
                top["connectivity"] = ex.get_top_connections(ch["connectivity"], k=10)
            results["channel_importance"][method] = ch
            results["region_importance"][method] = reg
            results["top_channels"][method] = top
        self.results_history.append(results)
        return results

    def analyze_dataset(self, dataloader, methods: List[str] = ["gradient"], max_samples: int = 100) -> Dict:
        """batches of 5 items are (erp, pw, conn, _, labels), of 4 items (erp, pw, _, labels); others are skipped"""
        ch_all = defaultdict(lambda: defaultdict(list))
        reg_all = defaultdict(lambda: defaultdict(list))
        n_analyzed = 0
        for batch in dataloader:
            if n_analyzed >= max_samples:
                break
            if len(batch) == 5:
                erp, pw, conn = batch[0], batch[1], batch[2]
            elif len(batch) == 4:
                erp, pw, conn = batch[0], batch[1], None
            else:
                continue
            res = self.analyze_sample(erp, pw, conn, methods=methods)
            for method in methods:
                for modality in ("erp", "pw"):
                    if modality in res["channel_importance"].get(method, {}):
                        for ch, v in res["channel_importance"][method][modality].items():
                            ch_all[method][f"{modality}_{ch}"].append(v)
                        for reg, v in res["region_importance"][method][modality].items():
                            reg_all[method][f"{modality}_{reg}"].append(v)
            n_analyzed += erp.shape[0]
        out = {"channel_importance": {}, "region_importance": {}, "n_samples": n_analyzed}
        for method in methods:
            out["channel_importance"][method] = {k: float(np.mean(v)) for k, v in ch_all[method].items()}
            out["region_importance"][method] = {k: float(np.mean(v)) for k, v in reg_all[method].items()}
        return out

    def get_channel_ranking(self, modality: str = "erp", method: str = "gradient") -> List[Tuple[str, float]]:
        if not self.results_history:
            raise ValueError("No analysis results. Run analyze_sample first.")
        scores = defaultdict(list)
        for res in self.results_history:
            for ch, v in res["channel_importance"].get(method, {}).get(modality, {}).items():
                scores[ch].append(v)
        return sorted(((ch, np.mean(v)) for ch, v in scores.items()), key=lambda kv: kv[1], reverse=True)
