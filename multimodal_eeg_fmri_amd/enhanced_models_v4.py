"""EEG temporal-encoder family on the MI355X HIP path.

Drop-in class surface for the reference's ``EEG_CODE/enhanced_models_v4.py``
(PositionalEncoding :30-55, TemporalTransformerBlock :58-107,
EnhancedERPEncoder :114-193, EnhancedPowerEncoder :196-285,
GNNConnectivityEncoder :292-413, LearnedFusionModule :420-488,
EnhancedTriModalFusionNet :495-657, get_fusion_weights :829-841): same class names, constructor signatures,
``forward`` conventions and ``state_dict`` keys/shapes, so the reference's
``best_*_fold*.pt`` checkpoints load unchanged.

The ``torch.nn`` leaf modules created in the constructors are *parameter
containers only* (they fix key names, shapes and the default initialisation);
``forward`` never calls them.  All arithmetic runs in the hand-written gfx950
kernels behind ``libmmeeg_hip.so`` (see ``ops.py`` / ``include/mmeeg_hip.h``);
there is no CPU or eager-PyTorch fallback: a CPU tensor or a missing library
raises.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import ops


def _drop(p: float) -> nn.Dropout:
    return nn.Dropout(p)


class PositionalEncoding(nn.Module):
    """Sinusoidal table ``pe`` (max_len, 1, d_model) added to the sequence.

    Reference quirk kept (enhanced_models_v4.py:49): a 3-D input is treated as
    batch-first only when ``x.size(1) != 1``.
    """

    def __init__(self, d_model: int, max_len: int = 5000, dropout: float = 0.1):
        super().__init__()
        self.dropout = _drop(dropout)
        pos = torch.arange(max_len, dtype=torch.float32)[:, None]
        freq = torch.exp(torch.arange(0, d_model, 2, dtype=torch.float32)
                         * (-math.log(10000.0) / d_model))
        table = torch.zeros(max_len, 1, d_model)
        table[:, 0, 0::2] = torch.sin(pos * freq)
        table[:, 0, 1::2] = torch.cos(pos * freq)
        self.register_buffer("pe", table)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.add_positional(x, self.pe, self.dropout.p, self.training)


class TemporalTransformerBlock(nn.Module):
    """Pre-norm MHA + FFN block; ``x`` is the fp32 residual stream (B, L, d)."""

    def __init__(self, d_model: int, nhead: int = 4, dim_feedforward: int = 512,
                 dropout: float = 0.1, activation: str = "gelu"):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout,
                                               batch_first=True)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.dropout = _drop(dropout)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.dropout1 = _drop(dropout)
        self.dropout2 = _drop(dropout)
        self.activation = nn.GELU() if activation == "gelu" else nn.ReLU()
        self._act = "gelu" if activation == "gelu" else "relu"
        self.nhead = nhead

    def forward(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        # ``mask`` = nn.MultiheadAttention's attn_mask (reference :98): (L, L) or (batch * heads, L, L), boolean
        # (True = not allowed) or additive float; the encoders themselves never pass one (reference :169-193)
        return ops.transformer_block(x, self, self.training, mask)

    def attention_weights(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None,
                          average_attn_weights: bool = True) -> torch.Tensor:
        """the second value of the reference's ``self.attn(x, x, x, attn_mask=mask)`` on ``norm1(x)`` (:99, which it
        discards): eval-mode attention probabilities, fp32 (B, L, L) averaged over the heads or (B, heads, L, L)"""
        return ops.block_attention_weights(self, x, mask, average_attn_weights)


class _TemporalAttentionReadout:
    """what the three EEG transformer encoders share: the attention of their transformer stack over time"""

    def attention_maps(self, x: torch.Tensor) -> List[torch.Tensor]:
        """one head-averaged (B, L, L) attention matrix per transformer layer, eval-mode semantics (frozen BatchNorm, no
        dropout) whatever the module's train / eval flags are; they are left as they were"""
        return ops.encoder_attention(self, x, "maps")

    def temporal_attention(self, x: torch.Tensor, method: str = "rollout", layer: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """per-time-step importance from the attention maps, without storing them: ``method`` "rollout" (all layers) or
        "received" (layer ``layer``, default last).  {"tokens": (B, L)} and, where the token-to-sample map is fixed,
        "time": (B, T), which sums to what "tokens" sums to."""
        return ops.encoder_temporal_attention(self, x, method, layer)


def _transformer_stack(hidden_dim, layers, heads, dropout):
    return nn.ModuleList([
        TemporalTransformerBlock(hidden_dim, nhead=heads,
                                 dim_feedforward=hidden_dim * 4, dropout=dropout)
        for _ in range(layers)])


def _pool_proj(hidden_dim, dropout):
    return nn.Sequential(nn.AdaptiveAvgPool1d(1), nn.Flatten(),
                         nn.Linear(hidden_dim, hidden_dim), nn.GELU(), _drop(dropout))


class EnhancedERPEncoder(_TemporalAttentionReadout, nn.Module):
    """(B, C, T) fp32 -> (B, hidden_dim): 3x [Conv1d-BN-GELU] (+MaxPool2 after
    the second) -> PE -> N transformer blocks -> mean over time -> Linear-GELU."""

    def __init__(self, in_channels: int, hidden_dim: int = 128,
                 num_transformer_layers: int = 2, num_heads: int = 4,
                 dropout: float = 0.3):
        super().__init__()
        self.conv_layers = nn.Sequential(
            nn.Conv1d(in_channels, 64, kernel_size=7, padding=3), nn.BatchNorm1d(64),
            nn.GELU(), _drop(dropout),
            nn.Conv1d(64, 128, kernel_size=5, padding=2), nn.BatchNorm1d(128),
            nn.GELU(), nn.MaxPool1d(2), _drop(dropout),
            nn.Conv1d(128, hidden_dim, kernel_size=3, padding=1), nn.BatchNorm1d(hidden_dim),
            nn.GELU(), _drop(dropout))
        self.pos_encoder = PositionalEncoding(hidden_dim, dropout=dropout)
        self.transformer_layers = _transformer_stack(hidden_dim, num_transformer_layers,
                                                     num_heads, dropout)
        self.output_proj = _pool_proj(hidden_dim, dropout)
        self.drop_p = dropout

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.erp_encoder_forward(self, x)


class EnhancedPowerEncoder(_TemporalAttentionReadout, nn.Module):
    """Multi-scale k=3/5/7 Conv1d front-end -> 1x1 fusion conv -> same tail."""

    def __init__(self, in_channels: int, hidden_dim: int = 128,
                 num_transformer_layers: int = 2, num_heads: int = 4,
                 dropout: float = 0.3):
        super().__init__()

        def scale(k):
            return nn.Sequential(nn.Conv1d(in_channels, 64, kernel_size=k, padding=k // 2),
                                 nn.BatchNorm1d(64), nn.GELU())
        self.conv_scale1 = scale(3)
        self.conv_scale2 = scale(5)
        self.conv_scale3 = scale(7)
        self.fusion = nn.Sequential(nn.Conv1d(192, hidden_dim, kernel_size=1),
                                    nn.BatchNorm1d(hidden_dim), nn.GELU(), _drop(dropout))
        self.pos_encoder = PositionalEncoding(hidden_dim, dropout=dropout)
        self.transformer_layers = _transformer_stack(hidden_dim, num_transformer_layers,
                                                     num_heads, dropout)
        self.output_proj = _pool_proj(hidden_dim, dropout)
        self.drop_p = dropout

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.power_encoder_forward(self, x)


class LearnedFusionModule(nn.Module):
    """0.5*softmax(logits/T) + 0.5*softmax(gate_net(cat)/T) weighted sum."""

    def __init__(self, num_modalities: int, hidden_dim: int,
                 use_temperature: bool = True, init_temperature: float = 1.0):
        super().__init__()
        self.num_modalities = num_modalities
        self.use_temperature = use_temperature
        self.fusion_logits = nn.Parameter(torch.ones(num_modalities))
        if use_temperature:
            self.temperature = nn.Parameter(torch.tensor(init_temperature))
        else:
            self.register_buffer("temperature", torch.tensor(1.0))
        self.gate_net = nn.Sequential(nn.Linear(hidden_dim * num_modalities, hidden_dim),
                                      nn.GELU(), _drop(0.2),
                                      nn.Linear(hidden_dim, num_modalities))

    def forward(self, modality_features: List[torch.Tensor], return_weights: bool = False):
        fused, w = ops.learned_fusion(self, list(modality_features), self.training)
        return (fused, w) if return_weights else fused


def _glorot(t: torch.Tensor) -> None:
    a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        t.uniform_(-a, a)


class _GATv2Base(nn.Module):
    """parameters and initialisation shared by GATv2Conv and GATv2EdgeConv: ``att`` (1, H, C), ``bias`` (H*C),
    ``lin_l`` / ``lin_r`` Linear(in, H*C) and, with ``edge_dim``, ``lin_edge`` Linear(edge_dim, H*C, bias=False) -
    torch_geometric's names and shapes, glorot weights, zero biases."""

    def __init__(self, in_channels, out_channels, heads, negative_slope, dropout, bias, edge_dim):
        super().__init__()
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.negative_slope, self.dropout, self.add_self_loops = True, negative_slope, dropout, True
        self.edge_dim = edge_dim
        self.lin_l = nn.Linear(in_channels, heads * out_channels, bias=bias)
        self.lin_r = nn.Linear(in_channels, heads * out_channels, bias=bias)
        if edge_dim is not None:
            self.lin_edge = nn.Linear(edge_dim, heads * out_channels, bias=False)
        self.att = nn.Parameter(torch.empty(1, heads, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(heads * out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        for lin in (self.lin_l, self.lin_r):
            _glorot(lin.weight)
            if lin.bias is not None:
                nn.init.zeros_(lin.bias)
        if self.edge_dim is not None:
            _glorot(self.lin_edge.weight)
        _glorot(self.att)
        if self.bias is not None:
            nn.init.zeros_(self.bias)


class GATv2Conv(_GATv2Base):
    """GATv2 graph attention (Brody et al. 2022) with the parameter names and shapes of torch_geometric's layer of
    the same name - ``att`` (1, H, C), ``bias`` (H*C), ``lin_l`` / ``lin_r`` Linear(in, H*C) - so that a state dict
    trained with it loads.  ``x`` is (N, in) or (B, N, in); every sample shares ``edge_index`` (2, E) =
    [source; target].  Runs on ``mm_gatv2_fwd`` / ``mm_gatv2_bwd``: at most 128 nodes, H*C <= 256, C in {16, 32, 64}.

    Edge features live in a class of their own, ``GATv2EdgeConv``: this one keeps refusing ``edge_dim`` and
    ``edge_attr`` with NotImplementedError (tests/test_gnn_host.py pins that), so code that relied on the refusal is
    not silently given another layer.  ``return_attention_weights=True`` -> ``(out, (edge_index', alpha))``:
    ``edge_index'`` (2, E') in torch_geometric's order (the listed non-loop edges in listed order, then the N
    self-loops), ``alpha`` (E', H) for 2-D ``x`` and (B, E', H) for 3-D ``x``.  Deviation: alpha is the softmax BEFORE
    attention dropout (what the kernel saves); torch_geometric returns it after dropout."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, concat: bool = True,
                 negative_slope: float = 0.2, dropout: float = 0.0, add_self_loops: bool = True, bias: bool = True,
                 edge_dim: Optional[int] = None, share_weights: bool = False):
        if not concat:
            raise NotImplementedError("GATv2Conv: concat=False (head averaging) is not implemented")
        if share_weights:
            raise NotImplementedError("GATv2Conv: share_weights=True is not implemented")
        if edge_dim is not None:
            raise NotImplementedError("GATv2Conv: edge features are not implemented here: use GATv2EdgeConv")
        if not add_self_loops:
            raise NotImplementedError("GATv2Conv: add_self_loops=False is not implemented")
        if not isinstance(in_channels, int):
            raise NotImplementedError("GATv2Conv: bipartite (source, target) input sizes are not implemented")
        super().__init__(in_channels, out_channels, heads, negative_slope, dropout, bias, None)

    def forward(self, x: torch.Tensor, edge_index: torch.Tensor, edge_attr=None, return_attention_weights=None):
        if edge_attr is not None:
            raise NotImplementedError("GATv2Conv: edge_attr is not implemented here: use GATv2EdgeConv")
        return ops.gatv2_conv_forward(self, x, edge_index, None, return_attention_weights)


class GATv2EdgeConv(_GATv2Base):
    """GATv2Conv with edge features, torch_geometric's ``GATv2Conv(edge_dim=D)``: its state dict loads (the extra key
    is ``lin_edge.weight`` (H*C, D)).  The attributes enter the score only, not the message:

        e[i<-j] = a^T leaky_relu(W_l h_j + W_r h_i + W_e a_ij)

    ``edge_attr`` is (E,) or (E, D) when the batch shares it, (B, E, D) per sample, its rows aligned with the listed
    ``edge_index``; D = ``edge_dim`` in 1..8.  Listed self-loops are dropped together with their attributes; the
    appended loop of node i gets ``fill_value``: 'mean' = the mean attribute of the remaining listed edges into i (0
    without any), or a constant.  A missing ``edge_attr``, a wrong D, E or B is a ValueError before any launch.
    ``return_attention_weights`` as in ``GATv2Conv``.  Runs on ``mm_gatv2_edge_fwd`` / ``mm_gatv2_edge_bwd``."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, edge_dim: int = 1,
                 negative_slope: float = 0.2, dropout: float = 0.0, bias: bool = True, fill_value="mean"):
        if isinstance(edge_dim, bool) or not isinstance(edge_dim, int) or not 1 <= edge_dim <= 8:
            raise ValueError(f"GATv2EdgeConv: edge_dim={edge_dim!r}, supported 1..8")
        ops._fill_args(fill_value)
        super().__init__(in_channels, out_channels, heads, negative_slope, dropout, bias, edge_dim)
        self.fill_value = fill_value

    def forward(self, x: torch.Tensor, edge_index: torch.Tensor, edge_attr: torch.Tensor = None,
                return_attention_weights=None):
        return ops.gatv2_conv_forward(self, x, edge_index, edge_attr, return_attention_weights)


class GNNConnectivityEncoder(nn.Module):
    """(B, nodes, nodes, conn_types) connectivity (or any shape that flattens to (B, nodes, -1)) -> (B, hidden_dim):
    per-node Linear-BN-GELU -> ``num_gat_layers`` x [GATv2Conv + GELU] over the shared electrode graph -> mean over
    nodes -> Linear-BN-GELU.  With ``edge_dim`` the layers are ``GATv2EdgeConv`` and ``forward`` takes ``edge_attr``
    ((E,), (E, D) or (B, E, D)); without one every sample's own connectivity is its edge feature,
    ea[b, e, :] = x[b, source e, target e, :], which needs the 4-D form and ``edge_dim == num_conn_types``."""

    def __init__(self, num_nodes: int, num_conn_types: int = 3, hidden_dim: int = 128, num_gat_layers: int = 2,
                 num_heads: int = 4, dropout: float = 0.3, edge_dim: Optional[int] = None):
        super().__init__()
        self.num_nodes = num_nodes
        self.num_conn_types = num_conn_types
        self.edge_dim = edge_dim
        self.node_proj = nn.Sequential(nn.Linear(num_nodes * num_conn_types, hidden_dim), nn.BatchNorm1d(hidden_dim),
                                       nn.GELU(), _drop(dropout))
        self.gat_layers = nn.ModuleList([
            GATv2Conv(hidden_dim, hidden_dim // num_heads, heads=num_heads, dropout=dropout, concat=True)
            if edge_dim is None else
            GATv2EdgeConv(hidden_dim, hidden_dim // num_heads, heads=num_heads, edge_dim=edge_dim, dropout=dropout)
            for _ in range(num_gat_layers)])
        self.output_proj = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.BatchNorm1d(hidden_dim),
                                         nn.GELU(), _drop(dropout))
        self.drop_p = dropout

    def create_graph_from_connectivity(self, conn_matrix: torch.Tensor,
                                       threshold: float = 0.5) -> Tuple[torch.Tensor, torch.Tensor]:
        """(batch, nodes, nodes) strengths -> (edge_index (2, E), edge_attr (E, 1)): the pairs whose batch mean
        exceeds ``threshold``.  Graph set-up, once per model: plain tensor indexing."""
        avg = conn_matrix.detach().mean(dim=0)
        edges = (avg > threshold).nonzero(as_tuple=False)
        return edges.t().contiguous(), avg[edges[:, 0], edges[:, 1]].unsqueeze(1)

    def forward(self, x: torch.Tensor, edge_index: torch.Tensor, edge_attr: Optional[torch.Tensor] = None) -> torch.Tensor:
        return ops.gnn_conn_encoder_forward(self, x, edge_index, edge_attr)


class EnhancedTriModalFusionNet(nn.Module):
    """ERP + Power transformer encoders, GNN (``use_gnn``) or MLP connectivity encoder, ERP-queries-all cross
    attention, learned 3-way fusion, BN-MLP classifier (reference :495-657; same child names and state_dict).
    ``edge_index`` is made from the first batch and kept as a plain attribute (it is not part of the state dict).
    ``gnn_edge_features``: the GNN encoder is built with ``edge_dim=num_conn_types`` and reads every sample's own
    connectivity strengths as the features of its edges."""

    def __init__(self, erp_channels: int, pw_channels: int, num_conn_nodes: int, num_conn_types: int = 3,
                 hidden_dim: int = 128, num_classes: int = 2, dropout: float = 0.3,
                 num_transformer_layers: int = 2, num_heads: int = 4, use_gnn: bool = True,
                 gnn_edge_features: bool = False):
        super().__init__()
        self.use_gnn = use_gnn
        self.erp_encoder = EnhancedERPEncoder(erp_channels, hidden_dim, num_transformer_layers, num_heads, dropout)
        self.pw_encoder = EnhancedPowerEncoder(pw_channels, hidden_dim, num_transformer_layers, num_heads, dropout)

        def mlp_bn(i, o):
            return [nn.Linear(i, o), nn.BatchNorm1d(o), nn.GELU(), _drop(dropout)]
        if use_gnn:
            self.conn_encoder = GNNConnectivityEncoder(num_conn_nodes, num_conn_types, hidden_dim, num_gat_layers=2,
                                                       num_heads=num_heads, dropout=dropout,
                                                       edge_dim=num_conn_types if gnn_edge_features else None)
        else:
            self.conn_encoder = nn.Sequential(*mlp_bn(num_conn_nodes * num_conn_nodes * num_conn_types, 256),
                                              *mlp_bn(256, hidden_dim))
        self.fusion = LearnedFusionModule(num_modalities=3, hidden_dim=hidden_dim, use_temperature=True)
        self.cross_attn = nn.MultiheadAttention(hidden_dim, num_heads=num_heads, dropout=dropout, batch_first=True)
        self.classifier = nn.Sequential(*mlp_bn(hidden_dim, hidden_dim), *mlp_bn(hidden_dim, hidden_dim // 2),
                                        nn.Linear(hidden_dim // 2, num_classes))
        self.edge_index = None
        self.drop_p = dropout

    def forward(self, erp: torch.Tensor, pw: torch.Tensor, conn: torch.Tensor, return_fusion_weights: bool = False):
        logits, weights, _ = ops.trimodal_forward(self, erp, pw, conn)
        return (logits, weights) if return_fusion_weights else logits


def get_fusion_weights(model: EnhancedTriModalFusionNet) -> Dict[str, float]:
    """the static fusion weights softmax(fusion_logits / temperature) and the temperature, as floats"""
    with torch.no_grad():                                # three scalars for a report, as get_fusion_weights_from_model
        temp = model.fusion.temperature
        w = torch.softmax(model.fusion.fusion_logits / temp, dim=0).tolist()
    return {"erp_weight": w[0], "pw_weight": w[1], "conn_weight": w[2], "temperature": temp.item()}
