"""GPU: GATv2EdgeConv, GNNConnectivityEncoder(edge_dim=...), return_attention_weights, attention_connectivity_importance and
EnhancedTriModalFusionNet(gnn_edge_features=True) on the HIP path against fp64 restatements (plain torch on the CPU,
autograd for the gradients) that extend those of tests/test_gnn_models_gpu.py with the edge term of the score,

    e[i<-j] = a^T leaky_relu(W_l h_j + W_r h_i + W_e a_ij),

and the attribute rule of tests/test_gnn_edge_kernels_gpu.py (_pack64).  The encoder is GNNConnectivityEncoder(12, 3, 64,
num_heads=4, edge_dim=3), B = 4, on the graph of create_graph_from_connectivity; without an ``edge_attr`` its edge features
are every sample's own connectivity, so the gradient with respect to ``conn`` flows through the node and the edge path.

Bounds: FWD = 5e-6 and BWD = 2e-5 of tests/test_gnn_models_gpu.py (same stage count: the edge term adds D <= 8 products
inside a stage, no stage), plus its train-mode BatchNorm amplification A / 4 A, taken from the oracle's own statistics."""
import pytest
import torch
import torch.nn.functional as F

from multimodal_eeg_fmri_amd import ops
import multimodal_eeg_fmri_amd.enhanced_models_v4 as E
from multimodal_eeg_fmri_amd.eeg_xai_analysis import ChannelImportanceExtractor, attention_connectivity_importance
from test_gnn_edge_kernels_gpu import _pack64
from test_gnn_models_gpu import BWD, FWD, _bn64, _edges, _Errs, _gelu, _lin64, _randomize, _rel, _split

pytestmark = pytest.mark.gpu

NODES, TYPES, HID, HEADS, BN = 12, 3, 64, 4, 4


def _randomize_edge(m, seed):
    _randomize(m, seed)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, E.GATv2EdgeConv):
                for b in (mod.bias, mod.lin_l.bias, mod.lin_r.bias):
                    b.copy_(0.1 * torch.randn(b.shape, generator=g))
    return m


def _gat_edge64(P, pre, x, ea_csr, src, dst, heads):
    """x (B, N, in), ea_csr (1 | B, E', D) -> (out (B, N, H C), alpha (B, E', H))"""
    Bn, n, _ = x.shape
    xl = (x @ P[pre + "lin_l.weight"].t() + P[pre + "lin_l.bias"]).view(Bn, n, heads, -1)
    xr = (x @ P[pre + "lin_r.weight"].t() + P[pre + "lin_r.bias"]).view(Bn, n, heads, -1)
    edge = (ea_csr @ P[pre + "lin_edge.weight"].t()).view(ea_csr.shape[0], -1, heads, xl.shape[-1])
    score = (F.leaky_relu(xl[:, src] + xr[:, dst] + edge, 0.2) * P[pre + "att"]).sum(-1)
    alpha = torch.zeros_like(score)
    for i in range(n):
        sel = (dst == i).nonzero().flatten()
        alpha = alpha.index_copy(1, sel, torch.softmax(score[:, sel], dim=1))
    out = torch.zeros_like(xl).index_add(1, dst, alpha.unsqueeze(-1) * xl[:, src])
    return out.reshape(Bn, n, -1) + P[pre + "bias"], alpha


def _gnn_edge64(P, S, pre, x, ei, heads, train, stats=None, alphas=None):
    """the encoder with its own connectivity as edge features; x (B, N, N, types)"""
    Bn, n = x.shape[0], x.shape[1]
    src, dst = _edges(ei, n)
    ea_csr = _pack64(x[:, ei[0], ei[1], :], ei, n, "mean")
    x = x.reshape(Bn, n, -1)
    if train:
        h = torch.stack([_gelu(_bn64(P, S, pre + "node_proj.1.", _lin64(P, pre + "node_proj.0.", x[i]), True, stats))
                         for i in range(Bn)])
    else:
        h = _gelu(_bn64(P, S, pre + "node_proj.1.", _lin64(P, pre + "node_proj.0.", x), False))
    for i in range(2):
        h, alpha = _gat_edge64(P, f"{pre}gat_layers.{i}.", h, ea_csr, src, dst, heads)
        h = _gelu(h)
        if alphas is not None:
            alphas.append(alpha.detach())
    return _gelu(_bn64(P, S, pre + "output_proj.1.", _lin64(P, pre + "output_proj.0.", h.mean(1)), train, stats))


def _tg_order(ei, n):
    """torch_geometric's edge order: the listed non-loop edges in listed order, then the n self-loops"""
    keep = ei[0] != ei[1]
    loops = torch.arange(n)
    return torch.stack([torch.cat([ei[0][keep], loops]), torch.cat([ei[1][keep], loops])])


def _csr_to_tg(ei, n):
    """index (E') that takes the oracle's CSR-ordered edges to torch_geometric's order"""
    ids = [(int(t), k) for k, (s, t) in enumerate(ei.t().tolist()) if s != t] + [(k, -1 - k) for k in range(n)]
    ids = [k for _, k in sorted(ids, key=lambda tk: tk[0])]
    where = {k: p for p, k in enumerate(ids)}
    kept = [k for k, (s, t) in enumerate(ei.t().tolist()) if s != t]
    return torch.tensor([where[k] for k in kept] + [where[-1 - i] for i in range(n)])


def _encoder_inputs():
    torch.manual_seed(41)
    m = _randomize_edge(E.GNNConnectivityEncoder(NODES, TYPES, HID, num_heads=HEADS, dropout=0.0, edge_dim=TYPES), 42).cuda()
    g = torch.Generator().manual_seed(43)
    x = torch.rand(BN, NODES, NODES, TYPES, generator=g)
    gy = torch.randn(BN, HID, generator=g)
    ei, strength = m.create_graph_from_connectivity(x[..., 0])
    assert ei.shape[0] == 2 and strength.shape == (ei.shape[1], 1) and bool((ei[0] == ei[1]).any())   # listed loops too
    return m, x, gy, ei


# ------------------------------------------------------------------------------------------ GNNConnectivityEncoder
def test_edge_encoder_eval_and_train_match_fp64():
    m, x, gy, ei = _encoder_inputs()
    eic = ei.cuda()
    errs = _Errs("GNN edge encoder")
    P, S = _split(m)
    m.eval()
    with torch.no_grad():
        got = m(x.cuda(), eic)
        want = _gnn_edge64(P, S, "", x.double(), ei, HEADS, False)
        assert torch.equal(m(x.cuda(), eic, x.cuda()[:, eic[0], eic[1], :]), got)      # the same attributes, passed in
    assert got.shape == (BN, HID)
    errs("eval out", _rel(got, want), FWD)
    m.train()
    xg = x.cuda().requires_grad_(True)
    out = m(xg, eic)
    out.backward(gy.cuda())
    x64 = x.double().requires_grad_(True)
    stats = {}
    want = _gnn_edge64(P, S, "", x64, ei, HEADS, True, stats)
    (want * gy.double()).sum().backward()
    A = stats.pop("amp")
    print(f"train-mode BatchNorm amplification A = {A:.3e}")
    fwd_t, bwd_t = FWD + A, BWD + 4 * A
    errs("train out", _rel(out, want), fwd_t)
    errs("d conn", _rel(xg.grad, x64.grad), bwd_t)
    # the edge path alone carries part of d conn: entries outside the graph's edges get the node path only
    zero = {"node_proj.0.bias": "node_proj.0.weight", "output_proj.0.bias": "output_proj.0.weight"}
    names = [k for k, _ in m.named_parameters()]
    assert "gat_layers.0.lin_edge.weight" in names and "gat_layers.1.lin_edge.weight" in names
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        if k in zero:
            scale = P[zero[k]].grad.norm().item()
            assert P[k].grad.norm().item() <= 1e-9 * scale, k
            errs("d " + k + " (zero)", p.grad.double().norm().item() / scale, bwd_t)
        else:
            errs("d " + k, _rel(p.grad, P[k].grad), bwd_t)
    errs.done()


def test_edge_path_carries_gradient_to_the_connectivity():
    """d out / d edge_attr alone, against the oracle: x fixed, the attributes a separate (B, E, D) leaf"""
    m, x, gy, ei = _encoder_inputs()
    m.eval()
    eic = ei.cuda()
    ea = x[:, ei[0], ei[1], :].clone()
    eag = ea.cuda().requires_grad_(True)
    out = m(x.cuda(), eic, eag)
    out.backward(gy.cuda())
    P, S = _split(m)
    ea64 = ea.double().requires_grad_(True)
    src, dst = _edges(ei, NODES)
    h = _gelu(_bn64(P, S, "node_proj.1.", _lin64(P, "node_proj.0.", x.double().reshape(BN, NODES, -1)), False))
    csr = _pack64(ea64, ei, NODES, "mean")
    for i in range(2):
        h = _gelu(_gat_edge64(P, f"gat_layers.{i}.", h, csr, src, dst, HEADS)[0])
    want = _gelu(_bn64(P, S, "output_proj.1.", _lin64(P, "output_proj.0.", h.mean(1)), False))
    (want * gy.double()).sum().backward()
    errs = _Errs("GNN edge encoder, edge path")
    errs("out", _rel(out, want), FWD)
    errs("d edge_attr", _rel(eag.grad, ea64.grad), BWD)
    errs.done()
    loops = (ei[0] == ei[1])
    assert torch.count_nonzero(eag.grad[:, loops.cuda()]) == 0 and torch.count_nonzero(eag.grad) > 0   # dropped rows get none


# ------------------------------------------------------------------------------------------- attention weights
@pytest.mark.parametrize("edge", [True, False], ids=["edge", "plain"])
def test_return_attention_weights_order_shape_and_values(edge):
    torch.manual_seed(51)
    n, fin, H, C, D = 9, 24, 2, 16, 2
    conv = (E.GATv2EdgeConv(fin, C, heads=H, edge_dim=D) if edge else E.GATv2Conv(fin, C, heads=H)).cuda().eval()
    g = torch.Generator().manual_seed(52)
    ei = torch.tensor([[0, 1, 2, 3, 4, 4, 5, 6, 7, 8, 0, 2, 2], [1, 2, 3, 4, 4, 5, 6, 7, 8, 0, 5, 7, 7]])   # (4, 4) listed, (2, 7) twice
    x = torch.randn(3, n, fin, generator=g)
    ea = torch.randn(ei.shape[1], D, generator=g)
    args = (ei.cuda(), ea.cuda()) if edge else (ei.cuda(),)
    P, _ = _split(conv)
    src, dst = _edges(ei, n)
    if edge:
        want_out, want_alpha = _gat_edge64(P, "", x.double(), _pack64(ea.double().unsqueeze(0), ei, n, "mean"), src, dst, H)
    else:
        P["lin_edge.weight"] = torch.zeros(H * C, 1, dtype=torch.float64)
        want_out, want_alpha = _gat_edge64(P, "", x.double(), torch.zeros(1, len(src), 1, dtype=torch.float64), src, dst, H)
    want_alpha = want_alpha[:, _csr_to_tg(ei, n)]
    Ec = ei.shape[1] - 1 + n
    for mode in ("inference", "tape"):
        xin = x.cuda().requires_grad_(mode == "tape")
        with torch.set_grad_enabled(mode == "tape"):
            out, (ei2, alpha) = conv(xin, *args, return_attention_weights=True)
            plain_out = conv(xin, *args)
        assert torch.equal(out, plain_out)
        assert ei2.shape == (2, Ec) and alpha.shape == (3, Ec, H) and not alpha.requires_grad
        assert torch.equal(ei2.cpu(), _tg_order(ei, n))
        sums = torch.zeros(3, n, H).index_add(1, ei2[1].cpu(), alpha.cpu())
        assert torch.allclose(sums, torch.ones(3, n, H), atol=1e-6)                     # the weights into each target
        assert _rel(alpha, want_alpha) <= FWD and _rel(out, want_out) <= FWD
    with torch.no_grad():                                                              # 2-D x: (E', H)
        out1, (ei1, alpha1) = conv(x[0].cuda(), *args, return_attention_weights=True)
    assert out1.shape == (n, H * C) and alpha1.shape == (Ec, H) and torch.equal(ei1, ei2)
    assert _rel(alpha1, want_alpha[0]) <= FWD


def test_edge_conv_gradients_with_shared_attributes_match_fp64():
    torch.manual_seed(61)
    n, fin, H, C, D = 7, 24, 2, 16, 1
    conv = _randomize_edge(E.GATv2EdgeConv(fin, C, heads=H, edge_dim=D, fill_value=0.5), 62).cuda().train()
    g = torch.Generator().manual_seed(63)
    ei = torch.tensor([[0, 1, 2, 3, 4, 5, 6, 0, 2, 2, 5], [1, 2, 3, 4, 5, 6, 0, 3, 2, 6, 1]])
    x, gy, ea = torch.randn(2, n, fin, generator=g), torch.randn(2, n, H * C, generator=g), torch.randn(ei.shape[1], generator=g)
    xg, eag = x.cuda().requires_grad_(True), ea.cuda().requires_grad_(True)            # (E,): one strength per edge
    out = conv(xg, ei.cuda(), eag)
    out.backward(gy.cuda())
    P, _ = _split(conv)
    x64, ea64 = x.double().requires_grad_(True), ea.double().requires_grad_(True)
    src, dst = _edges(ei, n)
    want, _ = _gat_edge64(P, "", x64, _pack64(ea64.view(1, -1, 1), ei, n, 0.5), src, dst, H)
    (want * gy.double()).sum().backward()
    errs = _Errs("GATv2EdgeConv")
    errs("out", _rel(out, want), FWD)
    errs("dx", _rel(xg.grad, x64.grad), BWD)
    errs("d edge_attr", _rel(eag.grad, ea64.grad), BWD)
    assert eag.grad.shape == ea.shape
    params = dict(conv.named_parameters())
    assert sorted(params) == ["att", "bias", "lin_edge.weight", "lin_l.bias", "lin_l.weight", "lin_r.bias", "lin_r.weight"]
    for k, p in params.items():
        assert p.grad is not None, k
        errs("d " + k, _rel(p.grad, P[k].grad), BWD)
    errs.done()


def test_attention_connectivity_importance_names_real_edges_and_sorts():
    m, x, _, ei = _encoder_inputs()
    names = [f"Ch{i}" for i in range(NODES)]
    m.train()
    imp = attention_connectivity_importance(m, x.cuda(), ei.cuda(), names)
    assert m.training                                                                 # the mode is put back
    real = {(names[s], names[t]) for s, t in ei.t().tolist() if s != t}
    assert set(imp) == real and all(a != b for a, b in imp)
    assert all(v > 0 for v in imp.values()) and sum(imp.values()) == pytest.approx(1.0, abs=1e-6)
    # against the oracle's alpha: mean over batch, heads and layers, loops left out, normalised
    P, S = _split(m)
    alphas = []
    _gnn_edge64(P, S, "", x.double(), ei, HEADS, False, alphas=alphas)
    mean = torch.stack([a.mean(dim=(0, 2)) for a in alphas]).mean(0)[_csr_to_tg(ei, NODES)]
    pairs = _tg_order(ei, NODES).t().tolist()
    want = {(names[s], names[t]): float(v) for (s, t), v in zip(pairs, mean) if s != t}
    total = sum(want.values())
    for k, v in imp.items():
        assert v == pytest.approx(want[k] / total, rel=1e-5), k
    top = ChannelImportanceExtractor(channel_names=names).get_top_connections(imp, k=5)
    assert len(top) == 5 and [v for _, v in top] == sorted(imp.values(), reverse=True)[:5]
    with pytest.raises(ValueError):
        attention_connectivity_importance(m, x.cuda(), ei.cuda(), names[:-1])


# --------------------------------------------------------------------------------------- EnhancedTriModalFusionNet
def _trimodal_step(seed):
    torch.manual_seed(seed)
    ops.set_dropout_seed(seed)
    m = E.EnhancedTriModalFusionNet(8, 8, NODES, hidden_dim=HID, gnn_edge_features=True).cuda().train()
    g = torch.Generator().manual_seed(seed + 2)
    erp, pw = torch.randn(4, 8, 64, generator=g).cuda(), torch.randn(4, 8, 64, generator=g).cuda()
    conn = torch.rand(4, NODES, NODES, TYPES, generator=g).cuda()
    y = torch.tensor([0, 1, 1, 0]).cuda()
    before = [l.lin_edge.weight.detach().clone() for l in m.conn_encoder.gat_layers]
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    loss = F.cross_entropy(m(erp, pw, conn), y)
    loss.backward()
    grads = [l.lin_edge.weight.grad.clone() for l in m.conn_encoder.gat_layers]
    opt.step()
    after = [l.lin_edge.weight.detach().clone() for l in m.conn_encoder.gat_layers]
    return loss.detach(), before, grads, after


def test_trimodal_with_edge_features_trains_lin_edge_and_is_reproducible():
    loss1, before, grads1, after1 = _trimodal_step(71)
    assert torch.isfinite(loss1)
    for b, g, a in zip(before, grads1, after1):
        assert torch.isfinite(g).all() and torch.count_nonzero(g) > 0 and not torch.equal(a, b)
    loss2, _, grads2, after2 = _trimodal_step(71)
    assert torch.equal(loss1, loss2)
    for u, v in zip(grads1 + after1, grads2 + after2):
        assert torch.equal(u, v)
