"""GPU: GATv2Conv, GNNConnectivityEncoder and EnhancedTriModalFusionNet on the HIP path against fp64 restatements of
the same modules (plain torch on the CPU, autograd for the gradients), written from the formulas: GATv2 as sums over an
edge list (Brody et al. eq. 7, torch_geometric's self-loop rule), BatchNorm1d with batch statistics / running-statistic
updates as nn.BatchNorm1d documents them, nn.MultiheadAttention with one query token, the learned fusion as
0.5 softmax(logits / T) + 0.5 softmax(gate(cat) / T).

Bounds (rel-L2, ||got - want|| / ||want||).  Every stage here is an fp32 row kernel whose own bound is <= 1.1e-6, typically 3e-7
(tests/test_gnn_kernels_gpu.py, tests/test_head_kernels_gpu.py); errors of stages in sequence add at most linearly.
  FWD = 5e-6   the longest forward chain (tri-modal net: 2 + 2 x 2 + 2 encoder stages, 3 attention, 3 fusion, 5 head) is
               about 20 stages, 20 x 2.5e-7 typical;
  BWD = 2e-5   a gradient passes the forward and the backward chain (twice the stages) and the BatchNorm backward
               divides by a standard deviation taken over as few as 4 rows;
  running statistics / fusion weights: FWD.
Train-mode BatchNorm adds a term that depends on the data, not on the kernels: the batch variance is formed in one pass
as E[z^2] - mean^2 from fp32 values (relative rounding 2^-24 of each term) summed in the project's fixed-point
accumulators (resolution 2^-28, csrc/common.h MM_ACC_STAT), so 1 / sqrt(var + eps) carries a relative error of up to
  amp_c = (2^-24 mean_c^2 + 2^-28) / (2 (var_c + eps))            per channel c
which is large where a channel barely varies over the batch - and the pooled rows that reach output_proj differ little
between samples (var down to 2e-5 at mean^2 / var = 1000).  A = the rms of amp over the channels, taken from the fp64
oracle's own statistics (the largest over the train-mode BatchNorm calls), is added to the forward bound; the BatchNorm
backward uses the reciprocal deviation once and the normalised value twice and starts from the perturbed forward, so
gradients get 4 A.  With the inputs below A = 2.3e-5 / 2.8e-5 (both from output_proj; node_proj's is 4e-7).
A gradient that is ZERO in exact arithmetic (a bias in front of a train-mode BatchNorm: the mean subtraction removes it)
has no relative error: its norm is held against BWD x the norm of the weight gradient of the same layer."""
import math

import pytest
import torch
import torch.nn.functional as F

from multimodal_eeg_fmri_amd import ops
import multimodal_eeg_fmri_amd.enhanced_models_v4 as E

pytestmark = pytest.mark.gpu

D64 = torch.float64
FWD, BWD = 5e-6, 2e-5


def _rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    den = want.norm().item()
    return (got - want).norm().item() / (den if den > 0 else 1.0)


class _Errs:
    def __init__(self, tag):
        self.tag, self.rows = tag, []

    def __call__(self, name, err, bound):
        self.rows.append((name, err, bound))
        print(f"ERR {self.tag} {name} {err:.3e} (bound {bound:.0e})")

    def done(self):
        bad = [r for r in self.rows if not r[1] <= r[2]]
        assert not bad, f"{self.tag}: " + ", ".join(f"{n} {e:.3e} > {b:.0e}" for n, e, b in bad)


def _randomize(m, seed):
    """non-trivial BatchNorm affine / running statistics and biases (the default initialisation leaves them 1 / 0)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.weight.copy_(0.5 + torch.rand(mod.weight.shape, generator=g))
                mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
                mod.running_mean.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.bias.shape, generator=g))
            if isinstance(mod, E.GATv2Conv):
                for b in (mod.bias, mod.lin_l.bias, mod.lin_r.bias):
                    b.copy_(0.1 * torch.randn(b.shape, generator=g))
            if isinstance(mod, E.LearnedFusionModule):
                mod.fusion_logits.copy_(torch.randn(mod.fusion_logits.shape, generator=g))
                mod.temperature.fill_(1.3)
    return m


# --------------------------------------------------------------------------------------------- fp64 restatements
def _gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def _edges(ei, n):
    pairs = [(int(s), int(t)) for s, t in ei.t().tolist() if s != t] + [(k, k) for k in range(n)]
    pairs = sorted(pairs, key=lambda st: st[1])
    return torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs])


def _gat64(P, pre, x, src, dst, heads):
    """x (B, N, in) -> (B, N, H C)"""
    Bn, n, _ = x.shape
    xl = (x @ P[pre + "lin_l.weight"].t() + P[pre + "lin_l.bias"]).view(Bn, n, heads, -1)
    xr = (x @ P[pre + "lin_r.weight"].t() + P[pre + "lin_r.bias"]).view(Bn, n, heads, -1)
    score = (F.leaky_relu(xl[:, src] + xr[:, dst], 0.2) * P[pre + "att"]).sum(-1)          # (B, E, H)
    alpha = torch.zeros_like(score)
    for i in range(n):
        sel = (dst == i).nonzero().flatten()
        alpha = alpha.index_copy(1, sel, torch.softmax(score[:, sel], dim=1))
    out = torch.zeros_like(xl).index_add(1, dst, alpha.unsqueeze(-1) * xl[:, src])
    return out.reshape(Bn, n, -1) + P[pre + "bias"]


def _bn64(P, S, pre, z, train, stats=None):
    """BatchNorm1d on rows; train: batch statistics, and the running-statistic update recorded in ``stats``"""
    if train:
        mean, var = z.mean(0), z.var(0, unbiased=False)
        if stats is not None:
            k = z.shape[0]
            rm, rv, cnt = stats.get(pre, (S[pre + "running_mean"], S[pre + "running_var"], 0))
            stats[pre] = (0.9 * rm + 0.1 * mean.detach(), 0.9 * rv + 0.1 * var.detach() * k / (k - 1), cnt + 1)
            amp = 0.5 * (2.0 ** -24 * mean.detach() ** 2 + 2.0 ** -28) / (var.detach() + 1e-5)
            stats["amp"] = max(stats.get("amp", 0.0), amp.pow(2).mean().sqrt().item())
    else:
        mean, var = S[pre + "running_mean"], S[pre + "running_var"]
    return (z - mean) / torch.sqrt(var + 1e-5) * P[pre + "weight"] + P[pre + "bias"]


def _lin64(P, pre, x):
    return x @ P[pre + "weight"].t() + P[pre + "bias"]


def _gnn64(P, S, pre, x, src, dst, heads, train, stats=None):
    Bn, n = x.shape[0], x.shape[1]
    x = x.reshape(Bn, n, -1)
    if train:                                                    # node_proj sample by sample: statistics over the nodes of one sample
        h = torch.stack([_gelu(_bn64(P, S, pre + "node_proj.1.", _lin64(P, pre + "node_proj.0.", x[i]), True, stats))
                         for i in range(Bn)])
    else:
        h = _gelu(_bn64(P, S, pre + "node_proj.1.", _lin64(P, pre + "node_proj.0.", x), False))
    for i in range(2):
        h = _gelu(_gat64(P, f"{pre}gat_layers.{i}.", h, src, dst, heads))
    return _gelu(_bn64(P, S, pre + "output_proj.1.", _lin64(P, pre + "output_proj.0.", h.mean(1)), train, stats))


def _split(m):
    """(parameters as fp64 leaves, buffers as fp64)"""
    P = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in m.named_parameters()}
    S = {k: v.detach().double().cpu().clone() for k, v in m.named_buffers()}
    return P, S


def _downstream64(P, S, m, e, w, conn, src, dst, heads):
    """eval-mode EnhancedTriModalFusionNet after the two temporal encoders -> (logits, fusion weights)"""
    Bn = conn.shape[0]
    if m.use_gnn:
        c = _gnn64(P, S, "conn_encoder.", conn, src, dst, heads, False)
    else:
        c = conn.reshape(Bn, -1)
        for a, b in (("0.", "1."), ("4.", "5.")):
            c = _gelu(_bn64(P, S, "conn_encoder." + b, _lin64(P, "conn_encoder." + a, c), False))
    Ed = e.shape[1]
    W, b = P["cross_attn.in_proj_weight"], P["cross_attn.in_proj_bias"]
    toks = torch.stack([e, w, c], dim=1)                                              # (B, 3, E)
    q = (e @ W[:Ed].t() + b[:Ed]).view(Bn, heads, 1, -1)
    k = (toks @ W[Ed:2 * Ed].t() + b[Ed:2 * Ed]).view(Bn, 3, heads, -1).transpose(1, 2)
    v = (toks @ W[2 * Ed:].t() + b[2 * Ed:]).view(Bn, 3, heads, -1).transpose(1, 2)
    a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(Ed // heads), dim=-1)
    enh = _lin64(P, "cross_attn.out_proj.", (a @ v).reshape(Bn, Ed))
    feats = [enh, w, c]
    T = P["fusion.temperature"]
    static = torch.softmax(P["fusion.fusion_logits"] / T, dim=0)
    g = _lin64(P, "fusion.gate_net.3.", _gelu(_lin64(P, "fusion.gate_net.0.", torch.cat(feats, dim=1))))
    wts = 0.5 * static + 0.5 * torch.softmax(g / T, dim=1)
    fused = (torch.stack(feats, dim=1) * wts.unsqueeze(2)).sum(1)
    h = fused
    for a_, b_ in (("0.", "1."), ("4.", "5.")):
        h = _gelu(_bn64(P, S, "classifier." + b_, _lin64(P, "classifier." + a_, h), False))
    return _lin64(P, "classifier.8.", h), wts


# ------------------------------------------------------------------------------------------------------- GATv2Conv
def test_gatv2conv_forward_and_all_gradients_match_fp64():
    torch.manual_seed(5)
    n, fin, H, C = 7, 24, 2, 16
    conv = _randomize(E.GATv2Conv(fin, C, heads=H), 6).cuda().train()
    g = torch.Generator().manual_seed(7)
    ei = torch.tensor([[0, 1, 2, 3, 4, 5, 6, 0, 2, 2, 5], [1, 2, 3, 4, 5, 6, 0, 3, 2, 6, 1]])
    x = torch.randn(2, n, fin, generator=g)
    gy = torch.randn(2, n, H * C, generator=g)
    xg = x.cuda().requires_grad_(True)
    out = conv(xg, ei.cuda())
    out.backward(gy.cuda())
    P, _ = _split(conv)
    x64 = x.double().requires_grad_(True)
    src, dst = _edges(ei, n)
    want = _gat64(P, "", x64, src, dst, H)
    (want * gy.double()).sum().backward()
    errs = _Errs("GATv2Conv")
    errs("out", _rel(out, want), FWD)
    errs("dx", _rel(xg.grad, x64.grad), BWD)
    params = dict(conv.named_parameters())
    assert sorted(params) == ["att", "bias", "lin_l.bias", "lin_l.weight", "lin_r.bias", "lin_r.weight"]
    for k, p in params.items():
        assert p.grad is not None, k
        errs("d " + k, _rel(p.grad, P[k].grad), BWD)
    errs.done()
    # (N, in) is (1, N, in)
    conv.eval()
    with torch.no_grad():
        a = conv(x[0].cuda(), ei.cuda())
        b = conv(x[:1].cuda(), ei.cuda())
    assert a.shape == (n, H * C) and torch.equal(a, b[0])
    assert _rel(a, want[0]) <= FWD


# ------------------------------------------------------------------------------------------ GNNConnectivityEncoder
def _ring_plus(n, seed):
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(n)
    extra = torch.randint(0, n, (2, 2 * n), generator=g)
    return torch.cat([torch.stack([i, (i + 1) % n]), extra], dim=1)


@pytest.mark.parametrize("nodes,hid", [(12, 64), (21, 128)])
def test_gnn_encoder_eval_and_train_match_fp64(nodes, hid):
    Bn, heads = 4, 4
    torch.manual_seed(11)
    m = _randomize(E.GNNConnectivityEncoder(num_nodes=nodes, num_conn_types=3, hidden_dim=hid, num_heads=heads,
                                            dropout=0.0), 12).cuda()
    g = torch.Generator().manual_seed(13)
    x = torch.rand(Bn, nodes, nodes, 3, generator=g)
    gy = torch.randn(Bn, hid, generator=g)
    ei = _ring_plus(nodes, 14)
    src, dst = _edges(ei, nodes)
    eic = ei.cuda()
    errs = _Errs(f"GNN encoder {nodes}/{hid}")
    # eval
    P, S = _split(m)
    m.eval()
    with torch.no_grad():
        got = m(x.cuda(), eic)
        want = _gnn64(P, S, "", x.double(), src, dst, heads, False)
    assert got.shape == (Bn, hid)
    errs("eval out", _rel(got, want), FWD)
    # train, dropout 0
    m.train()
    xg = x.cuda().requires_grad_(True)
    out = m(xg, eic)
    out.backward(gy.cuda())
    x64 = x.double().requires_grad_(True)
    stats = {}
    want = _gnn64(P, S, "", x64, src, dst, heads, True, stats)
    (want * gy.double()).sum().backward()
    A = stats.pop("amp")
    print(f"train-mode BatchNorm amplification A = {A:.3e}")
    fwd_t, bwd_t = FWD + A, BWD + 4 * A
    errs("train out", _rel(out, want), fwd_t)
    errs("dx", _rel(xg.grad, x64.grad), bwd_t)
    zero = {"node_proj.0.bias": "node_proj.0.weight", "output_proj.0.bias": "output_proj.0.weight"}   # removed by a train-mode BatchNorm
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        if k in zero:
            scale = P[zero[k]].grad.norm().item()
            assert P[k].grad.norm().item() <= 1e-9 * scale, k                          # zero in the oracle too
            errs("d " + k + " (zero)", p.grad.double().norm().item() / scale, bwd_t)
        else:
            errs("d " + k, _rel(p.grad, P[k].grad), bwd_t)
    bufs = dict(m.named_buffers())
    for pre, want_cnt in (("node_proj.1.", Bn), ("output_proj.1.", 1)):
        rm, rv, cnt = stats[pre]
        assert cnt == want_cnt
        errs(pre + "running_mean", _rel(bufs[pre + "running_mean"], rm), FWD)
        errs(pre + "running_var", _rel(bufs[pre + "running_var"], rv), FWD)
        assert int(bufs[pre + "num_batches_tracked"]) == want_cnt, pre
    errs.done()


# --------------------------------------------------------------------------------------- EnhancedTriModalFusionNet
def _trimodal(use_gnn, seed, dropout=0.3):
    torch.manual_seed(seed)
    m = _randomize(E.EnhancedTriModalFusionNet(8, 8, 12, hidden_dim=64, dropout=dropout, use_gnn=use_gnn), seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    erp, pw = torch.randn(4, 8, 64, generator=g), torch.randn(4, 8, 64, generator=g)
    conn = torch.rand(4, 12, 12, 3, generator=g)
    return m.cuda(), erp.cuda(), pw.cuda(), conn


@pytest.mark.parametrize("use_gnn", [True, False], ids=["gnn", "mlp"])
def test_trimodal_logits_weights_and_conn_gradient_match_fp64(use_gnn):
    m, erp, pw, conn = _trimodal(use_gnn, 21)
    m.eval()
    errs = _Errs(f"trimodal use_gnn={use_gnn}")
    with torch.no_grad():
        logits, weights = m(erp, pw, conn.cuda(), return_fusion_weights=True)
        assert torch.equal(m(erp, pw, conn.cuda()), logits)
        e, w = m.erp_encoder(erp).float(), m.pw_encoder(pw).float()
    assert logits.shape == (4, 2) and weights.shape == (4, 3)
    src = dst = None
    if use_gnn:
        # built once, from the first sample's first connectivity type at threshold 0.5, and kept
        want_ei = (conn[0, :, :, 0] > 0.5).nonzero().t()
        assert torch.equal(m.edge_index.cpu(), want_ei) and m.edge_index.is_cuda
        first = m.edge_index
        m(erp, pw, torch.flip(conn, dims=[0]).cuda())
        assert m.edge_index is first
        src, dst = _edges(want_ei, 12)
    else:
        assert m.edge_index is None
    P, S = _split(m)
    c64 = conn.double().requires_grad_(True)
    want_logits, want_w = _downstream64(P, S, m, e.double().cpu(), w.double().cpu(), c64, src, dst, 4)
    errs("logits", _rel(logits, want_logits), FWD)
    errs("fusion weights", _rel(weights, want_w), FWD)
    assert torch.allclose(weights.sum(1).cpu(), torch.ones(4), atol=1e-6)
    # eval mode with grad enabled: d logits / d conn through frozen BatchNorm
    # (with autograd on, the temporal encoders take their differentiable path: the oracle gets THOSE features)
    gy = torch.tensor([[1.0, -0.5], [0.3, 0.7], [-1.1, 0.2], [0.4, 0.9]])
    cg = conn.cuda().requires_grad_(True)
    out = m(erp, pw, cg)
    out.backward(gy.cuda())
    e, w = m.erp_encoder(erp).detach().float(), m.pw_encoder(pw).detach().float()
    want_logits, _ = _downstream64(P, S, m, e.double().cpu(), w.double().cpu(), c64, src, dst, 4)
    (want_logits * gy.double()).sum().backward()
    errs("logits (autograd on)", _rel(out, want_logits), FWD)
    errs("d logits / d conn", _rel(cg.grad, c64.grad), BWD)
    errs.done()
    fw = E.get_fusion_weights(m)
    assert sum(fw[k] for k in ("erp_weight", "pw_weight", "conn_weight")) == pytest.approx(1.0, abs=1e-6)
    assert fw["temperature"] == pytest.approx(1.3, abs=1e-6)


@pytest.mark.parametrize("use_gnn", [True, False], ids=["gnn", "mlp"])
def test_trimodal_ten_adam_steps_lower_the_cross_entropy(use_gnn):
    m, erp, pw, conn = _trimodal(use_gnn, 31, dropout=0.0)
    m.fusion.gate_net[2].p = 0.0
    m.train()
    conn = conn.cuda()
    y = torch.tensor([0, 1, 1, 0]).cuda()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = F.cross_entropy(m(erp, pw, conn), y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses
    if use_gnn:
        for k, p in m.conn_encoder.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
