"""GPU: mm_gatv2_fwd / mm_gatv2_bwd (csrc/gnn.hip) against an fp64 restatement of the GATv2 layer, written from the
paper (Brody et al., "How Attentive are Graph Attention Networks?", eq. 7) as plain sums over an edge list:

    e[i<-j] = a^T leaky_relu(W_l h_j + W_r h_i),  alpha = softmax over the edges into i,  out_i = sum_j alpha W_l h_j + bias

with torch_geometric's self-loop rule (listed self-loops dropped, one per node appended), attention dropout as a keep
mask on alpha (oracle/dropout_replica.py: keep_scale at element (b H + h) E' + e, e the edge's position after the stable
sort by target) and an optional exact-erf GELU on the output.  B = 3 throughout.

    case  N    H  C   graph
    1     5    1  16  no edges: self-loops only
    2     19   4  32  random directed, density ~0.3, listed self-loops, one duplicated edge, one node without incoming edge
    3     33   8  16  directed ring
    4     64   4  32  all ordered pairs
    5     128  4  64  random directed, density 0.1

Each case runs at p = 0 and p = 0.25 (an exact binary fraction: the kernel's threshold and the replica's are the same
integer), with and without the GELU epilogue.  Figures are rel-L2 errors ||got - want|| / ||want||; the bounds are
about twice the worst case measured on the MI355X over the 20 runs:

    out 1.6e-7 (bound 3.5e-7)   alpha 1.8e-7 (3.5e-7)   dxl 2.7e-7 (5.5e-7)   dxr 3.3e-7 (7e-7)
    datt 5.4e-7 (1.1e-6: the sum over all B N deg edges of a head, 12 288 terms in case 4)   dbias 1.8e-7 (4e-7)

Those scores are a few nats.  test_gatv2_subtracts_the_maximum_at_large_scores runs cases 2 and 4 with `att` scaled until the
edge scores span +-60 nats, each quantity bounded by 16 x the error of the same formula in fp32 torch on the CPU (measured:
at most 0.08 of that bound).

Exact: an (sample, node, head) whose incoming edges are all dropped leaves the bias alone; two backward runs give the
same bits; a second backward onto the same d att / d bias buffers doubles them (they are accumulated into)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle.dropout_replica import keep_scale
from multimodal_eeg_fmri_amd import ops
from test_kernels_gpu import _hip

pytestmark = pytest.mark.gpu

D64 = torch.float64
B = 3
SLOPE = 0.2
SEED = 0x5EED1234
BOUND = {"out": 3.5e-7, "alpha": 3.5e-7, "dxl": 5.5e-7, "dxr": 7e-7, "datt": 1.1e-6, "dbias": 4e-7}


def _rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    den = want.norm().item()
    return (got - want).norm().item() / (den if den > 0 else 1.0)


def _random_edges(n, density, seed):
    g = torch.Generator().manual_seed(seed)
    adj = torch.rand(n, n, generator=g) < density
    adj.fill_diagonal_(False)
    return adj.nonzero().t().contiguous()                       # row 0 = source, row 1 = target


def _edge_index(case):
    if case == 1:
        return torch.zeros(2, 0, dtype=torch.long)
    if case == 2:
        ei = _random_edges(19, 0.3, 21)
        ei = ei[:, ei[1] != 11]                                 # node 11: no incoming edge
        extra = torch.tensor([[3, 7, int(ei[0, 5])], [3, 7, int(ei[1, 5])]])       # two listed self-loops, edge 5 twice
        return torch.cat([ei[:, :9], extra, ei[:, 9:]], dim=1)
    if case == 3:
        i = torch.arange(33)
        return torch.stack([i, (i + 1) % 33])
    if case == 4:
        adj = ~torch.eye(64, dtype=torch.bool)
        return adj.nonzero().t().contiguous()
    return _random_edges(128, 0.1, 55)


SHAPES = {1: (5, 1, 16), 2: (19, 4, 32), 3: (33, 8, 16), 4: (64, 4, 32), 5: (128, 4, 64)}


def _prepare(ei, n):
    """the test's own statement of the self-loop rule and the stable sort by target -> (source, target) in CSR order"""
    pairs = [(int(s), int(t)) for s, t in ei.t().tolist() if s != t] + [(k, k) for k in range(n)]
    pairs = sorted(pairs, key=lambda st: st[1])                  # sorted() is stable
    return torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs])


@functools.lru_cache(maxsize=None)
def _case(case):
    n, h, c = SHAPES[case]
    ei = _edge_index(case)
    src, dst = _prepare(ei, n)
    g = torch.Generator().manual_seed(1000 + case)
    t = dict(ei=ei, src=src, dst=dst,
             xlr=torch.randn(B, n, 2 * h * c, generator=g),
             att=torch.randn(h, c, generator=g) / math.sqrt(c),
             bias=0.5 * torch.randn(h * c, generator=g),
             dout=torch.randn(B, n, h * c, generator=g))
    return t


def _oracle(t, n, h, c, keep, gelu, dtype=D64):
    """fp64 forward + autograd gradients; keep (B, H, E').  dtype = torch.float32: the same formula in plain fp32"""
    src, dst = t["src"], t["dst"]
    xlr = t["xlr"].to(dtype)
    xl = xlr[..., :h * c].reshape(B, n, h, c).clone().requires_grad_(True)
    xr = xlr[..., h * c:].reshape(B, n, h, c).clone().requires_grad_(True)
    att = t["att"].to(dtype).clone().requires_grad_(True)
    bias = t["bias"].to(dtype).clone().requires_grad_(True)
    score = (F.leaky_relu(xl[:, src] + xr[:, dst], SLOPE) * att).sum(-1)           # (B, E', H)
    alpha = torch.zeros_like(score)
    for i in range(n):                                                             # softmax over the edges into i
        sel = (dst == i).nonzero().flatten()
        alpha = alpha.index_copy(1, sel, torch.softmax(score[:, sel], dim=1))
    a = alpha * keep.to(dtype).permute(0, 2, 1)
    out = torch.zeros(B, n, h, c, dtype=dtype).index_add(1, dst, a.unsqueeze(-1) * xl[:, src]) + bias.view(h, c)
    out = out.reshape(B, n, h * c)
    pre = out
    if gelu:
        out = 0.5 * out * (1.0 + torch.erf(out / math.sqrt(2.0)))
    (out * t["dout"].to(dtype)).sum().backward()
    return dict(out=out.detach(), pre=pre.detach(), alpha=alpha.detach(), score=score.detach(),
                dxl=xl.grad.reshape(B, n, h * c), dxr=xr.grad.reshape(B, n, h * c), datt=att.grad, dbias=bias.grad)


def _run_kernels(t, n, h, c, p, gelu, runs=1):
    hip = _hip()
    graph = ops.gat_graph(t["ei"].cuda(), n)
    E, hc = graph.num_edges, h * c
    xlr = t["xlr"].cuda()
    att, bias, dout = t["att"].cuda(), t["bias"].cuda(), t["dout"].cuda()
    act = 1 if gelu else 0
    out = torch.full((B, n, hc), float("nan"), device="cuda")
    pre = torch.full((B, n, hc), float("nan"), device="cuda") if gelu else None
    alpha = torch.full((B, h, E), float("nan"), device="cuda")
    xr_ptr = xlr.data_ptr() + 4 * hc
    hip.call("mm_gatv2_fwd", xlr, xr_ptr, 2 * hc, att, bias, graph.rowptr, graph.col, out, pre, alpha,
             B, n, h, c, E, SLOPE, act, p, SEED, None)
    res = []
    datt, dbias = torch.zeros(h, c, device="cuda"), torch.zeros(hc, device="cuda")
    for _ in range(runs):
        dxlr = torch.full((B, n, 2 * hc), float("nan"), device="cuda")
        ds = torch.full((B, h, E), float("nan"), device="cuda")
        dz = torch.full((B, n, hc), float("nan"), device="cuda") if gelu else None
        part = torch.full((B, 2, hc), float("nan"), device="cuda")
        before = (datt.clone(), dbias.clone())
        hip.call("mm_gatv2_bwd", dout, pre, xlr, xr_ptr, 2 * hc, att, alpha, graph.rowptr, graph.col, graph.colptr,
                 graph.row, graph.perm, dxlr, dxlr.data_ptr() + 4 * hc, datt, dbias, ds, dz, part,
                 B, n, h, c, E, SLOPE, act, p, SEED, None)
        res.append(dict(dxl=dxlr[..., :hc].clone(), dxr=dxlr[..., hc:].clone(),
                        datt=datt - before[0], dbias=dbias - before[1]))
    torch.cuda.synchronize()
    return graph, dict(out=out, pre=pre, alpha=alpha), res, (datt, dbias)


def test_case_graphs_are_what_the_table_says():
    for case, (n, _, _) in SHAPES.items():
        t = _case(case)
        g = ops.gat_graph(t["ei"], n)
        assert torch.equal(g.col.long(), t["src"]) and g.rowptr.tolist() == [int((t["dst"] < i).sum()) for i in range(n + 1)]
        adj = torch.zeros(n, n)
        adj[t["ei"][0], t["ei"][1]] = 1
        if case in (2, 3):
            assert not torch.equal(adj, adj.t())                                   # a source/target swap cannot pass
    t2 = _case(2)
    ei = t2["ei"]
    assert int((ei[0] == ei[1]).sum()) == 2 and not bool((ei[1] == 11).any())
    assert ei.shape[1] - torch.unique(ei, dim=1).shape[1] == 1                      # one duplicated edge
    deg = torch.bincount(t2["dst"], minlength=19)
    assert deg[11] == 1 and len(t2["src"]) == ei.shape[1] - 2 + 19
    assert len(_case(4)["src"]) == 64 * 64 and len(_case(1)["src"]) == 5


@pytest.mark.parametrize("gelu", [False, True], ids=["linear", "gelu"])
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("case", [1, 2, 3, 4, 5])
def test_gatv2_fwd_bwd_match_fp64(case, p, gelu):
    n, h, c = SHAPES[case]
    t = _case(case)
    E = len(t["src"])
    keep = keep_scale(SEED, B * h * E, p).view(B, h, E)
    want = _oracle(t, n, h, c, keep, gelu)
    graph, fwd, (bwd,), _ = _run_kernels(t, n, h, c, p, gelu)
    assert graph.num_edges == E
    errs = {"out": _rel(fwd["out"], want["out"]), "alpha": _rel(fwd["alpha"].permute(0, 2, 1), want["alpha"])}
    for k in ("dxl", "dxr", "datt", "dbias"):
        errs[k] = _rel(bwd[k].reshape(want[k].shape), want[k])
    for k, v in errs.items():
        print(f"ERR gatv2 case {case} p {p} gelu {int(gelu)} {k} {v:.3e}")
    bad = {k: v for k, v in errs.items() if not v <= BOUND[k]}
    assert not bad, bad
    if p > 0:
        # (sample, node, head) with every incoming edge dropped: the aggregate is exactly 0, the bias is all that is left
        dropped = torch.zeros(B, n, h).index_add(1, t["dst"], (keep == 0).float().permute(0, 2, 1))
        alone = dropped == torch.bincount(t["dst"], minlength=n).view(1, n, 1)
        if case in (1, 3):
            assert bool(alone.any())
        lin = (fwd["pre"] if gelu else fwd["out"]).cpu().view(B, n, h, c)
        assert torch.equal(lin[alone], t["bias"].view(1, 1, h, c).expand(B, n, h, c)[alone])
        if case == 1:                                            # degree 1, edge dropped: nothing flows back either
            for k in ("dxl", "dxr"):
                assert torch.count_nonzero(bwd[k].cpu().view(B, n, h, c)[alone]) == 0


@pytest.mark.parametrize("case,p,gelu", [(2, 0.25, True), (4, 0.0, False)])
def test_gatv2_subtracts_the_maximum_at_large_scores(case, p, gelu):
    """`att` scaled until the edge scores span +-60 nats (every case above: a few nats, where exp needs no maximum
    subtracted).  The absolute bounds above assume scores of order 1; here each quantity is held to 16 x e32, e32 = the
    rel-L2 error of the same formula in plain fp32 torch on the CPU on the same inputs (test_norm_passes_gpu.py)."""
    n, h, c = SHAPES[case]
    t = dict(_case(case))
    E = len(t["src"])
    keep = keep_scale(SEED, B * h * E, p).view(B, h, E)
    t["att"] = t["att"] * (60.0 / _oracle(t, n, h, c, keep, gelu)["score"].abs().max().item())
    want = _oracle(t, n, h, c, keep, gelu)
    assert 59.0 < want["score"].abs().max().item() < 61.0
    assert want["score"].min().item() < -30.0 and want["score"].max().item() > 30.0
    cpu32 = _oracle(t, n, h, c, keep, gelu, torch.float32)
    _, fwd, (bwd,), _ = _run_kernels(t, n, h, c, p, gelu)
    got = {"out": fwd["out"], "alpha": fwd["alpha"].permute(0, 2, 1), **{k: bwd[k] for k in ("dxl", "dxr", "datt", "dbias")}}
    bad = {}
    for k, v in got.items():
        err, bound = _rel(v.reshape(want[k].shape), want[k]), 16 * _rel(cpu32[k], want[k])
        print(f"ERR gatv2 large scores case {case} p {p} gelu {int(gelu)} {k} {err:.3e} (bound {bound:.3e})")
        assert torch.isfinite(v).all(), k
        if not err <= bound:
            bad[k] = (err, bound)
    assert not bad, bad


@pytest.mark.parametrize("case,p,gelu", [(2, 0.25, True), (4, 0.0, False), (5, 0.25, True)])
def test_two_backward_runs_give_the_same_bits_and_accumulate(case, p, gelu):
    n, h, c = SHAPES[case]
    _, _, (r1, r2), (datt, dbias) = _run_kernels(_case(case), n, h, c, p, gelu, runs=2)
    for k in ("dxl", "dxr"):
        assert torch.equal(r1[k], r2[k]), k
    # the first run added g to zeros, the second g to g: exactly 2 g in fp32 when both runs formed the same g
    assert torch.equal(datt, 2 * r1["datt"]) and torch.equal(dbias, 2 * r1["dbias"])
    assert torch.count_nonzero(r1["datt"]) > 0 and torch.count_nonzero(r1["dbias"]) > 0
