"""GPU: "mm_gatv2_edge_fwd" / "mm_gatv2_edge_bwd" / "mm_gatv2_edge_pack" / "mm_gatv2_edge_pack_bwd" (csrc/gnn.hip) against
an fp64 restatement of GATv2 with edge features (torch_geometric's GATv2Conv(edge_dim = D)), written as plain sums over
an edge list:

    e[i<-j] = a^T leaky_relu(W_l h_j + W_r h_i + W_e a_ij),  alpha = softmax over the edges into i,
    out_i   = sum_j alpha W_l h_j + bias                       (the attributes enter the score only)

Self-loop rule: listed self-loops are dropped with their attributes, the appended loop of node i gets the mean of the
attributes of the remaining listed edges into i (0 without any) or a constant.  The oracle differentiates with respect to
the LISTED attributes, so "d edge_attr" below is what comes out of the pack backward.  Graphs, dropout replica and the
GELU epilogue are those of tests/test_gnn_kernels_gpu.py; B = 3.

    case  N    H  C   D  attributes  graph
    1     5    1  16  1  shared      no edges: self-loops only ('mean' gives 0; 1f = the same with fill_value = 1.0)
    2     19   4  32  3  per sample  case-2 graph; the two copies of the duplicated edge carry different attributes
    3     33   8  16  8  shared      directed ring: the loop's fill equals the one incoming attribute
    4     64   4  32  1  per sample  all ordered pairs, E' = 4 096, multi-chunk rows
    5     128  4  64  2  shared      random directed, density 0.1

Each case runs at p = 0 and p = 0.25, with and without the GELU epilogue.  Figures are rel-L2 errors; the bounds are about
twice the worst case measured on the MI355X over the 24 runs (none may exceed 5e-6: an fp32 kernel further than that from
fp64 is wrong, not rounded):

    out 1.8e-7 (bound 4e-7)   alpha 2.2e-7 (4.5e-7)   dxl 3.2e-7 (6.5e-7)   dxr 4.1e-7 (8.5e-7)   dbias 1.8e-7 (3.5e-7)
    datt 6.2e-7 (1.3e-6)   d lin_edge.weight 1.2e-6 (2.3e-6: like datt a sum over all B N deg edges of a head, of products
    with the raw attributes)   d edge_attr 4.9e-7 (1e-6; through the pack backward, against the oracle's listed gradient)

Exact: with lin_edge.weight = 0, out and alpha have the bits of "mm_gatv2_fwd" on the same inputs; two backward runs give
the same bits; a second backward doubles the accumulated d att, d bias and d lin_edge.weight; with a null d edge_attr
pointer every other output is unchanged."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle.dropout_replica import keep_scale
from multimodal_eeg_fmri_amd import ops
from test_kernels_gpu import _hip
from test_gnn_kernels_gpu import B, SEED, SHAPES, SLOPE, _edge_index, _prepare, _rel

pytestmark = pytest.mark.gpu

D64 = torch.float64
EDGE = {1: (1, False), 2: (3, True), 3: (8, False), 4: (1, True), 5: (2, False)}       # case -> (D, per sample)
BOUND = {"out": 4e-7, "alpha": 4.5e-7, "dxl": 6.5e-7, "dxr": 8.5e-7, "datt": 1.3e-6, "dbias": 3.5e-7, "dwe": 2.3e-6, "dea": 1e-6}
CASES = [1, "1f", 2, 3, 4, 5]


def _split_case(case):
    return (1, 1.0) if case == "1f" else (case, "mean")


@functools.lru_cache(maxsize=None)
def _case(case):
    n, h, c = SHAPES[case]
    d, per = EDGE[case]
    ei = _edge_index(case)
    src, dst = _prepare(ei, n)
    g = torch.Generator().manual_seed(2000 + case)
    return dict(ei=ei, src=src, dst=dst,
                xlr=torch.randn(B, n, 2 * h * c, generator=g),
                att=torch.randn(h, c, generator=g) / math.sqrt(c),
                bias=0.5 * torch.randn(h * c, generator=g),
                dout=torch.randn(B, n, h * c, generator=g),
                we=torch.randn(h * c, d, generator=g) / math.sqrt(d),
                ea=torch.randn(B if per else 1, ei.shape[1], d, generator=g))


def _pack64(ea, ei, n, fill):
    """the test's own statement of the attribute rule: listed (Bo, E, D) -> CSR order (Bo, E', D), differentiable"""
    ids = [(int(t), k) for k, (s, t) in enumerate(ei.t().tolist()) if s != t] + [(k, -1) for k in range(n)]
    ids = sorted(ids, key=lambda tk: tk[0])                                        # stable: listed order within a target
    eid = torch.tensor([k for _, k in ids])
    kept = eid[eid >= 0]
    tgt = ei[1][kept]
    if fill == "mean":
        deg = torch.bincount(tgt, minlength=n).clamp(min=1).view(1, n, 1)
        loops = torch.zeros(ea.shape[0], n, ea.shape[2], dtype=D64).index_add(1, tgt, ea[:, kept]) / deg
    else:
        loops = torch.full((ea.shape[0], n, ea.shape[2]), float(fill), dtype=D64)
    csr = torch.zeros(ea.shape[0], len(ids), ea.shape[2], dtype=D64)
    csr = csr.index_copy(1, (eid >= 0).nonzero().flatten(), ea[:, kept])
    return csr.index_copy(1, (eid < 0).nonzero().flatten(), loops)                 # the loop of node i is the i-th -1


def _oracle(t, n, h, c, keep, gelu, fill):
    src, dst = t["src"], t["dst"]
    xlr = t["xlr"].double()
    leaf = lambda v: v.double().clone().requires_grad_(True)
    xl, xr = leaf(xlr[..., :h * c].reshape(B, n, h, c)), leaf(xlr[..., h * c:].reshape(B, n, h, c))
    att, bias, we, ea = leaf(t["att"]), leaf(t["bias"]), leaf(t["we"]), leaf(t["ea"])
    ea_csr = _pack64(ea, t["ei"], n, fill)
    edge = (ea_csr @ we.t()).view(ea_csr.shape[0], -1, h, c)                       # (1 | B, E', H, C)
    score = (F.leaky_relu(xl[:, src] + xr[:, dst] + edge, SLOPE) * att).sum(-1)    # (B, E', H)
    alpha = torch.zeros_like(score)
    for i in range(n):
        sel = (dst == i).nonzero().flatten()
        alpha = alpha.index_copy(1, sel, torch.softmax(score[:, sel], dim=1))
    a = alpha * keep.double().permute(0, 2, 1)
    out = torch.zeros(B, n, h, c, dtype=D64).index_add(1, dst, a.unsqueeze(-1) * xl[:, src]) + bias.view(h, c)
    out = out.reshape(B, n, h * c)
    if gelu:
        out = 0.5 * out * (1.0 + torch.erf(out / math.sqrt(2.0)))
    (out * t["dout"].double()).sum().backward()
    return dict(out=out.detach(), alpha=alpha.detach(), ea_csr=ea_csr.detach(),
                dxl=xl.grad.reshape(B, n, h * c), dxr=xr.grad.reshape(B, n, h * c), datt=att.grad, dbias=bias.grad,
                dwe=we.grad, dea=ea.grad)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _run_kernels(t, n, h, c, p, gelu, fill="mean", runs=1, want_dea=True, we=None):
    hip = _hip()
    graph = ops.gat_graph(t["ei"].cuda(), n)
    E, hc = graph.num_edges, h * c
    Bo, El, D = t["ea"].shape
    xlr, att, bias, dout = t["xlr"].cuda(), t["att"].cuda(), t["bias"].cuda(), t["dout"].cuda()
    we = (t["we"] if we is None else we).cuda()
    ea = t["ea"].cuda()
    fill_mean, fill_v = (1, 0.0) if fill == "mean" else (0, float(fill))
    ea_csr = _nan(Bo, E, D)
    hip.call("mm_gatv2_edge_pack", ea if El else None, graph.eid, graph.rowptr, graph.indeg, ea_csr, Bo, n, El, E, D,
             fill_mean, fill_v)
    act = 1 if gelu else 0
    out, alpha = _nan(B, n, hc), _nan(B, h, E)
    pre = _nan(B, n, hc) if gelu else None
    xr_ptr = xlr.data_ptr() + 4 * hc
    hip.call("mm_gatv2_edge_fwd", xlr, xr_ptr, 2 * hc, att, bias, we, ea_csr, int(Bo != 1), graph.rowptr, graph.col, out,
             pre, alpha, B, n, h, c, E, D, SLOPE, act, p, SEED, None)
    res = []
    datt, dbias, dwe = torch.zeros(h, c, device="cuda"), torch.zeros(hc, device="cuda"), torch.zeros(hc, D, device="cuda")
    for _ in range(runs):
        dxlr, ds, part, wpart = _nan(B, n, 2 * hc), _nan(B, h, E), _nan(B, 2, hc), _nan(B, hc, D)
        dz = _nan(B, n, hc) if gelu else None
        dea_csr, epart, dea = (_nan(Bo, E, D), _nan(B, h, E, D), _nan(Bo, El, D)) if want_dea else (None, None, None)
        before = (datt.clone(), dbias.clone(), dwe.clone())
        hip.call("mm_gatv2_edge_bwd", dout, pre, xlr, xr_ptr, 2 * hc, att, we, ea_csr, int(Bo != 1), alpha, graph.rowptr,
                 graph.col, graph.colptr, graph.row, graph.perm, dxlr, dxlr.data_ptr() + 4 * hc, datt, dbias, dwe, dea_csr,
                 ds, dz, part, wpart, epart, B, n, h, c, E, D, SLOPE, act, p, SEED, None)
        if want_dea:
            hip.call("mm_gatv2_edge_pack_bwd", dea_csr, graph.pos if El else None, graph.tgt if El else None, graph.rowptr,
                     graph.indeg, dea if El else None, Bo, n, El, E, D, fill_mean)
        res.append(dict(dxl=dxlr[..., :hc].clone(), dxr=dxlr[..., hc:].clone(), datt=datt - before[0],
                        dbias=dbias - before[1], dwe=dwe - before[2], dea=dea))
    torch.cuda.synchronize()
    return graph, dict(out=out, pre=pre, alpha=alpha, ea_csr=ea_csr), res, (datt, dbias, dwe)


def test_case_attributes_are_what_the_table_says():
    t2 = _case(2)
    ei = t2["ei"]
    dup = [k for k in range(ei.shape[1]) if (ei[:, k] == ei[:, 5]).all()]
    assert len(dup) == 2 and not torch.equal(t2["ea"][:, dup[0]], t2["ea"][:, dup[1]])
    assert t2["ea"].shape == (B, ei.shape[1], 3) and _case(4)["ea"].shape == (B, 64 * 63, 1)
    assert _case(1)["ea"].shape == (1, 0, 1) and _case(3)["ea"].shape == (1, 33, 8) and _case(5)["ea"].shape[0] == 1
    # the pack kernel against the written rule, exactly where the rule involves no arithmetic
    for case, fill in ((1, "mean"), (1, 1.0), (3, "mean")):
        n, h, c = SHAPES[case]
        t = _case(case)
        _, fwd, _, _ = _run_kernels(t, n, h, c, 0.0, False, fill)
        want = _pack64(t["ea"].double(), t["ei"], n, fill)
        assert torch.equal(fwd["ea_csr"].cpu().double(), want), case                # 0, the constant, or mean of one = itself
    ring = _run_kernels(_case(3), 33, 8, 16, 0.0, False)[1]["ea_csr"].cpu()
    assert torch.equal(ring[:, 0::2], ring[:, 1::2])                                # every row: the incoming edge, then its loop


@pytest.mark.parametrize("gelu", [False, True], ids=["linear", "gelu"])
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("case", CASES)
def test_gatv2_edge_fwd_bwd_match_fp64(case, p, gelu):
    case, fill = _split_case(case)
    n, h, c = SHAPES[case]
    t = _case(case)
    E = len(t["src"])
    keep = keep_scale(SEED, B * h * E, p).view(B, h, E)
    want = _oracle(t, n, h, c, keep, gelu, fill)
    graph, fwd, (bwd,), _ = _run_kernels(t, n, h, c, p, gelu, fill)
    assert graph.num_edges == E
    errs = {"out": _rel(fwd["out"], want["out"]), "alpha": _rel(fwd["alpha"].permute(0, 2, 1), want["alpha"])}
    assert _rel(fwd["ea_csr"], want["ea_csr"]) <= 2e-7                               # a mean of fp32 values: a few ulp
    for k in ("dxl", "dxr", "datt", "dbias", "dwe", "dea"):
        if k == "dea" and t["ea"].shape[1] == 0:
            continue                                                               # case 1 lists no edge: nothing to compare
        errs[k] = _rel(bwd[k].reshape(want[k].shape), want[k])
    for k, v in errs.items():
        print(f"ERR gatv2_edge case {case} fill {fill} p {p} gelu {int(gelu)} {k} {v:.3e}")
    bad = {k: v for k, v in errs.items() if not v <= BOUND[k]}
    assert not bad, bad
    assert all(b <= 5e-6 for b in BOUND.values())


@pytest.mark.parametrize("case,p,gelu", [(2, 0.25, True), (3, 0.0, False), (4, 0.0, False), (5, 0.25, True)])
def test_zero_edge_weight_gives_the_bits_of_the_plain_kernel(case, p, gelu):
    n, h, c = SHAPES[case]
    t = _case(case)
    _, fwd, _, _ = _run_kernels(t, n, h, c, p, gelu, we=torch.zeros_like(t["we"]))
    hip = _hip()
    graph = ops.gat_graph(t["ei"].cuda(), n)
    E, hc = graph.num_edges, h * c
    xlr = t["xlr"].cuda()
    out, alpha = _nan(B, n, hc), _nan(B, h, E)
    hip.call("mm_gatv2_fwd", xlr, xlr.data_ptr() + 4 * hc, 2 * hc, t["att"].cuda(), t["bias"].cuda(), graph.rowptr,
             graph.col, out, _nan(B, n, hc) if gelu else None, alpha, B, n, h, c, E, SLOPE, 1 if gelu else 0, p, SEED, None)
    torch.cuda.synchronize()
    assert torch.equal(fwd["out"], out) and torch.equal(fwd["alpha"], alpha)
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("case,p,gelu", [(2, 0.25, True), (4, 0.0, False), (5, 0.25, True)])
def test_two_backward_runs_give_the_same_bits_and_accumulate(case, p, gelu):
    n, h, c = SHAPES[case]
    _, _, (r1, r2), (datt, dbias, dwe) = _run_kernels(_case(case), n, h, c, p, gelu, runs=2)
    for k in ("dxl", "dxr", "dea"):
        assert torch.equal(r1[k], r2[k]), k
    # the first run added g to zeros, the second g to g: exactly 2 g in fp32 when both runs formed the same g
    assert torch.equal(datt, 2 * r1["datt"]) and torch.equal(dbias, 2 * r1["dbias"]) and torch.equal(dwe, 2 * r1["dwe"])
    for k in ("datt", "dbias", "dwe", "dea"):
        assert torch.count_nonzero(r1[k]) > 0, k


@pytest.mark.parametrize("case,p,gelu", [(2, 0.25, True), (3, 0.0, False)])
def test_null_edge_attr_gradient_pointer_leaves_the_other_outputs_unchanged(case, p, gelu):
    n, h, c = SHAPES[case]
    _, _, (full,), _ = _run_kernels(_case(case), n, h, c, p, gelu)
    _, _, (lean,), _ = _run_kernels(_case(case), n, h, c, p, gelu, want_dea=False)
    assert lean["dea"] is None and torch.isfinite(full["dea"]).all()
    for k in ("dxl", "dxr", "datt", "dbias", "dwe"):
        assert torch.equal(full[k], lean[k]), k
