"""Plain-torch references of the fusion tails (csrc/fusion.hip) and the three classification losses (csrc/losses.hip),
one per operation, each written from the formula in the kernel's header comment.  Every function computes in the dtype
of its operands: on fp64 leaves it is the reference (gradients by torch.autograd), on fp32 copies of the same inputs it
is the "same formula in plain fp32" whose rel-L2 distance from the fp64 result is e32, the unit of the tests' bounds
(tests/test_fusion_tails_host.py computes it without a GPU, tests/test_fusion_loss_edges_gpu.py uses it):

    bound = max(16 * e32, floor),   floor = the figure tests/test_head_kernels_gpu.py allows for the quantity at order 1

The input families and shape lists of the loss tests live here too, so that the host test and the GPU test see the same
tensors."""
import math

import torch

D64 = torch.float64


def rel_l2(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    den = want.norm().item()
    return (got - want).norm().item() / (den if den > 0 else 1.0)


def bound(e32, floor):
    return max(16.0 * e32, floor)


# ------------------------------------------------------------------------------------------------------ fusion tails
def softmax2_concat(a, c, pa, pc):
    """out[b] = [w0 a[b] | w1 c[b]], (w0, w1) = softmax(pa[0], pc[0])"""
    w = torch.softmax(torch.cat([pa, pc]), 0)
    return torch.cat([w[0] * a, w[1] * c], dim=1)


def learned_fusion(feats, dyn, logits, temp):
    """w = 0.5 softmax(logits / T) + 0.5 softmax(dyn[b] / T); fused[b] = sum_m w[b][m] feat_m[b]; returns (fused, w)"""
    w = 0.5 * torch.softmax(logits / temp, 0).unsqueeze(0) + 0.5 * torch.softmax(dyn / temp, 1)
    fused = sum(w[:, m:m + 1] * feats[m] for m in range(len(feats)))
    return fused, w


def attn_1xk(ps, E, nhead, keep):
    """one query (token 0's q) over K key/value tokens, per head.  ps = K tensors (B, 3E) = [q | k | v]; keep (B, nhead, K)
    multiplies the probabilities before the mix (dropout keep * 1 / (1 - p)); returns ctx (B, E) and the head-averaged,
    un-dropped probabilities (B, K)"""
    B = ps[0].shape[0]
    dh = E // nhead
    q = ps[0][:, :E].view(B, nhead, dh)
    k = torch.stack([p[:, E:2 * E].view(B, nhead, dh) for p in ps], dim=2)          # (B, h, K, dh)
    v = torch.stack([p[:, 2 * E:].view(B, nhead, dh) for p in ps], dim=2)
    pr = torch.softmax((q.unsqueeze(2) * k).sum(-1) / math.sqrt(dh), dim=-1)        # (B, h, K)
    ctx = ((pr * keep).unsqueeze(-1) * v).sum(2).reshape(B, E)
    return ctx, pr.mean(1)


def gate2_mix(g, erp, pw, conn, boost):
    """gate = softmax(g[b][0:2]); comb[b] = [gate0 erp + gate1 pw | conn * boost]; returns (comb, gate)"""
    gate = torch.softmax(g, 1)
    return torch.cat([gate[:, :1] * erp + gate[:, 1:] * pw, conn * boost], dim=1), gate


# ------------------------------------------------------------------------------------------------------------ losses
def valid_rows(t, C):
    """the label rule of csrc/losses.hip: a row counts when its 64-bit label lies in [0, C)"""
    return (t >= 0) & (t < C)


def _row_terms(z, t, valid):
    """m, log(se), z[t] per row as the kernels form them (se = sum_c exp(z_c - m)); a dropped row reads class 0"""
    ts = torch.where(valid, t, torch.zeros_like(t))
    m = z.max(dim=1).values
    lse = m + torch.log(torch.exp(z - m[:, None]).sum(1))
    return lse, z.gather(1, ts[:, None]).squeeze(1), ts


def weighted_ce(z, t, cw=None, valid=None):
    """sum_b w[t_b] ce_b / sum_b w[t_b] over the valid rows, ce_b = m + log(se) - z[t_b]"""
    valid = valid_rows(t, z.shape[1]) if valid is None else valid
    lse, zt, ts = _row_terms(z, t, valid)
    w = (cw[ts] if cw is not None else torch.ones_like(zt)) * valid.to(z.dtype)
    return (w * (lse - zt)).sum() / w.sum()


def focal_per_sample(z, t, alpha, gamma, valid=None):
    """fl_b = alpha (1 - exp(-ce_b))^gamma ce_b (0 on a dropped row).  (1 - pt)^gamma is 0 where 1 - pt <= 0 (gamma > 0),
    written so that autograd gives that branch the gradient 0 and not 0 * inf"""
    valid = valid_rows(t, z.shape[1]) if valid is None else valid
    lse, zt, _ = _row_terms(z, t, valid)
    ce = lse - zt
    q = (1.0 - torch.exp(-ce)).clamp_min(0.0)
    if gamma == 0.0:
        qg = torch.ones_like(q)
    else:
        pos = q > 0
        qg = torch.where(pos, torch.where(pos, q, torch.ones_like(q)) ** gamma, torch.zeros_like(q))
    return alpha * qg * ce * valid.to(z.dtype)


def smoothed_ce(z, t, s, valid=None):
    """sum over the valid rows of (1 - s) nll_b + s mean_c(-logp_bc), divided by B (dropped rows included in B)"""
    valid = valid_rows(t, z.shape[1]) if valid is None else valid
    lse, zt, _ = _row_terms(z, t, valid)
    per = (1.0 - s) * (lse - zt) + s * (lse - z.sum(1) / z.shape[1])
    return (per * valid.to(z.dtype)).sum() / z.shape[0]


LOSS_SHAPES = [(1, 1), (1, 2), (255, 2), (256, 5), (257, 5), (513, 300)]
FAMILY_SHAPES = [(257, 5), (255, 2)]
FAMILIES = ["order1", "offset+", "offset-", "spread", "confident"]
BAD_LABELS = {0: -100, 100: 5, 256: 2 ** 32 + 1}            # at (257, 5): ignore_index, C, a label whose low word is class 1


def loss_inputs(family, B, C, seed=0):
    """(logits fp32 (B, C), int64 targets in [0, C)) of one input family"""
    g = torch.Generator().manual_seed(1000 * B + C + 7 * seed)
    z = 2.0 * torch.randn(B, C, generator=g)
    t = torch.randint(0, C, (B,), generator=g, dtype=torch.int64)
    if family == "order1":
        pass
    elif family == "offset+":
        z = z + 300.0
    elif family == "offset-":
        z = z - 300.0
    elif family == "spread":
        z = 30.0 * torch.randn(B, C, generator=g)
    elif family == "confident":                              # target logit = the others' maximum + U[6, 12)
        margin = 6.0 + 6.0 * torch.rand(B, generator=g)
        other = z.clone()
        other.scatter_(1, t[:, None], float("-inf"))
        z.scatter_(1, t[:, None], (other.max(1).values + margin)[:, None])
    else:
        raise ValueError(family)
    return z, t


def loss_eval(kind, z, t, dtype, cw=None, valid=None, alpha=1.0, gamma=0.0, scale=1.0, s=0.0):
    """one loss in ``dtype`` on copies of the fp32 inputs: dict(loss=, per=(focal only), dl=).  focal: loss = scale * sum_b
    fl_b and dl is the gradient of sum_b fl_b (the kernel's un-reduced d fl_b / d z)"""
    zr = z.to(dtype).clone().requires_grad_(True)
    cwd = cw.to(dtype) if cw is not None else None
    out = {}
    if kind == "weighted":
        loss = weighted_ce(zr, t, cwd, valid)
        loss.backward()
    elif kind == "focal":
        per = focal_per_sample(zr, t, alpha, gamma, valid)
        per.sum().backward()
        loss = scale * per.sum()
        out["per"] = per.detach()
    elif kind == "smoothed":
        loss = smoothed_ce(zr, t, s, valid)
        loss.backward()
    else:
        raise ValueError(kind)
    out["loss"], out["dl"] = loss.detach().reshape(1), zr.grad
    return out


def loss_case(kind, z, t, **kw):
    """(fp64 reference, {quantity: e32}) of one loss call"""
    want, c32 = loss_eval(kind, z, t, D64, **kw), loss_eval(kind, z, t, torch.float32, **kw)
    return want, {k: rel_l2(c32[k], want[k]) for k in want}


# ------------------------------------------------------------------------- fusion cases: inputs and (outputs, gradients)
LF_SHAPES = [(1, 1), (5, 63), (17, 65), (33, 130)]
S2C_SHAPES = [(1, 1, 1), (3, 64, 1), (7, 1, 130), (2100, 128, 130)]
S2C_LOGITS = [(0.3, -0.8), (100.0, -100.0), (-100.0, 100.0)]
GATE_SHAPES = [(1, 1), (5, 63), (6, 65), (1030, 256)]
ATTN_SHAPES = [(4, 4), (96, 1), (96, 3), (80, 5), (128, 16)]


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * 31 ** i for i, k in enumerate(key)) % (2 ** 31))


def _evaluate(fn, inputs, douts, dtype, names, gnames):
    """fn(*leaves) -> tuple of outputs; the gradients of sum_i <out_i, dout_i> over the outputs that have a dout"""
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in inputs]
    outs = fn(*leaves)
    sum((o * d.to(dtype)).sum() for o, d in zip(outs, douts) if d is not None).backward()
    res = {n: o.detach() for n, o in zip(names, outs)}
    res.update({n: l.grad for n, l in zip(gnames, leaves)})
    return res


def learned_fusion_case(M, B, H, T):
    g = _gen(M, B, H)
    return dict(feats=[torch.randn(B, H, generator=g) for _ in range(M)], dyn=2.0 * torch.randn(B, M, generator=g),
                logits=torch.randn(M, generator=g), temp=torch.tensor([T]), dfused=torch.randn(B, H, generator=g))


def learned_fusion_eval(c, dtype):
    M = len(c["feats"])
    return _evaluate(lambda *l: learned_fusion(l[:M], l[M], l[M + 1], l[M + 2]), c["feats"] + [c["dyn"], c["logits"], c["temp"]],
                     [c["dfused"], None], dtype, ["fused", "weights"], [f"df{m}" for m in range(M)] + ["ddyn", "dlogits", "dtemp"])


def s2c_case(B, Ha, Hc, pa, pc):
    g = _gen(B, Ha, Hc)
    return dict(a=torch.randn(B, Ha, generator=g), c=torch.randn(B, Hc, generator=g), pa=torch.tensor([pa]),
                pc=torch.tensor([pc]), dout=torch.randn(B, Ha + Hc, generator=g))


def s2c_eval(c, dtype):
    return _evaluate(lambda a, cc, pa, pc: (softmax2_concat(a, cc, pa, pc),), [c["a"], c["c"], c["pa"], c["pc"]], [c["dout"]],
                     dtype, ["out"], ["da", "dc", "dpa", "dpc"])


def gate_case(B, H, mult):
    g = _gen(B, H, 3)
    return dict(g=2.0 * mult * torch.randn(B, 2, generator=g), erp=torch.randn(B, H, generator=g),
                pw=torch.randn(B, H, generator=g), conn=torch.randn(B, H, generator=g),
                dcomb=torch.randn(B, 2 * H, generator=g), boost=1.5)


def gate_eval(c, dtype):
    return _evaluate(lambda g, e, p, cn: gate2_mix(g, e, p, cn, c["boost"]), [c["g"], c["erp"], c["pw"], c["conn"]],
                     [c["dcomb"], None], dtype, ["comb", "gate"], ["dg", "derp", "dpw", "dconn"])


def attn_case(E, nhead, B, K):
    g = _gen(E, nhead, B, K)
    return dict(ps=[torch.randn(B, 3 * E, generator=g) for _ in range(K)], dctx=torch.randn(B, E, generator=g), E=E,
                nhead=nhead)


def attn_eval(c, keep, dtype):
    K = len(c["ps"])
    return _evaluate(lambda *l: attn_1xk(l, c["E"], c["nhead"], keep.to(dtype)), c["ps"], [c["dctx"], None], dtype,
                     ["ctx", "attw"], [f"dp{j}" for j in range(K)])


def case_e32(evaluate, *args):
    """(fp64 reference dict, {quantity: e32}) of one fusion case"""
    want, c32 = evaluate(*args, D64), evaluate(*args, torch.float32)
    return want, {k: rel_l2(c32[k], want[k]) for k in want}
