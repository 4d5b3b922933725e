"""CPU: the fp64 references of oracle/fusion_tails.py against independent torch code, and the conditions of
tests/test_fusion_loss_edges_gpu.py (every e32 finite, and positive where it serves as that file's bound), before anything
runs on a GPU.

  - attn_1xk              nn.MultiheadAttention (eval, one query token, K = 1 .. 4 key tokens) at the GPU test's head counts
  - weighted_ce           F.cross_entropy(weight=, ignore_index=) with the out-of-range labels mapped to the ignore index
  - smoothed_ce, s = 0    F.cross_entropy;  s > 0: F.cross_entropy(label_smoothing=)
  - focal, gamma = 0      alpha * F.cross_entropy(reduction="none")
  - learned_fusion        the module formula of enhanced_models_v4.LearnedFusionModule, stacked and contracted by einsum
  - softmax2_concat, gate2_mix: F.softmax / torch.sigmoid forms

Everything here is fp64 against fp64: agreement to 1e-12 relative."""
import pytest
import torch
import torch.nn.functional as F

from oracle import fusion_tails as R

D64 = torch.float64
TIGHT = 1e-12


def _g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("E,nhead", R.ATTN_SHAPES)
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_attn_reference_is_multihead_attention_with_one_query(E, nhead, K):
    B = 5
    g = _g(E + nhead + K)
    mha = torch.nn.MultiheadAttention(E, nhead, dropout=0.3, batch_first=True).double().eval()
    with torch.no_grad():
        mha.in_proj_bias.copy_(torch.randn(3 * E, generator=g, dtype=D64) * 0.3)
    toks = torch.randn(B, K, E, generator=g, dtype=D64)
    with torch.no_grad():
        want, attw = mha(toks[:, :1], toks, toks, need_weights=True, average_attn_weights=True)
        ps = [F.linear(toks[:, j], mha.in_proj_weight, mha.in_proj_bias) for j in range(K)]
        ctx, aw = R.attn_1xk(ps, E, nhead, torch.ones(B, nhead, K, dtype=D64))
        got = mha.out_proj(ctx)
    assert R.rel_l2(got, want.squeeze(1)) < TIGHT and R.rel_l2(aw, attw.squeeze(1)) < TIGHT


def test_attn_reference_applies_the_keep_mask_to_the_probabilities():
    E, nhead, K, B = 12, 3, 3, 4
    g = _g(9)
    ps = [torch.randn(B, 3 * E, generator=g, dtype=D64) for _ in range(K)]
    keep = (torch.rand(B, nhead, K, generator=g) > 0.4).double() * 2.5
    ctx, aw = R.attn_1xk(ps, E, nhead, keep)
    full, aw1 = R.attn_1xk(ps, E, nhead, torch.ones(B, nhead, K, dtype=D64))
    assert torch.equal(aw, aw1)                                       # the reported weights are un-dropped
    solo = sum(R.attn_1xk([ps[0]] + ps[1:], E, nhead, keep * torch.eye(K, dtype=D64)[j])[0] for j in range(K))
    assert R.rel_l2(solo, ctx) < TIGHT and R.rel_l2(ctx, full) > 0.1


@pytest.mark.parametrize("B,C", R.LOSS_SHAPES)
@pytest.mark.parametrize("weighted", [False, True])
def test_weighted_ce_reference_is_cross_entropy_with_ignore_index(B, C, weighted):
    z, t = R.loss_inputs("order1", B, C)
    z = z.double()
    cw = 0.2 + torch.rand(C, generator=_g(B + C), dtype=D64) if weighted else None
    if B > 2:
        if weighted:
            cw[int(t[1])] = 0.0                                       # a zero weight on a class that occurs
        t = t.clone()
        t[0], t[B // 2], t[B - 1] = -100, C, 2 ** 32 + 1
        assert ((cw[t.clamp(0, C - 1)] if weighted else torch.ones(B)) * R.valid_rows(t, C)).sum() > 0
    zr, zt = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
    got = R.weighted_ce(zr, t, cw)
    got.backward()
    tt = torch.where(R.valid_rows(t, C), t, torch.full_like(t, -100))
    want = F.cross_entropy(zt, tt, weight=cw, ignore_index=-100)
    want.backward()
    assert abs(got.item() - want.item()) <= TIGHT * max(abs(want.item()), 1e-3)
    assert (zr.grad - zt.grad).abs().max().item() <= TIGHT
    assert torch.all(zr.grad[~R.valid_rows(t, C)] == 0)


@pytest.mark.parametrize("B,C", R.LOSS_SHAPES)
@pytest.mark.parametrize("s", [0.0, 0.1, 0.5])
def test_smoothed_ce_reference_is_cross_entropy(B, C, s):
    z, t = R.loss_inputs("order1", B, C)
    zr, zt = z.double().requires_grad_(True), z.double().requires_grad_(True)
    got = R.smoothed_ce(zr, t, s)
    got.backward()
    want = F.cross_entropy(zt, t, label_smoothing=s)
    want.backward()
    assert abs(got.item() - want.item()) <= TIGHT * max(abs(want.item()), 1e-3)
    assert (zr.grad - zt.grad).abs().max().item() <= TIGHT
    if B > 2:                                                         # dropped rows: no term, the divisor stays B
        bad = t.clone()
        bad[1] = C
        part = R.smoothed_ce(z.double(), bad, s)
        keep = torch.ones(B, dtype=torch.bool)
        keep[1] = False
        alone = F.cross_entropy(z.double()[keep], t[keep], label_smoothing=s, reduction="sum") / B
        assert abs(part.item() - alone.item()) <= TIGHT * max(abs(alone.item()), 1e-3)


@pytest.mark.parametrize("B,C", R.LOSS_SHAPES)
def test_focal_reference_at_gamma_0_is_alpha_times_cross_entropy(B, C):
    z, t = R.loss_inputs("order1", B, C)
    got = R.focal_per_sample(z.double(), t, 0.8, 0.0)
    want = 0.8 * F.cross_entropy(z.double(), t, reduction="none")
    assert (got - want).abs().max().item() <= TIGHT
    ce = F.cross_entropy(z.double(), t, reduction="none")             # gamma > 0: the notebook's formula
    for gamma in (0.5, 1.0, 2.0):
        want = 0.25 * (1 - torch.exp(-ce)) ** gamma * ce
        assert (R.focal_per_sample(z.double(), t, 0.25, gamma) - want).abs().max().item() <= TIGHT


@pytest.mark.parametrize("M", [2, 3])
@pytest.mark.parametrize("T", [0.7, 0.05])
def test_learned_fusion_reference_is_the_module_formula(M, T):
    c = R.learned_fusion_case(M, 17, 65, T)
    feats = [f.double() for f in c["feats"]]
    fused, w = R.learned_fusion(feats, c["dyn"].double(), c["logits"].double(), c["temp"].double())
    temp = c["temp"].double()
    static = F.softmax(c["logits"].double() / temp, dim=0)
    dynamic = F.softmax(c["dyn"].double() / temp, dim=-1)
    weights = 0.5 * static.unsqueeze(0).expand_as(dynamic) + 0.5 * dynamic
    want = torch.einsum("bm,bmh->bh", weights, torch.stack(feats, dim=1))
    assert R.rel_l2(fused, want) < TIGHT and R.rel_l2(w, weights) < TIGHT
    assert (w.sum(1) - 1).abs().max().item() < TIGHT


def test_softmax2_concat_and_gate2_mix_references():
    c = R.s2c_case(7, 1, 130, 0.3, -0.8)
    out = R.softmax2_concat(c["a"].double(), c["c"].double(), c["pa"].double(), c["pc"].double())
    w0 = torch.sigmoid(c["pa"].double() - c["pc"].double())           # softmax of two = sigmoid of the difference
    assert R.rel_l2(out, torch.cat([w0 * c["a"].double(), (1 - w0) * c["c"].double()], 1)) < TIGHT
    c = R.gate_case(6, 65, 1)
    comb, gate = R.gate2_mix(c["g"].double(), c["erp"].double(), c["pw"].double(), c["conn"].double(), c["boost"])
    g0 = torch.sigmoid(c["g"].double()[:, :1] - c["g"].double()[:, 1:])
    want = torch.cat([g0 * c["erp"].double() + (1 - g0) * c["pw"].double(), 1.5 * c["conn"].double()], 1)
    assert R.rel_l2(comb, want) < TIGHT and R.rel_l2(gate, torch.cat([g0, 1 - g0], 1)) < TIGHT


# ---------------------------------------------------------------------------- e32: the conditions of the GPU test's bounds
def _loss_calls(B):
    return [("weighted", {}), ("weighted", dict(cw=True))] + \
           [("focal", dict(alpha=a, gamma=gm, scale=sc)) for gm in (0.0, 0.5, 1.0, 2.0) for a, sc in ((0.8, 1.0 / B), (0.25, 1.0))] + \
           [("smoothed", dict(s=s)) for s in (0.0, 0.1, 0.5)]


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("B,C", R.FAMILY_SHAPES)
def test_loss_e32_is_finite_and_positive_in_every_family(family, B, C):
    z, t = R.loss_inputs(family, B, C)
    for kind, kw in _loss_calls(B):
        kw = dict(kw)
        if kw.pop("cw", False):
            kw["cw"] = 0.2 + torch.rand(C, generator=_g(C))
        want, e32 = R.loss_case(kind, z, t, **kw)
        for k, e in e32.items():
            print(f"E32 {family} B{B} C{C} {kind} {kw} {k} {e:.3e}")
            assert torch.isfinite(want[k]).all() and e == e and e < 1e-2, (kind, kw, k, e)
            if k != "loss":                                           # a scalar can round exactly; the tensors cannot
                assert e > 0, (kind, kw, k)
    if family == "confident":                                         # every row is confident: ce < 2 C exp(-6)
        ce = F.cross_entropy(z.double(), t, reduction="none")
        assert ce.max().item() < 2 * C * 2.5e-3 and ce.min().item() > 0


def test_loss_e32_with_dropped_rows():
    B, C = 257, 5
    z, t = R.loss_inputs("order1", B, C)
    t = t.clone()
    for b, lab in R.BAD_LABELS.items():
        t[b] = lab
    for kind, kw in _loss_calls(B):
        kw = dict(kw)
        if kw.pop("cw", False):
            kw["cw"] = 0.2 + torch.rand(C, generator=_g(C))
        want, e32 = R.loss_case(kind, z, t, **kw)
        assert torch.all(want["dl"][list(R.BAD_LABELS)] == 0)
        assert all(0 <= e < 1e-5 for e in e32.values()), e32


def test_fusion_e32_is_finite():
    rows = []
    for M in (2, 3):
        for B, H in R.LF_SHAPES:
            for T in (0.7, 0.05):
                rows.append((f"lf M{M} B{B} H{H} T{T}", R.case_e32(R.learned_fusion_eval, R.learned_fusion_case(M, B, H, T))[1]))
    for B, Ha, Hc in R.S2C_SHAPES[:3]:
        for pa, pc in R.S2C_LOGITS:
            rows.append((f"s2c {B} {Ha} {Hc} {pa}", R.case_e32(R.s2c_eval, R.s2c_case(B, Ha, Hc, pa, pc))[1]))
    for B, H in R.GATE_SHAPES[:3]:
        for mult in (1, 100):
            rows.append((f"gate {B} {H} x{mult}", R.case_e32(R.gate_eval, R.gate_case(B, H, mult))[1]))
    for E, nhead in R.ATTN_SHAPES:
        for K in (1, 2, 3, 4):
            c = R.attn_case(E, nhead, 5, K)
            rows.append((f"attn E{E} h{nhead} K{K}", R.case_e32(R.attn_eval, c, torch.ones(5, nhead, K))[1]))
    for tag, e32 in rows:
        for k, e in e32.items():
            print(f"E32 {tag} {k} {e:.3e}")
            assert e == e and e < float("inf"), (tag, k)
