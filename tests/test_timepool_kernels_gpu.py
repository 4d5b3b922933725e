"""The four tail kernels of the EEG baselines (csrc/timepool.hip: "mm_timepool_max_fwd", "mm_timepool_max_bwd",
"mm_timepool_avg_fwd", "mm_timepool_avg_bwd") against an fp64 restatement of their formulas (include/mmeeg_hip.h).

Operands are rounded to bf16 beforehand, so the fp64 reference is exact on the values the kernels see.  Shapes (B, L, P):
a single row, L < bins, overlapping bins, exactly one time chunk of the max kernel (64 rows), a chunk plus one row, several
chunks with the cross-wave merge, and a column-tile remainder (P = 48, 144 against tiles of 64).

Bounds: fp32 outputs rel-L2 <= 1e-5 against fp64 (tests/test_igemm1d_gpu.py records 3e-8 ... 5.4e-7 for the same fp32
accumulation: about 20 x the project's measured worst); dx of the max tail, bf16: one bf16 rounding, |got - want| <=
2^-8 |want| + 1e-30.  The arg-max must attain the fp64 maximum within 1e-5 max|y|, and the backward is checked GIVEN the
kernel's own arg-max, so no case is left out.

Measured on MI355X, worst rel-L2 over the shapes (a run prints every figure): max tail pooled 7.2e-8 (4.6e-7 in the
dropped-winner case, whose maxima are small), dw 5.5e-8, dbias 5.3e-8; avg tail xbin 2.6e-8, pooled 1.9e-7, dx 2.2e-7,
dw 1.0e-7, dbias 1.2e-7.  dx of the max tail met the one-rounding bound on every element.
"""
import pytest
import torch

from multimodal_eeg_fmri_amd import _hip as hip
from oracle.dropout_replica import keep_scale
from oracle.fixtures import seeded_randn

gpu = pytest.mark.gpu

K = 128
BINS = 4
SHAPES = [(1, 1, 16), (3, 3, 32), (2, 11, 144), (8, 64, 128), (2, 65, 32), (3, 200, 48)]
F32_BOUND = 1e-5


def _bf(t):
    return t.to(torch.bfloat16)


def _rel(got, want):
    got, want = got.detach().cpu().double(), want.double()
    return ((got - want).norm() / want.norm().clamp_min(1e-300)).item()


def _max_inputs(B, L, P, seed, bias_scale=0.1):
    x = _bf(seeded_randn(seed, B, L, K))
    w = _bf(seeded_randn(seed + 1, P, K) * 0.1)
    bias = seeded_randn(seed + 2, P) * bias_scale
    return x, w, bias


def _y64(x, w, bias, mask=None):
    y = x.double() @ w.double().t() + bias.double()
    return y if mask is None else y * mask.double()


def _max_fwd(x, w, bias, p=0.0, seed=0):
    B, L, _ = x.shape
    P = w.shape[0]
    pooled = torch.full((B, P), float("nan"), device="cuda")
    arg = torch.full((B, P), -1, dtype=torch.int32, device="cuda")
    hip.call("mm_timepool_max_fwd", x.cuda(), w.cuda(), bias.cuda(), pooled, arg, B, L, K, P, float(p), int(seed), None)
    return pooled, arg


def _max_bwd(dpooled, arg, x, w, p=0.0, seed=0, dw=None, dbias=None):
    B, L, _ = x.shape
    P = w.shape[0]
    dx = torch.full((B, L, K), float("nan"), dtype=torch.bfloat16, device="cuda")
    dw = torch.zeros(P, K, device="cuda") if dw is None else dw
    dbias = torch.zeros(P, device="cuda") if dbias is None else dbias
    hip.call("mm_timepool_max_bwd", dpooled.cuda(), arg, x.cuda(), w.cuda(), dx, dw, dbias, B, L, K, P, float(p), int(seed), None)
    return dx, dw, dbias


def _check_max(B, L, P, p, seed, bias_scale=0.1, bias=None, tag=""):
    """forward against fp64, then the backward given the kernel's own arg-max -> (y64, mask, arg on the CPU)"""
    x, w, b0 = _max_inputs(B, L, P, seed, bias_scale)
    bias = b0 if bias is None else bias
    mask = keep_scale(seed + 7, B * L * P, p).view(B, L, P) if p > 0 else torch.ones(B, L, P)
    y = _y64(x, w, bias, mask)
    pooled, arg = _max_fwd(x, w, bias, p, seed + 7)
    pooled2, arg2 = _max_fwd(x, w, bias, p, seed + 7)
    assert torch.equal(pooled, pooled2) and torch.equal(arg, arg2), "two forward launches differ"
    a = arg.cpu().long()
    assert ((a >= 0) & (a < L)).all()
    want = y.max(dim=1).values
    e_pool = _rel(pooled, want)
    at = y.gather(1, a.unsqueeze(1)).squeeze(1)
    assert (at >= want - 1e-5 * y.abs().max()).all(), "arg-max does not attain the maximum"
    # backward, given arg
    dpooled = seeded_randn(seed + 3, B, P)
    g = dpooled.double() * mask.double().gather(1, a.unsqueeze(1)).squeeze(1)
    onehot = torch.zeros(B, L, P, dtype=torch.float64).scatter_(1, a.unsqueeze(1), g.unsqueeze(1))
    dx_w = onehot @ w.double()
    dw_w = torch.einsum("blp,blk->pk", onehot, x.double())
    db_w = g.sum(0)
    dx, dw, dbias = _max_bwd(dpooled, arg, x, w, p, seed + 7)
    dx2, dw2, dbias2 = _max_bwd(dpooled, arg, x, w, p, seed + 7)
    assert torch.equal(dx.view(torch.int16), dx2.view(torch.int16)) and torch.equal(dw, dw2) and torch.equal(dbias, dbias2)
    dxc = dx.cpu().double()
    assert torch.isfinite(dxc).all(), "a row of dx was not written"
    assert ((dxc - dx_w).abs() <= 2.0 ** -8 * dx_w.abs() + 1e-30).all(), ((dxc - dx_w).abs() / dx_w.abs().clamp_min(1e-30)).max()
    e_dw = _rel(dw, dw_w) if dw_w.norm() > 0 else float(dw.abs().max())
    e_db = _rel(dbias, db_w) if db_w.norm() > 0 else float(dbias.abs().max())
    print(f"timepool max {tag}B{B} L{L} P{P} p{p}: pooled {e_pool:.2e} dw {e_dw:.2e} dbias {e_db:.2e}")
    assert e_pool <= F32_BOUND and e_dw <= F32_BOUND and e_db <= F32_BOUND
    return y, mask, a


@gpu
@pytest.mark.parametrize("B,L,P", SHAPES)
def test_max_tail_forward_and_backward_vs_fp64(B, L, P):
    _check_max(B, L, P, 0.0, 300 + L)


@gpu
@pytest.mark.parametrize("B,L,P", SHAPES)
def test_max_tail_with_dropout_vs_fp64(B, L, P):
    """p = 0.5: the mask of oracle.dropout_replica at index (b L + t) P + n, the same in forward and backward"""
    _check_max(B, L, P, 0.5, 400 + L)


def _dropped_winner_case():
    """(3, 200, 48), p = 0.5, bias = -3 std(y): most kept values are negative, so an exact 0 of a dropped element often wins.
    A kept winner needs a projection above 3 std among the ~L / 2 kept rows of its column (12 % of the columns at L = 200,
    4 % at L = 64: hence the long shape); seed 521 gives 78 % dropped and 22 % kept winners."""
    B, L, P, seed = 3, 200, 48, 521
    x, w, _ = _max_inputs(B, L, P, seed)
    std = (x.double() @ w.double().t()).std().item()
    return B, L, P, seed, torch.full((P,), -3.0 * std)


def test_dropped_winner_case_has_both_kinds_of_winners():
    """CPU side of the case below: >= 10 % of the columns are won by a dropped element (value 0, gradient 0) and >= 10 % by a
    kept one, on the reference"""
    B, L, P, seed, bias = _dropped_winner_case()
    x, w, _ = _max_inputs(B, L, P, seed)
    mask = keep_scale(seed + 7, B * L * P, 0.5).view(B, L, P)
    best = _y64(x, w, bias, mask).max(dim=1).values
    assert (best == 0).double().mean() >= 0.10 and (best > 0).double().mean() >= 0.10


@gpu
def test_max_tail_dropped_elements_compete_as_zeros():
    B, L, P, seed, bias = _dropped_winner_case()
    y, mask, a = _check_max(B, L, P, 0.5, seed, bias=bias, tag="dropped-winner ")
    best = y.max(dim=1).values
    dropped_at = mask.gather(1, a.unsqueeze(1)).squeeze(1) == 0
    assert (best == 0).double().mean() >= 0.10 and (best > 0).double().mean() >= 0.10
    # where a zero wins clearly (no kept value within 1e-4 of it), the kernel's winner is a dropped element - and the FIRST one
    kept_near = ((y.abs() < 1e-4) & (mask > 0)).any(dim=1)
    clear = (best == 0) & ~kept_near
    assert clear.any() and dropped_at[clear].all()
    first_dropped = (mask == 0).double().argmax(dim=1)
    assert torch.equal(a[clear], first_dropped[clear])


@gpu
def test_max_tail_exact_ties_go_to_the_smaller_index():
    """duplicated time rows (p = 0) give bit-equal projections; the pairs sit in one lane group (4, 6), in two waves (5, 41)
    and in two time chunks (17, 150) of a (3, 200, 48) problem.  Scaled by 16 (exact in bf16), the duplicates win the
    columns whose projection of that row is clearly positive: nearly half of them."""
    B, L, P, seed = 3, 200, 48, 610
    x, w, bias = _max_inputs(B, L, P, seed)
    pairs = [(4, 6), (5, 41), (17, 150)]
    x = x.float()
    for b, (t1, t2) in enumerate(pairs):
        x[b, t1] = x[b, t1] * 16.0
        x[b, t2] = x[b, t1]
    x = _bf(x)
    y = _y64(x, w, bias)
    best = y.max(dim=1).values
    for b, (t1, t2) in enumerate(pairs):
        dup = (y[b, t1] == best[b]) & (y[b, t2] == best[b])
        assert dup.double().mean() >= 0.25, (b, dup.double().mean())
    pooled, arg = _max_fwd(x, w, bias)
    a = arg.cpu().long()
    for b, (t1, t2) in enumerate(pairs):
        dup = (y[b, t1] == best[b]) & (y[b, t2] == best[b])
        assert (a[b][dup] == t1).all(), (b, a[b][dup])
    at = y.gather(1, a.unsqueeze(1)).squeeze(1)
    assert (at >= best - 1e-5 * y.abs().max()).all()
    assert _rel(pooled, best) <= F32_BOUND


@gpu
def test_max_tail_gradients_accumulate():
    """dw / dbias are added into: a second launch into the same buffers doubles them exactly"""
    B, L, P = 2, 11, 144
    x, w, bias = _max_inputs(B, L, P, 700)
    _, arg = _max_fwd(x, w, bias)
    dpooled = seeded_randn(703, B, P)
    _, dw, db = _max_bwd(dpooled, arg, x, w)
    dw1, db1 = dw.clone(), db.clone()
    _max_bwd(dpooled, arg, x, w, dw=dw, dbias=db)
    assert torch.equal(dw, 2 * dw1) and torch.equal(db, 2 * db1)


def _bins(L, bins=BINS):
    return [((i * L) // bins, -((-(i + 1) * L) // bins)) for i in range(bins)]


@gpu
@pytest.mark.parametrize("B,L,P", SHAPES)
def test_avg_tail_forward_and_backward_vs_fp64(B, L, P):
    seed = 800 + L
    x = _bf(seeded_randn(seed, B, L, K)).float()
    w = _bf(seeded_randn(seed + 1, P, K) * 0.1).float()
    bias = seeded_randn(seed + 2, P) * 0.1
    spans = _bins(L)
    if L == 11:
        assert spans == [(0, 3), (2, 6), (5, 9), (8, 11)]
    xbin_w = torch.stack([x[:, a:b].double().mean(1) for a, b in spans], dim=1)                       # (B, bins, K)
    pooled_w = (xbin_w @ w.double().t() + bias.double()).permute(0, 2, 1).reshape(B, P * BINS)           # Flatten of (B, P, bins)
    xbin = torch.full((B, BINS, K), float("nan"), device="cuda")
    pooled = torch.full((B, P * BINS), float("nan"), device="cuda")
    xc, wc, bc = x.cuda(), w.cuda(), bias.cuda()
    hip.call("mm_timepool_avg_fwd", xc, wc, bc, xbin, pooled, B, L, K, P, BINS)
    xbin2, pooled2 = torch.empty_like(xbin), torch.empty_like(pooled)
    hip.call("mm_timepool_avg_fwd", xc, wc, bc, xbin2, pooled2, B, L, K, P, BINS)
    assert torch.equal(xbin, xbin2) and torch.equal(pooled, pooled2)
    # the same function as projecting every step and pooling afterwards (what the notebook computes)
    steps = (x.double() @ w.double().t() + bias.double()).permute(0, 2, 1)                             # (B, P, L)
    late = torch.nn.functional.adaptive_avg_pool1d(steps, BINS).reshape(B, P * BINS)
    assert _rel(pooled_w, late) < 1e-12
    dpooled = seeded_randn(seed + 3, B, P * BINS)
    d3 = dpooled.double().view(B, P, BINS)
    u = torch.einsum("bpi,pk->bik", d3, w.double())
    dx_w = torch.zeros(B, L, K, dtype=torch.float64)
    for i, (a, b) in enumerate(spans):
        dx_w[:, a:b] += (u[:, i] / (b - a)).unsqueeze(1)
    dw_w = torch.einsum("bpi,bik->pk", d3, xbin_w)
    db_w = d3.sum(dim=(0, 2))
    dx = torch.full((B, L, K), float("nan"), device="cuda")
    dw, db = torch.zeros(P, K, device="cuda"), torch.zeros(P, device="cuda")
    hip.call("mm_timepool_avg_bwd", dpooled.cuda(), xbin, wc, dx, dw, db, B, L, K, P, BINS)
    dx2, dw2, db2 = torch.empty_like(dx), torch.zeros_like(dw), torch.zeros_like(db)
    hip.call("mm_timepool_avg_bwd", dpooled.cuda(), xbin, wc, dx2, dw2, db2, B, L, K, P, BINS)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2)
    assert torch.isfinite(dx).all(), "a row of dx was not written"
    errs = {"xbin": _rel(xbin, xbin_w), "pooled": _rel(pooled, pooled_w), "dx": _rel(dx, dx_w), "dw": _rel(dw, dw_w),
            "dbias": _rel(db, db_w)}
    print(f"timepool avg B{B} L{L} P{P}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= F32_BOUND for v in errs.values()), errs
    hip.call("mm_timepool_avg_bwd", dpooled.cuda(), xbin, wc, None, dw, db, B, L, K, P, BINS)      # accumulated into
    assert torch.equal(dw, 2 * dw2) and torch.equal(db, 2 * db2)


@gpu
def test_unsupported_sizes_are_refused():
    B, L, P = 2, 8, 32
    x16, w16 = torch.zeros(B, L, K, dtype=torch.bfloat16, device="cuda"), torch.zeros(544, K, dtype=torch.bfloat16, device="cuda")
    x32, w32 = torch.zeros(B, L, K, device="cuda"), torch.zeros(544, K, device="cuda")
    bias, big = torch.zeros(544, device="cuda"), torch.zeros(B, 544 * BINS, device="cuda")
    arg = torch.zeros(B, 544, dtype=torch.int32, device="cuda")
    xbin = torch.zeros(B, BINS, K, device="cuda")
    for k, p in ((64, P), (K, 24), (K, 528), (K, 0)):
        with pytest.raises(hip.HipLibraryError, match="timepool_max_fwd"):
            hip.call("mm_timepool_max_fwd", x16, w16, bias, big, arg, B, L, k, p, 0.0, 0, None)
        with pytest.raises(hip.HipLibraryError, match="timepool_max_bwd"):
            hip.call("mm_timepool_max_bwd", big, arg, x16, w16, torch.empty_like(x16), w32, bias, B, L, k, p, 0.0, 0, None)
        with pytest.raises(hip.HipLibraryError, match="timepool_avg_fwd"):
            hip.call("mm_timepool_avg_fwd", x32, w32, bias, xbin, big, B, L, k, p, BINS)
        with pytest.raises(hip.HipLibraryError, match="timepool_avg_bwd"):
            hip.call("mm_timepool_avg_bwd", big, xbin, w32, torch.empty_like(x32), w32.clone(), bias.clone(), B, L, k, p, BINS)
    with pytest.raises(hip.HipLibraryError, match="L=0"):
        hip.call("mm_timepool_max_fwd", x16, w16, bias, big, arg, B, 0, K, P, 0.0, 0, None)
    with pytest.raises(hip.HipLibraryError, match="bins"):
        hip.call("mm_timepool_avg_fwd", x32, w32, bias, xbin, big, B, L, K, P, 9)
