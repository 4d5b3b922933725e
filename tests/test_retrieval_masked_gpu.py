"""Retrieval with ignored temporal neighbours (mm_retrieval_masked, ops.retrieval(radius=), retrieval_metrics(radius=))
against an exact host oracle of the contract in include/mmeeg_hip.h: d = |ggid[j] - qgid[q]| without wrap; s* = max over
{d == 0} of s(q, j), NaN skipped; ranks = 1 + #{d > R, s >= s*}, Ng without a positive; negatives = #{d > R}; top-k = the
k best rows of {d == 0 or d > R} by (score descending, index ascending), NaN never, unfilled (-1, -inf).
Inputs are multiples of 1/64 with the second half of every row zero (`exact_rows` of tests/test_retrieval_groups_gpu.py),
so every fp32 dot product is exact, ties are common and the fp64 oracle needs no tolerance."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
from multimodal_eeg_fmri_amd.bridge_utils import rank_summary, retrieval_metrics

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 4, 1), (5, 7, 4, 1), (130, 257, 36, 2), (37, 1000, 64, 3), (2049, 4100, 64, 2)]


def exact_rows(n, d, gen):
    x = torch.randint(-64, 65, (n, d), generator=gen).double() / 64.0
    x[:, d // 2:] = 0                                   # a coarse grid: ties are common
    return x


def id_dist(qg, gg):
    return np.abs(np.asarray(qg)[:, None].astype(np.int64) - np.asarray(gg)[None, :].astype(np.int64))


def ref_masked(S, qg, gg, R, k):
    """-> ranks, negatives, top-k indices, top-k scores"""
    nq, ng = S.shape
    d = id_dist(qg, gg)
    pos = (d == 0) & ~np.isnan(S)
    sstar = np.where(pos, S, -np.inf).max(1)
    sstar[~pos.any(1)] = np.nan
    neg = d > R
    with np.errstate(invalid="ignore"):
        r = 1 + ((S >= sstar[:, None]) & neg).sum(1)
    r[np.isnan(sstar)] = ng
    valid = ((d == 0) | neg) & ~np.isnan(S)
    Sm = np.where(valid, S, -np.inf)
    order = np.lexsort((np.broadcast_to(np.arange(ng), S.shape), -Sm), axis=1)[:, :k]
    filled = np.take_along_axis(valid, order, 1)
    return r, neg.sum(1), np.where(filled, order, -1), np.where(filled, np.take_along_axis(Sm, order, 1), -np.inf)


def timeline(nq, ng, R, gen):
    """gallery ids: runs of 50 consecutive positions with stride 50 + R, shuffled; query ids drawn from the gallery's, and
    for nq >= 30 every 17th query gets an id no gallery row has"""
    gid = (np.arange(ng) // 50) * (50 + R) + np.arange(ng) % 50
    gid = gid[torch.randperm(ng, generator=gen).numpy()]
    qid = gid[torch.randint(0, ng, (nq,), generator=gen).numpy()].copy()
    if nq >= 30:
        qid[::17] = gid.max() + 1000
    return torch.from_numpy(qid).to(torch.int32), torch.from_numpy(gid).to(torch.int32)


def masked_call(q, g, qg, gg, R, k=0, ranks=True, negatives=True):
    """the raw entry point on a workspace full of NaN (no initialisation is needed) -> (ranks, negatives, idx, score)"""
    nq, d = q.shape
    ng = g.shape[0]
    c = ctypes.c_int(0)
    _hip.call("mm_retrieval_masked_ws_floats", nq, ng, d, k, ctypes.addressof(c))
    ws = torch.full((c.value,), float("nan"), device="cuda")
    r = torch.full((nq,), -7, dtype=torch.int32, device="cuda") if ranks else None
    n = torch.full((nq,), -7, dtype=torch.int32, device="cuda") if negatives else None
    ti = torch.full((nq, k), -7, dtype=torch.int32, device="cuda") if k else None
    ts = torch.full((nq, k), 7.0, device="cuda") if k else None
    _hip.call("mm_retrieval_masked", q, g, qg.to(torch.int32).cuda(), gg.to(torch.int32).cuda(), int(R), r, n, ti, ts, ws,
              nq, ng, d, k)
    return r, n, ti, ts


def cpu(t):
    return None if t is None else t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(nq, ng, d, R):
    """inputs, fp64 scores and the oracle at k = min(5, ng), computed once per shape"""
    gen = torch.Generator().manual_seed(nq + 13 * ng)
    q64, g64 = exact_rows(nq, d, gen), exact_rows(ng, d, gen)
    qg, gg = timeline(nq, ng, R, gen)
    S = (q64 @ g64.T).numpy()
    k = min(5, ng)
    return dict(q=q64.float().cuda(), g=g64.float().cuda(), qg=qg, gg=gg, S=S, k=k, want=ref_masked(S, qg.numpy(), gg.numpy(), R, k))


@pytest.mark.parametrize("nq,ng,d,R", SHAPES)
def test_exact_contract_on_representable_inputs(nq, ng, d, R):
    c = case(nq, ng, d, R)
    q, g, qg, gg, k = c["q"], c["g"], c["qg"], c["gg"], c["k"]
    wr, wn, wi, ws = c["want"]
    r, n, ti, ts = masked_call(q, g, qg, gg, R, k)
    assert np.array_equal(cpu(r), wr) and np.array_equal(cpu(n), wn)
    assert np.array_equal(cpu(ti), wi) and np.array_equal(cpu(ts).astype(np.float64), ws)
    # the radius matters: the grouped rank (R = 0) of some query is worse, and the absent ids rank Ng
    r0 = ref_masked(c["S"], qg.numpy(), gg.numpy(), 0, 1)[0]
    ignored = ((id_dist(qg, gg) > 0) & (id_dist(qg, gg) <= R)).sum(1)
    print(f"({nq}, {ng}, {d}, R={R}): rank differs from R = 0 for {(wr != r0).sum()} queries, {ignored.mean():.2f} ignored rows per query, "
          f"{(wr == ng).sum()} rank Ng")
    assert (wr <= r0).all() and (nq < 5 or (wr != r0).any())
    no_pos = ~np.isin(qg.numpy(), gg.numpy())
    assert (wr[no_pos] == ng).all() and (nq < 30 or no_pos.any())
    # no ignored row in any list
    dsel = np.abs(qg.numpy().astype(np.int64)[:, None] - gg.numpy().astype(np.int64)[np.maximum(cpu(ti), 0)])
    assert (((dsel == 0) | (dsel > R)) | (cpu(ti) < 0)).all()
    # the same through ops.retrieval
    r2, i2, s2, n2 = ops.retrieval(q, g, k=k, q_groups=qg, g_groups=gg, radius=R, return_negatives=True)
    assert r2.dtype == i2.dtype == n2.dtype == torch.int64
    assert torch.equal(r2, r.long()) and torch.equal(n2, n.long()) and torch.equal(i2, ti.long()) and torch.equal(s2, ts)
    r3, i3, s3 = ops.retrieval(q, g, q_groups=qg, g_groups=gg, radius=R)
    assert i3 is None and s3 is None and torch.equal(r3, r.long())
    # deterministic
    again = masked_call(q, g, qg, gg, R, k)
    assert all(torch.equal(a, b) for a, b in zip(again, (r, n, ti, ts)))
    # every combination of optional outputs gives the same values
    rn, nn, tin, tsn = masked_call(q, g, qg, gg, R, k, ranks=False)
    assert rn is None and torch.equal(nn, n) and torch.equal(tin, ti) and torch.equal(tsn, ts)
    _, nx, tix, tsx = masked_call(q, g, qg, gg, R, k, ranks=False, negatives=False)
    assert nx is None and torch.equal(tix, ti) and torch.equal(tsx, ts)
    ry, ny, _, _ = masked_call(q, g, qg, gg, R, 0, negatives=False)
    assert ny is None and torch.equal(ry, r)
    rz, nz, _, _ = masked_call(q, g, qg, gg, R, 0)
    assert torch.equal(rz, r) and torch.equal(nz, n)
    _, i4, s4 = ops.retrieval(q, g, k=k, ranks=False, q_groups=qg, g_groups=gg, radius=R)
    assert torch.equal(i4, ti.long()) and torch.equal(s4, ts)


def test_the_longest_lists():
    nq, ng, d, R = 37, 1000, 64, 3
    c = case(nq, ng, d, R)
    wr, wn, wi, ws = ref_masked(c["S"], c["qg"].numpy(), c["gg"].numpy(), R, 16)
    r, n, ti, ts = masked_call(c["q"], c["g"], c["qg"], c["gg"], R, 16)
    assert np.array_equal(cpu(r), wr) and np.array_equal(cpu(n), wn)
    assert np.array_equal(cpu(ti), wi) and np.array_equal(cpu(ts).astype(np.float64), ws)
    _, _, tin, tsn = masked_call(c["q"], c["g"], c["qg"], c["gg"], R, 16, ranks=False, negatives=False)
    assert torch.equal(tin, ti) and torch.equal(tsn, ts)


@pytest.mark.parametrize("n", [300, 2049])
def test_radius_zero_is_the_grouped_ranks_and_the_ungrouped_top_k(n):
    d, k = 128, 10
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(2 * n, d, generator=gen, dtype=torch.float64)
    x = (x / x.norm(dim=1, keepdim=True)).float()
    q, g = x[:n].cuda(), x[n:].cuda()
    g[7] = g[3]                                      # an exact duplicate of a positive (a tie against the query)
    ids = torch.arange(n)
    want_r, _, _ = ops.retrieval(q, g, q_groups=ids, g_groups=ids)
    _, want_i, want_s = ops.retrieval(q, g, k=k, ranks=False)
    r, neg, ti, ts = masked_call(q, g, ids, ids, 0, k)
    assert torch.equal(r.long(), want_r)
    assert torch.equal(ti.long(), want_i) and torch.equal(ts.view(torch.int32), want_s.view(torch.int32))
    assert torch.equal(neg.cpu(), torch.full((n,), n - 1, dtype=torch.int32))
    _, _, tin, tsn = masked_call(q, g, ids, ids, 0, k, ranks=False, negatives=False)
    assert torch.equal(tin.long(), want_i) and torch.equal(tsn.view(torch.int32), want_s.view(torch.int32))
    # subject ids (several positives per query) at R = 0: the grouped ranks again
    sub = torch.randint(0, n // 4, (n,), generator=gen)
    want_r, _, _ = ops.retrieval(q, g, q_groups=sub, g_groups=sub)
    assert torch.equal(masked_call(q, g, sub, sub, 0)[0].long(), want_r)


def test_the_id_distance_does_not_wrap():
    n, d = 200, 64
    gen = torch.Generator().manual_seed(5)
    q64, g64 = exact_rows(n, d, gen), exact_rows(n, d, gen)
    lo, hi = -(2 ** 31), 2 ** 31 - 1
    ids = torch.where(torch.arange(n) % 2 == 0, torch.tensor(lo), torch.tensor(hi)).to(torch.int32)
    ids = ids[torch.randperm(n, generator=gen)]
    q, g = q64.float().cuda(), g64.float().cuda()
    want, _, _ = ops.retrieval(q, g, q_groups=ids, g_groups=ids)
    oracle = ref_masked((q64 @ g64.T).numpy(), ids.numpy(), ids.numpy(), 1, 5)
    assert np.array_equal(want.cpu().numpy(), oracle[0])
    for R in (1, 2 ** 31 - 1):                       # the two ids are 2^32 - 1 apart: never within any int32 radius
        r, neg, ti, ts = masked_call(q, g, ids, ids, R, 5)
        assert torch.equal(r.long(), want)
        assert np.array_equal(cpu(neg), oracle[1]) and (cpu(neg) == n // 2).all()
        assert np.array_equal(cpu(ti), oracle[2]) and np.array_equal(cpu(ts).astype(np.float64), oracle[3])


def test_what_an_ignored_row_holds_does_not_matter():
    nq, ng, d, R = 130, 257, 36, 2
    c = case(nq, ng, d, R)
    q, g, qg, gg, k = c["q"], c["g"], c["qg"], c["gg"], c["k"]
    S, (wr, wn, wi, ws) = c["S"], c["want"]
    dist = id_dist(qg, gg)
    ign = (dist > 0) & (dist <= R)
    best = np.where(dist == 0, S, -np.inf)
    rows = [i for i in range(nq) if ign[i].sum() >= 2 and best[i].max() > 0][:4]
    assert len(rows) == 4
    for i in rows:
        jpos = int(best[i].argmax())
        for fill in (2.0 * g[jpos], torch.full((d,), float("nan"), device="cuda")):
            g2 = g.clone()
            g2[torch.from_numpy(np.flatnonzero(ign[i])).cuda()] = fill
            r, n, ti, ts = masked_call(q, g2, qg, gg, R, k)
            assert r[i].item() == wr[i] and n[i].item() == wn[i]
            assert np.array_equal(cpu(ti[i]), wi[i]) and np.array_equal(cpu(ts[i]).astype(np.float64), ws[i])
            _, _, tin, tsn = masked_call(q, g2, qg, gg, R, k, ranks=False, negatives=False)
            assert torch.equal(tin[i], ti[i]) and torch.equal(tsn[i], ts[i])
        # and it would matter without the radius: 2 x the best positive's row scores 2 s* >= s* > 0 in every ignored row
        g2 = g.clone()
        g2[torch.from_numpy(np.flatnonzero(ign[i])).cuda()] = 2.0 * g[jpos]
        r0 = masked_call(q, g2, qg, gg, 0)[0]
        assert r0[i].item() == wr[i] + ign[i].sum()


def test_nan_rows():
    nq, ng, d, R, k = 64, 900, 64, 2, 5
    gen = torch.Generator().manual_seed(8)
    q64, g64 = exact_rows(nq, d, gen), exact_rows(ng, d, gen)
    _, gg = timeline(nq, ng, R, gen)
    qg = gg[:nq].clone()
    q64[5] = float("nan")                            # every score NaN -> rank Ng, an empty list
    q64[9, 3] = float("nan")
    g64[(gg == qg[11]).nonzero().flatten()] = float("nan")              # all positives of query 11 NaN -> Ng
    g64[100] = float("nan")                          # a NaN row never counts and is never selected
    S = (q64 @ g64.T).numpy()
    wr, wn, wi, ws = ref_masked(S, qg.numpy(), gg.numpy(), R, k)
    assert wr[5] == ng and wr[9] == ng and wr[11] == ng and (wi[5] == -1).all() and (wr[[0, 1, 2]] < ng).all()
    r, n, ti, ts = masked_call(q64.float().cuda(), g64.float().cuda(), qg, gg, R, k)
    assert np.array_equal(cpu(r), wr) and np.array_equal(cpu(n), wn)
    assert np.array_equal(cpu(ti), wi) and np.array_equal(cpu(ts).astype(np.float64), ws)
    assert not (cpu(ti) == 100).any()


def test_gallery_scale_with_inexact_scores():
    nq, ng, d, R = 2049, 4100, 128, 2
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(nq + ng, d, generator=gen, dtype=torch.float64)
    x = (x / x.norm(dim=1, keepdim=True)).float()
    q, g = x[:nq].cuda(), x[nq:].cuda()
    qg, gg = timeline(nq, ng, R, gen)
    r = ops.retrieval(q, g, q_groups=qg, g_groups=gg, radius=R)[0].cpu()
    r_grouped = ops.retrieval(q, g, q_groups=qg, g_groups=gg)[0].cpu()
    assert (r <= r_grouped).all() and (r < r_grouped).any()
    rows = torch.randperm(nq, generator=gen)[:128]
    S = (q[rows.cuda()].double() @ g.double().T).cpu()
    dist = torch.from_numpy(id_dist(qg[rows], gg))
    same, far = dist == 0, dist > R
    sstar = torch.where(same, S, torch.tensor(-float("inf"), dtype=torch.float64)).max(1).values
    lo = 1 + ((S > sstar[:, None] + 1e-6) & far).sum(1)
    hi = 1 + ((S >= sstar[:, None] - 1e-6) & far).sum(1)
    has = same.any(1)
    assert ((r[rows] >= lo) & (r[rows] <= hi))[has].all() and (r[rows][~has] == ng).all()


def test_retrieval_metrics_with_a_radius():
    n, d, R = 600, 64, 2
    gen = torch.Generator().manual_seed(4)
    ids = timeline(n, n, R, gen)[1]
    ze, zf = exact_rows(n, d, gen), exact_rows(n, d, gen)
    m = retrieval_metrics(ze.float().cuda(), zf.float().cuda(), groups=ids, radius=R)
    m0 = retrieval_metrics(ze.float().cuda(), zf.float().cuda(), groups=ids)
    assert list(m0) == ["eeg_to_fmri", "fmri_to_eeg", "n", "chance"] and m["radius"] == R and m["n"] == n
    dist = id_dist(ids, ids)
    neg = (dist > R).sum(1)
    ignored = ((dist > 0) & (dist <= R)).sum(1)
    assert ignored.min() >= 2 and ignored.max() == 4
    for key, S in (("eeg_to_fmri", (ze @ zf.T).numpy()), ("fmri_to_eeg", (zf @ ze.T).numpy())):
        want = rank_summary(torch.from_numpy(ref_masked(S, ids.numpy(), ids.numpy(), R, 1)[0]))
        got = dict(m[key])
        assert got.pop("ignored_mean") == pytest.approx(ignored.mean(), rel=1e-12)
        assert got.pop("chance_R@1") == pytest.approx((1.0 / (neg + 1.0)).mean(), rel=1e-12)
        assert got == want
        assert m[key]["mean_rank"] <= m0[key]["mean_rank"] and m[key]["chance_R@1"] > m["chance"]
