"""Grouped retrieval ranks (mm_retrieval_grouped, ops.retrieval(q_groups=, g_groups=), retrieval_metrics(groups=))
against an exact host oracle of the contract in include/mmeeg_hip.h: s* = max over {j : ggid[j] = qgid[q]} of s(q, j)
(NaN scores ignored); rank = 1 + #{j : ggid[j] != qgid[q], s(q, j) >= s*}; no positive (or only NaN ones) -> Ng.
Inputs are multiples of 1/64 with D <= 256, so every fp32 dot product is exact and the fp64 oracle sees the same ties."""
import ctypes

import numpy as np
import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
from multimodal_eeg_fmri_amd.bridge_utils import rank_summary, retrieval_metrics

pytestmark = pytest.mark.gpu


def ref_grouped_ranks(S, qg, gg):
    nq, ng = S.shape
    pos = (qg[:, None] == gg[None, :]) & ~np.isnan(S)
    sstar = np.where(pos, S, -np.inf).max(1) if ng else np.full(nq, np.nan)
    sstar[~pos.any(1)] = np.nan
    with np.errstate(invalid="ignore"):
        ge = (S >= sstar[:, None]) & (qg[:, None] != gg[None, :])
    r = 1 + ge.sum(1)
    r[np.isnan(sstar)] = ng
    return r


def exact_rows(n, d, gen):
    x = torch.randint(-64, 65, (n, d), generator=gen).double() / 64.0
    x[:, d // 2:] = 0                                   # a coarse grid: ties are common
    return x


def random_groups(n, gen, max_size=9):
    sizes, k = [], 0
    while k < n:
        s = min(int(torch.randint(1, max_size + 1, (1,), generator=gen)), n - k)
        sizes.append(s)
        k += s
    ids = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    return ids[torch.randperm(n, generator=gen)]


def grouped_call(q, g, qg, gg):
    nq, d = q.shape
    ng = g.shape[0]
    c = ctypes.c_int(0)
    _hip.call("mm_retrieval_grouped_ws_floats", nq, ng, d, ctypes.addressof(c))
    ws = torch.empty(c.value, device="cuda")
    r = torch.full((nq,), -1, dtype=torch.int32, device="cuda")
    _hip.call("mm_retrieval_grouped", q, g, qg.to(torch.int32).cuda(), gg.to(torch.int32).cuda(), r, ws, nq, ng, d)
    return r


@pytest.mark.parametrize("nq,ng,d", [(1, 1, 4), (200, 200, 128), (37, 1000, 64), (1500, 300, 128), (3000, 5000, 128)])
def test_exact_contract_on_representable_inputs(nq, ng, d):
    gen = torch.Generator().manual_seed(nq + 13 * ng)
    q64, g64 = exact_rows(nq, d, gen), exact_rows(ng, d, gen)
    gg = random_groups(ng, gen)
    n_groups = int(gg.max()) + 1
    qg = torch.randint(0, n_groups + 3, (nq,), generator=gen)          # some queries have no positive in the gallery
    S = (q64 @ g64.T).numpy()
    want = ref_grouped_ranks(S, qg.numpy(), gg.numpy())
    r = grouped_call(q64.float().cuda(), g64.float().cuda(), qg, gg)
    assert np.array_equal(r.cpu().numpy(), want)
    r2, i2, s2 = ops.retrieval(q64.float().cuda(), g64.float().cuda(), q_groups=qg, g_groups=gg)
    assert i2 is None and s2 is None and np.array_equal(r2.cpu().numpy(), want)
    assert torch.equal(grouped_call(q64.float().cuda(), g64.float().cuda(), qg, gg), r)       # deterministic
    no_pos = ~np.isin(qg.numpy(), gg.numpy())
    assert (want[no_pos] == ng).all() and (nq < 30 or no_pos.any())


def test_duplicated_gallery_rows_and_nan_rows():
    nq, ng, d = 64, 900, 64
    gen = torch.Generator().manual_seed(8)
    q64, g64 = exact_rows(nq, d, gen), exact_rows(ng, d, gen)
    gg = random_groups(ng, gen, 5)
    qg = gg[:nq].clone()
    # exact duplicates of positives placed as other groups' rows, below and above, in other tiles
    for i in range(0, nq, 3):
        pos = (gg == qg[i]).nonzero().flatten()
        others = (gg != qg[i]).nonzero().flatten()
        for j in others[torch.randperm(len(others), generator=gen)[:2]]:
            g64[j] = g64[pos[0]]
    q64[5] = float("nan")                            # every score NaN -> rank Ng
    q64[9, 3] = float("nan")
    g64[(gg == qg[11]).nonzero().flatten()] = float("nan")              # all positives of query 11 NaN -> Ng
    g64[100] = float("nan")                          # a NaN row never counts
    S = (q64 @ g64.T).numpy()
    want = ref_grouped_ranks(S, qg.numpy(), gg.numpy())
    assert want[5] == ng and want[9] == ng and want[11] == ng
    r = grouped_call(q64.float().cuda(), g64.float().cuda(), qg, gg)
    assert np.array_equal(r.cpu().numpy(), want)


@pytest.mark.parametrize("n,d", [(300, 128), (4097, 128)])
def test_distinct_ids_give_the_ungrouped_ranks(n, d):
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(2 * n, d, generator=gen, dtype=torch.float64)
    x = (x / x.norm(dim=1, keepdim=True)).float()
    q, g = x[:n].cuda(), x[n:].cuda()
    g[7] = g[3]                                      # an exact duplicate of a positive (a tie against the query)
    ids = torch.arange(n)
    want, _, _ = ops.retrieval(q, g)
    got, _, _ = ops.retrieval(q, g, q_groups=ids, g_groups=ids)
    assert torch.equal(got, want)
    q64, g64 = exact_rows(n, d, gen), exact_rows(n, d, gen)
    want, _, _ = ops.retrieval(q64.float().cuda(), g64.float().cuda())
    got = grouped_call(q64.float().cuda(), g64.float().cuda(), ids, ids)
    assert torch.equal(got.long(), want)


def test_gallery_scale_with_random_group_sizes():
    n, d = 8192, 128
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(2 * n, d, generator=gen, dtype=torch.float64)
    x = (x / x.norm(dim=1, keepdim=True)).float()
    q, g = x[:n].cuda(), x[n:].cuda()
    ids = random_groups(n, gen, 12)
    r = ops.retrieval(q, g, q_groups=ids, g_groups=ids)[0].cpu()
    rows = torch.randperm(n, generator=gen)[:128]
    S = (q[rows.cuda()].double() @ g.double().T).cpu()
    same = ids[rows][:, None] == ids[None, :]
    sstar = torch.where(same, S, torch.tensor(-float("inf"), dtype=torch.float64)).max(1).values
    lo = 1 + ((S > sstar[:, None] + 1e-6) & ~same).sum(1)
    hi = 1 + ((S >= sstar[:, None] - 1e-6) & ~same).sum(1)
    assert ((r[rows] >= lo) & (r[rows] <= hi)).all()


def test_retrieval_metrics_with_groups():
    n, d = 600, 64
    gen = torch.Generator().manual_seed(4)
    ids = random_groups(n, gen, 6)
    base = torch.randn(int(ids.max()) + 1, d, generator=gen, dtype=torch.float64)
    zf = base[ids]                                   # one vector per subject, repeated (one volume per subject)
    ze = base[ids] + 0.3 * torch.randn(n, d, generator=gen, dtype=torch.float64)
    ze, zf = [(t / t.norm(dim=1, keepdim=True)).float().cuda() for t in (ze, zf)]
    m = retrieval_metrics(ze, zf, groups=ids)
    S = (ze.double() @ zf.double().T).cpu().numpy()
    same = ids.numpy()[:, None] == ids.numpy()[None, :]
    for key, M in (("eeg_to_fmri", S), ("fmri_to_eeg", S.T)):
        r = ops.retrieval(*((ze, zf) if key == "eeg_to_fmri" else (zf, ze)), q_groups=ids, g_groups=ids)[0].cpu().numpy()
        assert m[key] == rank_summary(torch.from_numpy(r))
        sstar = np.where(same, M, -np.inf).max(1)[:, None]
        lo = 1 + ((M > sstar + 1e-6) & ~same).sum(1)
        hi = 1 + ((M >= sstar - 1e-6) & ~same).sum(1)
        assert ((r >= lo) & (r <= hi)).all()
    # the ungrouped metrics count a subject's other volumes as misses: the grouped R@1 is at least as high
    mu = retrieval_metrics(ze, zf)
    assert m["eeg_to_fmri"]["R@1"] >= mu["eeg_to_fmri"]["R@1"] and m["eeg_to_fmri"]["R@1"] > 0.5
    assert mu["fmri_to_eeg"]["R@1"] < m["fmri_to_eeg"]["R@1"]
