"""Gallery-scale retrieval (mm_retrieval, ops.retrieval, retrieval_metrics, BridgeTrainer.embed / evaluate_retrieval)
against fp64 references that implement the contract of include/mmeeg_hip.h: rank = 1 + #{j != pos : s_j >= s_pos}
(ties count against the query), top-k by score descending then lower index, NaN never counted or selected."""
import numpy as np
import pytest
import torch

from multimodal_eeg_fmri_amd import ops
from multimodal_eeg_fmri_amd.bridge_utils import rank_summary, retrieval_metrics

pytestmark = pytest.mark.gpu

KMAX = ops.retrieval_kmax()


def ref_ranks(S, pos):
    """S (Nq, Ng) float64 scores, pos (Nq,) -> 1 + #{j != pos : S[q, j] >= S[q, pos]}; NaN positive -> Ng"""
    nq, ng = S.shape
    sp = S[np.arange(nq), pos]
    with np.errstate(invalid="ignore"):
        ge = S >= sp[:, None]
    ge[np.arange(nq), pos] = False
    r = 1 + ge.sum(1)
    r[np.isnan(sp)] = ng
    return r


def ref_topk(S, k):
    nq, ng = S.shape
    idx = np.full((nq, k), -1, dtype=np.int64)
    sc = np.full((nq, k), -np.inf)
    key = np.where(np.isnan(S), np.inf, -S)            # NaN last
    order = np.argsort(key, axis=1, kind="stable")[:, :k]   # stable: equal scores by lower index
    for q in range(nq):
        o = order[q][~np.isnan(S[q, order[q]])]
        idx[q, :len(o)] = o
        sc[q, :len(o)] = S[q, o]
    return idx, sc


def exact_rows(n, d, gen):
    """entries j / 64, |j| <= 64: every dot product (D <= 256) is exact in fp32, and ties are frequent"""
    return torch.randint(-64, 65, (n, d), generator=gen).double() / 64.0


def normed(n, d, gen):
    x = torch.randn(n, d, generator=gen, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).float()


@pytest.mark.parametrize("nq,ng,d,k", [(1, 1, 4, 1), (37, 1000, 128, 5), (4097, 4097, 128, 10), (300, 20000, 64, 16),
                                       (64, 5000, 256, KMAX)])
def test_exact_contract_on_representable_inputs(nq, ng, d, k):
    gen = torch.Generator().manual_seed(nq * 7 + ng)
    q64, g64 = exact_rows(nq, d, gen), exact_rows(ng, d, gen)
    # a coarse grid makes ties between the positive and other rows common
    q64[:, d // 2:] = 0
    g64[:, d // 2:] = 0
    S = (q64 @ g64.T).numpy()
    q, g = q64.float().cuda(), g64.float().cuda()
    pos = torch.randint(0, ng, (nq,), generator=gen)
    want_idx, want_sc = ref_topk(S, k)
    for positives in (None, pos) if nq <= ng else (pos,):
        p = np.arange(nq) if positives is None else positives.numpy()
        want_r = ref_ranks(S, p)
        r, ti, ts = ops.retrieval(q, g, positives, k=k)
        assert np.array_equal(r.cpu().numpy(), want_r)
        assert np.array_equal(ti.cpu().numpy(), want_idx)
        assert np.array_equal(ts.cpu().double().numpy(), want_sc)
        r_only, none_i, none_s = ops.retrieval(q, g, positives)
        assert none_i is None and none_s is None
        assert np.array_equal(r_only.cpu().numpy(), want_r)
    none_r, ti2, ts2 = ops.retrieval(q, g, k=k, ranks=False)
    assert none_r is None
    assert np.array_equal(ti2.cpu().numpy(), want_idx) and np.array_equal(ts2.cpu().double().numpy(), want_sc)


def test_exact_duplicates_of_the_positive_count_against_the_query():
    nq, ng, d = 256, 20000, 128
    gen = torch.Generator().manual_seed(5)
    g = normed(ng, d, gen)
    perm = torch.randperm(ng, generator=gen)
    pos = perm[:nq].clone()
    # queries near their positives: the positive's score sits far above the bulk, so few queries have near-ties
    q = torch.nn.functional.normalize(g[pos].double() + 0.1 * torch.randn(nq, d, generator=gen, dtype=torch.float64), dim=1).float()
    free = perm[nq:].tolist()                     # indices no positive uses, spread over the whole gallery
    copies = {}
    for i in range(nq):
        c = (0, 1, 7)[i % 3]
        at = [free.pop() for _ in range(c)]
        for j in at:
            g[j] = g[pos[i]]
        copies[i] = at
    # below and above pos[q], in other tiles / slices
    assert any(min(a) < pos[i] < max(a) for i, a in copies.items() if len(a) == 7)
    S = q.double() @ g.double().T
    r, _, _ = ops.retrieval(q.cuda(), g.cuda(), pos)
    r = r.cpu()
    checked = 0
    for i in range(nq):
        sp = S[i, pos[i]]
        other = torch.ones(ng, dtype=torch.bool)
        other[pos[i]] = False
        other[copies[i]] = False
        so = S[i][other]
        if ((so - sp).abs() < 1e-5).any():
            continue
        assert r[i].item() == 1 + len(copies[i]) + int((so > sp).sum()), i
        checked += 1
    assert checked > nq // 2


def test_random_embeddings_at_gallery_scale():
    n, d, k = 65536, 128, 10
    gen = torch.Generator().manual_seed(11)
    q, g = normed(n, d, gen).cuda(), normed(n, d, gen).cuda()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r1, i1, s1 = ops.retrieval(q, g, k=k)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 256 << 20
    r2, i2, s2 = ops.retrieval(q, g, k=k)
    assert torch.equal(r1, r2) and torch.equal(i1, i2) and torch.equal(s1, s2)        # bit-identical launches
    rows = torch.randperm(n, generator=gen)[:256]
    S = (q[rows.cuda()].double() @ g.double().T).cpu()
    sp = S[torch.arange(256), rows]
    lo = 1 + (S > sp[:, None] + 1e-6).sum(1)
    hi = 1 + (S >= sp[:, None] - 1e-6).sum(1) - 1             # the positive itself is not counted
    rk = r1.cpu()[rows]
    assert ((rk >= lo) & (rk <= hi)).all()
    top64 = S.topk(k, dim=1).values
    assert (s1.cpu()[rows].double() - top64).abs().max() <= 1e-6
    got64 = S.gather(1, i1.cpu()[rows])
    assert (got64 - s1.cpu()[rows].double()).abs().max() <= 1e-6
    assert (i1[:, 1:] != i1[:, :-1]).all()


def test_nan_rows_follow_the_contract():
    nq, ng, d, k = 40, 700, 64, 8
    gen = torch.Generator().manual_seed(3)
    q64, g64 = exact_rows(nq, d, gen), exact_rows(ng, d, gen)
    q64[3] = float("nan")
    q64[17, 5] = float("nan")
    g64[0] = float("nan")
    g64[250, 1] = float("nan")
    g64[19] = float("nan")                       # the positive of query 19 (pos = identity)
    S = (q64 @ g64.T).numpy()
    r, ti, ts = ops.retrieval(q64.float().cuda(), g64.float().cuda(), k=k)
    want_r = ref_ranks(S, np.arange(nq))
    assert want_r[3] == ng and want_r[17] == ng and want_r[19] == ng
    assert np.array_equal(r.cpu().numpy(), want_r)
    want_i, want_s = ref_topk(S, k)
    assert (want_i[3] == -1).all()
    assert np.array_equal(ti.cpu().numpy(), want_i)
    assert np.array_equal(ts.cpu().double().numpy(), want_s)
    # a gallery with fewer finite scores than k: unfilled slots are (-1, -inf)
    g_small = g64[:12].clone()                   # row 0 is NaN already
    g_small[2:] = float("nan")
    _, ti, ts = ops.retrieval(q64.float().cuda(), g_small.float().cuda(), k=4, ranks=False)
    finite_q = torch.ones(nq, dtype=torch.bool)
    finite_q[[3, 17]] = False
    assert (ti[:, 1:] == -1).all() and (ts[:, 1:] == float("-inf")).all()
    assert (ti[finite_q, 0] == 1).all() and (ti[~finite_q, 0] == -1).all()


def test_collapsed_encoder_ranks_last():
    q = torch.ones(8, 16, device="cuda") / 4
    r, _, _ = ops.retrieval(q, q.clone())
    assert (r == 8).all()


def _make_trainer(kind, mode="graph", C=8):
    from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer
    from multimodal_eeg_fmri_amd.crossmodal_v4_enhancements import MultiScaleSTFTPowerEncoder
    ops.set_seed_epoch(None)
    torch.manual_seed(0)
    enc = MultiScaleSTFTPowerEncoder(C, (16, 32), 8, 128, 2, 4, 0.1) if kind == "stft" else None
    return BridgeTrainer(eeg_channels=C, dropout=0.1, lr=1e-3, mode=mode, eeg_encoder=enc).train()


@pytest.mark.parametrize("kind", ["erp", "stft"])
def test_single_modality_embedding_is_the_paired_one(kind):
    from multimodal_eeg_fmri_amd.bridge_trainer import synthetic_pairs
    tr = _make_trainer(kind, mode="manual")
    eeg, fmri = synthetic_pairs(24, 8, 256, (16, 16, 16), seed=77)
    tr.train_step(eeg, fmri)
    ze, zf = tr.embed(eeg=eeg, batch_size=24)[0], tr.embed(fmri=fmri, batch_size=24)[1]
    assert tr.training
    tr.eval()
    with torch.no_grad():
        ze_p, zf_p = ops.contrastive_embed(tr.head.bridge, tr.eeg_encoder(eeg), tr.fmri_encoder(fmri), False)
    tr.train()
    assert torch.equal(ze, ze_p) and torch.equal(zf, zf_p)
    ze_c, zf_c = tr.embed(eeg.cpu(), fmri.cpu(), batch_size=7)          # host input, chunks of 7
    assert torch.nn.functional.cosine_similarity(ze_c, ze).min() >= 1 - 1e-6
    assert torch.nn.functional.cosine_similarity(zf_c, zf).min() >= 1 - 1e-6
    assert torch.allclose(ze.norm(dim=1), torch.ones(24, device="cuda"), atol=1e-5)


def test_evaluate_retrieval_matches_fp64_metrics():
    from multimodal_eeg_fmri_amd.bridge_trainer import synthetic_pairs
    tr = _make_trainer("erp")
    for i in range(3):
        tr.train_step(*synthetic_pairs(16, 8, 256, (16, 16, 16), seed=10 + i))
    eeg, fmri = synthetic_pairs(2048, 8, 256, (16, 16, 16), seed=999)
    out = tr.evaluate_retrieval(eeg, fmri, k=5)
    assert out["n"] == 2048 and out["chance"] == 1 / 2048
    ze, zf = tr.embed(eeg, fmri)
    S = (ze.double() @ zf.double().T).cpu()
    for key, M in (("eeg_to_fmri", S), ("fmri_to_eeg", S.T)):
        sp = M.diagonal()
        lo = 1 + (M > sp[:, None] + 1e-6).sum(1)
        hi = (M >= sp[:, None] - 1e-6).sum(1)
        m_lo, m_hi = rank_summary(lo), rank_summary(hi)
        got = out[key]
        for name in ("R@1", "R@5", "R@10", "median_rank", "mean_rank", "mrr"):
            a, b = sorted((m_lo[name], m_hi[name]))
            assert a - 1e-12 <= got[name] <= b + 1e-12, (key, name, got[name], a, b)
        idx, sc = out["topk"][key]
        assert idx.shape == (2048, 5)
        assert (sc.cpu().double() - M.topk(5, dim=1).values).abs().max() <= 1e-6
    assert out["eeg_to_fmri"]["R@10"] >= out["eeg_to_fmri"]["R@1"]
    assert retrieval_metrics(ze, zf) == {k: v for k, v in out.items() if k != "topk"}


def test_evaluation_does_not_disturb_training():
    from multimodal_eeg_fmri_amd.bridge_trainer import synthetic_pairs
    batches = [synthetic_pairs(16, 8, 256, (16, 16, 16), seed=500 + i) for i in range(3)]
    held = synthetic_pairs(300, 8, 256, (16, 16, 16), seed=600)

    def run(interrupt):
        ops.set_dropout_seed(4321)
        tr = _make_trainer("erp")
        losses = []
        for i in range(6):
            if interrupt and i == 3:
                tr.evaluate_retrieval(*held, batch_size=128)
            losses.append(tr.train_step(*batches[i % 3])["loss"].clone())
        torch.cuda.synchronize()
        params = [p.detach().clone() for p in tr.parameters()]
        bufs = [b.detach().clone() for b in tr.buffers()]
        ops.set_seed_epoch(None)
        return torch.stack(losses), params, bufs

    l1, p1, b1 = run(False)
    l2, p2, b2 = run(True)
    assert torch.isfinite(l1).all()
    assert torch.equal(l1, l2)
    assert all(torch.equal(a, b) for a, b in zip(p1, p2))
    assert all(torch.equal(a, b) for a, b in zip(b1, b2))
