"""The contrastive losses with ignored temporal neighbours (mm_clip_loss_own_rows_masked, mm_sigmoid_loss_own_rows_masked)
against an fp64 restatement of their contract (include/mmeeg_hip.h).  The int32 ids are positions on a timeline; with the
radius R and d = |gid_j - gid_r| (in exact integers): d == 0 positive, 0 < d <= R ignored, d > R negative; A(r) = the
keys that are not ignored, P(r) = the positives.
  InfoNCE: l_row(r) = LSE_{j in A(r)}(s C[r][j]) - LSE_{j in P(r)}(s C[r][j]), l_col(r) the same over column r,
           loss_r = (l_row + l_col) / 2 - autograd through masked logsumexp
  sigmoid: loss_r = sum_{j in A(r)} softplus(-y (s C[r][j] + b)), y = +1 on P(r), -1 elsewhere
scal = {mean own loss, top-1 e->f, top-1 f->e, d/d logit_scale [, d/d logit_bias]}; dz_local = d (sum over ranks of their
mean losses) / d (own rows); top-1 counts row r when its best positive reaches the maximum over A(r).  Every rank of a
W-rank group is emulated on one GPU through row0.  Shapes, points and tolerances: those of tests/test_sigmoid_loss_gpu.py
and tests/test_clip_groups_gpu.py, whose arithmetic and helpers these kernels share.  Measured on an MI355X over all
launches this file compares with fp64 (one per emulated rank): dz within 8.4e-7 of max(max|g|, 0.1), scalars within 6.6e-7 of
max(|fp64|, 0.1)."""
import ctypes
import functools
import math

import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
from test_sigmoid_loss_gpu import POINTS, SHAPES, _embeddings, _softplus

pytestmark = pytest.mark.gpu

LOSSES = ["infonce", "sigmoid"]
# (ids, radius): a shuffled timeline, every row has 2 to 4 ignored keys | two interleaved runs 100000 apart | positives
# and ignored keys in the same row
PATTERNS = {"timeline": 2, "runs": 1, "pairs": 1}
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def _ids(pattern, Bg, gen):
    if pattern == "timeline":
        return torch.randperm(Bg, generator=gen)
    if pattern == "runs":
        i = torch.arange(Bg)
        return (i % 2) * 100000 + i // 2
    return torch.randperm(Bg, generator=gen) // 2


def relations(gid, radius):
    """-> (positive, admitted) (Bg, Bg) bool from int64 differences: nothing wraps"""
    d = (gid.long()[:, None] - gid.long()[None, :]).abs()
    return d == 0, (d == 0) | (d > radius)


def ref_masked(loss, z_all, gid, radius, ls, lb, B):
    """fp64 autograd, all ranks on one graph -> ([scal per rank], d (sum over ranks of their mean losses) / d z_all)"""
    z = z_all.double().clone().requires_grad_(True)
    lso = torch.tensor(float(ls), dtype=torch.float64, requires_grad=True)
    lbo = torch.tensor(float(lb), dtype=torch.float64, requires_grad=True)
    N, Bg = z.shape[1] // 2, z.shape[0]
    assert Bg % B == 0
    pos, adm = relations(gid, radius)
    C = z[:, :N] @ z[:, N:].T
    ninf = torch.tensor(-math.inf, dtype=torch.float64)
    if loss == "infonce":
        L = lso.exp() * C
        La, Lp = torch.where(adm, L, ninf), torch.where(pos, L, ninf)
        loss_r = 0.5 * ((torch.logsumexp(La, 1) - torch.logsumexp(Lp, 1)) + (torch.logsumexp(La, 0) - torch.logsumexp(Lp, 0)))
    else:
        y = torch.where(pos, 1.0, -1.0).double()
        loss_r = torch.where(adm, _softplus(-y * (lso.exp() * C + lbo)), torch.zeros((), dtype=torch.float64)).sum(1)
    Cd = C.detach()
    Cp, Ca = torch.where(pos, Cd, ninf), torch.where(adm, Cd, ninf)
    hit_e, hit_f = Cp.max(1).values >= Ca.max(1).values, Cp.max(0).values >= Ca.max(0).values
    scals = []
    for row0 in range(0, Bg, B):
        own = slice(row0, row0 + B)
        mean = loss_r[own].mean()
        if loss == "infonce":
            (dls,) = torch.autograd.grad(mean, lso, retain_graph=True)
            extra = [dls]
        else:
            extra = list(torch.autograd.grad(mean, (lso, lbo), retain_graph=True))
        scals.append(torch.stack([mean.detach(), hit_e[own].double().mean(), hit_f[own].double().mean(), *extra]))
    (loss_r.sum() / B).backward()
    return scals, z.grad


@functools.lru_cache(maxsize=None)
def _inputs(W, B, N, point, pattern):
    """-> (z_all fp32 host, ids, ln s and b as the fp32 values the kernels read); shared by both losses, never written"""
    s, b, correlated = POINTS[point]
    gen = torch.Generator().manual_seed(W * 1000 + B + N + len(point) * 17 + len(pattern) * 3)
    z = _embeddings(W * B, N, correlated, gen)
    return z, _ids(pattern, W * B, gen), torch.tensor([math.log(s)]).float().item(), torch.tensor([b]).float().item()


def _run(loss, z_all, gid, ls, lb, B, row0, radius, grad=True, masked=True):
    """one launch pair of the masked entry point (``masked=False``: of the grouped one, which takes no radius)"""
    Bg, N2 = z_all.shape
    n = 4 if loss == "infonce" else 5
    dz = torch.full((B, N2), float("nan"), device="cuda") if grad else None
    scal = torch.full((n,), float("nan"), device="cuda")
    if loss == "infonce":
        if masked:
            ws = torch.empty(ops.clip_loss_masked_ws_floats(B, Bg), device="cuda")
            _hip.call("mm_clip_loss_own_rows_masked", z_all, gid, ls, scal, dz, ws, B, Bg, N2 // 2, row0, radius)
        else:
            ws = torch.empty(ops.clip_loss_grouped_ws_floats(B, Bg), device="cuda")
            _hip.call("mm_clip_loss_own_rows_grouped", z_all, gid, ls, scal, dz, ws, B, Bg, N2 // 2, row0)
    else:
        if masked:
            ws = torch.empty(ops.sigmoid_loss_masked_ws_floats(B, Bg), device="cuda")
            _hip.call("mm_sigmoid_loss_own_rows_masked", z_all, gid, ls, lb, scal, dz, ws, B, Bg, N2 // 2, row0, radius)
        else:
            ws = torch.empty(ops.sigmoid_loss_ws_floats(B, Bg), device="cuda")
            _hip.call("mm_sigmoid_loss_own_rows", z_all, gid, ls, lb, scal, dz, ws, B, Bg, N2 // 2, row0)
    return scal, dz


def _device(z, ids, ls, lb):
    return z.cuda(), ids.to(torch.int32).cuda(), torch.tensor([ls], device="cuda"), torch.tensor([lb], device="cuda")


def _assert_matches(loss, got_scal, got_dz, want, g):
    got = got_scal.cpu().double()
    k = [0] + list(range(3, got.numel()))
    print(f"scal {got.tolist()} want {want.tolist()} dz max err {(got_dz.cpu().double() - g).abs().max().item():.3e} "
          f"of {g.abs().max().item():.3e}")
    torch.testing.assert_close(got_dz.cpu().double(), g, rtol=1e-5, atol=max(1e-5 * g.abs().max().item(), 1e-6))
    torch.testing.assert_close(got[k], want[k], rtol=1e-5, atol=1e-6)
    assert torch.equal(got_scal[1:3].cpu(), want[1:3].float()), (got_scal, want)       # exact: count / B rounded to fp32 once


def test_workspace_sizes_agree_with_the_ops_helpers():
    c = ctypes.c_int(0)
    _hip.call("mm_clip_loss_masked_ws_floats", 32, 256, ctypes.addressof(c))
    assert c.value == ops.clip_loss_masked_ws_floats(32, 256) >= 8 * 256
    _hip.call("mm_sigmoid_loss_masked_ws_floats", 32, 256, ctypes.addressof(c))
    assert c.value == ops.sigmoid_loss_masked_ws_floats(32, 256) >= 5 * 32


@pytest.mark.parametrize("W,B,N", SHAPES)
def test_the_timeline_pattern_ignores_two_to_four_keys_in_every_row(W, B, N):
    _, ids, _, _ = _inputs(W, B, N, "tau", "timeline")
    pos, adm = relations(ids, PATTERNS["timeline"])
    ignored = (~adm).sum(1)
    assert 2 <= ignored.min().item() and ignored.max().item() <= 4 and bool((pos.sum(1) == 1).all())


@pytest.mark.parametrize("W,B,N", SHAPES)
@pytest.mark.parametrize("point", list(POINTS))
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("loss", LOSSES)
def test_masked_loss_matches_fp64(loss, W, B, N, point, pattern):
    z, ids, ls, lb = _inputs(W, B, N, point, pattern)
    R = PATTERNS[pattern]
    pos, adm = relations(ids, R)
    assert bool((~adm).any())                                   # the pattern ignores something
    if pattern == "pairs":
        assert bool(((pos.sum(1) == 2) & ((~adm).sum(1) > 0)).any())     # positives and ignored keys in the same row
    wants, grad = ref_masked(loss, z, ids, R, ls, lb, B)
    z_all, gid, lsd, lbd = _device(z, ids, ls, lb)
    for r, want in enumerate(wants):
        scal, dz = _run(loss, z_all, gid, lsd, lbd, B, r * B, R)
        _assert_matches(loss, scal, dz, want, grad[r * B:(r + 1) * B])
        scal2, dz2 = _run(loss, z_all, gid, lsd, lbd, B, r * B, R)
        assert torch.equal(dz, dz2) and torch.equal(scal, scal2)          # bit-reproducible
        scal3, _ = _run(loss, z_all, gid, lsd, lbd, B, r * B, R, grad=False)
        assert torch.equal(scal, scal3)                                   # dz = NULL: the same scalars


@pytest.mark.parametrize("W,B,N", SHAPES)
def test_a_radius_that_covers_the_timeline_leaves_infonce_nothing(W, B, N):
    """R >= Bg on a timeline: every other key of every row is ignored, A = P = {r}: loss and every dz element exactly 0"""
    z, ids, ls, lb = _inputs(W, B, N, "tau", "timeline")
    z_all, gid, lsd, lbd = _device(z, ids, ls, lb)
    for R in (W * B, INT_MAX):
        for r in range(W):
            scal, dz = _run("infonce", z_all, gid, lsd, lbd, B, r * B, R)
            assert scal.tolist() == [0.0, 1.0, 1.0, 0.0], scal
            assert torch.equal(dz, torch.zeros_like(dz))
    # the sigmoid loss keeps each row's own pair, and nothing else
    wants, grad = ref_masked("sigmoid", z, ids, W * B, ls, lb, B)
    for r, want in enumerate(wants):
        scal, dz = _run("sigmoid", z_all, gid, lsd, lbd, B, r * B, W * B)
        _assert_matches("sigmoid", scal, dz, want, grad[r * B:(r + 1) * B])


@pytest.mark.parametrize("W,B,N", SHAPES)
@pytest.mark.parametrize("loss", LOSSES)
def test_ids_at_the_two_ends_of_int32_are_not_neighbours(loss, W, B, N):
    """ids alternating -2^31 and 2^31 - 1 are 2^32 - 1 apart: with R = 1 nothing is ignored and the result is the grouped
    one.  A difference taken in 32 bits wraps to 1 and ignores every negative.  The two entry points are two
    instantiations of the same formulas with the same sets here; the bound is the one two such instantiations get
    elsewhere in this file and in tests/test_clip_groups_gpu.py (1e-6 absolute, top-1 equal)."""
    z, _, ls, lb = _inputs(W, B, N, "tau", "timeline")
    ids = torch.where(torch.arange(W * B) % 2 == 0, INT_MIN, INT_MAX)
    z_all, gid, lsd, lbd = _device(z, ids, ls, lb)
    assert gid.tolist()[:2] == [INT_MIN, INT_MAX]
    wants, grad = ref_masked(loss, z, ids, 1, ls, lb, B)
    for r, want in enumerate(wants):
        sm, dm = _run(loss, z_all, gid, lsd, lbd, B, r * B, 1)
        sg, dg = _run(loss, z_all, gid, lsd, lbd, B, r * B, 0, masked=False)
        assert (sm - sg).abs().max().item() <= 1e-6 and torch.equal(sm[1:3], sg[1:3]), (sm, sg)
        assert (dm - dg).abs().max().item() <= 1e-6
        _assert_matches(loss, sm, dm, want, grad[r * B:(r + 1) * B])


@pytest.mark.parametrize("W,B,N", SHAPES)
@pytest.mark.parametrize("loss", LOSSES)
def test_radius_zero_is_the_grouped_loss(loss, W, B, N):
    z, ids, ls, lb = _inputs(W, B, N, "tau", "pairs")
    z_all, gid, lsd, lbd = _device(z, ids, ls, lb)
    for r in range(W):
        sm, dm = _run(loss, z_all, gid, lsd, lbd, B, r * B, 0)
        sg, dg = _run(loss, z_all, gid, lsd, lbd, B, r * B, 0, masked=False)
        assert (sm - sg).abs().max().item() <= 1e-6 and torch.equal(sm[1:3], sg[1:3]), (sm, sg)
        assert (dm - dg).abs().max().item() <= 1e-6


@pytest.mark.parametrize("W,B,N", SHAPES)
@pytest.mark.parametrize("loss", LOSSES)
def test_an_ignored_key_does_not_reach_the_gradient(loss, W, B, N):
    """the zf half of a key that row r ignores is replaced by other finite values: dze_r keeps its bits (the coefficient of
    an ignored pair is 0.f, not a small number), while a row that admits the key moves"""
    z, ids, ls, lb = _inputs(W, B, N, "tau", "timeline")
    R, Bg = PATTERNS["timeline"], W * B
    pos, adm = relations(ids, R)
    rank = W - 1
    r = rank * B + B // 2                                       # an own row of the last rank
    own = range(rank * B, (rank + 1) * B)
    # a key it ignores, and an own row that admits that key (Bg = 5: the middle of the timeline is ignored by every row)
    j, other = max(((int(j), [q for q in own if adm[q, j] and q != j]) for j in torch.nonzero(~adm[r]).flatten()),
                   key=lambda t: len(t[1]))
    assert not adm[r, j] and r != j and other
    other = other[0]
    z2 = z.clone()
    z2[j, N:] = 3.0 * torch.randn(N, generator=torch.Generator().manual_seed(5)).float()      # finite, not even normalised
    _, gid, lsd, lbd = _device(z, ids, ls, lb)
    _, d1 = _run(loss, z.cuda(), gid, lsd, lbd, B, rank * B, R)
    _, d2 = _run(loss, z2.cuda(), gid, lsd, lbd, B, rank * B, R)
    assert torch.isfinite(d2).all()
    assert torch.equal(d1[r - rank * B, :N], d2[r - rank * B, :N])
    assert not torch.equal(d1[other - rank * B, :N], d2[other - rank * B, :N])


def test_the_ops_wrappers_reach_the_masked_kernels_and_need_ids():
    z, ids, ls, lb = _inputs(1, 32, 128, "tau", "timeline")
    N = 128
    for loss in LOSSES:
        wants, grad = ref_masked(loss, z, ids, 2, ls, lb, 32)
        zc = z.cuda().requires_grad_(True)
        lsp, lbp = torch.tensor(ls, device="cuda", requires_grad=True), torch.tensor(lb, device="cuda", requires_grad=True)
        if loss == "infonce":
            out = ops.clip_loss(zc[:, :N], zc[:, N:], lsp, None, ids, radius=2)
        else:
            out = ops.sigmoid_loss(zc[:, :N], zc[:, N:], lsp, lbp, None, ids, radius=2)
        out[0].backward()
        torch.testing.assert_close(out[0].detach().cpu().double(), wants[0][0], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(zc.grad.cpu().double(), grad, rtol=1e-5, atol=max(1e-5 * grad.abs().max().item(), 1e-6))
        torch.testing.assert_close(lsp.grad.cpu().double(), wants[0][3], rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError, match="needs group ids"):
        ops.clip_loss(zc[:, :N], zc[:, N:], lsp, None, None, radius=2)
    with pytest.raises(ValueError, match="needs group ids"):
        ops.sigmoid_loss(zc[:, :N], zc[:, N:], lsp, lbp, None, None, radius=2)


def test_bad_arguments_are_refused():
    z = torch.zeros(8, 8, device="cuda")
    gid = torch.zeros(8, dtype=torch.int32, device="cuda")
    ls = torch.zeros(1, device="cuda")
    scal = torch.empty(5, device="cuda")
    ws = torch.empty(64, device="cuda")
    with pytest.raises(Exception, match="clip_loss_own_rows_masked: null"):
        _hip.call("mm_clip_loss_own_rows_masked", z, None, ls, scal, None, ws, 8, 8, 4, 0, 1)
    with pytest.raises(Exception, match="radius=-1"):
        _hip.call("mm_clip_loss_own_rows_masked", z, gid, ls, scal, None, ws, 8, 8, 4, 0, -1)
    with pytest.raises(Exception, match="multiple of 4"):
        _hip.call("mm_clip_loss_own_rows_masked", z, gid, ls, scal, None, ws, 8, 8, 6, 0, 1)
    with pytest.raises(Exception, match="clip_loss_own_rows_masked: B=8 Bg=8 row0=1"):
        _hip.call("mm_clip_loss_own_rows_masked", z, gid, ls, scal, None, ws, 8, 8, 4, 1, 1)
    with pytest.raises(Exception, match="sigmoid_loss_own_rows_masked: null"):
        _hip.call("mm_sigmoid_loss_own_rows_masked", z, None, ls, ls, scal, None, ws, 8, 8, 4, 0, 1)
    with pytest.raises(Exception, match="sigmoid_loss_own_rows_masked: null"):
        _hip.call("mm_sigmoid_loss_own_rows_masked", z, gid, ls, None, scal, None, ws, 8, 8, 4, 0, 1)
    with pytest.raises(Exception, match="radius=-2"):
        _hip.call("mm_sigmoid_loss_own_rows_masked", z, gid, ls, ls, scal, None, ws, 8, 8, 4, 0, -2)
    with pytest.raises(Exception, match="multiple of 4"):
        _hip.call("mm_sigmoid_loss_own_rows_masked", z, gid, ls, ls, scal, None, ws, 8, 8, 6, 0, 1)
    with pytest.raises(Exception, match="sigmoid_loss_own_rows_masked: B=8 Bg=8 row0=1"):
        _hip.call("mm_sigmoid_loss_own_rows_masked", z, gid, ls, ls, scal, None, ws, 8, 8, 4, 1, 1)
