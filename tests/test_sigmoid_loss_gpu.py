"""Pairwise sigmoid loss (mm_sigmoid_loss_own_rows) against an fp64 restatement of its contract (include/mmeeg_hip.h):
u[r][j] = s C[r][j] + b, y = +1 for a positive pair (gid null: r == j, else gid_r == gid_j) and -1 otherwise,
l = softplus(-y u), loss_r = sum_j l[r][j]; scal5 = {mean own loss, top-1 e->f, top-1 f->e, d/d logit_scale, d/d logit_bias};
dz_local = d (sum over ranks of their mean losses) / d (own rows).  Every rank of a W-rank group is emulated on one GPU
through row0.  Tolerances: those of the InfoNCE kernel tests (tests/test_clip_groups_gpu.py), whose arithmetic and helpers
these kernels share."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from multimodal_eeg_fmri_amd import _hip, ops

pytestmark = pytest.mark.gpu

# (W, B, N): the trainer's shape | columns owned by other ranks | N % 32 tail, Bg < 8, B below a wave | Bg > 256 and B > 64
SHAPES = [(1, 32, 128), (4, 16, 128), (1, 5, 36), (2, 160, 64)]
# (s, b, correlated pairs): initialisation | positives and negatives both contribute | a trained regime
POINTS = {"init": (10.0, -10.0, False), "tau": (1 / 0.07, 0.0, False), "trained": (30.0, -12.0, True)}
PATTERNS = [None, "distinct", "pairs", "one", "random"]


def _softplus(x):
    return x.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))


def ref_sigmoid(z_all, gid, ls, lb, B, row0):
    """fp64: (loss, top1_e2f, top1_f2e, d loss / d logit_scale, d loss / d logit_bias) of the rank owning rows
    [row0, row0 + B), and d (sum over all ranks' losses) / d z_all"""
    z = z_all.double().clone().requires_grad_(True)
    lso = torch.tensor(float(ls), dtype=torch.float64, requires_grad=True)
    lbo = torch.tensor(float(lb), dtype=torch.float64, requires_grad=True)
    N = z.shape[1] // 2
    Bg = z.shape[0]
    C = z[:, :N] @ z[:, N:].T
    u = lso.exp() * C + lbo
    same = torch.eye(Bg, dtype=torch.bool) if gid is None else gid[:, None] == gid[None, :]
    y = torch.where(same, 1.0, -1.0).double()
    loss_r = _softplus(-y * u).sum(1)
    own = slice(row0, row0 + B)
    loss = loss_r[own].mean()
    dls, dlb = torch.autograd.grad(loss, (lso, lbo), retain_graph=True)
    (loss_r.sum() / B).backward()                       # every rank's mean over its B rows, summed over ranks
    Cd = C.detach()
    Cp = torch.where(same, Cd, torch.tensor(-math.inf, dtype=torch.float64))
    t_e = (Cp.max(1).values >= Cd.max(1).values)[own].double().mean()
    t_f = (Cp.max(0).values >= Cd.max(0).values)[own].double().mean()
    assert Bg % B == 0
    return torch.stack([loss.detach(), t_e, t_f, dls, dlb]), z.grad


def _ids(pattern, Bg, gen):
    """the id patterns of tests/test_clip_groups_gpu.py"""
    if pattern == "distinct":
        return torch.randperm(Bg, generator=gen) * 7 - 100                  # arbitrary values, compared for equality only
    if pattern == "pairs":
        return torch.randperm(Bg, generator=gen) // 2
    if pattern == "one":
        return torch.full((Bg,), 5)
    sizes, n = [], 0                                                         # random group sizes (1 .. 9) spanning the ranks
    while n < Bg:
        k = min(int(torch.randint(1, 10, (1,), generator=gen)), Bg - n)
        sizes.append(k)
        n += k
    ids = torch.repeat_interleave(torch.arange(len(sizes)) * 3 + 1000, torch.tensor(sizes))
    return ids[torch.randperm(Bg, generator=gen)]


def _embeddings(Bg, N, correlated, gen):
    ze = F.normalize(torch.randn(Bg, N, generator=gen, dtype=torch.float64), dim=1)
    noise = F.normalize(torch.randn(Bg, N, generator=gen, dtype=torch.float64), dim=1)
    zf = F.normalize(0.9 * ze + math.sqrt(1 - 0.81) * noise, dim=1) if correlated else noise
    return torch.cat([ze, zf], dim=1).float()


@functools.lru_cache(maxsize=None)
def _case(W, B, N, point, pattern):
    """-> (z_all fp32 host, ids or None, ln s and b as the fp32 values the kernel reads, [(want5, grad) per rank])"""
    s, b, correlated = POINTS[point]
    gen = torch.Generator().manual_seed(W * 1000 + B + N + len(point) * 17 + len(pattern or ""))
    Bg = W * B
    z = _embeddings(Bg, N, correlated, gen)
    ids = None if pattern is None else _ids(pattern, Bg, gen)
    ls = torch.tensor([math.log(s)]).float().item()
    lb = torch.tensor([b]).float().item()
    return z, ids, ls, lb, [ref_sigmoid(z, ids, ls, lb, B, r * B) for r in range(W)]


def _run(z_all, gid, ls, lb, B, row0, grad=True):
    Bg, N2 = z_all.shape
    dz = torch.full((B, N2), float("nan"), device="cuda") if grad else None
    scal = torch.full((5,), float("nan"), device="cuda")
    ws = torch.empty(ops.sigmoid_loss_ws_floats(B, Bg), device="cuda")
    _hip.call("mm_sigmoid_loss_own_rows", z_all, gid, ls, lb, scal, dz, ws, B, Bg, N2 // 2, row0)
    return scal, dz


def _device(z, ids, ls, lb):
    return (z.cuda(), None if ids is None else ids.to(torch.int32).cuda(), torch.tensor([ls], device="cuda"),
            torch.tensor([lb], device="cuda"))


def test_workspace_size():
    c = ctypes.c_int(0)
    _hip.call("mm_sigmoid_loss_ws_floats", 32, 256, ctypes.addressof(c))
    assert c.value == ops.sigmoid_loss_ws_floats(32, 256) >= 5 * 32


@pytest.mark.parametrize("W,B,N", SHAPES)
@pytest.mark.parametrize("point", list(POINTS))
@pytest.mark.parametrize("pattern", PATTERNS)
def test_sigmoid_loss_matches_fp64(W, B, N, point, pattern):
    z, ids, ls, lb, refs = _case(W, B, N, point, pattern)
    z_all, gid, lsd, lbd = _device(z, ids, ls, lb)
    for r, (want, grad) in enumerate(refs):
        scal, dz = _run(z_all, gid, lsd, lbd, B, r * B)
        g = grad[r * B:(r + 1) * B]
        got = scal.cpu().double()
        print(f"rank {r}: scal {got.tolist()} want {want.tolist()} "
              f"dz max err {(dz.cpu().double() - g).abs().max().item():.3e} of {g.abs().max().item():.3e}")
        torch.testing.assert_close(dz.cpu().double(), g, rtol=1e-5, atol=max(1e-5 * g.abs().max().item(), 1e-6))
        torch.testing.assert_close(got[[0, 3, 4]], want[[0, 3, 4]], rtol=1e-5, atol=1e-6)
        assert torch.equal(scal[1:3].cpu(), want[1:3].float()), (scal, want)      # exact: count / B rounded to fp32 once
        scal2, dz2 = _run(z_all, gid, lsd, lbd, B, r * B)
        assert torch.equal(dz, dz2) and torch.equal(scal, scal2)          # bit-reproducible
        scal3, _ = _run(z_all, gid, lsd, lbd, B, r * B, grad=False)       # eval: the same scalars
        assert torch.equal(scal, scal3)
        if pattern == "one":                                                 # every column is a positive: top-1 1
            assert scal[1].item() == 1.0 and scal[2].item() == 1.0


@pytest.mark.parametrize("W,B,N", SHAPES)
def test_distinct_ids_give_the_plain_loss(W, B, N):
    z, ids, ls, lb, _ = _case(W, B, N, "tau", "distinct")
    z_all, gid, lsd, lbd = _device(z, ids, ls, lb)
    for r in range(W):
        sg, dg = _run(z_all, gid, lsd, lbd, B, r * B)
        su, du = _run(z_all, None, lsd, lbd, B, r * B)
        assert (sg[[0, 3, 4]] - su[[0, 3, 4]]).abs().max().item() <= 1e-6
        assert torch.equal(sg[1:3], su[1:3])
        assert (dg - du).abs().max().item() <= 1e-6


def test_separated_pairs_keep_the_small_loss():
    """zf = ze at (s, b) = (30, -15): every pair is far on its side, each term is ~1e-7 .. 1e-5 and the loss ~2e-4.
    softplus through log1p keeps it to fp32 rounding; log(1 + exp(x)) quantises every term to 2^-24 and is ~1e-4 off."""
    B, N = 32, 128
    gen = torch.Generator().manual_seed(11)
    ze = F.normalize(torch.randn(B, N, generator=gen, dtype=torch.float64), dim=1).float()
    z = torch.cat([ze, ze], dim=1)
    ls, lb = torch.tensor([math.log(30.0)]).float().item(), -15.0
    want, _ = ref_sigmoid(z, None, ls, lb, B, 0)
    scal, _ = _run(*_device(z, None, ls, lb), B, 0)
    print(f"separated pairs: loss {scal[0].item():.9e} fp64 {want[0].item():.9e}")
    assert 1e-5 < want[0].item() < 1e-3
    torch.testing.assert_close(scal[0].cpu().double(), want[0], rtol=1e-5, atol=0)


def test_bad_arguments_are_refused():
    z = torch.zeros(8, 8, device="cuda")
    gid = torch.zeros(8, dtype=torch.int32, device="cuda")
    ls = torch.zeros(1, device="cuda")
    scal = torch.empty(5, device="cuda")
    ws = torch.empty(64, device="cuda")
    with pytest.raises(Exception, match="sigmoid_loss_own_rows: null"):
        _hip.call("mm_sigmoid_loss_own_rows", z, gid, ls, None, scal, None, ws, 8, 8, 4, 0)
    with pytest.raises(Exception, match="multiple of 4"):
        _hip.call("mm_sigmoid_loss_own_rows", z, gid, ls, ls, scal, None, ws, 8, 8, 6, 0)
    with pytest.raises(Exception, match="sigmoid_loss_own_rows: B=8 Bg=8 row0=1"):
        _hip.call("mm_sigmoid_loss_own_rows", z, gid, ls, ls, scal, None, ws, 8, 8, 4, 1)
