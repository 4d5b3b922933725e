"""The fp64 references of the InfoNCE and AdamW kernel tests (tests/test_clip_loss_shapes_gpu.py,
tests/test_adamw_kernels_gpu.py import them from here), and their own checks, which need no GPU.

ref_infonce      the contract of mm_clip_loss_own_rows / _grouped (include/mmeeg_hip.h) through fp64 autograd
closed_infonce   the same quantities of the own rows from the formulas in csrc/clip_loss.hip's header comment, in row chunks:
                 never more than ~chunk x Bg doubles alive (the Bg = 8172 case, where Bg^2 doubles are 534 MB)
ref_adamw        one step of csrc/optim.hip's header comment in fp64

Checked here: closed form == autograd to 1e-12 relative (plain and grouped, row0 not a multiple of B, Bg not a multiple of
B, several chunk sizes); ref_adamw == torch.optim.AdamW (+ clip_grad_norm_) on fp64 tensors; all-distinct ids == plain."""
import math

import pytest
import torch
import torch.nn.functional as F

NINF = -math.inf


def _same(gid, Bg):
    return torch.eye(Bg, dtype=torch.bool) if gid is None else gid[:, None] == gid[None, :]


def ref_infonce_ranks(z_all, gid, logit_scale, B, row0s):
    """ref_infonce for several row0 on one autograd graph -> ([scal4 per row0], d (sum over ranks) / d z_all)"""
    z = z_all.double().clone().requires_grad_(True)
    lso = torch.tensor(float(logit_scale), dtype=torch.float64, requires_grad=True)
    Bg, N = z.shape[0], z.shape[1] // 2
    C = z[:, :N] @ z[:, N:].T
    L = lso.exp() * C
    same = _same(gid, Bg)
    ninf = torch.tensor(NINF, dtype=torch.float64)
    l_row = torch.logsumexp(L, 1) - torch.logsumexp(torch.where(same, L, ninf), 1)
    l_col = torch.logsumexp(L, 0) - torch.logsumexp(torch.where(same, L, ninf), 0)
    loss_r = 0.5 * (l_row + l_col)
    Cd = C.detach()
    Cp = torch.where(same, Cd, ninf)
    top_e = Cp.max(1).values >= Cd.max(1).values
    top_f = Cp.max(0).values >= Cd.max(0).values
    scals = []
    for row0 in row0s:
        assert 0 <= row0 and row0 + B <= Bg
        own = slice(row0, row0 + B)
        loss = loss_r[own].mean()
        (dls,) = torch.autograd.grad(loss, lso, retain_graph=True)
        scals.append(torch.stack([loss.detach(), top_e[own].double().mean(), top_f[own].double().mean(), dls]))
    (loss_r.sum() / B).backward()                       # every rank's mean over its B rows, summed over ranks
    return scals, z.grad


def ref_infonce(z_all, gid, logit_scale, B, row0):
    """fp64 autograd: scal4 = (mean own loss, top-1 e->f, top-1 f->e, d loss / d logit_scale) of the rank owning rows
    [row0, row0 + B), and d (sum over all ranks of their mean losses) / d z_all = d (sum_r loss_r / B) / d z_all, whatever
    row0 is and whether or not B divides Bg.  gid None: pair r is the only positive of r."""
    scals, grad = ref_infonce_ranks(z_all, gid, logit_scale, B, [row0])
    return scals[0], grad


def _chunks(n, chunk):
    return [slice(a, min(a + chunk, n)) for a in range(0, n, chunk)]


def closed_infonce(z_all, gid, logit_scale, B, row0, chunk=1024):
    """the same scal4, and dz of the own rows only (B, 2N), in fp64 from the closed forms (csrc/clip_loss.hip):
        dL/dC[r][j] = 0.5/B s (P_row + P_col - 2 delta)[r][j]                     plain
                    = 0.5/B s (P_row + P_col - [gid_r = gid_j] (Q_row + Q_col))   grouped
        dze_r = sum_j dL/dC[r][j] zf_j        dzf_r = sum_j dL/dC[j][r] ze_j
        d loss_r / d logit_scale = s/2 ((E_row[C] - E_Qrow[C]) + (E_col[C] - E_Qcol[C]))
    in chunks of `chunk` rows: at most a few chunk x Bg matrices at a time."""
    z = z_all.double()
    Bg, N = z.shape[0], z.shape[1] // 2
    assert 0 <= row0 and row0 + B <= Bg
    ze, zf = z[:, :N], z[:, N:]
    s = math.exp(float(logit_scale))
    ar = torch.arange(Bg)

    def same_rows(sl):
        return (ar[sl, None] == ar[None, :]) if gid is None else (gid[sl, None] == gid[None, :])

    # pass 1: every row's and column's log-sum-exp over all columns and over its positive set
    lse_r, lse_c, lsp_r, lsp_c = (torch.empty(Bg, dtype=torch.float64) for _ in range(4))
    for sl in _chunks(Bg, chunk):
        same = same_rows(sl)
        for q, k, lse, lsp in ((ze, zf, lse_r, lsp_r), (zf, ze, lse_c, lsp_c)):     # rows of C, then columns of C
            L = s * (q[sl] @ k.T)
            lse[sl] = torch.logsumexp(L, 1)
            lsp[sl] = torch.logsumexp(L.masked_fill(~same, NINF), 1)
    # pass 2: the own rows
    dz = torch.empty(B, 2 * N, dtype=torch.float64)
    loss, dls, top_e, top_f = 0.0, 0.0, 0.0, 0.0
    for sl in _chunks(B, chunk):
        own = slice(row0 + sl.start, row0 + sl.stop)
        same = same_rows(own)
        tops = []
        # row r of C against (its own, every column's) normalisers; then column r of C against (every row's, its own)
        for half, q, k, mine, mine_p, other, other_p in ((0, ze, zf, lse_r, lsp_r, lse_c, lsp_c),
                                                         (1, zf, ze, lse_c, lsp_c, lse_r, lsp_r)):
            Cq = q[own] @ k.T
            L = s * Cq
            P_mine, Q_mine = torch.exp(L - mine[own, None]), torch.exp(L - mine_p[own, None]) * same
            G = P_mine + torch.exp(L - other[None, :]) - Q_mine - torch.exp(L - other_p[None, :]) * same
            dz[sl, half * N:(half + 1) * N] = (0.5 / B * s) * (G @ k)
            loss += 0.5 * (mine[own] - mine_p[own]).sum().item()
            dls += 0.5 * s * ((P_mine - Q_mine) * Cq).sum().item()
            tops.append((Cq.masked_fill(~same, NINF).max(1).values >= Cq.max(1).values).double().sum().item())
        top_e += tops[0]
        top_f += tops[1]
    return torch.tensor([loss / B, top_e / B, top_f / B, dls / B], dtype=torch.float64), dz


def ref_adamw(p, g, m, v, step, lr, beta1, beta2, eps, wd, max_norm, grad_scale):
    """one fused step in fp64 (csrc/optim.hip), `step` = the count BEFORE it -> (p, m, v, sumsq, clip, norm):
    norm = sqrt(sum g^2) grad_scale; clip = min(1, max_norm / (norm + 1e-6)) if max_norm > 0 else 1; g' = g grad_scale clip;
    p <- p (1 - lr wd); m <- b1 m + (1 - b1) g'; v <- b2 v + (1 - b2) g'^2; t = step + 1;
    p <- p - lr / (1 - b1^t) m / (sqrt(v) / sqrt(1 - b2^t) + eps)"""
    p, g, m, v = (x.double() for x in (p, g, m, v))
    sumsq = (g * g).sum().item()
    norm = math.sqrt(sumsq) * grad_scale
    clip = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    gs = g * (grad_scale * clip)
    t = step + 1
    p = p * (1.0 - lr * wd)
    m = beta1 * m + (1.0 - beta1) * gs
    v = beta2 * v + (1.0 - beta2) * gs * gs
    p = p - lr / (1.0 - beta1 ** t) * m / (v.sqrt() / math.sqrt(1.0 - beta2 ** t) + eps)
    return p, m, v, sumsq, clip, norm


# ---------------------------------------------------------------------------------------------------------------------------
def unit_pairs(Bg, N, gen, c=None):
    """[ze | zf] L2-normalised in fp64 and rounded to fp32; c None: independent pairs, else zf = normalize(ze + c noise)"""
    ze = F.normalize(torch.randn(Bg, N, generator=gen, dtype=torch.float64), dim=1)
    noise = F.normalize(torch.randn(Bg, N, generator=gen, dtype=torch.float64), dim=1)
    zf = noise if c is None else F.normalize(ze + c * noise, dim=1)
    return torch.cat([ze, zf], dim=1).float()


def _random_groups(Bg, gen):
    sizes, n = [], 0
    while n < Bg:
        k = min(int(torch.randint(1, 10, (1,), generator=gen)), Bg - n)
        sizes.append(k)
        n += k
    ids = torch.repeat_interleave(torch.arange(len(sizes)) * 3 + 1000, torch.tensor(sizes))
    return ids[torch.randperm(Bg, generator=gen)]


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("Bg,N,B,row0", [(21, 20, 5, 3), (64, 36, 16, 48)])
@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("s", [1.0, 1 / 0.07, 100.0])
def test_closed_form_is_the_autograd_reference(Bg, N, B, row0, grouped, s):
    gen = torch.Generator().manual_seed(Bg + N + int(grouped))
    z = unit_pairs(Bg, N, gen, c=2.5 if s == 100.0 else None)
    gid = _random_groups(Bg, gen) if grouped else None
    want, grad = ref_infonce(z, gid, math.log(s), B, row0)
    for chunk in (1024, 7, 1):                                              # one chunk; ragged chunks of Bg and of B; rows alone
        got, dz = closed_infonce(z, gid, math.log(s), B, row0, chunk=chunk)
        assert _rel(dz, grad[row0:row0 + B]) <= 1e-12
        assert torch.equal(got[1:3], want[1:3])
        assert ((got[[0, 3]] - want[[0, 3]]).abs() <= 1e-12 * want[[0, 3]].abs()).all(), (got, want)


def test_several_ranks_on_one_graph_are_the_single_calls():
    gen = torch.Generator().manual_seed(5)
    z, gid = unit_pairs(21, 20, gen), _random_groups(21, gen)
    scals, grad = ref_infonce_ranks(z, gid, 1.3, 5, [0, 3, 16])
    for row0, sc in zip([0, 3, 16], scals):
        want, g1 = ref_infonce(z, gid, 1.3, 5, row0)
        assert torch.equal(sc, want) and torch.equal(grad, g1)


@pytest.mark.parametrize("Bg,N,B,row0", [(21, 20, 5, 3), (64, 36, 16, 48)])
def test_distinct_ids_give_the_plain_result(Bg, N, B, row0):
    gen = torch.Generator().manual_seed(Bg)
    z = unit_pairs(Bg, N, gen)
    ids = torch.randperm(Bg, generator=gen) * 7 - 100
    for f in (ref_infonce, closed_infonce):
        sp, gp = f(z, None, 2.0, B, row0)
        sg, gg = f(z, ids, 2.0, B, row0)
        assert _rel(sg, sp) <= 1e-14 and _rel(gg, gp) <= 1e-14


def test_one_group_has_no_loss_and_no_gradient():
    gen = torch.Generator().manual_seed(9)
    z = unit_pairs(21, 20, gen)
    sc, dz = closed_infonce(z, torch.full((21,), 5), 2.0, 5, 3)
    assert abs(sc[0].item()) <= 1e-14 and sc[1].item() == 1.0 and sc[2].item() == 1.0 and dz.abs().max().item() <= 1e-14


@pytest.mark.parametrize("max_norm,grad_scale", [(0.0, 1.0), (1.0, 1.0), (1e9, 1.0), (0.5, 0.25)])
def test_ref_adamw_is_torch_adamw_in_fp64(max_norm, grad_scale):
    """grad_scale: what a data-parallel mean does to the gradient before clip_grad_norm_ sees it"""
    gen = torch.Generator().manual_seed(3)
    n, lr, b1, b2, eps, wd = 300, 3e-3, 0.8, 0.95, 1e-6, 0.02
    p = torch.randn(n, generator=gen, dtype=torch.float64)
    m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    ref = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for step in range(3):
        g = torch.randn(n, generator=gen, dtype=torch.float64) * (0.5 + step)
        ref.grad = g * grad_scale
        norm = torch.linalg.vector_norm(ref.grad).item()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([ref], max_norm)
        opt.step()
        p, m, v, sumsq, clip, gn = ref_adamw(p, g, m, v, step, lr, b1, b2, eps, wd, max_norm, grad_scale)
        assert abs(gn - norm) <= 1e-13 * norm and abs(sumsq - (g * g).sum().item()) <= 1e-13 * sumsq
        want_clip = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
        assert abs(clip - want_clip) <= 1e-13 and (clip == 1.0) == (want_clip == 1.0)
        st = opt.state[ref]
        assert _rel(p, ref.detach()) <= 1e-14 and _rel(m, st["exp_avg"]) <= 1e-14 and _rel(v, st["exp_avg_sq"]) <= 1e-14


def test_ref_adamw_resumes_at_a_late_step():
    """step = 9999 with given moments == torch.optim.AdamW loaded with step 9999"""
    gen = torch.Generator().manual_seed(4)
    n = 50
    p, m, g = (torch.randn(n, generator=gen, dtype=torch.float64) for _ in range(3))
    v = torch.rand(n, generator=gen, dtype=torch.float64)
    ref = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    opt.state[ref] = {"step": torch.tensor(9999.0), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    ref.grad = g.clone()
    opt.step()
    p1, m1, v1, _, clip, _ = ref_adamw(p, g, m, v, 9999, 1e-3, 0.9, 0.999, 1e-8, 0.01, 0.0, 1.0)
    assert clip == 1.0 and _rel(p1, ref.detach()) <= 1e-14 and _rel(m1, opt.state[ref]["exp_avg"]) <= 1e-14
