"""GPU: the three kernels of csrc/perturb.hip against torch / fp64 written here, never against the code under test.

* mm_perturb_expand does no arithmetic, so it is compared with ``torch.equal`` against an index construction in torch: all
  three unit kinds, row lengths that take the 16-byte path and ones that do not, windows / blocks whose edge is no multiple
  of 4 while the row length is (a float4 then straddles two units), ragged last windows and edge blocks, every baseline
  form, a sub-range of the mask table, an input one float off a 16-byte boundary, all-ones and all-zeros masks, B of 1 and
  3, and two shapes large enough for the grid-stride loop to take more than one trip (vector and scalar path).
* mm_perturb_pair_scores against fp64: unit-norm rows, fp32 products and one fp32 sum of N terms: |err| <= N * 2^-24.
* mm_perturb_shapley against the same formula in fp64 on the same fp32 scores: one fp32 rounding of an fp64 sum
  (rtol 2e-7, atol 1e-12); efficiency: sum_u phi[b][u] = v_full[b] - v_empty[b] up to the U roundings of phi,
  |diff| <= (U + 1) * 2^-24 * max(|phi|, |v_full - v_empty|).
Both reductions give the same bits when called twice."""
import itertools

import pytest
import torch

from multimodal_eeg_fmri_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda"


def unit_map(kind, shape, size):
    """unit index of every element of one sample, in torch"""
    if kind == 0:
        return torch.arange(shape[0]).view(-1, 1).expand(shape)
    if kind == 1:
        return (torch.arange(shape[1]) // size).view(1, -1).expand(shape)
    _, D, H, W = shape
    gh, gw = -(-H // size), -(-W // size)
    d, h, w = torch.meshgrid(torch.arange(D) // size, torch.arange(H) // size, torch.arange(W) // size, indexing="ij")
    return ((d * gh + h) * gw + w).unsqueeze(0).expand(shape)


def n_units(kind, shape, size):
    if kind == 0:
        return shape[0]
    if kind == 1:
        return -(-shape[1] // size)
    return -(-shape[1] // size) * -(-shape[2] // size) * -(-shape[3] // size)


def expand_call(x, base, base_rows, masks, kind, shape, size, m0, m):
    B = x.shape[0]
    dims = tuple(shape) + (1,) * (4 - len(shape))
    out = torch.full((m * B,) + tuple(shape), float("nan"), device=DEV)
    _hip.call("mm_perturb_expand", x, base, base_rows, masks, out, B, kind, *dims, size, masks.shape[1], m0, m)
    return out


def expand_want(x, base, masks, kind, shape, size, m0, m):
    keep = masks[m0:m0 + m].cpu()[:, unit_map(kind, shape, size)].bool().to(DEV)          # (m, *shape)
    b = torch.zeros_like(x) if base is None else base.expand_as(x)
    return torch.where(keep.unsqueeze(1), x.unsqueeze(0), b.unsqueeze(0)).reshape((m * x.shape[0],) + tuple(shape))


def off_boundary(t):
    """the same values in a contiguous tensor that starts one float past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


CASES = ([(0, (3, T), 1) for T in (7, 8)]
         + [(1, (3, T), w) for T, w in ((8, 4), (8, 3), (10, 4), (12, 6))] + [(1, (1, 12), 5)]
         + [(2, (Cv, D, H, W), s) for D, H, W, s in ((4, 4, 8, 2), (5, 6, 7, 4), (4, 4, 8, 3)) for Cv in (1, 2)])


@pytest.mark.parametrize("kind,shape,size", CASES, ids=[f"k{k}-{'x'.join(map(str, s))}-s{z}" for k, s, z in CASES])
def test_expand_equals_the_index_construction(kind, shape, size):
    U = n_units(kind, shape, size)
    g = torch.Generator().manual_seed(100 * kind + sum(shape) + size)
    masks = torch.cat([torch.randint(0, 2, (5, U), generator=g), torch.ones(1, U, dtype=torch.long),
                       torch.zeros(1, U, dtype=torch.long)]).to(torch.int32).to(DEV)
    M = masks.shape[0]
    for B in (1, 3):
        x = torch.randn((B,) + tuple(shape), generator=g).to(DEV)
        bases = {0: None, 1: torch.randn((1,) + tuple(shape), generator=g).to(DEV), B: torch.randn((B,) + tuple(shape), generator=g).to(DEV)}
        for base_rows, base in bases.items():
            got = expand_call(x, base, base_rows, masks, kind, shape, size, 0, M)
            want = expand_want(x, base, masks, kind, shape, size, 0, M)
            assert torch.equal(got, want), (B, base_rows)
            assert torch.equal(got[(M - 2) * B:(M - 1) * B], x)                               # all ones: the input itself
            assert torch.equal(got[(M - 1) * B:], torch.zeros_like(x) if base is None else base.expand_as(x).contiguous())
            sub = expand_call(x, base, base_rows, masks, kind, shape, size, 1, 3)             # m0 > 0, m < M - m0
            assert torch.equal(sub, want[B:4 * B])
            # one float off a 16-byte boundary: the scalar path, the same result
            xo = off_boundary(x)
            assert torch.equal(expand_call(xo, base, base_rows, masks, kind, shape, size, 1, 3), want[B:4 * B])
            if base is not None:
                assert torch.equal(expand_call(x, off_boundary(base), base_rows, masks, kind, shape, size, 1, 3), want[B:4 * B])


@pytest.mark.parametrize("T", [11000, 2741])
def test_expand_when_the_grid_stride_loop_takes_more_than_one_trip(T):
    """3 x 64 x 11000 values = 528 000 float4 and 3 x 64 x 2741 = 526 272 scalars: both beyond the 2048 x 256 lanes of a
    grid row; windows of 6 (no multiple of 4) with a ragged tail"""
    shape, size = (64, T), 6
    U = n_units(1, shape, size)
    g = torch.Generator().manual_seed(T)
    masks = torch.randint(0, 2, (3, U), generator=g).to(torch.int32).to(DEV)
    x = torch.randn((3,) + shape, generator=g).to(DEV)
    base = torch.randn((1,) + shape, generator=g).to(DEV)
    got = expand_call(x, base, 1, masks, 1, shape, size, 1, 2)
    assert torch.equal(got, expand_want(x, base, masks, 1, shape, size, 1, 2))


@pytest.mark.parametrize("B,m,N", [(1, 1, 1), (3, 5, 70), (2, 4, 128)])
def test_pair_scores_against_fp64(B, m, N):
    g = torch.Generator().manual_seed(B * 1000 + m * 100 + N)
    z = torch.nn.functional.normalize(torch.randn(m * B, N, generator=g), dim=1).to(DEV)
    zo = torch.nn.functional.normalize(torch.randn(B, N, generator=g), dim=1).to(DEV)
    v = torch.full((m, B), float("nan"), device=DEV)
    _hip.call("mm_perturb_pair_scores", z, zo, v, B, m, N)
    want = (z.double().view(m, B, N) * zo.double().unsqueeze(0)).sum(dim=2)
    err = (v.double() - want).abs().max().item()
    print(f"PERTURB_FIG pair_scores B={B} m={m} N={N} max_abs_err={err:.3e} bound={N * 2.0 ** -24:.3e}")
    assert err <= N * 2.0 ** -24
    again = torch.empty_like(v)
    _hip.call("mm_perturb_pair_scores", z, zo, again, B, m, N)
    assert torch.equal(v, again)


def shapley_fp64(v, v_empty, v_full, perm):
    """the formula of the header in fp64: v (P, U - 1, B), perm (P, U) -> phi (B, U)"""
    P, U = perm.shape
    B = v_full.numel()
    vals = torch.cat([v_empty.double().view(1, 1, B).expand(P, 1, B), v.double().view(P, U - 1, B),
                      v_full.double().view(1, 1, B).expand(P, 1, B)], dim=1)                   # (P, U + 1, B): v(q, 0 .. U)
    phi = torch.zeros(B, U, dtype=torch.float64)
    for q in range(P):
        for place, u in enumerate(perm[q].tolist()):
            phi[:, u] += vals[q, place + 1] - vals[q, place]
    return phi / P


@pytest.mark.parametrize("B,U,P", [(1, 1, 3), (2, 4, 24), (3, 7, 5)])
def test_shapley_against_fp64_and_efficiency(B, U, P):
    g = torch.Generator().manual_seed(B * 1000 + U * 100 + P)
    if (U, P) == (4, 24):
        perm = torch.tensor(list(itertools.permutations(range(4))))
    else:
        perm = torch.stack([torch.randperm(U, generator=g) for _ in range(P)])
    pos = torch.empty(P, U, dtype=torch.int32)
    for q in range(P):
        pos[q, perm[q]] = torch.arange(1, U + 1, dtype=torch.int32)
    v = torch.randn(P, max(U - 1, 0), B, generator=g)
    ve, vf = torch.randn(B, generator=g), torch.randn(B, generator=g)
    phi = torch.full((B, U), float("nan"), device=DEV)
    args = (v.to(DEV) if U > 1 else None, ve.to(DEV), vf.to(DEV), pos.to(DEV))
    _hip.call("mm_perturb_shapley", *args, phi, B, U, P)
    want = shapley_fp64(v, ve, vf, perm)
    print(f"PERTURB_FIG shapley B={B} U={U} P={P} max_abs_err={(phi.cpu().double() - want).abs().max().item():.3e}")
    torch.testing.assert_close(phi.cpu().double(), want, rtol=2e-7, atol=1e-12)
    total = phi.cpu().double().sum(dim=1)
    gap = vf.double() - ve.double()
    scale = torch.maximum(phi.cpu().double().abs().max(dim=1).values, gap.abs())
    assert ((total - gap).abs() <= (U + 1) * 2.0 ** -24 * scale).all(), (total - gap, scale)
    again = torch.empty_like(phi)
    _hip.call("mm_perturb_shapley", *args, again, B, U, P)
    assert torch.equal(phi, again)
