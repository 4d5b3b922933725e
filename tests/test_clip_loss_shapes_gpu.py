"""mm_clip_loss_own_rows and mm_clip_loss_own_rows_grouped (csrc/clip_loss.hip) against the fp64 references of
tests/test_clip_loss_refs_host.py at the shapes where their loops change path, at three temperatures, through every
emulated rank's row0.  Inputs are L2-normalised fp64 rows rounded to fp32; the reference sees the fp32 values.

Shapes (Bg, B, N, row0s):
  (3, 3, 4)        N < 32: the float4 sweep of clip_cosines is empty; Bg < 8: clip_dz_row is all tail
  (5, 5, 36)       N % 32 tail; most 8-lane groups of clip_cosines have no column
  (21, 5, 20)      Bg % 8 != 0; row0 = 3, 16: no multiple of B or of 8, and the last rows
  (257, 257, 32)   one column past 256; B > 64 with a one-row last chunk of the scalar sum
  (320, 160, 64)   Bg > 256; B = 64 + 64 + 32
  (2048, 8, 64)    eight sweeps of every j += 256 loop; own rows at both ends
every one at s = 1 / 0.07, the three middle ones also at s = 1 and at s = 100 with correlated pairs zf = normalize(ze +
c noise), c per shape such that the fp64 mean loss lies in [1e-3, 1] (asserted: the point cannot drift to where the loss
underflows); plain, and grouped with ids distinct / pairs / one / random sizes 1..9 shuffled over the ranks and over the
256-column boundary.  Largest accepted shape: Bg = 8172, N = 4 (64 KB of LDS), against the chunked closed form.

ERR lines: dz = rel-L2 of the own rows' gradient; loss and dls = absolute error of scal4[0] and scal4[3]; dz0 = max |dz| of
pattern `one`, whose gradient is zero because P = Q, in units of the gradient's coefficient s / (2B) (an absolute figure
would be one of B: 3 .. 257 here); dzc = max |dz| of the collapsed encoder, whose gradient is zero because sum_j (P_row +
P_col)[r][j] = 2.  Measured worst cases on the MI355X against fp64 and the bounds (2x .. 4x the worst, one per quantity
and temperature; BOUND below):
              s = 1                       s = 1 / 0.07                     s = 100
  dz     3.97e-7 (320x160x64) 1.2e-6   1.21e-6 (2048x8x64)    3.5e-6   1.41e-5 (257x257x32) 4e-5
  loss   3.53e-7 (320x160x64) 1e-6     2.32e-6 (8172x4x4)     6e-6     5.94e-7 (21x5x20)    1.8e-6
  dls    9.62e-9 (21x5x20)    3e-8     1.15e-6 (257x257x32)   3.5e-6   1.10e-6 (21x5x20)    3.3e-6
  dz0    0                    0        2.89e-7 (257x257x32)   9e-7     4.69e-6 (257x257x32) 1.5e-5
  dzc                                  1.95e-6 (Bg = 21)      5e-6
The loss at s = 1 / 0.07 is worst at Bg = 8172, where it is 26 (the table's six shapes: <= 7.4e-7 on losses of 3 .. 9).
dz0 is not zero although LSE = LSE_P bit for bit there: the compiler fuses `s cos - LSE` into an FMA at some uses in
clip_rows_kernel and rounds s cos first at others, so P and Q differ by the rounding of s cos, ulp(s) / 2 relative (0 at
s = 1, where the product is exact; the same figure at every shape once divided by s / (2B)).  That is the size of the
error every probability carries anyway, from the stored LSE, one float near s.  Forcing one form was tried both ways (an
explicit fmaf per exponent; contraction off in that loop): dz0 becomes 0, and either way the gradients of a training step
move in their last bits, which tests/test_trainer_groups_gpu.py does not absorb (its three-step comparison of a grouped
and an ungrouped trainer, its fit's choice of the best epoch).  The gradient arithmetic is therefore the parent's.
dzc: sum_j P = 1 only to the rounding of the stored LSE, ulp(17) / 2 = 1e-6 at Bg = 21, times s / (2B) 2 |z| = 1.4.
Two things this module found are fixed in the kernel.  The loss was LSE - s diag, two numbers near s (1.4e-6 off at s = 100
on a loss of 0.16, 5e-6 per row); it is s (max - diag) + log(sum) now.  The scalars were scaled by a rounded 1 / B, so a
top-1 fraction was count / B to an ulp only when B is no power of two; they are divided by B.
At s = 1 / 0.07 every case also passes the older tests' element-wise check (tests/test_clip_groups_gpu.py).
Exact by contract, asserted with torch.equal: top-1 fractions (count / B rounded to fp32 once), a second run's bits, the
loss-only call's scal4 and ws, the NaN tails behind ws / dz / scal4."""
import functools
import math

import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
from test_clip_groups_gpu import _ids
from test_clip_loss_refs_host import closed_infonce, ref_infonce_ranks, unit_pairs

pytestmark = pytest.mark.gpu

SHAPES = [(3, 3, 4, (0,)), (5, 5, 36, (0,)), (21, 5, 20, (0, 3, 16)), (257, 257, 32, (0,)), (320, 160, 64, (0, 160)),
          (2048, 8, 64, (0, 2040))]
ALL_POINTS = [(21, 5, 20), (257, 257, 32), (320, 160, 64)]                  # these also run at s = 1 and s = 100
POINTS = {"s1": 1.0, "tau": 1 / 0.07, "s100": 100.0}
# (c, seed shift) of zf = normalize(ze + c noise) at s = 100, chosen on the CPU per (Bg, N) such that the fp64 loss lies inside
# WINDOW: the mean over all rows (2.7e-1, 1.2e-1, 1.4e-1) AND every rank's that is checked (Bg = 21: 2.9e-1, 1.4e-1, 2.4e-1).
# A rank whose own pairs are all separated (the first draw at Bg = 21 had one with loss 4e-5) has a gradient 1e-4 of its
# terms, s / (2B) (P_row + P_col - 2): fp32 cannot give that difference a relative error worth a bound.
C100 = {(21, 20): (1.1, 4), (257, 32): (1.1, 0), (320, 64): (1.5, 0)}
WINDOW = (1e-3, 1.0)
PATTERNS = [None, "distinct", "pairs", "one", "random"]
CASES = [(sh, "tau") for sh in SHAPES] + [(sh, pt) for sh in SHAPES if sh[:3] in ALL_POINTS for pt in ("s1", "s100")]
TAIL = 64

BOUND = {
    ("dz", "s1"): 1.2e-6, ("dz", "tau"): 3.5e-6, ("dz", "s100"): 4e-5,
    ("dz0", "s1"): 0.0, ("dz0", "tau"): 9e-7, ("dz0", "s100"): 1.5e-5,
    ("dzc", "tau"): 5e-6,
    ("loss", "s1"): 1e-6, ("loss", "tau"): 6e-6, ("loss", "s100"): 1.8e-6,
    ("dls", "s1"): 3e-8, ("dls", "tau"): 3.5e-6, ("dls", "s100"): 3.3e-6,
}
# whatever is measured: at s = 1 / 0.07 nothing here is looser than the older tests at their shapes (tests/test_kernels_gpu.py,
# tests/test_clip_groups_gpu.py: dz 1e-5 relative, 1e-6 absolute where the gradient is zero; scalars rtol 1e-5 + atol 1e-6, 4e-5
# on their losses of 4); the stricter of their element-wise checks runs on every case as well (_errors)
assert BOUND[("dz", "tau")] <= 1e-5 and BOUND[("dz0", "tau")] * (1 / 0.07) / (2 * 16) <= 1e-6       # their smallest B is 16


@functools.lru_cache(maxsize=None)
def _z(Bg, N, point):
    """-> (z_all fp32 host, ln s as the fp32 value the kernel reads)"""
    c, shift = C100[(Bg, N)] if point == "s100" else (None, 0)
    gen = torch.Generator().manual_seed(Bg * 1000 + N + len(point) + shift)
    z = unit_pairs(Bg, N, gen, c=c)
    return z, torch.tensor([math.log(POINTS[point])]).float().item()


@functools.lru_cache(maxsize=None)
def _gid(Bg, pattern):
    return None if pattern is None else _ids(pattern, Bg, torch.Generator().manual_seed(Bg + len(pattern)))


@functools.lru_cache(maxsize=None)
def _case(Bg, B, N, row0s, point, pattern):
    """-> (z_all, ids or None, ln s, [scal4 per row0], d (sum over ranks) / d z_all), fp64 autograd, computed once"""
    z, ls = _z(Bg, N, point)
    ids = _gid(Bg, pattern)
    scals, grad = ref_infonce_ranks(z, ids, ls, B, list(row0s))
    return z, ids, ls, scals, grad


def _device(z, ids, ls):
    return z.cuda(), None if ids is None else ids.to(torch.int32).cuda(), torch.tensor([ls], device="cuda")


def _nan(n):
    return torch.full((n,), float("nan"), device="cuda")


def _run(z_all, gid, ls, B, row0, grad=True):
    """one call on NaN-filled buffers with TAIL floats behind each -> (scal4, dz (B, 2N) or None, ws); the tails must stay
    NaN and everything the contract promises must be finite (`no initialisation needed`, include/mmeeg_hip.h)"""
    Bg, N2 = z_all.shape
    floats = ops.clip_loss_ws_floats(B, Bg, gid is not None)
    ws, scal, dz = _nan(floats + TAIL), _nan(4 + TAIL), _nan(B * N2 + TAIL)
    if gid is None:
        _hip.call("mm_clip_loss_own_rows", z_all, ls, scal, dz if grad else None, ws, B, Bg, N2 // 2, row0)
    else:
        _hip.call("mm_clip_loss_own_rows_grouped", z_all, gid, ls, scal, dz if grad else None, ws, B, Bg, N2 // 2, row0)
    assert torch.isnan(ws[floats:]).all() and torch.isnan(scal[4:]).all() and torch.isnan(dz[B * N2:]).all()
    assert torch.isfinite(scal[:4]).all() and torch.isfinite(ws[:floats]).all()
    if not grad:
        assert torch.isnan(dz).all()
        return scal[:4], None, ws[:floats]
    assert torch.isfinite(dz[:B * N2]).all()
    return scal[:4], dz[:B * N2].view(B, N2), ws[:floats]


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


def _errors(tag, point, scal, dz, want, g, zero_grad):
    """print the ERR lines of one call, then assert them against BOUND"""
    got = scal.cpu().double()
    d = dz.cpu().double()
    errs = {"loss": (got[0] - want[0]).abs().item(), "dls": (got[3] - want[3]).abs().item()}
    if zero_grad:                                                            # in units of the gradient's coefficient s / (2B)
        errs["dz0"] = (d - g).abs().max().item() / (POINTS[point] / (2 * d.shape[0]))
    else:
        errs["dz"] = _rel(d, g)
    for k, v in errs.items():
        print(f"ERR clip {tag} {point} {k} {v:.3e}")
    print(f"    scal {got.tolist()} want {want.tolist()} |g|max {g.abs().max().item():.3e}")
    assert torch.equal(scal[1:3].cpu(), want[1:3].float()), (got, want)    # exact: count / B rounded to fp32 once
    bad = {k: v for k, v in errs.items() if not v <= BOUND[(k, point)]}
    assert not bad, bad
    if point == "tau":                                                       # the older tests' element-wise check
        torch.testing.assert_close(d, g, rtol=1e-5, atol=max(1e-5 * g.abs().max().item(), 1e-6))
        torch.testing.assert_close(got[[0, 3]], want[[0, 3]], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("shape,point", CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v[:3])))
@pytest.mark.parametrize("pattern", PATTERNS)
def test_infonce_matches_fp64(shape, point, pattern):
    Bg, B, N, row0s = shape
    z, ids, ls, scals, grad = _case(Bg, B, N, row0s, point, pattern)
    z_all, gid, lsd = _device(z, ids, ls)
    for row0, want in zip(row0s, scals):
        scal, dz, ws = _run(z_all, gid, lsd, B, row0)
        _errors(f"{Bg}x{B}x{N} row0 {row0} {pattern}", point, scal, dz, want, grad[row0:row0 + B], pattern == "one")
        scal2, dz2, ws2 = _run(z_all, gid, lsd, B, row0)
        assert torch.equal(dz, dz2) and torch.equal(scal, scal2) and torch.equal(ws, ws2)      # bit-reproducible
        scal3, _, ws3 = _run(z_all, gid, lsd, B, row0, grad=False)          # evaluation: dz_local = NULL
        assert torch.equal(scal, scal3) and torch.equal(ws, ws3)
        if pattern == "one":                                                 # every column is a positive
            assert scal[1].item() == 1.0 and scal[2].item() == 1.0


@pytest.mark.parametrize("shape", [sh for sh in SHAPES if sh[:3] in ALL_POINTS], ids=lambda v: "x".join(map(str, v[:3])))
def test_the_hot_point_stays_inside_its_loss_window(shape):
    """s = 100: the plain fp64 loss of the correlated batch, as the mean over all rows and as every checked rank's own, is
    neither saturated nor underflown"""
    Bg, B, N, row0s = shape
    z, ls = _z(Bg, N, "s100")
    losses = [ref_infonce_ranks(z, None, ls, Bg, [0])[0][0][0].item()] + [sc[0].item() for sc in _case(*shape, "s100", None)[3]]
    print(f"s = 100, Bg {Bg} N {N} (c, seed shift) {C100[(Bg, N)]}: fp64 mean loss, then per rank {losses}")
    assert all(WINDOW[0] <= x <= WINDOW[1] for x in losses)


@pytest.mark.parametrize("Bg,B,N,row0", [(21, 5, 20, 16), (320, 160, 64, 160)])
@pytest.mark.parametrize("pattern", [None, "random"])
def test_loss_only_call_has_the_same_bits(Bg, B, N, row0, pattern):
    """dz_local = NULL (evaluation): scal4 and the workspace rows of the first launch are those of the call with dz; all
    buffers start as NaN with a NaN tail that must survive (_run)"""
    z, ls = _z(Bg, N, "tau")
    z_all, gid, lsd = _device(z, _gid(Bg, pattern), ls)
    scal, dz, ws = _run(z_all, gid, lsd, B, row0)
    scal0, none, ws0 = _run(z_all, gid, lsd, B, row0, grad=False)
    assert none is None and torch.equal(scal, scal0) and torch.equal(ws, ws0)
    assert ws.numel() == (8 if pattern else 6) * Bg


@pytest.mark.parametrize("Bg,N,r,j", [(21, 20, 4, 17), (320, 64, 300, 7)])
def test_a_tie_counts_for_the_pair(Bg, N, r, j):
    """zf_j = zf_r bit for bit: row r of C has its maximum twice.  Top-1 e->f of row r stays 1 (a tie counts FOR the pair),
    and the row softmax gives the pair at most 1/2: loss_r >= log(2) / 2."""
    gen = torch.Generator().manual_seed(Bg + r)
    z = unit_pairs(Bg, N, gen, c=0.5)                                        # correlated: the diagonal is every row's maximum
    z[j, N:] = z[r, N:]
    ls = math.log(1 / 0.07)
    want = ref_infonce_ranks(z, None, ls, 1, [r])[0][0]
    assert want[1].item() == 1.0
    z_all, _, lsd = _device(z, None, ls)
    scal, _, _ = _run(z_all, None, lsd, 1, r)                                # B = 1: scal4 is row r's own
    assert scal[1].item() == 1.0
    assert scal[0].item() >= 0.5 * math.log(2.0)
    assert abs(scal[0].item() - want[0].item()) <= BOUND[("loss", "tau")]


@pytest.mark.parametrize("Bg,B,N", [(21, 5, 20), (320, 160, 64)])
@pytest.mark.parametrize("grouped", [False, True])
def test_collapsed_encoder(Bg, B, N, grouped):
    """every row the same unit vector: C is constant, both softmaxes are uniform: loss = log Bg, top-1 = 1 both ways (ties
    count for the pair), and the gradient vanishes (sum_j (2 / Bg - 2 delta_rj) = 0)"""
    gen = torch.Generator().manual_seed(Bg)
    z = unit_pairs(1, N, gen).repeat(Bg, 1)
    z[:, N:] = z[:, :N]
    ls = torch.tensor([math.log(1 / 0.07)]).float().item()
    ids = torch.arange(Bg) if grouped else None
    z_all, gid, lsd = _device(z, ids, ls)
    for row0 in (0, Bg - B):
        scal, dz, _ = _run(z_all, gid, lsd, B, row0)
        print(f"ERR clip collapsed {Bg} grouped {int(grouped)} tau loss {abs(scal[0].item() - math.log(Bg)):.3e}")
        print(f"ERR clip collapsed {Bg} grouped {int(grouped)} tau dzc {dz.abs().max().item():.3e}")
        assert abs(scal[0].item() - math.log(Bg)) <= BOUND[("loss", "tau")]
        assert scal[1].item() == 1.0 and scal[2].item() == 1.0
        assert dz.abs().max().item() <= BOUND[("dzc", "tau")]


@pytest.mark.parametrize("pattern", [None, "pairs"])
def test_largest_accepted_shape(pattern):
    """N = 4, Bg = 8172: 2N + 2Bg + 32 = 16384 LDS words, the 64 KB clip_check_shape accepts; accepted means launchable.
    Own rows: the last four.  Reference: the chunked closed form (Bg^2 doubles would be 534 MB)."""
    Bg, B, N = 8172, 4, 4
    row0 = Bg - B
    z, ls = _z(Bg, N, "tau")
    ids = _gid(Bg, pattern)
    want, g = closed_infonce(z, ids, ls, B, row0)
    z_all, gid, lsd = _device(z, ids, ls)
    scal, dz, _ = _run(z_all, gid, lsd, B, row0)
    torch.cuda.synchronize()
    _errors(f"{Bg}x{B}x{N} row0 {row0} {pattern}", "tau", scal, dz, want, g, False)
    scal2, dz2, _ = _run(z_all, gid, lsd, B, row0)
    assert torch.equal(dz, dz2) and torch.equal(scal, scal2)


def _refused(match, z, gid, B, Bg, N, row0):
    ls = torch.zeros(1, device="cuda")
    scal, dz, ws = _nan(4), _nan(max(B, 1) * 2 * N), _nan(8 * Bg)
    with pytest.raises(_hip.HipLibraryError, match=match):
        if gid is None:
            _hip.call("mm_clip_loss_own_rows", z, ls, scal, dz, ws, B, Bg, N, row0)
        else:
            _hip.call("mm_clip_loss_own_rows_grouped", z, gid, ls, scal, dz, ws, B, Bg, N, row0)
    torch.cuda.synchronize()
    assert torch.isnan(scal).all() and torch.isnan(dz).all() and torch.isnan(ws).all()       # a host check: nothing ran


@pytest.mark.parametrize("grouped", [False, True])
def test_bad_shapes_are_refused_before_any_launch(grouped):
    z = torch.zeros(8173, 8, device="cuda")
    gid = torch.zeros(8173, dtype=torch.int32, device="cuda") if grouped else None
    _refused("B=4 Bg=8 row0=5", z, gid, 4, 8, 4, 5)                          # row0 + B > Bg
    _refused("B=0 Bg=8 row0=0", z, gid, 0, 8, 4, 0)
    _refused("multiple of 4", z, gid, 4, 8, 6, 0)
    _refused("too large for LDS", z, gid, 4, 8173, 4, 0)                     # one row more than the largest accepted shape
