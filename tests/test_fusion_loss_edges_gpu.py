"""GPU: the nine entry points of csrc/fusion.hip and the three of csrc/losses.hip at ragged shapes, with every optional
argument absent, at saturated and offset inputs and at labels outside [0, C), against the fp64 references of
oracle/fusion_tails.py (gradients by fp64 autograd).  tests/test_head_kernels_gpu.py holds the order-1 cases at one
large shape each; this file holds the branches that one does not run:

  learned fusion   rows that are no multiple of the forward's 4 per block, B < 16 (idle waves of the one-block backward),
                   H < 64, T = 0.05 (dyn / T of std 40), weights = None
  softmax2 concat  H = 1 sides, 541 800 elements (past the 2048 x 256 grid), weight logits (100, -100): a dead side
  gate mix         gate = None, 527 360 elements, gate logits x 100
  attention        head counts that leave the four waves idle or uneven (1, 3, 5), dh = 1 and dh = 96, B = 1, K = 1,
                   attw = None, the device seed-epoch word
  losses           C = 1 and 2, B = 1, B across the 256-thread stride, C = 300, dlogits = None, a class weight of 0, logits
                   offset by +-300, of std 30, and batches of confident rows only; labels -100, C and 2^32 + 1 (dropped rows)
  everything       accumulated outputs (dpa, dpc, dlogits, dtemp, loss_out) from non-zero starts, two launches bit-equal,
                   refusals that leave the outputs untouched

Bounds.  None is taken from the kernels' output.  rel-L2 against fp64 <= max(16 e32, floor): e32 = the rel-L2 error of
the same reference formula evaluated in plain fp32 torch on the CPU on the same inputs (tests/test_fusion_tails_host.py
asserts each finite, the loss ones positive), 16 as in tests/test_norm_passes_gpu.py (another operation order, __expf,
__logf); floor = the figure tests/test_head_kernels_gpu.py allows for that quantity (FLOOR below).  Accumulated outputs
are compared through a launch onto zero, which yields the increment s exactly; a launch onto a non-zero start v must
then give v + s, and a second one v + s + s, each to one rounding of the sum and one of the increment (_accumulates: the
kernels end in `out += x * y`, which compiles to one FMA, so fl32(v + fl32(x y)) bit for bit is not what they compute).
What is exact is asserted with torch.equal: the dead side at saturated weights, K = 1 attention, dproj_f's q block,
C = 1 losses, dropped rows, optional outputs left out, the plain against the train 1x2 kernel, the epoch word against
its effective seed, two launches.  K = 2 of mm_attn_1xk does NOT give the bits of mm_attn_1x2_train on the MI355X: the
sums over the two keys are one expression there and a loop over j here, and the results differ in the last bit.  Both
kernels are therefore held to fp64 on the same case at the 1x2 bounds ("K2 shared" below).
At C = 1 the smoothed CE's gradient is p - (1 - s) - s with p = 1: the one rounding of 1 - s, at most 2^-24 / B.

Figures: rel-L2.  e32 and the bound are ranges over the cases, MI355X is the worst figure measured and, in brackets, the
largest fraction of its own bound that any case used.
    quantity                              e32                  bound                MI355X
    lf T0.7 fused                         2.3e-08 .. 7.4e-08   3.7e-07 .. 1.2e-06   7.4e-08 (0.06)
    lf T0.7 weights                       3.2e-08 .. 5.0e-08   5.1e-07 .. 8.0e-07   5.1e-08 (0.07)
    lf T0.7 df0..2                        8.5e-09 .. 1.2e-07   1.5e-07 .. 1.9e-06   2.3e-07 (0.16)
    lf T0.7 ddyn                          1.1e-07 .. 1.3e-05   1.7e-06 .. 2.2e-04   1.3e-05 (0.07)
    lf T0.7 dlogits                       1.0e-07 .. 6.0e-07   1.6e-06 .. 9.6e-06   6.7e-07 (0.32)
    lf T0.7 dtemp                         2.6e-08 .. 1.7e-06   1.5e-06 .. 2.7e-05   1.1e-06 (0.11)
    lf T0.05 fused                        0 .. 7.4e-08         1.5e-07 .. 1.2e-06   7.3e-08 (0.06)
    lf T0.05 weights                      1.6e-27 .. 7.3e-08   1.4e-07 .. 1.2e-06   7.2e-08 (0.06)
    lf T0.05 df0..2                       0 .. 4.9e-07         1.5e-07 .. 7.8e-06   2.5e-06 (0.80)
    lf T0.05 ddyn                         1.9e-07 .. 7.5e-01   3.1e-06 .. 1.2e+01   1.0e+00 (0.08)
    lf T0.05 dlogits                      3.8e-07 .. 7.4e-01   6.1e-06 .. 1.2e+01   7.4e-01 (0.40)
    lf T0.05 dtemp                        3.6e-07 .. 7.1e-01   5.8e-06 .. 1.1e+01   7.1e-01 (0.43)
    s2c out                               2.0e-08 .. 4.6e-08   3.1e-07 .. 7.3e-07   3.3e-08 (0.06)
    s2c da                                1.2e-08 .. 5.0e-08   2.0e-07 .. 8.0e-07   5.0e-08 (0.06)
    s2c dc                                2.1e-10 .. 5.1e-08   9.0e-08 .. 8.1e-07   3.1e-08 (0.06)
    s2c dpa                               4.7e-08 .. 4.4e-07   7.5e-07 .. 7.0e-06   2.0e-07 (0.07)
    s2c dpc                               7.7e-09 .. 4.4e-07   1.2e-07 .. 7.0e-06   2.0e-07 (0.07)
    s2c saturated out                     0                    8.0e-08              2.2e-86 (0.00)
    s2c saturated da                      0                    7.5e-08              0.0e+00 (0.00)
    s2c saturated dc                      0                    9.0e-08              0.0e+00 (0.00)
    gate x1 comb                          2.6e-08 .. 3.6e-08   4.2e-07 .. 5.8e-07   3.5e-08 (0.06)
    gate x1 gate                          2.5e-08 .. 4.5e-08   3.9e-07 .. 7.3e-07   3.9e-08 (0.06)
    gate x1 derp                          4.2e-08 .. 5.1e-08   6.8e-07 .. 8.1e-07   4.7e-08 (0.06)
    gate x1 dpw                           3.0e-08 .. 1.1e-07   4.8e-07 .. 1.7e-06   1.1e-07 (0.06)
    gate x1 dconn                         0 .. 3.0e-08         8.0e-08 .. 4.8e-07   3.0e-08 (0.06)
    gate x1 dg                            1.2e-08 .. 2.3e-07   4.5e-07 .. 3.8e-06   2.3e-07 (0.07)
    gate x100 comb                        2.3e-08 .. 2.6e-08   3.6e-07 .. 4.1e-07   2.6e-08 (0.06)
    gate x100 gate                        0 .. 8.3e-09         1.1e-07 .. 1.3e-07   8.3e-09 (0.06)
    gate x100 derp                        0 .. 8.8e-09         1.3e-07 .. 1.4e-07   8.9e-09 (0.06)
    gate x100 dpw                         0 .. 1.5e-08         1.3e-07 .. 2.4e-07   1.5e-08 (0.06)
    gate x100 dconn                       0 .. 3.0e-08         8.0e-08 .. 4.8e-07   3.0e-08 (0.06)
    gate x100 dg                          4.1e-08 .. 1.0e+00   6.5e-07 .. 1.6e+01   1.0e+00 (0.06)
    attn_1x2 ctx                          3.0e-08 .. 1.4e-07   4.7e-07 .. 2.2e-06   1.4e-07 (0.08)
    attn_1x2 attw                         1.7e-09 .. 7.0e-08   1.9e-07 .. 1.1e-06   8.8e-08 (0.18)
    attn_1x2 dp0                          5.2e-08 .. 1.1e-07   8.3e-07 .. 1.8e-06   3.5e-07 (0.25)
    attn_1x2 dp1                          5.3e-08 .. 3.1e-07   8.5e-07 .. 4.9e-06   2.1e-07 (0.21)
    attn_1xk ctx                          0 .. 1.7e-07         2.3e-07 .. 2.8e-06   2.3e-07 (0.17)
    attn_1xk attw                         0 .. 9.8e-08         1.6e-07 .. 1.6e-06   1.0e-07 (0.23)
    attn_1xk dp0..3                       0 .. 3.1e-07         3.0e-07 .. 5.0e-06   2.9e-07 (0.18)
    attn K2 shared (every quantity)       1.7e-09 .. 3.1e-07   1.9e-07 .. 4.9e-06   3.5e-07 (0.25)
    weighted shapes dl                    4.4e-08 .. 1.3e-07   7.0e-06              1.0e-06 (0.14)
    weighted shapes loss                  6.5e-09 .. 8.4e-08   7.0e-06              5.1e-07 (0.07)
    focal shapes per                      1.8e-09 .. 7.1e-08   3.0e-07 .. 1.1e-06   7.4e-08 (0.18)
    focal shapes loss                     1.8e-10 .. 9.5e-08   4.5e-07 .. 1.5e-06   1.2e-07 (0.19)
    focal shapes dl                       2.8e-08 .. 1.0e-07   4.4e-07 .. 1.6e-06   1.0e-07 (0.22)
    smoothed shapes loss                  2.7e-09 .. 9.7e-08   2.5e-07 .. 1.5e-06   5.7e-08 (0.13)
    smoothed shapes dl                    4.4e-08 .. 1.4e-07   7.0e-07 .. 2.2e-06   1.4e-07 (0.08)
    weighted order1 loss                  6.5e-09 .. 8.4e-08   7.0e-06              5.1e-07 (0.07)
    weighted order1 dl                    4.4e-08 .. 8.0e-08   7.0e-06              1.0e-06 (0.14)
    focal order1 per                      3.8e-08 .. 6.4e-08   6.0e-07 .. 1.0e-06   6.5e-08 (0.07)
    focal order1 loss                     8.8e-09 .. 9.5e-08   4.5e-07 .. 1.5e-06   1.1e-07 (0.19)
    focal order1 dl                       3.7e-08 .. 7.9e-08   5.9e-07 .. 1.3e-06   7.9e-08 (0.08)
    smoothed order1 loss                  6.5e-09 .. 9.7e-08   2.5e-07 .. 1.5e-06   5.7e-08 (0.06)
    smoothed order1 dl                    4.4e-08 .. 1.2e-07   7.0e-07 .. 2.0e-06   6.9e-08 (0.06)
    weighted offset loss                  4.7e-08 .. 7.0e-07   7.0e-06 .. 1.1e-05   6.3e-07 (0.08)
    weighted offset dl                    4.2e-08 .. 7.6e-08   7.0e-06              1.0e-06 (0.14)
    focal offset per                      2.6e-06 .. 4.6e-06   4.1e-05 .. 7.3e-05   4.6e-06 (0.06)
    focal offset loss                     8.9e-08 .. 7.4e-07   1.4e-06 .. 1.2e-05   7.4e-07 (0.18)
    focal offset dl                       3.5e-08 .. 3.7e-06   5.6e-07 .. 5.9e-05   3.7e-06 (0.07)
    smoothed offset loss                  4.7e-08 .. 6.5e-07   7.5e-07 .. 1.0e-05   7.3e-07 (0.29)
    smoothed offset dl                    4.2e-08 .. 1.2e-07   6.7e-07 .. 1.9e-06   6.7e-08 (0.07)
    weighted spread loss                  2.1e-09 .. 7.9e-08   7.0e-06              8.9e-07 (0.13)
    weighted spread dl                    1.5e-08 .. 6.7e-08   7.0e-06              9.8e-07 (0.14)
    focal spread per                      2.6e-08 .. 4.2e-08   4.2e-07 .. 6.8e-07   4.2e-08 (0.06)
    focal spread loss                     1.3e-09 .. 1.5e-07   4.5e-07 .. 2.4e-06   9.1e-08 (0.07)
    focal spread dl                       1.7e-08 .. 4.8e-08   2.7e-07 .. 7.7e-07   5.2e-08 (0.09)
    smoothed spread loss                  4.3e-10 .. 7.9e-08   2.5e-07 .. 1.3e-06   1.5e-07 (0.27)
    smoothed spread dl                    1.5e-08 .. 1.0e-07   3.0e-07 .. 1.6e-06   6.3e-08 (0.09)
    weighted confident loss               4.9e-07 .. 5.5e-05   7.8e-06 .. 8.8e-04   4.0e-05 (0.06)
    weighted confident dl                 1.7e-05 .. 3.8e-05   2.8e-04 .. 6.0e-04   3.9e-05 (0.13)
    focal confident per                   1.2e-04 .. 3.8e-04   1.9e-03 .. 6.0e-03   3.8e-04 (0.06)
    focal confident loss                  5.2e-07 .. 5.5e-05   8.4e-06 .. 8.8e-04   4.0e-05 (0.62)
    focal confident dl                    2.1e-05 .. 1.9e-04   3.4e-04 .. 3.0e-03   1.9e-04 (0.11)
    smoothed confident loss               7.6e-09 .. 5.5e-05   2.5e-07 .. 8.8e-04   4.0e-05 (0.08)
    smoothed confident dl                 6.4e-08 .. 3.8e-05   1.0e-06 .. 6.0e-04   3.9e-05 (0.14)
    weighted zero weight loss             7.1e-09              7.0e-06              4.1e-07 (0.06)
    weighted zero weight dl               5.1e-08              7.0e-06              6.2e-07 (0.09)
    weighted labels loss                  5.0e-08 .. 1.0e-07   7.0e-06              5.0e-08 (0.01)
    weighted labels dl                    5.0e-08 .. 7.0e-08   7.0e-06              1.1e-07 (0.02)
    focal labels per                      3.8e-08 .. 6.4e-08   6.0e-07 .. 1.0e-06   6.5e-08 (0.07)
    focal labels loss                     2.4e-09 .. 1.1e-07   4.5e-07 .. 1.8e-06   1.1e-07 (0.12)
    focal labels dl                       4.7e-08 .. 7.9e-08   7.5e-07 .. 1.3e-06   7.8e-08 (0.07)
    smoothed labels loss                  7.4e-10 .. 8.0e-08   2.5e-07 .. 1.3e-06   8.6e-08 (0.34)
    smoothed labels dl                    4.4e-08 .. 7.0e-08   7.0e-07 .. 1.1e-06   6.9e-08 (0.06)
Groups: lf = learned fusion (per temperature), s2c = softmax2 concat, gate = gate mix (per gate-logit scale), attn_* per
kernel, the losses per input family ("shapes" = the order-1 inputs over every (B, C)).  Where a softmax is saturated on
every row of a small case (ddyn, dlogits, dtemp at T = 0.05 with B <= 5; dg at gate logits x 100 with B <= 6) the fp64
gradient lies below fp32's underflow, the fp32 evaluation returns 0, e32 is of order 1 and the bound says nothing;
the larger shapes of the same group, where unsaturated rows carry the norm, are the check (their e32 is the low end).
Every figure is printed as "FIG <group> | <quantity> | <e32> | <bound> | <measured>" before anything is asserted.

Kernel changes made with these tests: the three loss kernels compare the 64-bit label with [0, C) before they index
anything with it (they used to cast it to int and read z[t], cw[t]); mm_learned_fusion_bwd and mm_softmax2_concat_bwd
refuse B = 0 / H = 0 like the other entry points (the former returned 0 and launched)."""
import pytest
import torch

from oracle import fusion_tails as R
from test_head_kernels_gpu import _Errs, _cu, _rel, keep_scale
from test_kernels_gpu import _hip

pytestmark = pytest.mark.gpu

NAN = float("nan")
# the bounds of tests/test_head_kernels_gpu.py at order-1 inputs
FLOOR = {
    "lf": dict(fused=1.5e-7, weights=1.4e-7, df0=1.5e-7, df1=1.5e-7, df2=1.5e-7, ddyn=6e-7, dlogits=9e-7, dtemp=1.5e-6),
    "s2c": dict(out=8e-8, da=7.5e-8, dc=9e-8, dpa=5e-9, dpc=5e-9),
    "gate": dict(comb=1e-7, gate=1.1e-7, derp=1.3e-7, dpw=1.3e-7, dconn=8e-8, dg=4.5e-7),
    "attn_1x2": dict(ctx=1.8e-7, attw=1.9e-7, dp0=3e-7, dp1=2.7e-7),
    "attn_1xk": dict(ctx=2.3e-7, attw=1.6e-7, dp0=3e-7, dp1=3e-7, dp2=3e-7, dp3=3e-7),
    "weighted": dict(loss=7e-6, dl=7e-6),
    "focal": dict(loss=4.5e-7, per=3e-7, dl=2.5e-7),
    "smoothed": dict(loss=2.5e-7, dl=3e-7),
}


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


class _Chk(_Errs):
    """_Errs with the bound max(16 e32, floor) and a finiteness check"""

    def __init__(self, group, tag):
        super().__init__(f"{group} {tag}")
        self.group = group

    def vs(self, name, got, want, e32, where=""):
        assert bool(torch.isfinite(got).all()), f"{self.tag} {name}: not finite"
        err, bound = _rel(got, want), R.bound(e32[name], FLOOR[self.group][name])
        print(f"FIG {self.group}{where} | {name} | {e32[name]:.3e} | {bound:.3e} | {err:.3e}")
        self(name, err, bound)


def _accumulates(launch, starts, names):
    """``launch(starts) -> tensors`` adds onto copies of ``starts``.  Returns the increments s (a launch onto zeros: exact)
    after asserting that a launch onto ``starts`` = v gives v + s, a second one onto that result v + s + s, and that two
    launches onto v give the same bits.  The kernels end in `out += x * y`, which the compiler may fuse (one rounding of
    v + x y instead of fl(v + fl(x y))): each sum is held to one rounding of itself and one of the increment,
    |got - (v + s)| <= 2^-24 (|got| + |s|), computed in fp64, where v + s is exact"""
    s = launch([torch.zeros_like(v) for v in starts])
    v1 = launch([v.clone() for v in starts])
    v1b = launch([v.clone() for v in starts])
    v2 = launch([v.clone() for v in v1])
    for n, v, a, a2, b, inc in zip(names, starts, v1, v1b, v2, s):
        assert bool((v != 0).all()), n
        assert torch.equal(a, a2), f"{n}: two launches onto the same start"
        v, a, b, inc = (t.detach().cpu().double() for t in (v, a, b, inc))
        for tag, got, base in (("first", a, v), ("second", b, a)):
            slack = 2.0 ** -24 * (got.abs() + inc.abs())
            assert bool(((got - (base + inc)).abs() <= slack).all()), f"{n}: {tag} launch onto a non-zero start"
    return s


def _refused(hip, name, outs, *args):
    with pytest.raises(hip.HipLibraryError, match=rf"{name} failed \(-"):
        hip.call(name, *args)
    torch.cuda.synchronize()
    for o in outs:
        assert bool(torch.isnan(o).all()), f"{name}: a refused call wrote an output"


# ------------------------------------------------------------------------------------------------------ learned fusion
def _lf_fwd(hip, c, weights=True):
    M, (B, H) = len(c["feats"]), c["feats"][0].shape
    f = [_cu(t) for t in c["feats"]] + [None] * (3 - M)
    fused, w = _nan(B, H), _nan(B, M) if weights else None
    hip.call("mm_learned_fusion", f[0], f[1], f[2], _cu(c["dyn"]), _cu(c["logits"]), _cu(c["temp"]), fused, w, B, H, M)
    return fused, w


def _lf_bwd(hip, c, starts):
    M, (B, H) = len(c["feats"]), c["feats"][0].shape
    f = [_cu(t) for t in c["feats"]] + [None] * (3 - M)
    dfs = [_nan(B, H) for _ in range(M)] + [None] * (3 - M)
    ddyn, dlog, dtemp = _nan(B, M), _cu(starts[0].clone()), _cu(starts[1].clone())
    hip.call("mm_learned_fusion_bwd", f[0], f[1], f[2], _cu(c["dyn"]), _cu(c["logits"]), _cu(c["temp"]), _cu(c["dfused"]),
             dfs[0], dfs[1], dfs[2], ddyn, dlog, dtemp, B, H, M)
    return dfs[:M] + [ddyn], [dlog, dtemp]


@pytest.mark.parametrize("T", [0.7, 0.05])
@pytest.mark.parametrize("B,H", R.LF_SHAPES)
@pytest.mark.parametrize("M", [2, 3])
def test_learned_fusion_ragged_rows_and_sharp_temperature(M, B, H, T):
    hip = _hip()
    c = R.learned_fusion_case(M, B, H, T)
    want, e32 = R.case_e32(R.learned_fusion_eval, c)
    chk = _Chk("lf", f"M{M} B{B} H{H} T{T}")
    fused, w = _lf_fwd(hip, c)
    chk.vs("fused", fused, want["fused"], e32, f" T{T}")
    chk.vs("weights", w, want["weights"], e32, f" T{T}")
    assert torch.equal(_lf_fwd(hip, c, weights=False)[0], fused)              # weights is optional
    again = _lf_fwd(hip, c)
    assert torch.equal(again[0], fused) and torch.equal(again[1], w)
    g = torch.Generator().manual_seed(B + H)
    starts = [torch.randn(M, generator=g) + 3.0, torch.randn(1, generator=g) - 3.0]
    stores = {}

    def launch(st):
        plain, acc = _lf_bwd(hip, c, st)
        if stores:                                                             # every launch: the same stored bits
            assert all(torch.equal(a, b) for a, b in zip(plain, stores["v"]))
        stores["v"] = plain
        return acc

    dlog, dtemp = _accumulates(launch, starts, ("dlogits", "dtemp"))
    for m in range(M):
        chk.vs(f"df{m}", stores["v"][m], want[f"df{m}"], e32, f" T{T}")
    chk.vs("ddyn", stores["v"][M], want["ddyn"], e32, f" T{T}")
    chk.vs("dlogits", dlog, want["dlogits"], e32, f" T{T}")
    chk.vs("dtemp", dtemp, want["dtemp"], e32, f" T{T}")
    chk.done()


# ----------------------------------------------------------------------------------------------------- softmax2 concat
def _s2c_bwd(hip, c, starts):
    B, Ha, Hc = c["a"].shape[0], c["a"].shape[1], c["c"].shape[1]
    da, dc, dpa, dpc = _nan(B, Ha), _nan(B, Hc), _cu(starts[0].clone()), _cu(starts[1].clone())
    hip.call("mm_softmax2_concat_bwd", _cu(c["dout"]), _cu(c["a"]), _cu(c["c"]), _cu(c["pa"]), _cu(c["pc"]), da, dc, dpa, dpc,
             B, Ha, Hc)
    return [da, dc], [dpa, dpc]


@pytest.mark.parametrize("pa,pc", R.S2C_LOGITS)
@pytest.mark.parametrize("B,Ha,Hc", R.S2C_SHAPES)
def test_softmax2_concat_past_the_grid_and_at_saturated_weights(B, Ha, Hc, pa, pc):
    hip = _hip()
    c = R.s2c_case(B, Ha, Hc, pa, pc)
    want, e32 = R.case_e32(R.s2c_eval, c)
    where = " saturated" if abs(pa) == 100 else ""
    chk = _Chk("s2c", f"B{B} Ha{Ha} Hc{Hc} pa{pa}")
    outs = []
    for _ in range(2):
        outs.append(_nan(B, Ha + Hc))
        hip.call("mm_softmax2_concat", _cu(c["a"]), _cu(c["c"]), _cu(c["pa"]), _cu(c["pc"]), outs[-1], B, Ha, Hc)
    assert torch.equal(outs[0], outs[1])
    chk.vs("out", outs[0], want["out"], e32, where)
    starts = [torch.tensor([0.25]), torch.tensor([-0.5])]
    stores = {}

    def launch(st):
        plain, acc = _s2c_bwd(hip, c, st)
        if stores:
            assert all(torch.equal(a, b) for a, b in zip(plain, stores["v"]))
        stores["v"] = plain
        return acc

    dpa, dpc = _accumulates(launch, starts, ("dpa", "dpc"))
    da, dc = stores["v"]
    if not where:
        for n, t in (("da", da), ("dc", dc), ("dpa", dpa), ("dpc", dpc)):
            chk.vs(n, t, want[n], e32)
    else:                                            # one weight is exactly 0 in fp32: its side is dead, no logit moves
        live, dead, dead_out = (da, dc, outs[0][:, Ha:]) if pa > 0 else (dc, da, outs[0][:, :Ha])
        chk.vs("da" if pa > 0 else "dc", live, want["da" if pa > 0 else "dc"], e32, where)
        assert bool((dead_out == 0).all()) and bool((dead == 0).all())
        assert bool((dpa == 0).all()) and bool((dpc == 0).all())              # increments of exactly 0: dpa, dpc unchanged
    chk.done()


# ------------------------------------------------------------------------------------------------------------ gate mix
def _gate_fwd(hip, c, gate=True):
    B, H = c["erp"].shape
    comb, gt = _nan(B, 2 * H), _nan(B, 2) if gate else None
    hip.call("mm_gate2_mix", _cu(c["g"]), _cu(c["erp"]), _cu(c["pw"]), _cu(c["conn"]), comb, gt, B, H, c["boost"])
    return comb, gt


@pytest.mark.parametrize("mult", [1, 100])
@pytest.mark.parametrize("B,H", R.GATE_SHAPES)
def test_gate2_mix_ragged_rows_past_the_grid_and_sharp_gates(B, H, mult):
    hip = _hip()
    c = R.gate_case(B, H, mult)
    want, e32 = R.case_e32(R.gate_eval, c)
    chk = _Chk("gate", f"B{B} H{H} x{mult}")
    comb, gt = _gate_fwd(hip, c)
    chk.vs("comb", comb, want["comb"], e32, f" x{mult}")
    chk.vs("gate", gt, want["gate"], e32, f" x{mult}")
    assert torch.equal(_gate_fwd(hip, c, gate=False)[0], comb)                 # gate is optional
    again = _gate_fwd(hip, c)
    assert torch.equal(again[0], comb) and torch.equal(again[1], gt)
    runs = []
    for _ in range(2):
        runs.append([_nan(B, H), _nan(B, H), _nan(B, H), _nan(B, 2)])
        hip.call("mm_gate2_mix_bwd", _cu(c["dcomb"]), _cu(c["g"]), _cu(c["erp"]), _cu(c["pw"]), *runs[-1], B, H, c["boost"])
    for n, a, b in zip(("derp", "dpw", "dconn", "dg"), *runs):
        assert torch.equal(a, b), n
        chk.vs(n, a, want[n], e32, f" x{mult}")
    chk.done()


# ----------------------------------------------------------------------------------------------------------- attention
SEED = 515


def _x2(hip, c, B, p, seed, epoch, backward, attw=True, plain=False):
    E, nhead = c["E"], c["nhead"]
    pe, pf = (_cu(t) for t in c["ps"])
    if plain:
        ctx, aw = _nan(B, E), _nan(B, 2)
        hip.call("mm_attn_1x2", pe, pf, ctx, aw, B, E, nhead)
        return [ctx, aw]
    if not backward:
        ctx, aw = _nan(B, E), _nan(B, 2) if attw else None
        hip.call("mm_attn_1x2_train", pe, pf, None, ctx, aw, None, None, B, E, nhead, p, seed, epoch, 0)
        return [ctx, aw]
    dpe, dpf = _nan(B, 3 * E), _nan(B, 3 * E)
    hip.call("mm_attn_1x2_train", pe, pf, _cu(c["dctx"]), None, None, dpe, dpf, B, E, nhead, p, seed, epoch, 1)
    return [dpe, dpf]


def _xk(hip, c, B, p, seed, epoch, backward, attw=True):
    E, nhead, K = c["E"], c["nhead"], len(c["ps"])
    pc = [_cu(t) for t in c["ps"]] + [None] * (4 - K)
    if not backward:
        ctx, aw = _nan(B, E), _nan(B, K) if attw else None
        hip.call("mm_attn_1xk", *pc, K, None, ctx, aw, None, None, None, None, B, E, nhead, p, seed, epoch, 0)
        return [ctx, aw]
    dps = [_nan(B, 3 * E) for _ in range(K)] + [None] * (4 - K)
    hip.call("mm_attn_1xk", *pc, K, _cu(c["dctx"]), None, None, *dps, B, E, nhead, p, seed, epoch, 1)
    return dps[:K]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("E,nhead", R.ATTN_SHAPES)
def test_attn_1x2_uneven_heads_and_head_dims(E, nhead, B):
    hip = _hip()
    c = R.attn_case(E, nhead, B, 2)
    for p in (0.0, 0.25):
        keep = keep_scale(SEED, B * nhead * 2, p).view(B, nhead, 2)
        want, e32 = R.case_e32(R.attn_eval, c, keep)
        chk = _Chk("attn_1x2", f"E{E} h{nhead} B{B} p{p}")
        ctx, aw = _x2(hip, c, B, p, SEED, None, 0)
        chk.vs("ctx", ctx, want["ctx"], e32)
        chk.vs("attw", aw, want["attw"], e32)
        assert torch.equal(_x2(hip, c, B, p, SEED, None, 0, attw=False)[0], ctx)   # attw is optional
        assert _same(_x2(hip, c, B, p, SEED, None, 0), [ctx, aw])
        if p == 0:                                                             # the eval entry point is the same kernel
            assert _same(_x2(hip, c, B, p, SEED, None, 0, plain=True), [ctx, aw])
        dpe, dpf = _x2(hip, c, B, p, SEED, None, 1)
        chk.vs("dp0", dpe, want["dp0"], e32)
        chk.vs("dp1", dpf, want["dp1"], e32)
        assert bool((dpf[:, :E] == 0).all())                                   # the second token's q is unused
        assert _same(_x2(hip, c, B, p, SEED, None, 1), [dpe, dpf])
        chk.done()


@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("E,nhead", R.ATTN_SHAPES)
def test_attn_1xk_uneven_heads_head_dims_and_one_key(E, nhead, B, K):
    hip = _hip()
    c = R.attn_case(E, nhead, B, K)
    for p in (0.0, 0.25):
        keep = keep_scale(SEED, B * nhead * K, p).view(B, nhead, K)
        want, e32 = R.case_e32(R.attn_eval, c, keep)
        chk = _Chk("attn_1xk", f"E{E} h{nhead} B{B} K{K} p{p}")
        ctx, aw = _xk(hip, c, B, p, SEED, None, 0)
        chk.vs("ctx", ctx, want["ctx"], e32)
        chk.vs("attw", aw, want["attw"], e32)
        assert torch.equal(_xk(hip, c, B, p, SEED, None, 0, attw=False)[0], ctx)
        assert _same(_xk(hip, c, B, p, SEED, None, 0), [ctx, aw])
        dps = _xk(hip, c, B, p, SEED, None, 1)
        for j in range(K):
            chk.vs(f"dp{j}", dps[j], want[f"dp{j}"], e32)
            if j:
                assert bool((dps[j][:, :E] == 0).all())
        assert _same(_xk(hip, c, B, p, SEED, None, 1), dps)
        if K == 1:                               # one key: probability 1, whatever the score
            v0 = c["ps"][0][:, 2 * E:].view(B, nhead, E // nhead)
            assert bool((aw == 1).all())
            assert torch.equal(ctx.cpu(), (keep * v0).reshape(B, E))
            assert bool((dps[0][:, :2 * E] == 0).all())                        # dq = dk = 0
        if K == 2:                               # the two-key kernel on the same seed: another rounding order (see above),
            two = _Chk("attn_1x2", f"E{E} h{nhead} B{B} p{p} against 1xk")          # so both are held to its bounds
            for got in (_x2(hip, c, B, p, SEED, None, 0) + _x2(hip, c, B, p, SEED, None, 1), [ctx, aw] + dps):
                for n, t in zip(("ctx", "attw", "dp0", "dp1"), got):
                    two.vs(n, t, want[n], e32, " K2 shared")
            chk.rows += two.rows
        chk.done()


def _eff_seed(seed, epoch):
    """csrc/common.h: mm_eff_seed"""
    return seed if epoch is None else (seed ^ ((epoch * 0x85EBCA6B + 0xC2B2AE35) & 0xFFFFFFFF)) & 0xFFFFFFFF


@pytest.mark.parametrize("run,K", [(_x2, 2), (_xk, 3)])
def test_attn_seed_epoch_word_is_the_effective_seed(run, K):
    hip = _hip()
    E, nhead, B, p, seed = 80, 5, 5, 0.25, 0x1234567
    c = R.attn_case(E, nhead, B, K)
    res = {}
    for e in (3, 4):
        ep = torch.tensor([e], dtype=torch.int32, device="cuda")
        eff = _eff_seed(seed, e)
        for backward in (0, 1):
            res[e, backward] = run(hip, c, B, p, seed, ep, backward)
            assert _same(res[e, backward], run(hip, c, B, p, eff, None, backward))
        keep = keep_scale(eff, B * nhead * K, p).view(B, nhead, K)
        want, e32 = R.case_e32(R.attn_eval, c, keep)
        assert _rel(res[e, 0][0], want["ctx"]) <= R.bound(e32["ctx"], FLOOR["attn_1x2" if K == 2 else "attn_1xk"]["ctx"])
    k3, k4 = (keep_scale(_eff_seed(seed, e), B * nhead * K, p) for e in (3, 4))
    assert not torch.equal(k3, k4)                                             # another epoch, another mask
    assert not torch.equal(res[3, 0][0], res[4, 0][0]) and not torch.equal(res[3, 1][0], res[4, 1][0])


# ------------------------------------------------------------------------------------------------------------ refusals
def test_fusion_entry_points_refuse_bad_arguments_without_writing():
    """a negative code and untouched outputs.  B = 0 is passed with the buffers of B = 1, so that the check met is the
    one on B and not the null pointer of an empty tensor"""
    hip = _hip()
    B, H, E = 1, 8, 8

    def x(*s):
        return torch.randn(*s).cuda()

    f, one = x(B, H), x(1)
    for M, f2 in ((1, f), (4, f), (3, None)):
        outs = [_nan(B, H), _nan(B, max(M, 1))]
        _refused(hip, "mm_learned_fusion", outs, f, f, f2, x(B, 4), x(4), one, *outs, B, H, M)
        outs = [_nan(B, H), _nan(B, H), _nan(B, H), _nan(B, 4), _nan(4), _nan(1)]
        _refused(hip, "mm_learned_fusion_bwd", outs, f, f, f2, x(B, 4), x(4), one, f, *outs, B, H, M)
    pe = x(B, 3 * E)
    for E_, nhead in ((34, 17), (10, 4)):
        p_ = x(B, 3 * E_)
        outs = [_nan(B, E_), _nan(B, 2)]
        _refused(hip, "mm_attn_1x2", outs, p_, p_, *outs, B, E_, nhead)
        _refused(hip, "mm_attn_1x2_train", outs, p_, p_, None, *outs, None, None, B, E_, nhead, 0.0, 1, None, 0)
        _refused(hip, "mm_attn_1xk", outs, p_, p_, None, None, 2, None, *outs, None, None, None, None, B, E_, nhead, 0.0, 1, None, 0)
        outs = [_nan(B, 3 * E_), _nan(B, 3 * E_)]
        _refused(hip, "mm_attn_1x2_train", outs, p_, p_, x(B, E_), None, None, *outs, B, E_, nhead, 0.0, 1, None, 1)
    for K, toks in ((0, [pe] * 4), (5, [pe] * 4), (3, [pe, None, pe, None]), (2, [None, pe, None, None])):
        outs = [_nan(B, E), _nan(B, 4)]
        _refused(hip, "mm_attn_1xk", outs, *toks, K, None, *outs, None, None, None, None, B, E, 2, 0.0, 1, None, 0)
        outs = [_nan(B, 3 * E) for _ in range(4)]
        _refused(hip, "mm_attn_1xk", outs, *toks, K, x(B, E), None, None, *outs, B, E, 2, 0.0, 1, None, 1)
    # B = 0, every entry point
    outs = [_nan(B, 2 * H)]
    _refused(hip, "mm_softmax2_concat", outs, f, f, one, one, *outs, 0, H, H)
    outs = [_nan(B, H), _nan(B, H), _nan(1), _nan(1)]
    _refused(hip, "mm_softmax2_concat_bwd", outs, x(B, 2 * H), f, f, one, one, *outs, 0, H, H)
    outs = [_nan(B, H), _nan(B, 2)]
    _refused(hip, "mm_learned_fusion", outs, f, f, None, x(B, 2), x(2), one, *outs, 0, H, 2)
    outs = [_nan(B, H), _nan(B, H), _nan(B, 2), _nan(2), _nan(1)]
    _refused(hip, "mm_learned_fusion_bwd", outs, f, f, None, x(B, 2), x(2), one, f, outs[0], outs[1], None, *outs[2:], 0, H, 2)
    outs = [_nan(B, E), _nan(B, 2)]
    _refused(hip, "mm_attn_1x2", outs, pe, pe, *outs, 0, E, 2)
    _refused(hip, "mm_attn_1x2_train", outs, pe, pe, None, *outs, None, None, 0, E, 2, 0.0, 1, None, 0)
    _refused(hip, "mm_attn_1xk", outs, pe, pe, None, None, 2, None, *outs, None, None, None, None, 0, E, 2, 0.0, 1, None, 0)
    outs = [_nan(B, 2 * H), _nan(B, 2)]
    _refused(hip, "mm_gate2_mix", outs, x(B, 2), f, f, f, *outs, 0, H, 1.5)
    outs = [_nan(B, H), _nan(B, H), _nan(B, H), _nan(B, 2)]
    _refused(hip, "mm_gate2_mix_bwd", outs, x(B, 2 * H), x(B, 2), f, f, *outs, 0, H, 1.5)


def test_losses_refuse_bad_arguments_without_writing():
    hip = _hip()
    B, C = 1, 3
    z, t = torch.randn(B, C).cuda(), torch.zeros(B, dtype=torch.int64).cuda()
    for s in (1.0, -0.1):
        outs = [_nan(1), _nan(B, C)]
        _refused(hip, "mm_smoothed_ce", outs, z, t, *outs, B, C, s)
    outs = [_nan(1), _nan(B, C)]
    _refused(hip, "mm_smoothed_ce", outs, z, t, *outs, 0, C, 0.1)
    _refused(hip, "mm_weighted_ce", outs, z, t, None, *outs, 0, C)
    outs = [_nan(1), _nan(B), _nan(B, C)]
    _refused(hip, "mm_focal_loss", outs, z, t, *outs, 0, C, 0.8, 2.0, 1.0)


# -------------------------------------------------------------------------------------------------------------- losses
def _loss_calls(B, C):
    cw = 0.2 + torch.rand(C, generator=torch.Generator().manual_seed(C))
    return [("weighted", {}), ("weighted", dict(cw=cw))] + \
           [("focal", dict(alpha=a, gamma=gm, scale=sc)) for gm in (0.0, 0.5, 1.0, 2.0) for a, sc in ((0.8, 1.0 / B), (0.25, 1.0))] + \
           [("smoothed", dict(s=s)) for s in (0.0, 0.1, 0.5)]


def _loss_launch(hip, kind, z, t, kw, start, dl=True, per=True):
    """one launch onto loss_out = start; returns dict(loss, dl, per) of device tensors (None where left out)"""
    B, C = z.shape
    out = _cu(start.clone())
    dlt = _nan(B, C) if dl else None
    pert = _nan(B) if per and kind == "focal" else None
    if kind == "weighted":
        hip.call("mm_weighted_ce", _cu(z), _cu(t), _cu(kw["cw"]) if "cw" in kw else None, out, dlt, B, C)
    elif kind == "focal":
        hip.call("mm_focal_loss", _cu(z), _cu(t), out, pert, dlt, B, C, kw["alpha"], kw["gamma"], kw["scale"])
    else:
        hip.call("mm_smoothed_ce", _cu(z), _cu(t), out, dlt, B, C, kw["s"])
    return dict(loss=out, dl=dlt, per=pert)


def _loss_run(hip, kind, z, t, kw):
    """the launches every loss case makes: onto zero (the increment), twice onto a non-zero loss_out (accumulation and
    two-launch bit equality of the stores), without the optional outputs (same loss bits)"""
    runs = []

    def launch(st):
        runs.append(_loss_launch(hip, kind, z, t, kw, st[0]))
        return [runs[-1]["loss"]]

    (loss,) = _accumulates(launch, [torch.tensor([0.75])], ("loss_out",))
    for r in runs[1:]:
        assert torch.equal(r["dl"], runs[0]["dl"])
        assert kind != "focal" or torch.equal(r["per"], runs[0]["per"])
    bare = _loss_launch(hip, kind, z, t, kw, torch.zeros(1), dl=False, per=False)
    assert torch.equal(bare["loss"], loss), "the loss depends on the optional outputs"
    return dict(loss=loss, dl=runs[0]["dl"], per=runs[0]["per"])


def _tag(kind, kw):
    return kind + "".join(f" {k}{v:.3g}" for k, v in kw.items() if k != "cw") + (" cw" if "cw" in kw else "")


@pytest.mark.parametrize("B,C", R.LOSS_SHAPES)
def test_losses_at_small_class_counts_and_across_the_thread_stride(B, C):
    hip = _hip()
    z, t = R.loss_inputs("order1", B, C)
    for kind, kw in _loss_calls(B, C):
        want, e32 = R.loss_case(kind, z, t, **kw)
        got = _loss_run(hip, kind, z, t, kw)
        chk = _Chk(kind, f"B{B} C{C} {_tag(kind, kw)}")
        if C == 1 and not (kind == "smoothed" and kw["s"] > 0):
            for k in want:                                                     # one class: ce = 0 and softmax - onehot = 0
                assert bool((got[k] == 0).all()), (kind, kw, k)
        elif C == 1:                                                           # p - (1 - s) - s: the rounding of 1 - s
            assert abs(got["loss"].item()) <= 2.0 ** -24 and got["dl"].abs().max().item() <= 2.0 ** -24 / B
            assert torch.all(want["loss"] == 0) and want["dl"].abs().max().item() < 1e-15
        else:
            for k in want:
                chk.vs(k, got[k], want[k], e32, " shapes")
        chk.done()


@pytest.mark.parametrize("B,C", R.FAMILY_SHAPES)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_losses_subtract_the_maximum_and_hold_on_confident_batches(family, B, C):
    hip = _hip()
    z, t = R.loss_inputs(family, B, C)
    rows = []
    for kind, kw in _loss_calls(B, C):
        want, e32 = R.loss_case(kind, z, t, **kw)
        got = _loss_run(hip, kind, z, t, kw)
        chk = _Chk(kind, f"{family} B{B} C{C} {_tag(kind, kw)}")
        for k in want:
            chk.vs(k, got[k], want[k], e32, f" {family}")
        rows += chk.rows
    bad = [r for r in rows if not r[1] <= r[2]]
    assert not bad, f"{family} B{B} C{C}: " + ", ".join(f"{n} {e:.3e} > {b:.3e}" for n, e, b in bad)


def test_a_class_weight_of_zero_silences_its_rows():
    hip = _hip()
    B, C = 257, 5
    z, t = R.loss_inputs("order1", B, C)
    cw = torch.tensor([0.7, 1.3, 0.0, 0.4, 2.0])
    assert 0 < int((t == 2).sum()) < B
    want, e32 = R.loss_case("weighted", z, t, cw=cw)
    got = _loss_run(hip, "weighted", z, t, dict(cw=cw))
    chk = _Chk("weighted", "zero class weight")
    for k in want:
        chk.vs(k, got[k], want[k], e32, " zero weight")
    assert bool((got["dl"][_cu(t == 2)] == 0).all()) and bool((want["dl"][t == 2] == 0).all())
    chk.done()


def test_a_label_outside_the_classes_drops_its_row():
    """labels -100, C and 2^32 + 1 (class 1 after a cast to int): the kernels compare the 64-bit label with [0, C) and
    index nothing with it.  Weighted CE: the row leaves both sums (ignore_index); focal: per_sample 0, nothing added;
    smoothed CE: nothing added, the divisor stays B; the gradient row is 0 in all three"""
    hip = _hip()
    B, C = 257, 5
    z, t = R.loss_inputs("order1", B, C)
    tb = t.clone()
    for b, lab in R.BAD_LABELS.items():
        tb[b] = lab
    bad = list(R.BAD_LABELS)
    okrow = torch.ones(B, dtype=torch.bool)
    okrow[bad] = False
    assert not R.valid_rows(tb, C)[bad].any() and int((tb[256] & 0xFFFFFFFF)) == 1
    for kind, kw in _loss_calls(B, C):
        want, e32 = R.loss_case(kind, z, tb, **kw)
        got = _loss_run(hip, kind, z, tb, kw)
        chk = _Chk(kind, f"labels {_tag(kind, kw)}")
        for k in want:
            chk.vs(k, got[k], want[k], e32, " labels")
        assert bool((got["dl"].cpu()[bad] == 0).all())
        if kind == "focal":
            assert bool((got["per"].cpu()[bad] == 0).all())
        if kind != "weighted":                       # the other rows do not know: same bits as with three valid labels
            ref = _loss_launch(hip, kind, z, t, kw, torch.zeros(1))
            assert torch.equal(got["dl"].cpu()[okrow], ref["dl"].cpu()[okrow])
            if kind == "focal":
                assert torch.equal(got["per"].cpu()[okrow], ref["per"].cpu()[okrow])
        chk.done()
