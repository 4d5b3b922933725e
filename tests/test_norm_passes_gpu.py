"""GPU: the streaming passes between the GEMMs - mm_bn_finalize, mm_bn_act_fwd / _bwd_reduce / _bwd_apply and
mm_layernorm_fwd / _bwd (csrc/elementwise.hip), mm_pool3d_bn_act_fwd / _bwd_reduce / _bwd_apply (csrc/conv3d.hip) and the
element routine bn_dz_pair (csrc/common.h) - against plain fp64 torch on the CPU, computed from the kernels' own operands
(bf16-at-rest inputs rounded first, gradients by fp64 autograd), on every branch the host code can launch: all five
activations, pool 1 / 2 with the dropout before or after the pool, the positional add and second dropout, both d(out) and
dy types, frozen statistics, every LayerNorm width and rows-per-wave path, and grids past every cap (so that the
grid-stride and software-pipelined loops take a second and third trip).

Dropout masks are oracle.dropout_replica.keep_scale at p = 0.25 / 0.5 (exact binary fractions); the mask index is the flat
channels-last index of the tensor the mask multiplies (_bn1d_ref, _ln_ref, _p3_ref say which).  Order of operations:
act -> (dropout if drop_first) -> pool -> (dropout otherwise) -> + pe[so] -> dropout 2.  A pool's winner is the FIRST maximum
in window order; arg = 4 (d & 1) + 2 (h & 1) + (w & 1); ysel is the winner's pre-BatchNorm bf16 value.

Exclusions (conditions on the fp64 reference, never on the kernels' output): pooled outputs whose winner and any other
activation of the window differ by less than 1e-5 (1 + |top|) without being equal (exact ties stay and must go to the first;
the 1-D pool-2 inputs and a quarter of the 3-D channels hold such ties on purpose), and, under ReLU, elements with
|z| < 1e-5.  The values compared are the ones the pool compares (after the mask when the dropout comes first).  A channel
sum, and the train-mode dy formed from it, cannot leave an element out, so every train-mode case is run on inputs whose fp64
reference has NOTHING excluded: the few offending y of the seeded draw are moved until that holds (_bn1d_inputs,
_p3_inputs), the test asserts it, and all of its bounds are the plain ones below.  Only the frozen-statistics cases, whose
checks are elementwise, leave elements out (asserted to be at most 0.1 %).

Bounds.  None is taken from the kernels' output.
  fp32 outputs, sums, statistics: rel-L2 against fp64 at most 16 x e32, e32 = the rel-L2 error of the same formula in plain
    fp32 torch on the CPU on the same inputs, computed by the test itself (16: __expf, rsqrtf, the polynomial erf and other
    summation orders against torch's libm).
  bf16 outputs: against the bf16 rounding of the fp64 reference every element within one bf16 ulp and at most 1 % different
    at all; rel-L2 against the unrounded reference at most 2^-9 + 16 e32 - or, on a tensor of a few dozen elements whose
    fp64 reference, rounded to bf16 exactly, is itself further than 2^-9 from the unrounded one (2^-9 is the typical cost
    of that rounding, 2^-8 its worst case), that distance + 16 e32.  The ulp of an element is taken at no
    less than 2^12 x the largest absolute error of the fp32 CPU evaluation of that tensor (about 2^-11 of its peak):
    dy = sc (dz - c0 - xhat c1) and z = y sc + sh cancel, their fp32 error is a few 2^-24 of the terms, not of the result,
    and cannot stay below the ulp of a result arbitrarily close to zero; at that size one ulp is 16 x the CPU's error.
  finalize envelope: |var - var64| / var64 <= c 2^-24 (1 + mean^2 / var), c = 16 x what the fp32 CPU evaluation of the same
    one-pass formula needs on the same inputs.
  exact: zeros of a mask, arg, ysel, frozen tails, loop-versus-split launches, two runs of one launch, the doubled dgb.

Figures: rel-L2 unless named.  e32 is what the tests compute on the CPU (range over the cases), the bound is 16 e32 of the
same case, and the MI355X column is the worst figure measured with, in brackets, the largest fraction of its own bound
that any case used.
    quantity                                  e32                bound               MI355X
    finalize scale                            4.0e-8             6.4e-7              1.5e-7 (0.25)
    finalize shift                            4.8e-8 .. 2.1e-7   7.7e-7 .. 3.4e-6    2.0e-7 (0.18)
    finalize mean                             2.4e-8 .. 4.1e-8   3.8e-7 .. 6.6e-7    4.1e-8 (0.06)
    finalize rstd                             2.9e-8 .. 4.8e-8   4.6e-7 .. 7.7e-7    1.2e-7 (0.15)
    finalize running mean                     2.4e-8 .. 4.9e-8   3.8e-7 .. 7.8e-7    4.9e-8 (0.06)
    finalize running variance                 3.3e-8 .. 7.6e-8   5.3e-7 .. 1.2e-6    7.6e-8 (0.08)
    eval finalize scale, shift                2.6e-8 .. 8.2e-8   4.2e-7 .. 1.3e-6    4.1e-8 (0.07)
    eval finalize rstd                        7.7e-10 .. 9.3e-10 1.2e-8 .. 1.5e-8    7.5e-10 (0.08); mean: exact
    finalize envelope constant c              2.7                43                  2.9 (0.07)
    bn_act out_f32                            4.2e-8 .. 1.6e-7   6.7e-7 .. 2.6e-6    1.2e-7 (0.11)
    bn_act dbeta                              2.5e-8 .. 1.6e-7   4.0e-7 .. 2.6e-6    1.7e-7 (0.17)
    bn_act dgamma                             8.4e-8 .. 2.1e-7   1.3e-6 .. 3.4e-6    2.3e-7 (0.23)
    bn_act dy_f32                             6.7e-8 .. 2.0e-7   1.1e-6 .. 3.2e-6    1.5e-7 (0.12)
    bn_act frozen out_f32, dy_f32             4.7e-8 .. 8.2e-8   7.5e-7 .. 1.3e-6    1.1e-7 (0.11)
    layernorm out_f32                         4.0e-8 .. 6.0e-8   6.4e-7 .. 9.6e-7    5.4e-8 (0.06)
    layernorm out_f32, rows of std 1e-3       7.8e-7 .. 1.7e-5   1.2e-5 .. 2.7e-4    1.2e-5 (0.09)
    layernorm mean                            3.9e-8 .. 7.7e-8   6.2e-7 .. 1.2e-6    7.6e-8 (0.08)
    layernorm rstd (rows of std 1e-3)         3.7e-8 .. 5.7e-8 (1.8e-8 .. 5.3e-8)    5.3e-8 (0.07), 4.8e-8 (0.08)
    layernorm dx                              3.9e-8 .. 7.6e-8   6.2e-7 .. 1.2e-6    7.6e-8 (0.08)
    layernorm dx, rows of std 1e-3            5.5e-8 .. 7.6e-7   8.8e-7 .. 1.2e-5    7.5e-7 (0.23)
    layernorm dgamma                          3.2e-7 .. 6.9e-6   5.1e-6 .. 1.1e-4    5.1e-6 (0.10)
    layernorm dbeta                           0 .. 1.4e-7        0 .. 2.2e-6         7.2e-8 (0.07)
    pool3d dbeta                              0 .. 1.7e-7        0 .. 2.7e-6         1.7e-7 (0.13)
    pool3d dgamma                             6.6e-8 .. 2.1e-7   1.1e-6 .. 3.4e-6    2.2e-7 (0.10)
    bf16 outputs                              more than 1 ulp off (bound 0) | differing at all (bound 1 %) | rel-L2 (bound
                                              2^-9 = 1.95e-3 + 16 e32, e32 as the fp32 row of the same quantity)
      bn_act out_bf16                         0 | 0.05 % | 1.6e-3 .. 2.1e-3 (0.96 of the bound; the 24-element tensors of
      bn_act dy_bf16                          0 | 0.04 % | 1.6e-3 .. 2.3e-3  (2, 6, 4) against their own rounding distance)
      layernorm out_bf16                      0 | 0.16 % | 1.7e-3 (0.84); the ulp count also per row group (std 1e-3 / others)
      layernorm dx_bf16 (p 0 and 0.25)        0 | 0.08 % | 1.9e-3 (0.94); likewise
      pool3d out                              0 | 0.12 % | 1.9e-3 (0.96)
      pool3d dy                               0 | 0.07 % | 2.0e-3 (0.99)
    excluded elements (frozen cases only)     at most 7.9e-5 of a test's elements (bound 1e-3); train-mode cases: none
Every figure is printed as "ERR <case> <quantity> <measured> (bound <bound>)" before anything is asserted.

test_reference_separates_wrong_kernels (CPU) evaluates the references with ten plausible kernel mistakes and asserts that
each lands more than 10 bounds from the right answer (for exact quantities: on more than 10 elements), and that the fp32
CPU evaluation rounded to bf16 stays inside the bf16 bounds.

Kernel defect these tests exposed, fixed with them: under ReLU pool3_bn_act_kernel (csrc/conv3d.hip) chose a window's
winner by the largest PRE-activation, so a window whose voxels are all <= 0 after BatchNorm - every activation 0, an exact
tie - recorded the voxel of the largest z in `arg` / `ysel` instead of the first one (10 .. 36 windows per case here).  The
scan now compares max(z, 0) under ReLU.  out and dy were and are the same (ReLU' is 0 at every voxel of such a window)."""
import math

import pytest
import torch

from oracle.dropout_replica import keep_scale
from multimodal_eeg_fmri_amd.ops import ACC_GRAD, ACC_STAT, ACT, acc_decode, acc_encode
from test_kernels_gpu import _grad, _hip
from test_head_kernels_gpu import _Errs, _rel

gpu = pytest.mark.gpu
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
EPS = 1e-5
ACTS = ["none", "gelu", "relu", "tanh", "sigmoid"]
U24 = 2.0 ** -24


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bf(x):
    return x.to(BF).to(x.dtype)


def _act(z, act, wrong=None):
    if act == "gelu":
        if wrong == "gelu_tanh":
            return 0.5 * z * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))
        return z * 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))
    return {"none": lambda t: t, "relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}[act](z)


def _mask(seed, shape, p, T):
    return keep_scale(seed, math.prod(shape), p).view(shape).to(T)


def _bf16_stats(got, want64, want32, keep=None):
    """bf16 output against the fp64 reference: (elements more than one ulp from bf16(want), fraction that differs at all,
    rel-L2 against the unrounded reference).  The ulp of an element is taken at no less than 2^12 x the largest absolute
    error of the fp32 CPU evaluation `want32` (module docstring): there one ulp is at least 16 x that error."""
    g, w = got.double(), want64.to(BF).double()
    d32 = (want32.double() - want64).abs()
    floor = 2.0 ** 12 * float((d32[keep] if keep is not None else d32).max())
    tol = 2.0 ** (torch.floor(torch.log2(w.abs().clamp_min(max(floor, 1e-300)))) - 7)
    bad, diff = (g - w).abs() > tol, g != w
    if keep is not None:
        bad, diff, g, want64 = bad[keep], diff[keep], g[keep], want64[keep]
    return int(bad.sum()), float(diff.double().mean()), _rel(g, want64)


def _chk32(E, name, got, r64, r32, keep=None):
    """fp32 quantity: rel-L2 against fp64 within 16 e32"""
    got, r64, r32 = got.detach().double().cpu(), r64.detach().double(), r32.detach().double()
    if keep is not None:
        got, r64, r32 = got[keep], r64[keep], r32[keep]
    e32 = _rel(r32, r64)
    print(f"E32 {E.tag} {name} {e32:.3e}")
    E(name, _rel(got, r64), 16 * e32)


def _chkbf(E, name, got, r64, r32, keep=None, ulp_only=False):
    """ulp_only: a group of rows with an fp32 error of its own gets its own ulp floor; the fraction that differs and the
    rel-L2 are the whole tensor's"""
    got, r64, r32 = got.detach().cpu(), r64.detach().double(), r32.detach().double()
    bad, diff, rel = _bf16_stats(got, r64, r32, keep)
    e32 = _rel(r32[keep], r64[keep]) if keep is not None else _rel(r32, r64)
    print(f"E32 {E.tag} {name} {e32:.3e}")
    E(name + " >1ulp", bad, 0)
    if ulp_only:
        return
    E(name + " differ", diff, 0.01)
    r0 = _rel(r64.to(BF).double()[keep], r64[keep]) if keep is not None else _rel(r64.to(BF).double(), r64)
    E(name + " rel", rel, max(2.0 ** -9, r0) + 16 * e32)      # r0: what rounding the reference itself to bf16 costs


def _excluded_ok(E, ex):
    E("excluded", float(ex.double().mean()), 1e-3)


# ------------------------------------------------------------------------------------------------------------ finalize
def _fin_ref(T, s1, s2, gam, bet, rm, rv, count, mom, eps=EPS, wrong=None):
    """train-mode finalize from the sums (the kernel's operands): out4 = scale, shift, mean, rstd; running statistics with
    the unbiased variance (count > 1)"""
    s1, s2, gam, bet, rm, rv = (t.to(T) for t in (s1, s2, gam, bet, rm, rv))
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp_min(0)
    unb = var * count / (count - 1) if count > 1 else var
    rstd = torch.rsqrt((unb if wrong == "unbiased_norm" else var) + eps)
    sc = gam * rstd
    return (torch.stack([sc, bet - mean * sc, mean, rstd]), (1 - mom) * rm + mom * mean,
            (1 - mom) * rv + mom * (var if wrong == "biased_running" else unb))


def _fin_eval_ref(T, gam, bet, rm, rv, cb, eps=EPS):
    gam, bet, rm, rv = (t.to(T) for t in (gam, bet, rm, rv))
    rstd = torch.rsqrt(rv + eps)
    sc = gam * rstd
    return torch.stack([sc, bet + ((cb.to(T) if cb is not None else 0) - rm) * sc, rm, rstd])


def _fin_inputs(N, count, seed, ratios=None):
    """sums of `count` samples per channel as the accumulator workspace holds them (decoded: the exact operands).  Every
    third channel has standard deviation 1e-2 (eps = 1e-5 moves its rstd by 5 %); `ratios`: |mean| / std per channel."""
    g = _g(seed)
    x = torch.randn(count, N, generator=g, dtype=F64)
    if ratios is None:
        x = x * 1.5 + 0.3
        x[:, 2::3] = x[:, 2::3] * (1e-2 / 1.5) + 0.005 - 0.3 * (1e-2 / 1.5)
    else:
        x = x + ratios
    ws = acc_encode(torch.stack([x.sum(0), (x * x).sum(0)]), ACC_STAT)
    s = acc_decode(ws, ACC_STAT)
    gam, bet = 0.5 + torch.rand(N, generator=g), torch.randn(N, generator=g) * 0.2
    rm, rv = torch.randn(N, generator=g) * 0.3, 0.5 + torch.rand(N, generator=g)
    return ws, s[0], s[1], gam, bet, rm, rv


FIN_ROWS = ["scale", "shift", "mean", "rstd"]


@gpu
@pytest.mark.parametrize("mom", [0.1, 1.0])
@pytest.mark.parametrize("count", [6, 12600])
@pytest.mark.parametrize("N", [4, 132])
def test_bn_finalize_train_vs_fp64(N, count, mom):
    """mode 0: all four rows of out4, both running statistics (unbiased variance: 20 % at count 6) and
    num_batches_tracked; N = 132 is two workgroups, the second ragged"""
    hip, E = _hip(), _Errs(f"fin N{N} c{count} m{mom}")
    ws, s1, s2, gam, bet, rm, rv = _fin_inputs(N, count, 100 * N + count)
    r64, r32 = (_fin_ref(T, s1, s2, gam, bet, rm, rv, float(count), mom) for T in (F64, F32))
    rmg, rvg, nb = rm.cuda(), rv.cuda(), torch.full((), 41, dtype=torch.int64, device="cuda")
    out4 = torch.full((4, N), float("nan"), device="cuda")
    hip.call("mm_bn_finalize", ws.cuda(), gam.cuda(), bet.cuda(), rmg, rvg, None, out4, N, float(count), mom, EPS, 0, nb)
    assert nb.item() == 42
    for i, nm in enumerate(FIN_ROWS):
        _chk32(E, nm, out4[i], r64[0][i], r32[0][i])
    _chk32(E, "run_mean", rmg, r64[1], r32[1])
    _chk32(E, "run_var", rvg, r64[2], r32[2])
    E.done()


@gpu
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("N", [4, 132])
def test_bn_finalize_eval_vs_fp64(N, bias):
    """mode 1: the running statistics (and the convolution's bias) folded into scale / shift; nothing else is written"""
    hip, E = _hip(), _Errs(f"fin-eval N{N} b{int(bias)}")
    g = _g(N + bias)
    gam, bet = 0.5 + torch.rand(N, generator=g), torch.randn(N, generator=g) * 0.2
    rm, rv = torch.randn(N, generator=g) * 0.3, 0.5 + torch.rand(N, generator=g)
    rv[2::3] = 1e-4
    cb = torch.randn(N, generator=g) * 0.5 if bias else None
    r64, r32 = (_fin_eval_ref(T, gam, bet, rm, rv, cb) for T in (F64, F32))
    rmg, rvg, nb = rm.cuda(), rv.cuda(), torch.full((), 5, dtype=torch.int64, device="cuda")
    out4 = torch.full((4, N), float("nan"), device="cuda")
    hip.call("mm_bn_finalize", None, gam.cuda(), bet.cuda(), rmg, rvg, cb.cuda() if bias else None, out4, N, 1.0, 0.1, EPS, 1, nb)
    assert nb.item() == 5 and torch.equal(rmg.cpu(), rm) and torch.equal(rvg.cpu(), rv)
    for i, nm in enumerate(FIN_ROWS):
        _chk32(E, nm, out4[i], r64[i], r32[i])
    assert torch.equal(out4[2].cpu(), rm)
    E.done()


def _envelope_inputs():
    N, count = 64, 12600
    ratios = torch.tensor([1.0, -1.0, 10.0, -10.0], dtype=F64).repeat(N // 4)
    return (N, count, ratios) + _fin_inputs(N, count, 7, ratios)


def _envelope_c(rv_out, s1, s2, count):
    """the constant the envelope needs: the variance read back from the running variance at momentum 1"""
    mean = s1 / count
    var = s2 / count - mean * mean
    got = rv_out.double().cpu() * (count - 1) / count
    return float(((got - var).abs() / var / (U24 * (1 + mean * mean / var))).max())


@gpu
def test_bn_finalize_one_pass_variance_envelope():
    """the kernel forms E[x^2] - E[x]^2 in fp32: how far that can be trusted, at |mean| / std = 1 and 10"""
    hip, E = _hip(), _Errs("fin-envelope")
    N, count, _, ws, s1, s2, gam, bet, rm, rv = _envelope_inputs()
    c32 = _envelope_c(_fin_ref(F32, s1, s2, gam, bet, rm, rv, float(count), 1.0)[2], s1, s2, count)
    rmg, rvg = rm.cuda(), rv.cuda()
    out4 = torch.empty(4, N, device="cuda")
    hip.call("mm_bn_finalize", ws.cuda(), gam.cuda(), bet.cuda(), rmg, rvg, None, out4, N, float(count), 1.0, EPS, 0, None)
    print(f"E32 fin-envelope c {c32:.3e}")
    E("c", _envelope_c(rvg, s1, s2, count), 16 * c32)
    E.done()


# ------------------------------------------------------------------------------------- 1-D BatchNorm / act / pool passes
def _bn1d_ref(T, y, gam, bet, act, pool, drop_first, p, seed, pe=None, p2=0.0, seed2=0, frozen=None, douts=(), wrong=None):
    """y (R, S, N) -> BatchNorm (batch statistics, or frozen = (run_mean, run_var, conv_bias)) -> act -> pool -> dropouts
    -> + pe.  Mask indices: the input (R, S, N) for pool 1 and for pool 2 with drop_first; the pooled output otherwise;
    the output after the positional add for dropout 2."""
    y, gam, bet = (t.to(T).clone().requires_grad_(True) for t in (y, gam, bet))
    R, S, N = y.shape
    So = S // pool
    if frozen is None:
        mean = y.mean((0, 1))
        var = ((y - mean) ** 2).mean((0, 1))
    else:
        mean, var = frozen[0].to(T) - (frozen[2].to(T) if frozen[2] is not None else 0), frozen[1].to(T)
    rstd = torch.rsqrt(var + EPS)
    xh = (y - mean) * rstd
    z = xh * gam + bet
    a = _act(z, act, wrong)
    m1 = lambda shape: _mask(seed, shape, p, T)                                      # noqa: E731
    cmp = None
    if pool == 1:
        o = a * m1((R, S, N))
    else:
        if drop_first and p > 0:
            a = a * (m1((R, So, N)).repeat_interleave(2, dim=1) if wrong == "mask_pooled" else m1((R, S, N)))
        cmp = a.view(R, So, 2, N)
        v0, v1 = cmp[:, :, 0], cmp[:, :, 1]
        o = torch.where(v0 > v1 if wrong == "tie_second" else v0 >= v1, v0, v1)
        if not drop_first:
            o = o * m1((R, So, N))
    m2 = _mask(seed2, (R, So, N), p2, T)
    if pe is not None:
        o = o * m2 + pe.to(T) if wrong == "drop2_first" else (o + pe.to(T)) * m2
    else:
        o = o * m2
    grads = [torch.autograd.grad(o, (y, gam, bet), d.to(T), retain_graph=True) for d in douts]
    zero = None                                                                      # outputs a mask makes exactly zero
    if p2 > 0:
        zero = m2 == 0
    elif pe is None and p > 0:
        zero = m1((R, So, N)) == 0 if (pool == 1 or not drop_first) else (m1((R, S, N)).view(R, So, 2, N) == 0).all(2)
    return dict(out=o.detach(), z=z.detach(), cmp=None if cmp is None else cmp.detach(), grads=grads, zero=zero)


def _near(top, other):
    d = (top - other).abs()
    return (d > 0) & (d < 1e-5 * (1 + top.abs()))


def _bn1d_excl(r, act, pool):
    """pooled-shape mask of the outputs the issue's conditions leave out (from the fp64 reference)"""
    R, S, N = r["z"].shape
    ex = torch.zeros(R, S // pool, N, dtype=torch.bool)
    if pool == 2:
        ex |= _near(r["cmp"].max(2).values, r["cmp"].min(2).values)
    if act == "relu":
        ex |= (r["z"].abs() < 1e-5).view(R, S // pool, pool, N).any(2)
    return ex


SEED1, SEED2 = 1000, 77


def _bn1d_inputs(R, S, N, act, pool, drop_first, p, with_pe=False, p2=0.0):
    """Inputs of one train-mode case, conditioned on their own fp64 reference: a channel sum cannot leave an element out,
    so the few y whose reference falls under an exclusion (a near-tie, a ReLU input within 1e-5 of 0) are moved until no
    element of the case does (they get mid-range values).  Pool 2: a twelfth of the windows hold the same value twice (exact ties: to the first)."""
    g = _g(R * S + N + pool)
    y = torch.randn(R, S, N, generator=g) * 1.5 + 0.3
    gam, bet = 0.5 + torch.rand(N, generator=g), torch.randn(N, generator=g) * 0.2
    pe = torch.randn(S // pool, N, generator=g) if with_pe else None
    dout = torch.randn(R, S // pool, N, generator=g)
    doutb = _bf(torch.randn(R, S // pool, N, generator=g))
    w = y.view(R, S // pool, pool, N)
    if pool == 2:
        w[:, ::3, 1, 1::4] = w[:, ::3, 0, 1::4]
    for k in range(1, 9):
        ex = _bn1d_excl(_bn1d_ref(F64, y, gam, bet, act, pool, drop_first, p, SEED1 + N, pe, p2, SEED2), act, pool)
        if not ex.any():
            return y, gam, bet, pe, dout, doutb
        for j in range(pool):
            w[:, :, j][ex] = 1.3 - 1.9 * j + 0.13 * k        # mid-range values, apart from each other and from 0
    raise AssertionError("inputs did not settle")


def _frozen_stats(N, g):
    cb = torch.randn(N, generator=g) * 0.2
    return 0.3 + cb + torch.randn(N, generator=g) * 0.2, 2.25 * (0.75 + 0.5 * torch.rand(N, generator=g)), cb


def _bn1d_joint(tag, R, S, N, act, pool, drop_first, p, with_pe=False, p2=0.0, variants=False):
    """finalize -> forward (bf16 and fp32 outputs of one launch) -> reduce -> apply (bf16 and fp32 dy of one launch)"""
    hip, E = _hip(), _Errs(tag)
    y, gam, bet, pe, dout, doutb = _bn1d_inputs(R, S, N, act, pool, drop_first, p, with_pe, p2)
    seed, seed2, So, A = SEED1 + N, SEED2, S // pool, ACT[act]
    r64, r32 = (_bn1d_ref(T, y, gam, bet, act, pool, drop_first, p, seed, pe, p2, seed2, douts=(dout, doutb)) for T in (F64, F32))
    assert not _bn1d_excl(r64, act, pool).any()                    # nothing is left out of a train-mode case
    yg, yd = y.cuda(), y.double()
    stats = acc_encode(torch.stack([yd.sum((0, 1)), (yd * yd).sum((0, 1))]), ACC_STAT).cuda()
    out4 = torch.full((4, N), float("nan"), device="cuda")
    hip.call("mm_bn_finalize", stats, gam.cuda(), bet.cuda(), torch.zeros(N, device="cuda"), torch.ones(N, device="cuda"),
             None, out4, N, float(R * S), 0.1, EPS, 0, None)
    peg = pe.cuda() if with_pe else None
    of = torch.full((R, So, N), float("nan"), device="cuda")
    ob = of.to(BF)
    hip.call("mm_bn_act_fwd", yg, out4[0], out4[1], peg, ob, of, R, S, N, A, pool, drop_first, p, seed, p2, seed2, None)
    assert torch.equal(of.to(BF), ob)
    _chk32(E, "out_f32", of, r64["out"], r32["out"])
    _chkbf(E, "out_bf16", ob, r64["out"], r32["out"])
    if r64["zero"] is not None:
        E("masked != 0", int((of.cpu()[r64["zero"]] != 0).sum()), 0)
    for k, (name, d) in enumerate((("f32", dout), ("bf16", doutb))):
        if k == 1 and not variants:
            break
        dbf, df = (None, d.cuda()) if k == 0 else (d.to(BF).cuda(), None)
        (dy64, dg64, db64), (dy32, dg32, db32) = r64["grads"][k], r32["grads"][k]
        sums = torch.zeros(32, 2, N, device="cuda")
        hip.call("mm_bn_act_bwd_reduce", yg, out4, dbf, df, sums, R, S, N, A, pool, drop_first, p, seed, p2, seed2, None)
        _chk32(E, f"dbeta[{name}]", _grad(sums)[0], db64, db32)
        _chk32(E, f"dgamma[{name}]", _grad(sums)[1], dg64, dg32)
        for nrep in ((32, 1) if variants else (32,)):
            sin = sums if nrep == 32 else _grad(sums).contiguous()
            dyf = torch.full((R, S, N), float("nan"), device="cuda")
            dyb = dyf.to(BF)
            hip.call("mm_bn_act_bwd_apply", yg, out4, dbf, df, sin, dyb, dyf, R, S, N, A, pool, drop_first, p, seed, p2,
                     seed2, None, 1, nrep)
            assert torch.equal(dyf.to(BF), dyb)
            _chk32(E, f"dy_f32[{name},{nrep}]", dyf, dy64, dy32)
            _chkbf(E, f"dy_bf16[{name},{nrep}]", dyb, dy64, dy32)
    if variants:
        sums2 = torch.zeros(32, 2, N, device="cuda")                      # two runs of one launch
        hip.call("mm_bn_act_bwd_reduce", yg, out4, dbf, df, sums2, R, S, N, A, pool, drop_first, p, seed, p2, seed2, None)
        assert torch.equal(sums2.view(torch.int64), sums.view(torch.int64))
        # frozen statistics: out4 from the eval finalize (with a conv bias), dy = scale * dz.  Nothing is summed here, so
        # the elements the conditions exclude under THESE statistics are simply left out
        g = _g(5)
        # (running statistics near the batch's own, so that z keeps its spread: a wider one puts several percent of the
        #  GELU values below 1e-5 in magnitude, and each of those is a near-tie with a dropped neighbour's 0)
        rm, rv, cb = _frozen_stats(N, g)
        f64, f32 = (_bn1d_ref(T, y, gam, bet, act, pool, drop_first, p, seed, pe, p2, seed2, (rm, rv, cb), (dout,)) for T in (F64, F32))
        exf = _bn1d_excl(f64, act, pool)
        _excluded_ok(E, exf)
        out4e = torch.full((4, N), float("nan"), device="cuda")
        hip.call("mm_bn_finalize", None, gam.cuda(), bet.cuda(), rm.cuda(), rv.cuda(), cb.cuda(), out4e, N, 1.0, 0.1, EPS, 1, None)
        hip.call("mm_bn_act_fwd", yg, out4e[0], out4e[1], peg, None, of, R, S, N, A, pool, drop_first, p, seed, p2, seed2, None)
        _chk32(E, "eval out_f32", of, f64["out"], f32["out"], ~exf)
        dyf = torch.full((R, S, N), float("nan"), device="cuda")
        hip.call("mm_bn_act_bwd_apply", yg, out4e, None, dout.cuda(), None, None, dyf, R, S, N, A, pool, drop_first, p, seed,
                 p2, seed2, None, 0, 1)
        _chk32(E, "eval dy_f32", dyf, f64["grads"][0][0], f32["grads"][0][0], ~exf.repeat_interleave(pool, dim=1))
    E.done()


COMBOS = [(1, 1, 0.0), (1, 1, 0.25), (2, 1, 0.0), (2, 1, 0.25), (2, 0, 0.25)]


@gpu
@pytest.mark.parametrize("pool,drop_first,p", COMBOS)
@pytest.mark.parametrize("act", ACTS)
def test_bn_act_every_activation_and_dropout_order_vs_fp64(act, pool, drop_first, p):
    """the full cross at (3, 64, 48): the generic instantiations (none, relu, tanh, sigmoid) and bn_dz_pair's
    masked-then-pooled branch included"""
    _bn1d_joint(f"bn1d {act} {pool}{drop_first}{p}", 3, 64, 48, act, pool, drop_first, p)


@gpu
@pytest.mark.parametrize("R,S,N", [(2, 6, 4), (2, 18, 516), (2, 18, 1024), (3, 4200, 128)])
@pytest.mark.parametrize("pool,drop_first,p", [(2, 1, 0.25), (2, 0, 0.25), (1, 1, 0.25)])
@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_bn_act_thread_layouts_and_loop_trips_vs_fp64(act, pool, drop_first, p, R, S, N):
    """N / 4 = 1 (256 rows per workgroup), 129 (idle threads), 256 (one row per workgroup, the N limit), and 12 600 /
    6 300 rows against 768 x 8 per trip: workgroups take 1, 2 and 3 iterations of the prefetching loop"""
    _bn1d_joint(f"bn1d {act} {pool}{drop_first} {R}x{S}x{N}", R, S, N, act, pool, drop_first, p)


@gpu
@pytest.mark.parametrize("pool,drop_first", [(1, 1), (2, 0)])
def test_bn_act_positional_add_and_second_dropout_vs_fp64(pool, drop_first):
    _bn1d_joint(f"bn1d pe pool{pool}", 3, 64, 48, "gelu", pool, drop_first, 0.25, with_pe=True, p2=0.5)


@gpu
@pytest.mark.parametrize("R,S,N", [(3, 64, 48), (3, 4200, 128)])
@pytest.mark.parametrize("act,pool,drop_first", [("gelu", 2, 1), ("tanh", 1, 1)])
def test_bn_act_backward_variants_vs_fp64(act, pool, drop_first, R, S, N):
    """d(out) as bf16 and as fp32, dy and dy_f32 of one launch, the sums as workspace (32) and decoded (1), frozen
    statistics (train = 0) with out4 from the eval finalize; compiled-in and generic kernels"""
    _bn1d_joint(f"bn1d variants {act} {R}x{S}x{N}", R, S, N, act, pool, drop_first, 0.25, variants=True)


@gpu
def test_bn_act_forward_grid_stride_vs_fp64():
    """(9, 1000, 468): 1 053 000 vectors against 4096 x 256 - a partial second sweep, i / nv with nv = 117"""
    hip, E = _hip(), _Errs("bn1d fwd stride")
    R, S, N = 9, 1000, 468
    g = _g(468)
    y = torch.randn(R, S, N, generator=g) * 1.5 + 0.3
    gam, bet = 0.5 + torch.rand(N, generator=g), torch.randn(N, generator=g) * 0.2
    outs = []
    for T in (F64, F32):
        yt = y.to(T)
        mean = yt.mean((0, 1))
        outs.append(_act((yt - mean) * torch.rsqrt(((yt - mean) ** 2).mean((0, 1)) + EPS) * gam.to(T) + bet.to(T), "gelu"))
    yd = y.double()
    stats = acc_encode(torch.stack([yd.sum((0, 1)), (yd * yd).sum((0, 1))]), ACC_STAT).cuda()
    out4 = torch.empty(4, N, device="cuda")
    hip.call("mm_bn_finalize", stats, gam.cuda(), bet.cuda(), torch.zeros(N, device="cuda"), torch.ones(N, device="cuda"),
             None, out4, N, float(R * S), 0.1, EPS, 0, None)
    of = torch.full((R, S, N), float("nan"), device="cuda")
    hip.call("mm_bn_act_fwd", y.cuda(), out4[0], out4[1], None, None, of, R, S, N, ACT["gelu"], 1, 1, 0.0, 0, 0.0, 0, None)
    _chk32(E, "out_f32", of, outs[0], outs[1])
    E.done()


# ----------------------------------------------------------------------------------------------------------- LayerNorm
LN_WIDTHS = [32, 64, 96, 128, 160, 192, 224, 256, 288, 320, 352, 384, 416, 448, 480, 512, 1024]


def _ln_ref(T, x, gam, bet, eps, douts=(), wrong=None):
    x, gam, bet = (t.to(T).clone().requires_grad_(True) for t in (x, gam, bet))
    D = x.shape[1]
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).sum(1, keepdim=True) / (D - 1 if wrong == "ln_dm1" else D)
    rstd = torch.rsqrt(var + eps)
    out = (x - mean) * rstd * gam + bet
    grads = [torch.autograd.grad(out, (x, gam, bet), d.to(T), retain_graph=True) for d in douts]
    return dict(out=out.detach(), stat=torch.cat([mean, rstd], 1).detach(), grads=grads)


def _ln_inputs(M, D, seed):
    g = _g(seed)
    x = torch.randn(M, D, generator=g) * 2 + 0.5
    x[3::7] = (x[3::7] - 0.5) * 5e-4 + 0.5                         # rows with standard deviation 1e-3: eps decides their rstd
    gam, bet = 0.5 + torch.rand(D, generator=g), torch.randn(D, generator=g)
    dy, dyb = torch.randn(M, D, generator=g), _bf(torch.randn(M, D, generator=g))
    dres = torch.randn(M, D, generator=g)
    return x, gam, bet, dy, dyb, dres


def _ln_case(M, D, eps=EPS):
    hip, E = _hip(), _Errs(f"ln M{M} D{D} eps{eps:g}")
    x, gam, bet, dy, dyb, dres = _ln_inputs(M, D, M + D)
    r64, r32 = (_ln_ref(T, x, gam, bet, eps, (dy, dyb)) for T in (F64, F32))
    xg, gg = x.cuda(), gam.cuda()
    of = torch.full((M, D), float("nan"), device="cuda")
    ob, stat = of.to(BF), torch.full((M, 2), float("nan"), device="cuda")
    hip.call("mm_layernorm_fwd", xg, gg, bet.cuda(), ob, of, stat, M, D, eps)
    assert torch.equal(of.to(BF), ob)
    small = torch.zeros(M, dtype=torch.bool)
    small[3::7] = True                                 # x - mean cancels on these rows: their e32 is 50 times the others'
    for nm, rows in (("", ~small), ("[std 1e-3]", small)):
        _chk32(E, "out_f32" + nm, of, r64["out"], r32["out"], rows)
        _chk32(E, "rstd" + nm, stat[:, 1], r64["stat"][:, 1], r32["stat"][:, 1], rows)
        _chkbf(E, "out_bf16" + nm, ob, r64["out"], r32["out"], rows, ulp_only=True)
    _chkbf(E, "out_bf16", ob, r64["out"], r32["out"])
    _chk32(E, "mean", stat[:, 0], r64["stat"][:, 0], r32["stat"][:, 0])
    # (a) fp32 dy, residual gradient, dx and dx_bf16 (p = 0.25) of one launch; launched twice into one dgb
    seed, p = 4242 + D, 0.25
    mask = _mask(seed, (M, D), p, F64)
    (dx64, dg64, db64), (dx32, dg32, db32) = r64["grads"][0], r32["grads"][0]
    dgb = torch.zeros(32, 2, D, device="cuda")
    res = []
    for _ in range(2):
        dx = torch.full((M, D), float("nan"), device="cuda")
        dxb = dx.to(BF)
        hip.call("mm_layernorm_bwd", None, dy.cuda(), xg, stat, gg, dres.cuda(), dx, dxb, dgb, M, D, p, seed, None)
        res.append((dx, dxb, acc_decode(dgb, ACC_GRAD).cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])      # two runs of one launch
    assert torch.equal(res[1][2], 2 * res[0][2])                                        # the workspace accumulates
    for nm, rows in (("", ~small), ("[std 1e-3]", small)):
        _chk32(E, "dx" + nm, res[0][0], dx64 + dres.double(), dx32 + dres, rows)
        _chkbf(E, "dx_bf16 p.25" + nm, res[0][1], (dx64 + dres.double()) * mask, (dx32 + dres).double() * mask, rows, ulp_only=True)
    _chkbf(E, "dx_bf16 p.25", res[0][1], (dx64 + dres.double()) * mask, (dx32 + dres).double() * mask)
    E("dx_bf16 masked != 0", int((res[0][1].cpu()[mask == 0] != 0).sum()), 0)
    _chk32(E, "dgamma", res[0][2][0], dg64, dg32)
    _chk32(E, "dbeta", res[0][2][1], db64, db32)
    # (b) bf16 dy, no residual gradient, no dropout
    (dx64, dg64, db64), (dx32, dg32, db32) = r64["grads"][1], r32["grads"][1]
    dgb2 = torch.zeros(32, 2, D, device="cuda")
    dx = torch.full((M, D), float("nan"), device="cuda")
    dxb = dx.to(BF)
    hip.call("mm_layernorm_bwd", dyb.to(BF).cuda(), None, xg, stat, gg, None, dx, dxb, dgb2, M, D, 0.0, 0, None)
    assert torch.equal(dx.to(BF), dxb)
    for nm, rows in (("", ~small), ("[std 1e-3]", small)):
        _chk32(E, "dx[bf16 dy]" + nm, dx, dx64, dx32, rows)
        _chkbf(E, "dx_bf16 p0" + nm, dxb, dx64, dx32, rows, ulp_only=True)
    _chkbf(E, "dx_bf16 p0", dxb, dx64, dx32)
    _chk32(E, "dgamma[bf16 dy]", _grad(dgb2)[0], dg64, dg32)
    _chk32(E, "dbeta[bf16 dy]", _grad(dgb2)[1], db64, db32)
    E.done()


@gpu
@pytest.mark.parametrize("D", LN_WIDTHS)
def test_layernorm_every_width_vs_fp64(D):
    """forward (fp32, bf16, stat) and backward at every width LN_DISPATCH knows, M = 37 (the last workgroup is ragged)"""
    _ln_case(37, D)


@gpu
def test_layernorm_eps_vs_fp64():
    _ln_case(37, 96, eps=1e-3)


@gpu
@pytest.mark.parametrize("M", [1027, 8197])
@pytest.mark.parametrize("D", [96, 128, 512, 1024])
def test_layernorm_rows_per_wave_paths_vs_fp64(D, M):
    """rows_per_wave 2 and 8 of the generic backward, rows_per_half 1 and 4 of the D = 128 one; the last workgroup
    breaks out of its row loop mid-wave"""
    _ln_case(M, D)


@gpu
@pytest.mark.parametrize("D", [48, 544])
def test_layernorm_refuses_unsupported_widths(D):
    hip = _hip()
    x, v = torch.zeros(4, D, device="cuda"), torch.ones(D, device="cuda")
    out, stat = torch.zeros(4, D, device="cuda"), torch.zeros(4, 2, device="cuda")
    with pytest.raises(hip.HipLibraryError):
        hip.call("mm_layernorm_fwd", x, v, v, None, out, stat, 4, D, EPS)
    with pytest.raises(hip.HipLibraryError):
        hip.call("mm_layernorm_bwd", None, x, x, stat, v, None, out, None, None, 4, D, 0.0, 0, None)
    assert not out.any()


# ----------------------------------------------------------------------------------------------------------- 3-D pool
def _win8(t, B, D, H, W, N):
    """(B, D, H, W, N) -> (B, D/2, H/2, W/2, N, 8) windows in order j = 4 d + 2 h + w (floors: tails are in no window)"""
    Do, Ho, Wo = D // 2, H // 2, W // 2
    return (t[:, :2 * Do, :2 * Ho, :2 * Wo].reshape(B, Do, 2, Ho, 2, Wo, 2, N).permute(0, 1, 3, 5, 7, 2, 4, 6)
            .reshape(B, Do, Ho, Wo, N, 8))


def _unwin(k, B, D, H, W, N, fill):
    """pooled-shape mask -> volume-shape mask (every voxel of the window; tails = fill)"""
    Do, Ho, Wo = D // 2, H // 2, W // 2
    out = torch.full((B, D, H, W, N), fill, dtype=k.dtype)
    out[:, :2 * Do, :2 * Ho, :2 * Wo] = (k[:, :, None, :, None, :, None, :].expand(B, Do, 2, Ho, 2, Wo, 2, N)
                                         .reshape(B, 2 * Do, 2 * Ho, 2 * Wo, N))
    return out


def _p3_ref(T, y, gam, bet, act, p, seed, frozen=None, dout=None, wrong=None):
    """bf16 volume y (B, D, H, W, N) -> BatchNorm3d (statistics over all voxels, tails included) -> act -> MaxPool3d(2)
    (first maximum in window order) -> dropout indexed on the pooled output"""
    y, gam, bet = (t.to(T).clone().requires_grad_(True) for t in (y, gam, bet))
    B, D, H, W, N = y.shape
    if frozen is None:
        flat = y.reshape(-1, N)
        mean = flat.mean(0)
        var = ((flat - mean) ** 2).mean(0)
    else:
        mean, var = frozen[0].to(T), frozen[1].to(T)
    rstd = torch.rsqrt(var + EPS)
    xh = (y - mean) * rstd
    z = xh * gam + bet
    a8 = _win8(_act(z, act), B, D, H, W, N)
    top = a8.detach().max(-1, keepdim=True).values
    j = torch.arange(8).expand(a8.shape)
    eq = a8.detach() == top
    arg = torch.where(eq, j, -1).max(-1).values if wrong == "tie_second" else torch.where(eq, j, 8).min(-1).values
    m = _mask(seed, arg.shape, p, T)
    out = a8.gather(-1, arg[..., None]).squeeze(-1) * m
    r = dict(out=out.detach(), arg=arg, a8=a8.detach(), z8=_win8(z.detach(), B, D, H, W, N), m=m,
             ysel=_win8(y.detach(), B, D, H, W, N).gather(-1, arg[..., None]).squeeze(-1))
    if dout is not None:
        dy, dg, db = torch.autograd.grad(out, (y, gam, bet), dout.to(T), allow_unused=frozen is not None)
        if wrong == "tail_zero":
            dy = dy * _unwin(torch.ones(arg.shape, dtype=T), B, D, H, W, N, 0.0)
        r.update(dy=dy, dg=dg, db=db)
    return r


def _p3_excl(r, act):
    ex = _near(r["a8"].max(-1, keepdim=True).values, r["a8"]).any(-1)
    if act == "relu":
        ex |= (r["z8"].abs() < 1e-5).any(-1)
    return ex


P3_SEED = 600


def _p3_inputs(B, D, H, W, N, act, p, train):
    """train: conditioned on the fp64 reference like _bn1d_inputs - the windows an exclusion applies to get eight new,
    well separated values until none is left (the sums and the train-mode dy cannot leave an element out)"""
    g = _g(D * H * W + N)
    y = torch.randn(B, D, H, W, N, generator=g) * 1.5 + 0.3
    y[..., 1::4] = (y[..., 1::4] * 4).round() / 4      # a coarse grid on a quarter of the channels: exact ties in the windows
    y = _bf(y)
    gam, bet = 0.5 + torch.rand(N, generator=g), torch.randn(N, generator=g) * 0.2
    bet[7::8] -= 1.0                                   # windows that are all negative after BN: GELU's falling branch can win
    rm, rv = 0.3 + torch.randn(N, generator=g) * 0.2, 1.5 + torch.rand(N, generator=g)
    dout = _bf(torch.randn(B, D // 2, H // 2, W // 2, N, generator=g))
    Do, Ho, Wo = D // 2, H // 2, W // 2
    for k in range(1, 9 if train else 1):
        ex = _p3_excl(_p3_ref(F64, y, gam, bet, act, p, P3_SEED + N), act)
        if not ex.any():
            break
        d8 = ex[..., None] * (torch.arange(8) - 3.5) * (k * 2.0 ** -4)
        y[:, :2 * Do, :2 * Ho, :2 * Wo] += (d8.reshape(B, Do, Ho, Wo, N, 2, 2, 2).permute(0, 1, 5, 2, 6, 3, 7, 4)
                                            .reshape(B, 2 * Do, 2 * Ho, 2 * Wo, N)).float()
        y = _bf(y)
    else:
        assert not train, "inputs did not settle"
    return y, gam, bet, rm, rv, dout


def _p3_case(B, D, H, W, N, act, p, train):
    hip, E = _hip(), _Errs(f"p3d {B}x{D}x{H}x{W}x{N} {act} p{p} t{train}")
    y, gam, bet, rm, rv, dout = _p3_inputs(B, D, H, W, N, act, p, train)
    seed, A, cnt = P3_SEED + N, ACT[act], B * D * H * W
    fr = None if train else (rm, rv)
    r64, r32 = (_p3_ref(T, y, gam, bet, act, p, seed, fr, dout) for T in (F64, F32))
    ex = _p3_excl(r64, act)                 # train: none (the sums cannot leave an element out); frozen: elementwise
    assert not (train and ex.any())
    _excluded_ok(E, ex)
    keep = ~ex
    yg = y.to(BF).cuda()
    out4 = torch.full((4, N), float("nan"), device="cuda")
    if train:
        flat = y.double().reshape(-1, N)
        stats = acc_encode(torch.stack([flat.sum(0), (flat * flat).sum(0)]), ACC_STAT).cuda()
        hip.call("mm_bn_finalize", stats, gam.cuda(), bet.cuda(), torch.zeros(N, device="cuda"), torch.ones(N, device="cuda"),
                 None, out4, N, float(cnt), 0.1, EPS, 0, None)
    else:
        hip.call("mm_bn_finalize", None, gam.cuda(), bet.cuda(), rm.cuda(), rv.cuda(), None, out4, N, 1.0, 0.1, EPS, 1, None)
    shp = r64["out"].shape
    ob = torch.full(shp, float("nan"), device="cuda").to(BF)
    ysel, arg = torch.full(shp, float("nan"), device="cuda").to(BF), torch.full(shp, 255, dtype=torch.uint8, device="cuda")
    hip.call("mm_pool3d_bn_act_fwd", yg, out4, ob, ysel, arg, B, D, H, W, N, A, p, seed, None)
    _chkbf(E, "out", ob, r64["out"], r32["out"], keep)
    E("masked != 0", int((ob.cpu()[r64["m"] == 0] != 0).sum()), 0)
    E("arg", int((arg.cpu().long() != r64["arg"])[keep].sum()), 0)
    E("ysel", int((ysel.cpu().double() != r64["ysel"])[keep].sum()), 0)
    ob2 = torch.empty_like(ob)                                          # eval form: no winners kept
    hip.call("mm_pool3d_bn_act_fwd", yg, out4, ob2, None, None, B, D, H, W, N, A, p, seed, None)
    assert torch.equal(ob2, ob)
    dg = dout.to(BF).cuda()
    dy = torch.full((B, D, H, W, N), float("nan"), device="cuda").to(BF)
    keep_dy = _unwin(keep, B, D, H, W, N, True)
    if train:
        sums = torch.zeros(32, 2, N, device="cuda")
        hip.call("mm_pool3d_bn_act_bwd_reduce", ysel, out4, dg, sums, B, D, H, W, N, A, p, seed, None)
        _chk32(E, "dbeta", _grad(sums)[0], r64["db"], r32["db"])
        _chk32(E, "dgamma", _grad(sums)[1], r64["dg"], r32["dg"])
        hip.call("mm_pool3d_bn_act_bwd_apply", yg, arg, out4, dg, sums, dy, B, D, H, W, N, A, p, seed, None, 1, 32)
        _chkbf(E, "dy", dy, r64["dy"], r32["dy"], keep_dy)
        dy1 = torch.full_like(dy, float("nan"))
        hip.call("mm_pool3d_bn_act_bwd_apply", yg, arg, out4, dg, _grad(sums).contiguous(), dy1, B, D, H, W, N, A, p, seed,
                 None, 1, 1)
        _chkbf(E, "dy[compact sums]", dy1, r64["dy"], r32["dy"], keep_dy)
    else:
        hip.call("mm_pool3d_bn_act_bwd_apply", yg, arg, out4, dg, None, dy, B, D, H, W, N, A, p, seed, None, 0, 1)
        _chkbf(E, "dy", dy, r64["dy"], r32["dy"], keep_dy)
        tails = ~_unwin(torch.ones(shp, dtype=torch.bool), B, D, H, W, N, False)
        E("frozen tails != 0", int((dy.cpu()[tails] != 0).sum()), 0)
    assert torch.isfinite(dy.float()).all()                            # every element of dy is written, the tails included
    E.done()


@gpu
@pytest.mark.parametrize("train", [1, 0])
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("B,D,H,W,N", [(2, 4, 6, 4, 8), (2, 5, 7, 6, 24)])
def test_pool3d_every_activation_vs_fp64(B, D, H, W, N, act, p, train):
    """N / 8 = 1, and N / 8 = 3 (does not divide 256) with two odd extents: out, ysel, arg, the sums and every element of
    dy, the tails included (dy is NaN before the launch)"""
    _p3_case(B, D, H, W, N, act, p, train)


@gpu
@pytest.mark.parametrize("B,D,H,W,N", [(1, 2, 2, 4, 1024), (3, 36, 36, 36, 64)])
def test_pool3d_widest_rows_and_reduce_grid_cap_vs_fp64(B, D, H, W, N):
    """N = 1024 (two pooled voxels per workgroup), and 17 496 pooled voxels against the reduce pass's 512 x 32"""
    _p3_case(B, D, H, W, N, "gelu", 0.25, 1)


@gpu
def test_pool3d_looping_launch_equals_launches_that_do_not_loop():
    """(2, 28, 30, 40, 1024): 8 400 pooled voxels against the forward / apply cap of 4096 x 2 per trip.  The whole batch
    must equal its two single-sample launches bit for bit; train = 1 with the compact sums halved for the half launches
    (inv_count doubles: c0 / c1 keep their bits)."""
    hip = _hip()
    B, D, H, W, N = 2, 28, 30, 40, 1024
    g = torch.Generator(device="cuda").manual_seed(3)
    y = (torch.randn(B, D, H, W, N, generator=g, device="cuda") * 1.5 + 0.3).to(BF)
    out4 = torch.stack([0.5 + torch.rand(N, generator=g, device="cuda"), torch.randn(N, generator=g, device="cuda") * 0.2,
                        torch.full((N,), 0.3, device="cuda"), torch.full((N,), 0.66, device="cuda")]).contiguous()
    shp = (B, D // 2, H // 2, W // 2, N)
    mk = lambda s, dt=BF: torch.zeros(s, dtype=dt, device="cuda")                    # noqa: E731
    ob, ys, ar = mk(shp), mk(shp), mk(shp, torch.uint8)
    hip.call("mm_pool3d_bn_act_fwd", y, out4, ob, ys, ar, B, D, H, W, N, 1, 0.0, 0, None)
    for b in range(B):
        o1, y1, a1 = mk(shp[1:]), mk(shp[1:]), mk(shp[1:], torch.uint8)
        hip.call("mm_pool3d_bn_act_fwd", y[b], out4, o1, y1, a1, 1, D, H, W, N, 1, 0.0, 0, None)
        assert torch.equal(o1, ob[b]) and torch.equal(y1, ys[b]) and torch.equal(a1, ar[b])
    dout = torch.randn(shp, generator=g, device="cuda").to(BF)
    sums = torch.randn(2 * N, generator=g, device="cuda") * 50
    for train in (0, 1):
        dy = torch.full((B, D, H, W, N), float("nan"), device="cuda").to(BF)
        hip.call("mm_pool3d_bn_act_bwd_apply", y, ar, out4, dout, sums, dy, B, D, H, W, N, 1, 0.0, 0, None, train, 1)
        assert torch.isfinite(dy.float()).all()
        for b in range(B):
            d1 = torch.full((D, H, W, N), float("nan"), device="cuda").to(BF)
            hip.call("mm_pool3d_bn_act_bwd_apply", y[b], ar[b], out4, dout[b], (sums * 0.5).contiguous(), d1, 1, D, H, W, N, 1,
                     0.0, 0, None, train, 1)
            assert torch.equal(d1, dy[b])


# ------------------------------------------------------------------------------------------------ the CPU self-check
def test_reference_separates_wrong_kernels():
    """Each reference, evaluated with one plausible kernel mistake, lands more than 10 bounds (16 e32; for exact
    quantities: more than 10 elements) from the right one on the tests' own inputs - so the GPU tests would fail on a
    kernel with that fault; and the fp32 CPU evaluation rounded to bf16 stays far inside the bf16 bounds."""
    def far(name, wrong, r64, r32, keep=None):
        if keep is not None:
            wrong, r64, r32 = wrong[keep], r64[keep], r32[keep]
        d, b = _rel(wrong, r64), 16 * _rel(r32, r64)
        print(f"SEP {name}: wrong {d:.3e} vs bound {b:.3e}")
        assert d > 10 * b, (name, d, b)

    # finalize (count 6): eps, unbiased variance in the normalisation, biased running variance
    ws, s1, s2, gam, bet, rm, rv = _fin_inputs(132, 6, 100 * 132 + 6)
    f64, f32 = (_fin_ref(T, s1, s2, gam, bet, rm, rv, 6.0, 0.1) for T in (F64, F32))
    far("eps 1e-6", _fin_ref(F64, s1, s2, gam, bet, rm, rv, 6.0, 0.1, eps=1e-6)[0][3], f64[0][3], f32[0][3])
    far("unbiased var in rstd", _fin_ref(F64, s1, s2, gam, bet, rm, rv, 6.0, 0.1, wrong="unbiased_norm")[0][3], f64[0][3], f32[0][3])
    far("biased running var", _fin_ref(F64, s1, s2, gam, bet, rm, rv, 6.0, 0.1, wrong="biased_running")[2], f64[2], f32[2])
    # 1-D passes at (3, 64, 48)
    R, S, N = 3, 64, 48
    for name, wrong, act, pool, df, wpe, p2 in (("mask on pooled index", "mask_pooled", "gelu", 2, 1, False, 0.0),
                                                ("dropout 2 before pe", "drop2_first", "gelu", 2, 0, True, 0.5),
                                                ("ties to the second (1-D)", "tie_second", "gelu", 2, 1, False, 0.0),
                                                ("tanh GELU", "gelu_tanh", "gelu", 1, 1, False, 0.0)):
        y, gam, bet, pe, dout, doutb = _bn1d_inputs(R, S, N, act, pool, df, 0.25, wpe, p2)
        a = (y, gam, bet, act, pool, df, 0.25, SEED1 + N, pe, p2, SEED2)
        r64, r32, rw = _bn1d_ref(F64, *a, douts=(dout,)), _bn1d_ref(F32, *a, douts=(dout,)), _bn1d_ref(F64, *a, douts=(dout,), wrong=wrong)
        assert not _bn1d_excl(r64, act, pool).any()
        if wrong != "tie_second":                       # (the tied values are equal: only the gradient's place tells)
            far(name + " out", rw["out"], r64["out"], r32["out"])
        if wrong != "drop2_first":                      # (an added constant: the gradient cannot tell)
            far(name + " dy", rw["grads"][0][0], r64["grads"][0][0], r32["grads"][0][0])
        for k64, k32 in ((r64["out"], r32["out"]), (r64["grads"][0][0], r32["grads"][0][0])):
            bad, diff, rel = _bf16_stats(k32.to(BF), k64, k32)
            assert bad == 0 and diff < 2.5e-3 and rel < 2.0 ** -9, (bad, diff, rel)
    # LayerNorm dividing by D - 1
    x, gam, bet, dy, dyb, dres = _ln_inputs(37, 128, 37 + 128)
    l64, l32, lw = _ln_ref(F64, x, gam, bet, EPS, (dy,)), _ln_ref(F32, x, gam, bet, EPS, (dy,)), _ln_ref(F64, x, gam, bet, EPS, (dy,), "ln_dm1")
    far("LayerNorm eps 1e-6 rstd", _ln_ref(F64, x, gam, bet, 1e-6)["stat"][3::7, 1], l64["stat"][3::7, 1], l32["stat"][3::7, 1])
    far("LayerNorm / (D - 1) out", lw["out"], l64["out"], l32["out"])
    far("LayerNorm / (D - 1) rstd", lw["stat"][:, 1], l64["stat"][:, 1], l32["stat"][:, 1])
    far("LayerNorm / (D - 1) dx", lw["grads"][0][0], l64["grads"][0][0], l32["grads"][0][0])
    bad, diff, rel = _bf16_stats(l32["out"].to(BF), l64["out"], l32["out"])
    assert bad == 0 and diff < 2.5e-3 and rel < 2.0 ** -9, (bad, diff, rel)
    # 3-D pool on the odd volume: ties to the later element, a tail voxel without its train-mode gradient
    B, D, H, W, N = 2, 5, 7, 6, 24
    y, gam, bet, rm, rv, dout = _p3_inputs(B, D, H, W, N, "gelu", 0.25, 1)
    p64, p32 = (_p3_ref(T, y, gam, bet, "gelu", 0.25, P3_SEED + N, None, dout) for T in (F64, F32))
    keep = ~_p3_excl(p64, "gelu")
    assert keep.all()
    pw = _p3_ref(F64, y, gam, bet, "gelu", 0.25, P3_SEED + N, None, dout, wrong="tie_second")
    nties = int((pw["arg"] != p64["arg"])[keep].sum())
    print(f"SEP ties to the later element: {nties} of {keep.numel()} args differ")
    assert nties > 10
    pt = _p3_ref(F64, y, gam, bet, "gelu", 0.25, P3_SEED + N, None, dout, wrong="tail_zero")
    keep_dy = _unwin(keep, B, D, H, W, N, True)
    bad, diff, rel = _bf16_stats(pt["dy"].to(BF), p64["dy"], p32["dy"], keep_dy)
    print(f"SEP tail voxels without gradient: {bad} elements more than one bf16 ulp off")
    assert bad > 10
    for k in ("out", "dy"):
        bad, diff, rel = _bf16_stats(p32[k].to(BF), p64[k], p32[k], keep if k == "out" else keep_dy)
        assert bad == 0 and diff < 2.5e-3 and rel < 2.0 ** -9, (k, bad, diff, rel)
