"""GPU: the attention kernels (csrc/attention.hip, csrc/attention_readout.hip) at SHARP scores against fp64.

Every other attention test draws qkv = randn, scores of order 1 nat, and at such scores attn_fwd_kernel never rescales its
accumulators by a finite factor: the lazy running maximum fires on a row's first tile (alpha = 0) and never again
(test_attention_sharp_scores_host.py::test_randn_inputs_never_rescale).  The inputs here (oracle/attention_tiles.py:
score_profiles) are built so that it does, hundreds to thousands of times per case, in waves that also hold rows that need no
rescale, across 128-key chunk boundaries and in the partial last tile, with the unnormalised probability up to 2^8; the host
file asserts all of that on the fp64 scores of every case below.
    ramp     +-1 log2 unit per key, rising rows (rescale at every tile) and falling rows (never) in one wave, -208 .. 208 nats
    spike    randn, plus the last key at +40 nats and the first key of the second chunk at +15 nats for two rows in three
    sharp    randn q, k times sqrt(8): scores of std 8 nats, rows close to one-hot
    offset+- every score at +-100 nats: without the maximum subtraction inf / inf resp. 0 / 0
The reference is `_ref` of test_attention_head_dims_gpu.py (fp64 softmax attention and autograd on the bf16 operands, the
dropout keep mask from oracle/dropout_replica.py); outputs are pre-filled with NaN.

Unmasked: head dim 32 through mm_attn_fwd / mm_attn_bwd (the exact kernels), 24 and 64 through mm_attn_fwd_hd / _bwd_hd (the
runtime-dh kernels of padded width 32 and 64), L = 256 (the FULL kernels, two key chunks) and 300 (general, three chunks, a
12-key last tile), p = 0 and 0.25: the twelve forward instantiations the default path launches, and their backward kernels.
dh 16 and 40 at B = 2, H = 3 for the batch / head index.  Masked (L = 300): `sharp` under a causal mask, and under an
anti-causal mask written with -1e4, -1e9 and the most negative fp32 in place of -inf - the leading chunks of a late query then
leave a finite, hugely negative running maximum that a later tile must rescale away completely.  Read-out: mm_attn_weights
and mm_attn_received on `spike` and `sharp` with the lse of the matching forward, at the tolerances of
test_attention_readout_kernels_gpu.py.

Bounds.  None is taken from the kernels' output.
  out, dq, dk, dv: rel-L2 against fp64 at most 2^-9 + 3 e_emu.  e_emu is the rel-L2 error of oracle.attention_tiles.emulate - an
    fp64 attention on the same lazy tiled loop that rounds where the kernels round (fp32 p, bf16 P and dS, bf16 outputs, delta
    from the stored bf16 O) - on the same case, computed by the test on the CPU; 2^-9 is the worst relative cost of the final
    bf16 rounding; 3 covers what the emulation leaves out (fp32 sums in the kernels' order, the hardware exp2).
  lse: elementwise |lse - lse64| <= 4e-6 + 8 2^-24 |lse64| (the masked-attention bound at |lse| ~ 1, and eight fp32 roundings
    at the magnitude of the lse).
  exact: two runs of one launch; under dropout, out is more than 5 x further from the no-dropout reference than from the masked one.
dq and dk of `spike` under dropout have e_emu of 3e-2 .. 1.1e-1: a row whose spike key survives is one-hot, dP - delta cancels
there, and delta = sum dO o O carries the bf16 rounding of O = v / (1 - p) (without dropout O = v exactly).  That is the
delta-from-stored-output formulation, not a defect.

Figures: rel-L2 (lse: the largest |lse - lse64| as a fraction of its elementwise bound), range over the cases; the MI355X
column is the worst figure measured with, in brackets, the largest fraction of its own bound that any case used.
    quantity  cases                  e_emu               bound               MI355X
    out       ramp                   1.8e-3              7.3e-3 .. 7.5e-3    1.8e-3 (0.25)
    out       spike                  1.3e-4 .. 1.8e-3    2.4e-3 .. 7.3e-3    1.8e-3 (0.24)
    out       sharp                  1.7e-3 .. 1.9e-3    7.0e-3 .. 7.6e-3    1.9e-3 (0.25)
    out       sharp, masked          1.6e-3 .. 1.8e-3    6.8e-3 .. 7.3e-3    1.8e-3 (0.24)
    out       offset+, offset-       2.3e-3 .. 2.5e-3    8.7e-3 .. 9.3e-3    2.5e-3 (0.26)
    dq        ramp                   3.1e-3 .. 4.1e-3    1.1e-2 .. 1.4e-2    4.1e-3 (0.29)
    dq        spike, p = 0           2.4e-3 .. 2.5e-3    9.2e-3 .. 9.5e-3    2.5e-3 (0.26)
    dq        spike, p = 0.25        3.5e-2 .. 6.2e-2    1.1e-1 .. 1.9e-1    6.2e-2 (0.33)
    dq        sharp                  4.8e-3 .. 6.4e-3    1.6e-2 .. 2.1e-2    6.4e-3 (0.30)
    dq        sharp, masked          5.1e-3 .. 6.1e-3    1.7e-2 .. 2.0e-2    6.1e-3 (0.30)
    dq        offset+, offset-       2.5e-3 .. 2.8e-3    9.5e-3 .. 1.0e-2    2.8e-3 (0.27)
    dk        ramp                   1.8e-3 .. 4.3e-3    7.4e-3 .. 1.5e-2    4.4e-3 (0.29)
    dk        spike, p = 0           2.3e-3 .. 2.4e-3    9.0e-3 .. 9.1e-3    2.4e-3 (0.26)
    dk        spike, p = 0.25        5.7e-2 .. 1.9e-1    1.7e-1 .. 5.8e-1    1.9e-1 (0.33)
    dk        sharp                  4.5e-3 .. 5.5e-3    1.5e-2 .. 1.8e-2    5.5e-3 (0.30)
    dk        sharp, masked          4.8e-3 .. 5.5e-3    1.6e-2 .. 1.9e-2    5.5e-3 (0.30)
    dk        offset+, offset-       2.3e-3 .. 2.6e-3    8.7e-3 .. 9.7e-3    2.6e-3 (0.27)
    dv        ramp                   2.0e-3 .. 2.8e-3    8.0e-3 .. 1.0e-2    2.9e-3 (0.27)
    dv        spike                  1.4e-3 .. 2.1e-3    6.2e-3 .. 8.2e-3    2.1e-3 (0.25)
    dv        sharp                  2.1e-3 .. 2.2e-3    8.2e-3 .. 8.5e-3    2.2e-3 (0.26)
    dv        sharp, masked          2.0e-3 .. 2.2e-3    8.0e-3 .. 8.4e-3    2.2e-3 (0.26)
    dv        offset+, offset-       2.3e-3 .. 2.4e-3    8.9e-3 .. 9.1e-3    2.4e-3 (0.26)
    lse       ramp                   (the emulation's    8.8e-5 .. 1.0e-4    4.3e-5 (0.42)
    lse       spike                   lse is asserted    2.3e-5              1.1e-5 (0.48)
    lse       sharp                   to be inside the   1.4e-5 .. 2.0e-5    4.9e-6 (0.31)
    lse       sharp, masked           same bound; bound  1.2e-5 .. 1.8e-5    5.1e-6 (0.34)
    lse       offset+, offset-        = at the worst     4.8e-5 .. 5.5e-5    1.4e-5 (0.30)
                                      element)
    read-out  weights                largest error / (atol + rtol |w|) 2.8e-3 (bound 1); |row sum - 1| 4.0e-6 (bound 2e-3)
    read-out  received               largest error / (atol + rtol |r|) 5.8e-4 (bound 1)
The kernels' figures agree with e_emu to two or three digits in every case: the emulation rounds what the kernels round.
With `l_run *= alpha` taken out of attn_fwd_kernel (tried once, not kept) 74 of the 89 tests here fail - all but the twelve
offset cases, which never rescale, and the three two-runs tests - while of the older attention tests only 13 with a random or anti-causal
additive mask notice; every older unmasked test stays green.
Every figure is printed as "ERR attn-sharp <case> <quantity> <measured> (bound <bound>)" before anything is asserted."""
import functools
import math

import pytest
import torch

from oracle import attention_tiles as AT
from oracle.dropout_replica import attn_keep_scale
from test_attention_head_dims_gpu import SEED, _ref, _run
from test_attention_readout_kernels_gpu import R_TOL, W_TOL, _forward_lse, _probs, _received, _received_ref, _weights
from test_kernels_gpu import _hip

pytestmark = pytest.mark.gpu

FMIN = torch.finfo(torch.float32).min


def _entry(dh):
    return ("mm_attn_fwd", "mm_attn_bwd") if dh == 32 else ("mm_attn_fwd_hd", "mm_attn_bwd_hd")


def _mask(kind, L):
    q, k = torch.arange(L).view(L, 1), torch.arange(L).view(1, L)
    if kind is None:
        return None
    if kind == "causal":
        return torch.zeros(L, L).masked_fill(k > q, float("-inf"))
    return torch.zeros(L, L).masked_fill(k < q, kind)        # anti-causal, a finite negative in place of -inf


@functools.lru_cache(maxsize=None)
def _case(profile, B, L, H, dh, p, mask_kind=None):
    """operands, fp64 reference and the emulation's error of one case, computed once on the CPU and never modified"""
    qkv, dout = AT.case_inputs(profile, B, L, H, dh)
    mask = _mask(mask_kind, L)
    ref = _ref(qkv, dout, B, L, H, dh, mask, p)
    emu = AT.emulate(qkv, dout, H, dh, mask, attn_keep_scale(SEED, B * H, L, p) if p > 0 else None)
    E = H * dh
    e_emu = dict(out=AT.rel_l2(emu[0], ref[0]))
    for name, g, w in zip(("dq", "dk", "dv"), AT.split3(emu[2], E), AT.split3(ref[2], E)):
        e_emu[name] = AT.rel_l2(g, w)
    assert ((emu[1] - ref[1]).abs() <= AT.lse_bound(ref[1])).all()
    return qkv, dout, mask, ref, e_emu


def _check(profile, B, L, H, dh, p, mask_kind=None):
    hip = _hip()
    qkv, dout, mask, ref, e_emu = _case(profile, B, L, H, dh, p, mask_kind)
    fwd, bwd = _entry(dh)
    out, lse, dqkv = _run(hip, qkv, dout, B, L, H, dh, mask, p, fwd=fwd, bwd=bwd)
    E = H * dh
    tag = f"{profile} B{B} L{L} H{H} dh{dh} p{p}" + ("" if mask_kind is None else f" mask {mask_kind}")
    rows = [("out", AT.rel_l2(out, ref[0]), AT.tensor_bound(e_emu["out"]))]
    for name, g, w in zip(("dq", "dk", "dv"), AT.split3(dqkv, E), AT.split3(ref[2], E)):
        rows.append((name, AT.rel_l2(g, w), AT.tensor_bound(e_emu[name])))
    lb = AT.lse_bound(ref[1])
    frac = ((lse.double() - ref[1]).abs() / lb).flatten()
    i = int(torch.nan_to_num(frac, nan=math.inf).argmax())
    rows.append(("lse", (lse.double() - ref[1]).abs().flatten()[i].item(), lb.flatten()[i].item()))
    for name, err, bound in rows:
        print(f"ERR attn-sharp {tag} {name} {err:.3e} (bound {bound:.3e}) e_emu {e_emu.get(name, float('nan')):.3e}")
    assert torch.isfinite(out).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv).all(), tag
    bad = [r for r in rows if not r[1] <= r[2]]
    assert not bad, f"{tag}: " + ", ".join(f"{n} {e:.3e} > {b:.3e}" for n, e, b in bad)
    if p > 0 and mask_kind is None:                      # the replica of the keep mask is not vacuous
        o_nodrop = _case(profile, B, L, H, dh, 0.0)[3][0]
        assert AT.rel_l2(out, o_nodrop) > 5 * AT.rel_l2(out, ref[0])
    return out, lse, dqkv


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("L", [256, 300])
@pytest.mark.parametrize("dh", [32, 24, 64])
@pytest.mark.parametrize("profile", ["ramp", "spike", "sharp"])
def test_attention_rescales_vs_fp64(profile, dh, L, p):
    _check(profile, 1, L, 2, dh, p)


@pytest.mark.parametrize("L", [256, 300])
@pytest.mark.parametrize("dh", [32, 24, 64])
@pytest.mark.parametrize("profile", ["offset+", "offset-"])
def test_attention_subtracts_the_maximum(profile, dh, L):
    _check(profile, 1, L, 2, dh, 0.0)


@pytest.mark.parametrize("dh", [16, 40])
def test_attention_rescales_in_every_batch_and_head(dh):
    _check("sharp", 2, 300, 3, dh, 0.25)


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("dh", [32, 24, 64])
@pytest.mark.parametrize("mask_kind", ["causal", -1e4, -1e9, FMIN], ids=["causal", "anti-1e4", "anti-1e9", "anti-fmin"])
def test_masked_attention_rescales_vs_fp64(mask_kind, dh, p):
    _check("sharp", 1, 300, 2, dh, p, mask_kind)


@pytest.mark.parametrize("profile,L,dh,p,mask_kind", [("ramp", 300, 24, 0.25, None), ("spike", 256, 32, 0.0, None),
                                                      ("sharp", 300, 64, 0.25, -1e9)])
def test_two_runs_give_the_same_bits(profile, L, dh, p, mask_kind):
    hip = _hip()
    qkv, dout, mask, _, _ = _case(profile, 1, L, 2, dh, p, mask_kind)
    fwd, bwd = _entry(dh)
    a = _run(hip, qkv, dout, 1, L, 2, dh, mask, p, fwd=fwd, bwd=bwd)
    b = _run(hip, qkv, dout, 1, L, 2, dh, mask, p, fwd=fwd, bwd=bwd)
    for x, y in zip(a, b):
        assert torch.isfinite(x).all() and torch.equal(x, y)


@pytest.mark.parametrize("L", [256, 257])
@pytest.mark.parametrize("dh", [32, 24, 64])
@pytest.mark.parametrize("profile", ["spike", "sharp"])
def test_readout_at_sharp_scores_vs_fp64(profile, dh, L):
    hip = _hip()
    B, H = 1, 2
    qkv, _ = AT.case_inputs(profile, B, L, H, dh)
    P = _probs(qkv, B, L, H, dh)
    qg = qkv.cuda().to(torch.bfloat16)
    r = torch.rand(B, L, generator=torch.Generator().manual_seed(L + dh)) + 0.1
    c = dict(qkv=qg, lse=_forward_lse(hip, qg, B, L, H, dh), mask=None, rg=r.cuda())
    tag = f"{profile} L{L} dh{dh}"
    for per_head in (False, True):
        w = _weights(hip, c, B, L, H, dh, per_head).cpu().double()
        want = P if per_head else P.mean(dim=1)
        rowsum = (w.sum(-1) - 1).abs().max().item()
        print(f"ERR attn-sharp readout {tag} weights per_head={int(per_head)} "
              f"{((w - want).abs() / (W_TOL['atol'] + W_TOL['rtol'] * want)).max().item():.3e} (bound 1, of atol + rtol |w|); "
              f"|rowsum - 1| {rowsum:.3e} (bound 2e-3)")
        torch.testing.assert_close(w, want, **W_TOL)
        assert rowsum < 2e-3
    for row_w, sw in ((False, 0.0), (True, 0.5)):
        out = _received(hip, c, B, L, H, dh, row_w, sw).cpu().double()
        rr = r.double() if row_w else torch.full((B, L), 1.0 / L, dtype=torch.float64)
        want = _received_ref(P.mean(dim=1), rr, sw)
        print(f"ERR attn-sharp readout {tag} received row_w={int(row_w)} sw={sw} "
              f"{((out - want).abs() / (R_TOL['atol'] + R_TOL['rtol'] * want)).max().item():.3e} (bound 1, of atol + rtol |r|)")
        torch.testing.assert_close(out, want, **R_TOL)
