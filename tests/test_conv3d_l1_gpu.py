"""GPU: every entry point of the fused first voxel layer (csrc/conv3d_l1.hip: Conv3d(1->32, k3, p1) -> BatchNorm3d ->
GELU -> MaxPool3d(2) -> Dropout) against a closed-form fp64 reference of the same operation, evaluated on the operands
the kernels see: the bf16-rounded volume, the bf16 weight image, the bf16 dout, the counter-hash dropout mask and the
max-pool routing the forward kernel reported.  What remains between the two is fp32 accumulation, the bf16 rounding of
dz in front of the weight-gradient MFMA and the fixed-point workspaces.

Inputs go beyond zero-mean noise: fMRI volumes are non-negative with a zero background and a mean far from zero, which
is where the linear-in-(S1, S2) weight gradient dW = sc (A1 - (S1/M) S - (S2/M) A3) can lose its cancellation."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle.dropout_replica import keep_scale
from test_kernels_gpu import _bf, _bn_fin, _hip, _prep_w

pytestmark = pytest.mark.gpu

EPS = 1e-5
SHAPES = [(2, 4, 8, 32),        # FULLT
          (3, 6, 10, 12),       # ragged H and W
          (2, 8, 16, 48),       # config-#4 width: one and a half tiles
          (1, 2, 2, 2),         # smallest legal shape
          (32, 32, 32, 32),     # C2: 2048 tiles, walked persistently
          (2, 62, 64, 64),      # 992 tiles: more than either persistent grid, a multiple of neither
          (4, 64, 64, 48)]      # config #4
INPUTS = ["randn", "mu3", "mu8", "brain", "negbeta"]


def _grad(ws):
    """gradient accumulator workspace -> fp64 sums (the fp32 helper of test_kernels_gpu rounds them)"""
    from multimodal_eeg_fmri_amd.ops import ACC_GRAD, acc_decode
    return acc_decode(ws, ACC_GRAD)


def _eff_seed(seed, epoch):
    """csrc/common.h: mm_eff_seed"""
    return seed if epoch is None else (seed ^ ((epoch * 0x85EBCA6B + 0xC2B2AE35) & 0xFFFFFFFF)) & 0xFFFFFFFF


def _volume(kind, B, D, H, W, g):
    """(a) randn, (b) randn + mu, (c) a masked brain: non-negative intensities inside an ellipsoid, exact zeros outside"""
    x = torch.randn(B, D, H, W, generator=g)
    if kind.startswith("mu"):
        return x + float(kind[2:])
    if kind == "brain":
        ax = [((torch.arange(n, dtype=torch.float64) + 0.5) / n - 0.5) / 0.38 for n in (D, H, W)]
        r2 = ax[0].view(-1, 1, 1) ** 2 + ax[1].view(1, -1, 1) ** 2 + ax[2].view(1, 1, -1) ** 2
        return torch.where((r2 <= 1.0).unsqueeze(0), (3.0 + x).clamp_min(0.0), torch.zeros(()))
    return x


def _case(kind, B, D, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = _volume(kind, B, D, H, W, g)
    w = _bf(torch.randn(32, 27, generator=g) * 0.25)
    bias = torch.randn(32, generator=g) * 0.2
    gam = 0.5 + torch.rand(32, generator=g)
    bet = torch.full((32,), -2.0) if kind == "negbeta" else torch.randn(32, generator=g) * 0.1
    if kind == "negbeta":
        gam = torch.ones(32)
    dout = _bf(torch.randn(B, D // 2, H // 2, W // 2, 32, generator=g))
    return x, w, bias, gam, bet, dout


def _wimg(hip, w):
    """the bf16 [32][32] (n, tap) image the layer-1 kernels read: w as (32, 27, 1) through mm_prep_conv_weight"""
    return _prep_w(hip, w.reshape(32, 27, 1), 32)[0]


def _cols(xb):
    """(27, B, D*H*W) fp64 im2col rows of the zero-padded volume"""
    B, D, H, W = xb.shape
    xp = F.pad(xb, (1, 1, 1, 1, 1, 1))
    return torch.stack([xp[:, kd:kd + D, kh:kh + H, kw:kw + W].reshape(B, -1)
                        for kd in range(3) for kh in range(3) for kw in range(3)])


def _windows(t):
    """(B, C, D, H, W) -> (B, C, D/2, H/2, W/2, 8), member j = (dd << 2) | (hh << 1) | ww"""
    B, C, D, H, W = t.shape
    return t.reshape(B, C, D // 2, 2, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(
        B, C, D // 2, H // 2, W // 2, 8)


def _gelu(z):
    return z * 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))


def _gelu_grad(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def ref_layer(xb, w, bias, gam, bet, keep, dout, route, train, stats=None):
    """closed-form fp64 reference of the layer and of its backward.  xb (B, D, H, W) bf16-rounded volume, w (32, 27)
    bf16 weights, keep (B, D/2, H/2, W/2, 32) dropout scale, dout the same shape (bf16 values), route (same shape, int64)
    the window member the backward routes to.  train: batch statistics; else ``stats`` = (mean, rstd) of the frozen
    BatchNorm.  Returns the pooled output (channels-last), the reference's own first arg-max, the window's largest
    activation gap at the routed member, and the gradients dW (32, 27), dbias, S1 = dbeta, S2 = dgamma."""
    B, D, H, W = xb.shape
    M = B * D * H * W
    b = bias.double() if bias is not None else torch.zeros(32, dtype=torch.float64)
    y = F.conv3d(xb.unsqueeze(1), w.view(32, 1, 3, 3, 3), b, padding=1)                    # (B, 32, D, H, W)
    if train:
        mean = y.mean(dim=(0, 2, 3, 4))
        rstd = 1.0 / torch.sqrt(((y - mean.view(1, -1, 1, 1, 1)) ** 2).mean(dim=(0, 2, 3, 4)) + EPS)
    else:
        mean, rstd = stats
    cv = lambda v: v.view(1, -1, 1, 1, 1)
    xhat = (y - cv(mean)) * cv(rstd)
    del y
    sc = gam.double() * rstd
    z = xhat * cv(gam.double()) + cv(bet.double())
    a = _windows(_gelu(z))
    amax, own = a.max(dim=-1)                         # torch: the FIRST maximal index, as nn.MaxPool3d
    cl = lambda t: t.permute(0, 2, 3, 4, 1)           # (B, C, Do, Ho, Wo) -> channels-last
    out = cl(amax) * keep.double()
    routed = a.gather(-1, route.permute(0, 4, 1, 2, 3).unsqueeze(-1)).squeeze(-1)
    gap = cl(amax - routed)
    del a
    zr = _windows(z).gather(-1, route.permute(0, 4, 1, 2, 3).unsqueeze(-1)).squeeze(-1)
    dzs = (dout.double() * keep.double()).permute(0, 4, 1, 2, 3) * _gelu_grad(zr)
    dz = torch.zeros(B, 32, D // 2, H // 2, W // 2, 8, dtype=torch.float64)
    dz.scatter_(-1, route.permute(0, 4, 1, 2, 3).unsqueeze(-1), dzs.unsqueeze(-1))
    dz = dz.reshape(B, 32, D // 2, H // 2, W // 2, 2, 2, 2).permute(0, 1, 2, 5, 3, 6, 4, 7).reshape(B, 32, D, H, W)
    S1 = dz.sum(dim=(0, 2, 3, 4))
    S2 = (dz * xhat).sum(dim=(0, 2, 3, 4))
    dy = (dz - cv(S1 / M) - xhat * cv(S2 / M)) * cv(sc) if train else dz * cv(sc)
    del dz, xhat, z
    cols = _cols(xb)                                                                    # (27, B, V)
    dW = torch.zeros(32, 27, dtype=torch.float64)
    for i in range(B):
        dW += dy[i].reshape(32, -1) @ cols[:, i].t()
    return dict(out=out, amax=cl(amax), own=cl(own), gap=gap, zr=cl(zr), dW=dW, dbias=dy.sum(dim=(0, 2, 3, 4)), S1=S1, S2=S2,
                mean=mean, rstd=rstd)


def _batch_stats(xb, w, bias):
    y = F.conv3d(xb.unsqueeze(1), w.view(32, 1, 3, 3, 3), bias.double(), padding=1)
    return y.mean(dim=(0, 2, 3, 4)), y.var(dim=(0, 2, 3, 4), unbiased=False)


def _rel(got, want, floor=0.0):
    """rel-L2; ``floor``: a scale for the denominator where the reference itself vanishes (S2 = sum dz xhat of an all-zero
    volume, whose xhat is identically 0, is measured against |S1|)"""
    return float((got - want).norm() / max(float(want.norm()), float(floor), 1e-300))


def _chan_rel(got, want):
    """worst per-channel rel-L2 of a (32, k) gradient, each channel against max(its own norm, the median channel norm)"""
    n = want.norm(dim=1)
    return float(((got - want).norm(dim=1) / torch.maximum(n, n.median()).clamp_min(1e-300)).max())


def _out4_eval(gam, bet, rm, rv, bias=None):
    """bn_fold_eval on the host: [scale, shift (+ conv bias folded), mean, rstd], fp32"""
    rstd = 1.0 / torch.sqrt(rv + EPS)
    sc = gam * rstd
    sh = bet - rm * sc if bias is None else bet + (bias - rm) * sc
    return torch.stack([sc, sh, rm, rstd]).float().contiguous()


class _Layer:
    """the layer's train-mode forward on the GPU (Gram statistics -> finalize), shared by the tests below"""

    def __init__(self, hip, kind, shape, seed, p=0.0, epoch=None):
        B, D, H, W = shape
        self.shape, self.p, self.seed, self.M = shape, p, seed, B * D * H * W
        self.x, self.w, self.bias, self.gam, self.bet, self.dout = _case(kind, B, D, H, W, seed)
        self.xg, self.wimg, self.bg = self.x.cuda(), _wimg(hip, self.w), self.bias.cuda()
        self.gg, self.btg, self.doutg = self.gam.cuda(), self.bet.cuda(), self.dout.cuda().to(torch.bfloat16)
        self.ep = torch.tensor([epoch], dtype=torch.int32, device="cuda") if epoch is not None else None
        self.epoch = epoch
        n_out = B * (D // 2) * (H // 2) * (W // 2) * 32
        self.keep = keep_scale(_eff_seed(seed, epoch), n_out, p).view(B, D // 2, H // 2, W // 2, 32)
        self.gram, self.stats = torch.zeros(32, 32, 32, device="cuda"), torch.zeros(32, 2, 32, device="cuda")
        hip.call("mm_conv3d_l1_gram", self.xg, self.wimg, self.bg, self.gram, self.stats, B, D, H, W)
        self.out4 = torch.full((4, 32), float("nan"), device="cuda")
        rm, rv, nb = torch.zeros(32, device="cuda"), torch.ones(32, device="cuda"), torch.zeros((), dtype=torch.long, device="cuda")
        hip.call("mm_bn_finalize", self.stats, self.gg, self.btg, rm, rv, None, self.out4, 32, float(self.M), 0.1, EPS, 0, nb)

    def winners(self, hip, out4, bias, train):
        B, D, H, W = self.shape
        out = torch.full((B, D // 2, H // 2, W // 2, 32), float("nan"), device="cuda").to(torch.bfloat16)
        arg = torch.full(out.shape, 255, dtype=torch.uint8, device="cuda")
        hip.call("mm_conv3d_l1_fwd_winners", self.xg, self.wimg, bias, out4, out, arg, B, D, H, W, train, self.p,
                 self.seed, self.ep)
        return out, arg

    def bwd(self, hip, out4, gram, train, bias=None, prefill=None, dbias0=None):
        B, D, H, W = self.shape
        sums, a1 = torch.zeros(32, 2, 32, device="cuda"), torch.zeros(32, 27, 32, device="cuda")
        dw = prefill.clone().cuda().view(32, 1, 3, 3, 3).contiguous()
        dbias = dbias0.clone().cuda()
        hip.call("mm_conv3d_l1_bwd", self.xg, self.wimg, self.bg if bias is None else bias, out4, self.doutg, sums, a1,
                 gram, dw, dbias, B, D, H, W, train, self.p, self.seed, self.ep)
        torch.cuda.synchronize()
        return sums, dw.view(32, 27).cpu(), dbias.cpu()


def _params(shapes, inputs):
    return [pytest.param(s, k, id=f"{'x'.join(map(str, s))}-{k}") for s in shapes for k in inputs]


def _dropout_of(shape, kind):
    """p = 0.3 with a seed_epoch word on every other case (deterministic by case), p = 0 otherwise"""
    h = (sum(shape) * 7 + len(kind) * 3 + ord(kind[0])) % 2
    return (0.3, 5 + sum(shape)) if h else (0.0, None)


def _ulp_bf16(v):
    """one bf16 step at |v| (normal range)"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -120)))
    return torch.pow(2.0, e - 7)


@pytest.mark.parametrize("shape,kind", _params(SHAPES, INPUTS))
def test_conv3d_l1_forward_vs_fp64(shape, kind):
    """mm_conv3d_l1 mode 1 (train, and eval with the bias folded into the shift), mm_conv3d_l1_fwd_fin and
    mm_conv3d_l1_fwd_winners: the three train outputs agree bit for bit (the finalize in the prologue writes the same
    out4); every output is within one bf16 step of the fp64 reference, plus 2^-16 absolute for the fp32 rounding of
    z = acc sc + shift where GELU is near 0 (measured worst over the grid: 0.512 of a step above 2^-8, 8.1e-6 absolute
    below it); the winners are the reference's FIRST arg-max except at near-ties (mismatch fraction <= 5e-5, measured
    1.8e-5; activation gap <= 2^-16 (1 + |max|)); on an exact tie (an all-zero neighbourhood of the masked brain) the
    winner is member 0."""
    hip = _hip()
    B, D, H, W = shape
    p, epoch = _dropout_of(shape, kind)
    L = _Layer(hip, kind, shape, seed=1000 + B * D + H * W, p=p, epoch=epoch)
    outs = []
    out1 = torch.full((B, D // 2, H // 2, W // 2, 32), float("nan"), device="cuda").to(torch.bfloat16)
    hip.call("mm_conv3d_l1", 1, L.xg, L.wimg, L.bg, L.out4, None, None, None, out1, None, None, B, D, H, W, 1, p,
             L.seed, L.ep)
    outs.append(out1)
    ow, arg = L.winners(hip, L.out4, L.bg, 1)
    outs.append(ow)
    rm, rv, nb = torch.zeros(32, device="cuda"), torch.ones(32, device="cuda"), torch.zeros((), dtype=torch.long, device="cuda")
    out4f = torch.full((4, 32), float("nan"), device="cuda")
    addr, keepalive = _bn_fin(L.stats, L.gg, L.btg, rm, rv, out4f, nb, L.M)
    outf = torch.full_like(out1, float("nan"))
    hip.call("mm_conv3d_l1_fwd_fin", L.xg, L.wimg, L.bg, addr, outf, B, D, H, W, p, L.seed, L.ep)
    outs.append(outf)
    torch.cuda.synchronize()
    assert torch.equal(out4f, L.out4)
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    route = arg.long().cpu()
    assert int(route.max()) <= 7
    xb = _bf(L.x).double()
    R = ref_layer(xb, L.w.double(), L.bias, L.gam, L.bet, L.keep, L.dout, route, True)
    got = out1.float().cpu().double()
    err = (got - R["out"]).abs()
    big = R["out"].abs() >= 2.0 ** -8
    print(f"\nMEASURE fwd {shape} {kind} p={p}: err/ulp {float((err / _ulp_bf16(R['out']))[big].max()) if big.any() else 0:.3f} "
          f"max abs err below 2^-8 {float(err[~big].max()) if (~big).any() else 0:.3e} "
          f"winner mismatch {float((route != R['own']).double().mean()):.2e}")
    assert bool((err <= _ulp_bf16(R["out"]) + 2.0 ** -16).all()), f"max err / ulp {float((err / _ulp_bf16(R['out'])).max())}"
    # winners: first arg-max except at near-ties
    miss = route != R["own"]
    frac = float(miss.double().mean())
    assert frac <= 5e-5, frac
    if miss.any():
        gap = R["gap"][miss]
        lim = 2.0 ** -16 * (1.0 + R["amax"][miss].abs())
        assert bool((gap <= lim).all()), float(gap.max())
    # exact ties: all eight members equal in fp64 -> member 0
    y = F.conv3d(xb.unsqueeze(1), L.w.double().view(32, 1, 3, 3, 3), L.bias.double(), padding=1)
    yw = _windows(y)
    tie = (yw.amax(-1) == yw.amin(-1)).permute(0, 2, 3, 4, 1)
    if kind == "brain":
        assert tie.any()
    assert bool((route[tie] == 0).all())
    # eval: frozen running statistics, the conv bias folded into the shift (bias = NULL)
    rm_e, rv_e = torch.randn(32) * 0.3 + R["mean"].float(), (0.5 + torch.rand(32)) / R["rstd"].float() ** 2
    o4 = _out4_eval(L.gam, L.bet, rm_e, rv_e, L.bias).cuda()
    oute = torch.full_like(out1, float("nan"))
    hip.call("mm_conv3d_l1", 1, L.xg, L.wimg, None, o4, None, None, None, oute, None, None, B, D, H, W, 0, 0.0, 0, None)
    torch.cuda.synchronize()
    o4c = o4.cpu().double()
    # the folded form has no separate bias: mean' = rm - bias, so that xhat = (conv - mean') rstd
    Re = ref_layer(xb, L.w.double(), None, L.gam, L.bet, torch.ones_like(L.keep), L.dout, route, False,
                   stats=(rm_e.double() - L.bias.double(), o4c[3]))
    erre = (oute.float().cpu().double() - Re["out"]).abs()
    assert bool((erre <= _ulp_bf16(Re["out"]) + 2.0 ** -16).all()), float((erre / _ulp_bf16(Re["out"])).max())


# Bounds: at most 3x the worst case measured over the whole grid of shapes x inputs (35 cases per test), and never
# above the ceilings 5e-3 (dW) / 1e-4 (sums).  Measured worst (rel-L2 per tensor):
#   dW (mode 4)         train 2.56e-3 (1x2x2x2 negbeta), frozen 2.14e-3 (2x62x64x64 brain): the bf16 rounding of dz
#   dW worst channel    train 6.39e-3, frozen 1.03e-2 (4x64x64x48 mu8)
#   dW (mode 3)         4.49e-5 (2x62x64x64 mu8)
#   S1 = dbeta          1.60e-6 (1x2x2x2 brain; 2.8e-7 elsewhere)    S2 = dgamma  1.49e-6 (4x64x64x48 mu8)
#   dbias (frozen)      5.08e-7 (1x2x2x2 negbeta)
# Without the mean correction of A1 (c0 = S1 / M alone), train-mode dW reached 8.17e-3 (32^4 mu8), 5.24e-3 (2x62x64x64 mu8),
# 5.11e-3 (4x64x64x48 mu8), and the one-term bf16 dy of mode 3 9.36e-3 (2x62x64x64 mu8).
DW_BOUND = 5e-3
CH_BOUND = 3e-2
DW3_BOUND = 1.3e-4
SUM_BOUND = 4.5e-6
DBIAS_BOUND = 1.5e-6


@pytest.mark.parametrize("shape,kind", _params(SHAPES, INPUTS))
def test_conv3d_l1_backward_train_bn_vs_fp64(shape, kind):
    """mm_conv3d_l1_bwd (mode 4 + l1_combine_kernel) with train-mode BatchNorm: gram from mm_conv3d_l1_gram, out4 from
    mm_bn_finalize, against the fp64 reference routed through the kernel's own winners (bounds and measurements: above).
    One run at mu / sigma = 30 (not asserted): dW 2.54e-3 (2x8x16x48) / 2.25e-3 (32^4), S2 1.2e-6, mode 3 3.6e-5.  dW (rel-L2 and worst channel),
    S1 = dbeta and S2 = dgamma; dw is ADDED to (pre-filled), dbias is untouched (its gradient is identically 0), two
    launches are bit-identical, mode 2's sums equal mode 4's bit for bit, and mode 3 (the two-pass weight gradient)
    meets the same bound."""
    hip = _hip()
    B, D, H, W = shape
    p, epoch = _dropout_of(shape, kind)
    L = _Layer(hip, kind, shape, seed=2000 + B * D + H * W, p=p, epoch=epoch)
    _, arg = L.winners(hip, L.out4, L.bg, 1)
    route = arg.long().cpu()
    R = ref_layer(_bf(L.x).double(), L.w.double(), L.bias, L.gam, L.bet, L.keep, L.dout, route, True)
    g = torch.Generator().manual_seed(B + W)
    prefill = torch.randn(32, 27, generator=g) * float(R["dW"].norm()) / math.sqrt(32 * 27)
    db0 = torch.randn(32, generator=g)
    sums, dw, dbias = L.bwd(hip, L.out4, L.gram, 1, prefill=prefill, dbias0=db0)
    sums_b, dw_b, dbias_b = L.bwd(hip, L.out4, L.gram, 1, prefill=prefill, dbias0=db0)
    i64 = lambda ws: ws.view(torch.int64)            # fixed-point workspaces: compare the integers, not float views
    assert torch.equal(i64(sums), i64(sums_b)) and torch.equal(dw, dw_b) and torch.equal(dbias, dbias_b)
    assert torch.equal(dbias, db0)
    S = _grad(sums).cpu()
    e_dw = _rel(dw.double() - prefill.double(), R["dW"])
    e_ch = _chan_rel(dw.double() - prefill.double(), R["dW"])
    e_s1, e_s2 = _rel(S[0], R["S1"]), _rel(S[1], R["S2"], R["S1"].norm())
    # mode 2: the sums alone, same bits
    sums2 = torch.zeros(32, 2, 32, device="cuda")
    hip.call("mm_conv3d_l1", 2, L.xg, L.wimg, L.bg, L.out4, L.doutg, None, sums2, None, None, None, B, D, H, W, 1,
             L.p, L.seed, L.ep)
    # mode 3: dW = x^T dy with dy formed per voxel from the compact sums
    dw3, db3 = torch.zeros(32, 27, 32, device="cuda"), torch.zeros(32, 32, device="cuda")
    compact = _grad(sums).float().cuda().contiguous()
    hip.call("mm_conv3d_l1", 3, L.xg, L.wimg, L.bg, L.out4, L.doutg, compact, None, None, dw3, db3, B, D, H, W, 1,
             L.p, L.seed, L.ep)
    torch.cuda.synchronize()
    e_dw3 = _rel(_grad(dw3).cpu().t(), R["dW"])
    print(f"\nMEASURE bwd_train {shape} {kind} p={p}: dW {e_dw:.3e} chan {e_ch:.3e} S1 {e_s1:.3e} S2 {e_s2:.3e} "
          f"mode3 {e_dw3:.3e}")
    assert torch.equal(i64(sums2), i64(sums))
    assert e_dw <= DW_BOUND and e_ch <= CH_BOUND and e_dw3 <= DW3_BOUND, (e_dw, e_ch, e_dw3)
    assert e_s1 <= SUM_BOUND and e_s2 <= SUM_BOUND, (e_s1, e_s2)


@pytest.mark.parametrize("shape,kind", _params(SHAPES, INPUTS))
def test_conv3d_l1_backward_frozen_bn_vs_fp64(shape, kind):
    """mm_conv3d_l1_bwd with frozen BatchNorm (train = 0, gram = NULL, eval out4 with the conv bias separate): dW and
    dbias = scale * S1 against the fp64 reference, both ADDED to pre-filled tensors."""
    hip = _hip()
    B, D, H, W = shape
    p, epoch = _dropout_of(shape, kind)
    L = _Layer(hip, kind, shape, seed=3000 + B * D + H * W, p=p, epoch=epoch)
    g = torch.Generator().manual_seed(7 + W)
    # running statistics near the batch's own, so that the activations sit where training put them
    mean, var = _batch_stats(_bf(L.x).double(), L.w.double(), L.bias)
    rm = mean.float() + torch.randn(32, generator=g) * 0.1
    rv = (0.7 + 0.6 * torch.rand(32, generator=g)) * var.float()
    o4 = _out4_eval(L.gam, L.bet, rm, rv).cuda()
    _, arg = L.winners(hip, o4, L.bg, 0)
    route = arg.long().cpu()
    o4c = o4.cpu().double()
    R = ref_layer(_bf(L.x).double(), L.w.double(), L.bias, L.gam, L.bet, L.keep, L.dout, route, False,
                  stats=(o4c[2], o4c[3]))
    prefill = torch.randn(32, 27, generator=g) * float(R["dW"].norm()) / math.sqrt(32 * 27)
    db0 = torch.randn(32, generator=g) * float(R["dbias"].norm()) / math.sqrt(32)
    sums, dw, dbias = L.bwd(hip, o4, None, 0, prefill=prefill, dbias0=db0)
    S = _grad(sums).cpu()
    e_dw = _rel(dw.double() - prefill.double(), R["dW"])
    e_ch = _chan_rel(dw.double() - prefill.double(), R["dW"])
    e_db = _rel(dbias.double() - db0.double(), R["dbias"])
    e_s1, e_s2 = _rel(S[0], R["S1"]), _rel(S[1], R["S2"], R["S1"].norm())
    print(f"\nMEASURE bwd_frozen {shape} {kind} p={p}: dW {e_dw:.3e} chan {e_ch:.3e} dbias {e_db:.3e} "
          f"S1 {e_s1:.3e} S2 {e_s2:.3e}")
    assert e_dw <= DW_BOUND and e_ch <= CH_BOUND, (e_dw, e_ch)
    assert e_db <= DBIAS_BOUND and e_s1 <= SUM_BOUND and e_s2 <= SUM_BOUND, (e_db, e_s1, e_s2)
