"""GPU: the voxel encoder at volume extents that are not multiples of 4 (MNI152 at 2 mm is 91 x 109 x 91, at 3 mm
61 x 73 x 61; EPI often has an odd slice count).  torch's semantics, exactly: the convolution covers the whole volume,
train-mode BatchNorm counts all B D H W conv outputs (the tail - the last plane / row / column that no pooling window
covers - included), MaxPool3d(2) floors, the tail gets no gradient through the pool but BatchNorm's backward term.

Every kernel of the fused first layer, the generic pooled BatchNorm pass, the convolution GEMMs at the layer shapes of
a 91 x 109 x 91 volume, the module (eval, train, frozen BatchNorm, d / d volume, dropout) and the trainer (graph replay,
host-fed loop) are checked against references that evaluate those semantics directly."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_functional as RF
from oracle.fixtures import build, seeded_randn

import multimodal_eeg_fmri_amd.fmri_utils as Fm
from test_conv3d_l1_gpu import (CH_BOUND, DW3_BOUND, DW_BOUND, SUM_BOUND, _chan_rel, _cols, _gelu, _gelu_grad, _grad,
                                _Layer, _rel, _ulp_bf16, _windows)
from test_kernels_gpu import _bf, _bn_fin, _hip, _prep_w, _stat, _vol_cl
from test_models_gpu import COS_TOL, _oracle_grads, _worst, bn_cancelled_biases, cos_min, rel_err

pytestmark = pytest.mark.gpu

EPS = 1e-5


def _floor2(t):
    """(B, C, D, H, W) -> its window extent 2[D/2] x 2[H/2] x 2[W/2] (the corner the pools cover)"""
    D, H, W = t.shape[2:]
    return t[:, :, :D // 2 * 2, :H // 2 * 2, :W // 2 * 2]


def _unwindows(t, D, H, W):
    """(B, C, D/2, H/2, W/2, 8) window members -> (B, C, D, H, W), zero on the tail"""
    B, C, Do, Ho, Wo, _ = t.shape
    v = t.reshape(B, C, Do, Ho, Wo, 2, 2, 2).permute(0, 1, 2, 5, 3, 6, 4, 7).reshape(B, C, 2 * Do, 2 * Ho, 2 * Wo)
    return F.pad(v, (0, W - 2 * Wo, 0, H - 2 * Ho, 0, D - 2 * Do))


def ref_layer_odd(xb, w, bias, gam, bet, keep, dout, route):
    """fp64 closed form of the fused layer's train-mode forward and backward at any extent (tests/test_conv3d_l1_gpu.py:
    ref_layer, with the pools floored and the BatchNorm statistics and dy over the whole volume)"""
    B, D, H, W = xb.shape
    M = B * D * H * W
    y = F.conv3d(xb.unsqueeze(1), w.view(32, 1, 3, 3, 3), bias.double(), padding=1)
    mean = y.mean(dim=(0, 2, 3, 4))
    rstd = 1.0 / torch.sqrt(((y - mean.view(1, -1, 1, 1, 1)) ** 2).mean(dim=(0, 2, 3, 4)) + EPS)
    cv = lambda v: v.view(1, -1, 1, 1, 1)
    xhat = (y - cv(mean)) * cv(rstd)
    sums = torch.stack([y.sum(dim=(0, 2, 3, 4)), (y * y).sum(dim=(0, 2, 3, 4))])
    del y
    sc = gam.double() * rstd
    z = xhat * cv(gam.double()) + cv(bet.double())
    a = _windows(_floor2(_gelu(z)))
    amax, own = a.max(dim=-1)
    cl = lambda t: t.permute(0, 2, 3, 4, 1)
    rt = route.permute(0, 4, 1, 2, 3).unsqueeze(-1)
    gap = cl(amax - a.gather(-1, rt).squeeze(-1))
    del a
    zr = _windows(_floor2(z)).gather(-1, rt).squeeze(-1)
    dzs = (dout.double() * keep.double()).permute(0, 4, 1, 2, 3) * _gelu_grad(zr)
    dzw = torch.zeros(*dzs.shape, 8, dtype=torch.float64)
    dzw.scatter_(-1, rt, dzs.unsqueeze(-1))
    dz = _unwindows(dzw, D, H, W)
    del dzw, z
    S1 = dz.sum(dim=(0, 2, 3, 4))
    S2 = (dz * xhat).sum(dim=(0, 2, 3, 4))
    dy = (dz - cv(S1 / M) - xhat * cv(S2 / M)) * cv(sc)
    del dz, xhat
    cols = _cols(xb)
    dW = torch.zeros(32, 27, dtype=torch.float64)
    for i in range(B):
        dW += dy[i].reshape(32, -1) @ cols[:, i].t()
    S = cols.sum(dim=(1, 2))
    return dict(out=cl(amax) * keep.double(), amax=cl(amax), own=cl(own), gap=gap, dW=dW, S1=S1, S2=S2, sums=sums, S=S)


L1_SHAPES = [(2, 5, 7, 9), (3, 7, 10, 33), (2, 9, 17, 35), (1, 91, 109, 91)]


@pytest.mark.parametrize("shape,kind", [pytest.param(s, k, id=f"{'x'.join(map(str, s))}-{k}")
                                        for s in L1_SHAPES for k in ("randn", "brain")])
def test_fused_layer1_at_odd_extents_vs_fp64(shape, kind):
    """mm_conv3d_l1_gram (M = B D H W, S and the BatchNorm statistics of the whole volume), the three forward entry
    points (pooled output and winners on the floored windows), mm_conv3d_l1_bwd (S1, S2, dW with the tail's BatchNorm
    term carried by S and A3), mode 2 (same sums) and mode 3 (dense dy over the whole volume), with the bounds of
    tests/test_conv3d_l1_gpu.py."""
    from multimodal_eeg_fmri_amd.ops import ACC_STAT, acc_decode
    hip = _hip()
    B, D, H, W = shape
    p, epoch = (0.3, 11) if (D + W) % 4 == 0 else (0.0, None)
    L = _Layer(hip, kind, shape, seed=5000 + B * D + H * W, p=p, epoch=epoch)
    xb = _bf(L.x).double()
    # --- Gram matrix: count, tap sums, statistics
    G = acc_decode(L.gram, ACC_STAT).cpu()
    assert float(G[27, 27]) == L.M, (float(G[27, 27]), L.M)
    # --- forward: mode 1, winners, fin agree bit for bit
    Do, Ho, Wo = D // 2, H // 2, W // 2
    out1 = torch.full((B, Do, Ho, Wo, 32), float("nan"), device="cuda").to(torch.bfloat16)
    hip.call("mm_conv3d_l1", 1, L.xg, L.wimg, L.bg, L.out4, None, None, None, out1, None, None, B, D, H, W, 1, p,
             L.seed, L.ep)
    ow, arg = L.winners(hip, L.out4, L.bg, 1)
    rm, rv, nb = torch.zeros(32, device="cuda"), torch.ones(32, device="cuda"), torch.zeros((), dtype=torch.long, device="cuda")
    out4f = torch.full((4, 32), float("nan"), device="cuda")
    addr, keepalive = _bn_fin(L.stats, L.gg, L.btg, rm, rv, out4f, nb, L.M)
    outf = torch.full_like(out1, float("nan"))
    hip.call("mm_conv3d_l1_fwd_fin", L.xg, L.wimg, L.bg, addr, outf, B, D, H, W, p, L.seed, L.ep)
    torch.cuda.synchronize()
    assert torch.equal(out4f, L.out4) and torch.equal(ow, out1) and torch.equal(outf, out1)
    route = arg.long().cpu()
    assert int(route.max()) <= 7
    R = ref_layer_odd(xb, L.w.double(), L.bias, L.gam, L.bet, L.keep, L.dout, route)
    G = G.double()
    torch.testing.assert_close(G[:27, 27], R["S"], rtol=3e-5, atol=3e-5 * float(G.abs().max()))
    # the BatchNorm sums derived from G, and mode 0 (statistics by recompute: it walks the volume extent too)
    got = _stat(L.stats).cpu().double()
    tol = dict(rtol=2e-5, atol=2e-5 * float(R["sums"].abs().max()))
    torch.testing.assert_close(got, R["sums"], **tol)
    stats0 = torch.zeros(32, 2, 32, device="cuda")
    hip.call("mm_conv3d_l1", 0, L.xg, L.wimg, L.bg, None, None, None, stats0, None, None, None, B, D, H, W, 1, 0.0, 0, None)
    torch.cuda.synchronize()
    torch.testing.assert_close(_stat(stats0).cpu().double(), R["sums"], **tol)
    got = out1.float().cpu().double()
    err = (got - R["out"]).abs()
    assert bool((err <= _ulp_bf16(R["out"]) + 2.0 ** -16).all()), float((err / _ulp_bf16(R["out"])).max())
    miss = route != R["own"]
    assert float(miss.double().mean()) <= 5e-5
    if miss.any():
        assert bool((R["gap"][miss] <= 2.0 ** -16 * (1.0 + R["amax"][miss].abs())).all())
    # --- backward: mode 4 + combine
    g = torch.Generator().manual_seed(B + W)
    prefill = torch.randn(32, 27, generator=g) * float(R["dW"].norm()) / math.sqrt(32 * 27)
    db0 = torch.randn(32, generator=g)
    sums, dw, dbias = L.bwd(hip, L.out4, L.gram, 1, prefill=prefill, dbias0=db0)
    S = _grad(sums).cpu()
    e_dw = _rel(dw.double() - prefill.double(), R["dW"])
    e_ch = _chan_rel(dw.double() - prefill.double(), R["dW"])
    e_s1, e_s2 = _rel(S[0], R["S1"]), _rel(S[1], R["S2"], R["S1"].norm())
    sums2 = torch.zeros(32, 2, 32, device="cuda")
    hip.call("mm_conv3d_l1", 2, L.xg, L.wimg, L.bg, L.out4, L.doutg, None, sums2, None, None, None, B, D, H, W, 1,
             L.p, L.seed, L.ep)
    dw3, db3 = torch.zeros(32, 27, 32, device="cuda"), torch.zeros(32, 32, device="cuda")
    compact = _grad(sums).float().cuda().contiguous()
    hip.call("mm_conv3d_l1", 3, L.xg, L.wimg, L.bg, L.out4, L.doutg, compact, None, None, dw3, db3, B, D, H, W, 1,
             L.p, L.seed, L.ep)
    torch.cuda.synchronize()
    e_dw3 = _rel(_grad(dw3).cpu().t(), R["dW"])
    print(f"\nMEASURE odd l1 {shape} {kind} p={p}: dW {e_dw:.3e} chan {e_ch:.3e} S1 {e_s1:.3e} S2 {e_s2:.3e} mode3 {e_dw3:.3e}")
    assert torch.equal(sums2.view(torch.int64), sums.view(torch.int64))
    assert torch.equal(dbias, db0)
    assert e_dw <= DW_BOUND and e_ch <= CH_BOUND and e_dw3 <= DW3_BOUND, (e_dw, e_ch, e_dw3)
    assert e_s1 <= SUM_BOUND and e_s2 <= SUM_BOUND, (e_s1, e_s2)


@pytest.mark.parametrize("N", [32, 64])
@pytest.mark.parametrize("train", [1, 0])
def test_pool3d_bn_act_at_odd_extents_vs_torch(N, train):
    """mm_pool3d_bn_act_fwd / _bwd_reduce / _bwd_apply on a 7 x 9 x 11 volume vs torch autograd of batch_norm -> gelu
    -> max_pool3d (fp64) on the same bf16 y.  dy is pre-filled with NaN: the apply pass must write every element, the
    tail's with BatchNorm's term (train) or exactly 0 (frozen)."""
    from multimodal_eeg_fmri_amd.ops import ACC_STAT, acc_encode
    hip = _hip()
    g = torch.Generator().manual_seed(N + train)
    B, D, H, W = 2, 7, 9, 11
    Do, Ho, Wo = D // 2, H // 2, W // 2
    y = (torch.randn(B, D, H, W, N, generator=g) * 1.3 + 0.2).to(torch.bfloat16)
    gam, bet = 0.5 + torch.rand(N, generator=g), torch.randn(N, generator=g) * 0.1
    dout = torch.randn(B, Do, Ho, Wo, N, generator=g).to(torch.bfloat16)
    yf = y.double()
    yt = yf.permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    if train:
        rm, rv = torch.zeros(N, dtype=torch.float64), torch.ones(N, dtype=torch.float64)
    else:
        rm = yf.mean(dim=(0, 1, 2, 3)) + torch.randn(N, generator=g).double() * 0.1
        rv = yf.var(dim=(0, 1, 2, 3)) * (0.7 + 0.6 * torch.rand(N, generator=g).double())
    z = F.batch_norm(yt, rm.clone(), rv.clone(), gam.double(), bet.double(), training=bool(train), eps=EPS)
    o = F.max_pool3d(F.gelu(z), 2)
    o.backward(dout.double().permute(0, 4, 1, 2, 3))
    want_out = o.detach().permute(0, 2, 3, 4, 1)
    want_dy = yt.grad.permute(0, 2, 3, 4, 1)
    yg = y.cuda()
    if train:
        cnt = B * D * H * W
        stats = acc_encode(torch.stack([y.float().sum(dim=(0, 1, 2, 3)), (y.float() ** 2).sum(dim=(0, 1, 2, 3))]),
                           ACC_STAT).contiguous().cuda()
        out4 = torch.full((4, N), float("nan"), device="cuda")
        nb = torch.zeros((), dtype=torch.long, device="cuda")
        hip.call("mm_bn_finalize", stats, gam.cuda(), bet.cuda(), torch.zeros(N, device="cuda"), torch.ones(N, device="cuda"),
                 None, out4, N, float(cnt), 0.1, EPS, 0, nb)
    else:
        rstd = 1.0 / torch.sqrt(rv + EPS)
        sc = gam.double() * rstd
        out4 = torch.stack([sc, bet.double() - rm * sc, rm, rstd]).float().contiguous().cuda()
    out = torch.full((B, Do, Ho, Wo, N), float("nan"), device="cuda").to(torch.bfloat16)
    ysel, arg = torch.empty_like(out), torch.empty(out.shape, dtype=torch.uint8, device="cuda")
    hip.call("mm_pool3d_bn_act_fwd", yg, out4, out, ysel, arg, B, D, H, W, N, 1, 0.0, 0, None)
    sums = torch.zeros(32, 2, N, device="cuda")
    hip.call("mm_pool3d_bn_act_bwd_reduce", ysel, out4, dout.cuda(), sums, B, D, H, W, N, 1, 0.0, 0, None)
    dy = torch.full((B, D, H, W, N), float("nan"), device="cuda").to(torch.bfloat16)
    hip.call("mm_pool3d_bn_act_bwd_apply", yg, arg, out4, dout.cuda(), sums, dy, B, D, H, W, N, 1, 0.0, 0, None, train, 32)
    torch.cuda.synchronize()
    got_out, got_dy = out.double().cpu(), dy.double().cpu()
    torch.testing.assert_close(got_out, want_out, rtol=1.6e-2, atol=2e-3)
    assert bool(torch.isfinite(got_dy).all())
    scale = float(want_dy.abs().max())
    assert rel_err(got_dy, want_dy) <= 1e-2, rel_err(got_dy, want_dy)
    tail = torch.ones(B, D, H, W, N, dtype=torch.bool)
    tail[:, :2 * Do, :2 * Ho, :2 * Wo] = False
    if train:
        assert float(want_dy[tail].abs().max()) > 0
        torch.testing.assert_close(got_dy[tail], want_dy[tail], rtol=1.6e-2, atol=1e-3 * scale)
    else:
        assert bool((got_dy[tail] == 0).all())
    # the winners' side: every element of the window extent within bf16 rounding (a routing flip at a near-tie would
    # move a whole entry: none at these values)
    torch.testing.assert_close(got_dy[~tail], want_dy[~tail], rtol=1.6e-2, atol=1e-2 * scale)


@pytest.mark.parametrize("Cin,Cout,D,H,W", [(32, 64, 45, 54, 45), (64, 128, 22, 27, 22)])
def test_conv3d_gemms_at_the_mni_layer_shapes(Cin, Cout, D, H, W):
    """layers 2 and 3 of a 91 x 109 x 91 volume (no extent a multiple of 4): forward (fp32 out with statistics, and the
    bf16 out of the training path), data gradient (the forward kernel on the transposed weights) and weight gradient vs
    F.conv3d on bf16 operands"""
    import ctypes
    hip = _hip()
    B = 1
    g = torch.Generator().manual_seed(Cin + D)
    x = _bf(torch.randn(B, Cin, D, H, W, generator=g)).requires_grad_(True)
    w = _bf(torch.randn(Cout, Cin, 3, 3, 3, generator=g) / math.sqrt(27 * Cin)).requires_grad_(True)
    bias = torch.randn(Cout, generator=g)
    dy = _bf(torch.randn(B, Cout, D, H, W, generator=g))
    y = F.conv3d(x, w, bias, padding=1)
    y.backward(dy)
    wf, wd = _prep_w(hip, w.detach().reshape(Cout, Cin, 27), Cin, Cout)
    xg = _vol_cl(x.detach())
    want = y.detach().permute(0, 2, 3, 4, 1)
    out = torch.empty(B, D, H, W, Cout, device="cuda")
    stats = torch.zeros(32, 2, Cout, device="cuda")
    hip.call("mm_conv3d_fwd", xg, wf, B, D, H, W, Cin, Cout, bias.cuda(), stats, out, None)
    outb = torch.empty(B, D, H, W, Cout, device="cuda", dtype=torch.bfloat16)
    statsb = torch.zeros(32, 2, Cout, device="cuda")
    hip.call("mm_conv3d_fwd", xg, wf, B, D, H, W, Cin, Cout, bias.cuda(), statsb, None, outb)
    torch.cuda.synchronize()
    torch.testing.assert_close(out.cpu(), want, rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(outb.float().cpu(), want, rtol=1.6e-2, atol=1e-2)
    st = _stat(stats).cpu()
    torch.testing.assert_close(st[0], want.sum(dim=(0, 1, 2, 3)), rtol=1e-3, atol=1.0)
    torch.testing.assert_close(st[1], (want * want).sum(dim=(0, 1, 2, 3)), rtol=1e-3, atol=1.0)
    torch.testing.assert_close(_stat(statsb).cpu(), st, rtol=1e-3, atol=1.0)
    dyg = _vol_cl(dy)
    n = ctypes.c_int(0)
    hip.call("mm_conv3d_wgrad_slots", B, D, H, W, Cin, Cout, ctypes.addressof(n))
    ws = torch.full((n.value, Cout, 27, Cin), float("nan"), device="cuda")
    hip.call("mm_conv3d_wgrad", dyg, xg, ws, None, B, D, H, W, Cin, Cout, Cin, 27 * Cin, 1, Cin, n.value, Cout * 27 * Cin, 1)
    dw = torch.zeros(Cout, Cin, 27, device="cuda")
    hip.call("mm_wgrad_scatter", ws, dw, Cout, Cin, 27, Cin, n.value)
    dx = torch.empty(B, D, H, W, Cin, device="cuda", dtype=torch.bfloat16)
    hip.call("mm_conv3d_fwd", dyg, wd, B, D, H, W, Cout, Cin, None, None, None, dx)
    torch.cuda.synchronize()
    assert rel_err(dw.cpu().view_as(w), w.grad) <= 1e-3, rel_err(dw.cpu().view_as(w), w.grad)
    want_dx = x.grad.permute(0, 2, 3, 4, 1)
    torch.testing.assert_close(dx.float().cpu(), want_dx, rtol=1.6e-2, atol=1e-2 * float(want_dx.abs().max()))


@pytest.mark.parametrize("shape", [(2, 1, 19, 21, 23), (1, 1, 61, 73, 61), (1, 1, 91, 109, 91)])
def test_volume_encoder_eval_at_odd_shapes_vs_oracle(shape):
    """as test_models_gpu.test_volume_encoder_eval_vs_oracle: cos >= 1 - 1e-4 vs the CPU restatement (torch semantics)"""
    m = build(Fm.fMRIVolumeEncoder3D, 41).eval()
    x = seeded_randn(141, *shape)
    with torch.no_grad():
        want = RF.volume_encoder3d(m.state_dict(), x)
        got = m.cuda()(x.cuda()).cpu()
    assert got.shape == want.shape
    assert cos_min(got, want) >= 1 - COS_TOL, cos_min(got, want)
    assert rel_err(got, want) < 2e-2


def _routed(monkeypatch, sd, x, route, stages):
    """the UNMODIFIED fp32 oracle with its two pools routed as the HIP path routed them; RF.max_pool3d_routed reshapes
    without flooring, so the tail is cropped in front of it"""
    real = RF.max_pool3d_routed
    monkeypatch.setattr(RF, "max_pool3d_routed", lambda h, r: real(_floor2(h), r))
    try:
        return RF.volume_encoder3d(sd, x, train=True, route=route, stages=stages)
    finally:
        monkeypatch.setattr(RF, "max_pool3d_routed", real)


@pytest.mark.parametrize("shape,seed", [((4, 1, 19, 21, 23), 43), ((2, 1, 33, 35, 37), 44)])
def test_volume_encoder_train_grads_at_odd_shapes_vs_oracle(shape, seed, monkeypatch):
    """train mode, odd at both pools: every parameter gradient <= 5e-2 rel-L2 vs the bf16-operand oracle and vs the
    unmodified fp32 oracle routed as the HIP path routed; the BatchNorm running statistics after the step match the
    oracle's batch statistics over all B D H W voxels (momentum 0.1, unbiased variance)"""
    from multimodal_eeg_fmri_amd import ops
    m = build(Fm.fMRIVolumeEncoder3D, seed, dropout=0.0).train()
    x = seeded_randn(300 + seed, *shape)
    gy = seeded_randn(400 + seed, shape[0], 64)
    _, g16 = _oracle_grads(RF.volume_encoder3d, m, x, gy=gy, emulate=True)
    mg = build(Fm.fMRIVolumeEncoder3D, seed, dropout=0.0).train().cuda()
    y = mg(x.cuda())
    y.backward(gy.cuda())
    zero = bn_cancelled_biases(mg)
    w16 = _worst(mg.named_parameters(), g16, zero=zero)
    assert w16[1] <= 5e-2, ("vs bf16-operand oracle", w16)
    winners = []
    mw = build(Fm.fMRIVolumeEncoder3D, seed, dropout=0.0).train().cuda()
    with torch.no_grad():
        out_w, _ = ops._vol_forward_impl(mw, x.cuda(), True, True, winners=winners)
    assert torch.equal(out_w, y.detach())
    route = tuple(w.long().permute(0, 4, 1, 2, 3).contiguous().cpu() for w in winners)
    D, H, W = shape[2:]
    assert route[0].shape[2:] == (D // 2, H // 2, W // 2)
    assert route[1].shape[2:] == (D // 4, H // 4, W // 4)
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}
    stages = {}
    out = _routed(monkeypatch, sd, x, route, stages)
    out.backward(gy)
    want = {k: v.grad for k, v in sd.items() if v.requires_grad and v.grad is not None}
    assert cos_min(y.detach().cpu(), out.detach()) >= 1 - COS_TOL
    w32 = _worst(mg.named_parameters(), want, zero=zero)
    assert w32[1] <= 5e-2, ("vs the unmodified fp32 oracle routed as the HIP path", w32)
    # running statistics: batch statistics of each conv output over the WHOLE volume, tail included
    c = "conv_layers."
    with torch.no_grad():
        ins = {"0": x, "5": stages["conv1"].detach(), "10": stages["conv2"].detach()}
        for conv, bn in (("0", "1"), ("5", "6"), ("10", "11")):
            yc = F.conv3d(ins[conv], sd[c + conv + ".weight"], sd[c + conv + ".bias"], padding=1)
            rm, rv = m.state_dict()[c + bn + ".running_mean"].clone(), m.state_dict()[c + bn + ".running_var"].clone()
            F.batch_norm(yc, rm, rv, training=True, momentum=0.1, eps=EPS)
            got_m = mg.state_dict()[c + bn + ".running_mean"].cpu()
            got_v = mg.state_dict()[c + bn + ".running_var"].cpu()
            torch.testing.assert_close(got_m, rm, rtol=1e-2, atol=2e-3 * float(rv.sqrt().max()))
            torch.testing.assert_close(got_v, rv, rtol=1e-2, atol=1e-4)
            assert int(mg.state_dict()[c + bn + ".num_batches_tracked"]) == 1


def test_volume_encoder_other_modes_at_an_odd_shape():
    """frozen-BatchNorm backward (fused layer 1), d / d volume (layer 1 as an implicit GEMM: the generic pooled pass's
    tail rule with frozen BatchNorm) and dropout 0.3 vs the masked oracle, at 19 x 21 x 23 (odd at both pools), with
    the tolerances of the even-shape tests in test_models_gpu.py"""
    from oracle.bf16_emulation import bf16_operands
    from oracle.dropout_replica import volume_encoder_train_with_masks
    from test_models_gpu import _log_seeds
    shape = (3, 1, 19, 21, 23)
    m = build(Fm.fMRIVolumeEncoder3D, 46, dropout=0.3).eval()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm3d):
                mod.running_mean.copy_(seeded_randn(19, *mod.running_mean.shape) * 0.1)
                mod.running_var.copy_(1.0 + 0.2 * seeded_randn(20, *mod.running_var.shape).abs())
    x = seeded_randn(146, *shape)
    gy = seeded_randn(147, 3, 64)
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}
    with bf16_operands():
        out = RF.volume_encoder3d(sd, x, train=False)
        out.backward(gy)
    want = {k: v.grad for k, v in sd.items() if v.requires_grad and v.grad is not None}
    before = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    mg = m.cuda()
    y = mg(x.cuda())
    y.backward(gy.cuda())
    assert cos_min(y.detach().cpu(), out.detach()) >= 1 - COS_TOL
    w = _worst(mg.named_parameters(), want)
    assert w[1] <= 6e-2, w
    # d / d volume
    sd = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}
    xo = x.clone().requires_grad_(True)
    with bf16_operands(l1_as_gemm=True):
        out = RF.volume_encoder3d(sd, xo, train=False)
        out.backward(gy)
    want = {k: v.grad for k, v in sd.items() if v.requires_grad and v.grad is not None}
    mg.zero_grad(set_to_none=True)
    xg = x.cuda().requires_grad_(True)
    y2 = mg(xg)
    y2.backward(gy.cuda())
    assert cos_min(y2.detach().cpu(), out.detach()) >= 1 - COS_TOL
    assert xg.grad is not None and xg.grad.shape == x.shape and bool(torch.isfinite(xg.grad).all())
    assert rel_err(xg.grad.cpu(), xo.grad) <= 8e-2, rel_err(xg.grad.cpu(), xo.grad)
    w = _worst(mg.named_parameters(), want)
    assert w[1] <= 6e-2, w
    for k, v in before.items():
        assert torch.equal(mg.state_dict()[k].cpu(), v), k
    # dropout 0.3 in train mode vs the masked oracle (mask index: the floored pooled channels-last tensor)
    p = 0.3
    m = build(Fm.fMRIVolumeEncoder3D, 47, dropout=p).train()
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}
    x = seeded_randn(148, 4, 1, 19, 21, 23)
    gy = seeded_randn(149, 4, 64)
    mg = m.cuda()

    def run():
        yy = mg(x.cuda())
        yy.backward(gy.cuda())
        return yy
    y, seeds = _log_seeds(run)
    assert len(seeds) == 4, seeds
    with bf16_operands():
        want = volume_encoder_train_with_masks(sd, x, seeds, p)
        want.backward(gy)
    assert torch.equal((y == 0).cpu(), (want == 0))
    assert cos_min(y.detach().cpu(), want.detach()) >= 1 - COS_TOL, cos_min(y.detach().cpu(), want.detach())
    bad = [(n, rel_err(q.grad.cpu(), sd[n].grad)) for n, q in mg.named_parameters()
           if sd[n].grad is not None and sd[n].grad.norm() >= 1e-4 and rel_err(q.grad.cpu(), sd[n].grad) > 6e-2]
    assert not bad, bad


def _mni3_pairs(B, seed):
    from multimodal_eeg_fmri_amd.bridge_trainer import synthetic_pairs
    return synthetic_pairs(B, 16, 256, (61, 73, 61), seed=seed)


def test_trainer_at_mni_3mm():
    """BridgeTrainer on 61 x 73 x 61 volumes: three graph-replayed steps are bit-identical to the eager tape; one graph
    step from the initial weights matches the CPU oracle (loss 1e-3, gradients <= 6e-2 vs the bf16-operand oracle); a
    HostFeeder loop at B = 3 (a volume batch whose element count is not a multiple of 4: the staging takes its
    per-input path) equals train_step"""
    from multimodal_eeg_fmri_amd import ops
    from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer
    from test_trainer_gpu import _bn_cancelled, _oracle_step
    batches = [_mni3_pairs(4, 900 + i) for i in range(3)]

    def run(mode):
        ops.set_seed_epoch(None)
        torch.manual_seed(0)
        tr = BridgeTrainer(eeg_channels=16, dropout=0.0, lr=1e-3, mode=mode).train()
        losses = [tr.train_step(*batches[i])["loss"].clone() for i in range(3)]
        torch.cuda.synchronize()
        ops.set_seed_epoch(None)
        return torch.stack(losses), tr.bucket.p.detach().clone(), tr
    lm, pm, _ = run("manual")
    lg, pg, trg = run("graph")
    assert trg.capture_mode == "one graph"
    assert torch.isfinite(lm).all() and torch.equal(lm, lg) and torch.equal(pm, pg), (lm, lg)
    # one graph step from the initial weights vs the oracle
    ops.set_seed_epoch(None)
    torch.manual_seed(0)
    tr = BridgeTrainer(eeg_channels=16, dropout=0.0, lr=1e-3, mode="graph").train()
    eeg, fmri = batches[0]
    l32, _, _, _ = _oracle_step(tr, eeg, fmri, emulate=False)
    _, _, _, g16 = _oracle_step(tr, eeg, fmri, emulate=True)
    tr.grad_probe = torch.zeros_like(tr.bucket.g)
    out = tr.train_step(eeg, fmri)
    torch.cuda.synchronize()
    ops.set_seed_epoch(None)
    assert abs(out["loss"].item() - l32) <= 1e-3 * max(1.0, abs(l32)), (out["loss"].item(), l32)
    named = {}
    for pre, mod in (("e.", tr.eeg_encoder), ("f.", tr.fmri_encoder), ("h.", tr.head)):
        named.update({pre + k: v for k, v in mod.named_parameters()})
    base = tr.bucket.g.data_ptr()
    zero = _bn_cancelled(tr)
    worst, checked = ("", 0.0), 0
    for n, q in named.items():
        sink = getattr(q, "_mm_grad", None)
        if sink is None or n not in g16 or (n not in zero and g16[n].norm() < 1e-5):
            continue
        off = (sink.data_ptr() - base) // 4
        got = tr.grad_probe[off:off + q.numel()].cpu().view(g16[n].shape).double()
        if n in zero:
            e = (got.norm() / g16[n[:-len("bias")] + "weight"].double().norm()).item()
        else:
            e = ((got - g16[n].double()).norm() / g16[n].double().norm()).item()
        worst = max(worst, (n, e), key=lambda t: t[1])
        checked += 1
    assert checked >= 20, checked
    assert worst[1] <= 6e-2, worst
    # the host-fed loop at B = 3
    small = [_mni3_pairs(3, 950 + i) for i in range(3)]
    assert small[0][1].numel() % 4 != 0

    def run3(feeder):
        ops.set_seed_epoch(None)
        ops.set_dropout_seed(77)
        torch.manual_seed(0)
        t = BridgeTrainer(eeg_channels=16, dropout=0.2, lr=1e-3).train()
        losses = [t.train_step(*small[0])["loss"].clone()]
        if feeder:
            fd = t.host_feeder()
            hosts = [t.pack_host_batch(*small[i % 3]) for i in range(1, 4)]
            fd.upload(hosts[0])
            for i in range(3):
                if i + 1 < 3:
                    fd.upload(hosts[i + 1])
                losses.append(fd.step()["loss"].clone())
        else:
            for i in range(1, 4):
                losses.append(t.train_step(*small[i % 3])["loss"].clone())
        torch.cuda.synchronize()
        ops.set_seed_epoch(None)
        return torch.stack(losses), t.bucket.p.detach().clone()
    l0, p0 = run3(False)
    l1, p1 = run3(True)
    assert torch.isfinite(l0).all() and torch.equal(l0, l1) and torch.equal(p0, p1)


@pytest.mark.parametrize("dhw", [(3, 16, 16), (16, 2, 16), (16, 16, 1)])
def test_extents_below_four_are_rejected_before_any_launch(dhw, monkeypatch):
    """an axis shorter than 4 leaves the second pool empty: ValueError from the module (train, eval, d / d volume) and
    from BridgeTrainer.train_step, with no library call made"""
    from multimodal_eeg_fmri_amd import _hip as H
    from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer
    m = build(Fm.fMRIVolumeEncoder3D, 48).cuda()
    tr = BridgeTrainer(eeg_channels=16, dropout=0.0).train()
    x = torch.randn(2, 1, *dhw, device="cuda")
    eeg = torch.randn(2, 16, 256, device="cuda")
    torch.cuda.synchronize()
    calls = []
    monkeypatch.setattr(H, "call", lambda *a: calls.append(a[0]))
    for train in (True, False):
        m.train(train)
        with pytest.raises(ValueError, match=">= 4"):
            m(x)
    with pytest.raises(ValueError, match=">= 4"):
        m.eval()(x.clone().requires_grad_(True))
    with pytest.raises(ValueError, match=">= 4"):
        tr.train_step(eeg, x)
    assert calls == []
    monkeypatch.undo()
    # the C ABI refuses extents below 2 on its own
    hip = _hip()
    with pytest.raises(hip.HipLibraryError, match=">= 2"):
        hip.call("mm_conv3d_l1_gram", torch.zeros(1, device="cuda"), torch.zeros(32, 32, device="cuda", dtype=torch.bfloat16),
                 None, torch.zeros(32, 32, 32, device="cuda"), torch.zeros(32, 2, 32, device="cuda"), 1, 1, 4, 4)
