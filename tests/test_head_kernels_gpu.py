"""GPU: the fp32 row kernels of csrc/heads.hip, fusion.hip, losses.hip and power_front.hip (and the small layout / reduction
kernels next to them) against plain fp64 references of the same operation, computed on the CPU from the kernels' own operands.

  - both projection heads (mm_proj_heads_fwd / _bwd: Linear -> LayerNorm -> GELU(erf) -> Dropout -> F.normalize), every
    output and every gradient, across the backward's 32-row chunks (B > 32), all four NE = ceil(N / 64) instantiations, the
    forward's T = 4 / 2 / 1 lane groups, K % 4 != 0 (the scalar loop) and K = 1024 (HEAD_MAXK);
  - the STFT power front end (mm_stft_power) at every accepted nfft: the radix-2 FFT kernel (8 .. 256) and the direct DFT
    (512, 1024) with and without the frame-block split, into a channel window of a wider row;
  - the small fused tails of the V4 / Lite / fMRI models and the losses at one large order-1 shape each (their ragged
    shapes, grid-stride second trips, absent optional arguments, saturated inputs and out-of-range labels are in
    tests/test_fusion_loss_edges_gpu.py), and the elementwise / layout kernels at sizes past every thread and grid stride.

Dropout masks come from the host replica (oracle/dropout_replica.py: keep_scale); rates are exact binary fractions, so
the kernels' fp32 threshold and the replica's fp64 one are the same integer.  Each figure is a rel-L2 error
||got - want|| / ||want|| unless named otherwise;
bounds are 3x the worst case measured on the MI355X:

    proj heads   z 3.2e-7  nrm 1.2e-7  z1 2.9e-7  hn 2.9e-7  stat 6.7e-8          (B 1..100, N 48..256, K 64..1024)
                 dx 3.6e-7  dW 2.8e-7  db 3.3e-7  dgamma 3.6e-7  dbeta 3.0e-7     accumulated onto non-zero gradients
    stft power   FFT (nfft <= 256): rel-L2 1.8e-7, max error / peak 2.8e-7; DFT (512, 1024): 1.1e-6, 2.2e-6
    small linear y 1.4e-7  pre 1.0e-7  dx 5.8e-7 (N = 1000)  dW 6.2e-8  db 6.4e-8
    act f32      fwd 5.7e-8  bwd 1.4e-7
    learned fusion  fused 6.4e-8  weights 4.9e-8  df 6.3e-8  ddyn 2.1e-7  dlogits 3.1e-7  dtemp 5.1e-7
    softmax2 concat out 2.7e-8  da 2.6e-8  dc 3.2e-8  dpa / dpc 1.8e-9;  gate2 mix 3.5e-8 .. 4.7e-8, dg 1.6e-7
    attn 1x2     ctx 6.7e-8  attw 6.6e-8  dproj 1.0e-7;  attn 1xk ctx 7.7e-8  attw 5.6e-8  dp 1.1e-7
    weighted CE  loss 2.4e-6  dlogits 2.4e-6 (B = 1000 with class weights: one thread's serial fp32 sums)
    focal        loss 1.6e-7  per-sample 1.1e-7  dlogits 9.0e-8;  smoothed CE loss 9.0e-8  dlogits 1.2e-7
    meanpool     fp32 7.6e-8  bf16 input 4.5e-8;  colsum fp32 5.0e-8  bf16 4.8e-10

Where the answer is exact (layout kernels, drop_path, add / mul, bf16 copies of fp32 outputs, bytes outside an output
window, optional outputs left out, two runs of the same launch) exactness is asserted."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle.dropout_replica import keep_scale
from multimodal_eeg_fmri_amd.ops import ACC_GRAD, acc_decode
from test_kernels_gpu import _hip

pytestmark = pytest.mark.gpu

D64 = torch.float64


def _rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    den = want.norm().item()
    return (got - want).norm().item() / (den if den > 0 else 1.0)


class _Errs:
    """collects (name, measured, bound) and fails once with every figure, so one run reports all of them"""

    def __init__(self, tag):
        self.tag, self.rows = tag, []

    def __call__(self, name, err, bound):
        self.rows.append((name, err, bound))
        print(f"ERR {self.tag} {name} {err:.3e} (bound {bound:.0e})")

    def done(self):
        bad = [r for r in self.rows if not r[1] <= r[2]]
        assert not bad, f"{self.tag}: " + ", ".join(f"{n} {e:.3e} > {b:.0e}" for n, e, b in bad)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _cu(t):
    return t.contiguous().cuda()


def _gelu(z):
    return z * 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))


def _act64(z, act):
    return {"none": lambda t: t, "gelu": _gelu, "relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}[act](z)


# ---------------------------------------------------------------------------------------------------- projection heads
HEAD_EPS = 1e-5
HEAD_TOL = dict(z=9e-7, nrm=3.6e-7, z1=8.7e-7, hn=8.6e-7, stat=1.9e-7,                  # 3x the measured worst cases
                dx=1e-6, dW=8.2e-7, db=9.8e-7, dgamma=1e-6, dbeta=8.9e-7)


def _head_case(B, N, K_e, K_f, seed):
    g = _g(seed)
    side = []
    for K in (K_e, K_f):
        x = torch.randn(B, K, generator=g) * 0.7 + 0.3
        W = torch.randn(N, K, generator=g) / math.sqrt(K)
        b = torch.randn(N, generator=g) * 0.1
        gam = 0.5 + torch.rand(N, generator=g)
        bet = torch.randn(N, generator=g) * 0.2
        side.append((x, W, b, gam, bet))
    dz = torch.randn(B, 2 * N, generator=g)
    return side, dz


def _head_ref(side, dz, keeps):
    """fp64 Linear -> LayerNorm -> GELU(erf) -> dropout -> F.normalize of both heads and the autograd gradients of
    sum(z * dz); returns the forward tensors and {name: grad} per side"""
    N = side[0][1].shape[0]
    outs, grads = [], []
    for m, (params, keep) in enumerate(zip(side, keeps)):
        x, W, b, gam, bet = (t.double().clone().requires_grad_(True) for t in params)
        z1 = x @ W.t() + b
        mean = z1.mean(dim=1, keepdim=True)
        var = ((z1 - mean) ** 2).mean(dim=1, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + HEAD_EPS)
        hn = (z1 - mean) * rstd * gam + bet
        a = _gelu(hn) * keep.double()
        nr = a.norm(dim=1, keepdim=True).clamp_min(1e-12)
        z = a / nr
        (z * dz[:, m * N:(m + 1) * N].double()).sum().backward()
        outs.append(dict(z=z.detach(), nrm=nr.detach().squeeze(1), z1=z1.detach(), hn=hn.detach(),
                         stat=torch.cat([mean, rstd], dim=1).detach()))
        grads.append(dict(dx=x.grad, dW=W.grad, db=b.grad, dg=gam.grad, dbe=bet.grad))
    return outs, grads


def _head_fwd(hip, side, B, N, p, seeds, saved=True):
    (xe, We, be, ge, bee), (xf, Wf, bf, gf, bef) = [[_cu(t) for t in s] for s in side]
    z = torch.full((B, 2 * N), float("nan"), device="cuda")
    nrm = torch.full((2, B), float("nan"), device="cuda")
    z1 = hn = stat = None
    if saved:
        z1 = torch.full((2, B, N), float("nan"), device="cuda")
        hn = torch.full((2, B, N), float("nan"), device="cuda")
        stat = torch.full((2, B, 2), float("nan"), device="cuda")
    hip.call("mm_proj_heads_fwd", xe, We, be, ge, bee, side[0][0].shape[1], xf, Wf, bf, gf, bef, side[1][0].shape[1],
             z1, hn, stat, z, nrm, B, N, HEAD_EPS, p, seeds[0], seeds[1], None)
    return dict(z=z, nrm=nrm, z1=z1, hn=hn, stat=stat)


def _head_bwd(hip, side, fwd, dz, B, N, p, seeds, prefill, want=("dx", "dW", "db", "dg", "dbe")):
    """gradient outputs pre-filled from ``prefill`` (the accumulated ones) or NaN (dx, plain stores); names not in
    ``want`` are passed as null"""
    outs = []
    for m in range(2):
        K = side[m][0].shape[1]
        o = {}
        for name, shape in (("dx", (B, K)), ("dW", (N, K)), ("db", (N,)), ("dg", (N,)), ("dbe", (N,))):
            if name not in want:
                o[name] = None
            elif name == "dx":
                o[name] = torch.full(shape, float("nan"), device="cuda")
            else:
                o[name] = _cu(prefill[m][name].clone())
        outs.append(o)
    e, f = outs
    hip.call("mm_proj_heads_bwd", _cu(dz), fwd["z"], fwd["nrm"], fwd["hn"], fwd["z1"], fwd["stat"],
             _cu(side[0][0]), _cu(side[0][1]), _cu(side[0][3]), side[0][0].shape[1],
             _cu(side[1][0]), _cu(side[1][1]), _cu(side[1][3]), side[1][0].shape[1],
             e["dx"], e["dW"], e["db"], e["dg"], e["dbe"], f["dx"], f["dW"], f["db"], f["dg"], f["dbe"], B, N, p,
             seeds[0], seeds[1], None)
    return outs


@pytest.mark.parametrize("B,N,K_e,K_f,p", [
    (1, 48, 130, 64, 0.0),            # NE 1, forward T = 4, K % 4 != 0 on the EEG side; one row
    (31, 64, 1024, 130, 0.375),       # NE 1 at its top, HEAD_MAXK (the dx partial buffer full)
    (32, 128, 256, 1024, 0.0),        # NE 2, T = 2: one whole backward chunk
    (33, 160, 130, 512, 0.375),       # NE 3, T = 1: a second chunk of one row
    (64, 256, 1024, 96, 0.375),       # NE 4, two whole chunks
    (100, 256, 512, 130, 0.0),        # four chunks, the last one of 4 rows
    (100, 48, 1024, 1024, 0.375),     # NE 1 with four chunks, both sides at HEAD_MAXK
])
def test_proj_heads_match_fp64(B, N, K_e, K_f, p):
    hip = _hip()
    side, dz = _head_case(B, N, K_e, K_f, B * 1000 + N + K_e + K_f)
    seeds = (0x1234 + B, 0xBEEF + N)
    keeps = [keep_scale(s, B * N, p).view(B, N) for s in seeds]       # mask index b * N + n, per head its own seed
    ref, rgrad = _head_ref(side, dz, keeps)
    err = _Errs(f"proj_heads B{B} N{N} K{K_e}/{K_f} p{p}")

    fwd = _head_fwd(hip, side, B, N, p, seeds)
    z = fwd["z"].cpu()
    for m in range(2):
        err(f"z[{m}]", _rel(z[:, m * N:(m + 1) * N], ref[m]["z"]), HEAD_TOL["z"])
        err(f"nrm[{m}]", _rel(fwd["nrm"][m], ref[m]["nrm"]), HEAD_TOL["nrm"])
        err(f"z1[{m}]", _rel(fwd["z1"][m], ref[m]["z1"]), HEAD_TOL["z1"])
        err(f"hn[{m}]", _rel(fwd["hn"][m], ref[m]["hn"]), HEAD_TOL["hn"])
        err(f"stat[{m}]", _rel(fwd["stat"][m], ref[m]["stat"]), HEAD_TOL["stat"])
    if p > 0:                                   # a dropped element is exactly zero in z
        for m in range(2):
            assert torch.all(z[:, m * N:(m + 1) * N][keeps[m] == 0] == 0)
    # the saved tensors are optional: the embeddings do not depend on whether they are written
    fwd2 = _head_fwd(hip, side, B, N, p, seeds, saved=False)
    assert torch.equal(fwd2["z"], fwd["z"]) and torch.equal(fwd2["nrm"], fwd["nrm"])

    # backward: the accumulated gradients start from non-zero values, the kernel must add to them
    gp = _g(7 + B)
    prefill = [{k: torch.randn(rgrad[m][k].shape, generator=gp, dtype=D64).float() * rgrad[m][k].std().item()
                for k in ("dW", "db", "dg", "dbe")} for m in range(2)]
    got = _head_bwd(hip, side, fwd, dz, B, N, p, seeds, prefill)
    for m in range(2):
        err(f"dx[{m}]", _rel(got[m]["dx"], rgrad[m]["dx"]), HEAD_TOL["dx"])
        for k, name in (("dW", "dW"), ("db", "db"), ("dg", "dgamma"), ("dbe", "dbeta")):
            err(f"{name}[{m}]", _rel(got[m][k].cpu().double() - prefill[m][k].double(), rgrad[m][k]), HEAD_TOL[name])
    err.done()
    # bit-reproducible: a second launch gives the same bits
    again = _head_bwd(hip, side, fwd, dz, B, N, p, seeds, prefill)
    for m in range(2):
        for k in got[m]:
            assert torch.equal(again[m][k], got[m][k]), k
    # optional outputs left out change nothing else
    part = _head_bwd(hip, side, fwd, dz, B, N, p, seeds, prefill, want=("dW", "db"))
    solo = _head_bwd(hip, side, fwd, dz, B, N, p, seeds, prefill, want=("dx",))
    for m in range(2):
        assert torch.equal(part[m]["dW"], got[m]["dW"]) and torch.equal(part[m]["db"], got[m]["db"])
        assert torch.equal(solo[m]["dx"], got[m]["dx"])


def test_proj_heads_reject_out_of_range_shapes():
    hip = _hip()
    B = 2
    for N, K in ((257, 64), (64, 1025)):
        side, dz = _head_case(B, N, K, 64, 3)
        with pytest.raises(hip.HipLibraryError, match="proj_heads_fwd"):
            _head_fwd(hip, side, B, N, 0.0, (1, 2))
        fake = dict(z=torch.zeros(B, 2 * N, device="cuda"), nrm=torch.ones(2, B, device="cuda"),
                    z1=torch.zeros(2, B, N, device="cuda"), hn=torch.zeros(2, B, N, device="cuda"),
                    stat=torch.ones(2, B, 2, device="cuda"))
        prefill = [{k: torch.zeros(s) for k, s in (("dW", (N, side[m][0].shape[1])), ("db", (N,)), ("dg", (N,)), ("dbe", (N,)))}
                   for m in range(2)]
        with pytest.raises(hip.HipLibraryError, match="proj_heads_bwd"):
            _head_bwd(hip, side, fake, dz, B, N, 0.0, (1, 2), prefill)


# ---------------------------------------------------------------------------------------------------------------- STFT
def _stft_ref(x, nfft, hop):
    """fp64 torch.stft(center=True, reflect, periodic Hann) power, channels-last (B, frames, C, F)"""
    B, C, T = x.shape
    win = torch.hann_window(nfft, periodic=True, dtype=D64)
    s = torch.stft(x.double().reshape(B * C, T), nfft, hop_length=hop, window=win, center=True, pad_mode="reflect",
                   return_complex=True)
    P = s.real ** 2 + s.imag ** 2                                     # (B*C, F, frames)
    return P.view(B, C, nfft // 2 + 1, -1).permute(0, 3, 1, 2)


@pytest.mark.parametrize("B,C,T,nfft,hop", [
    (2, 3, 5, 8, 2),           # T just above nfft / 2: a frame reflects at both ends
    (2, 3, 40, 8, 4),
    (1, 4, 9, 16, 3),
    (2, 2, 100, 16, 8),
    (2, 5, 17, 32, 16),
    (3, 2, 1000, 32, 7),
    (2, 4, 33, 64, 32),
    (2, 8, 1024, 64, 32),      # the config-#5 scales
    (2, 3, 65, 128, 32),
    (1, 6, 1000, 128, 32),
    (2, 2, 129, 256, 64),
    (1, 3, 1500, 256, 100),
    (1, 2, 257, 512, 128),     # DFT kernel from here on; small B * C: the frame blocks split over the grid
    (1, 2, 8000, 512, 64),     # 126 frames: 8 workgroups per (b, c) walk two frame blocks each
    (2, 512, 600, 512, 128),   # B * C = 1024: one workgroup per (b, c)
    (1, 3, 513, 1024, 256),
    (1, 3, 5000, 1024, 100),
    (1, 1024, 1100, 1024, 512),
])
def test_stft_power_matches_fp64_stft(B, C, T, nfft, hop):
    hip = _hip()
    g = _g(nfft * 7 + T + C)
    x = torch.randn(B, C, T, generator=g) + 0.2 * torch.sin(torch.arange(T) * 0.3)
    Fb = nfft // 2 + 1
    frames = T // hop + 1
    off, tail = 5, 3
    tot = off + C * Fb + tail
    want = _stft_ref(x, nfft, hop)
    assert want.shape == (B, frames, C, Fb)
    # sentinels outside the window must survive; the window itself is fully written
    o32 = torch.full((B, frames, tot), -7.25, device="cuda")
    o16 = torch.full((B, frames, tot), -3.5, device="cuda").to(torch.bfloat16)
    hip.call("mm_stft_power", _cu(x), o16, o32, B, C, T, nfft, hop, off, tot)
    o32, o16 = o32.cpu(), o16.cpu()
    for o, s in ((o32, -7.25), (o16, -3.5)):
        assert torch.all(o[:, :, :off] == s) and torch.all(o[:, :, off + C * Fb:] == s)
    got = o32[:, :, off:off + C * Fb].reshape(B, frames, C, Fb)
    assert torch.equal(o16[:, :, off:off + C * Fb], o32[:, :, off:off + C * Fb].to(torch.bfloat16))
    fft = nfft <= 256
    err = _Errs(f"stft nfft{nfft} B{B} C{C} T{T} hop{hop}")
    err("rel-L2", _rel(got, want), 5e-7 if fft else 3e-6)
    err("max/peak", (got.double() - want).abs().max().item() / want.abs().max().item(), 8e-7 if fft else 6e-6)
    err.done()
    # the f32-only and bf16-only forms write the same values
    o32b = torch.full((B, frames, tot), -7.25, device="cuda")
    hip.call("mm_stft_power", _cu(x), None, o32b, B, C, T, nfft, hop, off, tot)
    o16b = torch.full((B, frames, tot), -3.5, device="cuda").to(torch.bfloat16)
    hip.call("mm_stft_power", _cu(x), o16b, None, B, C, T, nfft, hop, off, tot)
    assert torch.equal(o32b.cpu(), o32) and torch.equal(o16b.cpu(), o16)


# -------------------------------------------------------------------------------------------------------- small linear
SMALL_ACTS = ["none", "gelu", "relu", "tanh", "sigmoid"]


@pytest.mark.parametrize("N", [3, 256, 300, 1000])
@pytest.mark.parametrize("act", SMALL_ACTS)
def test_small_linear_fwd_bwd_match_fp64(N, act):
    from multimodal_eeg_fmri_amd.ops import ACT
    hip = _hip()
    B, K = 7, 200 if N != 300 else 1000
    g = _g(N * 10 + ACT[act])
    x = torch.randn(B, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g) * 0.3
    scale = 0.5 + torch.rand(N, generator=g)
    shift = torch.randn(N, generator=g) * 0.2
    err = _Errs(f"small_linear N{N} {act}")
    for folded, p in ((False, 0.0), (True, 0.0), (True, 0.25), (False, 0.25)):
        seed = 99 + N
        pre64 = x.double() @ W.double().t() + bias.double()
        if folded:
            pre64 = pre64 * scale.double() + shift.double()
        keep = keep_scale(seed, B * N, p).view(B, N).double()
        y64 = _act64(pre64, act) * keep
        y = torch.full((B, N), float("nan"), device="cuda")
        pre = torch.full((B, N), float("nan"), device="cuda")
        hip.call("mm_small_linear_fwd", _cu(x), _cu(W), _cu(bias), _cu(scale) if folded else None,
                 _cu(shift) if folded else None, y, pre, B, K, N, ACT[act], p, seed, None)
        tag = f"{'bn' if folded else 'plain'} p{p}"
        err(f"y {tag}", _rel(y, y64), 4e-7)
        err(f"pre {tag}", _rel(pre, pre64), 3e-7)
        if p > 0:
            assert torch.all(y.cpu()[keep == 0] == 0)
        y2 = torch.full((B, N), float("nan"), device="cuda")       # pre is optional
        hip.call("mm_small_linear_fwd", _cu(x), _cu(W), _cu(bias), _cu(scale) if folded else None,
                 _cu(shift) if folded else None, y2, None, B, K, N, ACT[act], p, seed, None)
        assert torch.equal(y2, y)
    # backward (dy already through act'): dx = dy W (stores), dW += dy^T x, db += colsum(dy)
    dy = torch.randn(B, N, generator=g)
    dW0 = torch.randn(N, K, generator=g) * 0.5
    db0 = torch.randn(N, generator=g) * 0.5
    dx = torch.full((B, K), float("nan"), device="cuda")
    dW, db = _cu(dW0.clone()), _cu(db0.clone())
    hip.call("mm_small_linear_bwd", _cu(dy), _cu(x), _cu(W), dx, dW, db, B, K, N)
    err("dx", _rel(dx, dy.double() @ W.double()), 1.5e-6)
    err("dW", _rel(dW.cpu().double() - dW0.double(), dy.double().t() @ x.double()), 1.5e-7)
    err("db", _rel(db.cpu().double() - db0.double(), dy.double().sum(0)), 1.5e-7)
    err.done()
    dW2 = _cu(dW0.clone())                          # dx and db are optional
    hip.call("mm_small_linear_bwd", _cu(dy), _cu(x), _cu(W), None, dW2, None, B, K, N)
    assert torch.equal(dW2, dW)


@pytest.mark.parametrize("act", SMALL_ACTS)
def test_act_f32_and_its_backward_match_fp64(act):
    from multimodal_eeg_fmri_amd.ops import ACT
    hip = _hip()
    n = 600_001                                      # past the 2048 x 256 grid stride
    g = _g(ACT[act] + 40)
    z = torch.randn(n, generator=g) * 3
    gr = torch.randn(n, generator=g)
    err = _Errs(f"act_f32 {act}")
    for p in (0.0, 0.25):
        seed = 4242
        keep = keep_scale(seed, n, p).double()
        y = torch.full((n,), float("nan"), device="cuda")
        hip.call("mm_act_f32", _cu(z), y, n, ACT[act], p, seed, None)
        err(f"fwd p{p}", _rel(y, _act64(z.double(), act) * keep), 1.5e-7)
        zr = z.double().requires_grad_(True)
        _act64(zr, act).backward(gr.double())
        out = torch.full((n,), float("nan"), device="cuda")
        hip.call("mm_act_bwd_f32", _cu(gr), _cu(z), out, n, ACT[act], p, seed, None)
        err(f"bwd p{p}", _rel(out, zr.grad * keep), 4e-7)
        out2 = torch.full((n,), float("nan"), device="cuda")         # z = null: the dropout mask alone
        hip.call("mm_act_bwd_f32", _cu(gr), None, out2, n, ACT[act], p, seed, None)
        assert torch.equal(out2.cpu(), gr * keep.float())
    err.done()


# ------------------------------------------------------------------------------------------------- fusion / mixing tails
@pytest.mark.parametrize("M", [2, 3])
def test_learned_fusion_fwd_bwd_match_fp64(M):
    hip = _hip()
    B, H = 100, 300                                  # the backward's 16 waves walk 7 rows each; 5 lane passes per row
    g = _g(M)
    feats = [torch.randn(B, H, generator=g) for _ in range(M)]
    dyn = torch.randn(B, M, generator=g) * 2
    logits = torch.randn(M, generator=g)
    temp = torch.tensor([0.7])
    dfused = torch.randn(B, H, generator=g)
    fr = [f.double().requires_grad_(True) for f in feats]
    dr, lr, tr = (t.double().requires_grad_(True) for t in (dyn, logits, temp))
    w = 0.5 * torch.softmax(lr / tr, 0).unsqueeze(0) + 0.5 * torch.softmax(dr / tr, 1)
    fused = sum(w[:, m:m + 1] * fr[m] for m in range(M))
    (fused * dfused.double()).sum().backward()
    err = _Errs(f"learned_fusion M{M}")
    fc = [_cu(f) for f in feats] + [None] * (3 - M)
    out = torch.full((B, H), float("nan"), device="cuda")
    wout = torch.full((B, M), float("nan"), device="cuda")
    hip.call("mm_learned_fusion", fc[0], fc[1], fc[2], _cu(dyn), _cu(logits), _cu(temp), out, wout, B, H, M)
    err("fused", _rel(out, fused), 1.5e-7)
    err("weights", _rel(wout, w), 1.4e-7)
    dfs = [torch.full((B, H), float("nan"), device="cuda") for _ in range(M)] + [None] * (3 - M)
    ddyn = torch.full((B, M), float("nan"), device="cuda")
    dl0, dt0 = torch.randn(M, generator=g), torch.randn(1, generator=g)
    dlog, dtemp = _cu(dl0.clone()), _cu(dt0.clone())
    hip.call("mm_learned_fusion_bwd", fc[0], fc[1], fc[2], _cu(dyn), _cu(logits), _cu(temp), _cu(dfused), dfs[0], dfs[1],
             dfs[2], ddyn, dlog, dtemp, B, H, M)
    for m in range(M):
        err(f"df{m}", _rel(dfs[m], fr[m].grad), 1.5e-7)
    err("ddyn", _rel(ddyn, dr.grad), 6e-7)
    err("dlogits", _rel(dlog.cpu().double() - dl0.double(), lr.grad), 9e-7)
    err("dtemp", _rel(dtemp.cpu().double() - dt0.double(), tr.grad), 1.5e-6)
    err.done()


def test_softmax2_concat_and_gate2_mix_match_fp64():
    hip = _hip()
    B, Ha, Hc = 1000, 64, 100
    g = _g(11)
    a, c = torch.randn(B, Ha, generator=g), torch.randn(B, Hc, generator=g)
    pa, pc = torch.tensor([0.3]), torch.tensor([-0.8])
    dout = torch.randn(B, Ha + Hc, generator=g)
    ar, cr, par, pcr = (t.double().requires_grad_(True) for t in (a, c, pa, pc))
    w = torch.softmax(torch.cat([par, pcr]), 0)
    ref = torch.cat([w[0] * ar, w[1] * cr], dim=1)
    (ref * dout.double()).sum().backward()
    err = _Errs("softmax2_concat / gate2_mix")
    out = torch.full((B, Ha + Hc), float("nan"), device="cuda")
    hip.call("mm_softmax2_concat", _cu(a), _cu(c), _cu(pa), _cu(pc), out, B, Ha, Hc)
    err("s2c out", _rel(out, ref), 8e-8)
    da, dc = torch.full((B, Ha), float("nan"), device="cuda"), torch.full((B, Hc), float("nan"), device="cuda")
    dpa, dpc = _cu(torch.tensor([0.25])), _cu(torch.tensor([-0.5]))
    hip.call("mm_softmax2_concat_bwd", _cu(dout), _cu(a), _cu(c), _cu(pa), _cu(pc), da, dc, dpa, dpc, B, Ha, Hc)
    err("s2c da", _rel(da, ar.grad), 7.5e-8)
    err("s2c dc", _rel(dc, cr.grad), 9e-8)
    err("s2c dpa", _rel(dpa.cpu().double() - 0.25, par.grad), 5e-9)
    err("s2c dpc", _rel(dpc.cpu().double() + 0.5, pcr.grad), 5e-9)
    # HybridFusionModule mix: gate = softmax(g[b]); comb = [gate0 erp + gate1 pw | conn * boost]
    H, boost = 300, 1.5
    gl = torch.randn(B, 2, generator=g) * 2
    erp, pw, conn = (torch.randn(B, H, generator=g) for _ in range(3))
    dcomb = torch.randn(B, 2 * H, generator=g)
    glr, er, pr, cnr = (t.double().requires_grad_(True) for t in (gl, erp, pw, conn))
    gate = torch.softmax(glr, 1)
    comb = torch.cat([gate[:, :1] * er + gate[:, 1:] * pr, cnr * boost], dim=1)
    (comb * dcomb.double()).sum().backward()
    cb = torch.full((B, 2 * H), float("nan"), device="cuda")
    gt = torch.full((B, 2), float("nan"), device="cuda")
    hip.call("mm_gate2_mix", _cu(gl), _cu(erp), _cu(pw), _cu(conn), cb, gt, B, H, boost)
    err("mix comb", _rel(cb, comb), 1e-7)
    err("mix gate", _rel(gt, gate), 1.1e-7)
    outs = [torch.full((B, H), float("nan"), device="cuda") for _ in range(3)] + [torch.full((B, 2), float("nan"), device="cuda")]
    hip.call("mm_gate2_mix_bwd", _cu(dcomb), _cu(gl), _cu(erp), _cu(pw), *outs, B, H, boost)
    for name, o, w_ in zip(("derp", "dpw", "dconn", "dg"), outs, (er.grad, pr.grad, cnr.grad, glr.grad)):
        err(f"mix {name}", _rel(o, w_), dict(derp=1.3e-7, dpw=1.3e-7, dconn=8e-8, dg=4.5e-7)[name])
    err.done()


def _mha_1xk_ref(ps, E, nhead, keep):
    """one query (token 0's q) over K key/value tokens, per head; ps = [(B, 3E)] fp64 leaves; keep (B, nhead, K)"""
    B = ps[0].shape[0]
    dh = E // nhead
    q = ps[0][:, :E].view(B, nhead, dh)
    k = torch.stack([p[:, E:2 * E].view(B, nhead, dh) for p in ps], dim=2)          # (B, h, K, dh)
    v = torch.stack([p[:, 2 * E:].view(B, nhead, dh) for p in ps], dim=2)
    pr = torch.softmax((q.unsqueeze(2) * k).sum(-1) / math.sqrt(dh), dim=-1)        # (B, h, K)
    ctx = ((pr * keep).unsqueeze(-1) * v).sum(2).reshape(B, E)
    return ctx, pr.mean(1)


@pytest.mark.parametrize("E,nhead", [(128, 16), (256, 2), (64, 4)])
def test_attn_1x2_matches_fp64(E, nhead):
    hip = _hip()
    B = 300
    g = _g(E + nhead)
    pe, pf = torch.randn(B, 3 * E, generator=g), torch.randn(B, 3 * E, generator=g)
    dctx = torch.randn(B, E, generator=g)
    err = _Errs(f"attn_1x2 E{E} h{nhead}")
    ctx0, attw0 = _mha_1xk_ref([pe.double(), pf.double()], E, nhead, torch.ones(B, nhead, 2, dtype=D64))
    ctx = torch.full((B, E), float("nan"), device="cuda")
    attw = torch.full((B, 2), float("nan"), device="cuda")
    hip.call("mm_attn_1x2", _cu(pe), _cu(pf), ctx, attw, B, E, nhead)
    err("ctx", _rel(ctx, ctx0), 1.8e-7)
    err("attw", _rel(attw, attw0), 1.9e-7)
    for p in (0.0, 0.25):
        seed = 515
        keep = keep_scale(seed, B * nhead * 2, p).view(B, nhead, 2).double()        # index (b * nhead + h) * 2 + j
        per, pfr = pe.double().requires_grad_(True), pf.double().requires_grad_(True)
        cref, aref = _mha_1xk_ref([per, pfr], E, nhead, keep)
        (cref * dctx.double()).sum().backward()
        ctx = torch.full((B, E), float("nan"), device="cuda")
        attw = torch.full((B, 2), float("nan"), device="cuda")
        hip.call("mm_attn_1x2_train", _cu(pe), _cu(pf), None, ctx, attw, None, None, B, E, nhead, p, seed, None, 0)
        err(f"train ctx p{p}", _rel(ctx, cref), 2e-7)
        err(f"train attw p{p}", _rel(attw, aref), 1.9e-7)
        dpe = torch.full((B, 3 * E), float("nan"), device="cuda")
        dpf = torch.full((B, 3 * E), float("nan"), device="cuda")
        hip.call("mm_attn_1x2_train", _cu(pe), _cu(pf), _cu(dctx), None, None, dpe, dpf, B, E, nhead, p, seed, None, 1)
        err(f"dproj_e p{p}", _rel(dpe, per.grad), 3e-7)
        err(f"dproj_f p{p}", _rel(dpf, pfr.grad), 2.7e-7)
        assert torch.all(dpf[:, :E] == 0)                                            # the fMRI token's q is unused
    err.done()


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_attn_1xk_matches_fp64(K, p):
    hip = _hip()
    B, E, nhead = 300, 128, 8
    g = _g(K * 10 + int(p * 4))
    ps = [torch.randn(B, 3 * E, generator=g) for _ in range(K)]
    dctx = torch.randn(B, E, generator=g)
    seed = 77 + K
    keep = keep_scale(seed, B * nhead * K, p).view(B, nhead, K).double()            # index (b * nhead + h) * K + j
    pr = [t.double().requires_grad_(True) for t in ps]
    cref, aref = _mha_1xk_ref(pr, E, nhead, keep)
    (cref * dctx.double()).sum().backward()
    pc = [_cu(t) for t in ps] + [None] * (4 - K)
    err = _Errs(f"attn_1xk K{K} p{p}")
    ctx = torch.full((B, E), float("nan"), device="cuda")
    attw = torch.full((B, K), float("nan"), device="cuda")
    hip.call("mm_attn_1xk", *pc, K, None, ctx, attw, None, None, None, None, B, E, nhead, p, seed, None, 0)
    err("ctx", _rel(ctx, cref), 2.3e-7)
    err("attw", _rel(attw, aref), 1.6e-7)
    dps = [torch.full((B, 3 * E), float("nan"), device="cuda") for _ in range(K)] + [None] * (4 - K)
    hip.call("mm_attn_1xk", *pc, K, _cu(dctx), None, None, *dps, B, E, nhead, p, seed, None, 1)
    for j in range(K):
        err(f"dp{j}", _rel(dps[j], pr[j].grad), 3e-7)
        if j:
            assert torch.all(dps[j][:, :E] == 0)
    err.done()


def test_attn_1xk_and_1x2_subtract_the_maximum_at_large_scores():
    """projections x 8: scores q k / sqrt(dh) of std 64 nats (every case above: order 1, where exp needs no maximum subtracted).
    The absolute bounds above assume scores of order 1; here each quantity is held to 16 x e32, e32 = the rel-L2 error of
    the same formula in plain fp32 torch on the CPU on the same inputs (test_norm_passes_gpu.py)."""
    hip = _hip()
    B, E, nhead, p = 300, 128, 8, 0.25
    dh = E // nhead
    g = _g(4242)
    ps4 = [8.0 * torch.randn(B, 3 * E, generator=g) for _ in range(4)]
    dctx = torch.randn(B, E, generator=g)
    rows = []

    def refs(ps, keep):
        res = []
        for dt in (D64, torch.float32):
            leaves = [t.clone().to(dt).requires_grad_(True) for t in ps]
            ctx, attw = _mha_1xk_ref(leaves, E, nhead, keep.to(dt))
            (ctx * dctx.to(dt)).sum().backward()
            res.append([ctx.detach(), attw.detach()] + [t.grad for t in leaves])
        return res

    for K, ps, seed in ((4, ps4, 81), (2, ps4[:2], 515)):
        keep = keep_scale(seed, B * nhead * K, p).view(B, nhead, K)
        want, cpu32 = refs(ps, keep)
        q = ps[0][:, :E].view(B, nhead, 1, dh).double()
        k = torch.stack([t[:, E:2 * E].view(B, nhead, dh) for t in ps], dim=2).double()
        assert ((q * k).sum(-1) / math.sqrt(dh)).abs().max().item() > 100.0
        ctx = torch.full((B, E), float("nan"), device="cuda")
        attw = torch.full((B, K), float("nan"), device="cuda")
        dps = [torch.full((B, 3 * E), float("nan"), device="cuda") for _ in range(K)]
        if K == 4:
            pc = [_cu(t) for t in ps]
            hip.call("mm_attn_1xk", *pc, K, None, ctx, attw, None, None, None, None, B, E, nhead, p, seed, None, 0)
            hip.call("mm_attn_1xk", *pc, K, _cu(dctx), None, None, *dps, B, E, nhead, p, seed, None, 1)
        else:
            hip.call("mm_attn_1x2_train", _cu(ps[0]), _cu(ps[1]), None, ctx, attw, None, None, B, E, nhead, p, seed, None, 0)
            hip.call("mm_attn_1x2_train", _cu(ps[0]), _cu(ps[1]), _cu(dctx), None, None, *dps, B, E, nhead, p, seed, None, 1)
        names = [f"K{K} ctx", f"K{K} attw"] + [f"K{K} dp{j}" for j in range(K)]
        for name, a, w, c32 in zip(names, [ctx, attw] + dps, want, cpu32):
            rows.append((name, _rel(a, w), 16 * _rel(c32, w), bool(torch.isfinite(a).all())))
            print(f"ERR attn_1xk/1x2 large scores {name} {rows[-1][1]:.3e} (bound {rows[-1][2]:.3e})")
    bad = [r for r in rows if not (r[3] and r[1] <= r[2])]
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------- losses
def _targets(B, C, g):
    return torch.randint(0, C, (B,), generator=g, dtype=torch.int64)


@pytest.mark.parametrize("B,C", [(5, 3), (1000, 7)])
@pytest.mark.parametrize("weighted", [False, True])
def test_weighted_ce_matches_fp64(B, C, weighted):
    hip = _hip()
    g = _g(B + C + weighted)
    z, t = torch.randn(B, C, generator=g) * 2, _targets(B, C, g)
    cw = 0.2 + torch.rand(C, generator=g) if weighted else None
    zr = z.double().requires_grad_(True)
    loss = F.cross_entropy(zr, t, weight=cw.double() if weighted else None)
    loss.backward()
    out = _cu(torch.tensor([0.75]))
    dl = torch.full((B, C), float("nan"), device="cuda")
    hip.call("mm_weighted_ce", _cu(z), _cu(t), _cu(cw) if weighted else None, out, dl, B, C)
    err = _Errs(f"weighted_ce B{B} C{C} w{weighted}")
    err("loss", abs(out.item() - 0.75 - loss.item()) / abs(loss.item()), 7e-6)
    err("dlogits", _rel(dl, zr.grad), 7e-6)
    err.done()


@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0])
@pytest.mark.parametrize("B", [6, 1000])
def test_focal_loss_matches_fp64(gamma, B):
    hip = _hip()
    C, alpha, scale = 5, 0.8, 1.0 / B
    g = _g(B + int(gamma * 10))
    z, t = torch.randn(B, C, generator=g) * 2, _targets(B, C, g)
    z[0, t[0]] = 30.0                                # a confident row: 1 - pt ~ 1e-13 (fp32: 0 -> the q <= 0 branch)
    zr = z.double().requires_grad_(True)
    ce = F.cross_entropy(zr, t, reduction="none")
    fl = alpha * (1 - torch.exp(-ce)) ** gamma * ce
    fl.sum().backward()
    out = _cu(torch.tensor([-0.5]))
    per = torch.full((B,), float("nan"), device="cuda")
    dl = torch.full((B, C), float("nan"), device="cuda")
    hip.call("mm_focal_loss", _cu(z), _cu(t), out, per, dl, B, C, alpha, gamma, scale)
    err = _Errs(f"focal gamma{gamma} B{B}")
    want = scale * fl.sum().item()
    err("loss", abs(out.item() + 0.5 - want) / abs(want), 4.5e-7)
    err("per_sample", _rel(per, fl), 3e-7)
    err("dlogits", _rel(dl, zr.grad), 2.5e-7)
    err.done()
    out2 = _cu(torch.tensor([-0.5]))                 # per-sample and the gradient are optional
    hip.call("mm_focal_loss", _cu(z), _cu(t), out2, None, None, B, C, alpha, gamma, scale)
    assert torch.equal(out2, out)


@pytest.mark.parametrize("B,C", [(9, 4), (1000, 11)])
def test_smoothed_ce_matches_fp64(B, C):
    hip = _hip()
    s = 0.1
    g = _g(B * C)
    z, t = torch.randn(B, C, generator=g) * 2, _targets(B, C, g)
    zr = z.double().requires_grad_(True)
    logp = torch.log_softmax(zr, 1)
    loss = ((1 - s) * -logp.gather(1, t[:, None]).squeeze(1) + s * -logp.mean(1)).mean()
    loss.backward()
    out = _cu(torch.tensor([0.125]))
    dl = torch.full((B, C), float("nan"), device="cuda")
    hip.call("mm_smoothed_ce", _cu(z), _cu(t), out, dl, B, C, s)
    err = _Errs(f"smoothed_ce B{B} C{C}")
    err("loss", abs(out.item() - 0.125 - loss.item()) / abs(loss.item()), 2.5e-7)
    err("dlogits", _rel(dl, zr.grad), 3e-7)
    err.done()


# ----------------------------------------------------------------------------------------------- elementwise / layout
def test_drop_path_add_mul_are_exact():
    hip = _hip()
    B, inner = 1000, 601                             # 601 000 elements: past the 2048 x 256 grid stride
    g = _g(5)
    x, y = torch.randn(B, inner, generator=g), torch.randn(B, inner, generator=g)
    for p in (0.0, 0.25):
        out = torch.full((B, inner), float("nan"), device="cuda")
        hip.call("mm_drop_path", _cu(x), out, B, inner, p, 31337, None)
        keep = keep_scale(31337, B, p)                # one draw per sample
        assert torch.equal(out.cpu(), x * keep.view(B, 1))
        if p:
            assert 0 < int((keep == 0).sum()) < B
    n = B * inner
    o = torch.full((n,), float("nan"), device="cuda")
    hip.call("mm_add_f32", _cu(x.view(-1)), _cu(y.view(-1)), o, n)
    assert torch.equal(o.cpu(), (x + y).view(-1))
    hip.call("mm_mul_f32", _cu(x.view(-1)), _cu(y.view(-1)), o, n)
    assert torch.equal(o.cpu(), (x * y).view(-1))


def test_layout_packers_are_exact():
    hip = _hip()
    g = _g(6)
    B, C, T, Cp = 3, 37, 70, 48                      # ragged 32 x 32 transpose tiles in both directions
    gb = torch.randn(B, T, Cp, generator=g).to(torch.bfloat16)
    dx = torch.full((B, C, T), float("nan"), device="cuda")
    hip.call("mm_unpack_ntc_f32", _cu(gb), dx, B, C, T, Cp)
    assert torch.equal(dx.cpu(), gb.float()[:, :, :C].transpose(1, 2))
    nvox, Cp = 600_001, 16                           # 1.2 M 16-byte groups: the 4096-workgroup grid loops
    x = torch.randn(nvox, generator=g)
    y = torch.full((nvox, Cp), 5.0, device="cuda").to(torch.bfloat16)
    hip.call("mm_pack_volume_bf16", _cu(x), y, nvox, Cp)
    want = torch.zeros(nvox, Cp, dtype=torch.bfloat16)
    want[:, 0] = x.to(torch.bfloat16)
    assert torch.equal(y.cpu(), want)


@pytest.mark.parametrize("B,L,D", [(3, 1000, 100), (2, 7, 64), (1, 129, 300)])
def test_meanpool_matches_fp64(B, L, D):
    hip = _hip()
    g = _g(B * L + D)
    x = torch.randn(B, L, D, generator=g) + 0.5
    o32 = torch.full((B, D), float("nan"), device="cuda")
    o16 = torch.full((B, D), float("nan"), device="cuda").to(torch.bfloat16)
    hip.call("mm_meanpool_fwd", _cu(x), o32, o16, B, L, D)
    err = _Errs(f"meanpool B{B} L{L} D{D}")
    err("fwd", _rel(o32, x.double().mean(1)), 2e-7)
    assert torch.equal(o16.cpu(), o32.cpu().to(torch.bfloat16))
    gr = torch.randn(B, D, generator=g)
    dx = torch.full((B, L, D), float("nan"), device="cuda")
    hip.call("mm_meanpool_bwd", _cu(gr), dx, B, L, D)
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(L), dtype=torch.float32)
    assert torch.equal(dx.cpu(), (gr * inv).unsqueeze(1).expand(B, L, D))
    xb = x.to(torch.bfloat16)                        # the Lite encoders' bf16 form
    o = torch.full((B, D), float("nan"), device="cuda")
    hip.call("mm_meanpool_bf16", _cu(xb), o, B, L, D)
    err("bf16", _rel(o, xb.double().mean(1)), 1.3e-7)
    err.done()


@pytest.mark.parametrize("M,N", [(5000, 300), (37, 64), (100, 130)])
def test_colsum_matches_fp64(M, N):
    hip = _hip()
    g = _g(M + N)
    a = torch.randn(M, N, generator=g) + 0.25
    ab = a.to(torch.bfloat16)
    err = _Errs(f"colsum M{M} N{N}")
    for name, args, want in (("f32", (None, _cu(a)), a.double().sum(0)), ("bf16", (_cu(ab), None), ab.double().sum(0))):
        ws = torch.zeros(32, N, device="cuda")
        hip.call("mm_colsum", *args, ws, M, N)
        err(name, _rel(acc_decode(ws, ACC_GRAD), want), 1.4e-7 if name == "f32" else 1.4e-9)
    err.done()


def test_prep_many_equals_one_prep_conv_weight_per_tensor():
    """mm_prep_many (the batched weight-image launch without the arena clear) == mm_prep_conv_weight per tensor, bit for
    bit; 66 descriptors split into tables of 64, one without a data-gradient image"""
    import ctypes
    import struct
    from test_kernels_gpu import _cpad
    hip = _hip()
    g = _g(12)
    shapes = [(128, 64, 27), (64, 7, 7), (32, 1, 27)] + [(24, 40, 3)] * 63
    keep, raw, pairs = [], [], []
    for i, (cout, cin, k) in enumerate(shapes):
        cinp, coutp = _cpad(cin), _cpad(cout)
        dgrad = i != 1
        w = torch.randn(cout, cin, k, generator=g).cuda()
        wf_a = torch.empty(cout, k, cinp, dtype=torch.bfloat16, device="cuda")
        wd_a = torch.empty(cinp, k, coutp, dtype=torch.bfloat16, device="cuda") if dgrad else None
        hip.call("mm_prep_conv_weight", w, wf_a, wd_a, cout, cin, k, cinp, coutp if dgrad else 0)
        wf_b = torch.full_like(wf_a, float("nan"))
        wd_b = torch.full_like(wd_a, float("nan")) if dgrad else None
        raw.append(struct.pack("<QQQiiiiii", w.data_ptr(), wf_b.data_ptr(), wd_b.data_ptr() if dgrad else 0, cout, cin, k,
                               cinp, coutp if dgrad else 0, 0))
        keep.append(w)
        pairs.append((wf_a, wf_b))
        if dgrad:
            pairs.append((wd_a, wd_b))
    buf = b"".join(raw)
    host = ctypes.create_string_buffer(buf, len(buf))
    hip.call("mm_prep_many", ctypes.addressof(host), len(shapes))
    torch.cuda.synchronize()
    for a, b in pairs:
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
