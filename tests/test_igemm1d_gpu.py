"""GPU: the 1-D implicit-GEMM family of csrc/igemm1d*.hip (every nn.Conv1d and nn.Linear on the HIP path) against plain fp64
references of the same operation, computed on the CPU from the kernels' own operands: the packed bf16 activations and the
bf16 weight images that mm_prep_conv_weight returns.

  - the forward main loop in every reachable (tile, K-chunk) cell of conv1d_dispatch, taps 1 .. 9 (even tap counts at two
    pads), T in {1, 31, 33, 64, 65, ragged}, Cout in {4, 12, 20, 48, 132, 384}, Cin in {16, 32, 96, 128, 1088}, > 512 row
    tiles;
  - the generic epilogue (include/mmeeg_hip.h: v = acc * scale + shift, stats, out_pre, act'(gradz), act, dropout, residual
    and pe, max over pairs) one step at a time and in the combinations the models use, on the default dispatch and with
    MM_EPI_GENERIC=1, and split-K with the whole conv-block epilogue;
  - the data gradient (forward kernel on the flipped image, mm_unpack_ntc_f32) and mm_conv1d_dgrad_bn_reduce;
  - the weight gradient (mm_conv1d_wgrad at taps 1 / 3 / 5 / 7 in both stride layouts, ragged tiles, sample groups;
    mm_conv1d_wgrad_many over > 12 problems) with dbias;
  - the fused Linear forms (LayerNorm forward / backward, second GEMM, mean over rows, BatchNorm-backward reduce).

Dropout masks come from the host replica (oracle/dropout_replica.py: keep_scale); rates are binary fractions, so the kernels'
fp32 threshold and the replica's are the same integer.  Each figure is a rel-L2 error ||got - want|| / ||want||, "peak" is
max |got - want| / max |want|; bounds are 3x the worst case measured on the MI355X:

    forward      fp32 out 5.4e-7 (k 9 over 1 088 channels, Cout 4), peak 1.2e-6; 3.3e-8 .. 1e-7 elsewhere
    epilogue     fp32 out 1.4e-7, peak 5.3e-7 (GELU' x tanh); bf16-only outputs 1.7e-3 (bf16 rounding); stats 6.0e-8
    split-K      fp32 out 2.2e-7, stats 6.0e-8
    dgrad        fp32 dX 1.1e-7; unpacked bf16 dX 1.7e-3;  dgrad + BN reduce: bf16 d(out) 1.7e-3, sums 1.3e-7
    wgrad        slot sums 1.2e-7 (both layouts, scatter, grouped launch), dbias 2.8e-8
    Linear fwd   out 6.0e-8, LN stat 3.8e-8, LN rows (bf16) 1.7e-3, second GEMM (bf16) 1.7e-3, row means 8.1e-8
    Linear bwd   dX 8.5e-8, masked bf16 dX 1.7e-3, dgamma / dbeta 1.2e-7, second GEMM (bf16) 1.7e-3, BN sums 1.2e-7

238 tests, references included, take 4 s of pytest time on the MI355X.

Where the answer is exact it is asserted exactly: a bf16 output equals bf16(fp32 output) of the same launch, out_pre equals
bf16(v) of a launch that stores v, dropped positions hold exactly the residual, padded channels of a data gradient are 0,
bytes past an output (NaN-filled) are untouched, weight-gradient slots are all written (and nothing else), two runs give
the same bits."""
import ctypes
import math
import struct

import pytest
import torch

from oracle.dropout_replica import keep_scale
from multimodal_eeg_fmri_amd.ops import ACC_GRAD, ACC_STAT, acc_decode
from test_kernels_gpu import _cpad, _hip

pytestmark = pytest.mark.gpu

D64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
GUARD = 256                              # NaN-filled elements behind every output: must stay NaN

# 3x the worst cases measured on the MI355X (module docstring)
TOL = dict(fwd=1.6e-6, fwd_peak=3.5e-6, epi=4.1e-7, epi_peak=1.6e-6, epi_bf16=5.2e-3, stats=1.8e-7, splitk=6.5e-7,
           dgrad=3.2e-7, dgrad_bf16=5.1e-3, bnred_dx=5.1e-3, bnred=3.9e-7,
           wgrad=3.7e-7, dbias=8.4e-8, lin=1.8e-7, lin_stat=1.2e-7, lin_h=5.1e-3, lin_out2=5.1e-3, lin_pool=2.5e-7,
           lnb_dx=2.6e-7, lnb_dxb=5.1e-3, lnb_dgb=3.6e-7, lnb_do=5.1e-3, lnb_sums=3.6e-7)


def _rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    den = want.norm().item()
    return (got - want).norm().item() / (den if den > 0 else 1.0)


def _peak(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    den = want.abs().max().item()
    return (got - want).abs().max().item() / (den if den > 0 else 1.0)


class _Errs:
    """collects (name, measured, bound) and fails once with every figure, so one run reports all of them"""

    def __init__(self, tag):
        self.tag, self.rows = tag, []

    def __call__(self, name, err, bound=None):
        bound = TOL[name] if bound is None else bound
        self.rows.append((name, err, bound))
        print(f"ERR {self.tag} {name} {err:.3e} (bound {bound:.1e})")

    def done(self):
        bad = [r for r in self.rows if not r[1] <= r[2]]
        assert not bad, f"{self.tag}: " + ", ".join(f"{n} {e:.3e} > {b:.1e}" for n, e, b in bad)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32) if t.dtype == F32 else t


def _same(a, b):
    return torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _nanbuf(n, dtype):
    return torch.full((n + GUARD,), float("nan"), dtype=dtype, device="cuda")


def _take(buf, n, shape, what):
    buf = buf.cpu()
    assert torch.isnan(buf[n:].float()).all(), f"{what}: bytes past the output were written"
    return buf[:n].view(shape)


def _gelu(z):
    return z * 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))


def _act64(z, code):
    return {0: lambda t: t, 1: _gelu, 2: torch.relu, 3: torch.tanh, 4: torch.sigmoid}[code](z)


def _dact64(z, code):
    if code == 1:
        return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    if code == 2:
        return (z > 0).double()
    if code == 3:
        return 1.0 - torch.tanh(z) ** 2
    if code == 4:
        s = torch.sigmoid(z)
        return s * (1.0 - s)
    return torch.ones_like(z)


def _keep(seed, shape, p):
    """the kernels' dropout multiplier (fp32 1 / (1 - p) or 0) over the flat index of ``shape``, as fp64"""
    n = 1
    for s in shape:
        n *= s
    return keep_scale(seed, n, p).view(*shape).double()


def _wimg(hip, w, cinp, coutp=None):
    """w (Cout, Cin, k) fp32 -> forward image (Cout, k, cinp) bf16 [, data-gradient image (cinp, k, coutp) bf16] on the GPU"""
    cout, cin, k = w.shape
    wf = torch.empty(cout, k, cinp, dtype=BF16, device="cuda")
    wd = torch.empty(cinp, k, coutp, dtype=BF16, device="cuda") if coutp else None
    hip.call("mm_prep_conv_weight", w.contiguous().cuda(), wf, wd, cout, cin, k, cinp, coutp or 0)
    return wf, wd


def _conv64(x, W, pad):
    """x (B, T, C), W (N, k, C) -> y[b, t, n] = sum_{tap, c} x[b, t + tap - pad, c] W[n, tap, c], fp64"""
    x, W = x.double(), W.double()
    B, T, C = x.shape
    N, k, _ = W.shape
    xp = torch.zeros(B, T + k - 1, C, dtype=D64)
    xp[:, pad:pad + T] = x
    y = torch.zeros(B, T, N, dtype=D64)
    for tap in range(k):
        y += xp[:, tap:tap + T] @ W[:, tap].t()
    return y


# ------------------------------------------------------------------------------------------------ dispatch mirror
TILES = ("64x64", "32x128", "64x128")
KCTS = (16, 32, 64, 128)


def fwd_cell(B, T, Cin, Cout, taps):
    """the (tile, K-chunk width) that conv1d_dispatch (csrc/igemm1d.hip) picks for mm_conv1d_fwd: KCT 128 for a Linear
    (taps 1) with Cin % 128 == 0, else the largest of 64 / 32 / 16 dividing Cin; the 64 x 64 tile for k > 1 convolutions
    and Cout <= 64, else 32 x 128 while B * ceil(T / 64) * ceil(Cout / 128) <= 512 and 64 x 128 beyond.  It labels and
    picks the test shapes; nothing here asserts what the library does."""
    kct = 128 if taps == 1 and Cin % 128 == 0 else 64 if Cin % 64 == 0 else 32 if Cin % 32 == 0 else 16
    if Cout <= 64 or taps > 1:
        return "64x64", kct
    if B * (-(-T // 64)) * (-(-Cout // 128)) <= 512:
        return "32x128", kct
    return "64x128", kct


# every (tile, KCT) conv1d_dispatch can reach: the 64 x 64 tile takes KCT 128 only for taps 1 with Cout <= 64, the two
# 128-wide tiles only run taps 1
REACHABLE_CELLS = [(t, k) for t in TILES for k in KCTS]

# (B, T, Cin, Cout, taps, pad)
FWD_CASES = [
    # 64 x 64: Linear cells, narrow outputs
    (2, 33, 16, 4, 1, 0), (3, 65, 32, 12, 1, 0), (2, 31, 1088, 20, 1, 0), (2, 64, 128, 48, 1, 0), (5, 1, 96, 64, 1, 0),
    # 64 x 64: taps 2 .. 9, even tap counts at two pads
    (2, 100, 16, 48, 2, 0), (2, 65, 32, 20, 2, 1),
    (2, 64, 96, 48, 3, 1), (1, 33, 128, 12, 3, 0),
    (2, 31, 128, 132, 4, 1), (1, 1, 16, 384, 4, 2),
    (2, 130, 1088, 48, 5, 2), (3, 64, 32, 4, 5, 4),
    (2, 70, 16, 20, 6, 2), (1, 65, 96, 132, 6, 5),
    (2, 200, 128, 64, 7, 3), (1, 1, 32, 12, 7, 6),
    (2, 33, 16, 48, 8, 0), (1, 100, 128, 20, 8, 3),
    (2, 64, 32, 132, 9, 4), (1, 31, 1088, 4, 9, 8),
    # 32 x 128 (taps 1, Cout > 64, <= 512 row x column tiles), 4-column remainders
    (3, 1, 16, 132, 1, 0), (2, 65, 96, 384, 1, 0), (1, 33, 1088, 132, 1, 0), (2, 31, 128, 384, 1, 0),
    # 64 x 128 (> 512 tiles)
    (520, 64, 16, 72, 1, 0), (3, 11000, 32, 132, 1, 0), (257, 64, 192, 132, 1, 0), (171, 64, 128, 384, 1, 0),
    (1030, 1, 16, 132, 1, 0),
]


def _fwd_id(c):
    B, T, Cin, Cout, k, pad = c
    tile, kct = fwd_cell(B, T, Cin, Cout, k)
    return f"{tile}-kct{kct}-B{B}-T{T}-Cin{Cin}-Cout{Cout}-k{k}p{pad}"


def _launch(hip, xg, wf, B, T, Cin, Cout, taps, pad, o, splitk=0):
    """one mm_conv1d_fwd (or mm_conv1d_fwd_splitk) into NaN-guarded outputs; o = epilogue operands (GPU tensors) and
    switches -> {f32, bf16, pre (CPU, guard checked), stats (fp64 sums), stats_raw (the workspace words)}"""
    pool = o.get("pool", 1)
    To = T // pool
    n_out, n_pre = B * To * Cout, B * T * Cout
    of = _nanbuf(n_out, F32) if o.get("f32", True) else None
    ob = _nanbuf(n_out, BF16) if o.get("bf16", True) else None
    op = _nanbuf(n_pre, BF16) if o.get("pre") else None
    st = torch.zeros(32, 2, Cout, device="cuda") if o.get("stats") else None
    args = (xg, wf, B, T, Cin, Cout, taps, pad, o.get("scale"), o.get("shift"), o.get("act", 0), o.get("res"), o.get("pe"),
            pool, st, None if of is None else of[:n_out], None if ob is None else ob[:n_out],
            None if op is None else op[:n_pre], o.get("p", 0.0), o.get("seed", 0), None, o.get("gradz"), o.get("gz_act", 0))
    if splitk:
        ws = torch.full((splitk * B * T * Cout,), float("nan"), device="cuda")
        hip.call("mm_conv1d_fwd_splitk", *args, ws, splitk)
    else:
        hip.call("mm_conv1d_fwd", *args)
    out = {}
    if of is not None:
        out["f32"] = _take(of, n_out, (B, To, Cout), "f32")
    if ob is not None:
        out["bf16"] = _take(ob, n_out, (B, To, Cout), "bf16")
    if op is not None:
        out["pre"] = _take(op, n_pre, (B, T, Cout), "pre")
    if st is not None:
        out["stats"] = acc_decode(st, ACC_STAT).cpu()
        out["stats_raw"] = st.cpu()
    return out


@pytest.mark.parametrize("case", FWD_CASES, ids=[_fwd_id(c) for c in FWD_CASES])
def test_forward_dispatch_matrix_vs_fp64(case):
    """mm_conv1d_fwd main loop in each (tile, KCT) cell and at the T / Cout / taps / pad edges: fp32 output vs fp64 conv of
    the same bf16 operands (+ bias), bf16 output = bf16(fp32 output), nothing written past the output, same bits twice"""
    hip = _hip()
    B, T, Cin, Cout, k, pad = case
    g = _g(B * 7919 + T * 31 + Cin * 7 + Cout + 100 * k + pad)
    x = (torch.randn(B, T, Cin, generator=g) * 0.8 + 0.1).to(BF16)
    w = torch.randn(Cout, Cin, k, generator=g) / math.sqrt(Cin * k)
    bias = torch.randn(Cout, generator=g) * 0.2
    wf, _ = _wimg(hip, w, Cin)
    want = _conv64(x, wf.cpu(), pad) + bias.double()
    o = dict(shift=bias.cuda())
    xg = x.cuda()
    a = _launch(hip, xg, wf, B, T, Cin, Cout, k, pad, o)
    b = _launch(hip, xg, wf, B, T, Cin, Cout, k, pad, o)
    e = _Errs(_fwd_id(case))
    e("fwd", _rel(a["f32"], want))
    e("fwd_peak", _peak(a["f32"], want))
    e.done()
    assert _same(a["bf16"], a["f32"].to(BF16))
    assert _same(a["f32"], b["f32"]) and _same(a["bf16"], b["bf16"])


# ----------------------------------------------------------------------------------------------------- epilogue matrix
# act codes: 0 none, 1 GELU(erf), 2 ReLU, 3 tanh, 4 sigmoid; gz = gradz_act (a gradz tensor is passed)
EPI_CASES = [
    dict(id="plain"),
    dict(id="bf16_only", f32=False),
    dict(id="scale_shift", scale=1, shift=1),
    dict(id="gelu", shift=1, act=1), dict(id="relu", shift=1, act=2), dict(id="tanh", shift=1, act=3),
    dict(id="sigmoid", shift=1, act=4),
    dict(id="gradz_none", gz=0), dict(id="gradz_gelu", gz=1), dict(id="gradz_relu", gz=2), dict(id="gradz_tanh", gz=3),
    dict(id="gradz_sigmoid", gz=4), dict(id="gradz_gelu_shift_act", scale=1, shift=1, gz=1, act=3),
    dict(id="stats", shift=1, stats=1), dict(id="stats_scale_gelu", scale=1, shift=1, act=1, stats=1),
    dict(id="residual", shift=1, res=1), dict(id="pe", shift=1, pe=1), dict(id="pre", scale=1, shift=1, act=1, pre=1),
    dict(id="dropout", shift=1, p=0.25), dict(id="drop_res_relu", shift=1, act=2, p=0.5, res=1),
    dict(id="drop_res_pe_gelu", scale=1, shift=1, act=1, p=0.125, res=1, pe=1),
    dict(id="pool2", pool=2), dict(id="pool2_gelu", shift=1, act=1, pool=2), dict(id="pool2_relu", shift=1, act=2, pool=2),
    dict(id="pool2_tanh", shift=1, act=3, pool=2), dict(id="pool2_sigmoid", shift=1, act=4, pool=2),
    dict(id="pool2_stats", scale=1, shift=1, act=1, stats=1, pool=2),
    dict(id="pool2_drop_res", shift=1, act=1, p=0.25, res=1, pool=2),
    dict(id="pool2_pe", shift=1, act=1, pe=1, pool=2), dict(id="pool2_pre", shift=1, act=1, pre=1, pool=2),
    dict(id="pool2_gradz", gz=1, pool=2),
    # the combinations the models run
    dict(id="conv_block_fwd", shift=1, stats=1, bf16=False),                         # bias, BatchNorm sums, fp32 out
    dict(id="conv_bn_act_pe", scale=1, shift=1, act=1, p=0.25, pe=1),              # ops.conv_bn_act with the table
    dict(id="conv_bn_gelu_pool", scale=1, shift=1, act=1, stats=1, pool=2, f32=False),
    dict(id="ffn1_gelu", shift=1, act=1, p=0.25, pre=1, f32=False),
    dict(id="ffn1_relu", shift=1, act=2, p=0.25, pre=1, f32=False),                 # activation="relu" blocks
    dict(id="ffn2_dgrad_gelu", gz=1, p=0.25, f32=False),
    dict(id="ffn2_dgrad_relu", gz=2, p=0.25, f32=False),
    dict(id="outproj", shift=1, p=0.25, res=1, bf16=False),
]
EPI_SHAPES = {"conv": (2, 70, 64, 48, 5, 2), "linear": (2, 66, 128, 132, 1, 0)}
_OPERANDS = {}


def _operands(hip, key, shape):
    """per-shape operands, made once: packed input, weight image, fp64 accumulator, epilogue tensors"""
    if key in _OPERANDS:
        return _OPERANDS[key]
    B, T, Cin, Cout, k, pad = shape
    g = _g(sum(shape) + len(key))
    x = (torch.randn(B, T, Cin, generator=g) * 0.8).to(BF16)
    w = torch.randn(Cout, Cin, k, generator=g) * 1.5 / math.sqrt(Cin * k)
    wf, _ = _wimg(hip, w, Cin)
    t = dict(xg=x.cuda(), wf=wf, acc=_conv64(x, wf.cpu(), pad),
             scale=0.5 + torch.rand(Cout, generator=g), shift=torch.randn(Cout, generator=g) * 0.3,
             res=torch.randn(B, T, Cout, generator=g), pe=torch.randn(T + 3, Cout, generator=g) * 0.5,
             gradz=(torch.randn(B, T, Cout, generator=g) * 1.5).to(BF16))
    _OPERANDS[key] = t
    return t


def _epi64(t, c, seed):
    """include/mmeeg_hip.h's epilogue in fp64, literally: v = acc * scale + shift; stats of v; out_pre = v;
    v *= act'(gradz); act; dropout; + residual + pe[t]; max over t pairs"""
    acc = t["acc"]
    B, T, N = acc.shape
    v = acc * (t["scale"].double() if c.get("scale") else 1.0) + (t["shift"].double() if c.get("shift") else 0.0)
    stats = torch.stack([v.sum((0, 1)), (v * v).sum((0, 1))])
    pre = v
    if "gz" in c:
        v = v * _dact64(t["gradz"].double(), c["gz"])
    o = _act64(v, c.get("act", 0))
    if c.get("p"):
        o = o * _keep(seed, (B, T, N), c["p"])
    if c.get("res"):
        o = o + t["res"].double()
    if c.get("pe"):
        o = o + t["pe"][:T].double()
    if c.get("pool", 1) == 2:
        o = o.view(B, T // 2, 2, N).amax(2)
    return o, stats, pre


def _epi_args(t, c, seed):
    o = dict(f32=c.get("f32", True), bf16=c.get("bf16", True), pre=c.get("pre"), stats=c.get("stats"),
             act=c.get("act", 0), pool=c.get("pool", 1), p=c.get("p", 0.0), seed=seed)
    for name in ("scale", "shift", "res", "pe"):
        if c.get(name):
            o[name] = t[name].contiguous().cuda()
    if "gz" in c:
        o["gradz"], o["gz_act"] = t["gradz"].cuda(), c["gz"]
    return o


def _check_epilogue(hip, tag, t, c, shape, seed, splitk=0):
    B, T, Cin, Cout, k, pad = shape
    o = _epi_args(t, c, seed)
    a = _launch(hip, t["xg"], t["wf"], B, T, Cin, Cout, k, pad, o, splitk)
    b = _launch(hip, t["xg"], t["wf"], B, T, Cin, Cout, k, pad, o, splitk)
    want, stats, _ = _epi64(t, c, seed)
    e = _Errs(tag)
    if "f32" in a:
        e("splitk" if splitk else "epi", _rel(a["f32"], want))
        e("epi_peak", _peak(a["f32"], want))
        if "bf16" in a:
            assert _same(a["bf16"], a["f32"].to(BF16)), "bf16 output != bf16(fp32 output)"
    else:
        e("epi_bf16", _rel(a["bf16"], want))
    if "stats" in a:
        e("stats", _rel(a["stats"], stats))
        assert torch.equal(a["stats_raw"].view(torch.int64), b["stats_raw"].view(torch.int64))
    if "pre" in a:
        # out_pre = bf16(v), v as a launch that stores it (scale / shift only, fp32 out) has it
        vo = dict(f32=True, bf16=False, scale=o.get("scale"), shift=o.get("shift"))
        v = _launch(hip, t["xg"], t["wf"], B, T, Cin, Cout, k, pad, vo, splitk)["f32"]
        assert _same(a["pre"], v.to(BF16)), "out_pre != bf16(v)"
    if c.get("p") and c.get("res") and c.get("pool", 1) == 1 and "f32" in a:
        dropped = _keep(seed, (B, T, Cout), c["p"]) == 0
        rp = t["res"] + (t["pe"][:T] if c.get("pe") else 0.0)
        assert dropped.any() and torch.equal(a["f32"][dropped], rp[dropped]), "a dropped position != the residual"
    for name in ("f32", "bf16", "pre"):
        if name in a:
            assert _same(a[name], b[name]), f"{name}: two runs differ"
    e.done()


@pytest.mark.parametrize("generic", [False, True], ids=["dispatch", "generic"])
@pytest.mark.parametrize("shape", list(EPI_SHAPES), ids=list(EPI_SHAPES))
@pytest.mark.parametrize("case", EPI_CASES, ids=[c["id"] for c in EPI_CASES])
def test_epilogue_matrix_vs_fp64(case, shape, generic, monkeypatch):
    """every epilogue step alone and in the models' combinations, on a k = 5 convolution (64 x 64 tile, KCT 64) and a
    Linear with a 4-column remainder (32 x 128, KCT 128); on the default dispatch (compiled-in epilogues where one
    exists) and on the generic epilogue"""
    hip = _hip()
    if generic:
        monkeypatch.setenv("MM_EPI_GENERIC", "1")
    t = _operands(hip, shape, EPI_SHAPES[shape])
    _check_epilogue(hip, f"{case['id']}-{shape}-{'generic' if generic else 'dispatch'}", t, case, EPI_SHAPES[shape], 1234)


# the compiled-in epilogues of the 64 x 128 tile (FFN-1 forward, FFN-2 data gradient, QKV) only run past 512 tiles
BIG_EPI = [("ffn1_gelu", (1, 8256, 128, 512, 1, 0)), ("ffn2_dgrad_gelu", (1, 8256, 128, 512, 1, 0)),
           ("plain_qkv", (1, 10944, 128, 384, 1, 0))]


@pytest.mark.parametrize("name,shape", BIG_EPI, ids=[n for n, _ in BIG_EPI])
def test_large_linear_epilogues_vs_fp64(name, shape):
    hip = _hip()
    c = dict(next(x for x in EPI_CASES if x["id"] == name)) if name != "plain_qkv" else dict(id=name, shift=1, f32=False)
    assert fwd_cell(*shape[:4], shape[4]) == ("64x128", 128)
    t = _operands(hip, "big-" + name, shape)
    _check_epilogue(hip, name + "-64x128", t, c, shape, 99)


@pytest.mark.parametrize("shape,nsplit", [((2, 70, 1088, 64, 7, 3), 8), ((3, 34, 1024, 48, 5, 1), 5)])
def test_splitk_conv_block_epilogue_vs_fp64(shape, nsplit):
    """mm_conv1d_fwd_splitk with scale / shift, GELU, stats, pool 2 (and an fp32 copy): 17 chunks in slices of 3 leave a
    last slice of 2; 16 chunks in slices of 4 (nsplit 5 -> 4 slices)"""
    hip = _hip()
    t = _operands(hip, ("splitk",) + shape, shape)
    c = dict(id="splitk", scale=1, shift=1, act=1, stats=1, pool=2)
    _check_epilogue(hip, f"splitk-{nsplit}", t, c, shape, 5, splitk=nsplit)
    c = dict(id="splitk_pre", scale=1, shift=1, act=2, pre=1, p=0.25, res=1, pe=1)
    _check_epilogue(hip, f"splitk-{nsplit}-pre", t, c, shape, 6, splitk=nsplit)


# ------------------------------------------------------------------------------------------------------ data gradient
# (B, T, Cin, Cout, k, pad) of the FORWARD convolution whose input gradient is formed
DGRAD_CASES = [(2, 70, 20, 48, 5, 2), (3, 33, 8, 20, 7, 3), (2, 64, 64, 128, 3, 1), (1, 65, 19, 72, 1, 0),
               (2, 40, 20, 48, 4, 1), (2, 31, 100, 40, 7, 0)]


@pytest.mark.parametrize("case", DGRAD_CASES, ids=[f"B{c[0]}-T{c[1]}-Cin{c[2]}-Cout{c[3]}-k{c[4]}p{c[5]}" for c in DGRAD_CASES])
def test_data_gradient_via_flipped_image_vs_fp64(case):
    """dX = the forward kernel on dY (B, T, Coutp) with the flipped data-gradient image (Cinp, k, Coutp) at pad k - 1 - pad,
    then mm_unpack_ntc_f32: vs the fp64 adjoint of the convolution; padded channels exactly 0"""
    hip = _hip()
    B, T, Cin, Cout, k, pad = case
    cinp, coutp = _cpad(Cin), _cpad(Cout)
    g = _g(B + T + Cin + Cout + k + pad)
    w = torch.randn(Cout, Cin, k, generator=g) / math.sqrt(Cout * k)
    _, wd = _wimg(hip, w, cinp, coutp)
    wb = w.to(BF16).double()
    img = torch.zeros(cinp, k, coutp, dtype=D64)
    img[:Cin, :, :Cout] = wb.flip(2).permute(1, 2, 0)
    assert torch.equal(wd.cpu().double(), img), "data-gradient image"
    dy = torch.zeros(B, T, coutp, dtype=BF16)
    dy[:, :, :Cout] = torch.randn(B, T, Cout, generator=g).to(BF16)
    want = torch.zeros(B, T, Cin, dtype=D64)                         # adjoint of y[t] = sum_tap x[t + tap - pad] W[tap]
    for tap in range(k):
        s = tap - pad
        t0, t1 = max(0, -s), min(T, T - s)
        if t0 < t1:
            want[:, t0 + s:t1 + s] += dy[:, t0:t1, :Cout].double() @ wb[:, :, tap]
    a = _launch(hip, dy.cuda(), wd, B, T, coutp, cinp, k, k - 1 - pad, {})
    e = _Errs(f"dgrad-{case}")
    e("dgrad", _rel(a["f32"][..., :Cin], want))
    assert torch.equal(a["f32"][..., Cin:], torch.zeros(B, T, cinp - Cin)), "padded channels of dX"
    assert _same(a["bf16"], a["f32"].to(BF16))
    dx = _nanbuf(B * Cin * T, F32)
    hip.call("mm_unpack_ntc_f32", a["bf16"].cuda(), dx[:B * Cin * T], B, Cin, T, cinp)
    dx = _take(dx, B * Cin * T, (B, Cin, T), "unpack")
    assert torch.equal(dx, a["bf16"][..., :Cin].float().transpose(1, 2))
    e("dgrad_bf16", _rel(dx, want.transpose(1, 2)))
    e.done()


# (B, T, Cin = dY channels, Cout = the BatchNorm's channels, k, pool, act, p, drop_first)
BNRED_CASES = [(2, 70, 64, 48, 5, 1, 1, 0.25, 0), (2, 40, 32, 64, 3, 2, 1, 0.25, 0), (3, 33, 64, 20, 7, 2, 2, 0.5, 1),
               (2, 64, 128, 64, 3, 1, 2, 0.0, 0), (2, 50, 16, 40, 4, 2, 1, 0.125, 1), (1, 65, 96, 64, 1, 1, 1, 0.25, 0)]


def _bn_dz64(y, out4, g, act, pool, p, seed, drop_first):
    """elementwise.hip's BatchNorm + act [+ pool 2] [+ dropout] backward, fp64: dz at the (B, T * pool, N) pre-BN rows"""
    sc, sh = out4[0].double(), out4[1].double()
    y, g = y.double(), g.double()
    B, Tp, N = y.shape
    T = Tp // pool
    z = y * sc + sh
    if pool == 1:
        m = _keep(seed, (B, T, N), p) if p else 1.0
        return g * m * _dact64(z, act)
    z0, z1 = z[:, 0::2], z[:, 1::2]
    m0 = m1 = torch.ones_like(z0)
    if p and drop_first:
        km = _keep(seed, (B, Tp, N), p)
        m0, m1 = km[:, 0::2], km[:, 1::2]
        first = _act64(z0, act) * m0 >= _act64(z1, act) * m1
    else:
        if p:
            g = g * _keep(seed, (B, T, N), p)
        first = _act64(z0, act) >= _act64(z1, act)
    d = g * torch.where(first, m0, m1) * _dact64(torch.where(first, z0, z1), act)
    dz = torch.zeros_like(z)
    dz[:, 0::2] = torch.where(first, d, torch.zeros_like(d))
    dz[:, 1::2] = torch.where(first, torch.zeros_like(d), d)
    return dz


def _bn_sums64(y, out4, dz):
    xhat = (y.double() - out4[2].double()) * out4[3].double()
    return torch.stack([dz.sum((0, 1)), (dz * xhat).sum((0, 1))])


@pytest.mark.parametrize("generic", [False, True], ids=["dispatch", "generic"])
@pytest.mark.parametrize("case", BNRED_CASES, ids=[f"B{c[0]}-T{c[1]}-k{c[4]}-pool{c[5]}-act{c[6]}-p{c[7]}-df{c[8]}" for c in BNRED_CASES])
def test_dgrad_bn_reduce_vs_fp64(case, generic, monkeypatch):
    """mm_conv1d_dgrad_bn_reduce: the bf16 d(out) vs the fp64 GEMM (and = bf16 of the plain launch's fp32 output), the
    BatchNorm-backward sums {sum dz, sum dz * xhat} vs fp64 from that d(out)"""
    hip = _hip()
    if generic:
        monkeypatch.setenv("MM_EPI_GENERIC", "1")
    B, T, Cin, Cout, k, pool, act, p, df = case
    pad = k - 1 - k // 2
    g = _g(B * T + Cin + Cout + k + pool)
    wd = (torch.randn(Cout, k, Cin, generator=g) / math.sqrt(Cin * k)).to(BF16)
    dy = (torch.randn(B, T, Cin, generator=g) * 0.5).to(BF16)
    yb = torch.randn(B, T * pool, Cout, generator=g) * 1.2 + 0.1
    out4 = torch.stack([0.5 + torch.rand(Cout, generator=g), torch.randn(Cout, generator=g) * 0.2,
                        torch.randn(Cout, generator=g) * 0.1, 0.8 + 0.4 * torch.rand(Cout, generator=g)]).contiguous()
    dyg, wdg, ybg, o4g = dy.cuda(), wd.cuda(), yb.cuda(), out4.cuda()

    def run():
        dx = _nanbuf(B * T * Cout, BF16)
        sums = torch.zeros(32, 2, Cout, device="cuda")
        hip.call("mm_conv1d_dgrad_bn_reduce", dyg, wdg, B, T, Cin, Cout, k, pad, dx[:B * T * Cout], ybg, o4g, sums,
                 act, pool, df, p, 321, None)
        return _take(dx, B * T * Cout, (B, T, Cout), "dx"), sums.cpu()
    (dx, sums), (dx2, sums2) = run(), run()
    assert _same(dx, dx2) and torch.equal(sums.view(torch.int64), sums2.view(torch.int64))
    plain = _launch(hip, dyg, wdg, B, T, Cin, Cout, k, pad, dict(bf16=False))["f32"]
    assert _same(dx, plain.to(BF16))
    e = _Errs(f"bnred-{case}")
    e("bnred_dx", _rel(dx, _conv64(dy, wd, pad)))
    want = _bn_sums64(yb, out4, _bn_dz64(yb, out4, dx, act, pool, p, 321, df))
    e("bnred", _rel(acc_decode(sums, ACC_GRAD), want))
    e.done()


# ---------------------------------------------------------------------------------------------------- weight gradient
# (B, T, Cin, Cout, taps, pad, Cin_real, layout): "param" = strides of the (Cout, Cin_real, k) parameter, "ws" = the
# channel-contiguous [n][tap][Cin] workspace of autograd.py (summed by mm_wgrad_scatter)
WGRAD_CASES = [
    (2, 65, 24, 8, 1, 0, 24, "param"), (2, 1000, 24, 8, 1, 0, 24, "ws"), (3, 63, 72, 24, 3, 1, 66, "ws"),
    (4, 1, 16, 200, 5, 2, 16, "param"), (2, 65, 200, 72, 7, 0, 197, "ws"), (2, 130, 64, 64, 3, 2, 64, "param"),
    (1, 300, 8, 24, 5, 1, 8, "ws"), (2, 63, 24, 8, 7, 3, 19, "ws"), (2, 40, 32, 48, 7, 6, 20, "param"),
    (8, 40, 1576, 200, 3, 1, 1570, "ws"),          # 100 tiles: samples in groups of 3 (3, 3, 2)
    (1, 300, 1576, 200, 3, 0, 1576, "param"),      # two chunks of 3 and 2 row tiles
]
WGRAD_TAPS = (1, 3, 5, 7)


def _wgrad64(dy, x, taps, pad):
    """dW[n][tap][c] = sum_{b,t} dY[b,t,n] X[b,t+tap-pad,c], fp64"""
    dy, x = dy.double(), x.double()
    B, T, C = x.shape
    N = dy.shape[2]
    xp = torch.zeros(B, T + taps - 1, C, dtype=D64)
    xp[:, pad:pad + T] = x
    d2 = dy.reshape(-1, N).t()
    return torch.stack([d2 @ xp[:, tap:tap + T].reshape(-1, C) for tap in range(taps)], 1)


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[f"B{c[0]}-T{c[1]}-Cin{c[2]}-Cout{c[3]}-k{c[4]}p{c[5]}-r{c[6]}-{c[7]}"
                                                   for c in WGRAD_CASES])
def test_weight_gradient_vs_fp64(case):
    """mm_conv1d_wgrad: the sum of the slots vs fp64 dY^T X per tap, every slot element below Cin_real written and none
    beyond, dbias vs the fp64 column sums of dY, same bits twice; the ws layout also through mm_wgrad_scatter (+=)"""
    hip = _hip()
    B, T, Cin, Cout, k, pad, creal, layout = case
    g = _g(B * T + Cin * 3 + Cout + k * 11 + pad)
    x = torch.randn(B, T, Cin, generator=g).to(BF16)
    dy = torch.randn(B, T, Cout, generator=g).to(BF16)
    n = ctypes.c_int(0)
    hip.call("mm_conv1d_wgrad_slots", B, T, Cin, Cout, k, ctypes.addressof(n))
    slots = n.value
    want = _wgrad64(dy, x, k, pad)[:, :, :creal]                   # (Cout, k, Cin_real)
    if layout == "param":
        shape, strides = (slots, Cout, creal, k), (creal * k, k, 1)
    else:
        shape, strides = (slots, Cout, k, Cin), (k * Cin, 1, Cin)
    per = shape[1] * shape[2] * shape[3]

    def run():
        ws = _nanbuf(slots * per, F32)
        db = torch.zeros(32, Cout, device="cuda")
        hip.call("mm_conv1d_wgrad", dy.cuda(), x.cuda(), ws[:slots * per], db, B, T, Cin, Cout, k, pad, creal, *strides,
                 slots, per, 1)
        return _take(ws, slots * per, shape, "slots"), db.cpu()
    (ws, db), (ws2, db2) = run(), run()
    assert _same(ws, ws2) and torch.equal(db.view(torch.int64), db2.view(torch.int64))
    if layout == "param":
        got = ws.permute(0, 1, 3, 2)
    else:
        assert torch.isnan(ws[..., creal:]).all(), "slot elements beyond Cin_real were written"
        got = ws[..., :creal]
    assert not torch.isnan(got).any(), "a slot element was left unwritten"
    e = _Errs(f"wgrad-{case}")
    e("wgrad", _rel(got.double().sum(0), want))
    e("dbias", _rel(acc_decode(db, ACC_GRAD), dy.double().sum((0, 1))))
    if layout == "ws":
        base = torch.randn(Cout, creal, k, generator=g)
        dw = base.cuda()
        hip.call("mm_wgrad_scatter", ws.cuda(), dw, Cout, creal, k, Cin, slots)
        e("wgrad", _rel(dw.cpu().double() - base.double(), want.permute(0, 2, 1)))
    e.done()


def test_weight_gradient_refuses_other_tap_counts():
    """the weight-gradient kernel is compiled for taps 1, 3, 5, 7: 2 and 9 are refused, not run"""
    hip = _hip()
    B, T, Cin, Cout = 1, 64, 16, 16
    x = torch.zeros(B, T, Cin, dtype=BF16, device="cuda")
    dy = torch.zeros(B, T, Cout, dtype=BF16, device="cuda")
    for k in (2, 9):
        n = ctypes.c_int(0)
        hip.call("mm_conv1d_wgrad_slots", B, T, Cin, Cout, k, ctypes.addressof(n))
        ws = torch.full((n.value, Cout, k, Cin), float("nan"), device="cuda")
        with pytest.raises(hip.HipLibraryError, match="taps"):
            hip.call("mm_conv1d_wgrad", dy, x, ws, None, B, T, Cin, Cout, k, k // 2, Cin, k * Cin, 1, Cin, n.value,
                     Cout * k * Cin, 1)
        assert torch.isnan(ws).all()


# (B, T, Cin, Cout, Cin_real): 14 problems = two tables (12 + 2); ragged 128-tiles in both directions
WMANY_CASES = [(1, 200, 136, 200, 130), (2, 65, 24, 8, 24), (1, 1, 256, 136, 256), (1, 300, 128, 384, 128),
               (3, 64, 48, 32, 40), (1, 129, 264, 72, 260), (2, 33, 16, 256, 16), (1, 1000, 40, 24, 40),
               (1, 70, 200, 200, 200), (2, 31, 128, 128, 100), (1, 64, 8, 8, 8), (1, 500, 72, 136, 72),
               (4, 17, 136, 16, 136), (1, 260, 384, 128, 384)]


def test_grouped_weight_gradients_vs_fp64():
    """mm_conv1d_wgrad_many (Linear weight gradients on the 128 x 128 tile, one launch per 12 problems): each problem's
    slot sum vs fp64 dY^T X, dbias vs fp64, every slot element below Cin_real written and none beyond, same bits twice"""
    hip = _hip()
    g = _g(77)
    probs = []
    for B, T, Cin, Cout, creal in WMANY_CASES:
        x = torch.randn(B * T, Cin, generator=g).to(BF16)
        dy = torch.randn(B * T, Cout, generator=g).to(BF16)
        n = ctypes.c_int(0)
        hip.call("mm_conv1d_wgrad_many_slots", B, T, Cin, Cout, ctypes.addressof(n))
        probs.append((B, T, Cin, Cout, creal, x, dy, x.cuda(), dy.cuda(), n.value))

    def run():
        outs, descs = [], []
        for B, T, Cin, Cout, creal, _, _, xg, dyg, slots in probs:
            ws = _nanbuf(slots * Cout * Cin, F32)
            db = torch.zeros(32, Cout, device="cuda")
            descs.append(struct.pack("<QQQQiiiiiiii", dyg.data_ptr(), xg.data_ptr(), ws.data_ptr(), db.data_ptr(),
                                     B, T, Cin, Cout, creal, slots, 0, 0))
            outs.append((ws, db))
        raw = b"".join(descs)
        host = ctypes.create_string_buffer(raw, len(raw))
        hip.call("mm_conv1d_wgrad_many", ctypes.addressof(host), len(probs))
        return [(_take(ws, p[9] * p[3] * p[2], (p[9], p[3], p[2]), "slots"), db.cpu()) for (ws, db), p in zip(outs, probs)]
    a, b = run(), run()
    e = _Errs("wgrad_many")
    for (ws, db), (ws2, db2), (B, T, Cin, Cout, creal, x, dy, _, _, slots) in zip(a, b, probs):
        assert _same(ws, ws2) and torch.equal(db.view(torch.int64), db2.view(torch.int64))
        assert torch.isnan(ws[..., creal:]).all() and not torch.isnan(ws[..., :creal]).any()
        e("wgrad", _rel(ws[..., :creal].double().sum(0), dy.double().t() @ x[:, :creal].double()))
        e("dbias", _rel(acc_decode(db, ACC_GRAD), dy.double().sum(0)))
    e.done()


# ------------------------------------------------------------------------------------------------ fused Linear forms
LIN_M = (32, 288)
LIN_K = (16, 96, 192, 256)                     # KCT 16 / 32 / 64 / 128
LN_EPS = 1e-5


def _ln64(o, gam, bet):
    mean = o.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((o - mean) ** 2).mean(1, keepdim=True) + LN_EPS)
    return (o - mean) * rstd * gam.double() + bet.double(), torch.cat([mean, rstd], 1)


@pytest.mark.parametrize("K", LIN_K)
@pytest.mark.parametrize("M", LIN_M)
def test_fused_linear_forward_forms_vs_fp64(M, K):
    """mm_linear_fwd_ln / _gemm2 / _gemm2_act / mm_linear_fwd_meanpool: out = dropout(x W^T + b) + residual, its
    LayerNorm rows and statistics, the second GEMM (+ bias, act, dropout, pre-activation) on the kernel's own LayerNorm
    rows, the mean over row groups"""
    hip = _hip()
    g = _g(M * 1000 + K)
    p, seed, p2, seed2 = 0.25, 17, 0.125, 18
    x = (torch.randn(M, K, generator=g) * 0.7).to(BF16)
    wf, _ = _wimg(hip, torch.randn(128, K, 1, generator=g) / math.sqrt(K), K)
    W = wf.cpu().double().view(128, K)
    bias, res = torch.randn(128, generator=g) * 0.2, torch.randn(M, 128, generator=g)
    gam, bet = 0.5 + torch.rand(128, generator=g), torch.randn(128, generator=g) * 0.2
    w2f, _ = _wimg(hip, torch.randn(384, 128, 1, generator=g) / math.sqrt(128), 128)
    W2 = w2f.cpu().double().view(384, 128)
    b2 = torch.randn(384, generator=g) * 0.1
    act2 = 1 if K in (16, 192) else 2
    xg, bg, rg, gg, beg, b2g = x.cuda(), bias.cuda(), res.cuda(), gam.cuda(), bet.cuda(), b2.cuda()
    o_ref = (x.double() @ W.t() + bias.double()) * _keep(seed, (M, 128), p) + res.double()
    h_ref, st_ref = _ln64(o_ref, gam, bet)
    e = _Errs(f"linfwd-M{M}-K{K}")

    def bufs():
        return (_nanbuf(M * 128, F32), _nanbuf(M * 128, BF16), _nanbuf(M * 2, F32), _nanbuf(M * 384, BF16),
                _nanbuf(M * 384, BF16))
    runs = []
    for form in ("ln", "gemm2", "gemm2_act"):
        o, h, st, o2, z2 = bufs()
        common = (xg, wf, M, K, bg, rg, o[:M * 128], p, seed, None, gg, beg, LN_EPS, h[:M * 128], st[:M * 2])
        if form == "ln":
            hip.call("mm_linear_fwd_ln", *common)
        elif form == "gemm2":
            hip.call("mm_linear_fwd_ln_gemm2", *common, w2f, b2g, 384, o2[:M * 384])
        else:
            hip.call("mm_linear_fwd_ln_gemm2_act", *common, w2f, b2g, 384, o2[:M * 384], z2[:M * 384], act2, p2, seed2)
        out = dict(o=_take(o, M * 128, (M, 128), "out"), h=_take(h, M * 128, (M, 128), "ln_out"),
                   st=_take(st, M * 2, (M, 2), "ln_stat"))
        e("lin", _rel(out["o"], o_ref))
        e("lin_stat", _rel(out["st"], st_ref))
        e("lin_h", _rel(out["h"], h_ref))
        if form != "ln":
            out["o2"] = _take(o2, M * 384, (M, 384), "out2")
            v2 = out["h"].double() @ W2.t() + b2.double()
            if form == "gemm2":
                e("lin_out2", _rel(out["o2"], v2))
            else:
                out["z2"] = _take(z2, M * 384, (M, 384), "pre2")
                e("lin_out2", _rel(out["z2"], v2))
                e("lin_out2", _rel(out["o2"], _act64(v2, act2) * _keep(seed2, (M, 384), p2)))
        else:
            assert torch.isnan(o2.float()).all() and torch.isnan(z2.float()).all()
        runs.append(out)
    assert all(_same(runs[0][n], r[n]) for r in runs[1:] for n in ("o", "h", "st"))
    # mean over groups of rows_per_group rows (accumulator workspace of 64-bit fixed-point sums)
    rpg = 32 if M == 32 else 96
    o = _nanbuf(M * 128, F32)
    pool = torch.zeros(M // rpg, 2 * 128, device="cuda")
    hip.call("mm_linear_fwd_meanpool", xg, wf, M, K, bg, rg, o[:M * 128], p, seed, None, pool, rpg)
    o = _take(o, M * 128, (M, 128), "meanpool out")
    assert _same(o, runs[0]["o"])
    e("lin_pool", _rel(pool.cpu().view(torch.int64).double() * 2.0 ** -ACC_GRAD, o_ref.view(M // rpg, rpg, 128).mean(1)))
    e.done()


@pytest.mark.parametrize("K", LIN_K)
@pytest.mark.parametrize("M", LIN_M)
def test_fused_linear_backward_forms_vs_fp64(M, K):
    """mm_linear_dgrad_ln_bwd / _gemm2 / _bn_reduce: dX = LayerNorm-backward(dY W) + dres, the dropout-masked bf16 copy,
    dgamma / dbeta, the second data-gradient GEMM on the kernel's own masked rows, the BatchNorm-backward sums of the
    conv block below from the kernel's own fp32 rows"""
    hip = _hip()
    g = _g(M * 1000 + K + 1)
    p, seed = 0.25, 41
    _, wd = _wimg(hip, torch.randn(K, 128, 1, generator=g) / math.sqrt(128), 128, K)     # Linear 128 -> K under LN
    Wd = wd.cpu().double().view(128, K)
    _, wdo = _wimg(hip, torch.randn(128, 128, 1, generator=g) / math.sqrt(128), 128, 128)
    Wdo = wdo.cpu().double().view(128, 128)
    dy = (torch.randn(M, K, generator=g) * 0.3).to(BF16)
    x = torch.randn(M, 128, generator=g) * 1.5 + 0.3
    stat = torch.stack([x.mean(1), (x.var(1, unbiased=False) + LN_EPS).rsqrt()], 1).contiguous()
    gam, dres = 0.5 + torch.rand(128, generator=g), torch.randn(M, 128, generator=g) * 0.2
    yb = torch.randn(M, 128, generator=g) * 1.2 + 0.1
    out4 = torch.stack([0.5 + torch.rand(128, generator=g), torch.randn(128, generator=g) * 0.2,
                        torch.randn(128, generator=g) * 0.1, 0.8 + 0.4 * torch.rand(128, generator=g)]).contiguous()
    dyg, xg, sg, gg, rg = dy.cuda(), x.cuda(), stat.cuda(), gam.cuda(), dres.cuda()
    dyv = dy.double() @ Wd.t()
    xh = (x.double() - stat[:, :1].double()) * stat[:, 1:].double()
    gh = dyv * gam.double()
    dx_ref = stat[:, 1:].double() * (gh - gh.mean(1, keepdim=True) - xh * (gh * xh).mean(1, keepdim=True)) + dres.double()
    dgb_ref = torch.stack([(dyv * xh).sum(0), dyv.sum(0)])
    e = _Errs(f"linbwd-M{M}-K{K}")
    runs = []
    for form in ("plain", "gemm2", "bn_reduce"):
        dx, dxb, do = _nanbuf(M * 128, F32), _nanbuf(M * 128, BF16), _nanbuf(M * 128, BF16)
        dgb = torch.zeros(32, 2, 128, device="cuda")
        common = (dyg, wd, M, K, xg, sg, gg, rg, dx[:M * 128])
        if form == "plain":
            hip.call("mm_linear_dgrad_ln_bwd", *common, dxb[:M * 128], dgb, p, seed, None)
        elif form == "gemm2":
            hip.call("mm_linear_dgrad_ln_bwd_gemm2", *common, dxb[:M * 128], dgb, p, seed, None, wdo, do[:M * 128], 0)
        else:
            sums = torch.zeros(32, 2, 128, device="cuda")
            act = 1 if K in (16, 192) else 2
            hip.call("mm_linear_dgrad_ln_bwd_bn_reduce", *common, dgb, None, yb.cuda(), out4.cuda(), sums, act,
                     0.25, 51, 0.125, 52)
        out = dict(dx=_take(dx, M * 128, (M, 128), "dx"), dgb=acc_decode(dgb, ACC_GRAD).cpu())
        e("lnb_dx", _rel(out["dx"], dx_ref))
        e("lnb_dgb", _rel(out["dgb"], dgb_ref))
        if form != "bn_reduce":
            out["dxb"] = _take(dxb, M * 128, (M, 128), "dx_bf16")
            masked = out["dx"] * keep_scale(seed, M * 128, p).view(M, 128)
            assert _same(out["dxb"], masked.to(BF16)), "dx_bf16 != bf16(dx * mask)"
            e("lnb_dxb", _rel(out["dxb"], dx_ref * _keep(seed, (M, 128), p)))
        else:
            assert torch.isnan(dxb.float()).all()
            gdr = out["dx"].double() * _keep(52, (M, 128), 0.125)
            want = _bn_sums64(yb, out4, _bn_dz64(yb.view(1, M, 128), out4, gdr.view(1, M, 128), act, 1, 0.25, 51, 1))
            e("lnb_sums", _rel(acc_decode(sums, ACC_GRAD).cpu(), want))
        if form == "gemm2":
            e("lnb_do", _rel(_take(do, M * 128, (M, 128), "do"), out["dxb"].double() @ Wdo.t()))
        else:
            assert torch.isnan(do.float()).all()
        runs.append(out)
    assert all(_same(runs[0]["dx"], r["dx"]) for r in runs[1:])
    e.done()
