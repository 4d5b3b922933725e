"""GPU: the 3-D implicit-GEMM family (csrc/conv3d.hip, conv3d_stream.hip, conv3d_wres.hip, conv3d_wgrad.hip) through the
C ABI against plain fp64 references of the same operation, computed on the CPU from the kernels' own operands: the
bf16-rounded channels-last activations and the bf16-rounded weights (mm_prep_conv_weight rounds to nearest even, so
w.bfloat16() is the image's value whatever lane order the image is stored in).

  - mm_conv3d_fwd in every kernel instance its dispatcher can pick (`fwd_instance` restates the tile arithmetic and every
    case asserts the instance it is meant to hit): the four generic instances at Cin 16 / 32 / 96, Cout 16 .. 160 with
    ragged column blocks, odd D, ragged faces; the five weight-streaming instances below and at >= 256 tiles with the
    XCD tile order on and off; the weight-resident kernel at 64, 68 and 264 tiles and the generic kernel on the same
    operands at 63; fp32-only, bf16-only and both outputs, with and without bias and BatchNorm sums;
  - mm_conv3d_wgrad_slots / mm_conv3d_wgrad / mm_wgrad_scatter: one (ragged) face, odd face counts, one- and two-stage
    chunks, a short odd last chunk, D = 1, H and W < 8, Cin 16 / 96, Cin_real < Cin, Cout 8 / 24 / 48 / 96, both stride
    layouts, a slot base off 16-byte alignment, more slots than the grid uses, dbias, and the long chains of two training
    shapes;
  - what is refused: Cin 48, no output pointer, slot_mode 0, too few slots, Cin % 8 != 0.

Bounds (none comes from the kernels' measured error).  rel = ||got - want|| / ||want||, peak = max |got - want| / max |want|.
  fp32 outputs, slot sums   4 x e32, where e32 is the error of the SAME operation run in float32 on the CPU (F.conv3d /
                            conv3d_weight on .float() operands) against the fp64 reference, computed per case: two bits for
                            the different summation order (MFMA K-chain, K-group / wave partial sums through LDS, slots)
  bf16-only outputs         per element |got - want| <= 2^-8 |want| (one RNE rounding: half a bf16 ulp) + the fp32 peak
                            bound x max |want|; reported as the worst ratio to that bound (<= 1)
  BatchNorm sums, dbias     per channel |got - want| <= n 2^-24 sum|v| (sum v^2 for the second moment) + adds x 2^-(K + 1),
                            n = the longest fp32 partial-sum chain before the fixed-point accumulator (K = 28 / 40 bits, one
                            rint per add):  generic kernel 16 TM per lane + 1 lane exchange + WM wave rows + 1 (the square)
                            = 22 / 22 / 20 / 36 for <2,32,4,1> / <2,64,4,1> / <1,64,2,2> / <2,128,2,2>;  streaming kernel
                            4 OWN + 2 + WK + 1 = 15 / 21 / 36 for NW = 1 / 2 / 4;  weight-resident kernel 16 per tile of the
                            workgroup + 7;  dbias 8 per face of the chunk + 1.  Reported as the worst ratio (<= 1).

Worst cases measured on the MI355X (ERR lines of a run; bound beside it):

    e32 itself (16 CPU threads)   1.5e-8 (one ragged face) .. 4.9e-7 rel (K = 27 x 128), 1.1e-7 .. 1.4e-6 peak
    generic kernel    fp32 out rel 2.6e-7 (bound 1.5e-6; 96 -> 32), closest to its bound 0.40 x (32 -> 96);  peak 7.5e-7 (3.2e-6),
                      closest 0.76 x (32 -> 24);  bf16-only 0.995 of the per-element bound;  sums 0.11 of theirs
    streaming kernel  fp32 out rel 2.3e-7 (2.0e-6), closest 0.32 x;  peak 6.3e-7 (4.7e-6), closest 0.26 x;  bf16-only 0.994;
                      sums 0.078
    weight-resident   bf16 out 0.994 of the per-element bound;  sums 0.014
    weight gradient   slot sum rel 1.1e-7 (2.1e-6; layer 3 of the C2 step, chunks of 26 faces), closest 0.24 x (one ragged face:
                      bound 6.1e-8);  scatter 1.4e-7 (1.1e-6);  dbias 3.8e-4 of its bound (sums of bf16 values are nearly
                      exact in fp32)

42 GPU tests, references included, take 4.3 s of pytest time on the MI355X (the fp64 and float32 references about 1 s of it).

Exact, no tolerance: a bf16 output equals bf16(fp32 output) of the same launch; NaN-filled guard regions behind every
output stay NaN; every slot element below Cin_real and Cout is written and nothing else in the slot buffer; the two slot
layouts hold the same bits; a second launch gives identical bits.

test_wrong_references_fail_the_bounds (CPU) evaluates three deliberately wrong fp64 references per operation (halo wraps
into the neighbouring row / sample, one tap axis mirrored, the last 8 input channels dropped) and asserts that the float32
CPU result fails the bounds above against each of them."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from multimodal_eeg_fmri_amd.ops import ACC_GRAD, ACC_STAT, acc_decode
from test_kernels_gpu import _hip, _prep_w

D64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
GUARD = 256                              # NaN-filled elements behind every output: must stay NaN
E32_FACTOR = 4.0                         # two bits over the float32 CPU run of the same operation
U32 = 2.0 ** -24                         # fp32 unit round-off
BF16_HALF_ULP = 2.0 ** -8                # one RNE rounding to bf16, relative


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

    def __call__(self, name, err, bound):
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


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ dispatch mirror
def wres_tiles(B, D, H, W):
    return B * _cdiv(D, 4) * _cdiv(H, 8) * _cdiv(W, 8)


def tiles2(B, D, H, W):
    return B * _cdiv(D, 2) * _cdiv(H, 8) * _cdiv(W, 8)


def fwd_instance(B, D, H, W, Cin, Cout, f32, bf16):
    """the kernel instance mm_conv3d_fwd (csrc/conv3d.hip) launches, restated: the weight-resident kernel for 32 -> 64,
    bf16-only output and >= 64 tiles of 4 x 8 x 8; the streaming kernel for its three channel pairs (NW column groups per
    workgroup by the count of 2 x 8 x 8 tiles); else the generic kernel <TD, BN, WM, WN> by Cout, tile count and D's parity.
    It labels and picks the test shapes; every case asserts its own label."""
    t2 = tiles2(B, D, H, W)
    if Cin == 32 and Cout == 64 and bf16 and not f32 and wres_tiles(B, D, H, W) >= 64:
        return "wres"
    if (Cin, Cout) == (64, 128):
        return "stream<64,128,4>" if t2 >= 256 else "stream<64,128,2>"
    if (Cin, Cout) == (128, 64):
        return "stream<128,64,2>" if t2 >= 256 else "stream<128,64,1>"
    if (Cin, Cout) == (64, 32):
        return "stream<64,32,1>"
    if Cout <= 32:
        return "generic<2,32,4,1>"
    if Cout <= 64:
        return "generic<2,64,4,1>" if t2 >= 256 and D % 2 == 0 else "generic<1,64,2,2>"
    return "generic<2,128,2,2>" if t2 * _cdiv(Cout, 128) >= 256 and D % 2 == 0 else "generic<1,64,2,2>"


# the longest fp32 chain of the BatchNorm sums per instance (module docstring)
STAT_CHAIN = {"generic<2,32,4,1>": 22, "generic<2,64,4,1>": 22, "generic<1,64,2,2>": 20, "generic<2,128,2,2>": 36,
              "stream<64,128,4>": 36, "stream<64,128,2>": 21, "stream<128,64,2>": 21, "stream<128,64,1>": 15,
              "stream<64,32,1>": 15}


def stat_chain(inst, B, D, H, W):
    if inst != "wres":
        return STAT_CHAIN[inst]
    # conv3d_wres.hip: grid = min(256, tiles & ~7) workgroups, XCD x walks the x-th eighth of the tile list; a lane adds its
    # 16 values per channel and tile into one running sum, then + ragged-tile sum, 2 lane exchanges, 3 wave adds, the square
    nt = wres_tiles(B, D, H, W)
    grid = 256 if nt >= 256 else nt & ~7
    return 16 * _cdiv(_cdiv(nt, 8), grid // 8) + 7


def stream_grid_is_xcd_ordered(B, D, H, W):
    return tiles2(B, D, H, W) % 8 == 0


def wgrad_tiles(B, D, H, W):
    return B * D * _cdiv(H, 8) * _cdiv(W, 8)


def wgrad_tiles_per_wg(B, D, H, W, Cin, Cout):
    """csrc/conv3d_wgrad.hip: wgrad3d_tiles_per_wg, restated (faces of 1 x 8 x 8 per chunk = slot)"""
    total = wgrad_tiles(B, D, H, W)
    par = _cdiv(Cout, 32) * 3 * _cdiv(Cin, 32)
    chunks = max(1, min(256 // par, total // 8))
    per = _cdiv(total, chunks)
    return per + (per & 1)


# ------------------------------------------------------------------------------------------------------ references
def _conv64(x, w, T=D64, wrong=None):
    """x (B, D, H, W, Cin) bf16, w (Cout, Cin, 3, 3, 3) bf16-valued -> (B, D, H, W, Cout) in dtype T.  ``wrong``: a plausible
    kernel mistake, for test_wrong_references_fail_the_bounds"""
    x, w = x.to(T), w.to(T)
    if wrong == "mirror":
        w = w.flip(-1)
    if wrong == "drop8":
        x = x.clone()
        x[..., -8:] = 0
    if wrong == "wrap":
        B, D, H, W, C = x.shape
        xf = x.reshape(-1, C)
        y = torch.zeros(xf.shape[0], w.shape[0], dtype=T)
        for tap in range(27):
            kd, kh, kw = tap // 9 - 1, (tap // 3) % 3 - 1, tap % 3 - 1
            y += torch.roll(xf, -((kd * H + kh) * W + kw), 0) @ w.reshape(w.shape[0], C, 27)[:, :, tap].t()
        return y.view(B, D, H, W, -1)
    return F.conv3d(x.permute(0, 4, 1, 2, 3), w, None, padding=1).permute(0, 2, 3, 4, 1).contiguous()


def _wgrad64(dy, x, T=D64, wrong=None):
    """dy (B, D, H, W, Cout), x (B, D, H, W, Cin) bf16 -> dW (Cout, Cin, 27) in dtype T"""
    dy, x = dy.to(T), x.to(T)
    B, D, H, W, C = x.shape
    N = dy.shape[-1]
    if wrong == "drop8":
        x = x.clone()
        x[..., -8:] = 0
    if wrong == "wrap":
        xf, d2 = x.reshape(-1, C), dy.reshape(-1, N).t()
        return torch.stack([d2 @ torch.roll(xf, -(((t // 9 - 1) * H + (t // 3) % 3 - 1) * W + t % 3 - 1), 0) for t in range(27)], 2)
    dw = torch.nn.grad.conv3d_weight(x.permute(0, 4, 1, 2, 3), (N, C, 3, 3, 3), dy.permute(0, 4, 1, 2, 3), padding=1)
    if wrong == "mirror":
        dw = dw.flip(-1)
    return dw.reshape(N, C, 27)


_REFS = {}


def _fwd_ref(key, B, D, H, W, Cin, Cout):
    """per-shape operands and references, made once and left unchanged: x, w, bias (CPU), acc = fp64 convolution without
    bias, e32 = (rel, peak) of the float32 CPU convolution against it"""
    if key in _REFS:
        return _REFS[key]
    g = _g(B * 7919 + D * 131 + H * 17 + W * 5 + Cin * 3 + Cout)
    x = (torch.randn(B, D, H, W, Cin, generator=g) * 0.8 + 0.1).to(BF16)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / math.sqrt(27 * Cin)
    bias = torch.randn(Cout, generator=g) * 0.3
    wb = w.to(BF16)
    acc = _conv64(x, wb)
    a32 = _conv64(x, wb, F32)
    r = dict(x=x, w=w, bias=bias, acc=acc, e32=(_rel(a32, acc), _peak(a32, acc)))
    _REFS[key] = r
    return r


# ------------------------------------------------------------------------------------------------------- forward
pytest_gpu = pytest.mark.gpu

# output forms: (fp32 out, bf16 out, bias, BatchNorm sums)
BOTH, F32_ONLY, BF16_ONLY, BF16_PLAIN = (1, 1, 1, 1), (1, 0, 0, 1), (0, 1, 1, 0), (0, 1, 0, 0)
F32_PLAIN = (1, 0, 0, 0)
ALL_FORMS = (BOTH, F32_ONLY, BF16_ONLY, BF16_PLAIN)

# (B, D, H, W, Cin, Cout, instance, forms)
FWD_CASES = [
    # generic <2,32,4,1>: the generic first layer (odd D, ragged H and W); Cout below the tile and no multiple of 32;
    # the data-gradient form over three Cin chunks
    (2, 5, 11, 13, 16, 16, "generic<2,32,4,1>", ALL_FORMS),
    (1, 4, 9, 10, 32, 24, "generic<2,32,4,1>", ALL_FORMS),
    (2, 3, 8, 12, 96, 32, "generic<2,32,4,1>", (BF16_PLAIN, F32_PLAIN)),
    # generic <2,64,4,1>: >= 256 two-deep tiles, even D; an fp32 output keeps the weight-resident kernel away
    (4, 8, 32, 32, 32, 64, "generic<2,64,4,1>", (BOTH, F32_ONLY)),
    (8, 4, 32, 32, 16, 48, "generic<2,64,4,1>", ALL_FORMS),
    # generic <1,64,2,2>: odd D; two and three column blocks with a ragged last one
    (2, 3, 8, 8, 32, 64, "generic<1,64,2,2>", (BOTH, F32_ONLY)),
    (1, 2, 8, 8, 32, 96, "generic<1,64,2,2>", ALL_FORMS),
    (1, 2, 9, 7, 32, 160, "generic<1,64,2,2>", ALL_FORMS),
    # generic <2,128,2,2>: tiles x column blocks >= 256, even D; ragged inside the 128-wide block; two column blocks
    (16, 8, 9, 9, 32, 128, "generic<2,128,2,2>", ALL_FORMS),
    (16, 8, 9, 9, 32, 96, "generic<2,128,2,2>", (BOTH, BF16_PLAIN)),
    (8, 8, 9, 9, 32, 160, "generic<2,128,2,2>", (BOTH, BF16_PLAIN)),
    # streaming kernel: all five instances; >= 256 tiles with odd D and ragged faces (260 tiles: no multiple of 8, the XCD
    # tile order is off) and at 256 tiles (on); < 256 tiles with grids of 24 (on), 6 (off), 36 (off)
    (13, 9, 9, 9, 64, 128, "stream<64,128,4>", ALL_FORMS),
    (16, 8, 9, 9, 64, 128, "stream<64,128,4>", (BOTH, BF16_PLAIN)),
    (16, 8, 9, 9, 128, 64, "stream<128,64,2>", ALL_FORMS),
    (13, 9, 9, 9, 128, 64, "stream<128,64,2>", (BOTH, BF16_PLAIN)),
    (2, 3, 12, 20, 64, 128, "stream<64,128,2>", ALL_FORMS),
    (1, 2, 20, 12, 128, 64, "stream<128,64,1>", ALL_FORMS),
    (3, 5, 16, 16, 64, 32, "stream<64,32,1>", ALL_FORMS),
    (2, 4, 10, 9, 64, 32, "stream<64,32,1>", (BOTH, BF16_PLAIN)),
]
STREAM_XCD = {(13, 9, 9, 9): False, (16, 8, 9, 9): True, (2, 3, 12, 20): True, (1, 2, 20, 12): False, (3, 5, 16, 16): False,
              (2, 4, 10, 9): True}


def _fwd_id(c):
    B, D, H, W, Cin, Cout, inst, _ = c
    return f"{inst}-B{B}-{D}x{H}x{W}-{Cin}to{Cout}"


def _fwd_launch(hip, xg, wf, B, D, H, W, Cin, Cout, form, bias_g):
    """one mm_conv3d_fwd into NaN-guarded outputs -> {f32, bf16 (CPU, guard checked), stats (fp64 sums), stats_raw}"""
    f32, bf16, shift, stats = form
    n = B * D * H * W * Cout
    of = _nanbuf(n, F32) if f32 else None
    ob = _nanbuf(n, BF16) if bf16 else None
    st = torch.zeros(32, 2, Cout, device="cuda") if stats else None
    hip.call("mm_conv3d_fwd", xg, wf, B, D, H, W, Cin, Cout, bias_g if shift else None, st,
             None if of is None else of[:n], None if ob is None else ob[:n])
    out = {}
    if of is not None:
        out["f32"] = _take(of, n, (B, D, H, W, Cout), "out_f32")
    if ob is not None:
        out["bf16"] = _take(ob, n, (B, D, H, W, Cout), "out_bf16")
    if st is not None:
        out["stats"] = acc_decode(st, ACC_STAT).cpu()
        out["stats_raw"] = st.cpu()
    return out


def _stat_ratio(got, v, n, adds, k):
    """worst over channels and both moments of |got - want| / (n 2^-24 sum|v| [sum v^2] + adds 2^-(k + 1)); v (..., N) fp64"""
    v = v.reshape(-1, v.shape[-1])
    want = torch.stack([v.sum(0), (v * v).sum(0)])
    scale = torch.stack([v.abs().sum(0), (v * v).sum(0)])
    bound = n * U32 * scale + adds * 2.0 ** -(k + 1)
    return ((got.double() - want).abs() / bound).max().item()


def _bf16_ratio(got, want, peak_bound):
    """worst |got - want| / (2^-8 |want| + peak_bound max|want|)"""
    want = want.double()
    bound = BF16_HALF_ULP * want.abs() + peak_bound * want.abs().max()
    return ((got.double() - want).abs() / bound).max().item()


def _check_forward(hip, tag, r, B, D, H, W, Cin, Cout, inst, forms, xg=None, wf=None):
    """every form of one case against the shared fp64 reference (the first B samples of it)"""
    xg = r["x"][:B].contiguous().cuda() if xg is None else xg
    wf = _prep_w(hip, r["w"].reshape(Cout, Cin, 27), Cin)[0] if wf is None else wf
    bias_g = r["bias"].cuda()
    e_rel, e_peak = r["e32"]
    e = _Errs(tag)
    e("e32", e_rel, 1e-6)                                       # the yardstick itself: float32 on the CPU is near round-off
    faces = B * D * _cdiv(H, 8) * _cdiv(W, 8)                   # >= the workgroups that add into the accumulator
    for i, form in enumerate(forms):
        f32, bf16, shift, stats = form
        assert fwd_instance(B, D, H, W, Cin, Cout, f32, bf16) == inst, (form, fwd_instance(B, D, H, W, Cin, Cout, f32, bf16))
        want = r["acc"][:B] + (r["bias"].double() if shift else 0.0)
        a = _fwd_launch(hip, xg, wf, B, D, H, W, Cin, Cout, form, bias_g)
        name = "".join(s for s, on in zip(("f32", "+bf16" if f32 else "bf16", "+bias", "+stats"), form) if on)
        if f32:
            e(f"{name} rel", _rel(a["f32"], want), E32_FACTOR * e_rel)
            e(f"{name} peak", _peak(a["f32"], want), E32_FACTOR * e_peak)
            if bf16:
                assert _same(a["bf16"], a["f32"].to(BF16)), f"{tag} {name}: bf16 output != bf16(fp32 output)"
        else:
            e(f"{name} elem", _bf16_ratio(a["bf16"], want, E32_FACTOR * e_peak), 1.0)
        if stats:
            e(f"{name} sums", _stat_ratio(a["stats"], want, stat_chain(inst, B, D, H, W), faces, ACC_STAT), 1.0)
        if i == 0:
            b = _fwd_launch(hip, xg, wf, B, D, H, W, Cin, Cout, form, bias_g)
            for k in ("f32", "bf16"):
                assert k not in a or _same(a[k], b[k]), f"{tag} {name}: two runs differ in {k}"
            assert "stats" not in a or torch.equal(a["stats_raw"].view(torch.int64), b["stats_raw"].view(torch.int64))
    e.done()


@pytest_gpu
@pytest.mark.parametrize("case", FWD_CASES, ids=[_fwd_id(c) for c in FWD_CASES])
def test_forward_instances_vs_fp64(case):
    """mm_conv3d_fwd in the generic and the weight-streaming instances, every output form of the case"""
    hip = _hip()
    B, D, H, W, Cin, Cout, inst, forms = case
    if inst.startswith("stream"):
        assert stream_grid_is_xcd_ordered(B, D, H, W) == STREAM_XCD[(B, D, H, W)]
        assert (tiles2(B, D, H, W) >= 256) == (inst in ("stream<64,128,4>", "stream<128,64,2>"))
    r = _fwd_ref(case[:6], B, D, H, W, Cin, Cout)
    _check_forward(hip, _fwd_id(case), r, B, D, H, W, Cin, Cout, inst, forms)


# weight-resident kernel (32 -> 64, bf16 only): exactly 64 tiles (one per workgroup); 68 tiles on a grid of 64 (four
# workgroups take two), ragged in H and W; 264 tiles (more than 256, no multiple of 256), ragged in D, H and W
WRES_FORMS = ((0, 1, 1, 1), BF16_PLAIN, BF16_ONLY, (0, 1, 0, 1))
WRES_CASES = [(64, 4, 8, 8, 64), (17, 4, 9, 9, 68), (33, 6, 9, 9, 264)]


@pytest_gpu
@pytest.mark.parametrize("case", WRES_CASES, ids=[f"B{c[0]}-{c[1]}x{c[2]}x{c[3]}-{c[4]}tiles" for c in WRES_CASES])
def test_weight_resident_kernel_vs_fp64(case):
    """csrc/conv3d_wres.hip: bf16 output per element to half a bf16 ulp + the fp32 bound, BatchNorm sums to their chain"""
    hip = _hip()
    B, D, H, W, nt = case
    assert wres_tiles(B, D, H, W) == nt
    grid = 256 if nt >= 256 else nt & ~7
    assert (nt, grid) in ((64, 64), (68, 64), (264, 256))
    r = _fwd_ref(("wres",) + case, B, D, H, W, 32, 64)
    _check_forward(hip, f"wres-{nt}tiles", r, B, D, H, W, 32, 64, "wres", WRES_FORMS)
    if nt == 64:
        # the same operands, one sample (= tile) fewer: 63 tiles, the generic kernel runs
        assert wres_tiles(B - 1, D, H, W) == 63
        _check_forward(hip, "generic-63tiles", r, B - 1, D, H, W, 32, 64, "generic<1,64,2,2>", WRES_FORMS)


@pytest_gpu
def test_forward_refuses_cin_48_and_a_launch_without_output():
    hip = _hip()
    B, D, H, W, Cout = 1, 2, 8, 8, 32
    for Cin, with_out, msg in ((48, True, "Cin=48"), (32, False, "null")):
        x = torch.zeros(B, D, H, W, Cin, dtype=BF16, device="cuda")
        w = torch.zeros(Cout, 27, Cin, dtype=BF16, device="cuda")
        n = B * D * H * W * Cout
        out = _nanbuf(n, F32)
        with pytest.raises(hip.HipLibraryError, match=msg):
            hip.call("mm_conv3d_fwd", x, w, B, D, H, W, Cin, Cout, None, None, out[:n] if with_out else None, None)
        assert torch.isnan(out).all()


# ---------------------------------------------------------------------------------------------------- weight gradient
# (B, D, H, W, Cin, Cout, Cin_real, what): every case runs both stride layouts ("param": the strides of the (Cout,
# Cin_real, 27) parameter; "ws": the channel-contiguous [n][tap][Cin] workspace that mm_wgrad_scatter sums)
WGRAD_CASES = [
    (1, 1, 8, 8, 32, 32, 32, "one_face"),             # one stage whose second face is a phantom
    (1, 1, 5, 3, 32, 32, 32, "one_ragged_face"),
    (3, 1, 8, 8, 32, 64, 32, "three_faces"),          # two stages, odd: a phantom face
    (2, 4, 4, 4, 64, 128, 64, "layer3_of_16cubed"),   # H, W < 8
    (4, 1, 16, 16, 32, 32, 32, "depth_1"),            # both neighbouring kd planes are outside
    (2, 5, 9, 20, 32, 64, 32, "ragged_volume"),
    (3, 11, 7, 5, 32, 64, 32, "short_odd_last_chunk"),   # 33 ragged faces in chunks of 10: the last holds 3
    (2, 3, 9, 10, 16, 32, 16, "cin16"),
    (2, 3, 9, 10, 16, 32, 1, "cin16_real1"),
    (2, 3, 9, 10, 96, 32, 96, "cin96"),
    (2, 3, 9, 10, 32, 8, 32, "cout8"),
    (2, 3, 9, 10, 32, 24, 32, "cout24"),
    (2, 3, 9, 10, 32, 48, 32, "cout48"),
    (2, 3, 9, 10, 32, 96, 32, "cout96"),
    (2, 3, 9, 10, 64, 32, 40, "cin64_real40"),        # ws layout: block 0 takes the vector stores, block 1 the scalar ones
    # the longest chains: layer 3 of the C2 step (10 chunks of 26 faces) and 512 faces in chunks of 14, the ring at full depth
    (32, 8, 8, 8, 64, 128, 64, "c2_layer3"),
    (8, 16, 16, 16, 32, 64, 32, "deep_chunks"),
]


def _wgrad_ref(case):
    if case in _REFS:
        return _REFS[case]
    B, D, H, W, Cin, Cout, creal, _ = case
    g = _g(B * 7919 + D * 131 + H * 17 + W * 5 + Cin * 3 + Cout + creal)
    x = torch.randn(B, D, H, W, Cin, generator=g).to(BF16)
    dy = torch.randn(B, D, H, W, Cout, generator=g).to(BF16)
    want = _wgrad64(dy, x)
    w32 = _wgrad64(dy, x, F32)
    r = dict(x=x, dy=dy, want=want, e32=_rel(w32, want))
    _REFS[case] = r
    return r


def _wgrad_launch(hip, dyg, xg, dims, creal, layout, slots, nrep=None, rep_extra=0, dbias=True):
    """mm_conv3d_wgrad into a NaN-filled slot buffer of nrep slots (rep_stride = slot size + rep_extra floats) ->
    (slots as (nrep, per + rep_extra) CPU fp32, dbias workspace)"""
    B, D, H, W, Cin, Cout = dims
    nrep = slots if nrep is None else nrep
    if layout == "param":
        per, strides = Cout * creal * 27, (creal * 27, 27, 1)
    else:
        per, strides = Cout * 27 * Cin, (27 * Cin, 1, Cin)
    stride = per + rep_extra
    ws = _nanbuf(nrep * stride, F32)
    db = torch.zeros(32, Cout, device="cuda") if dbias else None
    hip.call("mm_conv3d_wgrad", dyg, xg, ws[:nrep * stride], db, B, D, H, W, Cin, Cout, creal, *strides, nrep, stride, 1)
    return _take(ws, nrep * stride, (nrep, stride), "slots"), (None if db is None else db.cpu())


def _slot_view(ws, layout, Cin, Cout, creal, per_extra=0):
    """(nrep, stride) -> (nrep, Cout, creal, 27) of the written elements; asserts that exactly those were written"""
    nrep = ws.shape[0]
    if layout == "param":
        per = Cout * creal * 27
        body = ws[:, :per].view(nrep, Cout, creal, 27)
        got = body
    else:
        per = Cout * 27 * Cin
        body = ws[:, :per].view(nrep, Cout, 27, Cin)
        assert torch.isnan(body[..., creal:]).all(), "slot elements beyond Cin_real were written"
        got = body[..., :creal].permute(0, 1, 3, 2)
    assert torch.isnan(ws[:, per:]).all(), "the gap between two slots was written"
    return got


@pytest_gpu
@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[7] for c in WGRAD_CASES])
def test_weight_gradient_vs_fp64(case):
    """mm_conv3d_wgrad in both layouts: slot sum vs fp64 (4 x e32), the two layouts hold the same bits, every element below
    Cin_real / Cout of every used slot written and nothing else, dbias to its chain bound, the scatter, same bits twice"""
    hip = _hip()
    B, D, H, W, Cin, Cout, creal, what = case
    dims = (B, D, H, W, Cin, Cout)
    n = ctypes.c_int(0)
    hip.call("mm_conv3d_wgrad_slots", B, D, H, W, Cin, Cout, ctypes.addressof(n))
    slots, tpw, total = n.value, wgrad_tiles_per_wg(*dims), wgrad_tiles(B, D, H, W)
    assert slots == _cdiv(total, tpw), (slots, total, tpw)
    last = total - (slots - 1) * tpw                           # faces in the last chunk
    if what in ("one_face", "one_ragged_face"):
        assert total == 1 and slots == 1                       # one stage
    if what == "three_faces":
        assert total == 3 and slots == 1 and tpw == 4          # two stages
    if what == "layer3_of_16cubed":
        assert (D, H, W) == (4, 4, 4) and (Cin, Cout) == (64, 128)
    if what == "short_odd_last_chunk":
        assert slots > 1 and last < tpw and last % 2 == 1, (total, tpw, slots, last)
    if what == "c2_layer3":
        assert (slots, tpw) == (10, 26)
    if what == "deep_chunks":
        assert total == 512 and tpw == 14 and slots == 37
    if what == "cin64_real40":
        assert 32 <= creal < Cin == 64
    r = _wgrad_ref(case)
    dyg, xg = r["dy"].cuda(), r["x"].cuda()
    want = r["want"][:, :creal]                                # (Cout, Cin_real, 27)
    e = _Errs(f"wgrad-{what}")
    e("e32", r["e32"], 1e-6)
    bound = E32_FACTOR * r["e32"]
    ws_p, db = _wgrad_launch(hip, dyg, xg, dims, creal, "param", slots)
    ws_c, db_c = _wgrad_launch(hip, dyg, xg, dims, creal, "ws", slots)
    ws_p2, db2 = _wgrad_launch(hip, dyg, xg, dims, creal, "param", slots)
    assert _same(ws_p, ws_p2) and torch.equal(db.view(torch.int64), db2.view(torch.int64)), "two runs differ"
    assert torch.equal(db.view(torch.int64), db_c.view(torch.int64))
    got_p, got_c = _slot_view(ws_p, "param", Cin, Cout, creal), _slot_view(ws_c, "ws", Cin, Cout, creal)
    assert not torch.isnan(got_p).any() and not torch.isnan(got_c).any(), "a slot element was left unwritten"
    assert _same(got_p, got_c), "the two slot layouts differ"
    e("slot sum rel", _rel(got_p.double().sum(0), want), bound)
    # dbias: every wave adds the 8 dY values per face of its k-steps into one running sum over the chunk, one lane exchange
    dyv = r["dy"].double().reshape(-1, Cout)
    db_bound = (8 * tpw + 1) * U32 * dyv.abs().sum(0) + 4 * slots * 2.0 ** -(ACC_GRAD + 1)
    e("dbias", ((acc_decode(db, ACC_GRAD) - dyv.sum(0)).abs() / db_bound).max().item(), 1.0)
    # the scatter of the channel-contiguous slots = the sum of the PyTorch-layout slots
    dw = torch.zeros(Cout, creal, 27, device="cuda")
    hip.call("mm_wgrad_scatter", ws_c.reshape(-1).cuda(), dw, Cout, creal, 27, Cin, slots)
    e("scatter vs slot sum", _rel(dw.cpu(), got_p.double().sum(0)), bound)
    e("scatter rel", _rel(dw.cpu(), want), bound)
    e.done()


@pytest_gpu
def test_weight_gradient_slot_bases_and_spare_slots():
    """rep_stride one float past the slot size puts slot 1 off 16-byte alignment (the vector stores turn off for it alone);
    nrep above the grid's chunk count leaves the spare slots untouched; without dbias"""
    hip = _hip()
    case = (2, 5, 9, 20, 32, 64, 32, "ragged_volume")
    B, D, H, W, Cin, Cout, creal, _ = case
    dims = case[:6]
    r = _wgrad_ref(case)
    dyg, xg = r["dy"].cuda(), r["x"].cuda()
    slots = _cdiv(wgrad_tiles(B, D, H, W), wgrad_tiles_per_wg(*dims))
    assert slots >= 2
    base, _ = _wgrad_launch(hip, dyg, xg, dims, creal, "ws", slots, dbias=False)
    off, _ = _wgrad_launch(hip, dyg, xg, dims, creal, "ws", slots, rep_extra=1, dbias=False)
    assert (Cout * 27 * Cin + 1) * 4 % 16 != 0
    assert _same(_slot_view(off, "ws", Cin, Cout, creal), _slot_view(base, "ws", Cin, Cout, creal))
    spare, _ = _wgrad_launch(hip, dyg, xg, dims, creal, "ws", slots, nrep=slots + 2, dbias=False)
    assert _same(spare[:slots], base) and torch.isnan(spare[slots:]).all(), "spare slots were written"
    e = _Errs("wgrad-slot-bases")
    e("slot sum rel", _rel(_slot_view(off, "ws", Cin, Cout, creal).double().sum(0), r["want"]), E32_FACTOR * r["e32"])
    e.done()


@pytest_gpu
def test_weight_gradient_refusals():
    """slot_mode 0, fewer slots than chunks, Cin % 8 != 0: an error, and the slot buffer stays NaN"""
    hip = _hip()
    B, D, H, W, Cout = 2, 5, 9, 20, 64
    for Cin, slot_mode, short, msg in ((32, 0, 0, "slot_mode"), (32, 1, 1, "slots"), (12, 1, 0, "channels")):
        n = ctypes.c_int(0)
        hip.call("mm_conv3d_wgrad_slots", B, D, H, W, Cin, Cout, ctypes.addressof(n))
        assert n.value >= 2
        x = torch.zeros(B, D, H, W, Cin, dtype=BF16, device="cuda")
        dy = torch.zeros(B, D, H, W, Cout, dtype=BF16, device="cuda")
        ws = torch.full((n.value, Cout, 27, Cin), float("nan"), device="cuda")
        with pytest.raises(hip.HipLibraryError, match=msg):
            hip.call("mm_conv3d_wgrad", dy, x, ws, None, B, D, H, W, Cin, Cout, Cin, 27 * Cin, 1, Cin, n.value - short,
                     Cout * 27 * Cin, slot_mode)
        assert torch.isnan(ws).all()


# ------------------------------------------------------------------------------------- that the comparison has teeth
def test_wrong_references_fail_the_bounds():
    """CPU: at a ragged shape, the float32 CPU result - which a correct kernel may be up to 4x worse than - misses the fp32
    bounds against each of three wrong fp64 references, for the forward and for the weight gradient; and the explicit
    per-tap form the wrong references are built from agrees with F.conv3d / conv3d_weight where nothing is wrong"""
    B, D, H, W, Cin, Cout = 2, 3, 9, 11, 64, 40
    g = _g(5)
    x = (torch.randn(B, D, H, W, Cin, generator=g) * 0.8 + 0.1).to(BF16)
    w = (torch.randn(Cout, Cin, 3, 3, 3, generator=g) / math.sqrt(27 * Cin)).to(BF16)
    dy = torch.randn(B, D, H, W, Cout, generator=g).to(BF16)
    for name, fn, ops_ in (("fwd", _conv64, (x, w)), ("wgrad", _wgrad64, (dy, x))):
        r64, r32 = fn(*ops_), fn(*ops_, F32)
        e_rel, e_peak = _rel(r32, r64), _peak(r32, r64)
        assert e_rel < 1e-6
        for wrong in ("wrap", "mirror", "drop8"):
            bad = fn(*ops_, wrong=wrong)
            d_rel, d_peak = _rel(r32, bad), _peak(r32, bad)
            print(f"SEP {name} {wrong}: rel {d_rel:.3e} vs bound {E32_FACTOR * e_rel:.3e}, peak {d_peak:.3e} vs {E32_FACTOR * e_peak:.3e}")
            assert d_rel > 100 * E32_FACTOR * e_rel and d_peak > 100 * E32_FACTOR * e_peak, (name, wrong)
            if name == "fwd":                                   # the bf16-only criterion too
                assert _bf16_ratio(r32.to(BF16), bad, E32_FACTOR * e_peak) > 1.0
                assert _bf16_ratio(r32.to(BF16), r64, E32_FACTOR * e_peak) <= 1.0
    # the wrap reference differs from the right one only where a tap leaves the volume: inside, it IS the convolution
    inner = _conv64(x, w, wrong="wrap")[:, 1:-1, 1:-1, 1:-1]
    assert _rel(inner, _conv64(x, w)[:, 1:-1, 1:-1, 1:-1]) < 1e-12
    # statistics criterion: a sum that misses the last row of voxels is outside the chain bound
    v = _conv64(x, w)
    short = torch.stack([v[:, :, :-1].sum((0, 1, 2, 3)), (v[:, :, :-1] ** 2).sum((0, 1, 2, 3))])
    assert _stat_ratio(short, v, 36, B * D * 4, ACC_STAT) > 1.0
    full = torch.stack([v.float().sum((0, 1, 2, 3)), (v.float() ** 2).sum((0, 1, 2, 3))])
    assert _stat_ratio(full, v, 36, B * D * 4, ACC_STAT) <= 1.0
