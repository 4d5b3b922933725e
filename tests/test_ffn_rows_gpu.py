"""GPU: a transformer block's row-wise forward as one launch (mm_ffn_rows_fwd: out-projection + norm2, both FFN Linears and
the second one's consumers) and the second GEMM it shares with mm_linear_fwd_ln_gemm2 / mm_linear_dgrad_ln_bwd_gemm2.

The fused launch re-arranges where values sit, not what is computed, so every output is held to torch.equal against the
chain of launches it replaces (mm_linear_fwd_ln -> mm_conv1d_fwd -> mm_linear_fwd_ln / _ln_gemm2 / _meanpool) on the same
inputs; one case per consumer is also restated in fp64 from the kernel's own bf16 operands, with the tolerance of
test_kernels_gpu.py's test of mm_linear_fwd_ln_gemm2_act (2e-2: bf16 outputs).  The trainer test holds a tape step and a
captured step to the same bits with the fusion on and off."""
import math

import pytest
import torch

from multimodal_eeg_fmri_amd.ops import ACC_GRAD
from test_kernels_gpu import _hip, _prep_w

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
EPS = 1e-5
GELU = 1
NQ = 384
RPG = 32


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), device="cuda").to(dtype)


_inputs_cache = {}


def _inputs(M, n1):
    """operands of one block's row-wise part (built once per shape, never modified)"""
    if (M, n1) in _inputs_cache:
        return _inputs_cache[M, n1]
    hip = _hip()
    g = torch.Generator().manual_seed(1000 * M + n1)
    d = {}
    d["wo_f64"] = torch.randn(128, 128, 1, generator=g) / math.sqrt(128)
    d["w1_f64"] = torch.randn(n1, 128, 1, generator=g) / math.sqrt(128)
    d["w2_f64"] = torch.randn(128, n1, 1, generator=g) / math.sqrt(n1)
    d["wq_f64"] = torch.randn(NQ, 128, 1, generator=g) / math.sqrt(128)
    d["wo"], _ = _prep_w(hip, d["wo_f64"], 128)
    d["w1"], _ = _prep_w(hip, d["w1_f64"], 128)
    d["w2"], _ = _prep_w(hip, d["w2_f64"], n1)
    d["wq"], _ = _prep_w(hip, d["wq_f64"], 128)
    d["x"] = (torch.randn(M, 128, generator=g) * 0.5).cuda().to(BF16)
    d["res"] = torch.randn(M, 128, generator=g).cuda()
    for n, w in (("bo", 128), ("b1", n1), ("b2", 128), ("bq", NQ), ("bet", 128), ("bet2", 128)):
        d[n] = (torch.randn(w, generator=g) * 0.1).cuda()
    d["gam"] = (0.5 + torch.rand(128, generator=g)).cuda()
    d["gam2"] = (0.5 + torch.rand(128, generator=g)).cuda()
    d["epoch"] = torch.tensor([0x9E3779B1 & 0x7FFFFFFF], dtype=torch.int32, device="cuda")      # non-zero seed epoch word
    _inputs_cache[M, n1] = d
    return d


def _run(d, M, n1, p, tail, pre, save, fused):
    """-> dict of every output; tail in ('ln', 'qkv', 'pool'); pre: pre-activation copy wanted; save: hidden output wanted"""
    hip = _hip()
    o = dict(x1=_nan((M, 128), F32), h2=_nan((M, 128), BF16), st2=_nan((M, 2), F32), y=_nan((M, 128), F32))
    z = _nan((M, n1), BF16) if pre else None
    g = _nan((M, n1), BF16) if (save or not fused) else None
    hn = st = q = pool = None
    if tail == "pool":
        pool = torch.zeros(M // RPG, 2 * 128, device="cuda")
    else:
        hn, st = _nan((M, 128), BF16), _nan((M, 2), F32)
        if tail == "qkv":
            q = _nan((M, NQ), BF16)
    ep = d["epoch"]
    head = (d["x"], d["wo"], M, 128, d["bo"], d["res"], o["x1"], p, 91, ep, d["gam"], d["bet"], EPS, o["h2"], o["st2"])
    if fused:
        hip.call("mm_ffn_rows_fwd", *head, d["w1"], d["b1"], n1, g, z, GELU, p, 92, d["w2"], d["b2"], o["y"], p, 93,
                 None if hn is None else d["gam2"], None if hn is None else d["bet2"], EPS, hn, st,
                 d["wq"] if q is not None else None, d["bq"] if q is not None else None, NQ if q is not None else 0, q,
                 pool, RPG if pool is not None else 0)
    else:
        hip.call("mm_linear_fwd_ln", *head)
        hip.call("mm_conv1d_fwd", o["h2"], d["w1"], 1, M, 128, n1, 1, 0, None, d["b1"], GELU, None, None, 1, None, None, g, z,
                 p, 92, ep, None, 0)
        tl = (g, d["w2"], M, n1, d["b2"], o["x1"], o["y"], p, 93, ep)
        if tail == "pool":
            hip.call("mm_linear_fwd_meanpool", *tl, pool, RPG)
        elif tail == "ln":
            hip.call("mm_linear_fwd_ln", *tl, d["gam2"], d["bet2"], EPS, hn, st)
        else:
            hip.call("mm_linear_fwd_ln_gemm2", *tl, d["gam2"], d["bet2"], EPS, hn, st, d["wq"], d["bq"], NQ, q)
    o.update(z=z, g=g if save else None, hn=hn, st=st, q=q, pool=None if pool is None else pool.view(torch.int64))
    return o


_chain_cache = {}


def _chain(M, n1, p, tail):
    """the chain of launches, computed once per case (pre-activation copy and hidden output both written)"""
    key = (M, n1, p, tail)
    if key not in _chain_cache:
        _chain_cache[key] = _run(_inputs(M, n1), M, n1, p, tail, True, True, False)
    return _chain_cache[key]


@pytest.mark.parametrize("pre,save", [(True, True), (False, True), (False, False)])
@pytest.mark.parametrize("tail", ["ln", "qkv", "pool"])
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("n1", [128, 512])
@pytest.mark.parametrize("M", [32, 96])
def test_ffn_rows_forward_equals_the_chain_of_launches(M, n1, p, tail, pre, save):
    """mm_ffn_rows_fwd: x1, norm2 rows and statistics, the pre-activation copy z, the hidden g, y, the consumer's LayerNorm
    rows / statistics / projection or the pool accumulator words - the bits of mm_linear_fwd_ln -> mm_conv1d_fwd ->
    mm_linear_fwd_ln / _ln_gemm2 / _meanpool; one tile and three (row0 > 0), one column group and four"""
    want = _chain(M, n1, p, tail)
    got = _run(_inputs(M, n1), M, n1, p, tail, pre, save, True)
    torch.cuda.synchronize()
    for name, t in got.items():
        if t is None:
            continue
        assert want[name] is not None, name
        if t.is_floating_point():
            assert torch.isfinite(t.float()).all(), name
        assert torch.equal(t, want[name]), (name, M, n1, p, tail)
    assert (got["z"] is not None) == pre and (got["g"] is not None) == save


@pytest.mark.parametrize("tail", ["ln", "qkv", "pool"])
def test_ffn_rows_forward_vs_fp64(tail):
    """each stage restated in fp64 from the launch's own upstream output and the bf16 weight images (p = 0)"""
    M, n1 = 96, 512
    d = _inputs(M, n1)
    o = _run(d, M, n1, 0.0, tail, True, True, True)
    torch.cuda.synchronize()
    c = {k: (v.cpu().double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}
    img = lambda n: d[n].cpu().double().view(d[n].shape[0], -1)        # forward weight image (Cout, Cin) as the kernel reads it
    tol = dict(rtol=2e-2, atol=2e-2)

    def ln(v, gam, bet):
        mean = v.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((v - mean) ** 2).mean(1, keepdim=True) + EPS)
        return (v - mean) * rstd * gam + bet, torch.cat([mean, rstd], 1)
    x1 = c["x"] @ img("wo").t() + c["bo"] + c["res"]
    torch.testing.assert_close(o["x1"].cpu().double(), x1, **tol)
    h2, st2 = ln(o["x1"].cpu().double(), c["gam"], c["bet"])
    torch.testing.assert_close(o["h2"].cpu().double(), h2, **tol)
    torch.testing.assert_close(o["st2"].cpu().double(), st2, **tol)
    z = o["h2"].cpu().double() @ img("w1").t() + c["b1"]
    torch.testing.assert_close(o["z"].cpu().double(), z, **tol)
    torch.testing.assert_close(o["g"].cpu().double(), torch.nn.functional.gelu(z), **tol)
    y = o["g"].cpu().double() @ img("w2").t() + c["b2"] + o["x1"].cpu().double()
    torch.testing.assert_close(o["y"].cpu().double(), y, **tol)
    yk = o["y"].cpu().double()
    if tail == "pool":
        torch.testing.assert_close(o["pool"].cpu().double().view(M // RPG, 128) * 2.0 ** -ACC_GRAD,
                                   yk.view(M // RPG, RPG, 128).mean(1), **tol)
        return
    hn, st = ln(yk, c["gam2"], c["bet2"])
    torch.testing.assert_close(o["hn"].cpu().double(), hn, **tol)
    torch.testing.assert_close(o["st"].cpu().double(), st, **tol)
    if tail == "qkv":
        torch.testing.assert_close(o["q"].cpu().double(), o["hn"].cpu().double() @ img("wq").t() + c["bq"], **tol)


def test_ffn_rows_forward_rejects_shapes_it_cannot_tile():
    """M not a multiple of 32, n1 not a multiple of 128, K != 128: the library's error, nothing launched"""
    hip = _hip()
    d = _inputs(96, 512)

    def call(M, K, n1):
        o = [_nan((96, 128), F32), _nan((96, 128), BF16), _nan((96, 2), F32), _nan((96, 512), BF16), _nan((96, 512), BF16),
             _nan((96, 128), F32), _nan((96, 128), BF16), _nan((96, 2), F32)]
        hip.call("mm_ffn_rows_fwd", d["x"], d["wo"], M, K, d["bo"], d["res"], o[0], 0.0, 1, None, d["gam"], d["bet"], EPS, o[1],
                 o[2], d["w1"], d["b1"], n1, o[3], o[4], GELU, 0.0, 2, d["w2"], d["b2"], o[5], 0.0, 3, d["gam2"], d["bet2"], EPS,
                 o[6], o[7], None, None, 0, None, None, 0)
        torch.cuda.synchronize()
        return o
    for bad in ((80, 128, 512), (96, 128, 448), (96, 64, 512)):
        with pytest.raises(hip.HipLibraryError):
            call(*bad)
    assert all(torch.isfinite(t.float()).all() for t in call(96, 128, 512))


@pytest.mark.parametrize("M", [32, 96])
def test_second_gemm_callers_equal_their_two_launch_forms(M):
    """mm_linear_fwd_ln_gemm2 (n2 = 384: the staging tiles wrap) and mm_linear_dgrad_ln_bwd_gemm2 against the same
    launch without the second GEMM followed by mm_conv1d_fwd on its bf16 rows"""
    hip = _hip()
    g = torch.Generator().manual_seed(77 + M)
    K = 512
    d = _inputs(M, 512)
    x = (torch.randn(M, K, generator=g) * 0.5).cuda().to(BF16)
    outs = []
    for fused in (False, True):
        o, h, st, q = _nan((M, 128), F32), _nan((M, 128), BF16), _nan((M, 2), F32), _nan((M, NQ), BF16)
        common = (x, d["w2"], M, K, d["b2"], d["res"], o, 0.3, 71, d["epoch"], d["gam"], d["bet"], EPS, h, st)
        if fused:
            hip.call("mm_linear_fwd_ln_gemm2", *common, d["wq"], d["bq"], NQ, q)
        else:
            hip.call("mm_linear_fwd_ln", *common)
            hip.call("mm_conv1d_fwd", h, d["wq"], 1, M, 128, NQ, 1, 0, None, d["bq"], 0, None, None, 1, None, None, q, None,
                     0.0, 0, None, None, 0)
        outs.append((o, h, st, q))
    for a, b in zip(*outs):
        assert torch.isfinite(b.float()).all() and torch.equal(a, b)
    # backward: dX = LayerNorm-backward(dY W) + dres, masked bf16 copy, then do = that copy x the out-projection's dgrad image
    _, wd = _prep_w(hip, torch.randn(K, 128, 1, generator=g) / math.sqrt(128), 128, K)
    _, wdo = _prep_w(hip, torch.randn(128, 128, 1, generator=g) / math.sqrt(128), 128, 128)
    dy = (torch.randn(M, K, generator=g) * 0.1).cuda().to(BF16)
    xin = torch.randn(M, 128, generator=g).cuda()
    stat = torch.stack([xin.mean(1), (xin.var(1, unbiased=False) + EPS).rsqrt()], 1).contiguous()
    outs = []
    for fused in (False, True):
        dx, dxb, dgb, do = _nan((M, 128), F32), _nan((M, 128), BF16), torch.zeros(32, 2, 128, device="cuda"), _nan((M, 128), BF16)
        common = (dy, wd, M, K, xin, stat, d["gam"], d["res"], dx, dxb, dgb, 0.3, 63, d["epoch"])
        if fused:
            hip.call("mm_linear_dgrad_ln_bwd_gemm2", *common, wdo, do, 0)
        else:
            hip.call("mm_linear_dgrad_ln_bwd", *common)
            hip.call("mm_conv1d_fwd", dxb, wdo, 1, M, 128, 128, 1, 0, None, None, 0, None, None, 1, None, None, do, None,
                     0.0, 0, None, None, 0)
        outs.append((dx, dxb, dgb.view(torch.int32), do))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert torch.isfinite(outs[1][3].float()).all()


@pytest.mark.parametrize("mode", ["manual", "graph"])
def test_trainer_step_is_bit_identical_with_the_row_fusions_off(mode, monkeypatch):
    """one tape step / one captured step at the knob loop's configuration of test_trainer_gpu.py: the default (whole
    row-wise part in one launch) against the second FFN Linear as its own launch and against both as their own"""
    from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
    from multimodal_eeg_fmri_amd import ops
    batch = synthetic_pairs(32, 64, 1024, (32, 32, 32), seed=300)

    def run(**knobs):
        for k, v in knobs.items():
            monkeypatch.setattr(ops, k, v)
        ops.set_seed_epoch(None)
        ops.set_dropout_seed(4321)
        torch.manual_seed(0)
        tr = BridgeTrainer(eeg_channels=64, dropout=0.2, lr=1e-3, mode=mode).train()
        loss = tr.train_step(*batch)["loss"].clone()
        torch.cuda.synchronize()
        params = [q.detach().clone() for m in (tr.eeg_encoder, tr.fmri_encoder, tr.head) for q in m.parameters()]
        ops.set_seed_epoch(None)
        monkeypatch.undo()
        return loss, params
    assert not ops._NO_FFN_ROWS and not ops._NO_FFN1_FUSE
    l0, p0 = run()
    assert torch.isfinite(l0).all()
    for knobs in (dict(_NO_FFN_ROWS=True), dict(_NO_FFN1_FUSE=True)):
        l1, p1 = run(**knobs)
        assert torch.equal(l0, l1), knobs
        assert len(p0) == len(p1) and all(torch.equal(a, b) for a, b in zip(p0, p1)), knobs
