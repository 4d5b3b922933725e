"""GPU: a transformer block's row-wise backward as one launch (mm_ffn_rows_bwd: linear2's data gradient with the hidden
activation's derivative and dropout mask, linear1's data gradient on the dz rows the workgroup still holds, norm2's backward
and the out-projection's data gradient).

The fused launch re-arranges where values sit, not what is computed, so every output is held to torch.equal against the
two launches it replaces (mm_conv1d_fwd with gradz -> mm_linear_dgrad_ln_bwd_gemm2) on the same inputs; one case is also
restated in fp64 from the kernel's own bf16 operands with the tolerances test_kernels_gpu.py applies to the replaced launches
(test_linear_dgrad_fused_with_layernorm_backward: dx 2e-3, LayerNorm parameter sums 2e-3 of their scale, masked bf16 rows
1e-2; test_linear_dgrad_ln_backward_with_second_gemm: a bf16 GEMM output rtol 2e-2 / atol 2e-3).  The trainer test holds
three tape steps and three captured steps to the same bits with the fusion on and off."""
import math

import pytest
import torch

from test_kernels_gpu import _grad, _hip, _prep_w

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
EPS = 1e-5
GELU = 1


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), device="cuda").to(dtype)


_inputs_cache = {}


def _inputs(M, n1, rpp):
    """operands of one block's row-wise backward (built once per shape, never modified); rpp = rows per skip-gradient row"""
    key = (M, n1, rpp)
    if key in _inputs_cache:
        return _inputs_cache[key]
    hip = _hip()
    g = torch.Generator().manual_seed(2000 * M + n1 + rpp)
    d = {}
    _, d["w2d"] = _prep_w(hip, torch.randn(128, n1, 1, generator=g) / math.sqrt(n1), n1, 128)     # linear2: n1 -> 128
    _, d["w1d"] = _prep_w(hip, torch.randn(n1, 128, 1, generator=g) / math.sqrt(128), 128, n1)    # linear1: 128 -> n1
    _, d["wod"] = _prep_w(hip, torch.randn(128, 128, 1, generator=g) / math.sqrt(128), 128, 128)  # out_proj: 128 -> 128
    d["dy2"] = (torch.randn(M, 128, generator=g) * 0.1).cuda().to(BF16)
    d["z"] = torch.randn(M, n1, generator=g).cuda().to(BF16)
    d["x1"] = (torch.randn(M, 128, generator=g) * 2 + 0.5).cuda()
    d["stat"] = torch.stack([d["x1"].mean(1), (d["x1"].var(1, unbiased=False) + EPS).rsqrt()], 1).contiguous()
    d["gam"] = (0.5 + torch.rand(128, generator=g)).cuda()
    d["dres"] = (torch.randn(M // rpp if rpp else M, 128, generator=g) * 0.1).cuda()
    d["epoch"] = torch.tensor([0x9E3779B1 & 0x7FFFFFFF], dtype=torch.int32, device="cuda")      # non-zero seed epoch word
    _inputs_cache[key] = d
    return d


def _run(d, M, n1, p, rpp, fused):
    hip = _hip()
    o = dict(dz=_nan((M, n1), BF16), dx1=_nan((M, 128), F32), dyo=_nan((M, 128), BF16), do=_nan((M, 128), BF16))
    dgb = torch.zeros(32, 2, 128, device="cuda")
    ep = d["epoch"]
    if fused:
        hip.call("mm_ffn_rows_bwd", d["dy2"], d["w2d"], M, n1, d["z"], GELU, p, 92, o["dz"], d["w1d"], d["x1"], d["stat"], d["gam"],
                 d["dres"], rpp, o["dx1"], o["dyo"], dgb, p, 91, ep, d["wod"], o["do"])
    else:
        hip.call("mm_conv1d_fwd", d["dy2"], d["w2d"], 1, M, 128, n1, 1, 0, None, None, 0, None, None, 1, None, None, o["dz"], None,
                 p, 92, ep, d["z"], GELU)
        hip.call("mm_linear_dgrad_ln_bwd_gemm2", o["dz"], d["w1d"], M, n1, d["x1"], d["stat"], d["gam"], d["dres"], o["dx1"],
                 o["dyo"], dgb, p, 91, ep, d["wod"], o["do"], rpp)
    o["dgb_words"] = dgb.view(torch.int32)
    o["dgb"] = dgb
    return o


_chain_cache = {}


def _chain(M, n1, p, rpp):
    """the two launches, computed once per case"""
    key = (M, n1, p, rpp)
    if key not in _chain_cache:
        _chain_cache[key] = _run(_inputs(M, n1, rpp), M, n1, p, rpp, False)
    return _chain_cache[key]


@pytest.mark.parametrize("M,n1,p,rpp,generic", [(32, 128, 0.0, 0, False), (32, 512, 0.3, 0, False), (64, 512, 0.3, 32, False),
                                                (96, 256, 0.2, 0, False), (32, 512, 0.3, 0, True)])
def test_ffn_rows_backward_equals_the_two_launches(M, n1, p, rpp, generic, monkeypatch):
    """mm_ffn_rows_bwd: dz, dx1, the masked rows dyo, do and the LayerNorm accumulator words - the bits of mm_conv1d_fwd
    (gradz) -> mm_linear_dgrad_ln_bwd_gemm2; one workgroup and several, one column group and four (weight prefetch, both
    z staging tiles), one skip-gradient row per sample, and the generic epilogue against the compiled-in chain"""
    want = _chain(M, n1, p, rpp)
    if generic:
        monkeypatch.setenv("MM_EPI_GENERIC", "1")
    got = _run(_inputs(M, n1, rpp), M, n1, p, rpp, True)
    torch.cuda.synchronize()
    for name in ("dz", "dx1", "dyo", "do", "dgb_words"):
        t = got[name]
        if t.is_floating_point():
            assert torch.isfinite(t.float()).all(), name
        assert torch.equal(t, want[name]), (name, M, n1, p, rpp, generic)
    assert got["do"].float().abs().max() > 1e-3 and got["dz"].float().abs().max() > 1e-3


def test_ffn_rows_backward_vs_fp64():
    """each stage restated in fp64 from the launch's own upstream bf16 output and the bf16 weight images"""
    M, n1, p = 64, 512, 0.3
    d = _inputs(M, n1, 0)
    o = _run(d, M, n1, p, 0, True)
    torch.cuda.synchronize()
    c = lambda t: t.cpu().double()                                     # noqa: E731
    # dz = (dy2 W2) * gelu'(z) * mask / (1 - p), one rounding to bf16: kept elements against the unmasked product
    zz = c(d["z"])
    cdf = 0.5 * (1.0 + torch.erf(zz / math.sqrt(2.0)))
    dgelu = cdf + zz * torch.exp(-0.5 * zz * zz) / math.sqrt(2.0 * math.pi)
    dz_ref = (c(d["dy2"]) @ c(d["w2d"]).view(n1, 128).t()) * dgelu / (1.0 - p)
    dz = c(o["dz"])
    kept = dz != 0
    frac = kept.double().mean().item()
    print(f"dz kept fraction {frac:.4f}; max |dz - ref| on kept {((dz - dz_ref)[kept]).abs().max().item():.3e}")
    assert abs(frac - (1.0 - p)) < 0.03
    torch.testing.assert_close(dz[kept], dz_ref.to(BF16).double()[kept], rtol=2e-2, atol=2e-3)
    # d h2 = dz W1, then LayerNorm backward + skip gradient
    dh = dz @ c(d["w1d"]).view(128, n1).t()
    x, mean, rstd, gam = c(d["x1"]), c(d["stat"])[:, :1], c(d["stat"])[:, 1:], c(d["gam"])
    xh = (x - mean) * rstd
    gh = dh * gam
    dx_ref = rstd * (gh - gh.mean(1, keepdim=True) - xh * (gh * xh).mean(1, keepdim=True)) + c(d["dres"])
    dx1 = c(o["dx1"])
    print(f"max |dx1 - ref| {(dx1 - dx_ref).abs().max().item():.3e}")
    torch.testing.assert_close(dx1, dx_ref, rtol=2e-3, atol=2e-3)
    dg_ref, db_ref = (dh * xh).sum(0), dh.sum(0)
    dg, db = _grad(o["dgb"])[0].cpu().double(), _grad(o["dgb"])[1].cpu().double()
    print(f"max |dgamma - ref| {(dg - dg_ref).abs().max().item():.3e} (scale {dg_ref.abs().max().item():.3e}); "
          f"max |dbeta - ref| {(db - db_ref).abs().max().item():.3e} (scale {db_ref.abs().max().item():.3e})")
    torch.testing.assert_close(dg, dg_ref, rtol=2e-3, atol=2e-3 * dg_ref.abs().max().item())
    torch.testing.assert_close(db, db_ref, rtol=2e-3, atol=2e-3 * db_ref.abs().max().item())
    # the masked bf16 rows: kept elements are dx1 / (1 - p)
    dyo = c(o["dyo"])
    kept = dyo != 0
    assert abs(kept.double().mean().item() - (1.0 - p)) < 0.03
    torch.testing.assert_close(dyo[kept], (dx1 / (1.0 - p))[kept], rtol=1e-2, atol=1e-2)
    # do = dyo Wo
    do_ref = (dyo @ c(d["wod"]).view(128, 128).t()).to(BF16).double()
    print(f"max |do - ref| {(c(o['do']) - do_ref).abs().max().item():.3e}")
    torch.testing.assert_close(c(o["do"]), do_ref, rtol=2e-2, atol=2e-3)


def test_ffn_rows_backward_rejects_shapes_it_cannot_tile():
    """n1 above 512, n1 not a multiple of 128, M not a multiple of 32, a null dz: the library's error with a message, and
    nothing launched (every output still holds its NaN fill)"""
    hip = _hip()
    d = _inputs(64, 512, 0)
    big = dict(z=torch.zeros(64, 640, device="cuda").to(BF16), w2d=torch.zeros(640, 128, device="cuda").to(BF16),
               w1d=torch.zeros(128, 640, device="cuda").to(BF16))

    def call(M, n1, null_dz=False):
        o = [_nan((64, 640), BF16), _nan((64, 128), F32), _nan((64, 128), BF16), _nan((64, 128), BF16)]
        dgb = torch.zeros(32, 2, 128, device="cuda")
        try:
            hip.call("mm_ffn_rows_bwd", d["dy2"], big["w2d"], M, n1, big["z"], GELU, 0.3, 92, None if null_dz else o[0], big["w1d"],
                     d["x1"], d["stat"], d["gam"], d["dres"], 0, o[1], o[2], dgb, 0.3, 91, d["epoch"], d["wod"], o[3])
        finally:
            torch.cuda.synchronize()
            assert all(torch.isnan(t.float()).all() for t in o) and not dgb.view(torch.int32).any()
    for bad in ((64, 640), (64, 192), (48, 512), (64, 512, True)):
        with pytest.raises(hip.HipLibraryError, match="ffn_rows_bwd"):
            call(*bad)


@pytest.mark.parametrize("mode", ["manual", "graph"])
def test_trainer_steps_are_bit_identical_with_the_backward_row_fusion_off(mode, monkeypatch):
    """three tape steps / three captured steps, dropout on, at the smallest shape of test_trainer_gpu.py: the default (the
    FFN-2 data gradient heads the norm2-backward launch, and the trainer then keeps conv block 2's weight gradient on the chain)
    against the two launches with the earlier hand-over; the default does take the fused launch"""
    from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
    from multimodal_eeg_fmri_amd import _hip as hipmod, autograd, ops
    batches = [synthetic_pairs(8, 16, 256, (16, 16, 16), seed=700 + i) for i in range(3)]
    calls = []
    real = hipmod.call
    monkeypatch.setattr(hipmod, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])

    def run(off):
        monkeypatch.setattr(autograd, "_NO_FFN_ROWS_BWD", off)
        del calls[:]
        ops.set_seed_epoch(None)
        ops.set_dropout_seed(4321)
        torch.manual_seed(0)
        tr = BridgeTrainer(eeg_channels=16, dropout=0.2, lr=1e-3, mode=mode).train()
        losses = torch.stack([tr.train_step(*batches[i])["loss"].clone() for i in range(3)])
        torch.cuda.synchronize()
        params = [q.detach().clone() for m in (tr.eeg_encoder, tr.fmri_encoder, tr.head) for q in m.parameters()]
        ops.set_seed_epoch(None)
        return losses, params, calls.count("mm_ffn_rows_bwd")
    assert not autograd._NO_FFN_ROWS_BWD and not autograd._NO_GEMM2
    l0, p0, n0 = run(False)
    l1, p1, n1 = run(True)
    assert n0 > 0 and n1 == 0
    assert torch.isfinite(l0).all()
    assert torch.equal(l0, l1)
    assert len(p0) == len(p1) and all(torch.equal(a, b) for a, b in zip(p0, p1))
