"""GPU: the product classes (HIP path) against the reference goldens and the
CPU oracle on identical seeded inputs.  Tolerances are stated per test:
bf16 MFMA operands with fp32 accumulation give ~1e-2 relative error per
activation, and the north-star bar of cosine similarity >= 1 - 1e-4 on the
embeddings."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_functional as RF
from oracle.fixtures import build, checksum, seeded_randn

import multimodal_eeg_fmri_amd.enhanced_models_v4 as E

pytestmark = pytest.mark.gpu
COS_TOL = 1e-4


def cos_min(a, b):
    return F.cosine_similarity(a.double().flatten(1), b.double().flatten(1), dim=1).min().item()


def rel_err(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-12)).item()


@pytest.mark.parametrize("tag", ["c1", "c2"])
def test_a3_erp_encoder_eval_vs_golden(golden, tag):
    fx = golden(f"a3_erp_{tag}.npz")
    B, C, T = (int(v) for v in fx["shape"])
    m = build(E.EnhancedERPEncoder, int(fx["seed"]), C, 128, 2, 4, 0.3).eval()
    np.testing.assert_allclose(checksum(m), fx["cks"], rtol=1e-6, atol=1e-6)
    x = seeded_randn(int(fx["x_seed"]), B, C, T)
    m = m.cuda()
    with torch.no_grad():
        y = m(x.cuda()).cpu()
    want = torch.as_tensor(fx["out"])
    assert y.shape == want.shape and y.dtype == torch.float32
    c = cos_min(y, want)
    assert c >= 1 - COS_TOL, f"cosine {c}"
    assert rel_err(y, want) < 2e-2


@pytest.mark.parametrize("tag", ["c1", "c2"])
def test_a3_erp_encoder_stages_vs_golden(golden, tag):
    """the six intermediate activations the reference golden holds (enhanced_models_v4.py:169-193: after each conv block,
    after the positional add, after each transformer block) against what the HIP path materialises at the same points
    (``stages=`` hook of ops._erp_forward_impl): bf16 conv-block outputs <= 1.5e-2 rel-L2 (bf16 operands + one bf16 rounding
    of the stored activation), the fp32 residual stream <= 1e-2, cosine per sample >= 1 - 1e-4 everywhere."""
    from multimodal_eeg_fmri_amd import ops
    fx = golden(f"a3_erp_{tag}.npz")
    B, C, T = (int(v) for v in fx["shape"])
    m = build(E.EnhancedERPEncoder, int(fx["seed"]), C, 128, 2, 4, 0.3).eval().cuda()
    x = seeded_randn(int(fx["x_seed"]), B, C, T).cuda()
    stages = {}
    with torch.no_grad():
        out, _ = ops._erp_forward_impl(m, x, False, False, stages=stages)
    assert cos_min(out.cpu(), torch.as_tensor(fx["out"])) >= 1 - COS_TOL
    stride = int(fx["stride"])                           # the fixture keeps every stride-th time step / token of a stage
    for name, tol in (("conv1", 1.5e-2), ("conv2", 1.5e-2), ("conv3", 1.5e-2), ("pos", 1e-2), ("block0", 1e-2), ("block1", 1e-2)):
        want = torch.as_tensor(fx[f"stage_{name}"])
        got = stages[name].float().cpu()
        if name.startswith("conv"):                      # reference layout (B, C, T); the HIP path is channels-last
            got = got[..., :want.shape[1]].permute(0, 2, 1)[:, :, ::stride]
        else:
            got = got[:, ::stride, :]
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert cos_min(got, want) >= 1 - COS_TOL, (name, cos_min(got, want))
        assert rel_err(got, want) < tol, (name, rel_err(got, want))


def _grad_check(name, got, want, rel_tol):
    e = rel_err(got, want)
    assert e < rel_tol, f"{name}: rel err {e:.3e}"


def test_a3_erp_encoder_train_grads_vs_golden(golden):
    """train-mode (batch-stat BN, dropout 0) forward, input grad and every
    parameter grad against the reference's autograd (golden (vii)).
    Tolerance: every GEMM operand (activations AND back-propagated gradients) is
    rounded to bf16, so errors compound with depth: 5e-2 relative L2 on parameter
    gradients, 8e-2 on the input gradient (deepest, ~20 roundings)."""
    fx = golden("a3_erp_train_grads.npz")
    m = build(E.EnhancedERPEncoder, int(fx["seed"]), 8, 128, 2, 4, 0.0).train().cuda()
    x = seeded_randn(int(fx["x_seed"]), 8, 8, 256).cuda().requires_grad_(True)
    gy = seeded_randn(int(fx["gy_seed"]), 8, 128).cuda()
    y = m(x)
    y.backward(gy)
    want = torch.as_tensor(fx["out"])
    assert cos_min(y.detach().cpu(), want) >= 1 - COS_TOL
    _grad_check("dx", x.grad.cpu(), torch.as_tensor(fx["dx"]), 8e-2)
    # (1) gradient norms pinned by the reference golden
    params = dict(m.named_parameters())
    for n, gn in zip((str(n) for n in fx["gnames"]), fx["gnorms"]):
        g = params[n].grad
        assert g is not None, n
        if gn < 1e-4:      # conv biases feed BatchNorm: true gradient ~0 (rounding noise only)
            continue
        assert abs(g.double().norm().item() - gn) <= 5e-2 * gn, (n, g.double().norm().item(), gn)
    # (2) full tensors against the CPU oracle (itself pinned to the same golden on CPU)
    mo = build(E.EnhancedERPEncoder, int(fx["seed"]), 8, 128, 2, 4, 0.0).train()
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in mo.state_dict().items()}
    xo = seeded_randn(int(fx["x_seed"]), 8, 8, 256).requires_grad_(True)
    RF.erp_encoder(sd, xo, train=True).backward(gy.cpu())
    bad = []
    for n, p in params.items():
        want_g = sd[n].grad
        if want_g.norm() < 1e-4:
            continue
        e = rel_err(p.grad.cpu(), want_g)
        if e > 5e-2:
            bad.append((n, e))
    assert not bad, bad
    # BatchNorm running statistics after one training step
    m_ref_cks = fx["cks_after"]
    np.testing.assert_allclose(checksum(m.cpu()), m_ref_cks, rtol=2e-3, atol=2e-3)


import multimodal_eeg_fmri_amd.fmri_utils as Fm


@pytest.mark.parametrize("shape", [(2, 1, 16, 16, 16), (2, 1, 32, 32, 32), (1, 1, 16, 16, 24),
                                   (1, 1, 64, 64, 48)])          # last: BASELINE config #4, full-resolution volume
def test_volume_encoder_eval_vs_oracle(shape):
    """a-X1 (extension, parity unpinned by the reference): HIP path vs the CPU
    restatement (== torch.nn.Conv3d semantics). cos >= 1 - 1e-4."""
    m = build(Fm.fMRIVolumeEncoder3D, 31).eval()
    x = seeded_randn(131, *shape)
    with torch.no_grad():
        want = RF.volume_encoder3d(m.state_dict(), x)
        got = m.cuda()(x.cuda()).cpu()
    assert got.shape == want.shape
    assert cos_min(got, want) >= 1 - COS_TOL, cos_min(got, want)
    assert rel_err(got, want) < 2e-2


def _oracle_grads(fn, m, *inputs, gy, emulate, l1_as_gemm=False, widths=(32, 64, 128)):
    from oracle.bf16_emulation import bf16_operands
    import contextlib
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}
    with (bf16_operands(l1_as_gemm=l1_as_gemm, widths=widths) if emulate else contextlib.nullcontext()):
        out = fn(sd, *inputs, train=True)
        out.backward(gy)
    return out.detach(), {k: v.grad for k, v in sd.items() if v.requires_grad and v.grad is not None}


def bn_cancelled_biases(module, prefix=""):
    """names of the conv biases that feed a train-mode BatchNorm directly.  The normalisation subtracts their per-channel
    constant again, so their exact gradient is 0; an oracle's value for it is rounding noise whose size depends on the
    host's summation order (thread count), so it is no yardstick for a relative error."""
    out = set()
    for name, mod in module.named_modules():
        if not isinstance(mod, torch.nn.Sequential):
            continue
        kids = list(mod.named_children())
        for (k, conv), (_, bn) in zip(kids, kids[1:]):
            if (isinstance(conv, torch.nn.modules.conv._ConvNd) and conv.bias is not None
                    and isinstance(bn, torch.nn.modules.batchnorm._BatchNorm) and bn.training):
                out.add(f"{prefix}{name + '.' if name else ''}{k}.bias")
    return out


def zero_grad_err(got, want_weight_grad):
    """error of a gradient whose exact value is 0 (bn_cancelled_biases): its norm relative to the oracle's gradient of
    the same layer's weight"""
    return (got.double().norm() / want_weight_grad.double().norm()).item()


def _worst(named_params, want, skip_below=1e-4, zero=()):
    """worst rel-L2 error of the parameter gradients against the oracle's; names in ``zero`` are held to their exact value
    0 instead (zero_grad_err), whatever rounding noise the oracle computed for them"""
    worst = ("", 0.0)
    for n, p in named_params:
        if n in zero:
            e = zero_grad_err(p.grad.cpu(), want[n[:-len("bias")] + "weight"])
        elif n not in want or want[n].norm() < skip_below:
            continue
        else:
            e = rel_err(p.grad.cpu(), want[n])
        if e > worst[1]:
            worst = (n, e)
    return worst


def test_volume_encoder_train_grads_vs_oracle():
    """Tolerances: <= 5e-2 rel-L2 per tensor against the oracle run with bf16-rounded
    GEMM operands (what the MFMA path computes), <= 2e-1 against pure fp32 (bf16
    rounding flips 2x2x2 max-pool argmaxes, which moves whole gradient entries)."""
    m = build(Fm.fMRIVolumeEncoder3D, 32, dropout=0.0).train()
    x = seeded_randn(132, 4, 1, 16, 16, 16)
    gy = seeded_randn(133, 4, 64)
    out32, g32 = _oracle_grads(RF.volume_encoder3d, m, x, gy=gy, emulate=False)
    _, g16 = _oracle_grads(RF.volume_encoder3d, m, x, gy=gy, emulate=True)
    mg = m.cuda()
    y = mg(x.cuda())
    y.backward(gy.cuda())
    assert cos_min(y.detach().cpu(), out32) >= 1 - COS_TOL
    zero = bn_cancelled_biases(mg)
    w16 = _worst(mg.named_parameters(), g16, zero=zero)
    w32 = _worst(mg.named_parameters(), g32, zero=zero)
    assert w16[1] <= 5e-2, ("vs bf16-operand oracle", w16)
    assert w32[1] <= 2e-1, ("vs fp32 oracle", w32)
    # against the UNMODIFIED fp32 oracle with the arg-max flips isolated: the gradients of layer 3 and of the head are formed
    # upstream of both max-pools' backward, so no flipped window reaches them - they must hold the tight bound; what the
    # loose bound above absorbs is confined to layers 1 and 2 (whose gradients pass through the pools' routing)
    no_pool = [(n, q) for n, q in mg.named_parameters() if n.startswith(("conv_layers.10", "conv_layers.11", "output_proj"))]
    assert len(no_pool) == 6
    wnp = _worst(no_pool, g32, zero=zero)
    assert wnp[1] <= 5e-2, ("layer 3 / head vs the unmodified fp32 oracle", wnp)


@pytest.mark.parametrize("shape,seed", [((4, 1, 16, 16, 16), 37), ((2, 1, 32, 32, 32), 38)])
def test_volume_encoder_grads_vs_unmodified_fp32_oracle_with_hip_routing(shape, seed):
    """the 2e-1 bound of layers 1-2 against plain fp32 was max-pool arg-max flips (two near-equal window
    members swap under bf16 operands and a whole gradient entry moves).  Here the UNMODIFIED fp32 oracle - no operand
    rounding anywhere - is evaluated with the two pools routed as the HIP path routed them (its saved / exported window
    winners, ops._vol_forward_impl(winners=...)): EVERY parameter gradient, layers 1 and 2 included, <= 5e-2 rel-L2.
    The routing itself must be a genuine arg-max of the oracle's own pre-pool activations up to near-ties: in at most
    2 % of the windows the member taken is not the oracle's maximum, and then it is within 2 % of the activation scale of it."""
    from multimodal_eeg_fmri_amd import ops
    m = build(Fm.fMRIVolumeEncoder3D, seed, dropout=0.0).train()
    x = seeded_randn(100 + seed, *shape)
    gy = seeded_randn(200 + seed, shape[0], 64)
    mg = build(Fm.fMRIVolumeEncoder3D, seed, dropout=0.0).train().cuda()
    y = mg(x.cuda())
    y.backward(gy.cuda())
    winners = []
    mw = build(Fm.fMRIVolumeEncoder3D, seed, dropout=0.0).train().cuda()         # same seed -> same weights, fresh BN buffers
    with torch.no_grad():
        out_w, _ = ops._vol_forward_impl(mw, x.cuda(), True, True, winners=winners)
    assert torch.equal(out_w, y.detach())                                         # the inspected forward IS the product forward
    route = tuple(w.long().permute(0, 4, 1, 2, 3).contiguous().cpu() for w in winners)
    assert len(route) == 2 and route[0].shape[1] == 32 and route[1].shape[1] == 64
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}
    stages = {}
    out = RF.volume_encoder3d(sd, x, train=True, route=route, stages=stages)
    out.backward(gy)
    want = {k: v.grad for k, v in sd.items() if v.requires_grad and v.grad is not None}
    assert cos_min(y.detach().cpu(), out.detach()) >= 1 - COS_TOL
    w = _worst(mg.named_parameters(), want, zero=bn_cancelled_biases(mg))
    assert w[1] <= 5e-2, ("every layer vs the unmodified fp32 oracle routed as the HIP path", w)
    # the routing is the oracle's own arg-max except at near-ties: per pooled element, the member the HIP path took holds
    # the window maximum of the ORACLE's pre-pool activations up to a small gap
    for act, r in (("act1", route[0]), ("act2", route[1])):
        a = stages[act].detach()
        taken = RF.max_pool3d_routed(a, r)
        best = F.max_pool3d(a, 2)
        gap = (best - taken) / a.abs().max()
        assert (gap > 0).float().mean().item() <= 2e-2, (act, (gap > 0).float().mean().item())
        assert gap.max().item() <= 2e-2, (act, gap.max().item())


# non-default widths: (16, 32, 96) runs the generic first layer (also in training), Cin 16 weight gradients, 32 -> 96 and its
# data gradient 96 -> 32; (32, 32, 64) runs 32 -> 64 with an fp32 output on the generic kernel and its data gradient 64 -> 32
# on the streaming kernel, with the weight image in that kernel's lane order
VOLUME_WIDTHS = [(16, 32, 96), (32, 32, 64)]
VOLUME_WIDTH_SHAPES = [(16, 16, 16), (13, 18, 11)]


@pytest.mark.parametrize("dhw", VOLUME_WIDTH_SHAPES, ids=["x".join(map(str, s)) for s in VOLUME_WIDTH_SHAPES])
@pytest.mark.parametrize("widths", VOLUME_WIDTHS, ids=["-".join(map(str, w)) for w in VOLUME_WIDTHS])
def test_volume_encoder_at_other_widths_eval_vs_oracle(widths, dhw):
    """fMRIVolumeEncoder3D(widths=...) in eval mode, at the bounds of test_volume_encoder_eval_vs_oracle"""
    m = build(Fm.fMRIVolumeEncoder3D, 41, widths=widths).eval()
    x = seeded_randn(141, 2, 1, *dhw)
    with torch.no_grad():
        want = RF.volume_encoder3d(m.state_dict(), x)
        got = m.cuda()(x.cuda()).cpu()
    assert got.shape == want.shape
    print(f"ERR widths {widths} {dhw} eval: 1 - cos {1 - cos_min(got, want):.3e}, rel {rel_err(got, want):.3e}")
    assert cos_min(got, want) >= 1 - COS_TOL, cos_min(got, want)
    assert rel_err(got, want) < 2e-2


@pytest.mark.parametrize("dhw", VOLUME_WIDTH_SHAPES, ids=["x".join(map(str, s)) for s in VOLUME_WIDTH_SHAPES])
@pytest.mark.parametrize("widths", VOLUME_WIDTHS, ids=["-".join(map(str, w)) for w in VOLUME_WIDTHS])
def test_volume_encoder_at_other_widths_train_grads_vs_oracle(widths, dhw):
    """train mode, dropout 0: every parameter gradient <= 5e-2 rel-L2 against the oracle run with bf16-rounded GEMM operands
    (the bound of test_volume_encoder_train_grads_vs_oracle); w0 != 32 takes the generic first layer, which the oracle
    mirrors with l1_as_gemm; the oracle is told the widths, so that it stores in bf16 what the HIP path stores in bf16 - the
    pre-BatchNorm output of the pooled layers - whose rounding decides near-tied max-pool windows"""
    m = build(Fm.fMRIVolumeEncoder3D, 42, widths=widths, dropout=0.0).train()
    x = seeded_randn(142, 4, 1, *dhw)
    gy = seeded_randn(143, 4, 64)
    out, _ = _oracle_grads(RF.volume_encoder3d, m, x, gy=gy, emulate=False)
    _, g16 = _oracle_grads(RF.volume_encoder3d, m, x, gy=gy, emulate=True, l1_as_gemm=widths[0] != 32, widths=widths)
    mg = m.cuda()
    y = mg(x.cuda())
    y.backward(gy.cuda())
    w16 = _worst(mg.named_parameters(), g16, zero=bn_cancelled_biases(mg))
    print(f"ERR widths {widths} {dhw} train: 1 - cos {1 - cos_min(y.detach().cpu(), out):.3e}, worst gradient {w16}")
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in mg.parameters())
    assert cos_min(y.detach().cpu(), out) >= 1 - COS_TOL
    assert w16[1] <= 5e-2, ("vs bf16-operand oracle", w16)


def test_volume_encoder_train_grads_at_config4_size_vs_oracle():
    """BASELINE config #4 (full-resolution 64 x 64 x 48 volume, B = 2), train mode: the W-resident layer-2
    kernel with 12+ tiles per workgroup, the generic kernel's large-grid configurations and the
    size-dependent weight-gradient slot counts.  Output cos >= 1 - 1e-4; gradients <= 6e-2 rel-L2 vs the
    oracle with bf16-rounded operands, <= 2e-1 vs pure fp32 (max-pool argmax flips)."""
    m = build(Fm.fMRIVolumeEncoder3D, 33, dropout=0.0).train()
    x = seeded_randn(134, 2, 1, 64, 64, 48)
    gy = seeded_randn(135, 2, 64)
    out32, g32 = _oracle_grads(RF.volume_encoder3d, m, x, gy=gy, emulate=False)
    _, g16 = _oracle_grads(RF.volume_encoder3d, m, x, gy=gy, emulate=True)
    mg = m.cuda()
    y = mg(x.cuda())
    y.backward(gy.cuda())
    assert cos_min(y.detach().cpu(), out32) >= 1 - COS_TOL
    zero = bn_cancelled_biases(mg)
    w16 = _worst(mg.named_parameters(), g16, zero=zero)
    w32 = _worst(mg.named_parameters(), g32, zero=zero)
    assert w16[1] <= 6e-2, ("vs bf16-operand oracle", w16)
    assert w32[1] <= 2e-1, ("vs fp32 oracle", w32)


def test_volume_encoder_frozen_bn_backward_vs_oracle():
    """eval-mode voxel encoder with a backward to follow (frozen BatchNorm: running statistics, no dropout, no
    statistic update): parameter gradients through the fused layer-1 kernels, and - when the volume itself asks
    for a gradient (saliency / integrated gradients on an end-to-end voxel path, the protocol of
    bridge_utils.py:158-229) - d / d volume through the implicit-GEMM form of layer 1.  Against the oracle's
    eval-mode autograd with bf16-rounded operands; the running statistics must not move."""
    from oracle.bf16_emulation import bf16_operands
    m = build(Fm.fMRIVolumeEncoder3D, 36, dropout=0.3).eval()
    with torch.no_grad():                              # non-trivial running statistics
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm3d):
                mod.running_mean.copy_(seeded_randn(17, *mod.running_mean.shape) * 0.1)
                mod.running_var.copy_(1.0 + 0.2 * seeded_randn(18, *mod.running_var.shape).abs())
    x = seeded_randn(136, 3, 1, 16, 16, 16)
    gy = seeded_randn(137, 3, 64)
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}
    xo = x.clone().requires_grad_(True)
    with bf16_operands():
        out = RF.volume_encoder3d(sd, xo, train=False)
        out.backward(gy)
    want = {k: v.grad for k, v in sd.items() if v.requires_grad and v.grad is not None}
    before = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    mg = m.cuda()
    # (1) parameters only: the fused layer-1 path
    y = mg(x.cuda())
    assert y.requires_grad
    y.backward(gy.cuda())
    assert cos_min(y.detach().cpu(), out.detach()) >= 1 - COS_TOL
    w = _worst(mg.named_parameters(), want)
    assert w[1] <= 6e-2, w
    assert mg.conv_layers[0].bias.grad is not None and mg.conv_layers[0].bias.grad.abs().max().item() > 0   # not zero with a frozen BN
    # (2) the volume wants a gradient too: layer 1 as an implicit GEMM, its pre-BatchNorm tensor kept in bf16
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
    assert xg.grad is not None and xg.grad.shape == x.shape
    assert rel_err(xg.grad.cpu(), xo.grad) <= 8e-2, rel_err(xg.grad.cpu(), xo.grad)
    w = _worst(mg.named_parameters(), want)
    assert w[1] <= 6e-2, w
    for k, v in before.items():
        assert torch.equal(mg.state_dict()[k].cpu(), v), k


import multimodal_eeg_fmri_amd.bridge_utils as Bu
import multimodal_eeg_fmri_amd.crossmodal_v4_enhancements as Cv


def _close(a, b, rtol, atol, what=""):
    torch.testing.assert_close(a.detach().float().cpu(), torch.as_tensor(b), rtol=rtol, atol=atol, msg=lambda m: what + ": " + m)


def test_a4_power_encoder_eval_vs_golden(golden):
    fx = golden("a4_power.npz")
    m = build(E.EnhancedPowerEncoder, int(fx["seed"]), 64, 128, 2, 4, 0.3).eval()
    np.testing.assert_allclose(checksum(m), fx["cks"], rtol=1e-6, atol=1e-6)
    x = seeded_randn(int(fx["x_seed"]), *[int(v) for v in fx["shape"]])
    with torch.no_grad():
        y = m.cuda()(x.cuda()).cpu()
    want = torch.as_tensor(fx["out"])
    assert cos_min(y, want) >= 1 - COS_TOL, cos_min(y, want)
    assert rel_err(y, want) < 2e-2


@pytest.mark.parametrize("M", [2, 3])
def test_a5_learned_fusion_vs_golden(golden, M):
    """fp32 kernels end to end -> 1e-5."""
    fx = golden("a5_fusion.npz")
    m = build(E.LearnedFusionModule, 16 + M, M, 128, perturb=False).eval()
    with torch.no_grad():
        m.fusion_logits.copy_(torch.linspace(0.5, 1.5, M))
        m.temperature.fill_(0.7)
    feats = [seeded_randn(110 + i, 8, 128).cuda() for i in range(M)]
    with torch.no_grad():
        f, w = m.cuda()(feats, return_weights=True)
    _close(f, fx[f"fused{M}"], 1e-5, 1e-5, "fused")
    _close(w, fx[f"w{M}"], 1e-5, 1e-6, "weights")


def test_a7_trimodal_lite_eval_vs_golden(golden):
    """a6 Lite conv encoders are bf16-MFMA (2e-2 rel-L2); a7 MLP/gates are fp32."""
    fx = golden("a7_lite.npz")
    m = build(Cv.EnhancedTriModalFusionNetV4Lite, int(fx["seed"]), 8, 8, 459).eval()
    np.testing.assert_allclose(checksum(m), fx["cks"], rtol=1e-6, atol=1e-6)
    s = [int(v) for v in fx["x_seeds"]]
    erp, pw, conn = seeded_randn(s[0], 8, 8, 256).cuda(), seeded_randn(s[1], 8, 8, 256).cuda(), seeded_randn(s[2], 8, 459).cuda()
    mg = m.cuda()
    with torch.no_grad():
        e, p, c = mg.erp_encoder(erp), mg.pw_encoder(pw), mg.conn_encoder(conn)
        logits, fused = mg(erp, pw, conn, return_fused_feats=True)
        _, wdict = mg(erp, pw, conn, return_fusion_weights=True)
    _close(c, fx["conn_feat"], 1e-4, 1e-5, "conn_feat")
    assert rel_err(e.cpu(), torch.as_tensor(fx["erp_feat"])) < 2e-2
    assert rel_err(p.cpu(), torch.as_tensor(fx["pw_feat"])) < 2e-2
    assert rel_err(fused.cpu(), torch.as_tensor(fx["fused"])) < 2e-2
    assert rel_err(logits.cpu(), torch.as_tensor(fx["logits"])) < 3e-2
    assert set(wdict) == {"erp_weight", "pw_weight", "conn_weight"}


def test_a9_fmri_fusion_eval_vs_golden(golden):
    fx = golden("a9_fmri.npz")
    m = build(Fm.fMRIFusionNet, int(fx["seed"]), 100, 200).eval()
    s = [int(v) for v in fx["x_seeds"]]
    with torch.no_grad():
        out, fused = m.cuda()(seeded_randn(s[0], 8, 100).cuda(), seeded_randn(s[1], 8, 200).cuda(), return_features=True)
    _close(out, fx["out"], 1e-4, 1e-5, "out")
    _close(fused, fx["fused"], 1e-4, 1e-5, "fused")
    g = m.get_fusion_weights()
    assert abs(g["activation"] + g["connectivity"] - 1.0) < 1e-6


def test_a11_bridge_eval_vs_golden(golden):
    """all four outputs + the reference's shape smoke test (_test_bridge.py:710-727)."""
    fx = golden("a11_bridge.npz")
    m = build(Bu.EEGfMRIBridgeFusionNet, int(fx["seed"])).eval()
    np.testing.assert_allclose(checksum(m), fx["cks"], rtol=1e-6, atol=1e-6)
    s = [int(v) for v in fx["x_seeds"]]
    eeg, fmri = seeded_randn(s[0], 8, 128).cuda(), seeded_randn(s[1], 8, 64).cuda()
    mg = m.cuda()
    with torch.no_grad():
        logits, fused, fw, aw = mg(eeg, fmri, return_features=True, return_weights=True)
        only = mg(eeg, fmri)
    assert logits.shape == (8, 2) and fused.shape == (8, 128) and fw.shape == (8, 2) and aw.shape == (8, 1, 2)
    assert torch.equal(only, logits)
    _close(logits, fx["logits"], 1e-4, 1e-5, "logits")
    _close(fused, fx["fused"], 1e-4, 1e-5, "fused")
    _close(fw, fx["fusion_w"], 1e-4, 1e-6, "fusion_w")
    _close(aw, fx["attn_w"], 1e-4, 1e-6, "attn_w")
    g = mg.get_fusion_weights()
    np.testing.assert_allclose([g["eeg_weight"], g["fmri_weight"], g["temperature"]], fx["gfw"], atol=1e-6)


def test_a7_trimodal_lite_train_grads_vs_oracle():
    """train-mode (batch-stat BN, dropout 0) logits + every parameter gradient of the
    V4-Lite net against the CPU oracle's autograd; conv encoders are bf16-MFMA
    (5e-2 vs the bf16-operand oracle), the MLP/gate half is fp32."""
    from oracle.bf16_emulation import bf16_operands
    m = build(Cv.EnhancedTriModalFusionNetV4Lite, 51, 8, 8, 459, dropout=0.0).train()
    erp, pw, conn = seeded_randn(151, 8, 8, 256), seeded_randn(152, 8, 8, 256), seeded_randn(153, 8, 459)
    tgt = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1])
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}
    with bf16_operands():
        logits_o, _, _ = RF.trimodal_lite(sd, erp, pw, conn, train=True)
    loss_o = RF.label_smoothing_ce(logits_o, tgt, 0.1)
    loss_o.backward()
    mg = m.cuda()
    logits = mg(erp.cuda(), pw.cuda(), conn.cuda())
    loss = Cv.LabelSmoothingCrossEntropy(0.1)(logits, tgt.cuda())
    loss.backward()
    assert rel_err(logits.detach().cpu(), logits_o.detach()) < 3e-2
    assert abs(loss.item() - loss_o.item()) < 2e-2
    bad = []
    for n, p in mg.named_parameters():
        w = sd[n].grad
        if w is None or w.norm() < 1e-5:
            continue
        assert p.grad is not None, n
        e = rel_err(p.grad.cpu(), w)
        if e > 8e-2:
            bad.append((n, round(e, 4)))
    assert not bad, bad


def test_run_training_lite_main_trains_on_gpu(tmp_path, monkeypatch):
    """BASELINE config #1 entry point: 2 folds x 3 epochs of the real loop."""
    import multimodal_eeg_fmri_amd.run_training_lite as R
    from multimodal_eeg_fmri_amd.config import Config
    monkeypatch.chdir(tmp_path)
    cfg = Config(None)
    cfg.n_splits = 2
    cfg.learning_rate = 2e-3
    cfg.synthetic["subjects"] = 24
    res = R.main(cfg, max_epochs=3)
    assert len(res) == 2 and all(0.0 <= r["Accuracy"] <= 1.0 for r in res)


def test_run_training_lite_main_trains_from_a_disk_tree(tmp_path, monkeypatch):
    """the reference's own route through main() (run_training_lite.py:360-396): label CSV + three directories of per-file
    .mat features -> EEGDatasetERP / PW / CONN -> per-subject aggregates -> the cross-validated Lite loop, on a synthetic
    tree with BASELINE config #1's encoder shapes (8 ch x 256 samples; 465 connectivity features = the strict upper triangle of 31 x 31)."""
    from scipy.io import savemat
    import multimodal_eeg_fmri_amd.run_training_lite as R
    from multimodal_eeg_fmri_amd.config import Config
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(3)
    root = tmp_path / "data"
    for d in ("erp", "pw", "conn"):
        (root / d).mkdir(parents=True)
    rows = ["subject,label"]
    for subj in range(1, 17):
        y = subj % 2
        rows.append(f"{subj},{3 if y else 1}")                    # load_labels(binary=True): <= 1 -> 0, else 1
        shift = 0.5 * (2 * y - 1)
        for f in ("1_Hz", "2_Hz"):
            savemat(root / "erp" / f"ERP_sub{subj:03d}_alpha_{f}.mat", {"ERP": rng.standard_normal((8, 256)) + shift})
            savemat(root / "pw" / f"pw_sub{subj:03d}_alpha_{f}.mat", {"powspctrm": rng.standard_normal((8, 256)) - shift})
        for c in ("open", "close"):
            m = rng.standard_normal((31, 31)) + shift
            savemat(root / "conn" / f"conn_sub{subj:03d}_alpha_{c}.mat", {"conn": m + m.T})
    (root / "labels.csv").write_text("\n".join(rows) + "\n")
    cfg = Config(None)
    cfg.eeg_path_erp, cfg.eeg_path_pw, cfg.eeg_path_conn, cfg.label_path = root / "erp", root / "pw", root / "conn", root / "labels.csv"
    cfg.subject_list, cfg.bands, cfg.eeg_segments = list(range(1, 17)), {"alpha": "Alpha"}, ["1_Hz", "2_Hz"]
    cfg.n_splits, cfg.learning_rate = 2, 2e-3
    res = R.main(cfg, max_epochs=3)                               # source="auto": the directories exist -> disk
    assert len(res) == 2 and all(0.0 <= r["Accuracy"] <= 1.0 for r in res)
    ds = R.load_disk_dataset(cfg)
    assert len(ds) == 16 and ds[0]["erp"].shape == (8, 256) and ds[0]["pw"].shape == (8, 256) and ds[0]["conn"].shape == (465,)


@pytest.mark.parametrize("shape", [(2, 8, 512), (2, 64, 1024)])       # second: BASELINE config #5 (6 272 conv input channels)
def test_aX3_stft_front_end_and_encoder_vs_oracle(shape):
    """extension a-X3 (parity unpinned by the reference; pinned to torch.stft): raw spectra to 2e-2 rel (bf16
    storage); z-scored spectra (normalize_modality, run_training_lite.py:48-51, 162) to 2e-2 abs; the
    encoder output on top of them to cosine >= 1 - 1e-4 - the north-star tolerance - also at the config-#5
    workload (64 ch x 1024 samples, n_fft 64 & 128, hop 32)."""
    from multimodal_eeg_fmri_amd import ops
    B, C, T = shape
    x = seeded_randn(161, B, C, T)
    spec = torch.cat([RF.stft_power(x, n, 32) for n in (64, 128)], dim=1)          # (B, C*F, frames)
    got = ops.stft_front_end(x.cuda(), (64, 128), 32).float().cpu()              # (B, frames, Cp)
    want = spec.transpose(1, 2)
    assert got.shape[1] == want.shape[1] == T // 32 + 1
    torch.testing.assert_close(got[:, :, :want.shape[2]], want, rtol=2e-2, atol=2e-2)
    gotn = ops.stft_front_end(x.cuda(), (64, 128), 32, normalize=True).float().cpu()
    wantn = RF.normalize_modality(spec).transpose(1, 2)
    torch.testing.assert_close(gotn[:, :, :wantn.shape[2]], wantn, rtol=1e-2, atol=2e-2)
    assert abs(gotn[:, :, :wantn.shape[2]].mean().item()) < 1e-2
    m = build(Cv.MultiScaleSTFTPowerEncoder, 61, C).eval()
    assert m.normalize and m.spec_channels == C * (33 + 65)
    with torch.no_grad():
        want_y = RF.stft_power_encoder(m.state_dict(), x)
        y = m.cuda()(x.cuda()).cpu()
    assert y.shape == (B, 128)
    assert cos_min(y, want_y) >= 1 - COS_TOL, cos_min(y, want_y)
    assert rel_err(y, want_y) < 2e-2


def test_aX3_gradient_wrt_raw_eeg_through_the_stft_front_end():
    """d / d raw EEG of the config-#5 model (eval mode, frozen BatchNorm: the saliency / integrated-gradients protocol of
    bridge_utils.py:158-229 on an end-to-end path): STFT power at two scales -> per-sample z-score -> EnhancedPowerEncoder,
    against autograd through the oracle (torch.stft) with bf16-rounded GEMM operands: rel-L2 <= 1e-1, cosine >= 0.99."""
    from oracle.bf16_emulation import bf16_operands
    B, C, T = 2, 8, 512
    m = build(Cv.MultiScaleSTFTPowerEncoder, 63, C, dropout=0.3).eval()
    x = seeded_randn(164, B, C, T)
    gy = seeded_randn(165, B, 128)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    xo = x.clone().requires_grad_(True)
    with bf16_operands():
        want = RF.stft_power_encoder(sd, xo, train=False)
        want.backward(gy)
    mg = m.cuda()
    xg = x.cuda().requires_grad_(True)
    y = mg(xg)
    y.backward(gy.cuda())
    assert cos_min(y.detach().cpu(), want.detach()) >= 1 - COS_TOL
    assert xg.grad is not None and xg.grad.shape == x.shape and torch.isfinite(xg.grad).all().item()
    e = rel_err(xg.grad.cpu(), xo.grad)
    c = F.cosine_similarity(xg.grad.cpu().flatten().double(), xo.grad.flatten().double(), dim=0).item()
    assert e <= 1e-1 and c >= 0.99, (e, c)


def test_aX3_config5_train_step_gradients_vs_oracle():
    """config #5 at its workload in TRAIN mode (batch-statistic BatchNorm, dropout 0): forward and every
    parameter gradient of the power encoder behind the STFT front-end vs the oracle with bf16-rounded GEMM
    operands (6e-2 rel-L2; gradients stop at the spectra)."""
    B, C, T = 2, 64, 1024
    m = build(Cv.MultiScaleSTFTPowerEncoder, 62, C, dropout=0.0).train()
    x = seeded_randn(162, B, C, T)
    gy = seeded_randn(163, B, 128)
    from oracle.bf16_emulation import bf16_operands
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}
    with bf16_operands():
        want = RF.stft_power_encoder(sd, x, train=True)
        want.backward(gy)
    mg = m.cuda()
    y = mg(x.cuda())
    y.backward(gy.cuda())
    assert cos_min(y.detach().cpu(), want.detach()) >= 1 - COS_TOL
    bad = [(n, rel_err(q.grad.cpu(), sd[n].grad)) for n, q in mg.named_parameters()
           if sd[n].grad is not None and sd[n].grad.norm() >= 1e-5 and rel_err(q.grad.cpu(), sd[n].grad) > 6e-2]
    assert not bad, bad


def test_a11_bridge_train_grads_vs_reference_golden(golden):
    """golden (vii): weighted-CE loss, input gradients and every parameter gradient norm of
    the bridge in train mode (dropout 0) as computed by the REFERENCE's autograd; plus full
    tensors vs the oracle.  fp32 kernels -> 1e-3."""
    fx = golden("a11_bridge_train_grads.npz")
    m = build(Bu.EEGfMRIBridgeFusionNet, int(fx["seed"]), dropout=0.0).train()
    m.fusion.gate_net[2].p = 0.0                      # hard-coded Dropout(0.2) (enhanced_models_v4.py:449)
    s = [int(v) for v in fx["x_seeds"]]
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}
    eo = seeded_randn(s[0], 8, 128).requires_grad_(True)
    fo = seeded_randn(s[1], 8, 64).requires_grad_(True)
    tgt, cw = torch.as_tensor(fx["target"]), torch.as_tensor(fx["class_w"])
    F.cross_entropy(RF.bridge_net(sd, eo, fo)[0], tgt, weight=cw).backward()
    mg = m.cuda()
    eeg = seeded_randn(s[0], 8, 128).cuda().requires_grad_(True)
    fmri = seeded_randn(s[1], 8, 64).cuda().requires_grad_(True)
    loss = Bu.WeightedCrossEntropy(cw.cuda())(mg(eeg, fmri), tgt.cuda())
    loss.backward()
    assert abs(loss.item() - float(fx["loss"])) < 1e-4
    torch.testing.assert_close(eeg.grad.cpu(), torch.as_tensor(fx["d_eeg"]), rtol=1e-3, atol=1e-5)
    torch.testing.assert_close(fmri.grad.cpu(), torch.as_tensor(fx["d_fmri"]), rtol=1e-3, atol=1e-5)
    params = dict(mg.named_parameters())
    for n, gn in zip((str(n) for n in fx["gnames"]), fx["gnorms"]):
        g = params[n].grad
        assert g is not None, n
        assert abs(g.double().norm().item() - gn) <= 1e-3 * max(gn, 1e-3), (n, g.double().norm().item(), gn)
        torch.testing.assert_close(g.cpu(), sd[n].grad, rtol=2e-3, atol=2e-5, msg=lambda t: n + ": " + t)


def test_a9_fmri_fusion_trains():
    m = build(Fm.fMRIFusionNet, 71, 100, 200, dropout=0.0).train()
    act, con = seeded_randn(171, 16, 100), seeded_randn(172, 16, 200)
    tgt = (seeded_randn(173, 16) > 0).long()
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}
    out_o, _ = RF.fmri_fusion_net(sd, act, con, train=True)
    F.cross_entropy(out_o, tgt).backward()
    mg = m.cuda()
    out = mg(act.cuda(), con.cuda())
    loss = Bu.WeightedCrossEntropy()(out, tgt.cuda())
    loss.backward()
    torch.testing.assert_close(out.detach().cpu(), out_o.detach(), rtol=1e-3, atol=1e-4)
    for n, p in mg.named_parameters():
        torch.testing.assert_close(p.grad.cpu(), sd[n].grad, rtol=5e-3, atol=5e-5, msg=lambda t: n + ": " + t)


def test_a4_power_encoder_train_grads_vs_oracle():
    """a4 training (three conv scales run as one merged k=7 conv + one BatchNorm(192), gradients
    sliced back): output, input gradient, every parameter gradient and the BatchNorm running
    statistics against the oracle's autograd.  Tolerances as for a3: <= 5e-2 rel-L2 per tensor vs
    the bf16-operand oracle, cosine >= 1 - 1e-4 on the output vs the fp32 oracle."""
    m = build(E.EnhancedPowerEncoder, 44, 16, 128, 2, 4, 0.0).train()
    x = seeded_randn(144, 4, 16, 128)
    gy = seeded_randn(145, 4, 128)
    xo = x.clone().requires_grad_(True)
    out32, _ = _oracle_grads(RF.power_encoder, m, xo, gy=gy, emulate=False)
    xe = x.clone().requires_grad_(True)
    _, g16 = _oracle_grads(RF.power_encoder, m, xe, gy=gy, emulate=True)
    # BatchNorm running statistics after one training step, from torch's own leaf ops
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        hs = []
        for name, pad in (("conv_scale1", 1), ("conv_scale2", 2), ("conv_scale3", 3)):
            yc = F.conv1d(x, sd[f"{name}.0.weight"], sd[f"{name}.0.bias"], padding=pad)
            hs.append(F.gelu(F.batch_norm(yc, sd[f"{name}.1.running_mean"], sd[f"{name}.1.running_var"],
                                          sd[f"{name}.1.weight"], sd[f"{name}.1.bias"], training=True)))
        yc = F.conv1d(torch.cat(hs, dim=1), sd["fusion.0.weight"], sd["fusion.0.bias"])
        F.batch_norm(yc, sd["fusion.1.running_mean"], sd["fusion.1.running_var"], sd["fusion.1.weight"],
                     sd["fusion.1.bias"], training=True)
    mg = m.cuda()
    xg = x.cuda().requires_grad_(True)
    y = mg(xg)
    y.backward(gy.cuda())
    assert cos_min(y.detach().cpu(), out32) >= 1 - COS_TOL
    w16 = _worst(mg.named_parameters(), g16, zero=bn_cancelled_biases(mg))
    assert w16[1] <= 5e-2, ("vs bf16-operand oracle", w16)
    _grad_check("dx", xg.grad.cpu(), xe.grad, 8e-2)
    for name in ("conv_scale1.1", "conv_scale2.1", "conv_scale3.1", "fusion.1"):
        for buf in ("running_mean", "running_var"):
            got = dict(mg.named_buffers())[f"{name}.{buf}"].cpu()
            torch.testing.assert_close(got, sd[f"{name}.{buf}"], rtol=2e-2, atol=2e-3, msg=f"{name}.{buf}")
        assert dict(mg.named_buffers())[f"{name}.num_batches_tracked"].item() == 1


def test_a3_erp_encoder_frozen_bn_backward_vs_oracle():
    """eval-mode encoder with a backward to follow (frozen BatchNorm: running statistics, no
    dropout): the saliency / fine-tuning path (bridge_utils.py:158-229).  Input gradient and
    parameter gradients vs the oracle's eval-mode autograd; running statistics must not move."""
    m = build(E.EnhancedERPEncoder, 45, 8, 128, 2, 4, 0.3).eval()
    with torch.no_grad():                              # non-trivial running statistics
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.copy_(seeded_randn(7, *mod.running_mean.shape) * 0.1)
                mod.running_var.copy_(1.0 + 0.2 * seeded_randn(8, *mod.running_var.shape).abs())
    x = seeded_randn(146, 4, 8, 256)
    gy = seeded_randn(147, 4, 128)
    from oracle.bf16_emulation import bf16_operands
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}
    xo = x.clone().requires_grad_(True)
    with bf16_operands():
        out = RF.erp_encoder(sd, xo, train=False)
        out.backward(gy)
    before = {k: v.clone() for k, v in m.state_dict().items() if "running" in k}
    mg = m.cuda()
    xg = x.cuda().requires_grad_(True)
    y = mg(xg)
    y.backward(gy.cuda())
    assert cos_min(y.detach().cpu(), out.detach()) >= 1 - COS_TOL
    _grad_check("dx", xg.grad.cpu(), xo.grad, 8e-2)
    want = {k: v.grad for k, v in sd.items() if v.requires_grad and v.grad is not None}
    w = _worst(mg.named_parameters(), want)
    assert w[1] <= 5e-2, w
    for k, v in before.items():
        assert torch.equal(mg.state_dict()[k].cpu(), v), k


def test_aX3_stft_power_encoder_trains():
    """config #5: the STFT front-end feeds a TRAINING power encoder (gradients stop at the spectra);
    a few fused-AdamW steps on a fixed batch reduce a regression loss."""
    from multimodal_eeg_fmri_amd.optim import FusedAdamW
    torch.manual_seed(0)
    m = Cv.MultiScaleSTFTPowerEncoder(8, dropout=0.1).cuda().train()
    x = seeded_randn(171, 4, 8, 512).cuda()
    target = seeded_randn(172, 4, 128).cuda()
    opt = FusedAdamW(m.parameters(), lr=2e-3, weight_decay=0.0, max_grad_norm=1.0)
    losses = []
    for _ in range(8):
        opt.zero_grad()
        loss = ((m(x) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses


@pytest.mark.parametrize("tag,name,n_in", [("trimodal_v4", "EnhancedTriModalFusionNetV4", 3),
                                            ("smart_v4", "EnhancedSmartFusionNetV4", 2)])
def test_f1_full_v4_classifiers_vs_reference_golden(golden, tag, name, n_in):
    """EnhancedTriModalFusionNetV4 / EnhancedSmartFusionNetV4 (a3 + a4 encoders, 1xK
    modality cross attention, learned fusion, BN-MLP head) on the HIP path.
    eval: logits / fusion weights / fused features vs the reference golden (cosine >= 1 - 1e-4 on the
    fused features; logits 3e-2 abs: two bf16 encoders feed a 5-layer fp32 head);
    train (dropout 0): every parameter-gradient norm within 6e-2 of the reference's autograd."""
    fx = golden(f"f1_{tag}.npz")
    args = (8, 8, 36) if n_in == 3 else (8, 8)
    m = build(getattr(Cv, name), int(fx["seed"]), *args).eval()
    np.testing.assert_allclose(checksum(m), fx["cks"], rtol=1e-6, atol=1e-6)
    s = [int(v) for v in fx["x_seeds"]]
    xs = [seeded_randn(s[0], 4, 8, 256), seeded_randn(s[1], 4, 8, 256)] + ([seeded_randn(s[2], 4, 36)] if n_in == 3 else [])
    with torch.no_grad():
        logits, weights, fused = m.cuda()(*[x.cuda() for x in xs], return_fusion_weights=True, return_fused_feats=True)
    assert cos_min(fused.cpu(), torch.as_tensor(fx["fused"])) >= 1 - COS_TOL
    _close(weights, fx["weights"], 1e-2, 2e-3, "fusion weights")
    _close(logits, fx["logits"], 3e-2, 3e-2, "logits")
    mt = build(getattr(Cv, name), int(fx["train_seed"]), *args, dropout=0.0).train().cuda()
    mt.fusion.gate_net[2].p = 0.0
    out = mt(*[x.cuda() for x in xs])
    out.backward(seeded_randn(int(fx["gy_seed"]), 4, 2).cuda())
    params = dict(mt.named_parameters())
    bad = []
    for n, gn in zip((str(v) for v in fx["t_gnames"]), fx["t_gnorms"]):
        if gn < 1e-4:
            continue
        g = params[n].grad
        assert g is not None, n
        e = abs(g.double().norm().item() - gn) / gn
        # 2- and 3-element tensors (fusion logits / last gate bias) sit at the end of the whole bf16 chain and
        # have no averaging over elements: 1e-1 for those, 6e-2 for every real weight tensor
        if e > (1e-1 if g.numel() <= 4 else 6e-2):
            bad.append((n, e))
    assert not bad, bad


def test_f2_batched_frozen_feature_extraction_matches_per_sample_loop():
    """extract_eeg_features / extract_fmri_features run every subject's samples in GPU
    batches; the result must equal the reference's one-forward-per-sample loop (same kernels, eval-mode
    BatchNorm: rows are independent) and feed BridgeFeatureDataset."""
    import multimodal_eeg_fmri_amd.fmri_utils as Fm2
    torch.manual_seed(3)
    eeg_model = Bu.ImprovedTriModalFusionNet(8, 8, 36, fusion_dim=128).cuda().eval()
    assert next(iter(eeg_model.state_dict())).startswith("model.")           # checkpoint key prefix
    g = torch.Generator().manual_seed(4)
    raw = []
    for subj, n in ((11, 3), (12, 1), (15, 4)):
        samples = [(torch.randn(8, 256, generator=g).numpy(), torch.randn(8, 256, generator=g).numpy(),
                    torch.randn(9, 4, generator=g).numpy()) for _ in range(n)]
        raw.append((samples, None, None, subj % 2, subj))
    got = Bu.extract_eeg_features(eeg_model, raw, "cuda", batch_size=5)
    assert sorted(got) == [11, 12, 15]
    with torch.no_grad():
        for samples, _, _, _, subj in raw:
            per = [eeg_model(erp=torch.tensor(e)[None].cuda(), pw=torch.tensor(p)[None].cuda(),
                             conn=torch.tensor(c).reshape(1, -1).cuda(), return_feats=True)["fused_feats"].cpu()
                   for e, p, c in samples]
            torch.testing.assert_close(got[subj], torch.cat(per).mean(0), rtol=1e-4, atol=1e-4)
    fm = Fm2.fMRIFusionNet(20, 30).cuda().eval()
    act = {s: torch.randn(20, generator=g) for s in (11, 12, 13)}
    conn = {s: torch.randn(30, generator=g) for s in (11, 12, 15)}
    ff = Bu.extract_fmri_features(fm, act, conn, [11, 12, 13, 15], "cuda", batch_size=2)
    assert sorted(ff) == [11, 12] and ff[11].shape == (64,)
    ds = Bu.BridgeFeatureDataset(got, ff, {11: 1, 12: 0}, [11, 12, 13, 15])
    assert len(ds) == 2 and ds[0][0].shape == (128,) and ds[0][1].shape == (64,)


def test_f4_bridge_saliency_and_integrated_gradients_vs_oracle():
    """BridgeGradientSaliency / BridgeIntegratedGradients on the HIP path (eval-mode
    backward of the bridge; IG's 50 interpolation points as one batch) against the reference
    algorithm (bridge_utils.py:158-229) run on the CPU oracle.  fp32 kernels: 1e-3 / 2e-3."""
    m = build(Bu.EEGfMRIBridgeFusionNet, 51).eval()
    eeg, fmri = seeded_randn(151, 6, 128), seeded_randn(152, 6, 64)
    sd = m.state_dict()

    def ref_grads(e, f, tgt):
        e = e.clone().requires_grad_(True); f = f.clone().requires_grad_(True)
        logits = RF.bridge_net(sd, e, f)[0]
        if tgt is None:
            tgt = logits.argmax(dim=1)
        logits.backward(gradient=torch.zeros_like(logits).scatter_(1, tgt.view(-1, 1), 1.0))
        return e.grad, f.grad, tgt
    ge, gf, tgt = ref_grads(eeg, fmri, None)
    mg = m.cuda()
    sal = Bu.BridgeGradientSaliency(mg, "cuda").compute(eeg, fmri)
    np.testing.assert_allclose(sal["eeg"], ge.abs().numpy(), rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(sal["fmri"], gf.abs().numpy(), rtol=1e-3, atol=1e-5)
    assert all(p.grad is None or True for p in mg.parameters())
    # integrated gradients, the reference loop on the oracle
    n_steps, tgt_ig, acc_e, acc_f = 20, None, [], []
    for alpha in np.linspace(0, 1, n_steps):
        a_e, a_f, tgt_ig = ref_grads(float(alpha) * eeg, float(alpha) * fmri, tgt_ig)
        acc_e.append(a_e); acc_f.append(a_f)
    want_e = (eeg * torch.stack(acc_e).mean(0)).abs().numpy()
    want_f = (fmri * torch.stack(acc_f).mean(0)).abs().numpy()
    ig = Bu.BridgeIntegratedGradients(mg, "cuda", n_steps=n_steps).compute(eeg, fmri)
    np.testing.assert_allclose(ig["eeg"], want_e, rtol=2e-3, atol=1e-5)
    np.testing.assert_allclose(ig["fmri"], want_f, rtol=2e-3, atol=1e-5)


# ------------------------------------------------------------------ round 2: a1 / a2 stand-alone, C2-shaped gradients
def test_a1_positional_encoding_standalone_vs_reference_golden(golden):
    """PositionalEncoding.forward as its own module (enhanced_models_v4.py:44-55), both layout branches,
    fp32 kernel: 1e-5 abs (the sinusoid table is rebuilt by the host's libm, whose sin/cos differ by an ulp
    between CPUs; the add itself is exact); train mode: the output is (x + pe) * keep-mask and backward
    applies the same mask."""
    fx = golden("a1a2_standalone.npz")
    m = E.PositionalEncoding(128, dropout=0.1).eval().cuda()
    s1, s2 = (int(v) for v in fx["pe_x_seeds"])
    xb, xs = seeded_randn(s1, 2, 96, 128).cuda(), seeded_randn(s2, 40, 1, 128).cuda()
    with torch.no_grad():
        _close(m(xb), fx["pe_out_bf"], 0, 1e-5, "batch-first")
        _close(m(xs), fx["pe_out_sf"], 0, 1e-5, "(seq, 1, d)")
    m.train()
    xg = xb.clone().requires_grad_(True)
    y = m(xg)
    want = torch.as_tensor(fx["pe_out_bf"]).cuda()
    kept = y != 0
    frac = kept.float().mean().item()
    assert 0.87 < frac < 0.93, frac                                   # p = 0.1
    torch.testing.assert_close(y[kept], (want / 0.9)[kept], rtol=1e-5, atol=1e-5)
    y.sum().backward()
    torch.testing.assert_close(xg.grad, kept.float() / 0.9, rtol=1e-6, atol=0)
    with pytest.raises(ValueError):
        m(torch.zeros(2, 6000, 128, device="cuda"))                   # longer than max_len


@pytest.mark.parametrize("tag", ["none", "causal", "float"])
def test_a2_transformer_block_standalone_and_masked_vs_reference_golden(golden, tag):
    """TemporalTransformerBlock.forward(x, mask) as its own module (enhanced_models_v4.py:88-105): eval
    output cos >= 1 - 1e-4 and rel-L2 <= 2e-2 (bf16 MFMA operands); train-mode (dropout 0) input gradient
    and parameter-gradient norms against the reference's autograd (5e-2)."""
    from oracle.make_goldens_r2 import masks
    fx = golden("a1a2_standalone.npz")
    msk = masks(96)[tag]
    m = build(E.TemporalTransformerBlock, int(fx["blk_seed"]), 128, 4, 512, 0.1).eval().cuda()
    x = seeded_randn(int(fx["blk_x_seed"]), 2, 96, 128)
    with torch.no_grad():
        y = m(x.cuda(), None if msk is None else msk.cuda()).cpu()
    want = torch.as_tensor(fx[f"blk_out_{tag}"])
    assert cos_min(y, want) >= 1 - COS_TOL, cos_min(y, want)
    assert rel_err(y, want) < 2e-2
    mt = build(E.TemporalTransformerBlock, int(fx["blk_train_seed"]), 128, 4, 512, 0.0).train().cuda()
    xg = x.cuda().requires_grad_(True)
    mt(xg, None if msk is None else msk.cuda()).backward(seeded_randn(int(fx["blk_gy_seed"]), 2, 96, 128).cuda())
    _grad_check("dx", xg.grad.cpu(), torch.as_tensor(fx[f"blk_dx_{tag}"]), 5e-2)
    params = dict(mt.named_parameters())
    for n, gn in zip((str(n) for n in fx[f"blk_{tag}_gnames"]), fx[f"blk_{tag}_gnorms"]):
        g = params[n].grad
        assert g is not None, n
        assert abs(g.double().norm().item() - gn) <= 5e-2 * gn + 1e-6, (n, g.double().norm().item(), gn)


@pytest.mark.parametrize("kind", ["float", "bool"])
def test_a2_transformer_block_with_a_per_head_mask_vs_oracle(kind):
    """nn.MultiheadAttention's 3-D attn_mask, (batch * heads, L, L) - one matrix per head of each sample (the reference
    itself only passes the 2-D form, enhanced_models_v4.py:98; this is the other form its MultiheadAttention accepts).
    L = 160: two key chunks with a ragged second one, queries over two workgroups.  Eval output cos >= 1 - 1e-4 and
    rel-L2 <= 2e-2; train-mode (dropout 0) input and parameter gradients 5e-2, against the CPU oracle (whose 3-D branch
    is pinned to torch.nn.MultiheadAttention by tests/test_oracle_golden.py).  A wrong leading size is refused."""
    B, L, H = 3, 160, 4
    g = torch.Generator().manual_seed(5)
    if kind == "float":
        msk = torch.randn(B * H, L, L, generator=g)
    else:
        msk = torch.rand(B * H, L, L, generator=g) < 0.3
        msk[:, torch.arange(L), torch.arange(L)] = False
    m = build(E.TemporalTransformerBlock, 21, 128, H, 512, 0.0).train().cuda()
    sd = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    x = seeded_randn(22, B, L, 128)
    gy = seeded_randn(23, B, L, 128)
    xo = x.clone().requires_grad_(True)
    want = RF.transformer_block(sd, "", xo, H, mask=msk)
    want.backward(gy)
    with torch.no_grad():
        y = m.eval()(x.cuda(), msk.cuda()).cpu()
    assert cos_min(y, want.detach()) >= 1 - COS_TOL, cos_min(y, want.detach())
    assert rel_err(y, want.detach()) < 2e-2
    xg = x.cuda().requires_grad_(True)
    m.train()(xg, msk.cuda()).backward(gy.cuda())
    _grad_check("dx", xg.grad.cpu(), xo.grad, 5e-2)
    for n, p in m.named_parameters():
        _grad_check(n, p.grad.cpu(), sd[n].grad, 5e-2)
    with pytest.raises(ValueError, match="batch \\* heads"):
        m(x.cuda(), msk[:H].cuda())


def test_a3_erp_encoder_train_grads_at_c2_shape_vs_reference_golden(golden):
    """the train-mode forward + backward at the shape bench.py times (64 ch x 1024 samples: L = 512 full-tile
    attention specialisation, the size-dependent slot counts of the weight-gradient kernels), against the
    REFERENCE's autograd: output cos >= 1 - 1e-4, input gradient 8e-2, every parameter-gradient norm 5e-2,
    full tensors vs the CPU oracle 5e-2, BatchNorm running statistics after the step."""
    fx = golden("a3_erp_train_grads_c2.npz")
    B, C, T = (int(v) for v in fx["shape"])
    m = build(E.EnhancedERPEncoder, int(fx["seed"]), C, 128, 2, 4, 0.0).train().cuda()
    x = seeded_randn(int(fx["x_seed"]), B, C, T).cuda().requires_grad_(True)
    gy = seeded_randn(int(fx["gy_seed"]), B, 128)
    y = m(x)
    y.backward(gy.cuda())
    assert cos_min(y.detach().cpu(), torch.as_tensor(fx["out"])) >= 1 - COS_TOL
    _grad_check("dx", x.grad.cpu()[:, :, ::8], torch.as_tensor(fx["dx_t8"]), 8e-2)
    params = dict(m.named_parameters())
    for n, gn in zip((str(n) for n in fx["gnames"]), fx["gnorms"]):
        if gn < 1e-4:
            continue
        g = params[n].grad
        assert abs(g.double().norm().item() - gn) <= 5e-2 * gn, (n, g.double().norm().item(), gn)
    mo = build(E.EnhancedERPEncoder, int(fx["seed"]), C, 128, 2, 4, 0.0).train()
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in mo.state_dict().items()}
    RF.erp_encoder(sd, seeded_randn(int(fx["x_seed"]), B, C, T), train=True).backward(gy)
    bad = [(n, rel_err(p.grad.cpu(), sd[n].grad)) for n, p in params.items()
           if sd[n].grad.norm() >= 1e-4 and rel_err(p.grad.cpu(), sd[n].grad) > 5e-2]
    assert not bad, bad
    np.testing.assert_allclose(checksum(m.cpu()), fx["cks_after"], rtol=2e-3, atol=2e-3)


def test_a3_erp_encoder_with_dropout_matches_masked_oracle():
    """every nn.Dropout site of the train-mode encoder (conv blocks, positional, attention probabilities,
    dropout1 / FFN / dropout2, head; enhanced_models_v4.py:132-143, 55, 71-73, 99-105, 166) with p = 0.3
    (what bench.py times): the HIP forward equals the CPU oracle evaluated with the SAME keep-masks (host
    replica of the counter hash, oracle/dropout_replica.py) and backward differentiates that function.
    Tolerances: output cos >= 1 - 1e-4; gradients 6e-2 rel-L2 vs the oracle with bf16-rounded GEMM operands."""
    from multimodal_eeg_fmri_amd import ops
    from oracle.bf16_emulation import bf16_operands
    from oracle.dropout_replica import erp_encoder_train_with_masks
    p = 0.3
    B, C, T = 4, 16, 256
    m = build(E.EnhancedERPEncoder, 51, C, 128, 2, 4, p).train()
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}
    x = seeded_randn(151, B, C, T)
    gy = seeded_randn(152, B, 128)
    seeds = []
    real = ops._next_seed

    def logged():
        s = real()
        seeds.append(s)
        return s
    ops.set_seed_epoch(None)
    ops.set_dropout_seed(777)
    ops._next_seed = logged
    try:
        mg = m.cuda()
        xg = x.cuda().requires_grad_(True)
        y = mg(xg)
        y.backward(gy.cuda())
    finally:
        ops._next_seed = real
    assert len(seeds) == 3 + 1 + 4 * 2 + 1, seeds
    xo = x.clone().requires_grad_(True)
    with bf16_operands():
        want = erp_encoder_train_with_masks(sd, xo, seeds, p, p, p)
        want.backward(gy)
    assert (y == 0).float().mean().item() > 0.2                       # the head's own dropout happened
    assert cos_min(y.detach().cpu(), want.detach()) >= 1 - COS_TOL, cos_min(y.detach().cpu(), want.detach())
    _grad_check("dx", xg.grad.cpu(), xo.grad, 8e-2)
    bad = [(n, rel_err(q.grad.cpu(), sd[n].grad)) for n, q in mg.named_parameters()
           if sd[n].grad is not None and sd[n].grad.norm() >= 1e-4 and rel_err(q.grad.cpu(), sd[n].grad) > 6e-2]
    assert not bad, bad


def _log_seeds(fn):
    """run fn() with ops._next_seed logging the dropout seeds it hands out (draw order)"""
    from multimodal_eeg_fmri_amd import ops
    seeds = []
    real = ops._next_seed

    def logged():
        v = real()
        seeds.append(v)
        return v
    ops.set_seed_epoch(None)
    ops.set_dropout_seed(4242)
    ops._next_seed = logged
    try:
        out = fn()
    finally:
        ops._next_seed = real
    return out, seeds


def test_volume_encoder_with_dropout_matches_masked_oracle():
    """the voxel encoder's four nn.Dropout sites (after each pooled / un-pooled conv block and after the head) at p = 0.3,
    the rate bench.py times: the fused layer-1 kernel, the pooled layer-2 pass (pool3d_bn_act), the layer-3
    BatchNorm pass and the pooled head all draw counter-hash masks; the HIP forward equals the CPU oracle evaluated with
    the SAME masks (oracle/dropout_replica.py) and backward differentiates that function.  Output cos >= 1 - 1e-4;
    gradients <= 6e-2 rel-L2 vs the oracle with bf16-rounded operands."""
    from oracle.bf16_emulation import bf16_operands
    from oracle.dropout_replica import volume_encoder_train_with_masks
    p = 0.3
    m = build(Fm.fMRIVolumeEncoder3D, 37, dropout=p).train()
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}
    x = seeded_randn(138, 4, 1, 16, 16, 16)
    gy = seeded_randn(139, 4, 64)
    mg = m.cuda()

    def run():
        y = mg(x.cuda())
        y.backward(gy.cuda())
        return y
    y, seeds = _log_seeds(run)
    assert len(seeds) == 4, seeds
    with bf16_operands():
        want = volume_encoder_train_with_masks(sd, x, seeds, p)
        want.backward(gy)
    assert 0.15 < (y == 0).float().mean().item() < 0.45               # the head's own dropout happened
    assert torch.equal((y == 0).cpu(), (want == 0))                    # ... with exactly the replica's mask
    assert cos_min(y.detach().cpu(), want.detach()) >= 1 - COS_TOL, cos_min(y.detach().cpu(), want.detach())
    bad = [(n, rel_err(q.grad.cpu(), sd[n].grad)) for n, q in mg.named_parameters()
           if sd[n].grad is not None and sd[n].grad.norm() >= 1e-4 and rel_err(q.grad.cpu(), sd[n].grad) > 6e-2]
    assert not bad, bad
