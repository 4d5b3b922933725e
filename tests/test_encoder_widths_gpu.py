"""GPU: the EEG transformer encoders, the v4 fusion classifier and the contrastive trainer at widths other than
128 x 4 heads (head dims 16, 24, 64 and 16 at 128 x 8): the non-128 paths of ops / autograd and the head-dim-generic
attention kernels (mm_attn_fwd_hd / mm_attn_bwd_hd), against the CPU oracle as in test_models_gpu.py /
test_trainer_gpu.py / test_checkpoint_gpu.py."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_functional as RF
from oracle.bf16_emulation import bf16_operands
from oracle.fixtures import build, seeded_randn

import multimodal_eeg_fmri_amd.crossmodal_v4_enhancements as Cv
import multimodal_eeg_fmri_amd.enhanced_models_v4 as E
from multimodal_eeg_fmri_amd import ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
from multimodal_eeg_fmri_amd.crossmodal_eeg_scr import ImprovedSmartFusionNet
from test_models_gpu import COS_TOL, _grad_check, _worst, bn_cancelled_biases, cos_min, zero_grad_err
from test_trainer_gpu import _bn_cancelled

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_seed_epoch():
    ops.set_seed_epoch(None)
    yield
    ops.set_seed_epoch(None)


def _oracle(fn, m, x, gy, nhead, emulate):
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}
    with (bf16_operands() if emulate else contextlib.nullcontext()):
        out = fn(sd, x, nhead=nhead, train=True)
        out.backward(gy)
    return out.detach(), {k: v.grad for k, v in sd.items() if v.requires_grad and v.grad is not None}


ENCODERS = [("erp", 64, 4), ("erp", 96, 4), ("erp", 256, 4), ("erp", 128, 8), ("power", 64, 4), ("power", 256, 4)]


@pytest.mark.parametrize("kind,hidden,heads", ENCODERS, ids=[f"{k}-{h}x{n}" for k, h, n in ENCODERS])
def test_encoder_at_width_vs_oracle(kind, hidden, heads):
    """eval output vs the fp32 oracle (cos >= 1 - 1e-4); train mode (dropout 0): output, input gradient, every parameter
    gradient and the BatchNorm running statistics vs the bf16-operand oracle (<= 5e-2 rel-L2 per tensor)"""
    cls, fn = (E.EnhancedERPEncoder, RF.erp_encoder) if kind == "erp" else (E.EnhancedPowerEncoder, RF.power_encoder)
    C, T = 8, 256
    m = build(cls, 60 + hidden + heads, C, hidden, 2, heads, 0.0)
    x = seeded_randn(170 + hidden, 4, C, T)
    # eval
    m.eval()
    with torch.no_grad():
        want = fn(m.state_dict(), x, nhead=heads)
        got = m.cuda()(x.cuda()).cpu()
    assert got.shape == (4, hidden)
    assert cos_min(got, want) >= 1 - COS_TOL, cos_min(got, want)
    # train
    m = m.cpu().train()
    gy = seeded_randn(171 + hidden, 4, hidden)
    xo = x.clone().requires_grad_(True)
    out32, _ = _oracle(fn, m, xo, gy, heads, emulate=False)
    xe = x.clone().requires_grad_(True)
    out16, g16 = _oracle(fn, m, xe, gy, heads, emulate=True)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    mg = m.cuda()
    xg = x.cuda().requires_grad_(True)
    y = mg(xg)
    y.backward(gy.cuda())
    assert cos_min(y.detach().cpu(), out32) >= 1 - COS_TOL
    assert ((y.detach().cpu().double() - out16.double()).norm() / out16.double().norm()).item() <= 5e-2
    w16 = _worst(mg.named_parameters(), g16, zero=bn_cancelled_biases(mg))
    assert w16[1] <= 5e-2, ("vs bf16-operand oracle", w16)
    _grad_check("dx", xg.grad.cpu(), xe.grad, 8e-2)
    _check_running_stats(mg, sd, x, kind)


def _check_running_stats(mg, sd, x, kind):
    """each BatchNorm's running statistics after the step = torch's train-mode batch_norm on the oracle's input to it"""
    with torch.no_grad():
        if kind == "erp":
            h = x
            seq = [("conv_layers.0", "conv_layers.1", 3, None), ("conv_layers.4", "conv_layers.5", 2, 2),
                   ("conv_layers.9", "conv_layers.10", 1, None)]
            for conv, bn, pad, pool in seq:
                yc = F.conv1d(h, sd[f"{conv}.weight"], sd[f"{conv}.bias"], padding=pad)
                rm, rv = sd[f"{bn}.running_mean"].clone(), sd[f"{bn}.running_var"].clone()
                h = F.gelu(F.batch_norm(yc, rm, rv, sd[f"{bn}.weight"], sd[f"{bn}.bias"], training=True))
                if pool:
                    h = F.max_pool1d(h, pool)
                _stats_close(mg, bn, rm, rv)
        else:
            hs = []
            for name, pad in (("conv_scale1", 1), ("conv_scale2", 2), ("conv_scale3", 3)):
                yc = F.conv1d(x, sd[f"{name}.0.weight"], sd[f"{name}.0.bias"], padding=pad)
                rm, rv = sd[f"{name}.1.running_mean"].clone(), sd[f"{name}.1.running_var"].clone()
                hs.append(F.gelu(F.batch_norm(yc, rm, rv, sd[f"{name}.1.weight"], sd[f"{name}.1.bias"], training=True)))
                _stats_close(mg, f"{name}.1", rm, rv)
            yc = F.conv1d(torch.cat(hs, dim=1), sd["fusion.0.weight"], sd["fusion.0.bias"])
            rm, rv = sd["fusion.1.running_mean"].clone(), sd["fusion.1.running_var"].clone()
            F.batch_norm(yc, rm, rv, sd["fusion.1.weight"], sd["fusion.1.bias"], training=True)
            _stats_close(mg, "fusion.1", rm, rv)


def _stats_close(mg, bn, rm, rv):
    bufs = dict(mg.named_buffers())
    torch.testing.assert_close(bufs[f"{bn}.running_mean"].cpu(), rm, rtol=2e-2, atol=2e-3, msg=f"{bn}.running_mean")
    torch.testing.assert_close(bufs[f"{bn}.running_var"].cpu(), rv, rtol=2e-2, atol=2e-3, msg=f"{bn}.running_var")
    assert bufs[f"{bn}.num_batches_tracked"].item() == 1


@pytest.mark.parametrize("wrapper", [False, True], ids=["v4", "improved"])
def test_smart_fusion_at_width_64_vs_oracle(wrapper):
    """EnhancedSmartFusionNetV4(hidden_dim=64) / ImprovedSmartFusionNet(fusion_dim=64), eval, vs ref_functional.smart_fusion_v4"""
    if wrapper:
        torch.manual_seed(81)
        m = ImprovedSmartFusionNet(8, 8, fusion_dim=64, dropout=0.3).eval()
        core, pre = m.model, "model."
    else:
        m = build(Cv.EnhancedSmartFusionNetV4, 82, 8, 8, hidden_dim=64).eval()
        core, pre = m, ""
    erp, pw = seeded_randn(183, 4, 8, 256), seeded_randn(184, 4, 8, 256)
    with torch.no_grad():
        logits_w, weights_w, fused_w = RF.smart_fusion_v4(m.state_dict(), erp, pw, pre)
        if wrapper:
            r = m.cuda()(erp.cuda(), pw.cuda(), return_feats=True)
            logits, weights, fused = r["logits"], r["gates"], r["fused_feats"]
        else:
            logits, weights, fused = core.cuda()(erp.cuda(), pw.cuda(), return_fusion_weights=True, return_fused_feats=True)
    assert fused.shape == (4, 64)
    assert cos_min(fused.cpu(), fused_w) >= 1 - COS_TOL
    torch.testing.assert_close(weights.cpu(), weights_w, rtol=1e-2, atol=2e-3)
    torch.testing.assert_close(logits.cpu(), logits_w, rtol=3e-2, atol=3e-2)


TRAINERS = [(64, 4), (256, 4), (128, 8)]
TR_IDS = [f"{h}x{n}" for h, n in TRAINERS]
SMALL = (8, 16, 256, (16, 16, 16))


def _make(hidden, heads, mode, dropout, seed=0, lr=1e-3, C=16):
    torch.manual_seed(seed)
    return BridgeTrainer(eeg_channels=C, hidden_dim=hidden, num_heads=heads, dropout=dropout, lr=lr, mode=mode).train()


def _oracle_step(tr, eeg, fmri, nhead, emulate):
    sd = {}
    for pre, m in (("e.", tr.eeg_encoder), ("f.", tr.fmri_encoder), ("h.", tr.head)):
        for k, v in m.state_dict().items():
            sd[pre + k] = v.detach().cpu().clone().requires_grad_(v.is_floating_point())
    with (bf16_operands() if emulate else contextlib.nullcontext()):
        fe = RF.erp_encoder(sd, eeg.cpu(), "e.", nhead=nhead, train=True)
        ff = RF.volume_encoder3d(sd, fmri.cpu(), "f.", train=True)
        ze, zf = RF.contrastive_head(sd, fe, ff, "h.bridge.")
        loss = RF.clip_loss(ze, zf, ze, zf, sd["h.logit_scale"].exp())[0]
        loss.backward()
    return loss.item(), ze.detach(), zf.detach(), {k: v.grad for k, v in sd.items() if v.requires_grad and v.grad is not None}


@pytest.mark.parametrize("hidden,heads", TRAINERS, ids=TR_IDS)
def test_trainer_step_at_width_vs_oracle(hidden, heads):
    """one step at dropout 0 on the tape: loss (1e-3), embeddings (cos >= 1 - 1e-4 vs fp32), every parameter gradient of
    the flat bucket <= 6e-2 rel-L2 vs the bf16-operand oracle"""
    B, C, T, vol = SMALL
    tr = _make(hidden, heads, "manual", 0.0, C=C)
    eeg, fmri = synthetic_pairs(B, C, T, vol, seed=4500 + hidden)
    l32, ze32, zf32, _ = _oracle_step(tr, eeg, fmri, heads, emulate=False)
    _, _, _, g16 = _oracle_step(tr, eeg, fmri, heads, emulate=True)
    with torch.no_grad():
        z, saved = tr._seg_forward(eeg, fmri)
        dz = torch.empty_like(z)
        tr._seg_loss(z, tr._scal, dz)
        tr._seg_backward(saved, dz, tr._scal)
        ops.arena.end()
    torch.cuda.synchronize()
    N = tr.head.bridge.bridge_dim
    cos_e = F.cosine_similarity(z[:, :N].cpu().double(), ze32.double(), dim=1).min().item()
    cos_f = F.cosine_similarity(z[:, N:].cpu().double(), zf32.double(), dim=1).min().item()
    assert cos_e >= 1 - 1e-4 and cos_f >= 1 - 1e-4, (cos_e, cos_f)
    assert abs(tr._scal[0].item() - l32) <= 1e-3 * max(1.0, abs(l32)), (tr._scal[0].item(), l32)
    named = {}
    for pre, m in (("e.", tr.eeg_encoder), ("f.", tr.fmri_encoder), ("h.", tr.head)):
        named.update({pre + k: v for k, v in m.named_parameters()})
    zero = _bn_cancelled(tr)
    worst, checked = ("", 0.0), 0
    for n, p in named.items():
        sink = getattr(p, "_mm_grad", None)
        if sink is None or n not in g16 or (n not in zero and g16[n].norm() < 1e-5):
            continue
        got = sink.detach().cpu().view(g16[n].shape).double()
        if n in zero:
            e = zero_grad_err(got, g16[n[:-len("bias")] + "weight"])
        else:
            e = ((got - g16[n].double()).norm() / g16[n].double().norm()).item()
        worst = max(worst, (n, e), key=lambda t: t[1])
        checked += 1
    assert checked >= 50, checked
    assert worst[1] <= 6e-2, ("vs bf16-operand oracle", worst)


@pytest.mark.parametrize("hidden,heads", TRAINERS, ids=TR_IDS)
def test_trainer_graph_equals_manual_at_width(hidden, heads):
    """dropout 0: the captured two-stream step replays what the eager tape computes, bit for bit, over four steps.
    Dropout 0.3: two graph-mode trainers from the same seeds replay the same bits (with dropout, graph and tape draw their
    seeds at different points of the stream - the capture's warm-up steps draw first - at every width)"""
    B, C, T, vol = SMALL
    batches = [synthetic_pairs(B, C, T, vol, seed=4600 + i) for i in range(2)]

    def run(mode, dropout):
        ops.set_dropout_seed(31)
        tr = _make(hidden, heads, mode, dropout, C=C)
        losses = [tr.train_step(*batches[i % 2])["loss"].clone() for i in range(4)]
        torch.cuda.synchronize()
        if mode == "graph":
            assert tr.capture_mode == "one graph"
        ops.set_seed_epoch(None)
        return torch.stack(losses), tr.bucket.p.detach().clone()

    a, b = run("manual", 0.0), run("graph", 0.0)
    assert torch.isfinite(a[0]).all()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c, d = run("graph", 0.3), run("graph", 0.3)
    assert torch.isfinite(c[0]).all() and not torch.equal(c[0], a[0])
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1])


@pytest.mark.parametrize("D", [32, 96, 160, 192, 224, 320])
def test_layernorm_at_width_vs_fp64(D):
    """mm_layernorm_fwd / _bwd at widths that are not 128 (the generic kernels; 96, 160, 224 are not multiples of 64)"""
    from multimodal_eeg_fmri_amd import _hip
    M = 300
    g = torch.Generator().manual_seed(D)
    x = torch.randn(M, D, generator=g) * 2 + 0.5
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
    dy = torch.randn(M, D, generator=g)
    xr = x.double().requires_grad_(True)
    y = F.layer_norm(xr, (D,), gamma.double(), beta.double(), 1e-5)
    y.backward(dy.double())
    xg = x.cuda()
    out = torch.full((M, D), float("nan"), device="cuda")
    stat = torch.empty(M, 2, device="cuda")
    _hip.call("mm_layernorm_fwd", xg, gamma.cuda(), beta.cuda(), None, out, stat, M, D, 1e-5)
    dx = torch.full((M, D), float("nan"), device="cuda")
    _hip.call("mm_layernorm_bwd", None, dy.cuda(), xg, stat, gamma.cuda(), None, dx, None, None, M, D, 0.0, 0, None)
    torch.cuda.synchronize()
    torch.testing.assert_close(out.cpu().double(), y.detach(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(dx.cpu().double(), xr.grad, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("hidden,heads", TRAINERS, ids=TR_IDS)
def test_trainer_learns_at_width(hidden, heads):
    """the loss falls over 30 graph-mode steps on a fixed set of synthetic pairs; embed / evaluate_retrieval run"""
    B, C, T, vol = SMALL
    ops.set_dropout_seed(5)
    tr = _make(hidden, heads, "graph", 0.1, lr=1e-3, C=C)
    batches = [synthetic_pairs(B, C, T, vol, seed=4700 + i) for i in range(4)]
    losses = torch.stack([tr.train_step(*batches[i % 4])["loss"].clone() for i in range(32)])
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all()
    assert losses[-4:].mean().item() < 0.9 * losses[:4].mean().item(), losses.tolist()
    eeg = torch.cat([b[0] for b in batches])
    fmri = torch.cat([b[1] for b in batches])
    ze, zf = tr.embed(eeg, fmri)
    assert ze.shape[0] == zf.shape[0] == 4 * B and torch.isfinite(ze).all() and torch.isfinite(zf).all()
    r = tr.evaluate_retrieval(eeg, fmri)
    assert r


@pytest.mark.parametrize("hidden,heads", TRAINERS, ids=TR_IDS)
def test_trainer_resume_at_width_is_exact(tmp_path, hidden, heads):
    B, C, T, vol = SMALL
    batches = [synthetic_pairs(B, C, T, vol, seed=4800 + i) for i in range(3)]

    def steps(tr, i0, k):
        out = [tr.train_step(*batches[i % 3])["loss"].clone() for i in range(i0, i0 + k)]
        torch.cuda.synchronize()
        return torch.stack(out)

    def snap(tr):
        b = tr.bucket
        return [t.detach().clone() for t in (b.p, b.m, b.v, b.state)] + [v.detach().clone() for v in tr.state_dict().values()]

    ops.set_dropout_seed(2024)
    a = _make(hidden, heads, "graph", 0.3, seed=0, C=C)
    steps(a, 0, 4)
    path = str(tmp_path / "ck.pt")
    a.save_checkpoint(path, epoch=1)
    want = steps(a, 4, 4)
    want_state = snap(a)
    b = _make(hidden, heads, "graph", 0.3, seed=11, C=C)
    ops.set_dropout_seed(77)
    b.load_checkpoint(path)
    got = steps(b, 4, 4)
    assert torch.isfinite(want).all()
    assert torch.equal(want, got), (want, got)
    for i, (x, y) in enumerate(zip(want_state, snap(b))):
        assert torch.equal(x, y), i
    other = _make(hidden, 8 if heads == 4 else 4, "manual", 0.3, C=C)      # same shapes, other head count
    with pytest.raises(ValueError, match="heads"):
        other.load_checkpoint(path)
