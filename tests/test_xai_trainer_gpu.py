"""GPU: BridgeTrainer.explain - the attribution of each pair's eval-mode cosine similarity ze_i . zf_i to the raw EEG
epoch and the raw volume.

* method="gradient" EQUALS (same bits: the same kernels on the same batch) torch autograd through the trainer's public
  modules in eval mode, for the ERP, Power and STFT encoder kinds; "gradient_x_input", the channel means and the scores
  follow from it.
* an fp64 central finite difference of the similarity (CPU oracle in double precision, the trainer's weights) along random
  directions agrees with the signed gradient.  The HIP operands are bf16, so no bound can be derived: the relative-L2
  error of the vector of directional derivatives was measured on the MI355X against the fp64 oracle, per input: EEG
  directions 0.04576, volume directions 0.08798 (`FD_MEASURED`); each is held to 3 x its own figure, 0.1373 and 0.2639
  (the convention of tests/test_attention_masked_gpu.py); DESIGN.md section 5g.
* integrated gradients ('zero' and 'mean' baselines): `explain(chunk_steps=1)` EQUALS, bit for bit, the reference's
  protocol written in torch on the same modules - interpolate in torch, one autograd pass per step, sum in step order,
  |(x - base) * (sum / n)| (same kernels on the same batch sizes, every fp32 operation of the attribution kernels rounded
  on its own, in torch's order).  The chunked engine's difference from it is printed, not bounded here: chunk sizes are
  asserted against chunk size 1 under per-output bounds in tests/test_xai_models_gpu.py.
* train_step, explain, train_step leaves the same bits as train_step, train_step - parameters, Adam moments, optimizer
  words, BatchNorm buffers, losses, the dropout seed counter - in graph mode (the captured graph goes on replaying) and
  in manual mode, dropout on.
* after a short fit on synthetic_pairs the attribution mass is not uniform (a sanity check, no quality threshold)."""
import numpy as np
import pytest
import torch

from oracle import ref_functional as RF

from multimodal_eeg_fmri_amd import ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs

pytestmark = pytest.mark.gpu

# relative-L2 error of the directional derivatives vs the fp64 oracle (MI355X), per input; bound = 3 x its own figure
FD_MEASURED = {"eeg": 0.04576, "fmri": 0.08798}


def _trainer(kind, C=8, **kw):
    import multimodal_eeg_fmri_amd.crossmodal_v4_enhancements as Cv
    import multimodal_eeg_fmri_amd.enhanced_models_v4 as E
    torch.manual_seed(0)
    enc = {"erp": None, "power": lambda: E.EnhancedPowerEncoder(C, dropout=0.3),
           "stft": lambda: Cv.MultiScaleSTFTPowerEncoder(C, dropout=0.3)}[kind]
    return BridgeTrainer(eeg_channels=C, dropout=0.3, eeg_encoder=None if enc is None else enc(), **kw)


@pytest.mark.parametrize("kind", ["erp", "power", "stft"])
def test_gradient_equals_autograd_through_the_public_modules(kind):
    ops.set_seed_epoch(None)
    tr = _trainer(kind, mode="manual").train()
    eeg, fmri = synthetic_pairs(4, 8, 512 if kind == "stft" else 256, (16, 16, 16), seed=7)
    out = tr.explain(eeg, fmri, method="gradient")
    assert tr.training and set(out) == {"eeg", "eeg_channels", "fmri", "scores"}
    assert out["eeg"].shape == eeg.shape and out["eeg_channels"].shape == eeg.shape[:2] and out["fmri"].shape == fmri.shape
    assert out["scores"].shape == (4,) and all(t.dtype == torch.float32 and t.is_cuda for t in out.values())
    tr.eval()
    e, f = eeg.clone().requires_grad_(True), fmri.clone().requires_grad_(True)
    ze, zf = tr.head.embed(tr.eeg_encoder(e), tr.fmri_encoder(f))
    score = (ze * zf).sum(dim=1)
    ge, gf = torch.autograd.grad(score.sum(), [e, f])
    tr.train()
    print("XAI_FIG explain-vs-autograd", kind, (out["eeg"] - ge.abs()).abs().max().item(), (out["fmri"] - gf.abs()).abs().max().item(),
          ge.abs().max().item(), gf.abs().max().item())
    assert ge.abs().max().item() > 0 and gf.abs().max().item() > 0
    assert torch.equal(out["eeg"], ge.abs()) and torch.equal(out["fmri"], gf.abs())
    torch.testing.assert_close(out["scores"], score.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(out["eeg_channels"], ge.abs().mean(dim=2), rtol=1e-5, atol=0)
    gxi = tr.explain(eeg, fmri, method="gradient_x_input")
    assert torch.equal(gxi["eeg"], ge.abs() * eeg.abs()) and torch.equal(gxi["fmri"], gf.abs() * fmri.abs())
    # integrated gradients: shapes, both baselines, completeness is NOT asserted (absolute values are returned)
    for baseline in ("zero", "mean"):
        ig = tr.explain(eeg, fmri, n_steps=5, baseline=baseline)
        assert ig["eeg"].shape == eeg.shape and ig["fmri"].shape == fmri.shape and torch.isfinite(ig["eeg"]).all()
        assert (ig["eeg"] >= 0).all() and ig["eeg"].sum().item() > 0 and ig["fmri"].sum().item() > 0
        torch.testing.assert_close(ig["eeg_channels"], ig["eeg"].mean(dim=2), rtol=1e-5, atol=0)
        assert torch.equal(ig["scores"], out["scores"])
        two = tr.explain(eeg, fmri, n_steps=5, baseline=baseline, chunk_steps=2)
        assert torch.equal(two["scores"], out["scores"])
    with pytest.raises(ValueError):
        tr.explain(eeg, fmri, method="shap")
    with pytest.raises(ValueError):
        tr.explain(eeg, fmri, baseline="median")
    with pytest.raises(ValueError):
        tr.explain(eeg[:2], fmri)


def test_fp64_finite_difference_of_the_similarity_agrees_with_the_gradient():
    ops.set_seed_epoch(None)
    tr = _trainer("erp", mode="manual").train()
    eeg, fmri = synthetic_pairs(2, 8, 256, (16, 16, 16), seed=9)
    _, _, _, (ge, gf), _ = tr._pair_gradients(eeg, fmri, 1, None)
    sd = {k: v.detach().double().cpu() for k, v in tr.state_dict().items()}

    def score(e, f):
        fe = RF.erp_encoder({k[len("eeg_encoder."):]: v for k, v in sd.items() if k.startswith("eeg_encoder.")}, e)
        ff = RF.volume_encoder3d({k[len("fmri_encoder."):]: v for k, v in sd.items() if k.startswith("fmri_encoder.")}, f)
        ze, zf = RF.contrastive_head({k[len("head.bridge."):]: v for k, v in sd.items() if k.startswith("head.bridge.")}, fe, ff)
        return (ze * zf).sum(dim=1)
    e0, f0 = eeg.double().cpu(), fmri.double().cpu()
    g = torch.Generator().manual_seed(3)
    h = 1e-5
    fd, proj = [], []
    with torch.no_grad():
        for _ in range(6):
            de = torch.randn(e0.shape, generator=g, dtype=torch.float64)
            df = torch.randn(f0.shape, generator=g, dtype=torch.float64)
            for d_e, d_f in ((de, torch.zeros_like(f0)), (torch.zeros_like(e0), df)):
                fd.append((score(e0 + h * d_e, f0 + h * d_f) - score(e0 - h * d_e, f0 - h * d_f)) / (2 * h))
                proj.append((ge.double().cpu() * d_e).flatten(1).sum(1) + (gf.double().cpu() * d_f).flatten(1).sum(1))
    fd, proj = torch.stack(fd), torch.stack(proj)                      # (12 directions, B)
    err_e = ((fd[0::2] - proj[0::2]).norm() / fd[0::2].norm()).item()
    err_f = ((fd[1::2] - proj[1::2]).norm() / fd[1::2].norm()).item()
    print(f"XAI_FIG finite-difference rel_l2 eeg={err_e:.5f} fmri={err_f:.5f} bounds={[3 * v for v in FD_MEASURED.values()]}")
    assert err_e <= 3 * FD_MEASURED["eeg"], (err_e, 3 * FD_MEASURED["eeg"])
    assert err_f <= 3 * FD_MEASURED["fmri"], (err_f, 3 * FD_MEASURED["fmri"])


def _per_step_protocol(tr, eeg, fmri, n_steps, baseline):
    """the reference's integrated-gradients loop in torch on the trainer's public modules (eval mode): independent of the
    attribution kernels and of the engine"""
    be = torch.zeros_like(eeg) if baseline == "zero" else eeg.mean(dim=0, keepdim=True).expand_as(eeg)
    bf = torch.zeros_like(fmri) if baseline == "zero" else fmri.mean(dim=0, keepdim=True).expand_as(fmri)
    se, sf = torch.zeros_like(eeg), torch.zeros_like(fmri)
    tr.eval()
    for alpha in np.linspace(0, 1, n_steps):
        a = float(np.float32(alpha))
        e = (be + a * (eeg - be)).requires_grad_(True)
        f = (bf + a * (fmri - bf)).requires_grad_(True)
        ze, zf = tr.head.embed(tr.eeg_encoder(e), tr.fmri_encoder(f))
        ge, gf = torch.autograd.grad((ze * zf).sum(), [e, f])
        se, sf = se + ge, sf + gf
    tr.train()
    tr.bucket.g.zero_()
    # (tensor / tensor: an IEEE division per element; torch turns a division by a host scalar into a product with 1 / n)
    return ((eeg - be) * (se / torch.full_like(se, n_steps))).abs(), ((fmri - bf) * (sf / torch.full_like(sf, n_steps))).abs()


@pytest.mark.parametrize("baseline", ["zero", "mean"])
def test_integrated_gradients_equal_the_per_step_protocol_in_torch(baseline):
    ops.set_seed_epoch(None)
    tr = _trainer("erp", mode="manual").train()
    eeg, fmri = synthetic_pairs(4, 8, 256, (16, 16, 16), seed=13)
    want_e, want_f = _per_step_protocol(tr, eeg, fmri, 6, baseline)
    one = tr.explain(eeg, fmri, n_steps=6, baseline=baseline, chunk_steps=1)
    print("XAI_FIG explain-IG chunk=1 vs torch protocol", baseline, (one["eeg"] - want_e).abs().max().item(),
          (one["fmri"] - want_f).abs().max().item(), want_e.max().item(), want_f.max().item())
    assert want_e.max().item() > 0 and want_f.max().item() > 0
    assert torch.equal(one["eeg"], want_e) and torch.equal(one["fmri"], want_f)
    rel = lambda a, b: ((a.double() - b.double()).norm() / b.double().norm()).item()      # noqa: E731
    for chunk in (2, 6, None):
        got = tr.explain(eeg, fmri, n_steps=6, baseline=baseline, chunk_steps=chunk)
        for k, want in (("eeg", want_e), ("fmri", want_f)):
            print(f"XAI_FIG explain-IG chunk={chunk} {baseline} {k} rel_l2={rel(got[k], want):.4e}")
            assert got[k].shape == want.shape and torch.isfinite(got[k]).all()
    # a single step is the baseline alone (alpha = 0): the scores are still those of the inputs
    s1 = tr.explain(eeg, fmri, n_steps=1, baseline=baseline)
    assert torch.equal(s1["scores"], one["scores"])


@pytest.mark.parametrize("mode", ["graph", "manual"])
def test_explain_between_two_steps_leaves_the_training_state_bit_for_bit(mode):
    batches = [synthetic_pairs(8, 8, 256, (16, 16, 16), seed=200 + i) for i in range(2)]

    def run(with_explain):
        ops.set_seed_epoch(None)
        ops.set_dropout_seed(4242)
        tr = _trainer("erp", lr=1e-3, mode=mode).train()
        losses = [tr.train_step(*batches[0])["loss"].clone()]
        if with_explain:
            torch.cuda.synchronize()
            b = tr.bucket
            before = [t.clone() for t in (b.p, b.g, b.m, b.v, b.state)] + [t.clone() for t in tr.buffers()]
            seeds = dict(ops._seed_state)
            cap = tr._cap
            for method, kw in (("integrated_gradients", dict(n_steps=4, baseline="mean")), ("gradient", {})):
                out = tr.explain(*batches[1], method=method, **kw)
                assert torch.isfinite(out["eeg"]).all() and out["eeg"].sum().item() > 0
            torch.cuda.synchronize()
            after = [b.p, b.g, b.m, b.v, b.state] + list(tr.buffers())
            assert all(torch.equal(x, y) for x, y in zip(before, after))
            assert {k: v for k, v in ops._seed_state.items() if k != "epoch"} == {k: v for k, v in seeds.items() if k != "epoch"}
            assert ops._seed_state["epoch"] is seeds["epoch"] and tr._cap is cap and tr.training
            assert all(p.grad is None for p in tr.parameters())
        losses.append(tr.train_step(*batches[1])["loss"].clone())
        losses.append(tr.train_step(*batches[0])["loss"].clone())
        torch.cuda.synchronize()
        b = tr.bucket
        state = [t.clone() for t in (b.p, b.m, b.v, b.state)] + [t.detach().clone() for t in tr.buffers()]
        ops.set_seed_epoch(None)
        return torch.stack(losses), state
    l1, s1 = run(True)
    l2, s2 = run(False)
    assert torch.isfinite(l1).all() and torch.equal(l1, l2), (l1, l2)
    assert len(s1) == len(s2) and all(torch.equal(a, b) for a, b in zip(s1, s2))


def test_attribution_mass_is_not_uniform_after_a_short_fit():
    """sanity only: synthetic_pairs puts the shared latent into every time point of a channel with channel-specific
    gains, so after a few steps the per-channel shares of the attribution are not all 1 / C (no threshold on quality)"""
    ops.set_seed_epoch(None)
    torch.manual_seed(0)
    tr = BridgeTrainer(eeg_channels=8, dropout=0.0, lr=1e-3).train()
    eeg, fmri = synthetic_pairs(16, 8, 256, (16, 16, 16), seed=11)
    for _ in range(20):
        tr.train_step(eeg, fmri)
    out = tr.explain(eeg[:8], fmri[:8], n_steps=6)
    ops.set_seed_epoch(None)
    share = (out["eeg_channels"].sum(0) / out["eeg_channels"].sum()).cpu().numpy()
    print("XAI_FIG channel shares after a short fit", np.round(share, 4), "scores", out["scores"].cpu().numpy().round(3))
    assert abs(share.sum() - 1) < 1e-5 and share.max() > share.min() and np.isfinite(share).all()
    vox = out["fmri"].flatten(1)
    assert (vox.max(dim=1).values > vox.mean(dim=1)).all()
