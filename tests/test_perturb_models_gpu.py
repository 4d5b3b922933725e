"""GPU: crossmodal_eeg_scr.InterpretabilityAnalyzer (the EEG notebook's class) on the batched perturbation engine, for a
model with connectivity features (EnhancedTriModalFusionNetV4Lite) and one without (EnhancedSmartFusionNetV4).

* compute_channel_importance over a loader of two batches equals the notebook's loop written here on the same GPU model -
  one clone and one forward per zeroed channel, F.softmax(...)[:, 1], the per-batch mean added up and divided by the number
  of SAMPLES - within rtol 1e-5, atol 1e-6; channel_drops equals the per-sample quantities of that loop.
* against fp64 (oracle/ref_functional.py, the model's weights): the class-1 probabilities of the 2C + 1 occluded batches -
  not the drops: a drop is the difference of two nearby probabilities and its relative error says little.  The HIP
  operands are bf16, so no bound can be derived: the relative-L2 error of the (2C + 1) x B probabilities was measured on the
  MI355X per model (`MEASURED`) and is held to 3 x its own figure (the BOUND_FACTOR convention of
  tests/test_xai_models_gpu.py); DESIGN.md section 5p.  (The occluded probabilities are recovered as p_full - drop, one
  more fp32 rounding, 6e-8: far below the figures.)
* compute_channel_shapley: per modality the values sum to p(inputs) - p(all channels zeroed) within the kernel test's bound
  (the empty coalition is the first mask and runs at batch size B, like the forward it is compared with); an int
  target_class and a tensor of one class per row agree.
* compute_integrated_gradients returns what IntegratedGradients(model).compute returns."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_functional as RF
from oracle.fixtures import build, seeded_randn

import multimodal_eeg_fmri_amd.crossmodal_v4_enhancements as Cv
import multimodal_eeg_fmri_amd.eeg_xai_analysis as X
from multimodal_eeg_fmri_amd.crossmodal_eeg_scr import InterpretabilityAnalyzer

pytestmark = pytest.mark.gpu

# relative-L2 error of the class-1 probabilities of the 2C + 1 occluded batches against the fp64 oracle (MI355X)
MEASURED = {"lite": 2.7662e-06, "smart_v4": 6.6504e-05}
BOUND_FACTOR = 3.0
C, B = 8, 4
NAMES = [f"E{i}" for i in range(C)]

MODELS = {
    "lite": (lambda: build(Cv.EnhancedTriModalFusionNetV4Lite, 70, C, C, 36), lambda sd, e, p, c: RF.trimodal_lite(sd, e, p, c)[0], True),
    "smart_v4": (lambda: build(Cv.EnhancedSmartFusionNetV4, 79, C, C), lambda sd, e, p, c: RF.smart_fusion_v4(sd, e, p)[0], False),
}


def _batch(i, with_conn):
    erp, pw = seeded_randn(271 + 10 * i, B, C, 256), seeded_randn(272 + 10 * i, B, C, 256)
    subjects, labels = torch.arange(B) + B * i, torch.arange(B) % 2
    if with_conn:
        return erp, pw, seeded_randn(273 + 10 * i, B, 36), subjects, labels
    return erp, pw, subjects, labels


@pytest.fixture(scope="module", params=sorted(MODELS))
def case(request):
    make, oracle, with_conn = MODELS[request.param]
    model = make()
    an = InterpretabilityAnalyzer(model, torch.device("cuda"), NAMES)
    return request.param, an, oracle, [_batch(i, with_conn) for i in range(2)]


def _notebook_loop(model, loader, device, n_names):
    """InterpretabilityAnalyzer.compute_channel_importance of the notebook, statement for statement, keeping the per-sample
    differences as well"""
    importance_erp, importance_pw, n_samples = np.zeros(n_names), np.zeros(n_names), 0
    per_sample = []
    with torch.no_grad():
        for batch in loader:
            if len(batch) == 5:
                erp, pw, conn, subjs, ys = batch
                conn = conn.to(device)
            else:
                erp, pw, subjs, ys = batch[:4]
                conn = None
            erp, pw = erp.to(device), pw.to(device)
            logits_base = model(erp, pw, conn) if conn is not None else model(erp, pw)
            probs_base = F.softmax(logits_base, dim=1)[:, 1]
            de, dp = [], []
            for ch in range(erp.shape[1]):
                erp_masked = erp.clone()
                erp_masked[:, ch, :] = 0
                logits = model(erp_masked, pw, conn) if conn is not None else model(erp_masked, pw)
                probs = F.softmax(logits, dim=1)[:, 1]
                importance_erp[ch] += (probs_base - probs).mean().item()
                de.append(probs_base - probs)
            for ch in range(pw.shape[1]):
                pw_masked = pw.clone()
                pw_masked[:, ch, :] = 0
                logits = model(erp, pw_masked, conn) if conn is not None else model(erp, pw_masked)
                probs = F.softmax(logits, dim=1)[:, 1]
                importance_pw[ch] += (probs_base - probs).mean().item()
                dp.append(probs_base - probs)
            per_sample.append((probs_base, torch.stack(de, dim=1), torch.stack(dp, dim=1)))
            n_samples += erp.shape[0]
    return importance_erp / n_samples, importance_pw / n_samples, per_sample


def test_channel_importance_equals_the_notebooks_loop(case):
    name, an, _, loader = case
    want_e, want_p, per_sample = _notebook_loop(an.model, loader, an.device, C)
    got_e, got_p = an.compute_channel_importance(loader)
    assert isinstance(got_e, np.ndarray) and got_e.shape == (C,) and got_p.shape == (C,) and got_e.dtype == np.float64
    print(f"PERTURB_FIG {name} importance vs notebook loop: erp {np.abs(got_e - want_e).max():.3e} pw {np.abs(got_p - want_p).max():.3e} "
          f"largest {np.abs(want_e).max():.3e} {np.abs(want_p).max():.3e}")
    assert np.abs(want_e).max() > 0 and np.abs(want_p).max() > 0
    np.testing.assert_allclose(got_e, want_e, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got_p, want_p, rtol=1e-5, atol=1e-6)
    for batch, (_, de, dp) in zip(loader, per_sample):
        drops = an.channel_drops(batch[0], batch[1], batch[2] if len(batch) == 5 else None)
        assert drops["erp"].shape == (B, C) and drops["pw"].shape == (B, C) and drops["erp"].is_cuda
        torch.testing.assert_close(drops["erp"], de, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(drops["pw"], dp, rtol=1e-5, atol=1e-6)
    # the default names are the notebook's 18: the arrays have 18 entries, the channels the data lacks stay 0
    wide = InterpretabilityAnalyzer(an.model, an.device).compute_channel_importance(loader[:1])
    assert wide[0].shape == (18,) and (wide[0][C:] == 0).all() and np.abs(wide[0][:C]).max() > 0


def test_occluded_probabilities_against_fp64(case):
    name, an, oracle, loader = case
    batch = loader[0]
    erp, pw, conn = batch[0], batch[1], (batch[2] if len(batch) == 5 else None)
    with torch.no_grad():
        logits = an.model(erp.cuda(), pw.cuda(), conn.cuda()) if conn is not None else an.model(erp.cuda(), pw.cuda())
        p_full = F.softmax(logits, dim=1)[:, 1]
    drops = an.channel_drops(erp, pw, conn)
    got = torch.cat([p_full.unsqueeze(1), p_full.unsqueeze(1) - drops["erp"], p_full.unsqueeze(1) - drops["pw"]], dim=1).double().cpu()
    sd = {k: v.detach().double().cpu() for k, v in an.model.state_dict().items()}
    e64, p64, c64 = erp.double(), pw.double(), (None if conn is None else conn.double())

    def p1(e, p):
        with torch.no_grad():
            return torch.softmax(oracle(sd, e, p, c64), dim=1)[:, 1]
    cols = [p1(e64, p64)]
    for ch in range(C):
        e = e64.clone()
        e[:, ch] = 0
        cols.append(p1(e, p64))
    for ch in range(C):
        p = p64.clone()
        p[:, ch] = 0
        cols.append(p1(e64, p))
    want = torch.stack(cols, dim=1)                                    # (B, 2C + 1)
    err = ((got - want).norm() / want.norm()).item()
    print(f"PERTURB_FIG {name} occluded class-1 probabilities vs fp64: rel_l2={err:.4e} bound={BOUND_FACTOR * MEASURED[name]:.4e}")
    assert err <= BOUND_FACTOR * MEASURED[name], (err, BOUND_FACTOR * MEASURED[name])


def test_channel_shapley_is_efficient_and_takes_a_class_per_row(case):
    name, an, _, loader = case
    batch = loader[1]
    erp, pw, conn = batch[0], batch[1], (batch[2] if len(batch) == 5 else None)
    dev = [t.cuda() for t in (erp, pw)] + ([conn.cuda()] if conn is not None else [])

    def p_of(e, p, cls):
        with torch.no_grad():
            logits = an.model(e, p, dev[2]) if conn is not None else an.model(e, p)
            return F.softmax(logits, dim=1)[:, cls].double().cpu()
    phi = an.compute_channel_shapley(erp, pw, conn, n_permutations=3, seed=11)
    assert phi["erp"].shape == (B, C) and phi["pw"].shape == (B, C) and phi["erp"].dtype == torch.float32 and phi["erp"].is_cuda
    full = p_of(dev[0], dev[1], 1)
    for k, empty in (("erp", p_of(torch.zeros_like(dev[0]), dev[1], 1)), ("pw", p_of(dev[0], torch.zeros_like(dev[1]), 1))):
        v = phi[k].double().cpu()
        gap = full - empty
        scale = torch.maximum(v.abs().max(dim=1).values, gap.abs())
        print(f"PERTURB_FIG {name} shapley efficiency {k}: {(v.sum(dim=1) - gap).abs().max().item():.3e} gap {gap.abs().max().item():.3e}")
        assert ((v.sum(dim=1) - gap).abs() <= (C + 1) * 2.0 ** -24 * scale).all(), (k, v.sum(dim=1) - gap, scale)
    ones = an.compute_channel_shapley(erp, pw, conn, target_class=torch.ones(B, dtype=torch.long), n_permutations=3, seed=11)
    assert torch.equal(ones["erp"], phi["erp"]) and torch.equal(ones["pw"], phi["pw"])
    zero = an.compute_channel_shapley(erp, pw, conn, target_class=0, n_permutations=3, seed=11)
    rows = torch.tensor([0, 1, 1, 0])
    mixed = an.compute_channel_shapley(erp, pw, conn, target_class=rows, n_permutations=3, seed=11)
    is1 = rows.cuda() == 1
    for k in ("erp", "pw"):
        assert torch.equal(mixed[k][is1], phi[k][is1]) and torch.equal(mixed[k][~is1], zero[k][~is1])
    assert not torch.equal(an.compute_channel_shapley(erp, pw, conn, n_permutations=3, seed=12)["erp"], phi["erp"])


def test_integrated_gradients_are_the_xai_modules(case):
    name, an, _, loader = case
    batch = loader[0]
    erp, pw, conn = batch[0], batch[1], (batch[2] if len(batch) == 5 else None)
    got = an.compute_integrated_gradients(erp, pw, conn, target_class=1, steps=4)
    # that class calls model(pw, erp[, conn]); the analyzer calls model(erp, pw[, conn]) as the notebook does
    want = X.IntegratedGradients(an.model, an.device, n_steps=4).compute(pw, erp, conn, target_class=1)
    assert isinstance(got, tuple) and len(got) == (3 if conn is not None else 2)
    assert np.array_equal(got[0], want["pw"]) and np.array_equal(got[1], want["erp"]) and got[0].shape == tuple(erp.shape)
    if conn is not None:
        assert np.array_equal(got[2], want["conn"])
    assert np.abs(got[0]).max() > 0 and np.abs(got[1]).max() > 0
