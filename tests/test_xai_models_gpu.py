"""GPU: GradientSaliency / IntegratedGradients of multimodal_eeg_fmri_amd.eeg_xai_analysis on the HIP path against the
reference's algorithm (EEG_CODE/eeg_xai_analysis.py:88-236) run ONE STEP AT A TIME, in fp32, on the CPU oracle model
(oracle/ref_functional.py) with the same weights - the pattern of test_f4_bridge_saliency_and_integrated_gradients_vs_oracle.

Models: EnhancedTriModalFusionNetV4 (with conn), EnhancedSmartFusionNetV4 (without), EnhancedTriModalFusionNetV4Lite.
Quirks checked: the model is called (pw, erp[, conn]); with target_class=None the class is the one predicted at alpha = 0
(the baseline); conn is not interpolated and is attributed |conn * mean_s grad|; the 'mean' baseline is the batch mean.

TOLERANCES.  The HIP operands are bf16 and the oracle is fp32, so no bound can be derived: the relative-L2 error of
EVERY output - per model, per method, erp / pw / conn separately - against the fp32 CPU oracle was measured on the MI355X
(never against the code under test) and THAT output's bound is 3 x its own figure (the convention of
tests/test_attention_masked_gpu.py, one bound per output).  The table is `MEASURED` below; its range per output kind is in
DESIGN.md section 5g: first encoder input 0.003-0.016, second encoder input 0.015-0.046, conn (fp32 kernels from end to
end) 1e-5 - 1.2e-4.  Every figure is printed before the test asserts.

BATCHING.  The engine at chunk sizes 2, 3, n_steps and the one its memory rule picks is compared with chunk size 1 (the
step-at-a-time loop through the same GPU model); each output is held to ITS OWN bound from the table (the 'mean' baseline
row).  Bit-for-bit agreement is not promised - the accumulation (mm_xai_accum) is chunk-invariant by construction and
tests/test_xai_kernels_gpu.py asserts that bit for bit, but the encoders' GEMM kernels may pick their tiling from the batch
size.  At these shapes the bits did agree for all three models when measured (the test prints it)."""
import numpy as np
import pytest
import torch

from oracle import ref_functional as RF
from oracle.fixtures import build, seeded_randn

import multimodal_eeg_fmri_amd.crossmodal_v4_enhancements as Cv
import multimodal_eeg_fmri_amd.eeg_xai_analysis as X
pytestmark = pytest.mark.gpu

N_STEPS = 6
# measured relative-L2 error of EVERY output against the fp32 CPU oracle on the MI355X: (model, method, output) -> figure;
# the bound of that output is 3 x its own figure
MEASURED = {
    ("trimodal_v4", "vanilla_gradient", "erp"): 0.00550,
    ("trimodal_v4", "vanilla_gradient", "pw"): 0.04560,
    ("trimodal_v4", "vanilla_gradient", "conn"): 0.00010,
    ("trimodal_v4", "gradient_x_input", "erp"): 0.00539,
    ("trimodal_v4", "gradient_x_input", "pw"): 0.03848,
    ("trimodal_v4", "gradient_x_input", "conn"): 0.00010,
    ("trimodal_v4", "integrated_gradients[zero]", "erp"): 0.00403,
    ("trimodal_v4", "integrated_gradients[zero]", "pw"): 0.01908,
    ("trimodal_v4", "integrated_gradients[zero]", "conn"): 0.00010,
    ("trimodal_v4", "integrated_gradients[mean]", "erp"): 0.00397,
    ("trimodal_v4", "integrated_gradients[mean]", "pw"): 0.01633,
    ("trimodal_v4", "integrated_gradients[mean]", "conn"): 0.00010,
    ("trimodal_v4", "integrated_gradients[target]", "erp"): 0.00331,
    ("trimodal_v4", "integrated_gradients[target]", "pw"): 0.02132,
    ("trimodal_v4", "integrated_gradients[target]", "conn"): 0.00012,
    ("trimodal_v4", "integrated_gradients[target=1]", "erp"): 0.00292,
    ("trimodal_v4", "integrated_gradients[target=1]", "pw"): 0.02207,
    ("trimodal_v4", "integrated_gradients[target=1]", "conn"): 0.00012,
    ("smart_v4", "vanilla_gradient", "erp"): 0.00375,
    ("smart_v4", "vanilla_gradient", "pw"): 0.03724,
    ("smart_v4", "gradient_x_input", "erp"): 0.00380,
    ("smart_v4", "gradient_x_input", "pw"): 0.03752,
    ("smart_v4", "integrated_gradients[zero]", "erp"): 0.00253,
    ("smart_v4", "integrated_gradients[zero]", "pw"): 0.02134,
    ("smart_v4", "integrated_gradients[mean]", "erp"): 0.00252,
    ("smart_v4", "integrated_gradients[mean]", "pw"): 0.02186,
    ("smart_v4", "integrated_gradients[target]", "erp"): 0.00453,
    ("smart_v4", "integrated_gradients[target]", "pw"): 0.02073,
    ("smart_v4", "integrated_gradients[target=1]", "erp"): 0.00529,
    ("smart_v4", "integrated_gradients[target=1]", "pw"): 0.02005,
    ("lite", "vanilla_gradient", "erp"): 0.01468,
    ("lite", "vanilla_gradient", "pw"): 0.03715,
    ("lite", "vanilla_gradient", "conn"): 0.00003,
    ("lite", "gradient_x_input", "erp"): 0.01386,
    ("lite", "gradient_x_input", "pw"): 0.03579,
    ("lite", "gradient_x_input", "conn"): 0.00002,
    ("lite", "integrated_gradients[zero]", "erp"): 0.01178,
    ("lite", "integrated_gradients[zero]", "pw"): 0.03216,
    ("lite", "integrated_gradients[zero]", "conn"): 0.00001,
    ("lite", "integrated_gradients[mean]", "erp"): 0.01631,
    ("lite", "integrated_gradients[mean]", "pw"): 0.01547,
    ("lite", "integrated_gradients[mean]", "conn"): 0.00002,
    ("lite", "integrated_gradients[target]", "erp"): 0.00930,
    ("lite", "integrated_gradients[target]", "pw"): 0.03702,
    ("lite", "integrated_gradients[target]", "conn"): 0.00002,
    ("lite", "integrated_gradients[target=1]", "erp"): 0.01293,
    ("lite", "integrated_gradients[target=1]", "pw"): 0.02596,
    ("lite", "integrated_gradients[target=1]", "conn"): 0.00002,
}
BOUND_FACTOR = 3.0

MODELS = {
    "trimodal_v4": (lambda: build(Cv.EnhancedTriModalFusionNetV4, 83, 8, 8, 36), lambda sd, a, b, c: RF.trimodal_v4(sd, a, b, c)[0], True),
    "smart_v4": (lambda: build(Cv.EnhancedSmartFusionNetV4, 79, 8, 8), lambda sd, a, b, c: RF.smart_fusion_v4(sd, a, b)[0], False),
    "lite": (lambda: build(Cv.EnhancedTriModalFusionNetV4Lite, 70, 8, 8, 36), lambda sd, a, b, c: RF.trimodal_lite(sd, a, b, c)[0], True),
}


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _inputs(with_conn):
    erp, pw = seeded_randn(171, 4, 8, 256), seeded_randn(172, 4, 8, 256)
    return erp, pw, (seeded_randn(173, 4, 36) if with_conn else None)


class Oracle:
    """the reference's algorithm, restated on the functional oracle: model(pw, erp[, conn]), one step at a time"""

    def __init__(self, fn, sd):
        self.fn, self.sd = fn, sd

    def grads(self, erp, pw, conn, tgt):
        erp = erp.clone().requires_grad_(True)
        pw = pw.clone().requires_grad_(True)
        conn = None if conn is None else conn.clone().requires_grad_(True)
        logits = self.fn(self.sd, pw, erp, conn)                       # power first
        if tgt is None:
            tgt = logits.argmax(dim=1)
        logits.backward(gradient=torch.zeros_like(logits).scatter_(1, tgt.view(-1, 1), 1.0))
        return erp.grad, pw.grad, (None if conn is None else conn.grad), tgt

    def saliency(self, erp, pw, conn, times_input):
        ge, gp, gc, _ = self.grads(erp, pw, conn, None)
        out = {"erp": ge.abs(), "pw": gp.abs()}
        if conn is not None:
            out["conn"] = gc.abs()
        if times_input:
            out = {k: v * {"erp": erp, "pw": pw, "conn": conn}[k].abs() for k, v in out.items()}
        return {k: v.numpy() for k, v in out.items()}

    def integrated(self, erp, pw, conn, baseline, n_steps, tgt=None):
        be = torch.zeros_like(erp) if baseline == "zero" else erp.mean(dim=0, keepdim=True).expand_as(erp)
        bp = torch.zeros_like(pw) if baseline == "zero" else pw.mean(dim=0, keepdim=True).expand_as(pw)
        acc = []
        for alpha in np.linspace(0, 1, n_steps):
            a = float(alpha)
            ge, gp, gc, tgt = self.grads(be + a * (erp - be), bp + a * (pw - bp), conn, tgt)
            acc.append((ge, gp, gc))
        out = {"erp": ((erp - be) * torch.stack([a[0] for a in acc]).mean(0)).abs().numpy(),
               "pw": ((pw - bp) * torch.stack([a[1] for a in acc]).mean(0)).abs().numpy()}
        if conn is not None:
            out["conn"] = (conn * torch.stack([a[2] for a in acc]).mean(0)).abs().numpy()
        return out, tgt


def _check(name, what, got, want, worst):
    assert set(got) == set(want), (what, set(got), set(want))
    for k in want:
        assert isinstance(got[k], np.ndarray) and got[k].shape == want[k].shape and got[k].dtype == np.float32, (what, k)
        e = rel(got[k], want[k])
        bound = BOUND_FACTOR * MEASURED[(name, what, k)]
        worst.append((e, bound, what, k))
        print(f"XAI_FIG {name} {what} {k} rel_l2={e:.4e} bound={bound:.4e}")


@pytest.mark.parametrize("name", list(MODELS))
def test_saliency_and_integrated_gradients_vs_the_reference_algorithm_on_the_oracle(name):
    make, fn, with_conn = MODELS[name]
    m = make().eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    orc = Oracle(fn, sd)
    erp, pw, conn = _inputs(with_conn)
    worst = []
    mg = m.cuda()
    sal = X.GradientSaliency(mg, torch.device("cuda"))
    _check(name, "vanilla_gradient", sal.vanilla_gradient(erp, pw, conn), orc.saliency(erp, pw, conn, False), worst)
    _check(name, "gradient_x_input", sal.gradient_x_input(erp, pw, conn), orc.saliency(erp, pw, conn, True), worst)
    ig = X.IntegratedGradients(mg, torch.device("cuda"), n_steps=N_STEPS)
    for baseline in ("zero", "mean"):
        want, tgt0 = orc.integrated(erp, pw, conn, baseline, N_STEPS)
        got = ig.compute(erp, pw, conn, baseline=baseline)
        # quirk: the class is the one predicted at alpha = 0, on both sides
        assert torch.equal(ig.last_target.cpu(), tgt0), (baseline, ig.last_target, tgt0)
        _check(name, f"integrated_gradients[{baseline}]", got, want, worst)
        # ... and giving that class explicitly is the same computation, bit for bit
        again = ig.compute(erp, pw, conn, target_class=tgt0, baseline=baseline)
        assert all(np.array_equal(got[k], again[k]) for k in got)
    # an explicit class (an int, as the reference's signature says, or one per sample)
    want, _ = orc.integrated(erp, pw, conn, "zero", N_STEPS, tgt=torch.tensor([1, 0, 1, 1]))
    _check(name, "integrated_gradients[target]", ig.compute(erp, pw, conn, target_class=torch.tensor([1, 0, 1, 1])), want, worst)
    want, _ = orc.integrated(erp, pw, conn, "zero", N_STEPS, tgt=torch.full((4,), 1))
    _check(name, "integrated_gradients[target=1]", ig.compute(erp, pw, conn, target_class=1), want, worst)
    assert all(p.grad is None for p in mg.parameters())                           # parameter .grad fields stay untouched
    over = [(what, k, e, bound) for e, bound, what, k in worst if not e <= bound]      # every figure was printed first
    assert not over, (name, over)


class _LinearProbe(torch.nn.Module):
    """logits = Linear([pw | erp]) through the HIP fp32 dense kernel: at the zero baseline the logits are the bias, so the
    class predicted there is known and differs from the inputs' own predictions"""

    def __init__(self, k):
        super().__init__()
        self.lin = torch.nn.Linear(k, 2)
        with torch.no_grad():
            self.lin.bias.copy_(torch.tensor([0.5, -0.5]))

    def forward(self, pw, erp):
        from multimodal_eeg_fmri_amd import small_autograd as sa
        return sa.linear(torch.cat([pw.flatten(1), erp.flatten(1)], dim=1), self.lin)


def test_the_class_is_fixed_at_alpha_zero_where_it_differs_from_the_inputs_class():
    """the alpha = 0 quirk where it is visible: a linear probe whose bias makes class 0 the prediction at the zero baseline
    while the inputs themselves are predicted as both classes.  fp32 kernels on both sides: rtol 1e-3, the tolerance of
    test_f4_bridge_saliency_and_integrated_gradients_vs_oracle for the same kind of kernel."""
    torch.manual_seed(5)
    m = _LinearProbe(2 * 8 * 64).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    fn = lambda sd, pw, erp, c: torch.nn.functional.linear(torch.cat([pw.flatten(1), erp.flatten(1)], 1), sd["lin.weight"], sd["lin.bias"])  # noqa: E731
    orc = Oracle(fn, sd)
    erp, pw = seeded_randn(181, 6, 8, 64) * 2, seeded_randn(182, 6, 8, 64) * 2
    _, _, _, at_input = orc.grads(erp, pw, None, None)
    _, _, _, at_base = orc.grads(torch.zeros_like(erp), torch.zeros_like(pw), None, None)
    assert at_base.tolist() == [0] * 6 and (at_input != at_base).any() and (at_input == at_base).any(), (at_input, at_base)
    ig = X.IntegratedGradients(m.cuda(), torch.device("cuda"), n_steps=8)
    got = ig.compute(erp, pw)
    assert torch.equal(ig.last_target.cpu(), at_base)
    want, _ = orc.integrated(erp, pw, None, "zero", 8)
    wrong, _ = orc.integrated(erp, pw, None, "zero", 8, tgt=at_input)
    for k in ("erp", "pw"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-3, atol=1e-6)
        assert rel(got[k], wrong[k]) > 0.1                       # (attributing the inputs' own classes is another result)
    sal = X.GradientSaliency(m, torch.device("cuda")).vanilla_gradient(erp, pw)        # saliency: the class at the input
    ws = orc.saliency(erp, pw, None, False)
    np.testing.assert_allclose(sal["erp"], ws["erp"], rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize("name", list(MODELS))
def test_chunk_sizes_and_the_step_at_a_time_loop_agree(name):
    make, fn, with_conn = MODELS[name]
    mg = make().eval().cuda()
    erp, pw, conn = _inputs(with_conn)
    ig = X.IntegratedGradients(mg, torch.device("cuda"), n_steps=N_STEPS)
    res = {}
    for chunk in (1, 2, 3, N_STEPS, None):                             # 1 = one pass per step; None = the memory rule
        ig.chunk_steps = chunk
        res[chunk] = ig.compute(erp, pw, conn, baseline="mean")
    bits, over = True, []
    for chunk in (2, 3, N_STEPS, None):
        for k in res[1]:
            e = rel(res[chunk][k], res[1][k])
            bound = BOUND_FACTOR * MEASURED[(name, "integrated_gradients[mean]", k)]       # that output's own bound
            bits = bits and np.array_equal(res[chunk][k], res[1][k])
            print(f"XAI_FIG {name} chunking chunk={chunk} {k} rel_l2={e:.3e} bound={bound:.3e}")
            if not e <= bound:
                over.append((chunk, k, e, bound))
    print(f"XAI_FIG {name} chunking bit_equal={bits}")
    assert not over, over


def test_explainer_results_and_dataset_aggregation():
    # connectivity features = 2 metrics x 28 channel pairs, the layout extract_connectivity_importance expects
    make = lambda: build(Cv.EnhancedTriModalFusionNetV4Lite, 70, 8, 8, 56)          # noqa: E731
    mg = make().eval().cuda()
    erp, pw, _ = _inputs(False)
    conn = seeded_randn(174, 4, 56)
    ex = X.EEGExplainer(mg, n_channels=8, device=torch.device("cuda"))
    ex.integrated_gradients.n_steps = N_STEPS
    r = ex.analyze_sample(erp, pw, conn)
    assert set(r) == {"attributions", "channel_importance", "region_importance", "top_channels", "prediction"}
    assert r["prediction"]["class"].shape == (4,) and r["prediction"]["probabilities"].shape == (4, 2)
    np.testing.assert_allclose(r["prediction"]["probabilities"].sum(1), 1.0, rtol=1e-5)
    for method in ("gradient", "integrated_gradients"):
        assert set(r["attributions"][method]) == {"erp", "pw", "conn"}
        ch = r["channel_importance"][method]
        assert list(ch["erp"]) == [f"Ch{i + 1}" for i in range(8)]
        # the shares are imp / (sum(imp) + 1e-8), the reference's normalisation: with attributions of an untrained net at
        # 1e-5 they sum to s / (s + 1e-8), visibly below 1 - so the values are held against that formula, not against 1
        for modality in ("erp", "pw"):
            imp = r["attributions"][method][modality].mean(axis=2).mean(axis=0)
            np.testing.assert_allclose(list(ch[modality].values()), imp / (imp.sum() + 1e-8), rtol=1e-6)
            assert 0.0 < sum(ch[modality].values()) <= 1.0 + 1e-6
        assert 0.0 < sum(ch["connectivity"].values()) <= 1.0 + 1e-6
        assert len(ch["connectivity"]) == 28 and len(r["top_channels"][method]["connectivity"]) == 10
        assert len(r["top_channels"][method]["pw"]) == 5 and set(r["region_importance"][method]["erp"]) == set(X.BRAIN_REGIONS)
    g = X.GradientSaliency(mg, torch.device("cuda")).gradient_x_input(erp, pw, conn)
    assert np.array_equal(r["attributions"]["gradient"]["erp"], g["erp"])          # 'gradient' means gradient x input
    rank = ex.get_channel_ranking("erp", "gradient")
    assert len(rank) == 8 and rank[0][1] >= rank[-1][1]
    loader = [(erp,), (erp, pw, conn, None, torch.zeros(4)), (erp, pw, conn, None, torch.zeros(4))]      # (a 1-tuple is skipped)
    ex2 = X.EEGExplainer(make().eval().cuda(), n_channels=8, device=torch.device("cuda"))
    agg = ex2.analyze_dataset(loader, methods=["gradient"], max_samples=4)
    assert agg["n_samples"] == 4 and set(agg["channel_importance"]["gradient"]) == {f"{m}_Ch{i + 1}" for m in ("erp", "pw") for i in range(8)}
    assert len(ex2.results_history) == 1


def test_a_model_without_a_tape_to_its_inputs_is_refused_not_attributed_as_zero():
    """the tabular fMRI net runs its eval forward detached: the engine raises instead of returning zero maps"""
    import multimodal_eeg_fmri_amd.fmri_utils as Fm
    m = build(Fm.fMRIFusionNet, 5, 20, 30).eval().cuda()
    with pytest.raises(RuntimeError):
        X.GradientSaliency(m, torch.device("cuda")).vanilla_gradient(seeded_randn(1, 4, 30), seeded_randn(2, 4, 20))
