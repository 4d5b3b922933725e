"""CPU: the host side of the attribution module (multimodal_eeg_fmri_amd/eeg_xai_analysis.py) - the
ChannelImportanceExtractor arithmetic against hand-computed arrays, the interpolation constants against np.linspace, the
memory rule that sizes the integrated-gradients batches, the public surface, and the argument checks of the new entry
points (they validate before touching the device).  None of this exists without the module."""
import ctypes
import inspect
import warnings

import numpy as np
import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
import multimodal_eeg_fmri_amd.eeg_xai_analysis as X


def test_channel_tables():
    assert len(X.STANDARD_10_20_19) == 19 and len(X.STANDARD_10_20_21) == 21 and len(X.EXTENDED_10_10_32) == 32
    assert X.STANDARD_10_20_21[:19] == X.STANDARD_10_20_19 and X.STANDARD_10_20_21[19:] == ["A1", "A2"]
    assert X.STANDARD_10_20_19[0] == "Fp1" and X.STANDARD_10_20_19[9] == "Cz" and X.STANDARD_10_20_19[-1] == "O2"
    assert X.EXTENDED_10_10_32[7:11] == ["FC5", "FC1", "FC2", "FC6"] and X.EXTENDED_10_10_32[-2:] == ["AF3", "AF4"]
    assert len(set(X.EXTENDED_10_10_32)) == 32
    assert list(X.BRAIN_REGIONS) == ["Frontal", "Central", "Temporal", "Parietal", "Occipital"]
    assert [len(v) for v in X.BRAIN_REGIONS.values()] == [10, 7, 8, 7, 5]
    for n, names in ((19, X.STANDARD_10_20_19), (21, X.STANDARD_10_20_21), (32, X.EXTENDED_10_10_32)):
        assert X.ChannelImportanceExtractor(n_channels=n).channel_names == names
    assert X.ChannelImportanceExtractor(n_channels=3).channel_names == ["Ch1", "Ch2", "Ch3"]
    assert X.ChannelImportanceExtractor(channel_names=["a", "b"]).n_channels == 2
    with pytest.raises(ValueError):
        X.ChannelImportanceExtractor()


def test_channel_importance_3d_and_2d_by_hand():
    ex = X.ChannelImportanceExtractor(channel_names=["Fz", "Cz", "Pz"])
    # two samples, three channels, two time points: time means [[1, 3, 0], [3, 1, 4]], sample means [2, 2, 2] -> 1/3 each
    a = np.array([[[0.0, 2.0], [2.0, 4.0], [0.0, 0.0]], [[2.0, 4.0], [1.0, 1.0], [3.0, 5.0]]])
    got = ex.extract_channel_importance(a)
    assert list(got) == ["Fz", "Cz", "Pz"] and all(isinstance(v, float) for v in got.values())
    np.testing.assert_allclose(list(got.values()), [1 / 3] * 3, rtol=1e-8)
    b = np.array([[[1.0, 1.0], [2.0, 4.0], [6.0, 6.0]]])                      # means [1, 3, 6] -> / (10 + 1e-8)
    np.testing.assert_allclose(list(ex.extract_channel_importance(b).values()), np.array([1, 3, 6]) / (10 + 1e-8), rtol=1e-12)
    # 2-D: (batch, channels * features) is read channel-major
    flat = b.reshape(1, 6)
    assert ex.extract_channel_importance(flat, "pw") == ex.extract_channel_importance(b)
    assert list(ex.extract_channel_importance(np.zeros((2, 3, 4))).values()) == [0.0, 0.0, 0.0]


def test_connectivity_importance_pair_order_and_normalisation():
    ex = X.ChannelImportanceExtractor(channel_names=["A", "B", "C", "D"])      # 6 pairs
    one = np.arange(1.0, 7.0)                                                  # metric 0
    attr = np.stack([np.concatenate([one, 3 * one]), np.concatenate([3 * one, 5 * one])])      # 2 samples, 2 metrics
    got = ex.extract_connectivity_importance(attr)
    assert list(got) == [("A", "B"), ("A", "C"), ("A", "D"), ("B", "C"), ("B", "D"), ("C", "D")]
    want = 3 * one                                                             # mean over metrics {2, 4} x, then samples
    np.testing.assert_allclose(list(got.values()), want / (want.sum() + 1e-8), rtol=1e-12)
    # a (batch, metrics, pairs) array is flattened the same way
    assert ex.extract_connectivity_importance(attr.reshape(2, 2, 6)) == got
    top = ex.get_top_connections(got, k=2)
    assert [p for p, _ in top] == [("C", "D"), ("B", "D")]


def test_region_means_and_top_channels():
    ex = X.ChannelImportanceExtractor(n_channels=19)
    imp = {name: float(i) for i, name in enumerate(X.STANDARD_10_20_19)}
    reg = ex.get_region_importance(imp)
    # Frontal members present: Fp1 Fp2 F7 F3 Fz F4 F8 = 0..6; Central: C3 Cz C4 = 8 9 10; Temporal: T3 T4 T5 T6 = 7 11 12 16;
    # Parietal: P3 Pz P4 = 13 14 15; Occipital: O1 O2 = 17 18
    assert reg == {"Frontal": 3.0, "Central": 9.0, "Temporal": 11.5, "Parietal": 14.0, "Occipital": 17.5}
    assert ex.get_region_importance({"Ch1": 1.0}) == {r: 0.0 for r in X.BRAIN_REGIONS}
    assert ex.get_top_channels(imp, k=3) == [("O2", 18.0), ("O1", 17.0), ("T6", 16.0)]
    assert len(ex.get_top_channels(imp)) == 5


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 8, 20, 50, 64, 100, 257, 1000])
def test_alpha_table_is_np_linspace_in_fp32(n):
    want = np.linspace(0, 1, n).astype(np.float32)
    got = ops.xai_alphas(n)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert got[0] == 0.0 and (n == 1 or got[-1] == 1.0)


def test_chunk_rule():
    """S_c = floor(budget / bytes of one step), clamped to [1, n_steps]: independent of n_steps below the clamp"""
    MB = 1 << 20
    assert ops.ig_chunk_steps(50, 226 * MB, 2048 * MB) == 9
    assert ops.ig_chunk_steps(500, 226 * MB, 2048 * MB) == 9            # follows from memory, not from n_steps
    assert ops.ig_chunk_steps(50, 3000 * MB, 2048 * MB) == 1            # one step always runs
    assert ops.ig_chunk_steps(5, 1 * MB, 2048 * MB) == 5                # never more than there are steps
    assert ops.ig_chunk_steps(50, 1024 * MB, 2048 * MB) == 2 and ops.ig_chunk_steps(50, 1025 * MB, 2048 * MB) == 1
    assert ops.ig_chunk_steps(50, 100 * MB) == (2 << 30) // (100 * MB) == ops.XAI_BUDGET_BYTES // (100 * MB)
    # the issue's example: 50 steps of one (32, 64, 1024) fp32 input are 419 MB when interpolated at once
    assert 50 * 32 * 64 * 1024 * 4 == 419_430_400
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        with pytest.raises(ValueError):
            ops.ig_chunk_steps(*bad)
    assert ops.ig_chunks(50, 9, first_alone=True) == [(0, 1), (1, 9), (10, 9), (19, 9), (28, 9), (37, 9), (46, 4)]
    assert ops.ig_chunks(8, 3) == [(0, 3), (3, 3), (6, 2)] and ops.ig_chunks(1, 4, first_alone=True) == [(0, 1)]
    for n, k, first in ((50, 9, True), (7, 7, False), (20, 1, True), (5, 8, False)):
        plan = ops.ig_chunks(n, k, first)
        assert [s for s, _ in plan] == [sum(c for _, c in plan[:i]) for i in range(len(plan))] and sum(c for _, c in plan) == n


def test_public_surface_names_and_signatures():
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()][1:]
    E = inspect.Parameter.empty
    assert params(X.GradientSaliency.__init__) == [("model", E), ("device", None)]
    for fn in (X.GradientSaliency.vanilla_gradient, X.GradientSaliency.gradient_x_input):
        assert params(fn) == [("erp", E), ("pw", E), ("conn", None), ("target_class", None)]
    assert params(X.IntegratedGradients.__init__) == [("model", E), ("device", None), ("n_steps", 50)]
    assert params(X.IntegratedGradients.compute) == [("erp", E), ("pw", E), ("conn", None), ("target_class", None), ("baseline", "zero")]
    assert params(X.SHAPExplainer.__init__) == [("model", E), ("background_data", E), ("device", None)]
    assert params(X.SHAPExplainer.compute_shap_values) == [("erp", E), ("pw", E), ("conn", None), ("n_background", 100)]
    assert params(X.ChannelImportanceExtractor.__init__) == [("channel_names", None), ("n_channels", None)]
    assert params(X.ChannelImportanceExtractor.extract_channel_importance) == [("attribution", E), ("modality", "erp")]
    assert params(X.ChannelImportanceExtractor.extract_connectivity_importance) == [("attribution", E)]
    assert params(X.ChannelImportanceExtractor.get_region_importance) == [("channel_importance", E)]
    assert params(X.ChannelImportanceExtractor.get_top_channels) == [("channel_importance", E), ("k", 5)]
    assert params(X.ChannelImportanceExtractor.get_top_connections) == [("conn_importance", E), ("k", 10)]
    assert params(X.EEGExplainer.__init__) == [("model", E), ("channel_names", None), ("n_channels", None), ("device", None)]
    assert params(X.EEGExplainer.analyze_sample) == [("erp", E), ("pw", E), ("conn", None), ("target_class", None),
                                                     ("methods", ["gradient", "integrated_gradients"])]
    assert params(X.EEGExplainer.analyze_dataset) == [("dataloader", E), ("methods", ["gradient"]), ("max_samples", 100)]
    assert params(X.EEGExplainer.get_channel_ranking) == [("modality", "erp"), ("method", "gradient")]
    for name in ("plot_channel_importance", "plot_topomap", "create_analysis_report"):       # not ported
        assert not hasattr(X, name)
    from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer
    assert params(BridgeTrainer.explain)[:5] == [("eeg", E), ("fmri", E), ("method", "integrated_gradients"), ("n_steps", 50),
                                                 ("baseline", "zero")]


def test_explainers_need_the_gpu_and_the_ranking_needs_history():
    import multimodal_eeg_fmri_amd.crossmodal_v4_enhancements as C
    m = C.EnhancedTriModalFusionNetV4Lite(8, 8, 36)
    ex = X.EEGExplainer(m, n_channels=8, device=torch.device("cpu"))
    assert not m.training and ex.channel_extractor is None and ex.results_history == []
    with pytest.raises(ValueError, match="Run analyze_sample first"):
        ex.get_channel_ranking()
    with pytest.raises(_hip.HipLibraryError):                 # no CPU fall-back
        X.GradientSaliency(m, torch.device("cpu")).vanilla_gradient(torch.randn(2, 8, 64), torch.randn(2, 8, 64), torch.randn(2, 36))
    assert not ops.attribution_active()


def test_shap_is_reported_missing_the_way_the_reference_does():
    try:
        import shap  # noqa: F401
        pytest.skip("shap is installed")
    except ImportError:
        pass
    import multimodal_eeg_fmri_amd.crossmodal_v4_enhancements as C
    m = C.EnhancedTriModalFusionNetV4Lite(8, 8, 36)
    with pytest.warns(UserWarning, match="SHAP not installed"):
        sh = X.SHAPExplainer(m, {"erp": torch.zeros(1, 8, 16), "pw": torch.zeros(1, 8, 16)}, device=torch.device("cpu"))
    assert sh._shap_available is False
    with pytest.raises(RuntimeError, match="SHAP not available"):
        sh.compute_shap_values(torch.zeros(1, 8, 16), torch.zeros(1, 8, 16))


def test_new_entry_points_refuse_invalid_arguments_before_any_launch():
    lib = _hip.load()
    p = ctypes.c_void_p(256)
    L = ctypes.c_int64
    cases = [
        ("mm_xai_interp", (None, None, 0, p, 5, 0, 5, L(2), L(8), None)),               # null x
        ("mm_xai_interp", (p, None, 0, p, 5, 3, 3, L(2), L(8), None)),                  # steps beyond n_steps
        ("mm_xai_interp", (p, None, 0, p, 0, 0, 1, L(2), L(8), None)),                  # n_steps < 1
        ("mm_xai_interp", (p, None, 0, p, 5, 0, 0, L(2), L(8), None)),                  # empty chunk
        ("mm_xai_interp", (p, None, 0, p, 5, 0, 5, L(0), L(8), None)),                  # no rows
        ("mm_xai_interp", (p, p, 3, p, 5, 0, 5, L(2), L(8), None)),                     # baseline rows neither 1 nor rows
        ("mm_xai_interp", (p, None, 2, p, 5, 0, 5, L(2), L(8), None)),                  # rows given without a baseline
        ("mm_xai_accum", (p, None, 1, L(8), None)),
        ("mm_xai_accum", (p, p, 0, L(8), None)),
        ("mm_xai_accum", (p, p, 1, L(0), None)),
        ("mm_xai_finish", (p, None, 0, p, None, None, 2, 3, L(8), 5, 0, None)),         # null attr
        ("mm_xai_finish", (p, None, 0, p, p, None, 2, 3, L(8), 5, 3, None)),            # unknown mode
        ("mm_xai_finish", (p, None, 0, p, p, None, 2, 0, L(8), 5, 0, None)),            # C = 0
        ("mm_xai_finish", (p, None, 0, p, p, None, 2, 3, L(8), 0, 0, None)),            # n_steps = 0
        ("mm_xai_finish", (p, p, 3, p, p, None, 2, 3, L(8), 5, 0, None)),               # baseline rows neither 1 nor B
        ("mm_xai_pair_score", (None, p, None, 2, 8, None)),
        ("mm_xai_pair_score", (p, p, None, 0, 8, None)),
        ("mm_xai_pair_score", (p, p, None, 2, 0, None)),
    ]
    for name, args in cases:
        rc = getattr(lib, name)(*args)
        assert rc == -1 and name[3:].encode() in lib.mm_last_error(), (name, args, rc, lib.mm_last_error())
