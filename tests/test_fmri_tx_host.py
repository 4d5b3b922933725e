"""CPU: host side of the fMRI notebook's transformer models (multimodal_eeg_fmri_amd/crossmodal_fmri_scr.py) - state_dict
layout against the notebook fixture, argument validation, the swapped-argument rule, subject splits, the subject vote and
the C header."""
import os
import types

import numpy as np
import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, fmri_utils, ops
from multimodal_eeg_fmri_amd import crossmodal_fmri_scr as X
from multimodal_eeg_fmri_amd import small_autograd as sa

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f5_fmri_notebook.npz")
H, L, A, C = 32, 2, 30, 21


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def _layout(sd):
    return [(k, ",".join(str(d) for d in v.shape)) for k, v in sd.items()]


def test_state_dict_names_and_shapes_equal_the_notebooks(gold):
    net = X.fMRIFusionNet(A, C, hidden_dim=H, num_transformer_layers=L)
    assert _layout(net.state_dict()) == list(zip(gold["sd_names"].tolist(), gold["sd_shapes"].tolist()))
    assert len(net.state_dict()) == 73
    assert "activation_encoder.transformer.layers.0.self_attn.in_proj_weight" in net.state_dict()
    assert sum(q.numel() for q in net.parameters()) == 59572
    for cls, d in ((X.fMRIActivationOnly, A), (X.fMRIConnectivityOnly, C)):
        single = cls(d, hidden_dim=H, num_layers=L)
        names = [k for k, _ in _layout(single.state_dict())]
        assert names == gold["single_names"].tolist()
    assert _layout(X.fMRIActivationOnly(A, hidden_dim=H, num_layers=L).state_dict()) == \
        list(zip(gold["single_names"].tolist(), gold["single_shapes"].tolist()))


def test_notebook_checkpoint_loads_strictly_and_the_mlp_class_still_refuses_it(gold):
    sd = {k: torch.from_numpy(gold["w/" + k]) for k in gold["sd_names"]}
    net = X.fMRIFusionNet(A, C, hidden_dim=H, num_transformer_layers=L)
    res = net.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(RuntimeError, match="activation_encoder.transformer.layers.0.self_attn.in_proj_weight"):
        fmri_utils.fMRIFusionNet(A, C, hidden_dim=H).load_state_dict(sd)
    assert len(fmri_utils.fMRIFusionNet(A, C, hidden_dim=H).state_dict()) != 73         # the MLP family is unchanged


def test_constructor_defaults_and_validation():
    import inspect
    sig = inspect.signature(X.fMRIFusionNet.__init__).parameters
    assert [(k, sig[k].default) for k in list(sig)[3:]] == [("hidden_dim", 64), ("num_classes", 2), ("dropout", 0.3),
                                                            ("num_transformer_layers", 2), ("num_heads", 4),
                                                            ("task", "classification")]
    for cls in (X.fMRIActivationOnly, X.fMRIConnectivityOnly):
        sig = inspect.signature(cls.__init__).parameters
        assert [(k, sig[k].default) for k in list(sig)[2:]] == [("hidden_dim", 64), ("num_classes", 2), ("dropout", 0.4),
                                                                ("task", "classification"), ("num_layers", 2)]
    assert list(inspect.signature(X.ActivationEncoder.__init__).parameters)[1:] == ["num_layers", "in_dim", "hidden_dim", "dropout"]
    assert issubclass(X.ConnectivityEncoder, X.ActivationEncoder)
    with pytest.raises(ValueError, match="hidden_dim"):
        X.ActivationEncoder(2, 10, 48, 0.1)
    with pytest.raises(ValueError, match="num_layers"):
        X.ActivationEncoder(0, 10, 64, 0.1)
    with pytest.raises(ValueError, match="num_layers"):
        X.fMRIActivationOnly(10, num_layers=9)
    with pytest.raises(ValueError, match="in_dim"):
        X.ConnectivityEncoder(2, 0, 64, 0.1)
    with pytest.raises(ValueError, match="dropout"):
        X.fMRIFusionNet(10, 10, dropout=1.0)
    with pytest.raises(ValueError, match="num_heads"):
        X.fMRIFusionNet(10, 10, num_heads=5)
    with pytest.raises(ValueError, match="task"):
        X.fMRIFusionNet(10, 10, task="ranking")
    assert X.fMRIFusionNet(10, 10, task="regression").head[3].out_features == 1
    assert X.fMRIFusionNet(10, 10, num_classes=3).head[3].out_features == 3
    w = X.fMRIFusionNet(10, 10).get_fusion_weights()
    assert w == {"activation": 0.5, "connectivity": 0.5}
    with pytest.raises(_hip.HipLibraryError):            # no CPU path
        X.ActivationEncoder(1, 4, 32, 0.0)(torch.zeros(2, 4))


def test_connectivity_only_encodes_the_first_argument_when_connectivity_is_none(monkeypatch):
    seen = []

    def fake(encs, xs, training):
        seen.append(xs[0])
        return [torch.zeros(xs[0].shape[0], encs[0].hidden_dim)]

    monkeypatch.setattr(sa, "tab_tx", fake)
    monkeypatch.setattr(sa, "linear", lambda x, lin, act="none", drop_p=0.0: torch.zeros(x.shape[0], lin.out_features))
    a, c = torch.ones(3, 7), torch.full((3, 7), 2.0)
    m = X.fMRIConnectivityOnly(7, hidden_dim=32)
    assert m(a, c).shape == (3, 2) and seen[-1] is c
    assert m(connectivity=c).shape == (3, 2) and seen[-1] is c
    m(a)
    assert seen[-1] is a                                   # the notebook's swapped-argument rule
    r = X.fMRIConnectivityOnly(7, hidden_dim=32, task="regression")
    assert r(a, c).shape == (3,)
    act_only = X.fMRIActivationOnly(7, hidden_dim=32)
    act_only(a, c)
    assert seen[-1] is a


def test_subject_split_indices():
    handler = X.fMRISubjectDataHandler(types.SimpleNamespace())
    ds = types.SimpleNamespace(samples=[{"subject": s} for s in (1, 2, 2, 5, 7, 5)])
    assert handler.get_subject_split_indices(ds, [2]) == ([0, 3, 4, 5], [1, 2])
    assert handler.get_subject_split_indices(ds, [np.int64(5), 1]) == ([1, 2, 4], [0, 3, 5])
    assert handler.get_subject_split_indices(ds, [9]) == ([0, 1, 2, 3, 4, 5], [])
    handler.subject_ids, handler.subject_labels = [1, 2, 5], {1: 0, 2: 1, 5: 1}
    ids, labs = handler.get_subject_ids_and_labels()
    assert ids.tolist() == [1, 2, 5] and labs.tolist() == [0, 1, 1]


def test_subject_vote_rounds_half_to_even():
    assert X.subject_vote([0, 1]) == 0                     # a 1:1 tie votes 0
    assert X.subject_vote([1, 1, 0, 0]) == 0
    assert X.subject_vote([1, 1, 0]) == 1
    assert X.subject_vote([0, 0, 1]) == 0
    assert X.subject_vote([1]) == 1


def test_load_labels_reads_scores(tmp_path):
    (tmp_path / "labels.csv").write_text("subject_id,Outcome,Score\n1,good,0.5\n2,poor,-1.5\n9,good,3\n")
    cls, reg = X.load_labels(tmp_path, [1, 2, 3])
    assert cls == {1: 1, 2: 0} and reg == {1: 0.5, 2: -1.5}


def test_header_declares_the_new_entry_points_at_abi_5():
    assert _hip.header_abi_version() == 5
    sigs = _hip.parse_header()
    assert "mm_tab_tx_fwd" in sigs and "mm_tab_tx_bwd" in sigs
    assert sigs["mm_tab_tx_fwd"].count("p") == 8 and sigs["mm_tab_tx_bwd"].count("p") == 12
    text = open(_hip.header_path()).read()
    assert text.count("CrossModal_fmri_scr.ipynb") >= 1
    assert ops.tab_tx_save_floats(2, 8, 64, 2) == 2 * 19 * 8 * 64 and ops.tab_tx_scratch_floats(1, 8, 64, 2) == 25 * 8 * 64


def test_run_experiment_uses_this_modules_models(monkeypatch):
    got = {}

    def fake(dataset, config, task="classification", **kw):
        got.update(kw, task=task)
        return {}, []

    monkeypatch.setattr(fmri_utils, "run_experiment", fake)
    X.run_experiment(None, None, task="regression", verbose=False)
    assert got["model_classes"] == {"fusion": X.fMRIFusionNet, "activation_only": X.fMRIActivationOnly,
                                    "connectivity_only": X.fMRIConnectivityOnly}
    assert got["task"] == "regression" and got["verbose"] is False
