"""GPU: the fMRI notebook's transformer models (multimodal_eeg_fmri_amd/crossmodal_fmri_scr.py) end to end.

* against tests/golden/f5_fmri_notebook.npz (tools/make_fmri_notebook_golden.py: the notebook's own classes in fp32 on
  the host): eval-mode ``output`` / ``fused`` of the three models and, for the fusion net, train-mode loss and every
  parameter gradient at dropout 0, for classification and regression;
* the fusion net at the notebook's defaults (H = 64, two layers, four heads; dropout 0 so that torch can be the oracle)
  against fp64 torch modules built here;
* launch count, a few fused-AdamW steps, the leave-one-subject-out driver and bridge feature extraction.

Tolerances: the fp32 head family's (tests/test_fmri_tx_kernels_gpu.py).  Gradient tensors below the 1e-5 norm line are
compared with the atol alone and listed in `SMALL`: everything that only shifts the input of ``fusion``'s BatchNorm1d by a
constant (train mode removes the batch mean) - the encoders' final ``norm.bias``, ``cross_attn``'s value bias and
``out_proj.bias``, ``fusion.0.bias`` - and the query / key rows of every ``in_proj``, which must be exact zeros."""
import copy
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from multimodal_eeg_fmri_amd import _hip, bridge_utils, ops
from multimodal_eeg_fmri_amd import crossmodal_fmri_scr as X
from multimodal_eeg_fmri_amd.optim import FusedAdamW

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f5_fmri_notebook.npz")
H, L, A, C, B = 32, 2, 30, 21, 8
SMALL = {"activation_encoder.norm.bias", "connectivity_encoder.norm.bias", "cross_attn.in_proj_bias", "cross_attn.out_proj.bias",
         "fusion.0.bias"}


@pytest.fixture(autouse=True)
def _no_seed_epoch():
    ops.set_seed_epoch(None)
    yield
    ops.set_seed_epoch(None)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def _weights(z, task, prefix=None):
    w = {k: torch.from_numpy(z["w/" + k]) for k in z["sd_names"]}
    if task == "regression":
        w["head.3.weight"], w["head.3.bias"] = torch.from_numpy(z["reg_head3_weight"]), torch.from_numpy(z["reg_head3_bias"])
    if prefix is None:
        return w
    return {("encoder." + k[len(prefix):] if k.startswith(prefix) else k): v for k, v in w.items()
            if k.startswith(prefix) or k.startswith("head.")}


def _inputs(z):
    return torch.from_numpy(z["activation"]).cuda(), torch.from_numpy(z["connectivity"]).cuda()


def _is_in_proj(name):
    return name.endswith(("in_proj_weight", "in_proj_bias"))


def _check_grads(model, want, hidden, small_expected):
    """want: {name: reference gradient (CPU)}; the query / key rows of every in_proj must be exact zeros"""
    small = set()
    for n, q in model.named_parameters():
        have, ref = q.grad.detach().cpu().double(), want[n].double()
        if _is_in_proj(n):
            assert ref[:2 * hidden].norm().item() < 1e-5, n
            assert torch.count_nonzero(have[:2 * hidden]).item() == 0, n
            have, ref = have[2 * hidden:], ref[2 * hidden:]
        if ref.norm().item() < 1e-5:
            small.add(n)
            torch.testing.assert_close(have, ref, rtol=0, atol=2e-5, msg=lambda m: f"{n}: {m}")
        else:
            torch.testing.assert_close(have, ref, rtol=2e-3, atol=2e-5, msg=lambda m: f"{n}: {m}")
    assert small == small_expected, small ^ small_expected


@pytest.mark.parametrize("task", ["classification", "regression"])
def test_three_models_equal_the_notebook_golden(gold, task):
    act, conn = _inputs(gold)
    kw = dict(hidden_dim=H, num_classes=2, dropout=0.0, task=task)
    net = X.fMRIFusionNet(A, C, num_transformer_layers=L, **kw)
    net.load_state_dict(_weights(gold, task))
    a_only = X.fMRIActivationOnly(A, num_layers=L, **kw)
    a_only.load_state_dict(_weights(gold, task, "activation_encoder."))
    c_only = X.fMRIConnectivityOnly(C, num_layers=L, **kw)
    c_only.load_state_dict(_weights(gold, task, "connectivity_encoder."))
    net, a_only, c_only = net.cuda().eval(), a_only.cuda().eval(), c_only.cuda().eval()
    tol = dict(rtol=1e-4, atol=1e-5)
    with torch.no_grad():
        out, fused = net(act, conn, return_features=True)
        assert out.shape == ((B, 2) if task == "classification" else (B,)) and fused.shape == (B, H)
        torch.testing.assert_close(out.cpu(), torch.from_numpy(gold[task + "/fusion_output"]), **tol)
        torch.testing.assert_close(fused.cpu(), torch.from_numpy(gold[task + "/fusion_fused"]), **tol)
        torch.testing.assert_close(net(act, conn).cpu(), out.cpu(), rtol=0, atol=0)
        torch.testing.assert_close(a_only(act, conn).cpu(), torch.from_numpy(gold[task + "/activation_only_output"]), **tol)
        torch.testing.assert_close(c_only(act, conn).cpu(), torch.from_numpy(gold[task + "/connectivity_only_output"]), **tol)
        torch.testing.assert_close(c_only(conn).cpu(), torch.from_numpy(gold[task + "/connectivity_only_output"]), **tol)
    # train mode, dropout 0: loss and every gradient
    net.train()
    out = net(act, conn)
    if task == "classification":
        loss = F.cross_entropy(out, torch.from_numpy(gold["class_labels"]).cuda())
    else:
        loss = F.mse_loss(out, torch.from_numpy(gold["reg_labels"]).cuda())
    loss.backward()
    torch.testing.assert_close(loss.detach().cpu(), torch.from_numpy(gold[task + "/train_loss"]), **tol)
    want = {n: torch.from_numpy(gold[task + "/grad/" + n]) for n, _ in net.named_parameters()}
    _check_grads(net, want, H, SMALL)


def _oracle_fusion(net, act, conn):
    """fp64, torch's own modules as the notebook calls them -> (output, fused)"""
    m = copy.deepcopy(net).cpu().double().train()
    enc = lambda e, x: e.norm(e.transformer(e.project(x).unsqueeze(1)).squeeze(1))       # noqa: E731
    a, c = enc(m.activation_encoder, act), enc(m.connectivity_encoder, conn)
    att, _ = m.cross_attn(a.unsqueeze(1), c.unsqueeze(1), c.unsqueeze(1))
    w = torch.softmax(torch.stack([m.activation_weight, m.connectivity_weight]), dim=0)
    fused = m.fusion(torch.cat([a * w[0], att.squeeze(1) * w[1]], dim=1))
    return m, m.head(fused), fused


def test_fusion_net_defaults_train_gradients_against_fp64():
    torch.manual_seed(41)
    g = torch.Generator().manual_seed(42)
    net = X.fMRIFusionNet(50, 45, dropout=0.0)            # hidden_dim 64, two layers, four heads
    assert net.activation_encoder.hidden_dim == 64 and net.activation_encoder.num_layers == 2 and net.cross_attn.num_heads == 4
    with torch.no_grad():
        for q in net.parameters():
            q.add_(torch.randn(q.shape, generator=g) * 0.05)
    act, conn, R = torch.randn(8, 50, generator=g), torch.randn(8, 45, generator=g), torch.randn(8, 2, generator=g)
    m, out64, fused64 = _oracle_fusion(net, act.double(), conn.double())
    (out64 * R.double()).sum().backward()
    dev = net.cuda().train()
    out, fused = dev(act.cuda(), conn.cuda(), return_features=True)
    (out * R.cuda()).sum().backward()
    torch.testing.assert_close(out.detach().cpu().double(), out64.detach(), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(fused.detach().cpu().double(), fused64.detach(), rtol=1e-4, atol=1e-5)
    _check_grads(dev, {n: q.grad for n, q in m.named_parameters()}, 64, SMALL)
    for n in ("cross_attn.in_proj_weight", "cross_attn.in_proj_bias"):
        assert torch.count_nonzero(dict(dev.named_parameters())[n].grad[:128]).item() == 0
    w = dev.get_fusion_weights()
    assert set(w) == {"activation", "connectivity"} and abs(w["activation"] + w["connectivity"] - 1.0) < 1e-6


def test_encoder_pass_is_one_forward_launch_and_one_backward_call(monkeypatch):
    """both stacks together: ONE mm_tab_tx_fwd launch; ONE mm_tab_tx_bwd call, which is the row pass and the parameter pass
    (two launches, include/mmeeg_hip.h)"""
    net = X.fMRIFusionNet(20, 10, hidden_dim=32, dropout=0.2).cuda().train()
    x = torch.randn(8, 20, device="cuda"), torch.randn(8, 10, device="cuda")
    calls = []
    real = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    net(*x).sum().backward()
    torch.cuda.synchronize()
    assert calls.count("mm_tab_tx_fwd") == 1
    assert 2 * calls.count("mm_tab_tx_bwd") <= 2 and calls.count("mm_tab_tx_bwd") == 1
    assert calls.index("mm_tab_tx_fwd") == 0 and calls[-1] == "mm_tab_tx_bwd"


def test_a_few_fused_adamw_steps_lower_the_loss():
    torch.manual_seed(3)
    net = X.fMRIFusionNet(12, 9, hidden_dim=32, dropout=0.0).cuda().train()
    g = torch.Generator().manual_seed(4)
    act, conn = torch.randn(8, 12, generator=g).cuda(), torch.randn(8, 9, generator=g).cuda()
    y = torch.tensor([0, 1, 0, 1, 1, 0, 1, 0]).cuda()
    opt = FusedAdamW(net.parameters(), lr=3e-3, weight_decay=1e-4)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = F.cross_entropy(net(act, conn), y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses


def _write_subjects(root, n=6, rows=5):
    """linearly separable synthetic subjects as the CSV tree the loaders read"""
    import pandas as pd
    rng = np.random.default_rng(0)
    labels = []
    for s in range(1, n + 1):
        y = s % 2
        d = root / f"sub-{s}"
        d.mkdir(parents=True)
        for t in ("sensory", "DMN"):
            pd.DataFrame(rng.normal(3.0 * (2 * y - 1), 0.3, size=(rows, 4)), columns=list("abcd")).assign(Subject=s).to_csv(
                d / f"subject_{s}_activation_{t}.csv", index=False)
        pd.DataFrame(rng.normal(2.0 * (2 * y - 1), 0.3, size=(3, 3))).to_csv(d / f"subject_{s}_fdr_PPI_Connectivity_DMN.csv", index=False)
        labels.append((s, y))
    (root / "labels").mkdir()
    pd.DataFrame(labels, columns=["Subject", "Label"]).to_csv(root / "labels" / "labels.csv", index=False)


def test_loso_evaluation_and_bridge_feature_extraction(tmp_path):
    _write_subjects(tmp_path)
    cfg = types.SimpleNamespace(data_dir=tmp_path, label_path=tmp_path / "labels", subject_list=list(range(1, 7)),
                                activation_types=["sensory", "DMN"], connectivity_types=["DMN"], agg_method="both", hidden_dim=32,
                                dropout=0.1, batch_size=8, num_epochs=4, learning_rate=3e-3, weight_decay=1e-4, patience=3,
                                grad_clip=1.0)
    handler = X.fMRISubjectDataHandler(cfg)
    handler.load_all()
    assert handler.subject_ids == [1, 2, 3, 4, 5, 6] and handler.reg_labels is None
    torch.manual_seed(0)
    df = X.run_fmri_loso_evaluation(handler, cfg, model_name="fusion", task="classification", verbose=False)
    assert list(df.columns) == ["subject_id", "true_label", "predicted_label", "confidence", "n_samples", "sample_accuracy", "correct"]
    assert list(df["subject_id"]) == [1, 2, 3, 4, 5, 6] and (df["n_samples"] == 1).all()
    assert (df["correct"] == (df["true_label"] == df["predicted_label"]).astype(int)).all()
    assert list(df["true_label"]) == [1, 0, 1, 0, 1, 0]
    assert ((df["confidence"] >= 0.5) & (df["confidence"] <= 1.0)).all()
    # bridge feature extraction: unchanged, through return_features=True
    ds = handler.build_dataset()
    net = X.fMRIFusionNet(ds[0][0].shape[0], ds[0][1].shape[0], hidden_dim=32).cuda()
    feats = bridge_utils.extract_fmri_features(net, handler.activation_features, handler.connectivity_features, cfg.subject_list,
                                               torch.device("cuda"))
    act = torch.stack([handler.activation_features[s] for s in cfg.subject_list]).cuda()
    conn = torch.stack([handler.connectivity_features[s] for s in cfg.subject_list]).cuda()
    with torch.no_grad():
        _, fused = net.eval()(act, conn, return_features=True)
    got = torch.stack([feats[s] for s in cfg.subject_list])
    assert got.shape == (6, 32)
    torch.testing.assert_close(got, fused.cpu(), rtol=0, atol=0)
