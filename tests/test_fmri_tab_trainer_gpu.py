"""GPU: BridgeTrainer on tabular fMRI features (`fmri_encoder=fMRITabularEncoder(...)`) at a small shape: 8 channels, 128
samples, 16 pairs (4 subjects x 4), activation_dim 37, connectivity_dim 50 (16 x 87 = 1392 floats: the fused staging
launch takes the fMRI batch) and one batch of 6 pairs (522 floats, no multiple of 4: the `copy_` fallback).  Dropout 0
unless said.  Graph replay and eager tape train bit-identically under all three objectives, the autograd surface agrees,
the branch is two launches, every parameter and running statistic moves, training learns, runs reproduce and resume bit
for bit, `explain` is the autograd gradient, the host-fed path gives the device path's losses, and a trainer built
without `fmri_encoder=` is what it was."""
import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
from multimodal_eeg_fmri_amd.bridge_trainer import (BridgeTrainer, synthetic_subject_pairs, synthetic_tabular_pairs,
                                                    synthetic_tabular_subject_pairs)
from multimodal_eeg_fmri_amd.fmri_utils import fMRITabularEncoder

pytestmark = pytest.mark.gpu

C, T, A, CF = 8, 128, 37, 50


@pytest.fixture(autouse=True)
def _no_seed_epoch():
    ops.set_seed_epoch(None)
    yield
    ops.set_seed_epoch(None)


def _trainer(mode, lr=1e-3, dropout=0.0, **kw):
    ops.set_seed_epoch(None)
    ops.set_dropout_seed(0x1234567)
    torch.manual_seed(0)
    enc = fMRITabularEncoder(A, CF, hidden_dim=64, dropout=dropout)
    tr = BridgeTrainer(eeg_channels=C, dropout=dropout, lr=lr, mode=mode, fmri_encoder=enc, **kw).train()
    if dropout == 0.0:
        tr.head.bridge.fusion.gate_net[2].p = 0.0           # (the fusion gate's hard-coded Dropout(0.2), classify only)
    return tr


@pytest.fixture(scope="module")
def batches():
    """(eeg, fmri, group ids, labels): 4 subjects x 4 epochs, shuffled; the label is the subject's parity"""
    out = []
    for i in range(3):
        eeg, fmri, g = synthetic_tabular_subject_pairs(4, 4, C, T, A, CF, seed=800 + i)
        perm = torch.randperm(eeg.shape[0], generator=torch.Generator().manual_seed(i))
        gids = g.cpu()[perm]
        out.append((eeg[perm.cuda()].contiguous(), fmri[perm.cuda()].contiguous(), (gids * 10 + i).to(torch.int32),
                    (gids % 2).to(torch.int64)))
    return out


@pytest.fixture(scope="module")
def odd_batch():
    eeg, fmri = synthetic_tabular_pairs(6, C, T, A, CF, seed=850)
    assert fmri.numel() % 4 != 0
    return eeg, fmri


PLAN = [(0, False), (1, True), (2, False), (0, True), (1, False)]       # plain and grouped batches alternate
OBJECTIVES = {"infonce": {}, "sigmoid": {"loss": "sigmoid"}, "classify": {"classify": True, "ce_weight": 0.5}}


def _run(tr, batches, plan):
    rows = []
    for i, grouped in plan:
        e, f, g, y = batches[i]
        out = tr.train_step(e, f, g if grouped else None, y if tr.classify else None)
        rows.append(out["loss"].clone())
    torch.cuda.synchronize()
    return torch.stack(rows)


def _bn_state(tr):
    return {k: v.clone() for k, v in tr.fmri_encoder.state_dict().items() if "running" in k or "num_batches" in k}


@pytest.mark.parametrize("objective", list(OBJECTIVES))
def test_graph_and_manual_steps_are_bit_identical(batches, odd_batch, objective):
    kw = OBJECTIVES[objective]
    tm, tg = _trainer("manual", **kw), _trainer("graph", **kw)
    lm, lg = _run(tm, batches, PLAN), _run(tg, batches, PLAN)
    assert tg.capture_mode == "one graph"
    assert torch.isfinite(lm).all()
    assert torch.equal(lm, lg), (lm - lg).abs().max().item()
    assert torch.equal(tm.bucket.p, tg.bucket.p)
    sm, sg = _bn_state(tm), _bn_state(tg)
    for k in sm:
        assert torch.equal(sm[k], sg[k]), k
        if "num_batches" in k:
            assert sm[k].item() == len(PLAN), k
    if objective == "infonce":                              # a batch whose fMRI floats are no multiple of 4: staged by copy_
        e, f = odd_batch
        for _ in range(2):                                  # the capture, then a replay that stages
            a, b = tm.train_step(e, f)["loss"].clone(), tg.train_step(e * 1.0, f * 1.0)["loss"].clone()
            assert torch.equal(a, b)
        assert torch.equal(tm.bucket.p, tg.bucket.p)


def test_autograd_mode_agrees_with_the_manual_step(batches):
    e, f, g, y = batches[0]
    for ids in (None, g):
        tm = _trainer("manual")
        tm.grad_clip = 0.0
        probe = {}
        real = tm._seg_adamw
        tm._seg_adamw = lambda: (probe.setdefault("g", tm.bucket.g.clone()), real())[1]    # the gradients, before AdamW clears them
        lm = tm.train_step(e, f, ids)["loss"].item()
        ta = _trainer("autograd")
        loss, _, _ = ta.forward(e, f, ops.group_ids(ids, 16, e.device))
        loss.backward()
        ta.bucket.absorb_autograd_grads()
        torch.cuda.synchronize()
        assert abs(loss.item() - lm) <= 1e-5, (loss.item(), lm)
        _, _, lo, hi = tm.groups[-1]
        got, want = probe["g"][lo:hi], ta.bucket.g[lo:hi]
        assert want.abs().max().item() > 0
        assert (got - want).abs().max().item() <= 1e-5, (got - want).abs().max().item()
        ta = _trainer("autograd")
        assert abs(ta.train_step(e, f, ids)["loss"].item() - lm) <= 1e-5


def _branch_launches(tr, batch, monkeypatch):
    """names of the launches of the second manual step, and of its fMRI branch alone: the forward's between phase stamps
    3 and 4, the backward's between 9 and 10 (`BridgeTrainer.STAMP_NAMES`)"""
    e, f = batch[:2]
    tr.train_step(e, f)                                     # the first step records the weight list
    tr.stamps = torch.zeros(16, dtype=torch.int64, device="cuda")
    calls = []
    real = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (calls.append((name, a[1] if name == "mm_debug_stamp" else None)), real(name, *a))[1])
    tr.train_step(e, f)
    monkeypatch.setattr(_hip, "call", real)
    torch.cuda.synchronize()
    at = {i: k for k, (n, i) in enumerate(calls) if n == "mm_debug_stamp"}
    names = [n for n, _ in calls]
    return [n for n in names if n != "mm_debug_stamp"], names[at[3] + 1:at[4]], names[at[9] + 1:at[10]]


def test_the_fmri_branch_is_two_launches(batches, monkeypatch):
    tab_all, tab_fwd, tab_bwd = _branch_launches(_trainer("manual"), batches[0], monkeypatch)
    assert tab_fwd == ["mm_fmri_tab_fwd"] and tab_bwd == ["mm_fmri_tab_bwd"]
    assert tab_all.count("mm_fmri_tab_fwd") == 1 and tab_all.count("mm_fmri_tab_bwd") == 1
    ops.set_dropout_seed(0x1234567)
    torch.manual_seed(0)
    vol = BridgeTrainer(eeg_channels=C, dropout=0.0, lr=1e-3, mode="manual").train()
    ev, fv, _ = synthetic_subject_pairs(4, 4, C, T, (16, 16, 16), seed=800)
    vol_all, vol_fwd, vol_bwd = _branch_launches(vol, (ev, fv), monkeypatch)
    assert len(vol_fwd) > 1 and len(vol_bwd) > 1 and "mm_fmri_tab_fwd" not in vol_all
    rest = [n for n in tab_all if n not in ("mm_fmri_tab_fwd", "mm_fmri_tab_bwd")]
    assert set(rest) <= set(vol_all)                        # nothing else is new in the step ...
    assert len(tab_all) == len(vol_all) - len(vol_fwd) - len(vol_bwd) + 2      # ... and nothing else left it


def test_a_step_moves_every_parameter_and_running_statistic(batches):
    tr = _trainer("graph")
    keys = list(tr.state_dict())
    before = {k: v.detach().clone() for k, v in tr.fmri_encoder.state_dict().items()}
    e, f, g, y = batches[0]
    tr.train_step(e, f)
    torch.cuda.synchronize()
    after = tr.fmri_encoder.state_dict()
    assert len(before) == 2 + 5 * 7
    for k, v in before.items():
        assert not torch.equal(after[k], v), k
        if "num_batches" in k:
            assert after[k].item() == 1
    assert list(tr.state_dict()) == keys
    w = tr.fmri_encoder.get_fusion_weights()
    assert abs(w["activation"] + w["connectivity"] - 1.0) < 1e-6 and w["activation"] != 0.5


def test_thirty_steps_lower_the_loss_and_retrieval_beats_chance(batches):
    tr = _trainer("graph", lr=1e-3)
    eeg, fmri = synthetic_tabular_pairs(16, C, T, A, CF, seed=860)
    losses = [tr.train_step(eeg, fmri)["loss"].item() for _ in range(30)]
    assert losses[-1] < losses[0], (losses[0], losses[-1])
    out = tr.evaluate_retrieval(eeg, fmri)
    assert out["n"] == 16
    assert out["eeg_to_fmri"]["R@1"] > 1 / 16 and out["fmri_to_eeg"]["R@1"] > 1 / 16, out
    ev = tr.evaluate(eeg, fmri)
    assert torch.isfinite(ev["loss"]).item() and tr.training
    ze, zf = tr.embed(eeg.cpu(), fmri.cpu(), batch_size=5)
    assert ze.shape == zf.shape == (16, 128)
    assert tr.predict(eeg, fmri)["logits"].shape == (16, 2)


def test_two_runs_with_dropout_are_bit_identical(batches):
    runs = []
    for _ in range(2):
        tr = _trainer("graph", dropout=0.3)
        losses = _run(tr, batches, [(i % 3, False) for i in range(6)])
        runs.append((losses, tr.bucket.p.clone(), _bn_state(tr)))
    assert torch.isfinite(runs[0][0]).all()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
    ref = _run(_trainer("graph", dropout=0.0), batches, [(0, False)])
    assert not torch.equal(ref[0], runs[0][0][0])           # the masks are really on


def test_checkpoint_resumes_bit_for_bit(batches, tmp_path):
    plan = [(i % 3, False) for i in range(6)]
    a = _trainer("graph", dropout=0.3)
    _run(a, batches, plan[:3])
    path = str(tmp_path / "ck.pt")
    a.save_checkpoint(path, epoch=1)
    want = _run(a, batches, plan[3:])
    torch.manual_seed(11)
    b = BridgeTrainer(eeg_channels=C, dropout=0.3, lr=1e-3, mode="graph",
                      fmri_encoder=fMRITabularEncoder(A, CF, hidden_dim=64, dropout=0.3)).train()
    b.load_checkpoint(path)
    got = _run(b, batches, plan[3:])
    assert torch.equal(want, got), (want, got)
    for x, y in zip((a.bucket.p, a.bucket.m, a.bucket.v, a.bucket.state), (b.bucket.p, b.bucket.m, b.bucket.v, b.bucket.state)):
        assert torch.equal(x, y)
    sa, sb = _bn_state(a), _bn_state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
        if "num_batches" in k:
            assert sa[k].item() == 6


def test_explain_is_the_autograd_gradient_of_the_eval_similarity(batches):
    tr = _trainer("manual", dropout=0.3)
    e, f, g, y = batches[0]
    tr.train_step(e, f)
    e, f = e[:5].contiguous(), f[:5].contiguous()
    state = {k: v.clone() for k, v in tr.state_dict().items()}
    out = tr.explain(e, f, method="gradient")
    assert tr.training and set(out) == {"eeg", "eeg_channels", "fmri", "fmri_activation", "fmri_connectivity", "scores"}
    assert out["eeg"].shape == e.shape and out["fmri"].shape == (5, A + CF) and out["scores"].shape == (5,)
    assert out["fmri_activation"].shape == (5, A) and out["fmri_connectivity"].shape == (5, CF)
    assert torch.equal(torch.cat([out["fmri_activation"], out["fmri_connectivity"]], dim=1), out["fmri"])
    assert out["fmri_activation"].data_ptr() == out["fmri"].data_ptr()
    for k, v in tr.state_dict().items():                    # parameters and BatchNorm buffers are where they were
        assert torch.equal(v, state[k]), k
    tr.eval()
    ee, ff = e.clone().requires_grad_(True), f.clone().requires_grad_(True)
    ze, zf = tr.head.embed(tr.eeg_encoder(ee), tr.fmri_encoder(ff))
    score = (ze * zf).sum(dim=1)
    ge, gf = torch.autograd.grad(score.sum(), [ee, ff])
    tr.train()
    assert gf.abs().max().item() > 0
    torch.testing.assert_close(out["fmri"], gf.abs(), rtol=1e-3, atol=1e-5)
    torch.testing.assert_close(out["eeg"], ge.abs(), rtol=1e-3, atol=1e-5)
    torch.testing.assert_close(out["scores"], score.detach(), rtol=1e-5, atol=1e-6)
    ig = tr.explain(e, f, n_steps=6, baseline="mean")       # the batched engine: 6 x 5 frozen rows per launch
    assert ig["fmri"].shape == (5, A + CF) and torch.isfinite(ig["fmri"]).all() and ig["fmri"].sum().item() > 0
    torch.testing.assert_close(ig["scores"], out["scores"], rtol=1e-5, atol=1e-6)     # (the same pairs inside a 30-row batch)


def test_host_fed_steps_give_the_device_paths_losses(batches):
    def run(packed):
        tr = _trainer("graph", dropout=0.2)
        losses = [tr.train_step(*batches[0][:2])["loss"].clone()]        # captures; fixes the shapes
        if packed == "feeder":
            feeder = tr.host_feeder()
            hosts = [tr.pack_host_batch(*batches[i % 3][:2]) for i in range(1, 5)]
            feeder.upload(hosts[0])
            for i in range(4):
                if i + 1 < 4:
                    feeder.upload(hosts[i + 1])
                losses.append(feeder.step()["loss"].clone())
        else:
            for i in range(1, 5):
                e, f = batches[i % 3][:2]
                if packed:
                    host = tr.pack_host_batch(e, f)
                    assert host.numel() == 16 * T * 16 * 2 + 16 * (A + CF) * 4
                    losses.append(tr.train_step_packed(host.cuda(non_blocking=True))["loss"].clone())
                else:
                    losses.append(tr.train_step(e, f)["loss"].clone())
        torch.cuda.synchronize()
        bufs = tr.input_buffers()
        assert bufs[1].shape == (16, A + CF)
        return torch.stack(losses), tr.bucket.p.clone()
    l0, p0 = run(False)
    l1, p1 = run(True)
    l2, p2 = run("feeder")
    assert torch.isfinite(l0).all()
    assert torch.equal(l0, l1) and torch.equal(p0, p1)
    assert torch.equal(l0, l2) and torch.equal(p0, p2)


def test_augmented_steps_are_bit_identical_in_graph_and_manual_mode(batches, odd_batch):
    """`augment=`: the staging launch carries the fMRI rows when their floats are a multiple of 4, `copy_` does otherwise"""
    from multimodal_eeg_fmri_amd.crossmodal_eeg_scr import EEGTransforms
    losses = {}
    for mode in ("graph", "manual"):
        tr = _trainer(mode, augment=EEGTransforms(p=0.6, seed=11))
        rows = [tr.train_step(*batches[i % 2][:2])["loss"].clone() for i in range(3)]
        rows += [tr.train_step(*odd_batch)["loss"].clone() for _ in range(2)]
        torch.cuda.synchronize()
        losses[mode] = torch.stack(rows)
        assert tr.augment_step == 5
    assert torch.isfinite(losses["graph"]).all()
    assert torch.equal(losses["graph"], losses["manual"]), losses
    plain = _run(_trainer("manual"), batches, [(0, False)])
    assert not torch.equal(plain[0], losses["manual"][0])   # the batch was really augmented


def test_fit_runs_on_tabular_batches(batches):
    tr = _trainer("graph")
    train = [(b[0], b[1], b[2]) for b in batches[:2]]
    e, f, g, y = batches[2]
    hist = tr.fit(train, 2, val=(e, f, g), warmup_epochs=0, patience=10)
    assert len(hist) == 2 and "eeg_to_fmri" in hist[0]["val"]


# the launches of one manual step of a trainer built without `fmri_encoder=` at this file's shape (16 pairs, 8 channels,
# 128 samples, 16^3 volumes, dropout 0), recorded on the commit before the tabular branch existed
DEFAULT_STEP_LAUNCHES = [
    "mm_prep_many_zero", "mm_pack_nct_bf16", "mm_conv1d_fwd", "mm_bn_act_fwd_fin", "mm_conv1d_fwd",
    "mm_bn_act_fwd_fin", "mm_conv1d_fwd", "mm_bn_act_fwd_ln_fin", "mm_conv1d_fwd", "mm_attn_fwd", "mm_ffn_rows_fwd",
    "mm_attn_fwd", "mm_ffn_rows_fwd", "mm_pooled_head_fwd", "mm_conv3d_l1_gram", "mm_conv3d_l1_fwd_fin",
    "mm_conv3d_fwd", "mm_pool3d_bn_act_fwd_fin", "mm_conv3d_fwd", "mm_bn_act_fwd_fin", "mm_meanpool_fwd",
    "mm_pooled_head_fwd", "mm_proj_heads_fwd", "mm_clip_loss_own_rows", "mm_proj_heads_bwd",
    "mm_pooled_head_bwd_rows", "mm_ffn_rows_bwd", "mm_attn_bwd", "mm_linear_dgrad_ln_bwd", "mm_ffn_rows_bwd",
    "mm_attn_bwd", "mm_linear_dgrad_ln_bwd_bn_reduce", "mm_bn_act_bwd_apply", "mm_conv1d_wgrad",
    "mm_conv1d_dgrad_bn_reduce", "mm_bn_act_bwd_apply", "mm_conv1d_wgrad", "mm_conv1d_dgrad_bn_reduce",
    "mm_bn_act_bwd_apply", "mm_conv1d_wgrad", "mm_flush_many", "mm_pooled_head_bwd", "mm_bn_act_bwd_reduce_bcast",
    "mm_bn_act_bwd_apply_bcast", "mm_conv3d_wgrad", "mm_conv3d_fwd", "mm_pool3d_bn_act_bwd_reduce",
    "mm_pool3d_bn_act_bwd_apply", "mm_conv3d_wgrad", "mm_conv3d_fwd", "mm_conv3d_l1_bwd", "mm_conv1d_wgrad_many",
    "mm_flush_many", "mm_conv1d_wgrad_many", "mm_flush_many", "mm_flush_many", "mm_sumsq", "mm_adamw_clip"]
DEFAULT_GROUPS = [['eeg conv block 1', 'main', 0, 3776],
                  ['eeg conv blocks 2-3', 'handed1', 3776, 94656],
                  ['eeg transformer stack + heads', 'handed0', 94656, 533057],
                  ['fmri encoder', 'fmri', 533057, 819329]]


def test_the_default_trainer_is_unchanged(batches, monkeypatch):
    _trainer("graph").train_step(*batches[0][:2])           # a tabular trainer has run in this process
    ops.set_seed_epoch(None)
    ops.set_dropout_seed(0x1234567)
    torch.manual_seed(0)
    d = BridgeTrainer(eeg_channels=C, dropout=0.0, lr=1e-3, mode="manual").train()
    assert d._fmri_kind == "volume" and type(d.fmri_encoder).__name__ == "fMRIVolumeEncoder3D"
    assert [list(g) for g in d.groups] == DEFAULT_GROUPS
    fkeys = [k for k in d.state_dict() if k.startswith("fmri_encoder.")]
    assert len(fkeys) == 3 * 7 + 2 and all("conv_layers" in k or "output_proj" in k for k in fkeys)
    ev, fv, _ = synthetic_subject_pairs(4, 4, C, T, (16, 16, 16), seed=800)
    d.train_step(ev, fv)
    calls = []
    real = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    out = d.train_step(ev, fv)
    monkeypatch.setattr(_hip, "call", real)
    torch.cuda.synchronize()
    assert torch.isfinite(out["loss"]).item() and set(out) == {"loss", "top1_e2f", "top1_f2e"}
    assert calls == DEFAULT_STEP_LAUNCHES, calls
