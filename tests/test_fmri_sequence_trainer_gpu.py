"""GPU: BridgeTrainer on fMRI frame sequences (`fmri_encoder=fMRISequenceEncoder3D(...)`) at a small shape: 8 channels, 128
samples, 16 pairs (4 subjects x 4), F = 3 frames of 8 x 8 x 8 voxels.  Dropout 0 unless said.  Graph replay and eager tape
train bit-identically under all three objectives, the autograd surface agrees, one frame with copied weights is the
default trainer, the branch is the volume branch plus one launch each way, every parameter and running statistic moves,
a planted lag is found, runs reproduce and resume bit for bit, `explain` and `perturb` are what the public modules give,
the key encoder's twin is generic, and a trainer built without `fmri_encoder=` is what it was.

Planted lag (`synthetic_sequence_pairs(frames=4, peak=2)`): 40 graph steps at lr 1e-3, chosen on the MI355X, where they
gave loss 2.878 -> 0.0005, R@1 1.0 both ways and batch-mean lag weights (0.2473, 0.2463, 0.2595, 0.2469); the whole test
takes 0.13 s."""
import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_sequence_pairs, synthetic_subject_pairs
from multimodal_eeg_fmri_amd.fmri_utils import fMRISequenceEncoder3D

pytestmark = pytest.mark.gpu

C, T, VOL, F = 8, 128, (8, 8, 8), 3


@pytest.fixture(autouse=True)
def _no_seed_epoch():
    ops.set_seed_epoch(None)
    yield
    ops.set_seed_epoch(None)


def _trainer(mode, lr=1e-3, dropout=0.0, frames=F, **kw):
    ops.set_seed_epoch(None)
    ops.set_dropout_seed(0x1234567)
    torch.manual_seed(0)
    enc = fMRISequenceEncoder3D(frames, 64, dropout=dropout)
    tr = BridgeTrainer(eeg_channels=C, dropout=dropout, lr=lr, mode=mode, fmri_encoder=enc, **kw).train()
    if dropout == 0.0:
        tr.head.bridge.fusion.gate_net[2].p = 0.0           # (the fusion gate's hard-coded Dropout(0.2), classify only)
    return tr


@pytest.fixture(scope="module")
def batches():
    """(eeg, fmri (16, F, 8, 8, 8), group ids, labels): 4 subjects x 4 epochs, shuffled; the subject's volume is frame 1 of
    its sequence, the other frames are noise; the label is the subject's parity"""
    out = []
    for i in range(3):
        eeg, vol, g = synthetic_subject_pairs(4, 4, C, T, VOL, seed=900 + i)
        fmri = torch.randn(16, F, *VOL, generator=torch.Generator().manual_seed(950 + i)).cuda()
        fmri[:, 1] = vol[:, 0]
        perm = torch.randperm(16, generator=torch.Generator().manual_seed(i))
        gids = g.cpu()[perm]
        out.append((eeg[perm.cuda()].contiguous(), fmri[perm.cuda()].contiguous(), (gids * 10 + i).to(torch.int32),
                    (gids % 2).to(torch.int64)))
    return out


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
def test_graph_and_manual_steps_are_bit_identical(batches, objective):
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
    assert tg.schedule.fmri_first is False and tg.input_buffers()[1].shape == (16, F, *VOL)


def test_autograd_mode_agrees_with_the_manual_step(batches):
    """the bound of test_trainer_gpu.py::test_trainer_modes_agree_on_first_steps (2e-2 relative), on the loss and on the
    fMRI group's gradients (rel-L2)"""
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
        assert abs(loss.item() - lm) <= 2e-2 * max(1.0, abs(lm)), (loss.item(), lm)
        _, _, lo, hi = tm.groups[-1]
        got, want = probe["g"][lo:hi], ta.bucket.g[lo:hi]
        assert want.abs().max().item() > 0 and want[-(64 + F):].abs().max().item() > 0      # the pool's two gradients among them
        err = ((got - want).norm() / want.norm()).item()
        assert err <= 2e-2, err
        ta = _trainer("autograd")
        la = ta.train_step(e, f, ids)["loss"].item()
        assert abs(la - lm) <= 2e-2 * max(1.0, abs(lm)), (la, lm)


@pytest.mark.parametrize("grad_clip", [0.0, 1.0])
def test_one_frame_with_copied_weights_is_the_default_trainer(batches, grad_clip):
    ops.set_dropout_seed(0x1234567)
    torch.manual_seed(0)
    d = BridgeTrainer(eeg_channels=C, dropout=0.0, lr=1e-3, mode="graph", grad_clip=grad_clip).train()
    s = BridgeTrainer(eeg_channels=C, dropout=0.0, lr=1e-3, mode="graph", grad_clip=grad_clip,
                      fmri_encoder=fMRISequenceEncoder3D.from_volume_encoder(d.fmri_encoder, frames=1)).train()
    s.eeg_encoder.load_state_dict(d.eeg_encoder.state_dict())
    s.head.load_state_dict(d.head.state_dict())
    ops.weights_changed()
    for k, v in d.state_dict().items():
        k2 = k.replace("fmri_encoder.", "fmri_encoder.frame_encoder.")
        assert torch.equal(s.state_dict()[k2], v), k
    eeg = [b[0] for b in batches]
    vols = [b[1][:, 1:2].contiguous() for b in batches]     # (16, 1, 8, 8, 8): a one-channel volume and a one-frame sequence
    ld = torch.stack([d.train_step(eeg[i % 3], vols[i % 3])["loss"].clone() for i in range(5)])
    ls = torch.stack([s.train_step(eeg[i % 3], vols[i % 3])["loss"].clone() for i in range(5)])
    torch.cuda.synchronize()
    assert torch.isfinite(ld).all()
    if grad_clip == 0.0:
        assert torch.equal(ld, ls), (ld, ls)
        assert torch.equal(d.bucket.p, s.bucket.p[:d.bucket.n])
    else:                                                   # the clipped norm's summation order moves with the bucket layout
        assert ((ld - ls).abs() / ld.abs()).max().item() <= 1e-6, (ld, ls)
    assert not s.fmri_encoder.lag_pool.query.any() and not s.fmri_encoder.lag_pool.lag_bias.any()    # one frame: no gradient


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


def test_the_branch_is_the_volume_branch_plus_one_launch_each_way(batches, monkeypatch):
    seq_all, seq_fwd, seq_bwd = _branch_launches(_trainer("manual"), batches[0], monkeypatch)
    ops.set_dropout_seed(0x1234567)
    torch.manual_seed(0)
    vol = BridgeTrainer(eeg_channels=C, dropout=0.0, lr=1e-3, mode="manual").train()
    vol_all, vol_fwd, vol_bwd = _branch_launches(vol, (batches[0][0], batches[0][1][:, 1:2].contiguous()), monkeypatch)
    assert seq_fwd == vol_fwd + ["mm_lagpool_fwd"], (seq_fwd, vol_fwd)
    assert seq_bwd == ["mm_lagpool_bwd"] + vol_bwd, (seq_bwd, vol_bwd)        # (the pool's parameter rows ride in the branch's one flush)
    assert vol_bwd[-1] == "mm_flush_many" and vol_bwd.count("mm_flush_many") == 1
    assert len(seq_all) == len(vol_all) + 2 and "mm_lagpool_fwd" not in vol_all and "mm_lagpool_bwd" not in vol_all


def test_two_steps_move_every_parameter_and_running_statistic(batches):
    tr = _trainer("graph")
    keys = list(tr.state_dict())
    before = {k: v.detach().clone() for k, v in tr.fmri_encoder.state_dict().items()}
    for i in range(2):
        tr.train_step(*batches[i][:2])
    torch.cuda.synchronize()
    after = tr.fmri_encoder.state_dict()
    assert len(before) == 3 * 7 + 2 + 2 and {"lag_pool.query", "lag_pool.lag_bias"} <= set(before)
    for k, v in before.items():
        assert not torch.equal(after[k], v), k
        if "num_batches" in k:
            assert after[k].item() == 2
    assert list(tr.state_dict()) == keys


PLANTED_STEPS, PLANTED_LR = 40, 1e-3


def test_a_planted_lag_is_found():
    """a sign test: the loss falls, retrieval beats chance, and frame 2 - the only one that carries the latent - gets the
    largest batch-mean lag weight"""
    tr = _trainer("graph", lr=PLANTED_LR, frames=4)
    eeg, fmri = synthetic_sequence_pairs(16, 4, 2, C, T, VOL, seed=960)
    losses = [tr.train_step(eeg, fmri)["loss"].item() for _ in range(PLANTED_STEPS)]
    w = tr.fmri_encoder.lag_weights(fmri).mean(dim=0)
    out = tr.evaluate_retrieval(eeg, fmri)
    print("PLANTED_FIG losses", losses[0], losses[-1], "weights", w.tolist(), "R@1", out["eeg_to_fmri"]["R@1"], out["fmri_to_eeg"]["R@1"])
    assert losses[-1] < losses[0], (losses[0], losses[-1])
    assert out["n"] == 16 and out["eeg_to_fmri"]["R@1"] > 1 / 16 and out["fmri_to_eeg"]["R@1"] > 1 / 16, out
    assert all(w[2].item() > w[f].item() for f in (0, 1, 3)), w.tolist()
    assert tr.training and tr.fmri_encoder.training
    ev = tr.evaluate(eeg, fmri)
    assert torch.isfinite(ev["loss"]).item()
    ze, zf = tr.embed(eeg.cpu(), fmri.cpu(), batch_size=5)
    assert ze.shape == zf.shape == (16, 128)
    assert tr.predict(eeg, fmri)["logits"].shape == (16, 2)
    hist = tr.fit([(eeg, fmri)], 1, val=(eeg, fmri), warmup_epochs=0, patience=10)
    assert len(hist) == 1 and "eeg_to_fmri" in hist[0]["val"]


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
    b = BridgeTrainer(eeg_channels=C, dropout=0.3, lr=1e-3, mode="graph", fmri_encoder=fMRISequenceEncoder3D(F, 64, dropout=0.3)).train()
    b.load_checkpoint(path)
    got = _run(b, batches, plan[3:])
    assert torch.equal(want, got), (want, got)
    for x, y in zip((a.bucket.p, a.bucket.m, a.bucket.v, a.bucket.state), (b.bucket.p, b.bucket.m, b.bucket.v, b.bucket.state)):
        assert torch.equal(x, y)
    sa, sb = _bn_state(a), _bn_state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    other = BridgeTrainer(eeg_channels=C, dropout=0.3, lr=1e-3, mode="graph", fmri_encoder=fMRISequenceEncoder3D(2, 64, dropout=0.3)).train()
    with pytest.raises(ValueError, match=r"fmri_branch differs: checkpoint \[kind='sequence', frames=3\], trainer \[kind='sequence', frames=2\]"):
        other.load_checkpoint(path)


def _eval_scores(tr, e, f):
    """the eval similarity on the public modules, as the existing `explain` / `perturb` tests form it: eval mode, autograd
    on, the inputs asking for a gradient"""
    ze, zf = tr.head.embed(tr.eeg_encoder(e), tr.fmri_encoder(f))
    return (ze * zf).sum(dim=1)


def test_explain_is_the_autograd_gradient_of_the_eval_similarity(batches):
    """the bound of the existing explain tests: rtol 1e-3, atol 1e-5"""
    tr = _trainer("manual", dropout=0.3)
    e, f, g, y = batches[0]
    tr.train_step(e, f)
    e, f = e[:5].contiguous(), f[:5].contiguous()
    state = {k: v.clone() for k, v in tr.state_dict().items()}
    out = tr.explain(e, f, method="gradient_x_input")
    assert tr.training and set(out) == {"eeg", "eeg_channels", "fmri", "fmri_frames", "lag_weights", "scores"}
    assert out["fmri"].shape == (5, F, *VOL) and out["fmri_frames"].shape == (5, F) and out["lag_weights"].shape == (5, F)
    torch.testing.assert_close(out["fmri_frames"], out["fmri"].flatten(2).sum(dim=2), rtol=1e-6, atol=0)
    assert torch.equal(out["lag_weights"], tr.fmri_encoder.lag_weights(f))
    torch.testing.assert_close(out["lag_weights"].sum(dim=1), torch.ones(5, device="cuda"), rtol=1e-6, atol=0)
    for k, v in tr.state_dict().items():                    # parameters and BatchNorm buffers are where they were
        assert torch.equal(v, state[k]), k
    tr.eval()
    ee, ff = e.clone().requires_grad_(True), f.clone().requires_grad_(True)
    score = _eval_scores(tr, ee, ff)
    ge, gf = torch.autograd.grad(score.sum(), [ee, ff])
    tr.train()
    assert all(gf[:, k].abs().max().item() > 0 for k in range(F))
    torch.testing.assert_close(out["fmri"], gf.abs() * f.abs(), rtol=1e-3, atol=1e-5)
    torch.testing.assert_close(out["eeg"], ge.abs() * e.abs(), rtol=1e-3, atol=1e-5)
    torch.testing.assert_close(out["scores"], score.detach(), rtol=1e-5, atol=1e-6)
    ig = tr.explain(e, f, n_steps=4, baseline="mean")
    assert ig["fmri"].shape == (5, F, *VOL) and torch.isfinite(ig["fmri"]).all() and ig["fmri_frames"].shape == (5, F)


def test_perturb_knocks_out_frames_and_blocks(batches):
    """the bound of the existing perturb tests: rtol 1e-5, atol 1e-6"""
    tr = _trainer("manual", dropout=0.3)
    e, f, g, y = batches[0]
    tr.train_step(e, f)
    e, f = e[:4].contiguous(), f[:4].contiguous()
    out = tr.perturb(e, f, fmri_units=("rows", 1), chunk_masks=1)
    assert tr.training and out["fmri"].shape == (4, F) and out["eeg"].shape == (4, C)
    tr.eval()
    full = _eval_scores(tr, e.clone().requires_grad_(True), f.clone().requires_grad_(True)).detach()
    drops = []
    for k in range(F):
        fk = f.clone()
        fk[:, k] = 0
        drops.append(full - _eval_scores(tr, e.clone().requires_grad_(True), fk.requires_grad_(True)).detach())
    fb = f.clone()
    fb[:, :, :4, 4:, :4] = 0                                # block (0, 1, 0) of every frame: unit 2 of 2 x 2 x 2
    block = full - _eval_scores(tr, e.clone().requires_grad_(True), fb.requires_grad_(True)).detach()
    tr.train()
    want = torch.stack(drops, dim=1)
    assert want.abs().max().item() > 0
    torch.testing.assert_close(out["scores"], full, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(out["fmri"], want, rtol=1e-5, atol=1e-6)
    assert torch.equal(tr.perturb(e, f, chunk_masks=1)["fmri"], out["fmri"])          # one frame per unit is the default
    blocks = tr.perturb(e, f, fmri_units=("blocks", 4), chunk_masks=1)
    assert blocks["fmri"].shape == (4, 8)
    torch.testing.assert_close(blocks["fmri"][:, 2], block, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError, match="fmri_units must be"):
        tr.perturb(e, f, fmri_units=("windows", 1))


def test_key_encoder_steps_are_bit_identical_in_graph_and_manual_mode(batches):
    kw = dict(bank_size=32, ema_decay=0.99, key_encoder=True)
    tm, tg = _trainer("manual", **kw), _trainer("graph", **kw)
    plan = [(i % 3, False) for i in range(3)]
    lm, lg = _run(tm, batches, plan), _run(tg, batches, plan)
    assert torch.isfinite(lm).all() and torch.equal(lm, lg)
    assert torch.equal(tm.bucket.p, tg.bucket.p) and torch.equal(tm.bucket.ema, tg.bucket.ema)
    assert type(tg._key["fmri_encoder"]).__name__ == "fMRISequenceEncoder3D" and tg.bank_filled == 32


# the launches of one manual step of a trainer built without `fmri_encoder=` at 16 pairs, 8 channels, 128 samples, 16^3
# volumes, dropout 0, as recorded on the commit before this branch existed (tests/test_fmri_tab_trainer_gpu.py pins the
# same list)
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


def test_the_default_trainer_is_unchanged(batches, monkeypatch):
    _trainer("graph").train_step(*batches[0][:2])           # a sequence trainer has run in this process
    ops.set_seed_epoch(None)
    ops.set_dropout_seed(0x1234567)
    torch.manual_seed(0)
    d = BridgeTrainer(eeg_channels=C, dropout=0.0, lr=1e-3, mode="manual").train()
    assert d._fmri_kind == "volume" and type(d.fmri_encoder).__name__ == "fMRIVolumeEncoder3D"
    assert "fmri_branch" not in d.checkpoint_state()["bridge_trainer_state"]
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
