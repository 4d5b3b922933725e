"""BridgeTrainer(loss="sigmoid") at a small shape, dropout 0: the graph replay and the eager tape train bit-identically
over alternating plain and grouped batches, the autograd surface agrees with them, the eval loss is the fp64 contract of
the pairwise sigmoid loss, `logit_bias` is trained and checkpointed, the default trainer is untouched, and a short `fit`
lowers the grouped loss."""
import pytest
import torch

from multimodal_eeg_fmri_amd import ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_subject_pairs
from test_sigmoid_loss_gpu import ref_sigmoid

pytestmark = pytest.mark.gpu

C, T, VOL = 8, 256, (16, 16, 16)


@pytest.fixture(autouse=True)
def _no_seed_epoch():
    ops.set_seed_epoch(None)
    yield
    ops.set_seed_epoch(None)


def _trainer(mode, lr=1e-3, **kw):
    ops.set_seed_epoch(None)
    torch.manual_seed(0)
    return BridgeTrainer(eeg_channels=C, dropout=0.0, lr=lr, mode=mode, **kw).train()


@pytest.fixture(scope="module")
def batches():
    out = []
    for i in range(3):
        eeg, fmri, g = synthetic_subject_pairs(4, 4, C, T, VOL, seed=900 + i)
        perm = torch.randperm(eeg.shape[0], generator=torch.Generator().manual_seed(i))
        out.append((eeg[perm.cuda()].contiguous(), fmri[perm.cuda()].contiguous(), (g.cpu()[perm] * 10 + i).to(torch.int32)))
    return out


PLAN = [(0, False), (1, True), (2, False), (0, True), (1, False)]      # plain and grouped batches alternate


def _run(tr, batches, plan):
    losses = []
    for i, grouped in plan:
        e, f, g = batches[i]
        losses.append(tr.train_step(e, f, g if grouped else None)["loss"].clone())
    torch.cuda.synchronize()
    return torch.stack(losses)


def test_graph_and_manual_steps_are_bit_identical_over_plain_and_grouped_batches(batches):
    tm, tg = _trainer("manual", loss="sigmoid"), _trainer("graph", loss="sigmoid")
    lm = _run(tm, batches, PLAN)
    lg = _run(tg, batches, PLAN)
    assert tg.capture_mode == "one graph" and tg.loss == "sigmoid"
    assert torch.isfinite(lm).all()
    assert torch.equal(lm, lg), (lm - lg).abs().max().item()
    assert torch.equal(tm.bucket.p, tg.bucket.p)


def test_autograd_mode_agrees_with_the_manual_step(batches):
    e, f, g = batches[0]
    for ids in (None, g):
        tm = _trainer("manual", loss="sigmoid")
        lm = tm.train_step(e, f, ids)["loss"].item()
        db = tm._scal[4].item()
        ta = _trainer("autograd", loss="sigmoid")
        loss, _, _ = ta.forward(e, f, ids)
        loss.backward()
        assert abs(ta.head.logit_bias.grad.item() - db) <= 1e-5, (ta.head.logit_bias.grad.item(), db)
        assert abs(ta.head.logit_scale.grad.item() - tm._scal[3].item()) <= 1e-5
        ta = _trainer("autograd", loss="sigmoid")
        la = ta.train_step(e, f, ids)["loss"].item()
        assert abs(la - lm) <= 1e-5 and abs(loss.item() - lm) <= 1e-5, (la, loss.item(), lm)


def test_evaluate_equals_the_fp64_contract(batches):
    """grouped: a batch of 4 subjects x 4 epochs with its ids; plain: 16 subjects x 1 epoch - with one volume per pair no two
    columns of C are equal up to rounding, so the exact top-1 flags do not hang on how fp32 orders copies of one volume"""
    tr = _trainer("graph", loss="sigmoid")
    _run(tr, batches, PLAN[:3])
    singles = synthetic_subject_pairs(16, 1, C, T, VOL, seed=950)
    for e, f, ids in (singles[:2] + (None,), batches[1]):
        out = tr.evaluate(e, f, ids)
        ze, zf = tr.embed(e, f)
        want, _ = ref_sigmoid(torch.cat([ze, zf], 1).cpu(), None if ids is None else ids.long(), tr.head.logit_scale.item(),
                              tr.head.logit_bias.item(), e.shape[0], 0)
        assert abs(out["loss"].item() - want[0].item()) <= 1e-5 * max(1.0, abs(want[0].item())), (out["loss"].item(), want[0].item())
        assert out["top1_e2f"].item() == want[1].item() and out["top1_f2e"].item() == want[2].item()


def test_logit_bias_is_trained(batches):
    tr = _trainer("graph", loss="sigmoid")
    assert tr.head.logit_bias.item() == -10.0
    assert any(p is tr.head.logit_bias and n == "head.logit_bias" for _, n, p, _ in tr.optimizer_param_map())
    _run(tr, batches, [(0, False), (1, False), (2, False)])
    assert tr.head.logit_bias.item() != -10.0


def test_the_default_trainer_is_unchanged(batches):
    _trainer("graph", loss="sigmoid").train_step(*batches[0][:2])         # a sigmoid trainer has run in this process
    d = _trainer("graph", loss="infonce")
    assert d.loss == "infonce" and "head.logit_bias" not in d.state_dict() and d._scal.numel() == 4
    assert "loss" not in d.checkpoint_state()["bridge_trainer_state"]
    e, f, g = batches[0]
    ops.set_seed_epoch(None)
    torch.manual_seed(0)
    k = BridgeTrainer(eeg_channels=C, dropout=0.0, lr=1e-3, mode="graph").train()      # built without the keyword
    for ids in (None, g):
        a, b = d.train_step(e, f, ids)["loss"].clone(), k.train_step(e, f, ids)["loss"].clone()
        assert torch.equal(a, b), (a.item(), b.item())
    assert torch.equal(d.bucket.p, k.bucket.p)


def test_checkpoint_resumes_bit_for_bit_and_refuses_the_other_loss(batches, tmp_path):
    a = _trainer("graph", loss="sigmoid")
    _run(a, batches, PLAN[:2])
    path = str(tmp_path / "ck.pt")
    a.save_checkpoint(path, epoch=1)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["bridge_trainer_state"]["loss"] == "sigmoid" and "head.logit_bias" in ck["model_state_dict"]
    want = _run(a, batches, PLAN[2:4])
    torch.manual_seed(11)
    b = BridgeTrainer(eeg_channels=C, dropout=0.0, lr=1e-3, mode="graph", loss="sigmoid").train()
    b.load_checkpoint(path)
    got = _run(b, batches, PLAN[2:4])
    assert torch.equal(want, got), (want, got)
    for x, y in zip((a.bucket.p, a.bucket.m, a.bucket.v, a.bucket.state), (b.bucket.p, b.bucket.m, b.bucket.v, b.bucket.state)):
        assert torch.equal(x, y)
    other = _trainer("graph")
    with pytest.raises(ValueError, match="loss"):
        other.load_checkpoint(path)


def test_a_short_fit_lowers_the_grouped_loss():
    k = 4                                                   # epochs (and copies of the volume) per subject in a batch
    eeg, fmri, groups = synthetic_subject_pairs(16, k, C, T, VOL, seed=31, epoch_noise=0.3)
    train = [(eeg[i:i + 16], fmri[i:i + 16], groups[i:i + 16]) for i in range(0, 64, 16)]
    tr = _trainer("graph", loss="sigmoid")
    before = sum(tr.evaluate(*b)["loss"].item() for b in train) / len(train)
    hist = tr.fit(train, 20, warmup_epochs=1, patience=100)
    after = sum(tr.evaluate(*b)["loss"].item() for b in train) / len(train)
    assert len(hist) == 20
    assert after < before, f"mean grouped evaluate loss before fit {before:.6f}, after {after:.6f}"
