"""BridgeTrainer(neighbour_radius=R) at the small shape of tests/test_clip_bank_trainer_gpu.py (8 channels, 128 samples,
16^3 volumes, 16 pairs; dropout 0) with timeline ids (`bridge_utils.timeline_ids`: two runs of 8 consecutive epochs,
shuffled): the graph replay and the eager tape train bit-identically; the autograd surface agrees with the tape, with
and without the classification branch; the step launches the masked entry point where the grouped trainer launches the
grouped one and nothing else differs; a checkpoint resumes bit for bit and refuses another radius; a step without
``groups=`` is refused."""
import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
from multimodal_eeg_fmri_amd.bridge_utils import timeline_ids

pytestmark = pytest.mark.gpu

C, T, VOL, B, R = 8, 128, (16, 16, 16), 16, 2
LOSSES = ["infonce", "sigmoid"]
ENTRY = {"infonce": ("mm_clip_loss_own_rows_grouped", "mm_clip_loss_own_rows_masked"),
         "sigmoid": ("mm_sigmoid_loss_own_rows", "mm_sigmoid_loss_own_rows_masked")}


@pytest.fixture(autouse=True)
def _no_seed_epoch():
    ops.set_seed_epoch(None)
    yield
    ops.set_seed_epoch(None)


def _trainer(mode, lr=1e-3, radius=R, **kw):
    ops.set_seed_epoch(None)
    ops.set_dropout_seed(0x1234567)
    torch.manual_seed(0)
    tr = BridgeTrainer(eeg_channels=C, dropout=0.0, lr=lr, mode=mode, neighbour_radius=radius, **kw).train()
    tr.head.bridge.fusion.gate_net[2].p = 0.0               # (the fusion gate's hard-coded Dropout(0.2), classify only)
    return tr


@pytest.fixture(scope="module")
def batches():
    """six batches of (eeg, fmri, timeline ids, labels): two runs of 8 consecutive epochs each, in a shuffled order"""
    out = []
    for i in range(6):
        eeg, fmri = synthetic_pairs(B, C, T, VOL, seed=700 + i)
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(i))
        runs, times = perm // 8, 40 * i + perm % 8
        ids = timeline_ids(runs, times, R)
        d = (ids.long()[:, None] - ids.long()[None, :]).abs()
        assert int(((d > 0) & (d <= R)).sum(1).min()) >= 2 and int((d == 0).sum(1).max()) == 1
        out.append((eeg, fmri, ids, (perm % 2).to(torch.int64)))
    return out


def _run(tr, batches, steps, start=0, labels=False):
    rows = []
    for b in batches[start:start + steps]:
        out = tr.train_step(b[0], b[1], b[2], b[3] if labels else None)
        rows.append(torch.stack([out[k].clone() for k in ("loss", "top1_e2f", "top1_f2e")]))
    torch.cuda.synchronize()
    return torch.stack(rows)


@pytest.mark.parametrize("loss", LOSSES)
def test_graph_and_manual_steps_are_bit_identical(batches, loss):
    tm, tg = _trainer("manual", loss=loss), _trainer("graph", loss=loss)
    lm, lg = _run(tm, batches, 4), _run(tg, batches, 4)
    assert tg.capture_mode == "one graph" and len(tg._cap["graphs"]) == 1
    assert torch.isfinite(lm).all()
    assert torch.equal(lm, lg), (lm - lg).abs().max().item()
    assert torch.equal(tm.bucket.p, tg.bucket.p)
    # and the neighbours matter: the grouped trainer's first step (the same weights) has more negatives in every row
    l0 = _run(_trainer("manual", radius=0, loss=loss), batches, 1)
    print(f"{loss}: masked {lm[:, 0].tolist()} grouped first step {l0[0, 0].item()}")
    assert l0[0, 0].item() > lm[0, 0].item()


@pytest.mark.parametrize("loss,classify", [("infonce", False), ("sigmoid", False), ("infonce", True)],
                         ids=["infonce", "sigmoid", "infonce-classify"])
def test_autograd_mode_agrees_with_the_manual_step(batches, loss, classify):
    """loss and gradients of the two surfaces at the tolerance tests/test_clip_bank_trainer_gpu.py uses for this pair (1e-5);
    with the classification branch the total loss, at the tolerance tests/test_bridge_cls_trainer_gpu.py uses for it (1e-5;
    that file bounds the classifier's own gradients, which do not pass through the contrastive loss, and no others)"""
    got = {}
    kw = dict(classify=True, ce_weight=0.5) if classify else {}
    for mode in ("manual", "autograd"):
        tr = _trainer(mode, lr=0.0, loss=loss, **kw)
        tr.grad_clip = 0.0
        probe = []
        real = tr._seg_adamw
        tr._seg_adamw = lambda probe=probe, tr=tr, real=real: (probe.append(tr.bucket.g.clone()), real())[1]
        losses = _run(tr, batches, 2, labels=classify)
        got[mode] = (losses, probe[1], tr)
    (lm, gm, tm), (la, ga, ta) = got["manual"], got["autograd"]
    assert (lm[:, 0] - la[:, 0]).abs().max().item() <= 1e-5, (lm, la)
    _, _, lo, hi = tm.groups[-1]
    assert ga[lo:hi].abs().max().item() > 0
    if classify:
        return
    print(f"fMRI group gradient diff {(gm[lo:hi] - ga[lo:hi]).abs().max().item():.3e}, whole bucket {(gm - ga).abs().max().item():.3e}")
    assert (gm[lo:hi] - ga[lo:hi]).abs().max().item() <= 1e-5


def _step_launches(tr, batch, monkeypatch, labels=False):
    args = batch if labels else batch[:3]
    tr.train_step(*args)                                     # the first step records the weight list
    calls = []
    real = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    tr.train_step(*args)
    monkeypatch.setattr(_hip, "call", real)
    torch.cuda.synchronize()
    return calls


@pytest.mark.parametrize("loss,classify", [("infonce", False), ("sigmoid", False), ("infonce", True)],
                         ids=["infonce", "sigmoid", "infonce-classify"])
def test_the_step_launches_the_masked_entry_point_in_place_of_the_grouped_one(batches, monkeypatch, loss, classify):
    kw = dict(classify=True, ce_weight=0.5) if classify else {}
    grouped = _step_launches(_trainer("manual", radius=0, loss=loss, **kw), batches[0], monkeypatch, classify)
    masked = _step_launches(_trainer("manual", loss=loss, **kw), batches[0], monkeypatch, classify)
    old, new = ENTRY[loss]
    assert grouped.count(old) == 1 and new not in grouped
    assert masked == [new if n == old else n for n in grouped]
    eval_calls = []
    tr = _trainer("manual", loss=loss, **kw)
    real = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (eval_calls.append(name), real(name, *a))[1])
    tr.evaluate(*(batches[0] if classify else batches[0][:3]))
    monkeypatch.setattr(_hip, "call", real)
    assert new in eval_calls and old not in eval_calls


def test_checkpoint_resumes_bit_for_bit_and_refuses_another_radius(batches, tmp_path):
    a = _trainer("graph")
    _run(a, batches, 3)
    path = str(tmp_path / "ck.pt")
    a.save_checkpoint(path, epoch=1)
    assert torch.load(path, map_location="cpu", weights_only=True)["bridge_trainer_state"]["neighbour_radius"] == R
    want = _run(a, batches, 3, 3)
    torch.manual_seed(11)
    b = BridgeTrainer(eeg_channels=C, dropout=0.0, lr=1e-3, mode="graph", neighbour_radius=R).train()
    b.load_checkpoint(path)
    got = _run(b, batches, 3, 3)
    assert torch.equal(want, got), (want, got)
    for x, y in zip((a.bucket.p, a.bucket.m, a.bucket.v, a.bucket.state), (b.bucket.p, b.bucket.m, b.bucket.v, b.bucket.state)):
        assert torch.equal(x, y)
    with pytest.raises(ValueError, match="neighbour_radius differs"):
        _trainer("graph", radius=0).load_checkpoint(path)
    with pytest.raises(ValueError, match="neighbour_radius differs"):
        _trainer("graph", radius=R + 1).load_checkpoint(path)


@pytest.mark.parametrize("mode", ["graph", "manual", "autograd"])
def test_a_step_without_groups_is_refused(batches, mode):
    tr = _trainer(mode)
    e, f, g, _ = batches[0]
    with pytest.raises(ValueError, match="groups="):
        tr.train_step(e, f)
    with pytest.raises(ValueError, match="groups="):
        tr.evaluate(e, f)
    assert torch.isfinite(tr.train_step(e, f, g)["loss"]).item()


def test_the_packed_host_fed_path_carries_the_ids(batches):
    """`train_step_packed` replays the captured masked step: the ids travel in the packed batch as for a grouped one"""
    runs = []
    for packed in (False, True):
        tr = _trainer("graph")
        losses = [tr.train_step(*batches[0][:3])["loss"].clone()]
        for e, f, g, _ in batches[1:3]:
            if packed:
                losses.append(tr.train_step_packed(tr.pack_host_batch(e, f, groups=g).cuda(non_blocking=True))["loss"].clone())
            else:
                losses.append(tr.train_step(e, f, g)["loss"].clone())
        torch.cuda.synchronize()
        runs.append((torch.stack(losses), tr))
    (l0, t0), (l1, t1) = runs
    assert torch.equal(l0, l1), (l0, l1)
    assert torch.equal(t0.bucket.p, t1.bucket.p)
