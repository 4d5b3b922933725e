"""BridgeTrainer(bank_size=K) at a small shape (8 channels, 128 samples, 16^3 volumes, 16 pairs; K = 40, so the ring wraps
inside the third push; dropout 0): the graph replay and the eager tape train bit-identically while the bank fills and
wraps, in plain and grouped runs, with ONE capture; the autograd surface agrees with the tape; the first step (and every
step of the warm-up) is the default trainer's, the next one is not; a checkpoint with a partly wrapped bank resumes bit
for bit; classify and the tabular encoder compose; the read-only calls leave the bank alone; a trainer without a bank
launches what it launched before."""
import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
from multimodal_eeg_fmri_amd.bridge_trainer import (BridgeTrainer, synthetic_pairs, synthetic_subject_pairs,
                                                    synthetic_tabular_pairs)
from multimodal_eeg_fmri_amd.fmri_utils import fMRITabularEncoder
from test_fmri_tab_trainer_gpu import DEFAULT_STEP_LAUNCHES

pytestmark = pytest.mark.gpu

C, T, VOL, B, K = 8, 128, (16, 16, 16), 16, 40


@pytest.fixture(autouse=True)
def _no_seed_epoch():
    ops.set_seed_epoch(None)
    yield
    ops.set_seed_epoch(None)


def _trainer(mode, lr=1e-3, **kw):
    ops.set_seed_epoch(None)
    ops.set_dropout_seed(0x1234567)
    torch.manual_seed(0)
    tr = BridgeTrainer(eeg_channels=C, dropout=0.0, lr=lr, mode=mode, **kw).train()
    tr.head.bridge.fusion.gate_net[2].p = 0.0               # (the fusion gate's hard-coded Dropout(0.2), classify only)
    return tr


@pytest.fixture(scope="module")
def batches():
    """six batches of (eeg, fmri, group ids, labels): 4 subjects x 4 epochs, shuffled; consecutive batches share two subject
    ids, so a grouped bank holds positives of the running batch"""
    out = []
    for i in range(6):
        eeg, fmri, g = synthetic_subject_pairs(4, 4, C, T, VOL, seed=600 + i)
        perm = torch.randperm(eeg.shape[0], generator=torch.Generator().manual_seed(i))
        gids = g.cpu()[perm]
        out.append((eeg[perm.cuda()].contiguous(), fmri[perm.cuda()].contiguous(), (gids + 2 * i).to(torch.int32),
                    (gids % 2).to(torch.int64)))
    return out


@pytest.fixture(scope="module")
def plain_batches():
    """one volume per pair: no two keys are equal up to rounding"""
    return [synthetic_pairs(B, C, T, VOL, seed=650 + i) for i in range(6)]


def _run(tr, batches, steps, grouped, start=0):
    rows = []
    for b in batches[start:start + steps]:
        out = tr.train_step(b[0], b[1], b[2] if grouped else None)
        rows.append(torch.stack([out[k].clone() for k in ("loss", "top1_e2f", "top1_f2e")]))
    torch.cuda.synchronize()
    return torch.stack(rows)


def _bank_equal(a, b, grouped):
    assert torch.equal(a._bank.state, b._bank.state), (a._bank.state.tolist(), b._bank.state.tolist())
    assert torch.equal(a._bank.bank, b._bank.bank)
    if grouped:
        assert torch.equal(a._bank.gid, b._bank.gid)


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_graph_and_manual_steps_are_bit_identical_while_the_ring_fills_and_wraps(batches, plain_batches, grouped):
    data = batches if grouped else plain_batches
    tm, tg = _trainer("manual", bank_size=K), _trainer("graph", bank_size=K)
    lm = _run(tm, data, 1, grouped)
    lg = _run(tg, data, 1, grouped)
    graph = tg._cap["graphs"][0]
    assert tg.bank_filled == B and tm.bank_filled == B      # the capture's two warm-up steps left no rows behind
    lm = torch.cat([lm, _run(tm, data, 5, grouped, 1)])
    lg = torch.cat([lg, _run(tg, data, 5, grouped, 1)])
    assert tg.capture_mode == "one graph" and len(tg._cap["graphs"]) == 1 and tg._cap["graphs"][0] is graph   # no new capture
    assert torch.isfinite(lm).all()
    assert torch.equal(lm, lg), (lm - lg).abs().max().item()
    assert torch.equal(tm.bucket.p, tg.bucket.p)
    _bank_equal(tm, tg, grouped)
    assert tg._bank.state.tolist() == [6 * B % K, K, 6, 0] and tg.bank_filled == K and tg.bank_size == K
    # the newest K rows are in the ring: the last push's rows sit right before the head
    assert tg._bank.bank.abs().sum(1).min().item() > 0


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_autograd_mode_agrees_with_the_manual_step(batches, plain_batches, grouped):
    """step 1 at learning rate 0 fills the bank and leaves the parameters alone; step 2 then has the bank in its softmax:
    loss and gradients of the two surfaces at the tolerance the trainer tests use for this pair (1e-5)"""
    data = batches if grouped else plain_batches
    got = {}
    for mode in ("manual", "autograd"):
        tr = _trainer(mode, lr=0.0, bank_size=K)
        tr.grad_clip = 0.0
        probe = []
        real = tr._seg_adamw
        tr._seg_adamw = lambda probe=probe, tr=tr, real=real: (probe.append(tr.bucket.g.clone()), real())[1]
        losses = _run(tr, data, 2, grouped)
        got[mode] = (losses, probe[1], tr)
    (lm, gm, tm), (la, ga, ta) = got["manual"], got["autograd"]
    assert tm.bank_filled == 2 * B and ta.bank_filled == 2 * B
    assert (tm._bank.bank - ta._bank.bank).abs().max().item() <= 1e-5
    assert (lm[:, 0] - la[:, 0]).abs().max().item() <= 1e-5, (lm, la)
    _, _, lo, hi = tm.groups[-1]
    assert ga[lo:hi].abs().max().item() > 0
    print(f"fMRI group gradient diff {(gm[lo:hi] - ga[lo:hi]).abs().max().item():.3e}, whole bucket {(gm - ga).abs().max().item():.3e}")
    assert (gm[lo:hi] - ga[lo:hi]).abs().max().item() <= 1e-5


def test_first_step_is_the_default_trainers_and_the_second_is_not(plain_batches):
    d, b = _trainer("graph"), _trainer("graph", bank_size=K)
    ld, lb = _run(d, plain_batches, 2, False)[:, 0], _run(b, plain_batches, 2, False)[:, 0]
    print(f"default {ld.tolist()} bank {lb.tolist()}")
    assert abs(lb[0].item() - ld[0].item()) <= 1e-6 * abs(ld[0].item())
    assert b.bank_filled == 2 * B
    # 16 more negatives in every softmax and the same positive: the loss can only be larger
    assert lb[1].item() != ld[1].item() and lb[1].item() > ld[1].item()
    one = _trainer("graph", bank_size=K)
    _run(one, plain_batches, 1, False)
    assert one.bank_filled == B


def test_warmup_steps_are_the_default_trainers_while_the_bank_fills(plain_batches, monkeypatch):
    """bank_warmup = 2: the bank fills during steps 1 and 2 without counting, and counts at step 3.  The bound on the warm-up
    steps is the first step's, 1e-6 relative to the default trainer's loss.  It holds on a step AFTER an optimizer update
    only because the warm-up steps launch the in-batch loss itself (and the push): mm_clip_bank_loss at n = 0 agrees with it
    to rounding, and a default trainer whose step-1 dz carries noise of 1e-7 x max|dz| already differs from itself by 4.5e-5
    at step 2 (AdamW's g / (|g| + eps); profiles/clip_bank_ab.txt).  In graph mode the step is captured again when the
    warm-up ends, and only then."""
    w = 2
    d, b = _trainer("graph"), _trainer("graph", bank_size=K, bank_warmup=w)
    ld = _run(d, plain_batches, w + 2, False)[:, 0]
    lb = _run(b, plain_batches, w, False)[:, 0]
    warm_graph = b._cap["graphs"][0]
    assert b._cap["bank_live"] is False and b._bank.state.tolist() == [w * B % K, w * B, w, 0]
    lb = torch.cat([lb, _run(b, plain_batches, 1, False, w)[:, 0]])
    live_graph = b._cap["graphs"][0]
    lb = torch.cat([lb, _run(b, plain_batches, 1, False, w + 1)[:, 0]])
    assert b._cap["bank_live"] is True and live_graph is not warm_graph and b._cap["graphs"][0] is live_graph
    print(f"default {ld.tolist()} bank(warmup={w}) {lb.tolist()} relative {[abs(x - y) / abs(y) for x, y in zip(lb.tolist(), ld.tolist())]}")
    assert b._bank.state.tolist() == [(w + 2) * B % K, K, w + 2, 0]     # the bank filled during the warm-up
    assert lb[w].item() > ld[w].item()                       # pushes == warmup: the 2 B bank rows count (more negatives)
    for i in range(w):
        assert abs(lb[i].item() - ld[i].item()) <= 1e-6 * abs(ld[i].item()), (i, lb[i].item(), ld[i].item())
    # graph and manual mode agree through the warm-up's end, and the launches are what the docstring says
    m = _trainer("manual", bank_size=K, bank_warmup=w)
    names, real = [], _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    lm = []
    for step in range(w + 2):
        names.clear()
        lm.append(m.train_step(*plain_batches[step])["loss"].clone())
        loss_launches = [n for n in names if n.startswith("mm_clip_") and not n.endswith("ws_floats")]
        assert loss_launches == (["mm_clip_loss_own_rows", "mm_clip_bank_push"] if step < w else ["mm_clip_bank_loss", "mm_clip_bank_push"]), (step, loss_launches)
    monkeypatch.setattr(_hip, "call", real)
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(lm), lb) and torch.equal(m.bucket.p, b.bucket.p)
    _bank_equal(m, b, False)


def test_checkpoint_with_a_partly_wrapped_bank_resumes_bit_for_bit(batches, tmp_path):
    a = _trainer("graph", bank_size=K)
    _run(a, batches, 3, True)
    assert a._bank.state.tolist() == [3 * B % K, K, 3, 0] and 3 * B % K != 0       # wrapped inside the third push
    path = str(tmp_path / "ck.pt")
    a.save_checkpoint(path, epoch=1)
    ck = torch.load(path, map_location="cpu", weights_only=True)["bridge_trainer_state"]["bank"]
    assert ck["size"] == K and ck["warmup"] == 0 and ck["grouped"] is True and ck["state"] == [3 * B % K, K, 3, 0]
    assert torch.equal(ck["rows"], a._bank.bank.cpu()) and torch.equal(ck["ids"], a._bank.gid.cpu())
    want = _run(a, batches, 3, True, 3)
    torch.manual_seed(11)
    b = BridgeTrainer(eeg_channels=C, dropout=0.0, lr=1e-3, mode="graph", bank_size=K).train()
    b.load_checkpoint(path)
    assert b.bank_filled == K
    got = _run(b, batches, 3, True, 3)
    assert torch.equal(want, got), (want, got)
    for x, y in zip((a.bucket.p, a.bucket.m, a.bucket.v, a.bucket.state), (b.bucket.p, b.bucket.m, b.bucket.v, b.bucket.state)):
        assert torch.equal(x, y)
    _bank_equal(a, b, True)
    with pytest.raises(ValueError, match="bank differs"):
        _trainer("graph").load_checkpoint(path)
    with pytest.raises(ValueError, match=r"bank\.size"):
        _trainer("graph", bank_size=2 * K).load_checkpoint(path)
    with pytest.raises(ValueError, match="reset_bank"):      # the loaded bank carries ids
        b.train_step(*batches[0][:2])


def test_classify_and_the_tabular_encoder_compose_with_a_bank(batches):
    e, f, g, y = batches[0]
    kw = dict(classify=True, ce_weight=0.5)
    d, b = _trainer("graph", **kw), _trainer("graph", bank_size=K, **kw)
    od = {k: v.item() for k, v in d.train_step(e, f, None, y).items()}
    ob = {k: v.item() for k, v in b.train_step(e, f, None, y).items()}
    assert abs(ob["contrastive_loss"] - od["contrastive_loss"]) <= 1e-6 * abs(od["contrastive_loss"]), (ob, od)
    assert abs(ob["ce_loss"] - od["ce_loss"]) <= 1e-6 * abs(od["ce_loss"]) and ob["cls_correct"] == od["cls_correct"]
    o2 = b.train_step(batches[1][0], batches[1][1], None, batches[1][3])
    assert torch.isfinite(o2["loss"]).item() and b.bank_filled == 2 * B
    torch.manual_seed(0)
    enc = fMRITabularEncoder(37, 50, hidden_dim=64, dropout=0.0)
    t = BridgeTrainer(eeg_channels=C, dropout=0.0, lr=1e-3, mode="graph", fmri_encoder=enc, bank_size=K).train()
    losses = []
    for i in range(3):
        et, ft = synthetic_tabular_pairs(B, C, T, 37, 50, seed=880 + i)
        losses.append(t.train_step(et, ft)["loss"].item())
    assert all(x == x and abs(x) < 1e4 for x in losses) and t._bank.state.tolist() == [3 * B % K, K, 3, 0]


def test_read_only_calls_leave_the_bank_alone(batches):
    tr = _trainer("graph", bank_size=K)
    _run(tr, batches, 2, True)
    before = [t.clone() for t in tr._bank.tensors()]
    e, f, g, y = batches[2]
    tr.evaluate(e, f, g)
    tr.evaluate(e, f)
    tr.evaluate_retrieval(e, f)
    tr.embed(e, f)
    with torch.no_grad():
        tr.forward(e, f, g)
    torch.cuda.synchronize()
    for x, y0 in zip(tr._bank.tensors(), before):
        assert torch.equal(x, y0)
    assert tr.training and tr.bank_filled == 2 * B


def test_the_packed_host_fed_path_carries_the_bank(batches):
    """`train_step_packed` replays the captured step: loss and push are nodes of it, the group ids travel in the packed batch"""
    runs = []
    for packed in (False, True):
        tr = _trainer("graph", bank_size=K)
        losses = [tr.train_step(*batches[0][:3])["loss"].clone()]
        for e, f, g, _ in batches[1:4]:
            if packed:
                losses.append(tr.train_step_packed(tr.pack_host_batch(e, f, groups=g).cuda(non_blocking=True))["loss"].clone())
            else:
                losses.append(tr.train_step(e, f, g)["loss"].clone())
        torch.cuda.synchronize()
        runs.append((torch.stack(losses), tr))
    (l0, t0), (l1, t1) = runs
    assert torch.equal(l0, l1), (l0, l1)
    assert torch.equal(t0.bucket.p, t1.bucket.p)
    _bank_equal(t0, t1, True)
    assert t1._bank.state.tolist() == [4 * B % K, K, 4, 0]


def test_grouping_cannot_switch_without_a_reset(batches):
    tr = _trainer("manual", bank_size=K)
    e, f, g, y = batches[0]
    tr.train_step(e, f)
    with pytest.raises(ValueError, match="reset_bank"):
        tr.train_step(e, f, g)
    assert tr.bank_filled == B
    tr.reset_bank()
    assert tr.bank_filled == 0
    tr.train_step(e, f, g)
    assert tr.bank_filled == B and tr._bank.gid[:B].cpu().tolist() == g.tolist()


def _step_launches(tr, batch, monkeypatch):
    tr.train_step(*batch)                                    # the first step records the weight list
    calls = []
    real = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    tr.train_step(*batch)
    monkeypatch.setattr(_hip, "call", real)
    torch.cuda.synchronize()
    return calls


def test_a_trainer_without_a_bank_launches_what_it_did_and_a_bank_trainer_one_more(plain_batches, monkeypatch):
    _trainer("graph", bank_size=K).train_step(*plain_batches[0])            # a bank trainer has run in this process
    d = _trainer("manual", bank_size=0)
    assert "bank" not in d.checkpoint_state()["bridge_trainer_state"] and d._bank is None
    assert _step_launches(d, plain_batches[0], monkeypatch) == DEFAULT_STEP_LAUNCHES
    want = list(DEFAULT_STEP_LAUNCHES)
    i = want.index("mm_clip_loss_own_rows")
    want[i:i + 1] = ["mm_clip_bank_loss", "mm_clip_bank_push"]
    assert _step_launches(_trainer("manual", bank_size=K), plain_batches[0], monkeypatch) == want
