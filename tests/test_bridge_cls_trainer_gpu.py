"""BridgeTrainer(classify=True) at a small shape (8 channels, 256 samples, 16^3 volumes, 16 pairs; dropout 0 unless said):
the graph replay and the eager tape train bit-identically over labelled plain and grouped batches, the autograd surface
agrees with them, the step costs exactly three more launches, the default trainer is untouched, checkpoints resume bit
for bit, `evaluate` / `predict` / `evaluate_classification` report what the fp64 oracle and `classification_metrics`
say, and training lowers the cross-entropy."""
import pytest
import torch
import torch.nn.functional as F

from multimodal_eeg_fmri_amd import _hip, ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_subject_pairs
from multimodal_eeg_fmri_amd.fmri_utils import classification_metrics
from oracle import ref_functional as RF

pytestmark = pytest.mark.gpu

C, T, VOL = 8, 256, (16, 16, 16)
CLS_PARTS = ("cross_attn", "fusion", "classifier")


@pytest.fixture(autouse=True)
def _no_seed_epoch():
    ops.set_seed_epoch(None)
    yield
    ops.set_seed_epoch(None)


def _trainer(mode, lr=1e-3, dropout=0.0, **kw):
    ops.set_seed_epoch(None)
    ops.set_dropout_seed(0x1234567)
    torch.manual_seed(0)
    tr = BridgeTrainer(eeg_channels=C, dropout=dropout, lr=lr, mode=mode, **kw).train()
    if dropout == 0.0:
        # the fusion gate's hard-coded Dropout(0.2) (enhanced_models_v4.py) is off too: a replayed step mixes its epoch
        # word into every mask, so only a step without masks is the same function in graph and manual mode
        tr.head.bridge.fusion.gate_net[2].p = 0.0
    return tr


@pytest.fixture(scope="module")
def batches():
    """(eeg, fmri, group ids, labels): 4 subjects x 4 epochs, the label is the subject's parity"""
    out = []
    for i in range(3):
        eeg, fmri, g = synthetic_subject_pairs(4, 4, C, T, VOL, seed=700 + i)
        perm = torch.randperm(eeg.shape[0], generator=torch.Generator().manual_seed(i))
        gids = g.cpu()[perm]
        out.append((eeg[perm.cuda()].contiguous(), fmri[perm.cuda()].contiguous(), (gids * 10 + i).to(torch.int32),
                    (gids % 2).to(torch.int64)))
    return out


PLAN = [(0, False), (1, True), (2, False), (0, True), (1, False)]      # labelled-plain and labelled-grouped alternate
KEYS = ("loss", "contrastive_loss", "ce_loss", "cls_correct")


def _run(tr, batches, plan):
    rows = []
    for i, grouped in plan:
        e, f, g, y = batches[i]
        out = tr.train_step(e, f, g if grouped else None, y)
        rows.append(torch.stack([out[k].clone() for k in KEYS]))
    torch.cuda.synchronize()
    return torch.stack(rows)


def test_graph_and_manual_steps_are_bit_identical_over_plain_and_grouped_batches(batches):
    kw = dict(classify=True, ce_weight=0.5, class_weight=[0.8, 1.3])
    tm, tg = _trainer("manual", **kw), _trainer("graph", **kw)
    lm = _run(tm, batches, PLAN)
    lg = _run(tg, batches, PLAN)
    assert tg.capture_mode == "one graph"
    assert torch.isfinite(lm).all()
    assert torch.equal(lm, lg), (lm - lg).abs().max().item()
    assert torch.equal(tm.bucket.p, tg.bucket.p)
    torch.testing.assert_close(lm[:, 0], lm[:, 1] + 0.5 * lm[:, 2], rtol=1e-6, atol=1e-6)    # loss = contrastive + ce_weight * ce


def test_autograd_mode_agrees_with_the_manual_step(batches):
    e, f, g, y = batches[0]
    for ids in (None, g):
        tm = _trainer("manual", classify=True, ce_weight=0.5, class_weight=[0.8, 1.3])
        tm.grad_clip = 0.0
        probe = {}
        real = tm._seg_adamw
        tm._seg_adamw = lambda: (probe.setdefault("g", tm.bucket.g.clone()), real())[1]       # the gradients, before AdamW clears them
        om = {k: v.item() for k, v in tm.train_step(e, f, ids, y).items()}
        ta = _trainer("autograd", classify=True, ce_weight=0.5, class_weight=[0.8, 1.3])
        lc, _, _, ce, _ = ta._forward_classify(e, f, ops.group_ids(ids, 16, e.device), y.to(torch.int32).cuda())
        (lc + 0.5 * ce).backward()
        assert abs(ce.item() - om["ce_loss"]) <= 1e-5 and abs(lc.item() + 0.5 * ce.item() - om["loss"]) <= 1e-5
        ta.bucket.absorb_autograd_grads()            # (the small_autograd functions add into the bucket themselves)
        for _, n, _, sl in tm.optimizer_param_map():
            if any(part in n for part in CLS_PARTS):
                got, want = probe["g"][sl], ta.bucket.g[sl]
                assert want.abs().max().item() > 0 or "in_proj_bias" in n, n
                assert (got - want).abs().max().item() <= 1e-5, (n, (got - want).abs().max().item())
        ta = _trainer("autograd", classify=True, ce_weight=0.5, class_weight=[0.8, 1.3])
        oa = {k: v.item() for k, v in ta.train_step(e, f, ids, y).items()}
        assert abs(oa["loss"] - om["loss"]) <= 1e-5 and abs(oa["ce_loss"] - om["ce_loss"]) <= 1e-5, (oa, om)
        assert oa["cls_correct"] == om["cls_correct"]


def test_a_step_moves_the_classifier_the_attention_the_heads_and_the_encoders(batches):
    tr = _trainer("graph", classify=True)
    before = {n: p.detach().clone() for n, p in tr.named_parameters()}
    e, f, g, y = batches[0]
    tr.train_step(e, f, None, y)
    torch.cuda.synchronize()
    moved = {n for n, p in tr.named_parameters() if not torch.equal(p.detach(), before[n])}
    for n in before:
        if any(part in n for part in CLS_PARTS + ("eeg_proj", "fmri_proj")):
            assert n in moved, n
    assert any(n.startswith("eeg_encoder.") for n in moved) and any(n.startswith("fmri_encoder.") for n in moved)


def test_the_step_costs_three_more_launches(batches, monkeypatch):
    import multimodal_eeg_fmri_amd._hip as hipmod
    e, f, g, y = batches[0]
    counts = {}
    for classify in (False, True):
        tr = _trainer("manual", classify=classify)
        tr.train_step(e, f, None, y if classify else None)          # the first step records the weight list
        calls = []
        real = hipmod.call
        monkeypatch.setattr(hipmod, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
        tr.train_step(e, f, None, y if classify else None)
        monkeypatch.setattr(hipmod, "call", real)
        counts[classify] = calls
    base, cls = counts[False], counts[True]
    assert len(cls) == len(base) + 3, (len(cls), len(base))
    assert cls.count("mm_proj_heads_bwd_da") == 1 and cls.count("mm_proj_heads_bwd") == 0
    assert cls.count("mm_bridge_cls_fwd") == 1 and cls.count("mm_bridge_cls_bwd") == 2
    assert base.count("mm_proj_heads_bwd") == 1 and not [n for n in base if "bridge_cls" in n or n.endswith("_da")]
    i = cls.index
    assert i("mm_proj_heads_fwd") < i("mm_bridge_cls_fwd") < i("mm_clip_loss_own_rows") < i("mm_bridge_cls_bwd") < i("mm_proj_heads_bwd_da")


def test_a_captured_step_records_three_more_launches_and_counts_on_the_trainers_own_word(batches, monkeypatch):
    """graph mode: the first step is two warm-up steps and the capture, nine launches more than a default trainer's; every
    mm_bridge_cls_fwd - the recorded one too - gets the trainer's ticket word, which exists before the capture begins"""
    import multimodal_eeg_fmri_amd._hip as hipmod
    e, f, g, y = batches[0]
    for classify in (False, True):                                  # (host-side size queries are cached from here on)
        _trainer("manual", classify=classify).train_step(e, f, None, y if classify else None)
    counts, tickets = {}, []
    real = hipmod.call

    def spy(name, *a):
        calls.append(name)
        if name == "mm_bridge_cls_fwd":
            tickets.append((a[28], torch.cuda.is_current_stream_capturing()))
        return real(name, *a)
    for classify in (False, True):
        tr = _trainer("graph", classify=classify)
        calls = []
        monkeypatch.setattr(hipmod, "call", spy)
        tr.train_step(e, f, None, y if classify else None)
        n_first = len(calls)
        tr.train_step(e, f, None, y if classify else None)          # a replay: staging only
        monkeypatch.setattr(hipmod, "call", real)
        counts[classify] = (n_first, len(calls) - n_first)
    assert counts[True][0] == counts[False][0] + 9 and counts[True][1] == counts[False][1], counts
    assert len(tickets) == 3 and [cap for _, cap in tickets] == [False, False, True]
    assert all(t is tr._cls_ticket for t, _ in tickets)
    torch.cuda.synchronize()
    assert tr._cls_ticket.item() == 0 and tr._cls_ticket.dtype == torch.int32


def test_two_classify_trainers_on_two_streams_do_not_share_a_word(batches):
    e, f, g, y = batches[0]
    ta, tb = _trainer("graph", classify=True), _trainer("graph", classify=True)
    want = ta.train_step(e, f, None, y)["ce_loss"].item()
    sb = torch.cuda.Stream()
    sb.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(sb):
        got = tb.train_step(e, f, None, y)["ce_loss"]
    sb.synchronize()
    assert ta._cls_ticket is not tb._cls_ticket and ta._cls_ticket.data_ptr() != tb._cls_ticket.data_ptr()
    assert got.item() == want and ta._cls_ticket.item() == 0 and tb._cls_ticket.item() == 0


def test_the_default_trainer_is_unchanged(batches):
    e, f, g, y = batches[0]
    _trainer("graph", classify=True).train_step(e, f, None, y)          # a classify trainer has run in this process
    d = _trainer("graph", classify=False, ce_weight=1.0, class_weight=None, num_classes=2)
    assert d._scal.numel() == 4 and "classify" not in d.checkpoint_state()["bridge_trainer_state"]
    ops.set_seed_epoch(None)
    ops.set_dropout_seed(0x1234567)
    torch.manual_seed(0)
    k = BridgeTrainer(eeg_channels=C, dropout=0.0, lr=1e-3, mode="graph").train()      # built without the keywords
    for ids in (None, g):
        a, b = d.train_step(e, f, ids), k.train_step(e, f, ids)
        assert set(a) == {"loss", "top1_e2f", "top1_f2e"}
        assert torch.equal(a["loss"].clone(), b["loss"].clone())
    assert torch.equal(d.bucket.p, k.bucket.p)


def test_checkpoint_resumes_bit_for_bit_and_names_what_differs(batches, tmp_path):
    kw = dict(classify=True, ce_weight=0.5, dropout=0.2)
    a = _trainer("graph", **kw)
    plan = [(0, False), (1, False), (2, False), (0, False)]      # one kind of batch: one capture, as test_checkpoint_gpu resumes it
    _run(a, batches, plan[:2])
    path = str(tmp_path / "ck.pt")
    a.save_checkpoint(path, epoch=1)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["bridge_trainer_state"]["classify"] == {"ce_weight": 0.5, "num_classes": 2, "class_weight": None}
    want = _run(a, batches, plan[2:])
    torch.manual_seed(11)
    b = BridgeTrainer(eeg_channels=C, lr=1e-3, mode="graph", **kw).train()
    b.load_checkpoint(path)
    got = _run(b, batches, plan[2:])
    assert torch.equal(want, got), (want, got)
    for x, y in zip((a.bucket.p, a.bucket.m, a.bucket.v, a.bucket.state), (b.bucket.p, b.bucket.m, b.bucket.v, b.bucket.state)):
        assert torch.equal(x, y)
    with pytest.raises(ValueError, match="ce_weight"):
        _trainer("graph", classify=True, ce_weight=1.0, dropout=0.2).load_checkpoint(path)
    with pytest.raises(ValueError, match="classify"):
        _trainer("graph", dropout=0.2).load_checkpoint(path)


def _oracle_eval(tr, e, f, y, cw):
    """fp64 bridge on the trainer's own encoder features -> (logits, ce, correct, fusion_w, attn_w)"""
    was = tr.training
    tr.eval()
    with torch.no_grad():
        fe, ff = tr.eeg_encoder(e).double().cpu(), tr.fmri_encoder(f).double().cpu()
    tr.train(was)
    sd = {k: v.detach().double().cpu() for k, v in tr.head.bridge.state_dict().items()}
    logits, _, fw, aw = RF.bridge_net(sd, fe, ff, nhead=tr.head.bridge.num_heads)
    ce = F.cross_entropy(logits, y.cpu().long(), weight=None if cw is None else torch.tensor(cw, dtype=torch.float64))
    return logits, ce.item(), float((logits.argmax(1) == y.cpu()).sum()), fw, aw.reshape(-1, 2)


def test_evaluate_predict_and_metrics(batches):
    cw = [0.8, 1.3]
    tr = _trainer("graph", classify=True, ce_weight=0.5, class_weight=cw)
    _run(tr, batches, PLAN[:3])
    e, f, g, y = batches[1]
    s0 = dict(ops._seed_state)
    pred = tr.predict(e.cpu(), f, batch_size=5)                 # host input, uneven chunks
    assert ops._seed_state == s0 and tr.training
    logits, ce, correct, fw, aw = _oracle_eval(tr, e, f, y, cw)
    torch.testing.assert_close(pred["logits"].double().cpu(), logits, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(pred["fusion_weights"].double().cpu(), fw, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(pred["attn_weights"].double().cpu(), aw, rtol=1e-4, atol=1e-5)
    assert torch.equal(pred["pred"], pred["logits"].argmax(dim=1))
    torch.testing.assert_close(pred["probs"], torch.softmax(pred["logits"], dim=1))
    for ids in (None, g):
        out = tr.evaluate(e, f, ids, labels=y)
        assert abs(out["ce_loss"].item() - ce) <= 1e-4 and out["cls_correct"].item() == correct
        plain = _trainer_eval_contrastive(tr, e, f, ids)
        assert abs(out["contrastive_loss"].item() - plain) <= 1e-6
        assert abs(out["loss"].item() - (plain + 0.5 * out["ce_loss"].item())) <= 1e-5
    assert ops._seed_state == s0
    got = tr.evaluate_classification(e, f, y, batch_size=7)
    want = classification_metrics(y.numpy(), pred["pred"].cpu().numpy(), pred["probs"].cpu().numpy(), 2)
    assert got == want and set(got) == {"Accuracy", "F1", "Precision", "Recall", "AUC"}
    # `predict` is available on any trainer
    d = _trainer("graph")
    assert d.predict(e, f)["logits"].shape == (16, 2)


def _trainer_eval_contrastive(tr, e, f, ids):
    """the contrastive eval loss through the surface every trainer has (`forward` in eval mode)"""
    was = tr.training
    tr.eval()
    ops.weights_changed()
    with torch.no_grad():
        loss = tr.forward(e, f, ids)[0].item()
    tr.train(was)
    return loss


def test_thirty_steps_on_one_batch_lower_the_cross_entropy(batches):
    tr = _trainer("graph", lr=1e-3, classify=True)
    e, f, g, y = batches[0]
    ces = [tr.train_step(e, f, None, y)["ce_loss"].item() for _ in range(30)]
    assert ces[-1] < ces[0], (ces[0], ces[-1])


def test_fit_reports_and_monitors_classification_accuracy(batches):
    tr = _trainer("graph", classify=True)
    train = [(b[0], b[1], None, b[3]) for b in batches[:2]]
    e, f, g, y = batches[2]
    hist = tr.fit(train, 2, val=(e, f, None, y), warmup_epochs=0, monitor="classification.Accuracy", patience=10)
    assert len(hist) == 2
    for h in hist:
        acc = h["val"]["classification"]["Accuracy"]
        assert 0.0 <= acc <= 1.0 and h["monitor"] == acc
        assert "eeg_to_fmri" in h["val"]
