"""BridgeTrainer(key_encoder=True) at the bank trainer test's small shape (8 channels x 128 samples, 16^3 volumes, 16 pairs,
K = 40: the ring wraps inside the third push; dropout 0 unless stated): graph replay and eager tape train bit-identically
while the ring fills and wraps; the autograd surface agrees with the tape; the rows a step pushes are the batch's embeddings
under the AVERAGED weights and the running statistics as they stood BEFORE the step; nothing reaches the keys; one capture
serves warm-up and live bank; a checkpoint resumes bit for bit; the launch lists; and the compositions.

Tolerances.  Autograd against manual: 1e-5 on the loss and on the fMRI group's gradient, what
tests/test_clip_bank_trainer_gpu.py uses for the same comparison.  Pushed rows against the module surface (`embed` inside
`ema_weights()`): 1e-5 absolute on unit-norm rows, the project's bound for the tape against the module forward of the same
weights (tests/test_clip_bank_trainer_gpu.py, tests/test_fmri_tab_trainer_gpu.py); the figure is printed - both run the same
eval kernels, and it was 0 in graph and manual mode at all four steps - and the wrong weights (2.7e-2 .. 4.1e-2) or the wrong
statistics (9.5e-2) miss it by three orders of magnitude (asserted below at > 1e-2, so that the check cannot pass vacuously)."""
import types

import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops, optim
from multimodal_eeg_fmri_amd.bridge_trainer import (BridgeTrainer, synthetic_pairs, synthetic_subject_pairs,
                                                    synthetic_tabular_pairs)
from multimodal_eeg_fmri_amd.crossmodal_eeg_scr import EEGTimeTransforms, EEGTransforms
from multimodal_eeg_fmri_amd.fmri_utils import VolumeTransforms, fMRITabularEncoder
from test_fmri_tab_trainer_gpu import DEFAULT_STEP_LAUNCHES

pytestmark = pytest.mark.gpu

C, T, VOL, B, K = 8, 128, (16, 16, 16), 16, 40
KEY = dict(bank_size=K, ema_decay=0.99, key_encoder=True)


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
        tr.head.bridge.fusion.gate_net[2].p = 0.0           # (the fusion gate's hard-coded Dropout(0.2), classify only)
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


def _training_state_equal(a, b):
    for x, y in zip((a.bucket.p, a.bucket.m, a.bucket.v, a.bucket.state, a.bucket.ema),
                    (b.bucket.p, b.bucket.m, b.bucket.v, b.bucket.state, b.bucket.ema)):
        assert torch.equal(x, y)
    assert all(torch.equal(x, y) for x, y in zip(a.buffers(), b.buffers()))


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_graph_and_manual_steps_are_bit_identical_while_the_ring_fills_and_wraps(batches, plain_batches, grouped):
    data = batches if grouped else plain_batches
    tm, tg = _trainer("manual", **KEY), _trainer("graph", **KEY)
    lm = _run(tm, data, 1, grouped)
    lg = _run(tg, data, 1, grouped)
    graph = tg._cap["graphs"][0]
    assert tg.bank_filled == B and tm.bank_filled == B      # the capture's two warm-up steps left no rows behind
    lm = torch.cat([lm, _run(tm, data, 5, grouped, 1)])
    lg = torch.cat([lg, _run(tg, data, 5, grouped, 1)])
    assert tg.capture_mode == "one graph" and len(tg._cap["graphs"]) == 1 and tg._cap["graphs"][0] is graph   # no new capture
    assert torch.isfinite(lm).all()
    assert torch.equal(lm, lg), (lm - lg).abs().max().item()
    _training_state_equal(tm, tg)
    _bank_equal(tm, tg, grouped)
    assert tg._bank.state.tolist() == [6 * B % K, K, 6, 0] and tg.bank_filled == K
    assert tg._bank.bank.abs().sum(1).min().item() > 0
    # the keys are not the queries: a bank trainer's losses on the same batches differ from step 1 on
    lb = _run(_trainer("graph", bank_size=K, ema_decay=0.99), data, 2, grouped)
    assert lb[1, 0].item() != lg[1, 0].item()


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_autograd_mode_agrees_with_the_manual_step(batches, plain_batches, grouped):
    """step 1 at learning rate 0 fills the bank and leaves the parameters alone; step 2 then has the bank in its softmax:
    loss and gradients of the two surfaces at the tolerance tests/test_clip_bank_trainer_gpu.py uses for this pair (1e-5)"""
    data = batches if grouped else plain_batches
    got = {}
    for mode in ("manual", "autograd"):
        tr = _trainer(mode, lr=0.0, **KEY)
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


def _pushed_rows(tr, head_before):
    slots = [(head_before + i) % K for i in range(B)]
    return tr._bank.bank[slots].clone()


@pytest.mark.parametrize("mode", ["graph", "manual"])
def test_pushed_rows_are_the_averaged_weights_embeddings_under_the_statistics_before_the_step(plain_batches, mode):
    tr = _trainer(mode, **KEY)
    worst = 0.0
    for t, (eeg, fmri) in enumerate(plain_batches[:4]):
        # before step t: the batch under the averaged weights, eval form, through the module surface
        with tr.ema_weights():
            ze, zf = tr.embed(eeg, fmri)
        want = torch.cat([ze, zf], dim=1)
        live = torch.cat(tr.embed(eeg, fmri), dim=1)
        head = 0 if tr._bank is None else int(tr._bank.state[0].item())
        stats_before = [b.clone() for b in tr.buffers()]
        tr.train_step(eeg, fmri)
        torch.cuda.synchronize()
        got = _pushed_rows(tr, head)
        err = (got - want).abs().max().item()
        worst = max(worst, err)
        print(f"{mode} step {t}: pushed rows vs ema_weights() + eval(): {err:.3e}; vs the live weights {(got - live).abs().max().item():.3e}")
        assert err <= 1e-5
        assert any(not torch.equal(x, y) for x, y in zip(stats_before, tr.buffers()))      # the online pass did update them
        if t >= 1:       # the average differs from the weights by now: the online weights' rows are NOT what was pushed
            assert (got - live).abs().max().item() > 1e-2
        # and the same weights under the statistics AFTER the step are not either
        if t == 3:
            with tr.ema_weights():
                after = torch.cat(tr.embed(eeg, fmri), dim=1)
            print(f"  same batch under the statistics after the step: {(after - want).abs().max().item():.3e}")
            assert (after - want).abs().max().item() > 1e-2
    assert not torch.equal(tr.bucket.ema, tr.bucket.p)


def test_nothing_reaches_the_keys(plain_batches):
    """`bucket.ema` after a step is what the parent's update gives from the step's own gradients (the same host call on
    copies of the buffers, bit for bit) - and within the parent's one-step bound of the fp64 rule on the new weights; the
    twins hold no gradient"""
    from test_ema_host import ema_reference
    tr = _trainer("manual", **KEY)
    _run(tr, plain_batches, 2, False)
    snap = {}
    real = tr._seg_adamw

    def spy():
        b = tr.bucket
        snap.update({k: getattr(b, k).clone() for k in ("p", "g", "m", "v", "state", "ema")}, n=b.n)
        real()
    tr._seg_adamw = spy
    _run(tr, plain_batches, 1, False, 2)
    ema_old = snap["ema"].clone()
    copy = types.SimpleNamespace(**snap)
    optim.adamw_update(copy, tr.betas, tr.eps, tr.grad_clip, 1.0, 1, None, tr.weight_decay, tr.ema_decay, tr.ema_warmup)
    torch.cuda.synchronize()
    assert torch.equal(copy.p, tr.bucket.p) and torch.equal(copy.ema, tr.bucket.ema)
    d = tr.bucket.state[5].double().item()
    ref = ema_reference(ema_old.cpu(), tr.bucket.p.cpu(), d)
    bound = 8 * 2.0 ** -24 * torch.maximum(tr.bucket.p.cpu().abs(), ema_old.cpu().abs()).double()
    assert bool(((tr.bucket.ema.cpu().double() - ref).abs() <= bound).all())
    for name, twin in tr._key.items():
        mods = [twin.eeg_proj, twin.fmri_proj] if name == "bridge" else [twin]
        for m in mods:
            for p in m.parameters():
                assert not p.requires_grad and p.grad is None and not hasattr(p, "_mm_grad")


def test_parameters_state_dict_and_bucket_are_those_of_the_trainer_without_a_key_encoder():
    a, b = _trainer("graph", **KEY), _trainer("graph", bank_size=K, ema_decay=0.99)
    assert list(a.state_dict()) == list(b.state_dict())
    assert [tuple(p.shape) for p in a.parameters()] == [tuple(p.shape) for p in b.parameters()]
    assert a.bucket.n == b.bucket.n and a.groups == b.groups
    assert torch.equal(a.bucket.p, b.bucket.p)
    assert set(a.checkpoint_state()["model_state_dict"]) == set(b.checkpoint_state()["model_state_dict"])


def test_one_capture_serves_the_warmup_and_the_live_bank(plain_batches, monkeypatch):
    """bank_warmup = 2: the same kernel runs with n = 0 on the device during steps 1 and 2 (their loss is the loss against
    the batch's keys alone), the bank counts at step 3, and the step is captured ONCE"""
    w = 2
    captures = []
    real_capture = BridgeTrainer._capture
    monkeypatch.setattr(BridgeTrainer, "_capture", lambda self, *a, **k: (captures.append(1), real_capture(self, *a, **k))[1])
    g = _trainer("graph", bank_warmup=w, **KEY)
    lg = _run(g, plain_batches, 1, False)
    graph = g._cap["graphs"][0]
    words = [g._bank.state.tolist()]
    for i in range(1, w + 2):
        lg = torch.cat([lg, _run(g, plain_batches, 1, False, i)])
        words.append(g._bank.state.tolist())
    assert len(captures) == 1 and g._cap["graphs"][0] is graph and g._cap["bank_live"] is True
    assert words == [[(i + 1) * B % K, min((i + 1) * B, K), i + 1, 0] for i in range(w + 2)]
    m = _trainer("manual", bank_warmup=w, **KEY)
    names, real = [], _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    lm = []
    for step in range(w + 2):
        names.clear()
        lm.append(m.train_step(*plain_batches[step])["loss"].clone())
        assert [n for n in names if n.startswith("mm_clip_") and not n.endswith("ws_floats")] == ["mm_clip_key_loss", "mm_clip_bank_push"]
    monkeypatch.setattr(_hip, "call", real)
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(lm), lg[:, 0])
    _training_state_equal(m, g)
    _bank_equal(m, g, False)
    # without a warm-up the bank counts from step 2 on: step 1 is the same step, step 2 has 16 more negatives
    l0 = _run(_trainer("graph", **KEY), plain_batches, 2, False)[:, 0]
    print(f"warmup {w}: {lg[:, 0].tolist()}  no warm-up: {l0.tolist()}")
    assert l0[0].item() == lg[0, 0].item() and l0[1].item() > lg[1, 0].item()


def test_checkpoint_with_a_partly_wrapped_bank_resumes_bit_for_bit(batches, tmp_path):
    a = _trainer("graph", **KEY)
    _run(a, batches, 3, True)
    assert a._bank.state.tolist() == [3 * B % K, K, 3, 0] and 3 * B % K != 0       # wrapped inside the third push
    path = str(tmp_path / "ck.pt")
    a.save_checkpoint(path, epoch=1)
    ck = torch.load(path, map_location="cpu", weights_only=True)["bridge_trainer_state"]
    assert ck["bank"]["key_encoder"] is True and ck["bank"]["state"] == [3 * B % K, K, 3, 0]
    assert torch.equal(ck["bank"]["rows"], a._bank.bank.cpu()) and torch.equal(ck["ema"]["shadow"], a.bucket.ema.cpu())
    want = _run(a, batches, 3, True, 3)
    torch.manual_seed(11)
    b = BridgeTrainer(eeg_channels=C, dropout=0.0, lr=1e-3, mode="graph", **KEY).train()
    b.load_checkpoint(path)
    got = _run(b, batches, 3, True, 3)
    assert torch.equal(want, got), (want, got)
    _training_state_equal(a, b)
    _bank_equal(a, b, True)
    with pytest.raises(ValueError, match=r"bank\.key_encoder differs"):
        _trainer("graph", bank_size=K, ema_decay=0.99).load_checkpoint(path)
    plain = str(tmp_path / "plain.pt")
    _trainer("graph", bank_size=K, ema_decay=0.99).save_checkpoint(plain, epoch=0)
    with pytest.raises(ValueError, match=r"bank\.key_encoder differs"):
        _trainer("graph", **KEY).load_checkpoint(plain)


# ---------------------------------------------------------------- launch lists
def _step_launches(tr, batch, monkeypatch):
    tr.train_step(*batch)                                    # the first step records the weight list
    calls = []
    real = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    tr.train_step(*batch)
    monkeypatch.setattr(_hip, "call", real)
    torch.cuda.synchronize()
    return [n for n in calls if not n.endswith("ws_floats")]


def _eval_form_launches(tr, batch, monkeypatch):
    """the launches of each encoder branch's eval form (`live=False`), recorded on a trainer's own modules - without the
    weight-image launches: inside a step the images are the recorded list's, built by its one mm_prep_many_zero"""
    eeg, fmri = batch
    out = []
    real = _hip.call
    for fn in (lambda: tr._eeg.forward(tr.eeg_encoder, eeg, None, False), lambda: tr._fmri.forward(tr.fmri_encoder, fmri, False)):
        calls = []
        monkeypatch.setattr(_hip, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
        with torch.no_grad():
            fn()
        monkeypatch.setattr(_hip, "call", real)
        out.append([n for n in calls if n != "mm_prep_conv_weight"])
    torch.cuda.synchronize()
    return out


def test_launch_lists(plain_batches, monkeypatch):
    batch = plain_batches[0]
    _trainer("graph", **KEY).train_step(*batch)              # a key trainer has run in this process
    assert _step_launches(_trainer("manual"), batch, monkeypatch) == DEFAULT_STEP_LAUNCHES
    bank = list(DEFAULT_STEP_LAUNCHES)
    i = bank.index("mm_clip_loss_own_rows")
    bank[i:i + 1] = ["mm_clip_bank_loss", "mm_clip_bank_push"]
    assert _step_launches(_trainer("manual", bank_size=K), batch, monkeypatch) == bank
    bank[-1] = "mm_adamw_clip_ema"
    ref = _trainer("manual", bank_size=K, ema_decay=0.99)
    assert _step_launches(ref, batch, monkeypatch) == bank
    eeg_eval, fmri_eval = _eval_form_launches(ref, batch, monkeypatch)
    assert len(eeg_eval) > 3 and "mm_attn_fwd" in eeg_eval and len(fmri_eval) > 3 and "mm_conv3d_l1" in fmri_eval

    def with_key_pass(base, fmri_twin):
        want = list(base)
        want[want.index("mm_clip_bank_loss")] = "mm_clip_key_loss"
        j = want.index("mm_proj_heads_fwd")
        want.insert(j + 1, "mm_proj_heads_fwd")              # the twin heads
        if fmri_twin:
            f = want.index("mm_conv3d_l1_gram")
            want[f:f] = fmri_eval                            # in front of the online fMRI pass
        want[1:1] = eeg_eval                                 # in front of the online EEG pass (behind the weight images)
        return want
    got = _step_launches(_trainer("manual", **KEY), batch, monkeypatch)
    assert got == with_key_pass(bank, True), got
    # a frozen encoder has no twin: no second fMRI launch
    frozen = _step_launches(_trainer("manual", bank_size=K, ema_decay=0.99, freeze=("fmri_encoder",)), batch, monkeypatch)
    got = _step_launches(_trainer("manual", freeze=("fmri_encoder",), **KEY), batch, monkeypatch)
    assert got == with_key_pass(frozen, False), got
    for name in ("mm_conv3d_l1", "mm_conv3d_fwd"):               # (the frozen encoder's online pass is the eval form)
        assert got.count(name) == frozen.count(name) > 0


# ---------------------------------------------------------------- compositions, at dropout 0.1
def _graph_and_manual(make, step, steps):
    """``steps`` steps of make("graph") and of make("manual") on the same dropout stream -> (graph losses, manual losses,
    the two trainers).  A captured step's seeds are those its capture drew (after its two eager warm-up steps) mixed with
    the device epoch word, which every update launch advances; the eager run is given exactly that stream: the same
    counter value before every step, and an epoch word of its own holding the value the replay read."""
    tg = make("graph")
    lg = [step(tg, 0)]
    per_step = (ops._seed_state["step"] - tg._cap["seed_step"]) // 3       # the capture drew 3 steps' seeds
    lg += [step(tg, i) for i in range(1, steps)]
    torch.cuda.synchronize()
    first_epoch = int(tg._cap["epoch"].item()) - steps
    counter = tg._cap["seed_step"] + 2 * per_step
    tm = make("manual")
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.set_seed_epoch(word)
    lm = []
    for i in range(steps):
        ops._seed_state["step"] = counter
        word.fill_(first_epoch + i)
        lm.append(step(tm, i))
    torch.cuda.synchronize()
    ops.set_seed_epoch(None)
    return torch.stack(lg), torch.stack(lm), tg, tm


def test_classify_and_the_tabular_encoder_compose():
    feed = [synthetic_tabular_pairs(B, C, T, 37, 50, seed=880 + i) for i in range(3)]
    labels = [(torch.arange(B) + i) % 2 for i in range(3)]

    def make(mode):
        ops.set_seed_epoch(None)
        ops.set_dropout_seed(0x1234567)
        torch.manual_seed(0)
        enc = fMRITabularEncoder(37, 50, hidden_dim=64, dropout=0.1)
        return BridgeTrainer(eeg_channels=C, dropout=0.1, lr=1e-3, mode=mode, fmri_encoder=enc, classify=True, ce_weight=0.5,
                             **KEY).train()
    lg, lm, tg, tm = _graph_and_manual(make, lambda tr, i: tr.train_step(*feed[i], None, labels[i])["loss"].clone(), 3)
    assert torch.isfinite(lg).all() and torch.equal(lg, lm), (lg, lm)
    _training_state_equal(tg, tm)
    _bank_equal(tg, tm, False)
    assert tg._bank.state.tolist() == [3 * B % K, K, 3, 0] and set(tg._key) == {"eeg_encoder", "fmri_encoder", "bridge"}


def test_the_three_augmenters_compose(plain_batches):
    def make(mode):
        return _trainer(mode, dropout=0.1, augment=EEGTransforms(p=0.6, seed=11),
                        eeg_time_augment=EEGTimeTransforms(p_shift=0.7, max_shift=4, p_scale=0.5, p_mask=0.5, seed=3),
                        fmri_augment=VolumeTransforms(seed=5), **KEY)
    lg, lm, tg, tm = _graph_and_manual(make, lambda tr, i: tr.train_step(*plain_batches[i])["loss"].clone(), 3)
    assert torch.isfinite(lg).all() and torch.equal(lg, lm), (lg, lm)
    _training_state_equal(tg, tm)
    _bank_equal(tg, tm, False)
    assert tg.augment_step == 3 and tg.fmri_augment_step == 3
    # the keys saw the augmented batch: without the augmenters the first loss is another
    plain = _trainer("manual", dropout=0.1, **KEY)
    assert plain.train_step(*plain_batches[0])["loss"].item() != lm[0].item()


def test_the_packed_host_fed_path_composes(batches):
    def make(mode):
        return _trainer(mode, dropout=0.1, **KEY)

    def step(tr, i):
        e, f, g, _ = batches[i]
        if tr.mode == "graph" and i > 0:
            return tr.train_step_packed(tr.pack_host_batch(e, f, groups=g).cuda(non_blocking=True))["loss"].clone()
        return tr.train_step(e, f, g)["loss"].clone()
    lg, lm, tg, tm = _graph_and_manual(make, step, 4)
    assert torch.isfinite(lg).all() and torch.equal(lg, lm), (lg, lm)
    _training_state_equal(tg, tm)
    _bank_equal(tg, tm, True)
    assert tg._bank.state.tolist() == [4 * B % K, K, 4, 0]


def test_read_only_calls_run_no_key_pass_and_leave_the_bank_alone(batches, monkeypatch):
    tr = _trainer("graph", **KEY)
    _run(tr, batches, 2, True)
    before = [t.clone() for t in tr._bank.tensors()]
    e, f, g, y = batches[2]
    calls, real = [], _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    tr.evaluate(e, f, g)
    tr.evaluate_retrieval(e, f)
    tr.embed(e, f)
    monkeypatch.setattr(_hip, "call", real)
    torch.cuda.synchronize()
    assert "mm_clip_key_loss" not in calls and "mm_clip_bank_push" not in calls
    assert calls.count("mm_pooled_head_fwd") == 2 * 3        # one pass of each encoder per call: no key pass
    for x, y0 in zip(tr._bank.tensors(), before):
        assert torch.equal(x, y0)
    tr.reset_bank()
    assert tr.bank_filled == 0
