"""BridgeTrainer(ema_decay=) at a small shape (8 channels x 256 samples, 16^3 volumes, 8 pairs, dropout 0): the average
costs the step nothing it can see - losses, parameters, Adam moments and optimizer words are a default trainer's to the
bit -, follows the fp64 recursion over the step's own parameters, is the same bits in graph and manual mode, can be
evaluated with (`ema_weights`) and exported (`ema_state_dict`) without disturbing training, travels through checkpoints
bit for bit, and drives `fit`'s validation.

The bound on the shadow after t steps is the kernel test's (tests/test_adamw_ema_kernels_gpu.py):
8 * 2^-24 * M * min(t, 1 / (1 - d)), M the largest |p| or |ema| met so far, d = 0.9 without the warm-up of the decay."""
import pytest
import torch

from multimodal_eeg_fmri_amd import ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
from test_ema_host import ema_decay_schedule, ema_reference

pytestmark = pytest.mark.gpu

B, C, T, VOL = 8, 8, 256, (16, 16, 16)
U = 2.0 ** -24
D = torch.tensor(0.9, dtype=torch.float32).item()


@pytest.fixture(autouse=True)
def _no_seed_epoch():
    ops.set_seed_epoch(None)
    yield
    ops.set_seed_epoch(None)


def _trainer(mode="graph", seed=0, **kw):
    ops.set_seed_epoch(None)
    ops.set_dropout_seed(0x1234567)
    torch.manual_seed(seed)
    return BridgeTrainer(eeg_channels=C, dropout=0.0, lr=1e-3, mode=mode, **kw).train()


@pytest.fixture(scope="module")
def batches():
    return [synthetic_pairs(B, C, T, VOL, seed=700 + i) for i in range(3)]


@pytest.fixture(scope="module")
def val():
    return synthetic_pairs(16, C, T, VOL, seed=77)


def _run(tr, batches, steps, start=0, snapshots=None):
    losses = []
    for i in range(start, start + steps):
        losses.append(tr.train_step(*batches[i % len(batches)])["loss"].clone())
        if snapshots is not None:
            snapshots.append((tr.bucket.p.cpu(), tr.bucket.state[:8].cpu()))
    torch.cuda.synchronize()
    return torch.stack(losses)


def _state(tr):
    b = tr.bucket
    return {"p": b.p.clone(), "m": b.m.clone(), "v": b.v.clone(), "words": b.state[:5].clone(),
            "buffers": [t.clone() for t in tr.buffers()]}


def _assert_state_equal(a, b):
    for k in ("p", "m", "v", "words"):
        assert torch.equal(a[k], b[k]), k
    assert len(a["buffers"]) == len(b["buffers"]) and all(torch.equal(x, y) for x, y in zip(a["buffers"], b["buffers"]))


@pytest.fixture(scope="module")
def graph_run(batches):
    """the averaging trainer in graph mode over 6 steps (3 batches, twice), with the parameters after every step.
    No warm-up of the decay: at d = 0.9 the shadow remembers its start for the whole run (0.9^6 = 0.53), so a shadow
    that the capture's own warm-up steps had moved would miss the recursion by far more than the bound."""
    tr = _trainer("graph", ema_decay=0.9, ema_warmup=False)
    shadow0 = tr.bucket.ema.cpu()
    snaps = []
    losses = _run(tr, batches, 6, snapshots=snaps)
    return {"tr": tr, "losses": losses, "snaps": snaps, "shadow0": shadow0, "state": _state(tr), "ema": tr.bucket.ema.clone()}


def test_the_step_of_an_averaging_trainer_is_the_default_trainers_to_the_bit(batches, graph_run):
    plain = _trainer("graph")
    losses = _run(plain, batches, 6)
    assert torch.isfinite(losses).all() and torch.equal(losses, graph_run["losses"])
    _assert_state_equal(_state(plain), graph_run["state"])
    assert plain.bucket.ema is None and torch.isfinite(graph_run["tr"].bucket.state[5]).item()
    assert plain.bucket.state[5].item() == 0.0                            # never written by mm_adamw_clip
    assert "ema" not in plain.checkpoint_state()["bridge_trainer_state"]
    assert set(graph_run["tr"].checkpoint_state()["bridge_trainer_state"]["ema"]) == {"decay", "warmup", "shadow"}


def test_shadow_follows_the_fp64_recursion_over_the_steps_own_parameters(graph_run):
    ref = graph_run["shadow0"].double()
    M = ref.abs().max().item()
    for t, (p, words) in enumerate(graph_run["snaps"], start=1):
        d = words[5].double().item()
        assert words[0].item() == t and d == ema_decay_schedule(t - 1, D, False) == D
        ref = ema_reference(ref, p, d)
        M = max(M, p.abs().max().item(), ref.abs().max().item())
    err = (graph_run["ema"].cpu().double() - ref).abs().max().item()
    bound = 8 * U * M * min(6, 1.0 / (1.0 - D))
    print(f"ERR ema trainer 6 steps err {err:.3e} bound {bound:.3e} M {M:.3f}")
    assert err <= bound
    assert not torch.equal(graph_run["ema"], graph_run["state"]["p"])


def test_graph_and_manual_mode_keep_the_same_shadow(batches, graph_run):
    man = _trainer("manual", ema_decay=0.9, ema_warmup=False)
    losses = _run(man, batches, 6)
    assert torch.equal(losses, graph_run["losses"])
    assert torch.equal(man.bucket.ema, graph_run["ema"]) and torch.equal(man.bucket.p, graph_run["state"]["p"])


def test_autograd_mode_keeps_an_average_too(batches):
    tr = _trainer("autograd", ema_decay=0.9, ema_warmup=False)
    shadow0 = tr.bucket.ema.cpu()
    _run(tr, batches, 1)
    d = tr.bucket.state[5].item()
    assert d == D
    ref = ema_reference(shadow0, tr.bucket.p.cpu(), d)
    bound = 8 * U * torch.maximum(tr.bucket.p.cpu().abs(), shadow0.abs()).double()
    assert bool(((tr.bucket.ema.cpu().double() - ref).abs() <= bound).all())


def test_ema_weights_evaluates_with_the_average_and_leaves_training_alone(batches, val):
    tr = _trainer("graph", ema_decay=0.9)
    twin = _trainer("graph", ema_decay=0.9)
    _run(tr, batches, 3)
    _run(twin, batches, 3)
    live, shadow = tr.bucket.p.clone(), tr.bucket.ema.clone()
    live_embed = tr.embed(val[0], val[1])
    with tr.ema_weights():
        assert torch.equal(tr.bucket.p, shadow) and torch.equal(tr.bucket.ema, live)
        ze, zf = tr.embed(val[0], val[1])
        with pytest.raises(RuntimeError, match="ema_weights"):
            tr.train_step(*batches[0])
        with pytest.raises(RuntimeError, match="ema_weights"):
            tr.checkpoint_state()
    assert torch.equal(tr.bucket.p, live) and torch.equal(tr.bucket.ema, shadow)
    assert not torch.equal(ze, live_embed[0])
    # a fresh default trainer that loads the exported average (and the live buffers it comes with) embeds the same bits
    sd = tr.ema_state_dict()
    assert all(not v.is_cuda for v in sd.values()) and set(sd) == set(tr.state_dict())
    for k, b_live in tr.named_buffers():
        assert k not in sd or torch.equal(b_live.cpu(), sd[k]), k
    fresh = _trainer("graph", seed=5)
    fresh.load_state_dict(sd)
    ops.weights_changed()
    fe, ff = fresh.embed(val[0], val[1])
    assert torch.equal(fe, ze) and torch.equal(ff, zf)
    # the model state dict outside the context holds the live weights
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in tr.bucket.params]), live)
    # and the next three steps are those of a twin that was never disturbed
    a, b = _run(tr, batches, 3, start=3), _run(twin, batches, 3, start=3)
    assert torch.equal(a, b)
    _assert_state_equal(_state(tr), _state(twin))
    assert torch.equal(tr.bucket.ema, twin.bucket.ema)
    tr.sync_ema()
    assert torch.equal(tr.bucket.ema, tr.bucket.p)


def test_checkpoint_resume_is_exact_including_the_average(tmp_path, batches):
    """with the warm-up of the decay (the default): the decay of steps 4..6 comes from the restored step counter"""
    a = _trainer("graph", ema_decay=0.9)
    _run(a, batches, 3)
    path = str(tmp_path / "ck.pt")
    a.save_checkpoint(path, epoch=1)
    saved_shadow = a.bucket.ema.clone()
    ck = torch.load(path, map_location="cpu", weights_only=True)
    ema = ck["bridge_trainer_state"]["ema"]
    assert ema["decay"] == 0.9 and ema["warmup"] is True and torch.equal(ema["shadow"], a.bucket.ema.cpu())
    assert ema["shadow"].dtype == torch.float32 and tuple(ema["shadow"].shape) == (a.bucket.n,)
    msd = ck["model_state_dict"]                                      # always the live weights
    names = {id(p): n for n, p in a.named_parameters()}
    assert torch.equal(torch.cat([msd[names[id(q)]].reshape(-1) for q in a.bucket.params]), a.bucket.p.cpu())
    want_losses = _run(a, batches, 3, start=3)                        # the uninterrupted run
    b = _trainer("graph", seed=11, ema_decay=0.9)
    ptr = b.bucket.ema.data_ptr()
    b.load_checkpoint(path)
    assert b.bucket.ema.data_ptr() == ptr and torch.equal(b.bucket.ema, saved_shadow)
    losses = _run(b, batches, 3, start=3)
    assert torch.isfinite(losses).all() and torch.equal(losses, want_losses)
    _assert_state_equal(_state(b), _state(a))
    assert torch.equal(b.bucket.ema, a.bucket.ema) and not torch.equal(a.bucket.ema, saved_shadow)
    assert b.bucket.state[5].item() == a.bucket.state[5].item() < D    # step 6: 7 / 16


def test_checkpoints_of_another_averaging_setup_are_refused_untouched(batches):
    with_ema = _trainer("manual", ema_decay=0.9)
    without = _trainer("manual", seed=3)
    _run(with_ema, batches, 1)
    _run(without, batches, 1)
    ck_with, ck_without = with_ema.checkpoint_state(), without.checkpoint_state()
    cases = [(without, ck_with, "ema differs"), (with_ema, ck_without, "ema differs"),
             (_trainer("manual", seed=4, ema_decay=0.99), ck_with, "ema.decay differs"),
             (_trainer("manual", seed=4, ema_decay=0.9, ema_warmup=False), ck_with, "ema.warmup differs")]
    for tr, ck, msg in cases:
        before = _state(tr)
        shadow = None if tr.bucket.ema is None else tr.bucket.ema.clone()
        with pytest.raises(ValueError, match=msg):
            tr.load_checkpoint_state(ck)
        _assert_state_equal(before, _state(tr))
        assert shadow is None or torch.equal(shadow, tr.bucket.ema)


def _fit(tr, batches, val, **kw):
    train = [batches[0], batches[1]]
    return tr.fit(train, 3, val=val, warmup_epochs=0, patience=10, **kw)


def test_fit_validates_with_the_average_by_default(batches, val):
    tr = _trainer("graph", ema_decay=0.9)
    hist = _fit(tr, batches, val)
    assert len(hist) == 3 and all(h["val"] is not None for h in hist)
    best = [h for h in hist if h["improved"]][-1]                       # the state `fit` restored (the last epoch's, if that
    with tr.ema_weights():                                              # was the best: then nothing was restored)
        got = tr.evaluate_retrieval(val[0], val[1])
    assert got == best["val"]
    if best is hist[-1]:
        assert got == hist[-1]["val"]
    live = tr.evaluate_retrieval(val[0], val[1])
    ze_l, _ = tr.embed(val[0], val[1])
    with tr.ema_weights():
        ze_a, _ = tr.embed(val[0], val[1])
    assert not torch.equal(ze_l, ze_a)                                  # (the two sets of weights do differ)
    assert set(live) == set(got)


def test_fit_validate_with_live_is_a_default_trainers_fit(batches, val):
    a = _trainer("graph", ema_decay=0.9)
    ha = _fit(a, batches, val, validate_with="live")
    b = _trainer("graph")
    hb = _fit(b, batches, val)
    assert ha == hb
    with pytest.raises(ValueError, match="validate_with"):
        _fit(b, batches, val, validate_with="ema")
