"""BridgeTrainer(lr_scale=, no_decay=, freeze=) at a small shape (8 channels x 256 samples, 16^3 volumes, 8 pairs, dropout 0).

Everything compared with `torch.equal` is exact by contract: the per-segment update kernel writes, for every segment, the
bits the plain kernel writes with that segment's learning rate and weight decay (tests/test_adamw_groups_kernels_gpu.py),
and the gradients of a step do not depend on the optimizer's table.  The one tolerance, 1e-5 on the loss and on the
gradients between the eager tape and the autograd surface, is the one the trainer tests use for that pair
(tests/test_fmri_tab_trainer_gpu.py, tests/test_clip_bank_trainer_gpu.py)."""
import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, bridge_branches, ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
from multimodal_eeg_fmri_amd.fmri_utils import fMRITabularEncoder

pytestmark = pytest.mark.gpu

B, C, T, VOL = 8, 8, 256, (16, 16, 16)
LR, WD = 1e-3, 0.05
COMPONENTS = BridgeTrainer.COMPONENTS
TABLE = dict(lr_scale={"eeg_encoder": 0.1, "fmri_encoder": 0.5, "head": 2.0}, no_decay=True, weight_decay=WD)


def f32(x):
    return torch.tensor(float(x), dtype=torch.float32).item()


@pytest.fixture(autouse=True)
def _no_seed_epoch():
    ops.set_seed_epoch(None)
    yield
    ops.set_seed_epoch(None)


def _trainer(mode="graph", seed=0, lr=LR, **kw):
    ops.set_seed_epoch(None)
    ops.set_dropout_seed(0x1234567)
    torch.manual_seed(seed)
    return BridgeTrainer(eeg_channels=C, dropout=0.0, lr=lr, mode=mode, **kw).train()


@pytest.fixture(scope="module")
def batches():
    return [synthetic_pairs(B, C, T, VOL, seed=700 + i) for i in range(3)]


def _run(tr, batches, steps, start=0, snaps=None):
    losses = []
    for i in range(start, start + steps):
        losses.append(tr.train_step(*batches[i % len(batches)])["loss"].clone())
        if snaps is not None:
            snaps.append(tr.bucket.p.clone())
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


def _component_mask(tr, name):
    mask = torch.zeros(tr.bucket.n, dtype=torch.bool)
    off = 0
    for p, c in zip(tr.bucket.params, tr._param_component):
        mask[off:off + p.numel()] = c == name
        off += p.numel()
    return mask.cuda()


def _ndim_mask(tr):
    """True at the elements of the parameters with ndim <= 1"""
    mask = torch.zeros(tr.bucket.n, dtype=torch.bool)
    off = 0
    for p in tr.bucket.params:
        mask[off:off + p.numel()] = p.ndim <= 1
        off += p.numel()
    return mask.cuda()


def _frozen_tensors(tr, names):
    return [t.detach().clone() for c in names for t in list(getattr(tr, c).parameters()) + list(getattr(tr, c).buffers())]


@pytest.fixture(scope="module")
def default_run(batches):
    """the default trainer in graph mode over 4 steps, with the parameters after every step"""
    tr = _trainer("graph")
    p0 = tr.bucket.p.clone()
    snaps = []
    losses = _run(tr, batches, 4, snaps=snaps)
    return {"tr": tr, "p0": p0, "losses": losses, "snaps": snaps, "state": _state(tr)}


# (a) --------------------------------------------------------------------------------------------------------------------
def test_multipliers_of_one_are_the_default_trainer(batches, default_run):
    calls = []
    real = _hip.call
    tr = _trainer("graph", lr_scale={c: 1.0 for c in COMPONENTS})
    _hip.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        losses = _run(tr, batches, 4)
    finally:
        _hip.call = real
    assert torch.isfinite(losses).all() and torch.equal(losses, default_run["losses"])
    _assert_state_equal(_state(tr), default_run["state"])
    assert "mm_adamw_clip" in calls and "mm_adamw_clip_groups" not in calls   # a uniform table launches the plain kernel
    assert tr.groups == default_run["tr"].groups and "param_groups" not in tr.checkpoint_state()["bridge_trainer_state"]


# (b) --------------------------------------------------------------------------------------------------------------------
def test_one_multiplier_everywhere_is_the_default_trainer_at_the_product_rate(batches):
    scaled = _trainer("graph", lr_scale={c: 0.1 for c in COMPONENTS})
    plain = _trainer("graph", lr=(torch.tensor(LR, dtype=torch.float32) * torch.tensor(0.1, dtype=torch.float32)).item())
    assert scaled._grouped and not plain._grouped
    a, b = _run(scaled, batches, 4), _run(plain, batches, 4)
    assert torch.equal(a, b)
    sa, sb = _state(scaled), _state(plain)
    assert sa["words"][2].item() == f32(LR) and sb["words"][2].item() == f32(f32(LR) * f32(0.1))
    sa["words"][2] = sb["words"][2]                                           # (the learning-rate word is the base rate)
    _assert_state_equal(sa, sb)


# (c) --------------------------------------------------------------------------------------------------------------------
def test_a_multiplier_of_zero_holds_one_component_and_nothing_else(batches, default_run):
    tr = _trainer("graph", lr_scale={"fmri_encoder": 0.0})
    held = _component_mask(tr, "fmri_encoder")
    assert 0 < int(held.sum()) < tr.bucket.n and torch.equal(tr.bucket.p, default_run["p0"])
    bufs0 = [t.clone() for t in tr.fmri_encoder.buffers()]
    snaps = []
    _run(tr, batches, 3, snaps=snaps)
    assert torch.equal(tr.bucket.p[held], default_run["p0"][held])            # bit-equal to its initial values
    assert any(not torch.equal(a, b) for a, b in zip(bufs0, tr.fmri_encoder.buffers()))     # BatchNorm statistics moved
    assert not torch.equal(tr.bucket.m[held], torch.zeros_like(tr.bucket.m[held]))          # ... and the Adam moments
    # step 1: the same gradients, the same clip - every other parameter is the default trainer's to the bit
    assert torch.equal(snaps[0][~held], default_run["snaps"][0][~held])
    assert not torch.equal(default_run["snaps"][0][held], default_run["p0"][held])


# (d) --------------------------------------------------------------------------------------------------------------------
def test_no_decay_takes_the_decay_off_vectors_and_scalars_only(batches):
    nd = _trainer("manual", no_decay=True, weight_decay=WD)
    with_wd, without = _trainer("manual", weight_decay=WD), _trainer("manual", weight_decay=0.0)
    for tr in (nd, with_wd, without):
        _run(tr, batches, 1)
    small = _ndim_mask(nd)
    assert 0 < int(small.sum()) < nd.bucket.n
    assert torch.equal(nd.bucket.p[small], without.bucket.p[small])
    assert torch.equal(nd.bucket.p[~small], with_wd.bucket.p[~small])
    assert not torch.equal(with_wd.bucket.p[small], without.bucket.p[small])   # (the decay does show at this size)
    assert torch.equal(nd.bucket.m, with_wd.bucket.m) and torch.equal(nd.bucket.v, with_wd.bucket.v)


# (e) --------------------------------------------------------------------------------------------------------------------
def test_graph_and_manual_mode_are_bit_equal_and_autograd_agrees(batches):
    tg, tm = _trainer("graph", **TABLE), _trainer("manual", **TABLE)
    lg, lm = _run(tg, batches, 3), _run(tm, batches, 3)
    assert tg.capture_mode == "one graph" and torch.isfinite(lg).all()
    assert torch.equal(lg, lm)
    _assert_state_equal(_state(tg), _state(tm))
    # the autograd surface: step 1's loss at 1e-5 (the same weights), the steps behind the per-segment update at the
    # tolerance of tests/test_trainer_gpu.py::test_trainer_modes_agree_on_first_steps
    la = _run(_trainer("autograd", **TABLE), batches, 3)
    print(f"ERR param groups autograd vs manual losses {[abs(a - b) for a, b in zip(la.tolist(), lm.tolist())]}")
    assert abs(la[0].item() - lm[0].item()) <= 1e-5
    for a, b in zip(la.tolist(), lm.tolist()):
        assert abs(a - b) <= 2e-2 * max(1.0, abs(a)), (la, lm)


# (f) --------------------------------------------------------------------------------------------------------------------
def test_set_lr_scale_keeps_the_captured_graph_and_changes_one_component(batches):
    tr, twin = _trainer("graph", lr_scale={"eeg_encoder": 0.5}), _trainer("graph", lr_scale={"eeg_encoder": 0.5})
    _run(tr, batches, 2)
    _run(twin, batches, 2)
    graph = tr._cap["graphs"][0]
    before = tr.bucket.p.clone()
    assert torch.equal(before, twin.bucket.p)
    tr.set_lr_scale("fmri_encoder", 0.0)
    assert tr.lr_scales == {"eeg_encoder": 0.5, "fmri_encoder": 0.0, "head": 1.0}
    _run(tr, batches, 1, start=2)
    _run(twin, batches, 1, start=2)
    assert len(tr._cap["graphs"]) == 1 and tr._cap["graphs"][0] is graph       # no new capture
    held = _component_mask(tr, "fmri_encoder")
    assert torch.equal(tr.bucket.p[held], before[held]) and not torch.equal(twin.bucket.p[held], before[held])
    assert torch.equal(tr.bucket.p[~held], twin.bucket.p[~held])               # that component only
    assert torch.equal(tr.bucket.m, twin.bucket.m) and torch.equal(tr.bucket.v, twin.bucket.v)
    tr.set_lr_scale("fmri_encoder", 1.0)                                       # released: it moves again, same graph
    mid = tr.bucket.p.clone()
    _run(tr, batches, 1)
    assert tr._cap["graphs"][0] is graph and not torch.equal(tr.bucket.p[held], mid[held])


# (g) --------------------------------------------------------------------------------------------------------------------
BACKWARDS = {"eeg_encoder": ("erp_encoder_bwd",), "fmri_encoder": ("volume_encoder_bwd", "fmri_tab_bwd")}


def _launches(tr, batch, monkeypatch):
    """-> (names of the launches of one manual step, {encoder: the names launched inside its backward function})"""
    names, inside, depth = [], {c: [] for c in BACKWARDS}, {c: 0 for c in BACKWARDS}
    real_call = _hip.call

    def call(entry, *a):
        names.append((entry, tuple(c for c in BACKWARDS if depth[c])))
        for c in BACKWARDS:
            if depth[c]:
                inside[c].append(entry)
        return real_call(entry, *a)

    def wrap(c, fn):
        def run(*a, **kw):
            depth[c] += 1
            try:
                return fn(*a, **kw)
            finally:
                depth[c] -= 1
        return run
    monkeypatch.setattr(_hip, "call", call)
    for c, fns in BACKWARDS.items():
        for fn in fns:
            monkeypatch.setattr(bridge_branches, fn, wrap(c, getattr(bridge_branches, fn)))
    try:
        tr.train_step(*batch)
        torch.cuda.synchronize()
    finally:
        monkeypatch.undo()
    return names, inside


def _names(launches):
    return [entry for entry, _ in launches]


@pytest.fixture(scope="module")
def default_launches(batches):
    mp = pytest.MonkeyPatch()
    tr = _trainer("manual")
    tr.train_step(*batches[0])                                                # (the first step also records the weight list)
    launches, inside = _launches(tr, batches[1], mp)
    # an encoder's own backward kernels: launched inside its backward function and nowhere else in the step
    own = {c: set(inside[c]) - {entry for entry, where in launches if c not in where} for c in BACKWARDS}
    assert all(own.values()), own
    return _names(launches), own


def _grads_of_step_one(mode, batches, **kw):
    tr = _trainer(mode, **kw)
    tr.grad_clip = 0.0
    probe = {}
    real = tr._seg_adamw
    tr._seg_adamw = lambda: (probe.setdefault("g", tr.bucket.g.clone()), real())[1]   # the gradients, before AdamW clears them
    loss = tr.train_step(*batches[0])["loss"].item()
    torch.cuda.synchronize()
    return tr, loss, probe["g"]


@pytest.mark.parametrize("freeze", [("fmri_encoder",), ("eeg_encoder",), ("eeg_encoder", "fmri_encoder")],
                         ids=["fmri", "eeg", "both"])
def test_a_frozen_encoder_is_untouched_and_its_backward_is_not_launched(batches, default_launches, freeze, monkeypatch):
    _, own = default_launches
    finals = {}
    for mode in ("manual", "graph", "autograd"):
        tr = _trainer(mode, freeze=freeze)
        assert tr.bucket.n == sum(p.numel() for p in tr.parameters() if p.requires_grad)
        frozen0 = _frozen_tensors(tr, freeze)
        if mode == "manual":
            tr.train_step(*batches[0])
            launches, inside = _launches(tr, batches[1], monkeypatch)
            names = _names(launches)
            tr.train_step(*batches[2])
            torch.cuda.synchronize()
            for c in freeze:
                assert not inside[c] and not own[c] & set(names), (c, sorted(own[c] & set(names)))
            for c in set(BACKWARDS) - set(freeze):
                assert inside[c] and own[c] <= set(names)
            assert names.count("mm_sumsq") == 1 and names.count("mm_adamw_clip") == 1 and "mm_adamw_clip_groups" not in names
        else:
            losses = _run(tr, batches, 3)
            assert torch.isfinite(losses).all()
        assert all(torch.equal(a, b) for a, b in zip(frozen0, _frozen_tensors(tr, freeze))), mode
        assert all(not getattr(tr, c).training for c in freeze) and tr.head.training
        finals[mode] = tr.bucket.p.clone()
    assert torch.equal(finals["manual"], finals["graph"])
    # step 1: the remaining parameters' gradients on the eager tape and on the autograd surface
    tm, lm, gm = _grads_of_step_one("manual", batches, freeze=freeze)
    ta, la, ga = _grads_of_step_one("autograd", batches, freeze=freeze)
    diff = (gm - ga).abs().max().item()
    print(f"ERR freeze {freeze} manual vs autograd loss {abs(lm - la):.3e} gradients {diff:.3e} of {gm.abs().max().item():.3e}")
    assert gm.abs().max().item() > 0 and gm.numel() == tm.bucket.n
    assert abs(lm - la) <= 1e-5 and diff <= 1e-5


def test_a_frozen_tabular_encoder(batches, monkeypatch):
    from multimodal_eeg_fmri_amd.bridge_trainer import synthetic_tabular_pairs
    A, CF = 12, 20
    data = [synthetic_tabular_pairs(B, C, T, A, CF, seed=820 + i) for i in range(2)]

    def make(mode):
        ops.set_seed_epoch(None)
        ops.set_dropout_seed(0x1234567)
        torch.manual_seed(0)
        enc = fMRITabularEncoder(A, CF, hidden_dim=64, dropout=0.0)
        return BridgeTrainer(eeg_channels=C, dropout=0.0, lr=LR, mode=mode, fmri_encoder=enc, freeze=("fmri_encoder",)).train()
    finals = {}
    for mode in ("manual", "graph"):
        tr = make(mode)
        frozen0 = _frozen_tensors(tr, ("fmri_encoder",))
        if mode == "manual":
            tr.train_step(*data[0])
            launches, inside = _launches(tr, data[1], monkeypatch)
            names = _names(launches)
            assert "mm_fmri_tab_bwd" not in names and "mm_fmri_tab_fwd" in names and not inside["fmri_encoder"]
        else:
            _run(tr, data, 2)
        assert all(torch.equal(a, b) for a, b in zip(frozen0, _frozen_tensors(tr, ("fmri_encoder",))))
        finals[mode] = tr.bucket.p.clone()
    assert torch.equal(finals["manual"], finals["graph"])


# (h) --------------------------------------------------------------------------------------------------------------------
def test_checkpoint_resume_is_exact_with_a_table_and_a_frozen_encoder(tmp_path, batches):
    kw = dict(lr_scale={"eeg_encoder": 0.1, "head": 2.0}, no_decay=True, weight_decay=WD, freeze=("fmri_encoder",))
    a = _trainer("graph", **kw)
    _run(a, batches, 2)
    a.set_lr_scale("eeg_encoder", 0.25)                                       # the multipliers travel as they are NOW
    path = str(tmp_path / "ck.pt")
    a.save_checkpoint(path, epoch=1)
    pg = torch.load(path, map_location="cpu", weights_only=True)["bridge_trainer_state"]["param_groups"]
    assert pg["multipliers"] == [0.25, 1.0, 2.0] and pg["no_decay"] is True and pg["freeze"] == ["fmri_encoder"]
    assert pg["seg_end"] == a._table.ends and pg["seg_wd"] == a._table.wds and 0.0 in pg["seg_wd"] and WD in pg["seg_wd"]
    want = _run(a, batches, 3, start=2)
    b = _trainer("graph", seed=11, **dict(kw, lr_scale=None))
    b.load_checkpoint(path)
    assert b.lr_scales == a.lr_scales and torch.equal(b._table.mult, a._table.mult) and torch.equal(b._table.wd, a._table.wd)
    got = _run(b, batches, 3, start=2)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    _assert_state_equal(_state(b), _state(a))


def test_checkpoints_of_another_freeze_or_no_decay_are_refused_untouched(batches):
    src = _trainer("manual", no_decay=True, freeze=("fmri_encoder",))
    _run(src, batches, 1)
    ck = src.checkpoint_state()
    cases = [(_trainer("manual", seed=3, no_decay=True), "freeze differs"),
             (_trainer("manual", seed=3, freeze=("fmri_encoder",)), "no_decay differs"),
             (_trainer("manual", seed=3, no_decay=True, freeze=("eeg_encoder",)), "freeze differs"),
             (_trainer("manual", seed=3), "no_decay differs")]
    for tr, msg in cases:
        _run(tr, batches, 1)
        before, scales, mults = _state(tr), tr.lr_scales, tr._table.mult.clone()
        with pytest.raises(ValueError, match=msg):
            tr.load_checkpoint_state(ck)
        _assert_state_equal(before, _state(tr))
        assert tr.lr_scales == scales and torch.equal(tr._table.mult, mults)


# (i) --------------------------------------------------------------------------------------------------------------------
def test_fit_moves_the_base_rate_only(batches):
    tr = _trainer("graph", **TABLE)
    mult0 = tr._table.mult.clone()
    val = synthetic_pairs(16, C, T, VOL, seed=77)
    hist = tr.fit([batches[0], batches[1]], 2, val=val, warmup_epochs=0, patience=10)
    assert len(hist) == 2 and all(h["val"] is not None and h["steps"] == 2 for h in hist)
    assert tr.lr_scales == TABLE["lr_scale"] and torch.equal(tr._table.mult, mult0)
    assert tr.lr != LR and tr.bucket.state[2].item() == f32(tr.lr)             # the schedule did move the base rate
    assert tr.bucket.state[0].item() == 4.0
