"""BridgeTrainer checkpoint / resume and `fit` on the MI355X: a resumed run continues bit for bit - losses, every
parameter, the Adam moments, the optimizer words and the BatchNorm buffers equal the uninterrupted run's - in graph and
manual mode, into a fresh or an already-captured trainer, whatever drew dropout seeds before the load."""
import os

import pytest
import torch

from multimodal_eeg_fmri_amd import ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs

pytestmark = pytest.mark.gpu

SMALL = (8, 16, 256, (16, 16, 16))
C2 = (32, 64, 1024, (32, 32, 32))


@pytest.fixture(autouse=True)
def _no_seed_epoch():
    ops.set_seed_epoch(None)
    yield
    ops.set_seed_epoch(None)


def _batches(shape, n=3, seed=300):
    B, C, T, vol = shape
    return [synthetic_pairs(B, C, T, vol, seed=seed + i) for i in range(n)]


def _make(shape, mode, seed, dropout=0.3, lr=1e-3):
    torch.manual_seed(seed)
    return BridgeTrainer(eeg_channels=shape[1], dropout=dropout, lr=lr, mode=mode).train()


def _steps(tr, batches, i0, k):
    out = [tr.train_step(*batches[i % len(batches)])["loss"].clone() for i in range(i0, i0 + k)]
    torch.cuda.synchronize()
    return torch.stack(out)


def _snap(tr):
    b = tr.bucket
    return [t.detach().clone() for t in (b.p, b.m, b.v, b.state)] + [v.detach().clone() for v in tr.state_dict().values()]


def _assert_same(ref, got):
    assert len(ref) == len(got)
    for i, (a, b) in enumerate(zip(ref, got)):
        assert torch.equal(a, b), (i, (a.double() - b.double()).abs().max().item())


def _unrelated_seeds(n=5):
    for _ in range(n):
        ops._next_seed()


def _resume_case(tmp_path, shape, save_mode, load_mode, dropout=0.3, warm_target=False):
    ops.set_dropout_seed(2024)
    batches = _batches(shape)
    a = _make(shape, save_mode, 0, dropout)
    _steps(a, batches, 0, 5)
    path = str(tmp_path / "ck.pt")
    a.save_checkpoint(path, epoch=1)
    want_losses = _steps(a, batches, 5, 5)
    want = _snap(a)
    b = _make(shape, load_mode, 11, dropout)
    if warm_target:                                   # a trainer that has already captured (and run) its own step
        _steps(b, _batches(shape, seed=900), 0, 3)
    ops.set_dropout_seed(77)
    _unrelated_seeds()
    b.load_checkpoint(path)
    got_losses = _steps(b, batches, 5, 5)
    assert torch.isfinite(want_losses).all()
    assert torch.equal(want_losses, got_losses), (want_losses, got_losses)
    _assert_same(want, _snap(b))
    return a, b


@pytest.mark.parametrize("shape", [SMALL, C2], ids=["small", "c2"])
def test_graph_mode_resume_is_exact(tmp_path, shape):
    a, b = _resume_case(tmp_path, shape, "graph", "graph")
    assert b.capture_mode == a.capture_mode == "one graph"


def test_manual_mode_resume_is_exact(tmp_path):
    _resume_case(tmp_path, SMALL, "manual", "manual")


def test_resume_into_a_trainer_that_has_already_captured(tmp_path):
    _resume_case(tmp_path, SMALL, "graph", "graph", warm_target=True)


def test_graph_checkpoint_resumed_in_manual_mode_at_dropout_0(tmp_path):
    """the one-graph step and the eager tape run the same kernels in the same order: at dropout 0 a graph-mode
    checkpoint continues in manual mode on the same bits"""
    _resume_case(tmp_path, SMALL, "graph", "manual", dropout=0.0)


def _fit_train(shape):
    batches = _batches(shape)
    return lambda epoch: batches[epoch % 3:] + batches[:epoch % 3]         # a reproducible per-epoch order


def _ck_equal(p, q):
    a = torch.load(p, map_location="cpu", weights_only=True)
    b = torch.load(q, map_location="cpu", weights_only=True)
    assert a["epoch"] == b["epoch"] and a["metrics"] == b["metrics"]
    _assert_same(list(a["model_state_dict"].values()), list(b["model_state_dict"].values()))
    for i, st in a["optimizer_state_dict"]["state"].items():
        _assert_same(list(st.values()), list(b["optimizer_state_dict"]["state"][i].values()))
    assert a["bridge_trainer_state"]["fit"] == b["bridge_trainer_state"]["fit"]


def test_fit_interrupted_and_resumed_equals_uninterrupted(tmp_path):
    E, E1 = 6, 3
    val = synthetic_pairs(32, 16, 256, (16, 16, 16), seed=77)
    train = _fit_train(SMALL)
    kw = dict(val=val, warmup_epochs=2, patience=10)

    ops.set_dropout_seed(5)
    a = _make(SMALL, "graph", 0)
    hist = a.fit(train, E, checkpoint_dir=str(tmp_path / "a"), **kw)
    want = _snap(a)
    assert [h["epoch"] for h in hist] == list(range(1, E + 1))
    assert all(h["val"] is not None for h in hist) and hist[0]["improved"]

    def dies_after(e):
        if e > E1:
            raise KeyboardInterrupt
        return train(e)
    ops.set_seed_epoch(None)
    ops.set_dropout_seed(5)
    b = _make(SMALL, "graph", 0)
    with pytest.raises(KeyboardInterrupt):
        b.fit(dies_after, E, checkpoint_dir=str(tmp_path / "b"), **kw)
    ops.set_seed_epoch(None)
    c = _make(SMALL, "graph", 12)
    ops.set_dropout_seed(999)
    _unrelated_seeds()
    got = c.fit(train, E, checkpoint_dir=str(tmp_path / "b"), resume=True, **kw)
    assert got == hist
    _assert_same(want, _snap(c))
    _ck_equal(str(tmp_path / "a" / "best.pt"), str(tmp_path / "b" / "best.pt"))
    _ck_equal(str(tmp_path / "a" / "last.pt"), str(tmp_path / "b" / "last.pt"))
    # the restored model is the best epoch's
    best = torch.load(str(tmp_path / "a" / "best.pt"), map_location="cpu", weights_only=True)
    assert best["epoch"] == max((h for h in hist if h["improved"]), key=lambda h: h["epoch"])["epoch"]
    for k, v in a.state_dict().items():
        assert torch.equal(v.cpu(), best["model_state_dict"][k]), k


def test_fit_stops_at_a_plateau_and_restores_the_best_epoch(tmp_path):
    scores = iter([0.1, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5])
    val = synthetic_pairs(16, 16, 256, (16, 16, 16), seed=78)
    ops.set_dropout_seed(6)
    tr = _make(SMALL, "graph", 0)
    hist = tr.fit(_fit_train(SMALL), 10, val=val, warmup_epochs=1, patience=2, monitor=lambda m: next(scores),
                  checkpoint_dir=str(tmp_path))
    assert [h["monitor"] for h in hist] == [0.1, 0.5, 0.5, 0.5]
    assert [h["improved"] for h in hist] == [True, True, False, False] and hist[-1]["stop"]
    best = torch.load(str(tmp_path / "best.pt"), map_location="cpu", weights_only=True)
    last = torch.load(str(tmp_path / "last.pt"), map_location="cpu", weights_only=True)
    assert best["epoch"] == 2 and last["epoch"] == 4
    sd = tr.state_dict()
    for k, v in sd.items():
        assert torch.equal(v.cpu(), best["model_state_dict"][k]), k
    assert any(not torch.equal(best["model_state_dict"][k], last["model_state_dict"][k]) for k in sd)
    # only the model is restored: the moments are the last epoch's
    assert torch.equal(tr.bucket.m.cpu(), torch.cat([last["optimizer_state_dict"]["state"][i]["exp_avg"].reshape(-1)
                                                     for i, *_ in sorted(tr.optimizer_param_map(), key=lambda e: e[3].start)]))


def test_validation_leaves_the_training_trajectory_unchanged():
    """evaluation draws no dropout seeds and touches nothing the step reads: fit with val (no checkpoint_dir) trains on
    the same bits as the same loop without val (the optimizer state is not part of the best-state restore)"""
    val = synthetic_pairs(32, 16, 256, (16, 16, 16), seed=79)
    runs = []
    for v in (val, None):
        ops.set_seed_epoch(None)
        ops.set_dropout_seed(7)
        tr = _make(SMALL, "graph", 0)
        hist = tr.fit(_fit_train(SMALL), 5, val=v, warmup_epochs=2)
        b = tr.bucket
        runs.append(([(h["lr"], h["train_loss"], h["steps"]) for h in hist], [t.clone() for t in (b.m, b.v, b.state)]))
    assert runs[0][0] == runs[1][0]
    _assert_same(runs[0][1], runs[1][1])


def test_data_parallel_checkpoint_and_fit_on_two_ranks():
    from tools import checkpoint_rehearsal
    r0, r1 = checkpoint_rehearsal.run(2)
    for r in (r0, r1):
        assert r["losses_equal"] and r["state_equal"], r
        assert r["same_params_across_ranks"] and r["fit_same_params_across_ranks"], r
        assert r["capture_mode"] == "3 segments + 2 eager collectives", r
        assert r["best_epoch"] == 2 and r["restored_is_best"], r
    assert r0["stop_epoch"] == r1["stop_epoch"] == 4, (r0, r1)
    assert r0["history_monitor"] == r1["history_monitor"] == [0.1, 0.5, 0.5, 0.5]
