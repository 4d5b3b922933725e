"""Host side of the cross-batch negative bank: the header declares the entry points, every rule of
`BridgeTrainer(bank_size=, bank_warmup=)` raises its error type before any launch (CPU tensors, no library call), the
documented ring semantics of the push as a host model, and the checkpoint container with and without a bank."""
import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, dp, ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer


def _cpu_trainer(**kw):
    torch.manual_seed(0)
    return BridgeTrainer(eeg_channels=8, device="cpu", **kw)


def _cpu_batch(B):
    return torch.zeros(B, 8, 128), torch.zeros(B, 1, 16, 16, 16)


@pytest.fixture
def no_launch(monkeypatch):
    """any library call fails the test: the rules must raise before a launch"""
    def refuse(name, *a):
        raise AssertionError(f"{name} was called")
    monkeypatch.setattr(_hip, "call", refuse)


def test_header_declares_the_entry_points_and_hip_maps_them():
    sigs = _hip.parse_header()
    assert sigs["mm_clip_bank_loss"] == "p" * 9 + "iiii"            # z gid bank bank_gid state logit_scale scal4 dz ws | B K N warmup
    assert sigs["mm_clip_bank_push"] == "p" * 5 + "iii"
    assert sigs["mm_clip_bank_ws_floats"] == "iiip"
    assert _hip.header_abi_version() == 5


def test_clip_bank_check_rejects_what_the_kernels_do_not_serve(no_launch):
    ops.clip_bank_check(32, 4096, 128, 0, "t")
    ops.clip_bank_check(8, 8, 4, 3, "t")
    for args, msg in (((9, 8, 128, 0), "does not fit"), ((0, 8, 128, 0), "does not fit"), ((4, 8, 6, 0), "multiple of 4"),
                      ((4, 8, 0, 0), "multiple of 4"), ((4, 8, 128, -1), "warmup"), ((1, 0, 128, 0), "at least one row")):
        with pytest.raises(ValueError, match=msg):
            ops.clip_bank_check(*args, "t")


def test_constructor_rules(no_launch, monkeypatch):
    with pytest.raises(ValueError, match="bank_size"):
        _cpu_trainer(bank_size=-1)
    with pytest.raises(ValueError, match="bank_warmup"):
        _cpu_trainer(bank_size=64, bank_warmup=-2)
    with pytest.raises(ValueError, match="sigmoid"):
        _cpu_trainer(bank_size=64, loss="sigmoid")
    monkeypatch.setattr(dp, "world_size", lambda group: 2 if group is not None else 1)
    with pytest.raises(NotImplementedError, match="gathered rows"):
        _cpu_trainer(bank_size=64, group=object())
    tr = _cpu_trainer(bank_size=64, bank_warmup=3)
    assert tr.bank_size == 64 and tr.bank_filled == 0 and tr._bank is None      # storage comes with the first step
    with pytest.raises(AttributeError):
        tr.bank_size = 8                                                        # read-only
    d = _cpu_trainer()
    assert d.bank_size == 0 and d.bank_filled == 0


def test_a_batch_larger_than_the_bank_is_refused_before_any_launch(no_launch):
    tr = _cpu_trainer(bank_size=8, mode="manual")
    with pytest.raises(ValueError, match="does not fit"):
        tr.train_step(*_cpu_batch(16))
    assert tr._bank is None and tr._bank_grouped is None


def test_grouping_is_fixed_by_the_first_step_and_reset_bank_lifts_it(no_launch):
    tr = _cpu_trainer(bank_size=32, mode="manual")
    tr._bank_prepare(8, False, "train_step")                    # what a first plain step does before its launches
    assert tr._bank is not None and tr._bank.bank.shape == (32, 256) and tr._bank.state.tolist() == [0, 0, 0, 0]
    ids = torch.arange(8) // 2
    with pytest.raises(ValueError, match="reset_bank"):
        tr.train_step(*_cpu_batch(8), groups=ids)
    tr.reset_bank()
    tr._bank_prepare(8, True, "train_step")                     # now a grouped run may begin
    with pytest.raises(ValueError, match="reset_bank"):
        tr.train_step(*_cpu_batch(8))
    storage = tr._bank.bank.data_ptr()
    tr.reset_bank()
    tr._bank_prepare(8, False, "train_step")
    assert tr._bank.bank.data_ptr() == storage                  # the storage (and a captured step's pointers) stays


def ring_push(words, B, K):
    """the documented push on the host: rows go to slots (head + i) mod K, THEN head, filled and pushes advance"""
    head, filled, pushes = words[:3]
    return [(head + i) % K for i in range(B)], [(head + B) % K, min(filled + B, K), pushes + 1, 0]


def test_ring_model_matches_the_documented_semantics():
    K, B = 16, 6
    words, owner = [0, 0, 0, 0], [None] * K
    for step in range(7):
        slots, words = ring_push(words, B, K)
        for i, s in enumerate(slots):
            owner[s] = (step, i)
        rows = (step + 1) * B
        assert words == [rows % K, min(rows, K), step + 1, 0]
        # the ring never wraps before it is full: the valid slots are [0, filled), and they hold the newest rows
        assert all(o is not None for o in owner[:words[1]]) and all(o is None for o in owner[words[1]:])
        newest = {(q // B, q % B) for q in range(max(rows - K, 0), rows)}
        assert {o for o in owner if o is not None} == newest
    assert ring_push([10, 16, 4, 0], 6, 16)[0] == [10, 11, 12, 13, 14, 15][:6]
    assert ring_push([12, 12, 2, 0], 6, 16) == ([12, 13, 14, 15, 0, 1], [2, 16, 3, 0])      # wraps inside a batch
    assert ring_push([0, 8, 5, 0], 8, 8) == (list(range(8)), [0, 8, 6, 0])                  # B = K


def test_checkpoint_container_with_and_without_a_bank(no_launch):
    d = _cpu_trainer()
    assert "bank" not in d.checkpoint_state()["bridge_trainer_state"]
    tr = _cpu_trainer(bank_size=32, bank_warmup=2)
    ck = tr.checkpoint_state()["bridge_trainer_state"]["bank"]
    assert ck == {"size": 32, "warmup": 2, "grouped": None, "state": [0, 0, 0, 0], "rows": None, "ids": None}
    # a bank with content (filled on the host as three pushes of 8 grouped rows would)
    tr._bank_prepare(8, True, "train_step")
    words = [0, 0, 0, 0]
    for step in range(3):
        slots, words = ring_push(words, 8, 32)
        tr._bank.bank[slots] = torch.randn(8, 256)
        tr._bank.gid[slots] = torch.arange(8, dtype=torch.int32) + 10 * step
    tr._bank.state.copy_(torch.tensor(words, dtype=torch.int32))
    sd = tr.checkpoint_state()
    ck = sd["bridge_trainer_state"]["bank"]
    assert ck["size"] == 32 and ck["warmup"] == 2 and ck["grouped"] is True and ck["state"] == [24, 24, 3, 0]
    assert torch.equal(ck["rows"], tr._bank.bank) and torch.equal(ck["ids"], tr._bank.gid)
    assert tr.bank_filled == 24
    other = _cpu_trainer(bank_size=32, bank_warmup=2)
    other.load_checkpoint_state(sd)
    assert other._bank_grouped is True and other._bank.grouped and other.bank_filled == 24
    assert torch.equal(other._bank.bank, tr._bank.bank) and torch.equal(other._bank.gid, tr._bank.gid)
    assert other._bank.state.tolist() == [24, 24, 3, 0]
    with pytest.raises(ValueError, match="reset_bank"):          # the loaded bank is a grouped one
        other.train_step(*_cpu_batch(8))
    for kw, field in ((dict(), "bank differs"), (dict(bank_size=16, bank_warmup=2), r"bank\.size"),
                      (dict(bank_size=32, bank_warmup=0), r"bank\.warmup")):
        with pytest.raises(ValueError, match=field):
            _cpu_trainer(**kw).load_checkpoint_state(sd)
    with pytest.raises(ValueError, match="bank differs"):
        _cpu_trainer(bank_size=32).load_checkpoint_state(d.checkpoint_state())
