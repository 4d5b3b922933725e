"""CPU: the host side of the ignored-neighbour contrastive losses - the four masked entry points in the header, the
unchanged ABI version, `bridge_utils.timeline_ids`, the constructor and argument errors of
`BridgeTrainer(neighbour_radius=)` and the checkpoint field (the trainer constructs on CPU; nothing here launches a
kernel)."""
import re

import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer
from multimodal_eeg_fmri_amd.bridge_utils import timeline_ids


def _trainer(seed=0, **kw):
    torch.manual_seed(seed)
    kw.setdefault("eeg_channels", 8)
    return BridgeTrainer(device="cpu", mode="manual", **kw)


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", " ", open(_hip.header_path()).read(), flags=re.S)
    m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in the header"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_four_masked_entry_points():
    assert _declaration("mm_clip_loss_own_rows_masked") == [
        "const float* z_all", "const int* gid_all", "const float* logit_scale", "float* scal4", "float* dz_local",
        "float* ws", "int B", "int Bg", "int N", "int row0", "int radius", "hipStream_t stream"]
    assert _declaration("mm_sigmoid_loss_own_rows_masked") == [
        "const float* z_all", "const int* gid_all", "const float* logit_scale", "const float* logit_bias", "float* scal5",
        "float* dz_local", "float* ws", "int B", "int Bg", "int N", "int row0", "int radius", "hipStream_t stream"]
    for name in ("mm_clip_loss_masked_ws_floats", "mm_sigmoid_loss_masked_ws_floats"):
        assert _declaration(name) == ["int B", "int Bg", "int* floats_host", "hipStream_t stream"]
    sigs = _hip.parse_header()
    # the masked forms are the grouped forms plus one int in front of the stream: the own-rows signature is unchanged
    assert sigs["mm_clip_loss_own_rows_masked"] == sigs["mm_clip_loss_own_rows_grouped"] + "i"
    assert sigs["mm_sigmoid_loss_own_rows_masked"] == sigs["mm_sigmoid_loss_own_rows"] + "i"
    assert sigs["mm_clip_loss_masked_ws_floats"] == sigs["mm_clip_loss_grouped_ws_floats"]
    assert sigs["mm_sigmoid_loss_masked_ws_floats"] == sigs["mm_sigmoid_loss_ws_floats"]


def test_abi_version_is_unchanged():
    assert _hip.header_abi_version() == 5                      # entry points were only added


def test_timeline_ids_separate_runs_and_keep_distances():
    runs = torch.tensor([7, 7, 7, 3, 3, 3, 7])
    times = torch.tensor([10, 11, 14, 10, 14, 12, 11])
    for radius in (0, 1, 4, 100):
        ids = timeline_ids(runs, times, radius)
        assert ids.dtype == torch.int32 and ids.shape == (7,)
        d = (ids.long()[:, None] - ids.long()[None, :]).abs()
        same_run = runs[:, None] == runs[None, :]
        dt = (times[:, None] - times[None, :]).abs()
        assert torch.equal(d[same_run], dt[same_run])           # inside a run: the distance in time
        assert bool((d[~same_run] > radius).all())              # across runs: never a neighbour, never a positive
        assert ids[1].item() == ids[6].item()                   # equal (run, t): equal ids, positives of each other
    assert timeline_ids(torch.tensor([5, 9]), torch.tensor([0, 0]), 2).tolist() == [0, 3]     # stride = span + radius + 1
    assert timeline_ids(torch.tensor([0, 0, 1]), torch.tensor([-4, 5, -4]), 1).tolist() == [0, 9, 11]
    assert timeline_ids(torch.tensor([], dtype=torch.int64), torch.tensor([], dtype=torch.int64), 1).shape == (0,)


def test_timeline_ids_refuse_what_int32_cannot_hold_and_bad_arguments():
    timeline_ids(torch.tensor([0, 1]), torch.tensor([0, 2 ** 30 - 2]), 0)              # 2^31 - 3: fits
    with pytest.raises(ValueError, match="int32"):
        timeline_ids(torch.tensor([0, 1, 2]), torch.tensor([0, 2 ** 30, 5]), 0)
    with pytest.raises(ValueError, match="int32"):
        timeline_ids(torch.tensor([0, 1]), torch.tensor([0, 5]), 2 ** 31)
    with pytest.raises(ValueError, match="radius"):
        timeline_ids(torch.tensor([0]), torch.tensor([0]), -1)
    with pytest.raises(ValueError, match="integer"):
        timeline_ids(torch.tensor([0]), torch.tensor([0.5]), 1)
    with pytest.raises(ValueError, match="2 runs but 3 times"):
        timeline_ids(torch.tensor([0, 1]), torch.tensor([0, 1, 2]), 1)


@pytest.mark.parametrize("kw", [dict(bank_size=64), dict(bank_size=64, key_encoder=True, ema_decay=0.99)],
                         ids=["bank", "key_encoder"])
def test_a_bank_and_a_radius_are_refused_at_construction(kw):
    with pytest.raises(ValueError, match="no ignore relation") as e:
        _trainer(neighbour_radius=2, **kw)
    assert "neighbour_radius" in str(e.value) and "bank" in str(e.value)
    _trainer(neighbour_radius=0, **kw)                          # radius 0: the trainer it always was


def test_a_negative_radius_is_refused():
    with pytest.raises(ValueError, match="neighbour_radius"):
        _trainer(neighbour_radius=-1)


@pytest.mark.parametrize("loss", ["infonce", "sigmoid"])
def test_a_radius_needs_groups_in_every_entry_point(loss):
    tr = _trainer(neighbour_radius=2, loss=loss)
    eeg, fmri = torch.zeros(4, 8, 256), torch.zeros(4, 1, 16, 16, 16)
    for call in (tr.train_step, tr.forward, tr.evaluate):
        with pytest.raises(ValueError, match="groups=") as e:
            call(eeg, fmri)
        assert "neighbour_radius=2" in str(e.value)
    tr = _trainer(neighbour_radius=1, classify=True)
    with pytest.raises(ValueError, match="groups="):
        tr.evaluate(eeg, fmri, labels=torch.zeros(4, dtype=torch.int64))


def test_ops_refuse_a_radius_without_ids_before_any_launch():
    z, one = torch.zeros(4, 8), torch.zeros(1)
    with pytest.raises(ValueError, match="needs group ids"):
        ops.clip_loss_own_rows(z, None, one, torch.zeros(4), None, 4, 0, radius=1)
    with pytest.raises(ValueError, match="needs group ids"):
        ops.sigmoid_loss_own_rows(z, None, one, one, torch.zeros(5), None, 4, 0, radius=3)
    with pytest.raises(ValueError, match="radius must be >= 0"):
        ops.clip_loss_own_rows(z, torch.zeros(4, dtype=torch.int32), one, torch.zeros(4), None, 4, 0, radius=-1)


def test_the_checkpoint_records_the_radius_only_when_set_and_refuses_another():
    d = _trainer()
    cd = d.checkpoint_state()
    assert "neighbour_radius" not in cd["bridge_trainer_state"]
    assert list(cd["bridge_trainer_state"]) == list(_trainer(neighbour_radius=0).checkpoint_state()["bridge_trainer_state"])
    m = _trainer(neighbour_radius=2)
    cm = m.checkpoint_state()
    assert cm["bridge_trainer_state"]["neighbour_radius"] == 2
    assert [k for k in cm["bridge_trainer_state"] if k != "neighbour_radius"] == list(cd["bridge_trainer_state"])
    m.load_checkpoint_state(cm)
    for tr, ck, words in ((d, cm, ("checkpoint 2", "trainer 0")), (m, cd, ("checkpoint 0", "trainer 2")),
                          (_trainer(neighbour_radius=3), cm, ("checkpoint 2", "trainer 3"))):
        before = tr.bucket.p.clone()
        with pytest.raises(ValueError, match="neighbour_radius differs") as e:
            tr.load_checkpoint_state(ck)
        assert all(w in str(e.value) for w in words)
        assert torch.equal(tr.bucket.p, before)
