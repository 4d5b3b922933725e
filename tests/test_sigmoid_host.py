"""CPU: the host side of `BridgeTrainer(loss="sigmoid")` - the loss name, the one extra bucket slot (`logit_bias`, in the
heads' layer group), the unchanged default trainer and the checkpoint refusal between the two losses (the trainer
constructs on CPU; nothing here launches a kernel)."""
import math

import pytest
import torch

from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer
from multimodal_eeg_fmri_amd.bridge_utils import EEGfMRIContrastiveBridge


def _trainer(seed=0, **kw):
    torch.manual_seed(seed)
    kw.setdefault("eeg_channels", 8)
    return BridgeTrainer(device="cpu", mode="manual", **kw)


def test_unknown_loss_name_is_refused_and_lists_the_two():
    for build in (lambda: _trainer(loss="triplet"), lambda: EEGfMRIContrastiveBridge(loss="triplet")):
        with pytest.raises(ValueError) as e:
            build()
        assert "infonce" in str(e.value) and "sigmoid" in str(e.value) and "triplet" in str(e.value)


def test_head_parameters_and_initial_values():
    h = EEGfMRIContrastiveBridge(loss="sigmoid")
    assert h.logit_scale.item() == pytest.approx(math.log(10.0)) and h.logit_bias.item() == -10.0
    h = EEGfMRIContrastiveBridge(loss="sigmoid", init_scale=5.0, init_bias=-3.0)
    assert h.logit_scale.item() == pytest.approx(math.log(5.0)) and h.logit_bias.item() == -3.0
    d = EEGfMRIContrastiveBridge()
    assert d.loss == "infonce" and not hasattr(d, "logit_bias") and "logit_bias" not in d.state_dict()
    assert d.logit_scale.item() == pytest.approx(math.log(1 / 0.07))
    assert list(EEGfMRIContrastiveBridge(loss="infonce").state_dict()) == list(d.state_dict())


def test_sigmoid_bucket_has_one_more_slot_in_the_heads_group():
    d, s = _trainer(), _trainer(loss="sigmoid")
    assert s.loss == "sigmoid" and d.loss == "infonce"
    assert s.bucket.n == d.bucket.n + 1 and s._scal.numel() == 5 and d._scal.numel() == 4
    b = s.bucket
    off = (s.head.logit_bias.data_ptr() - b.p.data_ptr()) // 4
    off_scale = (s.head.logit_scale.data_ptr() - b.p.data_ptr()) // 4
    assert off == off_scale + 1                                    # right after logit_scale
    name, ready, lo, hi = next(g for g in s.groups if g[2] <= off < g[3])
    assert "heads" in name and lo <= off_scale < hi
    assert ready == next(g for g in d.groups if "heads" in g[0])[1]
    # every other group keeps its size; the groups after the heads' move up by one
    assert [(g[0], g[1], g[3] - g[2]) for g in s.groups] == [(g[0], g[1], g[3] - g[2] + ("heads" in g[0])) for g in d.groups]
    assert any(p is s.head.logit_bias for _, _, p, _ in s.optimizer_param_map())
    assert s.head.logit_bias.item() == -10.0                       # the value survived the move into the bucket


def test_default_trainer_is_the_trainer_without_the_keyword():
    a, b = _trainer(), _trainer(loss="infonce")
    assert a.groups == b.groups and a.bucket.n == b.bucket.n
    assert list(a.state_dict()) == list(b.state_dict()) and "head.logit_bias" not in a.state_dict()
    assert torch.equal(a.bucket.p, b.bucket.p)
    ca, cb = a.checkpoint_state(), b.checkpoint_state()
    assert "loss" not in ca["bridge_trainer_state"] and "loss" not in cb["bridge_trainer_state"]
    assert list(ca["bridge_trainer_state"]) == list(cb["bridge_trainer_state"])
    a.load_checkpoint_state(cb)


@pytest.mark.parametrize("written_by,loaded_into", [("sigmoid", "infonce"), ("infonce", "sigmoid")])
def test_a_checkpoint_of_the_other_loss_is_refused_by_name(written_by, loaded_into):
    ck = _trainer(loss=written_by).checkpoint_state()
    assert ck["bridge_trainer_state"].get("loss") == (None if written_by == "infonce" else "sigmoid")
    tr = _trainer(seed=3, loss=loaded_into)
    before = tr.bucket.p.clone()
    with pytest.raises(ValueError, match="loss differs") as e:
        tr.load_checkpoint_state(ck)
    assert written_by in str(e.value) and loaded_into in str(e.value)
    assert torch.equal(tr.bucket.p, before)


def test_compatibility_on_containers_built_by_hand():
    """the refusal reads the field, not the shapes: a sigmoid container whose `loss` field is edited is refused by a
    sigmoid trainer, and a default container with the field set to "infonce" loads into a default trainer"""
    s = _trainer(loss="sigmoid")
    ck = s.checkpoint_state()
    s.load_checkpoint_state(ck)
    ck["bridge_trainer_state"]["loss"] = "infonce"
    with pytest.raises(ValueError, match="loss differs"):
        s.load_checkpoint_state(ck)
    del ck["bridge_trainer_state"]["loss"]
    with pytest.raises(ValueError, match="loss differs"):
        s.load_checkpoint_state(ck)
    d = _trainer()
    ck = d.checkpoint_state()
    ck["bridge_trainer_state"]["loss"] = "infonce"
    d.load_checkpoint_state(ck)
    ck["bridge_trainer_state"]["loss"] = "sigmoid"
    with pytest.raises(ValueError, match="loss differs"):
        d.load_checkpoint_state(ck)
