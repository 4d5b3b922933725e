"""Averaged weights (EMA), host side: argument validation of `BridgeTrainer(ema_decay=)`, `FusedAdamW(ema_decay=)` and
`fit(validate_with=)`, the header's declaration of mm_adamw_clip_ema, and the fp64 decay schedule the GPU tests compare
the kernel's state[5] with (`ema_decay_schedule`, checked here against a table computed by hand)."""
import re

import pytest
import torch

from multimodal_eeg_fmri_amd import _hip
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer
from multimodal_eeg_fmri_amd.optim import FusedAdamW


def ema_decay_schedule(step_before: int, ema_decay: float, ema_warmup: bool) -> float:
    """the decay mm_adamw_clip_ema uses in the step that starts at step count ``step_before``, in fp64: with
    t = step_before + 1, min(ema_decay, (1 + t) / (10 + t)) under warm-up, ema_decay without (include/mmeeg_hip.h)"""
    t = step_before + 1
    return min(float(ema_decay), (1.0 + t) / (10.0 + t)) if ema_warmup else float(ema_decay)


def ema_reference(shadow, p_new, d):
    """fp64: shadow + (1 - d) (p_new - shadow)"""
    shadow, p_new = shadow.double(), p_new.double()
    return shadow + (1.0 - d) * (p_new - shadow)


def test_schedule_helper_agrees_with_a_hand_computed_table():
    # step count before the step -> t -> (1 + t) / (10 + t)
    #     0 -> 1     -> 2 / 11          7 -> 8 -> 9 / 18 = 0.5         89 -> 90 -> 91 / 100
    #  9999 -> 10000 -> 10001 / 10010 = 0.99910089..., above 0.999: the cap holds
    table = [(0, 0.999, True, 2 / 11), (7, 0.999, True, 0.5), (89, 0.999, True, 0.91), (9999, 0.999, True, 0.999),
             (0, 0.999, False, 0.999), (7, 0.9, False, 0.9), (0, 0.1, True, 0.1), (8990, 0.999, True, 0.999)]
    for step, d, warm, want in table:
        assert ema_decay_schedule(step, d, warm) == pytest.approx(want, rel=1e-15), (step, d, warm)
    # the counters of the kernel test land on both sides of the min
    assert ema_decay_schedule(0, 0.999, True) < 0.999 and ema_decay_schedule(7, 0.999, True) < 0.999
    assert 10001 / 10010 > 0.999 and ema_decay_schedule(9999, 0.999, True) == 0.999
    # t = 8990: (1 + t) / (10 + t) = 8991 / 9000 = 0.999 exactly at the crossing
    assert 8991 / 9000 == pytest.approx(0.999, rel=1e-15)


def test_ema_reference_is_a_fixed_point_where_shadow_equals_p():
    p = torch.randn(16)
    assert torch.equal(ema_reference(p, p, 0.37), p.double())
    assert torch.equal(ema_reference(torch.zeros(4), torch.ones(4), 0.75), torch.full((4,), 0.25, dtype=torch.float64))


@pytest.mark.parametrize("decay", [-0.1, 1.0, 1.5, float("nan")])
def test_trainer_rejects_a_decay_outside_the_range(decay):
    with pytest.raises(ValueError, match="ema_decay"):
        BridgeTrainer(eeg_channels=8, dropout=0.0, device="cpu", ema_decay=decay)


@pytest.mark.parametrize("decay", [-1e-3, 1.0])
def test_fused_adamw_rejects_a_decay_outside_the_range(decay):
    with pytest.raises(ValueError, match="ema_decay"):
        FusedAdamW([torch.nn.Parameter(torch.zeros(3))], ema_decay=decay)


def test_default_trainer_has_no_average_and_says_so():
    tr = BridgeTrainer(eeg_channels=8, dropout=0.0, device="cpu")
    assert tr.ema_decay == 0.0 and tr.bucket.ema is None
    assert "ema" not in tr.checkpoint_state()["bridge_trainer_state"]
    for call in (tr.sync_ema, tr.ema_state_dict, lambda: tr.ema_weights().__enter__()):
        with pytest.raises(RuntimeError, match="ema_decay"):
            call()


def test_averaging_trainer_allocates_the_shadow_as_a_copy_of_the_bucket():
    tr = BridgeTrainer(eeg_channels=8, dropout=0.0, device="cpu", ema_decay=0.99, ema_warmup=False)
    b = tr.bucket
    assert b.ema is not None and b.ema.data_ptr() != b.p.data_ptr() and torch.equal(b.ema, b.p)
    ck = tr.checkpoint_state()["bridge_trainer_state"]["ema"]
    assert ck["decay"] == 0.99 and ck["warmup"] is False
    assert ck["shadow"].dtype == torch.float32 and tuple(ck["shadow"].shape) == (b.n,) and torch.equal(ck["shadow"], b.p)


def test_fit_validate_with_ema_needs_an_averaging_trainer():
    tr = BridgeTrainer(eeg_channels=8, dropout=0.0, device="cpu")
    with pytest.raises(ValueError, match="validate_with"):
        tr.fit([], 2, warmup_epochs=0, validate_with="ema")
    with pytest.raises(ValueError, match="validate_with"):
        tr.fit([], 2, warmup_epochs=0, validate_with="shadow")


def test_header_declares_the_entry_point_and_keeps_the_abi_version():
    sigs = _hip.parse_header()
    assert sigs["mm_adamw_clip"] == "ppppp" + "l" + "ffffff" + "i" + "p"            # its argument list is unchanged
    assert sigs["mm_adamw_clip_ema"] == sigs["mm_adamw_clip"] + "pfi"
    assert _hip.header_abi_version() == 5
    text = open(_hip.header_path()).read()
    assert re.search(r"state\[5\]", text), "the header documents the decay word next to words 0 to 4"
