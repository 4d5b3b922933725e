"""GPU: how a batch reaches the captured step's static buffers - the `_hip.call` names the second `train_step` of a
graph-mode trainer issues (after the capture), what the static buffers then hold, and what happens to the caller's
tensors, for every subset of the three augmenters under five feeds.  The name lists are literals: what the trainer issued
before its staging code was folded into one decision (`TrainerStagingMixin._stage`), recorded on that commit."""
import itertools

import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
from multimodal_eeg_fmri_amd.crossmodal_eeg_scr import EEGTimeTransforms, EEGTransforms
from multimodal_eeg_fmri_amd.fmri_utils import VolumeTransforms

pytestmark = pytest.mark.gpu

B, C, T, VOL = 4, 8, 64, (8, 8, 8)
T_STFT = 256                                   # the STFT front end's epochs (n_fft 16 and 32, hop 8), as in the other trainer tests
B_ODD, VOL_ODD = 3, (5, 7, 9)                  # 3 * 315 floats: no multiple of 4, the fMRI copy cannot ride in the staging launch

PLAN, AUG, TAUG = "mm_eeg_augment_plan", "mm_stage_inputs_aug", "mm_stage_inputs_taug"
STAGE, PACK = "mm_stage_inputs", "mm_pack_nct_bf16"
VOLUME = ["mm_volume_augment_plan", "mm_volume_augment"]

FEEDS = ["contiguous", "static buffers", "transposed eeg", "stft", "odd volume"]
SUBSETS = list(itertools.product((False, True), repeat=3))          # (augment=, eeg_time_augment=, fmri_augment=)


def _id(subset):
    return "+".join(n for n, on in zip(("eeg", "time", "volume"), subset) if on) or "none"


# what the trainer issued before the fold, per feed and augmenter subset
_FUSED = {"eeg": [PLAN, AUG], "time": [TAUG], "eeg+time": [PLAN, TAUG],                    # the augmenters' launches stage the batch
          "volume": VOLUME + [PACK], "eeg+volume": VOLUME + [PLAN, AUG], "time+volume": VOLUME + [TAUG],
          "eeg+time+volume": VOLUME + [PLAN, TAUG]}
NAMES = {
    "contiguous": dict(_FUSED, none=[STAGE]),
    "static buffers": dict(_FUSED, none=[PACK]),
    "odd volume": dict(_FUSED, none=[PACK]),                         # (the fMRI batch: a tensor copy)
    "transposed eeg": {                                              # augmented to a new fp32 batch, which is then staged plainly
        "none": [PACK], "eeg": [PLAN, AUG, STAGE], "time": [TAUG, STAGE], "eeg+time": [PLAN, TAUG, STAGE],
        "volume": VOLUME + [PACK], "eeg+volume": VOLUME + [PLAN, AUG, PACK], "time+volume": VOLUME + [TAUG, PACK],
        "eeg+time+volume": VOLUME + [PLAN, TAUG, PACK]},
    "stft": {                                                        # no packed operand: the augmenters' launches, then tensor copies
        "none": [], "eeg": [PLAN, AUG], "time": [TAUG], "eeg+time": [PLAN, TAUG],
        "volume": VOLUME, "eeg+volume": VOLUME + [PLAN, AUG], "time+volume": VOLUME + [TAUG],
        "eeg+time+volume": VOLUME + [PLAN, TAUG]},
}


@pytest.fixture(autouse=True)
def _no_seed_epoch():
    ops.set_seed_epoch(None)
    yield
    ops.set_seed_epoch(None)


@pytest.fixture(scope="module")
def batches():
    return {"erp": [synthetic_pairs(B, C, T, VOL, seed=900 + i) for i in range(2)],
            "stft": [synthetic_pairs(B, C, T_STFT, VOL, seed=910 + i) for i in range(2)],
            "odd volume": [synthetic_pairs(B_ODD, C, T, VOL_ODD, seed=920 + i) for i in range(2)]}


def _augmenters(eeg_aug, time_aug, vol_aug):
    return (EEGTransforms(p=1.0, seed=5) if eeg_aug else None,
            EEGTimeTransforms(p_shift=1.0, max_shift=16, p_scale=1.0, p_invert=0.5, p_mask=1.0, seed=6) if time_aug else None,
            VolumeTransforms(p_flip=1.0, p_shift=1.0, max_shift=2, p_scale=1.0, p_noise=1.0, p_erase=1.0, seed=13) if vol_aug else None)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


@pytest.mark.parametrize("subset", SUBSETS, ids=_id)
@pytest.mark.parametrize("feed", FEEDS)
def test_launches_buffers_and_the_callers_tensors(batches, monkeypatch, feed, subset):
    base, time_aug, vol_aug = _augmenters(*subset)
    pairs = batches[feed if feed in ("stft", "odd volume") else "erp"]
    kw = {}
    if feed == "stft":
        from multimodal_eeg_fmri_amd.crossmodal_v4_enhancements import MultiScaleSTFTPowerEncoder
        torch.manual_seed(0)
        kw["eeg_encoder"] = MultiScaleSTFTPowerEncoder(C, (16, 32), 8, 128, 2, 4, 0.0)
    ops.set_dropout_seed(2024)
    torch.manual_seed(0)
    tr = BridgeTrainer(eeg_channels=C, dropout=0.0, lr=1e-3, mode="graph", augment=base, eeg_time_augment=time_aug,
                       fmri_augment=vol_aug, **kw).train()
    tr.train_step(*pairs[0])                                         # the capture (its warm-up steps consume no step index)
    torch.cuda.synchronize()
    c = tr._cap
    assert (c["xb"] is None) == (feed == "stft")

    eeg0, fmri0 = pairs[1]
    eeg, fmri = eeg0, fmri0
    if feed == "static buffers":                                     # an in-place loader: the batches ARE the static buffers
        eeg, fmri = tr.input_buffers()
        eeg.copy_(eeg0)
        fmri.copy_(fmri0)
    elif feed == "transposed eeg":
        eeg = eeg0.transpose(1, 2).contiguous().transpose(1, 2)      # (B, T, C) memory seen as (B, C, T)
        assert not eeg.is_contiguous() and torch.equal(eeg, eeg0)
    torch.cuda.synchronize()

    names, real = [], _hip.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(_hip, "call", spy)
    loss = tr.train_step(eeg, fmri)["loss"].item()
    monkeypatch.setattr(_hip, "call", real)
    torch.cuda.synchronize()
    assert loss == loss
    assert names == NAMES[feed][_id(subset)], names
    assert tr.augment_step == (2 if subset[0] or subset[1] else 0) and tr.fmri_augment_step == (2 if subset[2] else 0)

    # the static buffers hold the batches the augmenters' front doors give at step index 1, bit for bit
    ref_base, ref_time, ref_vol = _augmenters(*subset)
    want_eeg = ref_time.batch(eeg0, 1, 0, base=ref_base) if ref_time is not None else \
        ref_base.batch(eeg0, 1, 0) if ref_base is not None else eeg0
    want_fmri = ref_vol.batch(fmri0, 1, 0) if ref_vol is not None else fmri0
    assert (subset[0] or subset[1]) == (not torch.equal(want_eeg, eeg0)) and subset[2] == (not torch.equal(want_fmri, fmri0))
    eeg_buf, fmri_buf = tr.input_buffers()
    assert torch.equal(_bits(fmri_buf), _bits(want_fmri))
    if c["xb"] is None:
        assert torch.equal(_bits(eeg_buf), _bits(want_eeg))          # the step reads the fp32 batch
    else:
        assert torch.equal(_bits(c["xb"]), _bits(ops.pack_nct(want_eeg)))   # the step reads the packed operand only

    # the caller's tensors are only read - except a volume batch that is the static buffer, augmented where it lies
    assert torch.equal(_bits(eeg), _bits(eeg0))
    if not (feed == "static buffers" and subset[2]):
        assert torch.equal(_bits(fmri), _bits(fmri0))
