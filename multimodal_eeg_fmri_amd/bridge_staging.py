"""How a batch reaches a captured step's static inputs (`TrainerStagingMixin._stage`: the one decision of a graph-mode
`train_step` before its replay), and `AUGMENTERS`, the one table of the augmenters a trainer may hold: the step counters, the
packed host path's refusals and the checkpoint (bridge_checkpoint.py) go through it."""
from typing import NamedTuple

import torch

from . import _hip, dp, ops


class Augmenter(NamedTuple):
    attr: str           # the trainer attribute, constructor keyword and checkpoint key
    counter: str        # the trainer attribute that holds its next step index (the two EEG augmenters share one)
    noun: str           # in the packed host path's refusal
    ckpt_noun: str      # in the checkpoint's "written with / without ..." refusal
    reason: str         # why a batch packed on the host cannot take it


AUGMENTERS = (
    Augmenter("augment", "_aug_step", "an augmenter", "an augmenter",
              "a batch that is already packed to bf16 on the host cannot be augmented after the fact (the noise scale needs "
              "the fp32 sample)"),
    Augmenter("eeg_time_augment", "_aug_step", "a temporal EEG augmenter", "a temporal augmenter",
              "a batch that is already packed to bf16 on the host cannot be augmented after the fact (the shift gathers from "
              "the fp32 sample)"),
    Augmenter("fmri_augment", "_fmri_aug_step", "a volume augmenter", "a volume augmenter",
              "the packed path copies the host's bytes straight into the static inputs the volume augmentation writes (one "
              "copy, no launch that could augment)"),
)


def _dev_f32(t: torch.Tensor) -> bool:
    """what a kernel reads where it lies: a contiguous fp32 device tensor"""
    return t.dtype == torch.float32 and t.is_cuda and t.is_contiguous()


def _scratch(c: dict, key: str) -> torch.Tensor:
    """a tensor shaped like the static ``c[key]``, kept with the capture as ``c[key + "_scratch"]``: no allocation per step"""
    if c.get(key + "_scratch") is None:
        c[key + "_scratch"] = torch.empty(c[key].shape, dtype=torch.float32, device=c[key].device)
    return c[key + "_scratch"]


class TrainerStagingMixin:
    def _take_step(self, counter: str):
        """this `train_step`'s index from ``counter`` (one per call, whatever the mode), None without an augmenter that draws with it"""
        if all(getattr(self, a.attr) is None for a in AUGMENTERS if a.counter == counter):
            return None
        step = getattr(self, counter)
        setattr(self, counter, step + 1)
        return step

    def _no_packed_augment(self, who: str):
        if self.classify:
            raise ValueError(f"{who}: the packed host-fed path carries no class labels; feed a classify=True trainer "
                             "through train_step(eeg, fmri, groups, labels)")
        for a in AUGMENTERS:
            if getattr(self, a.attr) is not None:
                raise ValueError(f"{who}: this trainer has {a.noun}, and {a.reason}; feed train_step(eeg, fmri) from device "
                                 f"tensors, or build the trainer without {a.attr}=")

    def _augmented_eeg(self, eeg, aug_step):
        """the augmented copy of an EEG batch of any dtype and layout at step index ``aug_step``: both EEG augmenters in
        one pass when both exist"""
        if self.eeg_time_augment is not None:
            return self.eeg_time_augment.batch(eeg, aug_step, dp.rank(self.group), base=self.augment)
        return self.augment.batch(eeg, aug_step, dp.rank(self.group))

    def _stage(self, c, eeg, fmri, aug_step, fmri_aug_step):
        """a batch into the static inputs of the captured step ``c``.  ``aug_step`` / ``fmri_aug_step``: the step index of
        the EEG / volume augmentation, None without that augmenter.  The shifts are gathers and never run in place: a
        source that overlaps its static buffer (an in-place loader) is augmented into a scratch tensor and copied."""
        rank = dp.rank(self.group)
        # ---- fMRI: augmented into the static buffer by the two launches of csrc/volume_augment.hip - else a pending copy
        if fmri_aug_step is not None:
            src = fmri.detach().to(c["fmri"].device, torch.float32).contiguous()     # (the tensor itself when it already is all that)
            dst = _scratch(c, "fmri") if ops._overlap(src, c["fmri"]) else c["fmri"]
            c["fmri_aug_plan"] = ops.volume_augment_into(src, dst, step=fmri_aug_step, rank=rank, plan=c.get("fmri_aug_plan"),
                                                         **self.fmri_augment.kernel_args(fmri.shape))
            if dst is not c["fmri"]:
                c["fmri"].copy_(dst)
            fmri = c["fmri"]
        copy_fmri = fmri.data_ptr() != c["fmri"].data_ptr()
        # ---- EEG, augmented
        if aug_step is not None:
            args = dict(base_args=None if self.augment is None else self.augment.kernel_args(eeg.shape[1]),
                        time_args=None if self.eeg_time_augment is None else self.eeg_time_augment.kernel_args(eeg.shape[2]),
                        step=aug_step, rank=rank, plan=c.get("aug_plan"))
            if c["xb"] is not None and _dev_f32(eeg):
                # straight into the packed operand, the augmentation between the staging launch's load and its transpose
                # tile; that launch takes the fMRI copy along when it can (16-byte aligned, a multiple of 4 floats)
                ride = copy_fmri and _dev_f32(fmri) and fmri.numel() % 4 == 0 and fmri.data_ptr() % 16 == 0
                c["aug_plan"] = ops.eeg_augmenters_into(eeg, c["xb"], None, fmri_dst=c["fmri"] if ride else None,
                                                        fmri_src=fmri if ride else None, **args)
                if copy_fmri and not ride:
                    c["fmri"].copy_(fmri)
                return
            # the step reads the fp32 batch (the STFT front end), or the batch is no contiguous fp32 device tensor: augment
            # to fp32, then stage that plainly
            if self.eeg_time_augment is not None and _dev_f32(eeg):
                dst = _scratch(c, "eeg") if ops._overlap(eeg, c["eeg"]) else c["eeg"]
                c["aug_plan"] = ops.eeg_augmenters_into(eeg, None, dst, **args)
                eeg = dst
            else:
                eeg = self._augmented_eeg(eeg, aug_step)
        # ---- EEG, plainly (with the pending fMRI copy)
        copy_eeg, (Bx, Cx, Tx) = eeg.data_ptr() != c["eeg"].data_ptr(), eeg.shape
        if (c["xb"] is not None and copy_eeg and copy_fmri and _dev_f32(eeg) and _dev_f32(fmri) and eeg.numel() % 4 == 0
                and fmri.numel() % 4 == 0 and (eeg.data_ptr() | fmri.data_ptr()) % 16 == 0):
            # ONE launch: EEG batch packed into the first convolution's bf16 operand, fMRI batch copied
            # (no fp32 copy of the EEG batch: the captured step reads the packed operand only - c["eeg"] gives it its shape)
            _hip.call("mm_stage_inputs", eeg, c["xb"], None, Bx, Cx, Tx, c["xb"].shape[2], c["fmri"], fmri, fmri.numel())
            return
        if copy_fmri:                                       # each input on its own: a loader may fill only one in place
            c["fmri"].copy_(fmri)
        # the fp32 batch into c["eeg"] when the step itself reads c["eeg"], or the pack launch cannot read the batch where it lies
        if copy_eeg and (c["xb"] is None or not _dev_f32(eeg)):
            c["eeg"].copy_(eeg)
            eeg = c["eeg"]
        if c["xb"] is not None:
            _hip.call("mm_pack_nct_bf16", eeg, c["xb"], Bx, Cx, Tx, c["xb"].shape[2])
