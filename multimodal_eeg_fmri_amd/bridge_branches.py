"""What `BridgeTrainer` asks of its two encoder branches - `EEG_BRANCHES` (erp | power | stft) and `FMRI_BRANCHES` (volume |
tabular: one fMRI item per pair) with `FMRI_SEQUENCE_BRANCH` beside them (sequence: F frames per pair; `fmri_branch` looks a
kind up in both), plain tables in the style of `bridge_staging.AUGMENTERS` holding exactly what the trainer asks today - and
`step_schedule`, which decides a step's issue order once, as a pure function (the step's `ops.block_plan`).  The entries reach
the forward / backward functions through `ops`' attributes and this module's globals, looked up at call time: a test that
patches ``bridge_branches.erp_encoder_bwd`` sees the step's call."""
import math
from typing import Callable, Mapping, NamedTuple, Optional, Tuple

from . import ops
from .autograd import erp_encoder_bwd, fmri_tab_bwd, power_encoder_bwd, sequence_encoder_bwd, volume_encoder_bwd
from .crossmodal_v4_enhancements import MultiScaleSTFTPowerEncoder
from .enhanced_models_v4 import EnhancedERPEncoder, EnhancedPowerEncoder
from .fmri_utils import fMRISequenceEncoder3D, fMRITabularEncoder


class EEGBranch(NamedTuple):
    kind: str             # the checkpoint's "eeg_kind"
    encoder: type
    raw_input: bool       # the captured step reads the raw fp32 batch (else the first convolution's packed bf16 (B, T, Cp) operand)
    hands_over: bool      # its backward's hooks hand weight-gradient sums to the side stream (else they never fire)
    forward: Callable     # (encoder, eeg, xb, live) -> (features, saved); live False = frozen: the eval form, nothing saved, no seed drawn
    backward: Callable    # (bag, saved, dfe, after_blocks=, after_conv2=, after_conv3=) -> what to call after the bag's flush, or None
    layout: Callable      # (encoder, head_params) -> [(group name, ready point, parameters)] in bucket order


def _erp_layout(enc, head_params):
    cl = enc.conv_layers
    conv1 = list(cl[0].parameters()) + list(cl[1].parameters())
    conv23 = [p for i in (4, 5, 9, 10) for p in cl[i].parameters()]
    seen = {id(p) for p in conv1 + conv23}
    rest = [p for p in enc.parameters() if id(p) not in seen]
    return [("eeg conv block 1", "main", conv1), ("eeg conv blocks 2-3", "handed1", conv23),
            ("eeg transformer stack + heads", "handed0", rest + head_params)]


def _one_group_layout(enc, head_params):
    return [("eeg encoder + heads", "main", list(enc.parameters()) + head_params)]


def _erp_backward(bag, saved, dfe, **hooks):
    erp_encoder_bwd(bag, saved, dfe, **hooks)


def _power_backward(bag, saved, dfe, **hooks):
    return power_encoder_bwd(bag, saved, dfe)[1]      # finish(): the merged 192-channel conv / BatchNorm gradients back into the six real parameters


def _stft_forward(enc, eeg, xb, live):
    # config #5: the parameter-free multi-scale STFT power front-end (z-scored per sample), then a4
    return ops._power_forward_impl(enc.encoder, ops.stft_front_end(eeg, enc.n_ffts, enc.hop, enc.normalize), live, False)


# in the order `select_eeg` tests the types
EEG_BRANCHES = {b.kind: b for b in (
    EEGBranch("erp", EnhancedERPEncoder, False, True, lambda enc, eeg, xb, live: ops._erp_forward_impl(enc, eeg, live, live, xb=xb),
              _erp_backward, _erp_layout),
    EEGBranch("stft", MultiScaleSTFTPowerEncoder, True, False, _stft_forward, _power_backward, _one_group_layout),
    EEGBranch("power", EnhancedPowerEncoder, False, False,
              lambda enc, eeg, xb, live: ops._power_forward_impl(enc, xb if xb is not None else ops.pack_nct(eeg), live, False),
              _power_backward, _one_group_layout))}


def select_eeg(encoder) -> EEGBranch:
    for b in EEG_BRANCHES.values():
        if isinstance(encoder, b.encoder):
            return b
    raise TypeError(f"BridgeTrainer: no tape for an EEG encoder of type {type(encoder).__name__}")


class FMRIBranch(NamedTuple):
    kind: str
    check: Callable                     # (encoder, batch shape, training, who): ValueError before the first launch of a step
    capture_words: Optional[Callable]   # (encoder, device) -> int32 words that exist before a capture and are zero at its start
    forward: Callable                   # (encoder, fmri, live) -> (features, saved)
    backward: Callable                  # (bag, saved, dff)
    can_be_longer: bool                 # may outlast the EEG chain (`step_schedule`'s fmri_first)
    perturb_default: Tuple[str, int]    # `perturb`'s fmri_units=None
    perturb_kinds: Tuple[str, ...]      # the unit kinds `perturb` takes ...
    perturb_what: str                   # ... and how its refusal words them
    explain_views: Optional[Callable]   # (encoder, attribution, fMRI batch) -> further entries of `explain`'s result
    augmentable: bool                   # fmri_augment= (a VolumeTransforms) is allowed ...
    not_augmentable_why: str = ""       # ... and why not
    perturb_shape: Optional[Callable] = None   # (unit kind, sample shape) -> the sample shape `perturb` cuts its units from (None: as it is)
    checkpoint_tag: Optional[Callable] = None  # (encoder) -> what a checkpoint records of the branch beside its kind (None: nothing)


FMRI_BRANCHES = {b.kind: b for b in (
    FMRIBranch("volume", lambda enc, shape, training, who: ops.check_volume_shape(shape), None,
               lambda enc, fmri, live: ops._vol_forward_impl(enc, fmri, live, live),
               lambda bag, saved, dff: volume_encoder_bwd(bag, saved, dff),
               True, ("blocks", 8), ("blocks",), "('blocks', s) for the voxel encoder", None, True),
    # one launch each way (the backward: plain stores into the bucket's fMRI range): never the longer branch
    FMRIBranch("tabular", lambda enc, shape, training, who: ops.fmri_tab_check(enc, shape, training, f"{who} (tabular fMRI encoder)"),
               lambda enc, device: enc.tickets(device),
               lambda enc, fmri, live: ops._tab_forward_impl(enc, fmri, live, live),
               lambda bag, saved, dff: fmri_tab_bwd(bag, saved, dff),
               False, ("windows", 1), ("windows",), "('windows', w) for a tabular fMRI encoder",
               lambda enc, attr, fmri: dict(zip(("fmri_activation", "fmri_connectivity"), enc.split(attr))),   # views of the (B, A + C) attribution
               False, "the fMRITabularEncoder's input is a feature table (build the trainer without fmri_augment=, or with the "
               "voxel encoder)"))}

# F frames per pair: the volume branch's launches on the B * F volumes plus the lag pool's one launch each way (DESIGN.md
# section 5x).  ("rows", 1): one unit = one frame, the sample viewed as (F, D * H * W); ("blocks", s): the volume branch's
# kind with Cv = F, all frames of a block go together
FMRI_SEQUENCE_BRANCH = FMRIBranch(
    "sequence", lambda enc, shape, training, who: ops.check_sequence_shape(enc, shape, f"{who} (fMRI sequence encoder)"), None,
    lambda enc, fmri, live: ops._seq_forward_impl(enc, fmri, live),
    lambda bag, saved, dff: sequence_encoder_bwd(bag, saved, dff),
    True, ("rows", 1), ("rows", "blocks"), "('rows', 1) = one frame or ('blocks', s) for an fMRI sequence encoder",
    lambda enc, attr, fmri: {"fmri_frames": attr.flatten(2).sum(dim=2), "lag_weights": enc.lag_weights(fmri)},
    False, "a flip or shift must be the same for all frames of a sample, and VolumeTransforms draws per volume (build the "
    "trainer without fmri_augment=)",
    lambda kind, shape: (shape[0], math.prod(shape[1:])) if kind == "rows" else tuple(shape),
    lambda enc: {"frames": int(enc.frames)})


def fmri_branch(kind: str) -> FMRIBranch:
    return FMRI_SEQUENCE_BRANCH if kind == FMRI_SEQUENCE_BRANCH.kind else FMRI_BRANCHES[kind]


def select_fmri(encoder, fmri_dim: int) -> FMRIBranch:
    """``encoder``: the constructor's ``fmri_encoder`` (None = the voxel encoder, which the trainer builds)"""
    if encoder is None:
        return FMRI_BRANCHES["volume"]
    if isinstance(encoder, fMRISequenceEncoder3D):
        if encoder.out_dim != fmri_dim:
            raise ValueError(f"BridgeTrainer: fmri_dim={fmri_dim} but the fMRISequenceEncoder3D ends in {encoder.out_dim} features")
        return FMRI_SEQUENCE_BRANCH
    if not isinstance(encoder, fMRITabularEncoder):
        raise TypeError(f"BridgeTrainer: fmri_encoder must be an fMRITabularEncoder or None (the voxel encoder), got "
                        f"{type(encoder).__name__} (frame sequences take an fMRISequenceEncoder3D)")
    if encoder.hidden_dim != fmri_dim:
        raise ValueError(f"BridgeTrainer: fmri_dim={fmri_dim} but the fMRITabularEncoder ends in {encoder.hidden_dim} features")
    return FMRI_BRANCHES["tabular"]


def input_layout(eeg: EEGBranch, eeg_shape, fmri_numel: int, grouped: bool, labelled: bool = False):
    """byte counts (n_e, n_f, n_g, n_l) of a captured step's flat static input buffer = [EEG operand | fMRI batch fp32 |
    group ids int32 (grouped captures only) | class labels int32 (labelled captures only)]: what `pack_host_batch` fills on
    the host and `train_step_packed` copies in one piece.  EEG operand: the first convolution's packed bf16 (B, T, Cp)
    image (the STFT front-end reads the raw fp32 batch instead and keeps that)."""
    B, C, T = eeg_shape
    return B * C * T * 4 if eeg.raw_input else B * T * ops.cpad(C) * 2, fmri_numel * 4, B * 4 if grouped else 0, B * 4 if labelled else 0


class StepSchedule(NamedTuple):
    fmri_first: bool      # the fMRI branch is issued first in both passes (else the EEG chain)
    hand: bool            # the EEG chain hands its weight-gradient slot sums to the side stream
    handed_convs: int     # how many conv weight gradients (blocks 3, 2) go with the hand-over: 0 | 1 | 2
    eeg_live: bool        # the EEG encoder's backward is issued (it is not frozen)
    fmri_live: bool
    reduce_order: Tuple[Tuple[str, str], ...]   # (ready point, "side" | "main" stream) of the per-group all-reduces, in issue order


def step_schedule(eeg_kind: str, fmri_kind: str, frozen, fmri_shape, fused_rows: bool, env: Mapping[str, str]) -> StepSchedule:
    """``fmri_shape``: one sample's; ``fused_rows``: every saved transformer block takes mm_ffn_rows_bwd
    (`autograd.ffn_rows_bwd_fused`; it bears on ``handed_convs`` only); ``env``: the environment.
    The longer branch is issued FIRST.  The voxel branch outlasts the EEG chain from config #4's volumes on (64 x 64 x 48 =
    6 x the voxels of 32^3, 1.4 ms of kernels against 1.1 ms): its stream then takes no work from the chain and is issued
    first.  MM_FMRI_LONGER=0/1 overrides - not for a branch that cannot be the longer one (the tabular branch's two launches)."""
    eeg_live, fmri_live = "eeg_encoder" not in frozen, "fmri_encoder" not in frozen
    fmri_first = False
    if fmri_branch(fmri_kind).can_be_longer:
        forced = env.get("MM_FMRI_LONGER")
        fmri_first = forced == "1" if forced is not None else math.prod(fmri_shape) >= 4 * 32 ** 3
    # the transformer stack's weight-gradient slot sums and parameter reductions (~50 MB of reads) do not wait for the
    # end of the chain: they are handed to the side stream, which is idle once the fMRI branch is done - unless that
    # branch is the longer one: then nothing is handed over, the chain flushes its own sums, and the fMRI backward is
    # issued first  (a frozen EEG encoder hands nothing over)
    hand = not fmri_first and eeg_live
    # MM_CONV_WGRADS_HANDED: 1 = block 2's only (default: block 3's weight gradient stays on the chain), 2 = blocks 3
    # and 2 (round 2 / early round 3, when the chain was the later stream), 0 = none.  Which stream ends later
    # decides: 0.773-0.776 / 0.782-0.799 / 0.789-0.793 ms per step for 1 / 2 / 0 (profiles/r03_second_half_ab.txt).
    # With the blocks' row-wise backward in one launch (mm_ffn_rows_bwd) the chain is ~40 us shorter and the side
    # stream ends last: the default is then 0 (0.735-0.738 against 0.751-0.758 ms for 1, profiles/ffn_rows_bwd_ab.txt)
    fused = EEG_BRANCHES[eeg_kind].hands_over and eeg_live and fused_rows
    handed_convs = int(env.get("MM_CONV_WGRADS_HANDED", "0" if fused else "1")) if hand else 0
    if hand:    # the fMRI encoder's group after its backward, each handed group after its flush - all hidden beside the chain
        order = (("fmri", "side"), ("handed0", "side"), ("handed1", "side"), ("main", "main"))
    else:       # the chain's groups are final first; the fMRI encoder's goes out last
        order = (("handed0", "main"), ("handed1", "main"), ("main", "main"), ("fmri", "side"))
    return StepSchedule(fmri_first, hand, handed_convs, eeg_live, fmri_live, order)
