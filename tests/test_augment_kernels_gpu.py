"""GPU: the EEG augmentation kernels (csrc/augment.hip: mm_eeg_augment_plan + mm_stage_inputs_aug, through
`ops.eeg_augment` and by name) against the fp64 replica of the random stream in tests/test_augment_host.py: decisions and
dropped channels exactly, the standard deviation and the noise to measured-and-capped bounds, the packed operand and the
p = 0 outputs bit for bit against the existing packers."""
import numpy as np
import pytest
import torch

from test_augment_host import replica, stream_word
from test_kernels_gpu import _hip

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5, 7), (3, 19, 37), (2, 33, 64), (2, 64, 160)]
PS = [0.0, 0.3, 1.0]
NF, SEED, STEP, RANK = 0.05, 5, 3, 0

# Errors against the fp64 replica, measured on an MI355X as the maximum over SHAPES x PS (this file's inputs):
#   relative error of std_b                                               MEASURED_STD = 4.4e-8
#   |noise term - replica's| in units of noise_factor * std_b             MEASURED_NOISE = 9.9e-6
# (worst cases 4.364e-8 at (1, 5, 7) and 9.830e-6 at (3, 19, 37), p = 1; the first is fp32 rounding of std_b, the second
# the fp32 rounding of out = x + noise at |x| in [8, 16) sigma: 2^-21 / 0.05 = 9.5e-6).  The test bounds
# are 4 x the measured maxima (margin for shapes not in the list) and may not exceed 2^-9: beyond that the error would move
# the bf16 operand.
MEASURED_STD, MEASURED_NOISE = 4.4e-8, 9.9e-6
STD_BOUND, NOISE_BOUND = 4 * MEASURED_STD, 4 * MEASURED_NOISE
CAP = 2.0 ** -9


def _batch(B, C, T):
    """fp32 samples with unit spread and a mean offset of up to 8 sigma (the last sample's)"""
    g = torch.Generator().manual_seed(1000 * B + 10 * C + T)
    x = torch.randn(B, C, T, generator=g)
    return x + 8.0 * torch.arange(1, B + 1).view(B, 1, 1) / B


def _kw(C, p, step=STEP, rank=RANK):
    return dict(p_noise=p, p_drop=p, noise_factor=NF, n_drop=max(1, int(0.1 * C)), seed=SEED, step=step, rank=rank)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("B,C,T", SHAPES)
def test_augment_matches_the_replica(B, C, T, p):
    from multimodal_eeg_fmri_amd import ops
    hip = _hip()
    x = _batch(B, C, T)
    xg = x.cuda()
    (out, xb), (noise_on, mask, std) = ops.eeg_augment(xg, packed=True, return_plan=True, **_kw(C, p))
    want = replica(x.numpy(), **_kw(C, p))
    out_c, noise_on, mask, std = out.cpu().numpy(), noise_on.cpu().numpy(), mask.cpu().numpy(), std.cpu().numpy()
    # exact: decisions, dropped channels, untouched samples
    assert np.array_equal(noise_on, want["noise_on"]) and np.array_equal(mask, want["drop_mask"])
    assert mask.shape == (B, C) and (out_c[mask] == 0).all()
    assert np.array_equal(np.signbit(out_c[mask]), np.zeros_like(out_c[mask], dtype=bool))        # +0.0f
    idle = ~noise_on & ~mask.any(axis=1)
    assert np.array_equal(out_c[idle].view(np.int32), x.numpy()[idle].view(np.int32))
    assert np.array_equal(out_c[~noise_on][~mask[~noise_on]].view(np.int32), x.numpy()[~noise_on][~mask[~noise_on]].view(np.int32))
    if p == 1.0:
        assert noise_on.all() and (mask.sum(axis=1) == max(1, int(0.1 * C))).all()
    if p == 0.0:
        assert not noise_on.any() and not mask.any()
    # packed == mm_pack_nct_bf16(fp32 output), padding channels zero included
    cp = ops.cpad(C)
    ref = torch.full((B, T, cp), float("nan"), dtype=torch.bfloat16, device="cuda")
    hip.call("mm_pack_nct_bf16", out, ref, B, C, T, cp)
    assert xb.shape == (B, T, cp) and torch.equal(xb.view(torch.int16), ref.view(torch.int16))
    assert (xb[:, :, C:] == 0).all()
    # tolerance: the standard deviation and the noise term
    std_err = float(np.max(np.abs(std.astype(np.float64) - want["std"]) / want["std"]))
    keep = noise_on[:, None] & ~mask
    unit = (float(np.float32(NF)) * want["std"])[:, None, None]
    err = np.abs((out_c.astype(np.float64) - x.numpy().astype(np.float64)) - want["noise"]) / unit
    noise_err = float(err[keep].max()) if keep.any() else 0.0
    print(f"augment ({B}, {C}, {T}) p = {p}: std rel err {std_err:.3e}, noise err {noise_err:.3e} (units of noise_factor * std)")
    assert STD_BOUND <= CAP and NOISE_BOUND <= CAP
    assert std_err <= STD_BOUND and noise_err <= NOISE_BOUND
    if keep.any():
        assert np.abs(out_c[keep] - x.numpy()[keep]).max() > 0  # (noise was really added where it is on)


@pytest.mark.parametrize("B,C,T", SHAPES)
def test_p0_equals_stage_inputs_and_outputs_are_optional(B, C, T):
    """by name: p = 0 gives mm_stage_inputs' three outputs bit for bit; either EEG output, and the fMRI copy, may be absent"""
    from multimodal_eeg_fmri_amd import ops
    hip = _hip()
    x = _batch(B, C, T).cuda()
    g = torch.Generator().manual_seed(7)
    fmri = torch.randn(B, 1, 8, 8, 12, generator=g).cuda()
    cp = ops.cpad(C)
    nan_bf = lambda: torch.full((B, T, cp), float("nan"), dtype=torch.bfloat16, device="cuda")   # noqa: E731
    xb0, e0, f0 = nan_bf(), torch.full_like(x, float("nan")), torch.full_like(fmri, float("nan"))
    hip.call("mm_stage_inputs", x, xb0, e0, B, C, T, cp, f0, fmri, fmri.numel())
    words, _, _ = ops.eeg_augment_plan_layout(B, C, T)
    plan = torch.empty(words, dtype=torch.int32, device="cuda")
    s = [stream_word(SEED, STEP, RANK, k) for k in ("noise_decision", "drop_decision", "channel_keys", "gauss_a", "gauss_b")]
    assert tuple(s) == ops.augment_streams(SEED, STEP, RANK)
    n_drop = max(1, int(0.1 * C))

    def run(p, xb, e, f):
        hip.call("mm_eeg_augment_plan", x, plan, words, B, C, T, p, p, n_drop, s[0], s[1], s[2])
        hip.call("mm_stage_inputs_aug", x, plan, words, xb, e, B, C, T, cp, NF, s[3], s[4], f, None if f is None else fmri,
                 0 if f is None else fmri.numel())
    xb1, e1, f1 = nan_bf(), torch.full_like(x, float("nan")), torch.full_like(fmri, float("nan"))
    run(0.0, xb1, e1, f1)
    assert torch.equal(xb1.view(torch.int16), xb0.view(torch.int16))
    assert torch.equal(e1.view(torch.int32), e0.view(torch.int32)) and torch.equal(f1, fmri)
    # p = 1 with every combination of outputs: the same bits wherever an output exists
    xb2, e2, f2 = nan_bf(), torch.full_like(x, float("nan")), torch.full_like(fmri, float("nan"))
    run(1.0, xb2, e2, f2)
    assert not torch.equal(e2, x) and torch.equal(f2, fmri)
    xb3, e3 = nan_bf(), torch.full_like(x, float("nan"))
    run(1.0, xb3, None, None)
    run(1.0, None, e3, None)
    assert torch.equal(xb3.view(torch.int16), xb2.view(torch.int16)) and torch.equal(e3.view(torch.int32), e2.view(torch.int32))


def test_runs_are_bit_identical_and_step_and_rank_matter():
    from multimodal_eeg_fmri_amd import ops
    B, C, T = 3, 19, 37
    x = _batch(B, C, T).cuda()
    a, pa = ops.eeg_augment(x, return_plan=True, **_kw(C, 1.0))
    b, pb = ops.eeg_augment(x, return_plan=True, **_kw(C, 1.0))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and all(torch.equal(u, v) for u, v in zip(pa, pb))
    other_step = ops.eeg_augment(x, **_kw(C, 1.0, step=STEP + 1))
    other_rank = ops.eeg_augment(x, **_kw(C, 1.0, rank=RANK + 1))
    assert not torch.equal(a, other_step) and not torch.equal(a, other_rank) and not torch.equal(other_step, other_rank)
    # the EEGTransforms front door runs the same launches
    from multimodal_eeg_fmri_amd.crossmodal_eeg_scr import EEGTransforms
    aug = EEGTransforms(p=1.0, noise_factor=NF, seed=SEED)
    assert torch.equal(aug.batch(x, STEP, RANK), a)
    # ... and its CPU path draws the same stream: same dropped channels; each path is within NOISE_BOUND of the replica
    cpu = aug.batch(x.cpu(), STEP, RANK)
    assert torch.equal((cpu == 0).all(dim=2), (a.cpu() == 0).all(dim=2))
    unit = NF * x.cpu().double().reshape(B, -1).std(dim=1).view(B, 1, 1)
    assert ((cpu.double() - a.cpu().double()).abs() / unit).max().item() <= 2 * NOISE_BOUND


def test_error_paths():
    from multimodal_eeg_fmri_amd import ops
    hip = _hip()
    with pytest.raises(ValueError, match="C \\* T >= 2"):
        ops.eeg_augment(torch.zeros(2, 1, 1, device="cuda"), **_kw(1, 0.3))
    with pytest.raises(ValueError, match="n_drop"):
        ops.eeg_augment(torch.zeros(2, 4, 8, device="cuda"), **dict(_kw(4, 0.3), n_drop=5))
    x = torch.zeros(2, 1, 1, device="cuda")
    plan = torch.zeros(64, dtype=torch.int32, device="cuda")
    with pytest.raises(hip.HipLibraryError, match="C \\* T >= 2"):
        hip.call("mm_eeg_augment_plan", x, plan, 64, 2, 1, 1, 0.3, 0.3, 1, 1, 2, 3)
    with pytest.raises(hip.HipLibraryError, match="C \\* T >= 2"):
        hip.call("mm_stage_inputs_aug", x, plan, 64, None, torch.empty_like(x), 2, 1, 1, 16, NF, 4, 5, None, None, 0)
    B, C, T = 2, 4, 8
    x = torch.randn(B, C, T, device="cuda")
    words, _, _ = ops.eeg_augment_plan_layout(B, C, T)
    plan = torch.zeros(words, dtype=torch.int32, device="cuda")
    with pytest.raises(hip.HipLibraryError, match="plan needs"):
        hip.call("mm_eeg_augment_plan", x, plan, words - 1, B, C, T, 0.3, 0.3, 1, 1, 2, 3)
    with pytest.raises(hip.HipLibraryError, match="probabilities"):
        hip.call("mm_eeg_augment_plan", x, plan, words, B, C, T, 1.5, 0.3, 1, 1, 2, 3)
    hip.call("mm_eeg_augment_plan", x, plan, words, B, C, T, 0.3, 0.3, 1, 1, 2, 3)
    xb = torch.empty(B, T, 16, dtype=torch.bfloat16, device="cuda")
    fmri = torch.randn(2 * 8 * 8 * 12 + 4, device="cuda")
    dst = torch.empty_like(fmri)
    n = 2 * 8 * 8 * 12
    for d, s, k in ((dst, fmri, n - 2), (dst[1:], fmri, n), (dst, fmri[1:], n), (dst, None, n), (dst, fmri, 0)):
        with pytest.raises(hip.HipLibraryError, match="fMRI copy needs"):
            hip.call("mm_stage_inputs_aug", x, plan, words, xb, None, B, C, T, 16, NF, 4, 5, d, s, k)
    with pytest.raises(hip.HipLibraryError, match="at least one output"):
        hip.call("mm_stage_inputs_aug", x, plan, words, None, None, B, C, T, 16, NF, 4, 5, None, None, 0)
    with pytest.raises(hip.HipLibraryError, match="at least one output"):
        hip.call("mm_stage_inputs_aug", x, plan, words, None, x, B, C, T, 16, NF, 4, 5, None, None, 0)      # in place
