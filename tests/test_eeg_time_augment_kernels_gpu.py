"""GPU: the temporal EEG augmentation kernel (csrc/augment.hip: mm_stage_inputs_taug, through `ops.eeg_time_augment` and by
name) against the fp64 replica of tests/test_eeg_time_augment_host.py: the per-sample draws, the gather, the zeros and the
single fp32 product bit for bit, the noise to the bound of tests/test_augment_kernels_gpu.py, the packed operand and the
all-zero-probability outputs bit for bit against the existing kernels."""
import numpy as np
import pytest
import torch

from multimodal_eeg_fmri_amd.crossmodal_eeg_scr import EEGTimeTransforms, EEGTransforms
from test_augment_kernels_gpu import CAP, NF, NOISE_BOUND, SHAPES, _batch
from test_eeg_time_augment_host import _base_kw, _time_kw, time_replica
from test_kernels_gpu import _hip

pytestmark = pytest.mark.gpu

MAX_SHIFT = {(1, 5, 7): 3, (3, 19, 37): 33, (2, 33, 64): 5, (2, 64, 160): 40}
SEED, STEP, RANK = 5, 3, 0
TIME_PS = {"p0": (0.0, 0.0, 0.0, 0.0), "p1": (1.0, 1.0, 1.0, 1.0), "mixed": (0.5, 0.5, 0.5, 0.5)}


def _aug(shape, ps):
    return EEGTimeTransforms(p_shift=ps[0], max_shift=MAX_SHIFT[shape], p_scale=ps[1], scale_range=0.1, p_invert=ps[2], p_mask=ps[3],
                             mask_fraction=0.25, seed=SEED)


def _base():
    return EEGTransforms(p=1.0, noise_factor=NF, seed=SEED)


def _check(shape, aug, base, step, rank=RANK):
    """one launch (two with ``base``) against the replica; -> the replica's dict"""
    from multimodal_eeg_fmri_amd import ops
    hip = _hip()
    B, C, T = shape
    x = _batch(B, C, T)
    (out, xb), plan = ops.eeg_time_augment(x.cuda(), time_args=aug.kernel_args(T), base_args=None if base is None else base.kernel_args(C),
                                           step=step, rank=rank, packed=True, return_plan=True)
    want = time_replica(x.numpy(), base=_base_kw(base, C), step=step, rank=rank, **_time_kw(aug, T))
    # the draws: flags, s_b, the bits of g_b, the window
    flags = sum(plan["flags"][k].cpu().numpy().astype(int) << i for i, k in enumerate(("shift", "scale", "invert", "mask")))
    assert np.array_equal(flags, want["flags"]) and np.array_equal(plan["shift"].cpu().numpy(), want["shift"])
    assert np.array_equal(plan["gain"].cpu().numpy().view(np.int32), want["gain"].view(np.int32))
    assert np.array_equal(plan["mask_start"].cpu().numpy(), want["mask_start"])
    assert np.array_equal(plan["mask_len"].cpu().numpy(), want["mask_len"])
    got = out.cpu().numpy()
    # without noise: the gather, the zeros as +0.0f, the single fp32 product - bit for bit
    quiet = ~want["noisy"]
    assert np.array_equal(got[quiet].view(np.int32), want["out"].astype(np.float32)[quiet].view(np.int32))
    # with noise: the existing kernel's bound on the noise term, scaled by the gain, plus the one more rounding of the product
    unit = (float(np.float32(NF)) * want["std"] * np.abs(want["gain"].astype(np.float64)))[:, None, None]
    bound = NOISE_BOUND * unit + 2.0 ** -23 * np.abs(want["out"])
    err = np.abs(got.astype(np.float64) - want["out"])
    if want["noisy"].any():
        worst = float((err / bound)[want["noisy"]].max())
        in_units = float((err / np.broadcast_to(unit, err.shape))[want["noisy"]].max())
        print(f"taug {shape} step {step}: max err / bound {worst:.3f}, max bound {bound[want['noisy']].max():.3e}, "
              f"max err {in_units:.3e} (units of noise_factor * std * |g|)")
        assert bound[want["noisy"]].max() <= CAP
        assert (err[want["noisy"]] <= bound[want["noisy"]]).all()
        assert (got[want["noisy"]] != (want["out"] - want["noise"] * want["gain"][:, None, None]).astype(np.float32)[want["noisy"]]).any()
    # packed == mm_pack_nct_bf16(fp32 output), padding channels zero included
    cp = ops.cpad(C)
    ref = torch.full((B, T, cp), float("nan"), dtype=torch.bfloat16, device="cuda")
    hip.call("mm_pack_nct_bf16", out, ref, B, C, T, cp)
    assert xb.shape == (B, T, cp) and torch.equal(xb.view(torch.int16), ref.view(torch.int16))
    assert (xb[:, :, C:] == 0).all()
    if base is not None:
        noise_on, mask, _ = plan["base"]
        assert noise_on.all() and (mask.sum(dim=1) == max(1, int(0.1 * C))).all()
    return want


@pytest.mark.parametrize("with_base", [False, True], ids=["time only", "with EEGTransforms"])
@pytest.mark.parametrize("ps", list(TIME_PS))
@pytest.mark.parametrize("shape", SHAPES)
def test_it_matches_the_replica_and_the_packed_operand_is_the_pack_of_the_output(shape, ps, with_base):
    want = _check(shape, _aug(shape, TIME_PS[ps]), _base() if with_base else None, STEP)
    if ps == "p0":
        assert not want["flags"].any() and (want["gain"] == 1.0).all()
    if ps == "p1":
        assert (want["flags"] == 15).all() and (want["mask_len"] == max(1, int(0.25 * shape[2]))).all()


def _coverage(shape):
    """{case: first step in 0..63 at seed 5, rank 0, all probabilities 1 whose draws (on the host) contain it}"""
    B, C, T = shape
    aug = _aug(shape, TIME_PS["p1"])
    L = aug.mask_len(T)
    cases = {"an odd positive shift": lambda d: ((d["shift"] > 0) & (d["shift"] % 2 == 1)).any(),
             "an odd negative shift": lambda d: ((d["shift"] < 0) & (d["shift"] % 2 == 1)).any(),
             "an even non-zero shift": lambda d: ((d["shift"] != 0) & (d["shift"] % 2 == 0)).any(),
             "a shift of 0": lambda d: (d["shift"] == 0).any(),
             "a mask starting at an odd t": lambda d: (d["mask_start"] % 2 == 1).any(),
             "a mask starting at 0": lambda d: (d["mask_start"] == 0).any()}
    if MAX_SHIFT[shape] >= 32:
        cases["|s_b| >= 32"] = lambda d: (np.abs(d["shift"]) >= 32).any()
    if T > 32:
        cases["a mask straddling a multiple of 32"] = lambda d: (d["mask_start"] // 32 != (d["mask_start"] + L - 1) // 32).any()
    found = {}
    for step in range(64):
        d = aug.draws(B, T, step, RANK)
        for name, hit in cases.items():
            if name not in found and hit(d):
                found[name] = step
    return aug, cases, found


@pytest.mark.parametrize("shape", SHAPES)
def test_coverage_of_shift_parities_long_shifts_and_mask_positions(shape):
    aug, cases, found = _coverage(shape)
    print(shape, found)
    assert set(found) == set(cases), set(cases) - set(found)
    assert max(found.values()) <= 23, found
    for step in sorted(set(found.values())):
        _check(shape, aug, _base(), step)


def _taug(hip, x, plan, words, xb, out, cp, sg, tk, ts, tp, fdst, fsrc, nf=NF):
    B, C, T = x.shape
    hip.call("mm_stage_inputs_taug", x, plan, words, xb, out, B, C, T, cp, nf, sg[0], sg[1], tk["p_shift"], tk["max_shift"],
             tk["p_scale"], tk["scale_range"], tk["p_invert"], tk["p_mask"], tk["mask_len"], *ts, tp, fdst, fsrc,
             0 if fsrc is None else fsrc.numel())


@pytest.mark.parametrize("B,C,T", SHAPES)
def test_time_probabilities_0_equal_the_existing_kernels_and_outputs_are_optional(B, C, T):
    """by name: with a plan the outputs are mm_stage_inputs_aug's, without one mm_stage_inputs' - bit for bit, fMRI copy included"""
    from multimodal_eeg_fmri_amd import ops
    hip = _hip()
    x = _batch(B, C, T).cuda()
    g = torch.Generator().manual_seed(7)
    fmri = torch.randn(B, 1, 8, 8, 12, generator=g).cuda()
    cp = ops.cpad(C)
    nan_bf = lambda: torch.full((B, T, cp), float("nan"), dtype=torch.bfloat16, device="cuda")   # noqa: E731
    nan_like = lambda t: torch.full_like(t, float("nan"))                                        # noqa: E731
    tk = _aug((B, C, T), TIME_PS["p0"]).kernel_args(T)
    ts = ops.eeg_time_augment_streams(SEED, STEP, RANK)
    s = ops.augment_streams(SEED, STEP, RANK)
    words, _, _ = ops.eeg_augment_plan_layout(B, C, T)
    plan = torch.empty(words, dtype=torch.int32, device="cuda")
    # with a plan (noise and drops of p = 1)
    hip.call("mm_eeg_augment_plan", x, plan, words, B, C, T, 1.0, 1.0, max(1, int(0.1 * C)), s[0], s[1], s[2])
    xb0, e0, f0 = nan_bf(), nan_like(x), nan_like(fmri)
    hip.call("mm_stage_inputs_aug", x, plan, words, xb0, e0, B, C, T, cp, NF, s[3], s[4], f0, fmri, fmri.numel())
    assert not torch.equal(e0, x)
    xb1, e1, f1 = nan_bf(), nan_like(x), nan_like(fmri)
    tp = torch.full((B, 8), -1, dtype=torch.int32, device="cuda")
    _taug(hip, x, plan, words, xb1, e1, cp, s[3:], tk, ts, tp, f1, fmri)
    assert torch.equal(xb1.view(torch.int16), xb0.view(torch.int16)) and torch.equal(e1.view(torch.int32), e0.view(torch.int32))
    assert torch.equal(f1, fmri) and torch.equal(f0, fmri)
    one = int(np.float32(1.0).view(np.int32))
    assert tp.tolist() == [[0, 0, one, 0, 0, 0, 0, 0]] * B
    # either output alone, no fMRI copy, no time plan: the same bits
    xb2, e2 = nan_bf(), nan_like(x)
    _taug(hip, x, plan, words, xb2, None, cp, s[3:], tk, ts, None, None, None)
    _taug(hip, x, plan, words, None, e2, cp, s[3:], tk, ts, None, None, None)
    assert torch.equal(xb2.view(torch.int16), xb0.view(torch.int16)) and torch.equal(e2.view(torch.int32), e0.view(torch.int32))
    # without a plan: mm_stage_inputs / mm_pack_nct_bf16
    xb3, e3, f3 = nan_bf(), nan_like(x), nan_like(fmri)
    hip.call("mm_stage_inputs", x, xb3, e3, B, C, T, cp, f3, fmri, fmri.numel())
    xb4, e4, f4 = nan_bf(), nan_like(x), nan_like(fmri)
    _taug(hip, x, None, 0, xb4, e4, cp, (0, 0), tk, ts, None, f4, fmri, nf=0.0)
    assert torch.equal(xb4.view(torch.int16), xb3.view(torch.int16)) and torch.equal(e4.view(torch.int32), x.view(torch.int32))
    assert torch.equal(e3.view(torch.int32), x.view(torch.int32)) and torch.equal(f4, fmri)
    xb5 = nan_bf()
    hip.call("mm_pack_nct_bf16", x, xb5, B, C, T, cp)
    assert torch.equal(xb4.view(torch.int16), xb5.view(torch.int16))


def test_runs_are_bit_identical_and_step_and_rank_matter():
    from multimodal_eeg_fmri_amd import ops
    shape = (3, 19, 37)
    B, C, T = shape
    x = _batch(B, C, T).cuda()
    aug, base = _aug(shape, TIME_PS["p1"]), _base()
    kw = dict(time_args=aug.kernel_args(T), base_args=base.kernel_args(C))
    a, pa = ops.eeg_time_augment(x, step=STEP, rank=RANK, return_plan=True, **kw)
    b, pb = ops.eeg_time_augment(x, step=STEP, rank=RANK, return_plan=True, **kw)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert all(torch.equal(pa[k], pb[k]) for k in ("shift", "gain", "mask_start", "mask_len"))
    other_step, ps = ops.eeg_time_augment(x, step=STEP + 1, rank=RANK, return_plan=True, **kw)
    other_rank, pr = ops.eeg_time_augment(x, step=STEP, rank=RANK + 1, return_plan=True, **kw)
    assert not torch.equal(a, other_step) and not torch.equal(a, other_rank) and not torch.equal(other_step, other_rank)
    assert not torch.equal(pa["gain"], ps["gain"]) and not torch.equal(pa["gain"], pr["gain"])
    # the EEGTimeTransforms front door runs the same launches; its `draws` are the plan
    assert torch.equal(aug.batch(x, STEP, RANK, base=base), a)
    d = aug.draws(B, T, STEP, RANK)
    assert np.array_equal(d["shift"], pa["shift"].cpu().numpy()) and np.array_equal(d["gain"], pa["gain"].cpu().numpy())
    # without noise the CPU path is the kernel's bits: a gather, zeros and one fp32 product
    alone = aug.batch(x, STEP, RANK)
    assert torch.equal(aug.batch(x.cpu(), STEP, RANK).view(torch.int32), alone.cpu().view(torch.int32))
    assert not torch.equal(alone, x)


def test_error_paths():
    from multimodal_eeg_fmri_amd import ops
    hip = _hip()
    B, C, T = 2, 4, 8
    x = torch.randn(B, C, T, device="cuda")
    xb = torch.empty(B, T, 16, dtype=torch.bfloat16, device="cuda")
    ok = dict(p_shift=0.5, max_shift=3, p_scale=0.3, scale_range=0.1, p_invert=0.0, p_mask=0.3, mask_len=2)
    ts = (1, 2, 3, 4, 5, 6, 7)
    _taug(hip, x, None, 0, xb, None, 16, (0, 0), ok, ts, None, None, None)
    for bad, msg in (({"p_shift": 1.5}, "probabilities"), ({"p_scale": -0.5}, "probabilities"), ({"p_invert": 2.0}, "probabilities"),
                     ({"p_mask": float("nan")}, "probabilities"), ({"max_shift": -1}, "max_shift"), ({"max_shift": T}, "max_shift"),
                     ({"scale_range": 1.0}, "scale_range"), ({"scale_range": -0.1}, "scale_range"),
                     ({"mask_len": 0}, "mask length"), ({"mask_len": T + 1}, "mask length")):
        with pytest.raises(hip.HipLibraryError, match=msg):
            _taug(hip, x, None, 0, xb, None, 16, (0, 0), dict(ok, **bad), ts, None, None, None)
    # source and fp32 output overlapping: in place, and a shifted view of one buffer
    buf = torch.zeros(B * C * T + 8, device="cuda")
    src, dst = buf[:B * C * T].view(B, C, T), buf[8:].view(B, C, T)
    for s_, d_ in ((x, x), (src, dst), (dst, src)):
        with pytest.raises(hip.HipLibraryError, match="overlap"):
            _taug(hip, s_, None, 0, None, d_, 16, (0, 0), ok, ts, None, None, None)
        with pytest.raises(ValueError, match="overlap"):
            ops.eeg_time_augment_into(s_, None, d_, time_args=dict(ok, seed=0), step=0)
    with pytest.raises(hip.HipLibraryError, match="at least one output"):
        _taug(hip, x, None, 0, None, None, 16, (0, 0), ok, ts, None, None, None)
    with pytest.raises(hip.HipLibraryError, match="Cp"):
        _taug(hip, x, None, 0, xb, None, 3, (0, 0), ok, ts, None, None, None)
    fmri = torch.randn(2 * 8 * 8 * 12 + 4, device="cuda")
    fdst = torch.empty_like(fmri)
    with pytest.raises(hip.HipLibraryError, match="fMRI copy needs"):
        _taug(hip, x, None, 0, xb, None, 16, (0, 0), ok, ts, None, fdst[1:], fmri[1:])
    # with a plan: mm_stage_inputs_aug's refusals
    words, _, _ = ops.eeg_augment_plan_layout(B, C, T)
    plan = torch.zeros(words, dtype=torch.int32, device="cuda")
    with pytest.raises(hip.HipLibraryError, match="plan needs"):
        _taug(hip, x, plan, words - 1, xb, None, 16, (4, 5), ok, ts, None, None, None)
    one = torch.zeros(2, 1, 1, device="cuda")
    tiny = dict(ok, max_shift=0, mask_len=1)
    with pytest.raises(hip.HipLibraryError, match="C \\* T >= 2"):
        _taug(hip, one, plan, words, None, torch.empty_like(one), 16, (4, 5), tiny, ts, None, None, None)
    _taug(hip, one, None, 0, None, torch.empty_like(one), 16, (0, 0), tiny, ts, None, None, None)    # (no such limit without a plan)
    # the host surface refuses before any launch
    with pytest.raises(ValueError, match="max_shift"):
        EEGTimeTransforms(max_shift=T).batch(x, 0)
    with pytest.raises(ValueError, match="C \\* T >= 2"):
        EEGTimeTransforms(max_shift=0).batch(one, 0, base=EEGTransforms())
