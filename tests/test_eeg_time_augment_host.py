"""CPU: the temporal EEG augmenter (`EEGTimeTransforms`, crossmodal_eeg_scr.py) - its numpy path and its
`draws` against an fp64 replica written HERE from the transform's rules (the stream primitives and the `EEGTransforms`
replica are those of tests/test_augment_host.py; nothing of the transform is imported from the package), the statistics of
its seven draws, every refusal, the header, and the trainer's host-side handling (checkpoint key, shared step index,
refusals).  tests/test_eeg_time_augment_kernels_gpu.py ties the kernel to the same replica."""
import numpy as np
import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer
from multimodal_eeg_fmri_amd.crossmodal_eeg_scr import EEGTimeTransforms, EEGTransforms
from test_augment_host import M32, M64, h, replica, stream_word, thresh

PURPOSE = {"shift_decision": 19, "shift_amount": 20, "scale_decision": 21, "scale_u": 22, "invert_decision": 23,
           "mask_decision": 24, "mask_start": 25}


# ---------------------------------------------------------------- the replica (fp64; from the rules of DESIGN.md 5u)
def time_stream_word(seed, step, rank, purpose):
    z = (seed * 0x9E3779B97F4A7C15 + step * 0xBF58476D1CE4E5B9 + rank * 0x94D049BB133111EB
         + (PURPOSE[purpose] + 1) * 0xD6E8FEB86659FD93) & M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z ^ (z >> 32)) & M32


def time_draws(B, T, *, p_shift, max_shift, p_scale, scale_range, p_invert, p_mask, mask_len, seed, step, rank=0):
    """-> dict(flags (B,) int, shift (B,), gain (B,) fp32, mask_start (B,), mask_len (B,)): the time plan's words"""
    s = {k: time_stream_word(seed, step, rank, k) for k in PURPOSE}
    b = np.arange(B)
    draw = lambda k: h(s[k], b)                                   # noqa: E731
    uniform = lambda k, n: ((draw(k) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)   # noqa: E731
    on = {k: draw(k + "_decision") < np.uint64(thresh(p)) for k, p in
          (("shift", p_shift), ("scale", p_scale), ("invert", p_invert), ("mask", p_mask))}
    shift = np.where(on["shift"], uniform("shift_amount", 2 * max_shift + 1) - max_shift, 0)
    factor = (1.0 + float(np.float32(scale_range)) * (draw("scale_u").astype(np.float64) * 2.0 ** -31 - 1.0)).astype(np.float32)
    factor = np.where(on["scale"], factor, np.float32(1.0))
    gain = np.where(on["invert"], -factor, factor).astype(np.float32)
    start = np.where(on["mask"], uniform("mask_start", T - mask_len + 1), 0)
    flags = on["shift"] * 1 + on["scale"] * 2 + on["invert"] * 4 + on["mask"] * 8
    return {"flags": flags, "on": on, "shift": shift, "gain": gain, "mask_start": start, "mask_len": np.where(on["mask"], mask_len, 0)}


def time_replica(x, *, base=None, step, rank=0, **time_kw):
    """x: (B, C, T) fp32 values; ``base``: the keywords of test_augment_host.replica without step / rank, or None ->
    the draws of `time_draws` plus out (B, C, T) fp64, noisy (B, C, T) bool (elements that took noise), noise (B, C, T)
    fp64 (z * noise_factor * std_b at the OUTPUT position; 0 where off) and std (B,)"""
    x = np.asarray(x, dtype=np.float64)
    B, C, T = x.shape
    d = time_draws(B, T, step=step, rank=rank, **time_kw)
    if base is None:
        noise, dropped, std = np.zeros_like(x), np.zeros((B, C), dtype=bool), np.zeros(B)
    else:
        r = replica(x, step=step, rank=rank, **base)
        noise, dropped, std = r["noise"], r["drop_mask"], r["std"]
    out, noisy = np.zeros_like(x), np.zeros(x.shape, dtype=bool)
    t = np.arange(T)
    for b in range(B):
        masked = (t >= d["mask_start"][b]) & (t < d["mask_start"][b] + d["mask_len"][b])           # rule 1
        ts = t - d["shift"][b]
        src = (ts >= 0) & (ts < T)                                                                  # rule 3
        live = ~masked[None, :] & ~dropped[b][:, None] & src[None, :]                               # rule 4 applies
        v = x[b][:, np.clip(ts, 0, T - 1)]
        if noise[b].any():                                        # (the sample's noise scale is non-zero; else -0.0 stays -0.0)
            v = v + noise[b]
        if d["on"]["scale"][b] or d["on"]["invert"][b]:
            v = v * float(d["gain"][b])
        out[b] = np.where(live, v, 0.0)
        noisy[b] = live & (noise[b] != 0)
    return dict(d, out=out, noisy=noisy, noise=noise, std=std)


def _x(shape, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) + offset


def _time_kw(aug, T):
    return dict(p_shift=aug.p_shift, max_shift=aug.max_shift, p_scale=aug.p_scale, scale_range=aug.scale_range,
                p_invert=aug.p_invert, p_mask=aug.p_mask, mask_len=max(1, int(aug.mask_fraction * T)), seed=aug.seed)


def _base_kw(base, C):
    return None if base is None else dict(p_noise=base.p_noise, p_drop=base.p_drop, noise_factor=base.noise_factor,
                                          n_drop=max(1, int(base.drop_fraction * C)), seed=base.seed)


# ---------------------------------------------------------------- API
def test_constructor_defaults_and_errors():
    a = EEGTimeTransforms()
    assert (a.p_shift, a.max_shift, a.p_scale, a.scale_range, a.p_invert, a.p_mask, a.mask_fraction, a.seed) == \
        (0.5, 16, 0.3, 0.1, 0.0, 0.3, 0.1, 0)
    assert a.params() == {"seed": 0, "p_shift": 0.5, "max_shift": 16, "p_scale": 0.3, "scale_range": 0.1, "p_invert": 0.0,
                          "p_mask": 0.3, "mask_fraction": 0.1}
    assert a.kernel_args(256)["mask_len"] == 25 and a.kernel_args(5)["mask_len"] == 1 and "mask_fraction" not in a.kernel_args(5)
    for kw in ({"p_shift": -0.1}, {"p_shift": 1.5}, {"p_scale": 2.0}, {"p_invert": -1.0}, {"p_mask": float("nan")}, {"p_mask": "0.3"},
               {"max_shift": -1}, {"max_shift": 1.5}, {"scale_range": -0.1}, {"scale_range": 1.0}, {"mask_fraction": 0.0},
               {"mask_fraction": 1.5}, {"mask_fraction": -0.2}):
        with pytest.raises(ValueError, match="EEGTimeTransforms"):
            EEGTimeTransforms(**kw)
    EEGTimeTransforms(p_shift=0, p_scale=1, p_invert=1.0, p_mask=0.0, max_shift=0, scale_range=0.0, mask_fraction=1.0)


def test_every_refusal_of_the_check():
    ok = dict(p_shift=0.5, max_shift=3, p_scale=0.3, scale_range=0.1, p_invert=0.0, p_mask=0.3, mask_len=2)
    ops.eeg_time_augment_check(2, 4, 8, **ok)
    for bad, msg in (({"p_shift": 1.5}, "p_shift"), ({"p_scale": -0.1}, "p_scale"), ({"p_invert": 2.0}, "p_invert"),
                     ({"p_mask": float("nan")}, "p_mask"), ({"max_shift": -1}, "max_shift"), ({"max_shift": 8}, "max_shift"),
                     ({"scale_range": 1.0}, "scale_range"), ({"scale_range": -0.5}, "scale_range"),
                     ({"mask_len": 0}, "masked window"), ({"mask_len": 9}, "masked window")):
        with pytest.raises(ValueError, match=msg):
            ops.eeg_time_augment_check(2, 4, 8, **dict(ok, **bad))
    # 5i's shape limits hold when an EEGTransforms rides along - and only then
    ops.eeg_time_augment_check(2, 1, 1, **dict(ok, max_shift=0, mask_len=1))
    with pytest.raises(ValueError, match="C \\* T >= 2"):
        ops.eeg_time_augment_check(2, 1, 1, n_drop=1, **dict(ok, max_shift=0, mask_len=1))
    with pytest.raises(ValueError, match="n_drop"):
        ops.eeg_time_augment_check(2, 4, 8, n_drop=5, **ok)
    with pytest.raises(ValueError, match="2\\^32"):
        ops.eeg_time_augment_check(1 << 20, 64, 128, n_drop=1, **ok)
    with pytest.raises(ValueError, match="B \\* C"):                # the kernel's 32-bit row index, also without an EEGTransforms
        ops.eeg_time_augment_check(1 << 16, 1 << 16, 8, **ok)
    # the CPU path refuses the same, before anything runs
    aug = EEGTimeTransforms(max_shift=8)
    with pytest.raises(ValueError, match="max_shift"):
        aug.batch(torch.zeros(2, 4, 8), 0)
    with pytest.raises(ValueError, match="C \\* T >= 2"):
        EEGTimeTransforms(max_shift=0).batch(torch.zeros(2, 1, 1), 0, base=EEGTransforms())
    with pytest.raises(ValueError, match="\\(B, C, T\\)"):
        aug.batch(torch.zeros(4, 8), 0)
    with pytest.raises(TypeError, match="EEGTransforms"):
        aug.batch(torch.zeros(2, 4, 32), 0, base=lambda t: t)
    # the shift is a gather: no overlap of source and fp32 output (refused on any device, before a launch)
    buf = torch.zeros(2 * 4 * 8 + 8)
    x, out = buf[:64].view(2, 4, 8), buf[8:72].view(2, 4, 8)
    for dst in (x, out):
        with pytest.raises(ValueError, match="overlap"):
            ops.eeg_time_augment_into(x, None, dst, time_args=EEGTimeTransforms(max_shift=3).kernel_args(8), step=0)


def test_header_declares_the_entry_point_and_the_abi_is_5():
    sigs = _hip.parse_header()
    # mm_stage_inputs_aug's arguments, then 4 probabilities / max_shift / scale_range / mask_len, 7 stream words, the time plan
    assert sigs["mm_stage_inputs_taug"] == "pplpp" + "iiii" + "fuu" + "fiffffi" + "uuuuuuu" + "p" + "ppl"
    assert sigs["mm_stage_inputs_aug"] == "pplpp" + "iiii" + "fuu" + "ppl"
    assert _hip.header_abi_version() == 5
    assert ops.EEG_TIME_AUG_PURPOSES == tuple(PURPOSE) and ops.EEG_TIME_AUG_FLAGS == ("shift", "scale", "invert", "mask")
    for seed, step, rank in ((0, 0, 0), (5, 3, 0), (21, 7, 3)):
        assert ops.eeg_time_augment_streams(seed, step, rank) == tuple(time_stream_word(seed, step, rank, k) for k in PURPOSE)
    # purposes of its own: no word shared with the EEG or the volume augmenter at equal (seed, step, rank)
    words = set(ops.eeg_time_augment_streams(5, 3, 0))
    assert len(words) == 7 and not words & set(ops.augment_streams(5, 3, 0)) and not words & set(ops.volume_augment_streams(5, 3, 0))


def test_call_counts_steps_and_state_dict_round_trips():
    x = _x((8, 32), 2)
    a = EEGTimeTransforms(p_shift=1.0, max_shift=4, p_scale=1.0, p_mask=1.0, seed=5)
    keep = x.clone()
    first = [a(x) for _ in range(3)]
    assert torch.equal(x, keep) and first[0].shape == x.shape and first[0].data_ptr() != x.data_ptr()
    assert not torch.equal(first[0], first[1]) and not torch.equal(first[1], first[2])
    assert a.state_dict() == {"seed": 5, "calls": 3}
    b = EEGTimeTransforms(p_shift=1.0, max_shift=4, p_scale=1.0, p_mask=1.0, seed=0)
    b.load_state_dict(a.state_dict())
    assert torch.equal(a(x), b(x)) and a.state_dict() == b.state_dict() == {"seed": 5, "calls": 4}
    assert torch.equal(a.batch(x[None], step=1)[0], first[1])                              # __call__ k == batch(step = k)
    with pytest.raises(ValueError):
        a(torch.zeros(8))


# ---------------------------------------------------------------- CPU path and draws against the replica
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 19, 37), (1, 33, 64)])
@pytest.mark.parametrize("p", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("with_base", [False, True])
def test_cpu_path_and_draws_equal_the_replica(shape, p, with_base):
    B, C, T = shape
    x = _x(shape, 100 + C, offset=3.0)
    x[0, 0, 0] = -0.0
    base = EEGTransforms(p=1.0 if p else 0.5, noise_factor=0.05, seed=21) if with_base else None
    for step, rank in ((0, 0), (7, 0), (7, 3)):
        aug = EEGTimeTransforms(p_shift=p, max_shift=min(5, T - 1), p_scale=p, scale_range=0.2, p_invert=p / 2, p_mask=p,
                                mask_fraction=0.25, seed=9)
        want = time_replica(x.numpy(), base=_base_kw(base, C), step=step, rank=rank, **_time_kw(aug, T))
        d = aug.draws(B, T, step, rank)
        flags = sum(d["flags"][k].astype(int) << i for i, k in enumerate(("shift", "scale", "invert", "mask")))
        assert np.array_equal(flags, want["flags"]) and np.array_equal(d["shift"], want["shift"])
        assert np.array_equal(d["gain"].view(np.int32), want["gain"].view(np.int32))
        assert np.array_equal(d["mask_start"], want["mask_start"]) and np.array_equal(d["mask_len"], want["mask_len"])
        got = aug.batch(x, step, rank, base=base).numpy()
        # without noise: the gather, the zeros (+0.0f) and the one fp32 product, bit for bit (the fp64 product of two fp32
        # values is exact, so its fp32 rounding is the fp32 product)
        quiet = ~want["noisy"]
        assert np.array_equal(got[quiet].view(np.int32), want["out"].astype(np.float32)[quiet].view(np.int32))
        # with noise: v = fp32(x + z * scale) carries half an ulp of v and the two roundings of the fp32 noise scale (2^-23 of
        # the noise term, as in test_augment_host.py); the gain multiplies that error, and its product rounds once more
        g = np.abs(want["gain"].astype(np.float64))[:, None, None]
        pre = np.where(g != 0, np.abs(want["out"]) / np.where(g != 0, g, 1), 0)
        tol = (g * (2.0 ** -24 * pre + 2.0 ** -23 * np.abs(want["noise"])) + 2.0 ** -24 * np.abs(want["out"])) * (1 + 2.0 ** -20)
        assert (np.abs(got.astype(np.float64) - want["out"]) <= tol).all()
        if with_base and p:                                       # (the base's p is 1 there)
            assert want["noisy"].any()
        if p == 0.0:
            assert not flags.any()
            if not with_base:
                assert np.array_equal(got.view(np.int32), x.numpy().view(np.int32))            # -0.0 included
        if p == 1.0:
            assert (flags & 0b1011 == 0b1011).all() and (want["mask_len"] == max(1, int(0.25 * T))).all()


def test_a_sample_without_a_source_takes_no_noise():
    """rule 3: the positions a shift uncovers are +0.0f exactly, also under noise of p = 1"""
    B, C, T = 8, 3, 16
    x = _x((B, C, T), 4, offset=8.0)
    aug = EEGTimeTransforms(p_shift=1.0, max_shift=6, p_scale=0.0, p_invert=1.0, p_mask=0.0, seed=2)
    y = aug.batch(x, 0, base=EEGTransforms(p_noise=1.0, p_drop=0.0, seed=2)).numpy()
    sh = aug.draws(B, T, 0)["shift"]
    assert (sh > 0).any() and (sh < 0).any()
    for b in range(B):
        gap = y[b][:, :sh[b]] if sh[b] > 0 else y[b][:, T + sh[b]:] if sh[b] < 0 else y[b][:, :0]
        assert (gap.view(np.int32) == 0).all()                                               # +0.0f, not -0.0f
        assert (y[b][:, max(sh[b], 0):T + min(sh[b], 0)] < 0).all()                          # inverted, x = 8 +- 1 and noise of 0.05 sigma


# ---------------------------------------------------------------- stream statistics (4096 samples, 5 standard errors)
N = 4096


def _corr(a, b):
    a, b = a.astype(float) - a.mean(), b.astype(float) - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_decision_rates_and_independence():
    ps = {"shift": 0.5, "scale": 0.3, "invert": 0.2, "mask": 0.4}
    aug = EEGTimeTransforms(p_shift=ps["shift"], max_shift=2, p_scale=ps["scale"], p_invert=ps["invert"], p_mask=ps["mask"],
                            mask_fraction=0.25, seed=0)
    f = aug.draws(N, 8, step=0)["flags"]
    for k, p in ps.items():
        print(k, f[k].mean())
        assert abs(f[k].mean() - p) <= 5 * np.sqrt(p * (1 - p) / N), k
    names = list(ps)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert abs(_corr(f[a], f[b])) <= 5 / np.sqrt(N), (a, b)
    # ... and from EEGTransforms' two decisions at equal seed and step (purposes 0 and 1)
    idx = np.arange(N)
    for purpose in ("noise_decision", "drop_decision"):
        other = h(stream_word(0, 0, 0, purpose), idx) < np.uint64(thresh(0.3))
        assert abs(other.mean() - 0.3) <= 5 * np.sqrt(0.21 / N)
        for k in names:
            assert abs(_corr(f[k], other)) <= 5 / np.sqrt(N), (k, purpose)


def test_shift_and_mask_start_are_uniform():
    aug = EEGTimeTransforms(p_shift=1.0, max_shift=2, p_scale=0.0, p_mask=1.0, mask_fraction=0.25, seed=0)
    d = aug.draws(N, 8, step=0)
    assert set(d["mask_len"].tolist()) == {2}
    for name, values, k in (("shift", d["shift"] + 2, 5), ("mask_start", d["mask_start"], 7)):
        share = np.bincount(values, minlength=k) / N
        print(name, share)
        assert len(share) == k and (np.abs(share - 1 / k) <= 5 * np.sqrt((1 / k) * (1 - 1 / k) / N)).all(), name
    assert abs(_corr(d["shift"], d["mask_start"])) <= 5 / np.sqrt(N)
    # off: shift, start and length read 0, the gain 1.0f (-1.0f when only the inversion is on)
    off = EEGTimeTransforms(p_shift=0.0, p_scale=0.0, p_invert=1.0, p_mask=0.0).draws(64, 8, step=0)
    assert not off["shift"].any() and not off["mask_start"].any() and not off["mask_len"].any()
    assert (off["gain"].view(np.int32) == np.float32(-1.0).view(np.int32)).all()
    assert (EEGTimeTransforms(p_shift=0.0, p_scale=0.0, p_mask=0.0).draws(64, 8, step=0)["gain"] == 1.0).all()


# ---------------------------------------------------------------- the trainer's host side
def _trainer(seed=0, **kw):
    torch.manual_seed(seed)
    return BridgeTrainer(eeg_channels=8, device="cpu", mode="manual", **kw)


def test_checkpoint_carries_the_augmenter_only_when_there_is_one():
    plain = _trainer().checkpoint_state()
    assert "eeg_time_augment" not in plain["bridge_trainer_state"]
    mk = lambda: EEGTimeTransforms(p_shift=0.4, max_shift=7, p_invert=0.1, mask_fraction=0.2, seed=17)   # noqa: E731
    tr = _trainer(eeg_time_augment=mk())
    ck = tr.checkpoint_state()
    assert ck["bridge_trainer_state"]["eeg_time_augment"] == {"seed": 17, "step": 0, "p_shift": 0.4, "max_shift": 7, "p_scale": 0.3,
                                                              "scale_range": 0.1, "p_invert": 0.1, "p_mask": 0.3, "mask_fraction": 0.2}
    assert set(ck["bridge_trainer_state"]) == set(plain["bridge_trainer_state"]) | {"eeg_time_augment"}
    assert ck["bridge_trainer_state"]["format"] == plain["bridge_trainer_state"]["format"] == 1
    ck["bridge_trainer_state"]["eeg_time_augment"]["step"] = 41
    other = _trainer(seed=3, eeg_time_augment=mk())
    other.load_checkpoint_state(ck)
    assert other.augment_step == 41 and other.checkpoint_state()["bridge_trainer_state"]["eeg_time_augment"]["step"] == 41
    assert torch.equal(other.bucket.p, tr.bucket.p)
    # both augmenters share the step index
    both = _trainer(augment=EEGTransforms(seed=1), eeg_time_augment=mk()).checkpoint_state()["bridge_trainer_state"]
    assert both["augment"]["step"] == both["eeg_time_augment"]["step"] == 0
    ck2 = _trainer(augment=EEGTransforms(seed=1), eeg_time_augment=mk()).checkpoint_state()
    ck2["bridge_trainer_state"]["augment"]["step"] = 3            # (a damaged file: the shared index disagrees with itself)
    with pytest.raises(ValueError, match="share one step index"):
        _trainer(seed=3, augment=EEGTransforms(seed=1), eeg_time_augment=mk()).load_checkpoint_state(ck2)
    with pytest.raises(TypeError, match="EEGTimeTransforms"):
        _trainer(eeg_time_augment=EEGTransforms())
    with pytest.raises(TypeError, match="EEGTransforms"):
        _trainer(augment=EEGTimeTransforms())


def test_checkpoint_of_another_augmenter_is_refused_before_anything_is_touched():
    with_aug = _trainer(eeg_time_augment=EEGTimeTransforms(seed=1)).checkpoint_state()
    without = _trainer().checkpoint_state()
    cases = [(_trainer(seed=3), with_aug), (_trainer(seed=3, eeg_time_augment=EEGTimeTransforms(seed=1)), without)]
    cases += [(_trainer(seed=3, eeg_time_augment=EEGTimeTransforms(**kw)), with_aug) for kw in
              ({"seed": 2}, {"seed": 1, "p_shift": 0.4}, {"seed": 1, "max_shift": 8}, {"seed": 1, "scale_range": 0.2},
               {"seed": 1, "p_invert": 0.5}, {"seed": 1, "mask_fraction": 0.2})]
    for tr, ck in cases:
        before = [t.clone() for t in (tr.bucket.p, tr.bucket.m, tr.bucket.v, tr.bucket.state)]
        with pytest.raises(ValueError, match="eeg_time_augment differs"):
            tr.load_checkpoint_state(ck)
        assert all(torch.equal(a, b) for a, b in zip(before, (tr.bucket.p, tr.bucket.m, tr.bucket.v, tr.bucket.state)))
        assert tr.augment_step == 0
    _trainer(seed=3).load_checkpoint_state(without)                # an old (augmenter-free) checkpoint loads as before


def test_packed_host_path_refuses_the_trainer():
    tr = _trainer(eeg_time_augment=EEGTimeTransforms(seed=1))
    eeg, fmri = torch.randn(2, 8, 64), torch.randn(2, 1, 16, 16, 16)
    for call in (lambda: tr.pack_host_batch(eeg, fmri), lambda: tr.train_step_packed(torch.zeros(8, dtype=torch.uint8)),
                 lambda: tr.host_feeder()):
        with pytest.raises(ValueError, match="temporal EEG augmenter"):
            call()
