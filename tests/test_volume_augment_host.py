"""CPU: the fMRI volume augmenter (`VolumeTransforms`, fmri_utils.py) - its numpy path against an fp64 replica written HERE
from the transform's definition (only h(stream, idx) and thresh of the 5i replica are reused, as 5q says),
the statistics of its draws, every refusal, and the trainer's host-side handling of a volume augmenter (checkpoint key,
load refusals, constructor and packed-path refusals).  tests/test_volume_augment_kernels_gpu.py ties the kernels to the
same replica."""
import numpy as np
import pytest
import torch

from multimodal_eeg_fmri_amd import ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer
from multimodal_eeg_fmri_amd.crossmodal_eeg_scr import EEGTransforms
from multimodal_eeg_fmri_amd.fmri_utils import VolumeTransforms, fMRITabularEncoder
from test_augment_host import h, thresh
from test_augment_host import stream_word as eeg_stream_word

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
VPURPOSE = {"flip_decision": 5, "shift_decision": 6, "shift_z": 7, "shift_y": 8, "shift_x": 9, "scale_decision": 10,
            "scale_u": 11, "noise_decision": 12, "gauss_a": 13, "gauss_b": 14, "erase_decision": 15, "erase_z": 16,
            "erase_y": 17, "erase_x": 18}
FLAGS = ("flip", "shift", "scale", "noise", "erase")


# ---------------------------------------------------------------- the replica (fp64; from section 5q)
def stream_word(seed, step, rank, purpose):
    z = (seed * 0x9E3779B97F4A7C15 + step * 0xBF58476D1CE4E5B9 + rank * 0x94D049BB133111EB
         + (VPURPOSE[purpose] + 1) * 0xD6E8FEB86659FD93) & M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z ^ (z >> 32)) & M32


def uniform_int(hv, n):
    return np.array([(int(v) * int(n)) >> 32 for v in hv], dtype=np.int64)


def draws(B, dims, *, p_flip, p_shift, max_shift, p_scale, scale_range, p_noise, p_erase, erase, seed, step, rank=0, **_):
    """the per-sample draws: flags {name: bool (B,)}, shift int (B, 3), factor fp32 (B,), erase_box int (B, 6)"""
    s = {k: stream_word(seed, step, rank, k) for k in VPURPOSE}
    b = np.arange(B)
    p = dict(flip=p_flip, shift=p_shift, scale=p_scale, noise=p_noise, erase=p_erase)
    flags = {k: h(s[k + "_decision"], b) < np.uint64(thresh(p[k])) for k in FLAGS}
    shift = np.stack([uniform_int(h(s["shift_" + ax], b), 2 * max_shift + 1) - max_shift for ax in "zyx"], axis=1)
    shift = shift * flags["shift"][:, None]
    u = h(s["scale_u"], b).astype(np.float64) * 2.0 ** -31 - 1.0
    factor = np.where(flags["scale"], 1.0 + float(np.float32(scale_range)) * u, 1.0).astype(np.float32)
    corner = [uniform_int(h(s["erase_" + ax], b), n - e + 1) for ax, n, e in zip("zyx", dims, erase)]
    box = np.stack(corner + [np.full(B, e) for e in erase], axis=1) * flags["erase"][:, None]
    return {"flags": flags, "shift": shift, "factor": factor, "erase_box": box}


def replica(x, *, noise_factor, fill, seed, step, rank=0, **kw):
    """x: (B, 1, D, H, W) array of fp32 values -> the draws plus, in fp64: std (B,), gathered (the source voxel of every
    output voxel; fill outside), scaled (gathered x factor), noise (z * noise_factor * std_b where it applies, else 0), out;
    and the bool masks inside (the voxel has a source voxel) and erased"""
    x = np.asarray(x, dtype=np.float64)
    B, _, D, H, W = x.shape
    V, half = D * H * W, (D * H * W + 1) // 2
    d = draws(B, (D, H, W), seed=seed, step=step, rank=rank, **kw)
    ga, gb = stream_word(seed, step, rank, "gauss_a"), stream_word(seed, step, rank, "gauss_b")
    fill = float(np.float32(fill))
    z, y, xx = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    out = {k: np.empty((B, 1, D, H, W)) for k in ("gathered", "scaled", "noise", "out")}
    out.update(inside=np.empty((B, 1, D, H, W), dtype=bool), erased=np.empty((B, 1, D, H, W), dtype=bool), std=np.empty(B))
    for b in range(B):
        dz, dy, dx = d["shift"][b]
        zs, ys, xs = z - dz, y - dy, xx - dx
        inside = (zs >= 0) & (zs < D) & (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
        sx = W - 1 - xs if d["flags"]["flip"][b] else xs
        g = np.where(inside, x[b, 0][np.clip(zs, 0, D - 1), np.clip(ys, 0, H - 1), np.clip(sx, 0, W - 1)], fill)
        scaled = np.where(inside & d["flags"]["scale"][b], g * float(d["factor"][b]), g)
        std = x[b].std(ddof=1)
        idx = b * half + np.arange(half)
        u1 = (h(ga, idx).astype(np.float64) + 1.0) / 4294967296.0
        u2 = h(gb, idx).astype(np.float64) / 4294967296.0
        r = np.sqrt(-2.0 * np.log(u1))
        zz = np.empty(2 * half)
        zz[0::2], zz[1::2] = r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)
        ez, ey, ex, ed, eh, ew = d["erase_box"][b]
        erased = (z >= ez) & (z < ez + ed) & (y >= ey) & (y < ey + eh) & (xx >= ex) & (xx < ex + ew)       # (empty when off)
        on = d["flags"]["noise"][b] and float(np.float32(noise_factor)) * std != 0
        noise = zz[:V].reshape(D, H, W) * (float(np.float32(noise_factor)) * std) * (inside & ~erased & on)
        res = np.where(erased, fill, scaled + noise)
        for k, v in (("gathered", g), ("scaled", scaled), ("noise", noise), ("out", res), ("inside", inside), ("erased", erased)):
            out[k][b, 0] = v
        out["std"][b] = std
    return dict(d, **out)


def _x(shape, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) + offset


def _all(p, **kw):
    return dict(dict(p_flip=p, p_shift=p, p_scale=p, p_noise=p, p_erase=p), **kw)


def fp32_tolerance(want):
    """what fp32 arithmetic may differ from the fp64 replica by: one rounding of the scaled value and one of the result
    (2^-24 relative each), four in the noise term (std_b, its product with noise_factor, z, their product: 4 x 2^-24 =
    2^-22 of the term); second-order terms are covered by the factor 1 + 2^-20"""
    return (2.0 ** -24 * (np.abs(want["scaled"]) + np.abs(want["out"])) + 2.0 ** -22 * np.abs(want["noise"])) * (1 + 2.0 ** -20)


# ---------------------------------------------------------------- CPU path against the replica
@pytest.mark.parametrize("shape", [(3, 1, 5, 7, 9), (2, 1, 4, 4, 4)])
@pytest.mark.parametrize("p", [0.0, 0.5, 1.0])
def test_cpu_path_equals_the_replica(shape, p):
    x = _x(shape, 100 + shape[0], offset=3.0)
    for step, rank, fill in ((0, 0, 0.0), (7, 0, -1.5), (7, 3, 0.0)):
        aug = VolumeTransforms(seed=21, max_shift=2, fill=fill, **_all(p))
        kw = aug.kernel_args(shape)
        assert kw["erase"] == tuple(max(1, int(0.25 * n)) for n in shape[2:])
        want = replica(x.numpy(), step=step, rank=rank, **kw)
        got = aug.batch(x, step, rank).numpy()
        mine = aug.draws(shape[0], shape[2:], step, rank)
        for k in FLAGS:
            assert np.array_equal(mine["flags"][k], want["flags"][k]), k
            assert want["flags"][k].all() if p == 1.0 else not want["flags"][k].any() if p == 0.0 else True
        assert np.array_equal(mine["shift"], want["shift"]) and np.array_equal(mine["erase_box"], want["erase_box"])
        assert np.array_equal(mine["factor"].view(np.int32), want["factor"].view(np.int32))
        filled = want["erased"] | ~want["inside"]
        assert (got[filled] == np.float32(fill)).all()
        assert (np.abs(got.astype(np.float64) - want["out"]) <= fp32_tolerance(want)).all()
        idle = ~(want["flags"]["scale"] | (want["noise"] != 0).any(axis=(1, 2, 3, 4)))      # pure gather, fill and erase
        assert np.array_equal(got[idle].view(np.int32), want["out"][idle].astype(np.float32).view(np.int32))
        if p == 0.0:
            assert np.array_equal(got.view(np.int32), x.numpy().view(np.int32))
        if p == 1.0:
            assert (np.abs(want["shift"]) <= 2).all() and (want["noise"] != 0).any()


def test_no_decision_passes_through_bit_for_bit():
    x = _x((3, 1, 5, 7, 9), 5, offset=-2.0)
    x[0, 0, 0, 0, 0] = -0.0
    for aug in (VolumeTransforms(seed=3, **_all(0.0)), VolumeTransforms(seed=3, max_shift=0, **_all(0.0, p_shift=1.0))):
        y = aug.batch(x, 4)
        assert y.data_ptr() != x.data_ptr() and np.array_equal(y.numpy().view(np.int32), x.numpy().view(np.int32))
    # the noise alone on a constant sample (std_b = 0) changes nothing either
    c = torch.full((2, 1, 4, 4, 4), 2.5)
    y = VolumeTransforms(seed=3, **_all(0.0, p_noise=1.0)).batch(c, 0)
    assert np.array_equal(y.numpy().view(np.int32), c.numpy().view(np.int32))


def test_call_is_the_per_sample_form_with_its_own_counter():
    aug = VolumeTransforms(seed=5, **_all(1.0))
    x = _x((1, 5, 7, 9), 2)
    first = [aug(x) for _ in range(3)]
    assert first[0].shape == x.shape and not torch.equal(first[0], first[1]) and not torch.equal(first[1], first[2])
    assert aug.state_dict() == {"seed": 5, "calls": 3}
    other = VolumeTransforms(seed=0, **_all(1.0))
    other.load_state_dict(aug.state_dict())
    assert torch.equal(aug(x), other(x)) and other.state_dict() == {"seed": 5, "calls": 4}
    assert torch.equal(aug.batch(x[None], step=1)[0], first[1])                            # __call__ k == batch(step = k)
    assert aug(x[0]).shape == (5, 7, 9)
    with pytest.raises(ValueError, match="VolumeTransforms"):
        aug(torch.zeros(2, 5, 7, 9))
    assert VolumeTransforms().params() == {"seed": 0, "p_flip": 0.5, "p_shift": 0.5, "max_shift": 2, "p_scale": 0.3,
                                           "scale_range": 0.1, "p_noise": 0.3, "noise_factor": 0.05, "p_erase": 0.3,
                                           "erase_fraction": 0.25, "fill": 0.0}


# ---------------------------------------------------------------- statistics of the draws
N = 4096


def _corr(a, b):
    a, b = a.astype(float) - a.mean(), b.astype(float) - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_decision_statistics():
    aug = VolumeTransforms(seed=0)                                 # the defaults: 0.5, 0.5, 0.3, 0.3, 0.3; max_shift 2
    d = draws(N, (4, 4, 4), step=0, **aug.kernel_args((N, 1, 4, 4, 4)))
    mine = aug.draws(N, (4, 4, 4), 0)
    assert all(np.array_equal(mine["flags"][k], d["flags"][k]) for k in FLAGS)
    assert np.array_equal(mine["shift"], d["shift"]) and np.array_equal(mine["erase_box"], d["erase_box"])
    rates = dict(flip=0.5, shift=0.5, scale=0.3, noise=0.3, erase=0.3)
    for k, p in rates.items():
        got = d["flags"][k].mean()
        print(k, got)
        assert abs(got - p) <= 5 * np.sqrt(p * (1 - p) / N), (k, got)
    for i, a in enumerate(FLAGS):
        for b in FLAGS[i + 1:]:
            c = _corr(d["flags"][a], d["flags"][b])
            assert abs(c) <= 5 / np.sqrt(N), (a, b, c)
    on = d["flags"]["shift"]
    k = int(on.sum())
    for ax in range(3):
        share = np.array([(d["shift"][on, ax] == v).mean() for v in range(-2, 3)])
        print("shift", ax, share)
        assert (np.abs(share - 0.2) <= 5 * np.sqrt(0.2 * 0.8 / k)).all(), (ax, share)
    assert (d["shift"][~on] == 0).all()
    for a in range(3):
        for b in range(a + 1, 3):
            assert abs(_corr(d["shift"][on, a], d["shift"][on, b])) <= 5 / np.sqrt(k)
    on = d["flags"]["erase"]
    k = int(on.sum())
    assert (d["erase_box"][on, 3:] == 1).all() and (d["erase_box"][~on] == 0).all()       # max(1, int(0.25 * 4)) = 1
    for ax in range(3):
        share = np.array([(d["erase_box"][on, ax] == v).mean() for v in range(4)])
        print("erase corner", ax, share)
        assert (np.abs(share - 0.25) <= 5 * np.sqrt(0.25 * 0.75 / k)).all(), (ax, share)
    f = d["factor"][d["flags"]["scale"]].astype(np.float64)
    assert (np.abs(f - 1) <= 0.1 * (1 + 2.0 ** -23)).all() and (d["factor"][~d["flags"]["scale"]] == 1).all()
    m = len(f)
    assert abs(f.mean() - 1) <= 5 * 0.1 / np.sqrt(3 * m)            # uniform on [0.9, 1.1): sd 0.1 / sqrt(3)


def test_it_is_independent_of_the_eeg_augmenter_at_the_same_seed_and_step():
    assert len(ops.augment_streams(0, 0, 0)) == 5 and len(ops.volume_augment_streams(0, 0, 0)) == 14
    for seed, step, rank in ((0, 0, 0), (9, 3, 1)):
        words = ops.volume_augment_streams(seed, step, rank)
        assert words == tuple(stream_word(seed, step, rank, k) for k in VPURPOSE)
        assert list(VPURPOSE) == list(ops.VOL_AUG_PURPOSES)
        assert len(set(words) | set(ops.augment_streams(seed, step, rank))) == 19
    d = draws(N, (4, 4, 4), step=0, **VolumeTransforms(seed=0).kernel_args((N, 1, 4, 4, 4)))
    for purpose in ("noise_decision", "drop_decision"):
        eeg = h(eeg_stream_word(0, 0, 0, purpose), np.arange(N)) < np.uint64(thresh(0.3))
        for k in FLAGS:
            c = _corr(eeg, d["flags"][k])
            assert abs(c) <= 5 / np.sqrt(N), (purpose, k, c)
    # ... and drawing volumes does not move the EEG augmenter's numbers
    x = _x((4, 8, 16), 1)
    a = EEGTransforms(p=1.0, seed=2).batch(x, 5)
    VolumeTransforms(seed=2, **_all(1.0)).batch(_x((2, 1, 4, 4, 4), 2), 5)
    assert torch.equal(a, EEGTransforms(p=1.0, seed=2).batch(x, 5))


# ---------------------------------------------------------------- refusals
def test_constructor_refusals():
    bad = [{"p_flip": -0.1}, {"p_shift": 1.5}, {"p_scale": float("nan")}, {"p_noise": "0.3"}, {"p_erase": 2}, {"max_shift": -1},
           {"max_shift": 1.5}, {"scale_range": -0.1}, {"scale_range": 1.0}, {"erase_fraction": 0.0}, {"erase_fraction": 1.5},
           {"noise_factor": float("inf")}, {"noise_factor": float("nan")}, {"fill": float("nan")}, {"fill": float("-inf")}]
    for kw in bad:
        with pytest.raises(ValueError, match="VolumeTransforms"):
            VolumeTransforms(**kw)
    VolumeTransforms(p_flip=0, p_shift=1, max_shift=0, scale_range=0.0, erase_fraction=1.0, noise_factor=-0.05, fill=-1.0)


def _virtual(*shape):
    """a tensor of that shape that owns one float (the checks come before anything reads it)"""
    return torch.zeros(1).expand(*shape)


def test_batch_and_ops_refuse_before_anything_runs():
    aug = VolumeTransforms(seed=1)
    for shape, msg in (((2, 2, 4, 4, 4), "one channel"), ((2, 1, 1, 1, 1), "D \\* H \\* W >= 2"), ((2, 4, 4, 4), "\\(B, 1, D, H, W\\)"),
                       ((1, 1, 2048, 1024, 1024), "below 2\\^31"), ((8, 1, 1024, 1024, 1024), "below 2\\^32"),
                       ((2, 1, 2, 8, 8), "max_shift"), ((2, 1, 8, 8, 2), "max_shift")):
        with pytest.raises(ValueError, match=msg):
            aug.batch(_virtual(*shape), 0)
    assert VolumeTransforms(max_shift=3).batch(torch.zeros(1, 1, 4, 4, 4), 0).shape == (1, 1, 4, 4, 4)
    with pytest.raises(ValueError, match="max_shift"):
        VolumeTransforms(max_shift=4).batch(torch.zeros(1, 1, 4, 4, 4), 0)
    good = VolumeTransforms().kernel_args((2, 1, 4, 4, 4))
    assert VolumeTransforms().check((2, 1, 4, 4, 4)) == good and good.pop("seed") == 0
    ops.volume_augment_check((2, 1, 4, 4, 4), **good)
    for key, value, msg in (("p_flip", 1.5, "p_flip"), ("p_shift", -0.5, "p_shift"), ("p_scale", float("nan"), "p_scale"),
                            ("p_noise", 2.0, "p_noise"), ("p_erase", -1.0, "p_erase"), ("max_shift", -1, "max_shift"),
                            ("max_shift", 4, "max_shift"), ("scale_range", 1.0, "scale_range"), ("scale_range", -0.1, "scale_range"),
                            ("noise_factor", float("inf"), "finite"), ("fill", float("nan"), "finite"),
                            ("erase", (0, 1, 1), "extents"), ("erase", (1, 5, 1), "extents")):
        with pytest.raises(ValueError, match=msg):
            ops.volume_augment_check((2, 1, 4, 4, 4), **dict(good, **{key: value}))
    x = torch.zeros(2, 1, 4, 4, 4)
    with pytest.raises(ValueError, match="overlap"):               # (before the device is asked for: CPU tensors get this far)
        ops.volume_augment_into(x, x, seed=0, step=0, **good)
    with pytest.raises(ValueError, match="overlap"):
        ops.volume_augment_into(x[:1], x.view(-1)[32:96].view(1, 1, 4, 4, 4), seed=0, step=0, **good)
    assert ops.volume_augment_plan_layout(2, 4, 4, 4) == (2 * 16 + 4 * 2 * 1, 16, 1)
    assert ops.volume_augment_plan_layout(1, 64, 64, 65) == (16 + 4 * 33, 16, 33)      # 266 240 voxels: chunks of 8192


# ---------------------------------------------------------------- the trainer's host side
def _trainer(fmri_augment=None, seed=0, **kw):
    torch.manual_seed(seed)
    return BridgeTrainer(eeg_channels=8, device="cpu", mode="manual", fmri_augment=fmri_augment, **kw)


def test_checkpoint_carries_the_volume_augmenter_only_when_there_is_one():
    plain = _trainer().checkpoint_state()
    assert "fmri_augment" not in plain["bridge_trainer_state"]
    eeg_only = _trainer(augment=EEGTransforms(seed=1)).checkpoint_state()
    assert set(eeg_only["bridge_trainer_state"]) == set(plain["bridge_trainer_state"]) | {"augment"}
    aug = VolumeTransforms(p_flip=0.4, max_shift=1, fill=-1.0, seed=17)
    tr = _trainer(aug)
    ck = tr.checkpoint_state()
    assert ck["bridge_trainer_state"]["fmri_augment"] == dict(aug.params(), step=0)
    assert set(ck["bridge_trainer_state"]) == set(plain["bridge_trainer_state"]) | {"fmri_augment"}
    assert set(ck) == set(plain) and ck["bridge_trainer_state"]["format"] == plain["bridge_trainer_state"]["format"]
    both = _trainer(aug, augment=EEGTransforms(seed=1)).checkpoint_state()
    assert set(both["bridge_trainer_state"]) == set(plain["bridge_trainer_state"]) | {"augment", "fmri_augment"}
    ck["bridge_trainer_state"]["fmri_augment"]["step"] = 41
    other = _trainer(VolumeTransforms(p_flip=0.4, max_shift=1, fill=-1.0, seed=17), seed=3)
    assert tr.fmri_augment_step == other.fmri_augment_step == 0
    other.load_checkpoint_state(ck)
    assert other.fmri_augment_step == 41 and other.augment_step == 0
    assert other.checkpoint_state()["bridge_trainer_state"]["fmri_augment"]["step"] == 41
    assert torch.equal(other.bucket.p, tr.bucket.p)


def test_checkpoint_of_another_volume_augmenter_is_refused_before_anything_is_touched():
    with_aug = _trainer(VolumeTransforms(seed=1)).checkpoint_state()
    without = _trainer().checkpoint_state()
    cases = [(_trainer(seed=3), with_aug, "fmri_augment differs: the checkpoint was written with a volume augmenter"),
             (_trainer(VolumeTransforms(seed=1), seed=3), without, "fmri_augment differs: the checkpoint was written without a volume augmenter"),
             (_trainer(VolumeTransforms(seed=2), seed=3), with_aug, "fmri_augment differs: checkpoint"),
             (_trainer(VolumeTransforms(max_shift=1, seed=1), seed=3), with_aug, "fmri_augment differs: checkpoint"),
             (_trainer(VolumeTransforms(fill=1.0, seed=1), seed=3), with_aug, "fmri_augment differs: checkpoint")]
    for tr, ck, msg in cases:
        before = [t.clone() for t in (tr.bucket.p, tr.bucket.m, tr.bucket.v, tr.bucket.state)]
        with pytest.raises(ValueError, match=msg):
            tr.load_checkpoint_state(ck)
        assert all(torch.equal(a, b) for a, b in zip(before, (tr.bucket.p, tr.bucket.m, tr.bucket.v, tr.bucket.state)))
        assert tr.fmri_augment_step == 0
    _trainer(seed=3).load_checkpoint_state(without)                # an old (augmenter-free) checkpoint loads as before


def test_constructor_takes_a_volume_augmenter_only_with_the_voxel_encoder():
    with pytest.raises(TypeError, match="VolumeTransforms"):
        _trainer(fmri_augment=EEGTransforms())
    with pytest.raises(TypeError, match="VolumeTransforms"):
        _trainer(fmri_augment=lambda v: v)
    with pytest.raises(TypeError, match="EEGTransforms"):          # augment= keeps taking the EEG augmenter only
        _trainer(augment=VolumeTransforms())
    with pytest.raises(ValueError, match="fMRITabularEncoder"):
        _trainer(fmri_augment=VolumeTransforms(), fmri_encoder=fMRITabularEncoder(10, 20, hidden_dim=64))
    assert _trainer().fmri_augment is None and _trainer(VolumeTransforms()).fmri_augment_step == 0


def test_packed_host_path_refuses_a_volume_augmenting_trainer():
    tr = _trainer(VolumeTransforms(seed=1))
    eeg, fmri = torch.randn(2, 8, 64), torch.randn(2, 1, 16, 16, 16)
    for call in (lambda: tr.pack_host_batch(eeg, fmri), lambda: tr.train_step_packed(torch.zeros(8, dtype=torch.uint8)),
                 lambda: tr.host_feeder()):
        with pytest.raises(ValueError, match="has a volume augmenter"):
            call()
