"""CPU: the EEG augmenter (`EEGTransforms`, crossmodal_eeg_scr.py) - its API, its numpy path against an fp64 replica of the
random stream written HERE from the stream's definition (csrc/augment.hip's header; nothing of it is imported
from the package), the statistics of that stream, and the trainer's host-side handling of an augmenter (checkpoint key,
refusals).  tests/test_augment_kernels_gpu.py ties the kernels to the same replica."""
import numpy as np
import pytest
import torch

from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer
from multimodal_eeg_fmri_amd.crossmodal_eeg_scr import EEGTransforms

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
PURPOSE = {"noise_decision": 0, "drop_decision": 1, "channel_keys": 2, "gauss_a": 3, "gauss_b": 4}


# ---------------------------------------------------------------- the replica (fp64; from the stream definition)
def stream_word(seed, step, rank, purpose):
    z = (seed * 0x9E3779B97F4A7C15 + step * 0xBF58476D1CE4E5B9 + rank * 0x94D049BB133111EB
         + (PURPOSE[purpose] + 1) * 0xD6E8FEB86659FD93) & M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z ^ (z >> 32)) & M32


def h(stream, idx):
    """h(stream, idx) on an integer array of indices < 2^32 -> uint64 array of 32-bit values"""
    u = np.uint64
    x = (np.asarray(idx, dtype=np.uint64) * u(0x9E3779B1) + u(stream)) & u(M32)
    x = x ^ (x >> u(16))
    x = (x * u(0x7FEB352D)) & u(M32)
    x = x ^ (x >> u(15))
    x = (x + u(((stream << 16) | (stream >> 16)) & M32)) & u(M32)
    x = (x * u(0x846CA68B)) & u(M32)
    return x ^ (x >> u(16))


def thresh(p):
    p = float(np.float32(p))
    return 0 if p <= 0 else 1 << 32 if p >= 1 else int(p * 4294967296.0)


def replica(x, *, p_noise, p_drop, noise_factor, n_drop, seed, step, rank=0):
    """x: (B, C, T) array of fp32 values -> dict(noise_on (B,), drop_mask (B, C), std (B,), noise (B, C, T), out (B, C, T)),
    everything in fp64: `noise` is z * noise_factor * std_b where noise is on (0 elsewhere), `out` the augmented batch"""
    x = np.asarray(x, dtype=np.float64)
    B, C, T = x.shape
    s = {k: stream_word(seed, step, rank, k) for k in PURPOSE}
    noise_on = h(s["noise_decision"], np.arange(B)) < np.uint64(thresh(p_noise))
    drop_on = h(s["drop_decision"], np.arange(B)) < np.uint64(thresh(p_drop))
    keys = h(s["channel_keys"], np.arange(B * C)).reshape(B, C)
    c = np.arange(C)
    less = (keys[:, None, :] < keys[:, :, None]) | ((keys[:, None, :] == keys[:, :, None]) & (c[None, None, :] < c[None, :, None]))
    drop_mask = drop_on[:, None] & (less.sum(-1) < n_drop)
    std = x.reshape(B, -1).std(axis=1, ddof=1)
    half = (T + 1) // 2
    idx = np.arange(B * C * half)
    u1 = (h(s["gauss_a"], idx).astype(np.float64) + 1.0) / 4294967296.0
    u2 = h(s["gauss_b"], idx).astype(np.float64) / 4294967296.0
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.empty((B, C, 2 * half))
    z[:, :, 0::2] = (r * np.cos(2 * np.pi * u2)).reshape(B, C, half)
    z[:, :, 1::2] = (r * np.sin(2 * np.pi * u2)).reshape(B, C, half)
    z = z[:, :, :T]
    noise = z * (float(np.float32(noise_factor)) * std * noise_on)[:, None, None]
    out = x + noise
    out[drop_mask] = 0.0
    return {"noise_on": noise_on, "drop_mask": drop_mask, "std": std, "noise": noise, "out": out}


def _x(shape, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) + offset


# ---------------------------------------------------------------- API
def test_constructor_errors():
    for kw in ({"p": -0.1}, {"p": 1.5}, {"p_noise": 2.0}, {"p_drop": -1.0}, {"p": "0.3"}, {"noise_factor": -0.01},
               {"noise_factor": float("nan")}, {"drop_fraction": 0.0}, {"drop_fraction": 1.5}, {"drop_fraction": -0.1}):
        with pytest.raises(ValueError, match="EEGTransforms"):
            EEGTransforms(**kw)
    a = EEGTransforms(0.2, 0.1)                                  # the reference's positional signature
    assert (a.p, a.noise_factor, a.p_noise, a.p_drop, a.drop_fraction, a.seed) == (0.2, 0.1, 0.2, 0.2, 0.1, 0)
    b = EEGTransforms(p=0.5, p_drop=0.0, drop_fraction=1.0, seed=9)
    assert (b.p_noise, b.p_drop) == (0.5, 0.0)
    assert EEGTransforms().p == 0.3 and EEGTransforms().noise_factor == 0.05


def test_call_returns_a_new_tensor_of_the_same_shape():
    aug = EEGTransforms(p=1.0, seed=4)
    x = _x((19, 37), 1)
    keep = x.clone()
    y = aug(x)
    assert y is not x and y.data_ptr() != x.data_ptr() and y.shape == x.shape and y.dtype == x.dtype
    assert torch.equal(x, keep) and not torch.equal(y, x)
    y0 = EEGTransforms(p=0.0)(x)
    assert y0.data_ptr() != x.data_ptr() and torch.equal(y0, x)
    with pytest.raises(ValueError):
        aug(torch.tensor(1.0))
    flat = _x((24,), 3)                                          # (what the aggregated datasets hand over: dimension 0 = channels)
    assert aug(flat).shape == (24,) and int((aug(flat) == 0).sum()) == 2
    with pytest.raises(ValueError, match="C \\* T >= 2"):
        aug.batch(torch.randn(2, 1, 1), 0)


@pytest.mark.parametrize("C", [5, 10, 19, 30, 64])
def test_n_drop_is_the_references_expression(C):
    aug = EEGTransforms(p_noise=0.0, p_drop=1.0, seed=C)
    y = aug.batch(_x((4, C, 6), C), step=0)
    zeroed = (y == 0).all(dim=2).sum(dim=1)
    assert zeroed.tolist() == [max(1, int(0.1 * C))] * 4 and aug.n_drop(C) == max(1, int(0.1 * C))


def test_state_dict_round_trip_continues_the_call_counter():
    x = _x((8, 16), 2)
    a = EEGTransforms(p=1.0, seed=5)
    first = [a(x) for _ in range(3)]
    assert not torch.equal(first[0], first[1]) and not torch.equal(first[1], first[2])     # each call is its own step
    sd = a.state_dict()
    assert sd == {"seed": 5, "calls": 3}
    b = EEGTransforms(p=1.0, seed=0)
    b.load_state_dict(sd)
    assert torch.equal(a(x), b(x)) and a.state_dict() == b.state_dict() == {"seed": 5, "calls": 4}
    assert torch.equal(EEGTransforms(p=1.0, seed=5)(x), first[0])
    assert torch.equal(a.batch(x[None], step=1)[0], first[1])                              # __call__ k == batch(step = k)


def test_it_is_what_the_dataset_hook_receives():
    import contextlib
    import io
    from multimodal_eeg_fmri_amd.crossmodal_v4_enhancements import BalancedTriModalDataset
    erp = {(s, 0): torch.full((4, 6), float(s)) + _x((4, 6), s) for s in (1, 2)}
    pw = {(s, 0): _x((4, 6), 10 + s) for s in (1, 2)}
    conn = {s: _x((5, 5), 20 + s) for s in (1, 2)}
    with contextlib.redirect_stdout(io.StringIO()):
        plain = BalancedTriModalDataset(erp, pw, conn, {1: 0, 2: 1})
        ds = BalancedTriModalDataset(erp, pw, conn, {1: 0, 2: 1}, transform=EEGTransforms(p=1.0, seed=1))
    e, p, c = ds[0][:3]
    assert e.shape == plain[0][0].shape and not torch.equal(e, plain[0][0]) and not torch.equal(p, plain[0][1])
    assert torch.equal(c, plain[0][2])


# ---------------------------------------------------------------- CPU path against the replica
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 19, 37), (1, 33, 64)])
@pytest.mark.parametrize("p", [0.0, 0.5, 1.0])
def test_cpu_path_equals_the_replica(shape, p):
    B, C, T = shape
    x = _x(shape, 100 + C, offset=3.0)
    for step, rank in ((0, 0), (7, 0), (7, 3)):
        aug = EEGTransforms(p=p, noise_factor=0.05, seed=21)
        want = replica(x.numpy(), p_noise=p, p_drop=p, noise_factor=0.05, n_drop=max(1, int(0.1 * C)), seed=21, step=step, rank=rank)
        got = aug.batch(x, step, rank).numpy()
        dropped = (got == 0).all(axis=2)
        assert np.array_equal(dropped, want["drop_mask"])
        changed = ((got != x.numpy()) & ~dropped[:, :, None]).any(axis=(1, 2))
        assert np.array_equal(changed, want["noise_on"])
        assert np.array_equal(got[~changed & ~dropped.any(axis=1)], x.numpy()[~changed & ~dropped.any(axis=1)])
        # fp32 rounding: half an ulp of the result; the fp32 noise scale carries two roundings (std_b, its product with
        # noise_factor), 2^-23 of the noise term
        tol = 2.0 ** -24 * np.abs(want["out"]) + 2.0 ** -23 * np.abs(want["noise"])
        assert (np.abs(got.astype(np.float64) - want["out"]) <= tol).all()
        if p == 1.0:
            assert dropped.sum() == B * max(1, int(0.1 * C)) and changed.all()
        if p == 0.0:
            assert np.array_equal(got, x.numpy())


# ---------------------------------------------------------------- stream statistics
N_STAT = 8 * 16 * 4096


@pytest.fixture(scope="module")
def residuals():
    """standardised noise r = (out - x) / (noise_factor * std_b) of the CPU path at p_noise = 1, p_drop = 0 (a valid setting:
    the drop decision is then never taken, so no channel needs excluding), for (step, rank) = (0, 0), (1, 0), (0, 1)"""
    x = _x((8, 16, 4096), 11)
    aug = EEGTransforms(p_noise=1.0, p_drop=0.0, noise_factor=0.05, seed=0)
    std = x.double().reshape(8, -1).std(dim=1)
    out = {}
    for step, rank in ((0, 0), (1, 0), (0, 1)):
        y = aug.batch(x, step, rank)
        out[step, rank] = ((y.double() - x.double()) / (0.05 * std)[:, None, None]).numpy()
    return out


def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_noise_moments(residuals):
    r = residuals[0, 0].ravel()
    N = r.size
    assert N == N_STAT == 524288
    mean, var = r.mean(), r.var()
    kurt = ((r - mean) ** 4).mean() / var ** 2
    tail, q = (np.abs(r) > 3).mean(), 0.0026998
    print(f"mean {mean:.3e} var-1 {var - 1:.3e} kurt-3 {kurt - 3:.3e} tail-q {tail - q:.3e}")
    assert abs(mean) <= 5 / np.sqrt(N)
    assert abs(var - 1) <= 5 * np.sqrt(2 / N)
    assert abs(kurt - 3) <= 5 * np.sqrt(96 / N)
    assert abs(tail - q) <= 5 * np.sqrt(q * (1 - q) / N)


def test_noise_correlations(residuals):
    r = residuals[0, 0]
    bound = 5 / np.sqrt(N_STAT)
    pairs = {"lag 1 along t": (r[:, :, :-1], r[:, :, 1:]),
             "the two members of a Box-Muller pair": (r[:, :, 0::2], r[:, :, 1::2]),
             "step s and s + 1": (r, residuals[1, 0]),
             "rank 0 and rank 1": (r, residuals[0, 1])}
    got = {k: _corr(a, b) for k, (a, b) in pairs.items()}
    print(got, bound)
    for k, v in got.items():
        assert abs(v) <= bound, (k, v, bound)


def test_decision_statistics():
    n, C, T = 4096, 6, 8
    x = _x((n, C, T), 12) + 5.0                                   # (no value is 0: a zero channel is a dropped channel)
    y = EEGTransforms(p=0.3, seed=0).batch(x, step=0).numpy()
    dropped = (y == 0).all(axis=2)
    drop_on = dropped.any(axis=1)
    noise_on = ((y != x.numpy()) & ~dropped[:, :, None]).any(axis=(1, 2))
    assert set(dropped.sum(axis=1)[drop_on].tolist()) == {1}       # exactly n_drop = max(1, int(0.6)) = 1 channel
    se = np.sqrt(0.21 / n)
    print(noise_on.mean(), drop_on.mean(), _corr(noise_on.astype(float), drop_on.astype(float)))
    assert abs(noise_on.mean() - 0.3) <= 5 * se and abs(drop_on.mean() - 0.3) <= 5 * se
    assert abs(_corr(noise_on.astype(float), drop_on.astype(float))) <= 5 / np.sqrt(n)
    k = int(drop_on.sum())
    share = dropped[drop_on].sum(axis=0) / k
    print(share)
    assert (np.abs(share - 1 / 6) <= 5 * np.sqrt((1 / 6) * (5 / 6) / k)).all()
    want = replica(x.numpy(), p_noise=0.3, p_drop=0.3, noise_factor=0.05, n_drop=1, seed=0, step=0)
    assert np.array_equal(noise_on, want["noise_on"]) and np.array_equal(dropped, want["drop_mask"])


# ---------------------------------------------------------------- the trainer's host side
def _trainer(augment=None, seed=0):
    torch.manual_seed(seed)
    return BridgeTrainer(eeg_channels=8, device="cpu", mode="manual", augment=augment)


def test_checkpoint_carries_the_augmenter_only_when_there_is_one():
    plain = _trainer().checkpoint_state()
    assert "augment" not in plain["bridge_trainer_state"]
    tr = _trainer(EEGTransforms(0.3, 0.05, p_drop=0.2, drop_fraction=0.25, seed=17))
    ck = tr.checkpoint_state()
    assert ck["bridge_trainer_state"]["augment"] == {"seed": 17, "step": 0, "p_noise": 0.3, "p_drop": 0.2, "noise_factor": 0.05,
                                                     "drop_fraction": 0.25}
    assert set(ck["bridge_trainer_state"]) == set(plain["bridge_trainer_state"]) | {"augment"}
    assert set(ck) == set(plain) and ck["bridge_trainer_state"]["format"] == plain["bridge_trainer_state"]["format"]
    ck["bridge_trainer_state"]["augment"]["step"] = 41
    other = _trainer(EEGTransforms(0.3, 0.05, p_drop=0.2, drop_fraction=0.25, seed=17), seed=3)
    other.load_checkpoint_state(ck)
    assert other.augment_step == 41 and other.checkpoint_state()["bridge_trainer_state"]["augment"]["step"] == 41
    assert torch.equal(other.bucket.p, tr.bucket.p)
    with pytest.raises(TypeError, match="EEGTransforms"):
        _trainer(augment=lambda t: t)


def test_checkpoint_of_another_augmenter_is_refused_before_anything_is_touched():
    with_aug = _trainer(EEGTransforms(seed=1)).checkpoint_state()
    without = _trainer().checkpoint_state()
    cases = [(_trainer(seed=3), with_aug, "written with an augmenter"),
             (_trainer(EEGTransforms(seed=1), seed=3), without, "written without an augmenter"),
             (_trainer(EEGTransforms(seed=2), seed=3), with_aug, "augment differs"),
             (_trainer(EEGTransforms(p=0.4, seed=1), seed=3), with_aug, "augment differs"),
             (_trainer(EEGTransforms(noise_factor=0.1, seed=1), seed=3), with_aug, "augment differs"),
             (_trainer(EEGTransforms(drop_fraction=0.2, seed=1), seed=3), with_aug, "augment differs")]
    for tr, ck, msg in cases:
        before = [t.clone() for t in (tr.bucket.p, tr.bucket.m, tr.bucket.v, tr.bucket.state)]
        with pytest.raises(ValueError, match=msg):
            tr.load_checkpoint_state(ck)
        assert all(torch.equal(a, b) for a, b in zip(before, (tr.bucket.p, tr.bucket.m, tr.bucket.v, tr.bucket.state)))
        assert tr.augment_step == 0
    _trainer(seed=3).load_checkpoint_state(without)                # an old (augmenter-free) checkpoint loads as before


def test_packed_host_path_refuses_an_augmenting_trainer():
    tr = _trainer(EEGTransforms(seed=1))
    eeg, fmri = torch.randn(2, 8, 64), torch.randn(2, 1, 16, 16, 16)
    for call in (lambda: tr.pack_host_batch(eeg, fmri), lambda: tr.train_step_packed(torch.zeros(8, dtype=torch.uint8)),
                 lambda: tr.host_feeder()):
        with pytest.raises(ValueError, match="cannot be augmented after the fact"):
            call()
