"""GPU: `BridgeTrainer(augment=EEGTransforms(...))` - the augmentation draws nothing from the dropout stream, the three modes
index its steps alike (through the capture's warm-ups), it reaches every EEG branch, inference never sees it, a resumed run
continues bit for bit, and the packed host path refuses it."""
import pytest
import torch

from multimodal_eeg_fmri_amd import ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
from multimodal_eeg_fmri_amd.crossmodal_eeg_scr import EEGTransforms

pytestmark = pytest.mark.gpu

B, C, T, VOL = 16, 16, 256, (16, 16, 16)


@pytest.fixture(autouse=True)
def _no_seed_epoch():
    ops.set_seed_epoch(None)
    yield
    ops.set_seed_epoch(None)


@pytest.fixture(scope="module")
def batches():
    return [synthetic_pairs(B, C, T, VOL, seed=700 + i) for i in range(2)]


def _make(mode, augment, dropout, seed=0, **kw):
    ops.set_seed_epoch(None)
    ops.set_dropout_seed(2024)
    torch.manual_seed(seed)
    return BridgeTrainer(eeg_channels=C, dropout=dropout, lr=1e-3, mode=mode, augment=augment, **kw).train()


def _steps(tr, feed, k, i0=0):
    out = [tr.train_step(*feed[i % len(feed)])["loss"].clone() for i in range(i0, i0 + k)]
    torch.cuda.synchronize()
    return torch.stack(out)


def _snap(tr):
    b = tr.bucket
    return [t.detach().clone() for t in (b.p, b.m, b.v, b.state)] + [v.detach().clone() for v in tr.state_dict().values()]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


def test_p0_augmenter_has_no_effect_and_draws_no_dropout_seeds(batches):
    plain = _make("graph", None, 0.3)
    want = _steps(plain, batches, 3)
    want_state, seeds = _snap(plain), dict(ops._seed_state, epoch=None)
    aug = _make("graph", EEGTransforms(p=0.0, seed=3), 0.3)
    got = _steps(aug, batches, 3)
    assert torch.isfinite(want).all() and torch.equal(want, got), (want, got)
    assert _same(want_state, _snap(aug)) and dict(ops._seed_state, epoch=None) == seeds
    assert aug.augment_step == 3 and plain.augment_step == 0


@pytest.mark.parametrize("feed", ["one batch object", "two alternating batches"])
def test_graph_and_manual_mode_index_the_steps_alike(batches, feed):
    feed = batches[:1] if feed == "one batch object" else batches
    losses = {}
    for mode in ("graph", "manual"):
        tr = _make(mode, EEGTransforms(p=0.6, seed=11), 0.0)
        losses[mode] = _steps(tr, feed, 4)
        assert tr.augment_step == 4                               # (the capture's two warm-up steps consumed none)
    assert torch.isfinite(losses["graph"]).all()
    assert torch.equal(losses["graph"], losses["manual"]), losses


@pytest.fixture(scope="module")
def by_hand(batches):
    """manual mode, dropout 0, no augmenter: 3 steps on the plain batches, and 3 on `aug.batch(eeg, step=k)` fed by hand"""
    aug = EEGTransforms(p=1.0, seed=5)
    plain = _steps(_make("manual", None, 0.0), batches, 3)
    fed = [(aug.batch(batches[k % 2][0], step=k), batches[k % 2][1]) for k in range(3)]
    return plain, _steps(_make("manual", None, 0.0), fed, 3)


@pytest.mark.parametrize("mode", ["graph", "manual"])
def test_it_augments_and_equals_feeding_the_augmented_batches_by_hand(batches, by_hand, mode):
    plain, want = by_hand
    got = _steps(_make(mode, EEGTransforms(p=1.0, seed=5), 0.0), batches, 3)
    assert got[0] != plain[0], (got, plain)
    assert torch.equal(got, want), (got, want)


def test_autograd_mode_augments_too(batches):
    aug = EEGTransforms(p=1.0, seed=5)
    got = _steps(_make("autograd", EEGTransforms(p=1.0, seed=5), 0.0), batches, 2)
    fed = [(aug.batch(batches[k][0], step=k), batches[k][1]) for k in range(2)]
    assert torch.equal(got, _steps(_make("autograd", None, 0.0), fed, 2)), got


def test_inference_is_untouched(batches):
    eeg, fmri = batches[0]
    a, b = _make("graph", None, 0.3), _make("graph", EEGTransforms(p=1.0, seed=5), 0.3)
    for tr in (a, b):
        tr.train_step(eeg, fmri)
    with torch.no_grad():
        b.bucket.p.copy_(a.bucket.p)
        for x, y in zip(b.buffers(), a.buffers()):
            x.copy_(y)
    ops.weights_changed()
    ea, eb = a.evaluate(eeg, fmri), b.evaluate(eeg, fmri)
    assert all(torch.equal(ea[k], eb[k]) for k in ea)
    za, zb = a.embed(eeg, fmri), b.embed(eeg, fmri)
    assert torch.equal(za[0], zb[0]) and torch.equal(za[1], zb[1])
    assert b.augment_step == 1


@pytest.mark.parametrize("mode", ["graph", "manual"])
def test_resume_continues_bit_for_bit(batches, mode, tmp_path):
    a = _make(mode, EEGTransforms(p=0.6, seed=9), 0.3)
    _steps(a, batches, 3)
    path = str(tmp_path / "ck.pt")
    a.save_checkpoint(path, epoch=1)
    want, want_state = _steps(a, batches, 3, i0=3), _snap(a)
    b = _make(mode, EEGTransforms(p=0.6, seed=9), 0.3, seed=4)
    ops.set_dropout_seed(77)
    b.load_checkpoint(path)
    assert b.augment_step == 3
    got = _steps(b, batches, 3, i0=3)
    assert torch.isfinite(want).all() and torch.equal(want, got), (want, got)
    assert _same(want_state, _snap(b)) and a.augment_step == b.augment_step == 6
    with pytest.raises(ValueError, match="augment differs"):
        _make(mode, None, 0.3).load_checkpoint(path)


@pytest.mark.parametrize("kind", ["power", "stft"])
def test_other_eeg_branches_are_augmented_through_the_fp32_batch(batches, kind):
    from multimodal_eeg_fmri_amd.crossmodal_v4_enhancements import MultiScaleSTFTPowerEncoder
    from multimodal_eeg_fmri_amd.enhanced_models_v4 import EnhancedPowerEncoder

    def step(augment):
        ops.set_seed_epoch(None)
        torch.manual_seed(0)
        enc = MultiScaleSTFTPowerEncoder(C, (16, 32), 8, 128, 2, 4, 0.0) if kind == "stft" else EnhancedPowerEncoder(C, 128, 2, 4, 0.0)
        tr = _make("graph", augment, 0.0, eeg_encoder=enc)
        assert tr._eeg_kind == kind
        return tr.train_step(*batches[0])["loss"].item()
    plain, aug = step(None), step(EEGTransforms(p=1.0, seed=5))
    assert aug == aug and abs(aug) < float("inf") and aug != plain, (plain, aug)


def test_packed_path_refuses_an_augmenting_trainer(batches):
    tr = _make("graph", EEGTransforms(seed=1), 0.0)
    tr.train_step(*batches[0])
    with pytest.raises(ValueError, match="cannot be augmented after the fact"):
        tr.train_step_packed(torch.zeros(tr._cap["in"].numel(), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="cannot be augmented after the fact"):
        tr.pack_host_batch(*batches[0])
    with pytest.raises(ValueError, match="cannot be augmented after the fact"):
        tr.host_feeder()
