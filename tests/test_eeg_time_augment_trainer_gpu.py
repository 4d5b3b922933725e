"""GPU: `BridgeTrainer(eeg_time_augment=EEGTimeTransforms(...))` - the temporal augmentation draws nothing from the dropout
stream, the modes index its steps alike (through the capture's warm-ups), it composes with `augment=` and `fmri_augment=` in
the same launches, it reaches every EEG branch, inference never sees it, a resumed run continues bit for bit, an in-place
loader works, and the packed host path refuses it.  Shapes and helpers are tests/test_augment_trainer_gpu.py's."""
import pytest
import torch

from multimodal_eeg_fmri_amd import ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
from multimodal_eeg_fmri_amd.crossmodal_eeg_scr import EEGTimeTransforms, EEGTransforms
from multimodal_eeg_fmri_amd.fmri_utils import VolumeTransforms
from test_augment_trainer_gpu import B, C, T, VOL, _same, _snap, _steps

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_seed_epoch():
    ops.set_seed_epoch(None)
    yield
    ops.set_seed_epoch(None)


@pytest.fixture(scope="module")
def batches():
    return [synthetic_pairs(B, C, T, VOL, seed=700 + i) for i in range(2)]


def _make(mode, time_aug, dropout, seed=0, **kw):
    ops.set_seed_epoch(None)
    ops.set_dropout_seed(2024)
    torch.manual_seed(seed)
    return BridgeTrainer(eeg_channels=C, dropout=dropout, lr=1e-3, mode=mode, eeg_time_augment=time_aug, **kw).train()


def _every(seed=5):
    return EEGTimeTransforms(p_shift=1.0, max_shift=16, p_scale=1.0, p_invert=0.5, p_mask=1.0, seed=seed)


def _none(seed=3):
    return EEGTimeTransforms(p_shift=0.0, p_scale=0.0, p_invert=0.0, p_mask=0.0, seed=seed)


def test_p0_augmenter_has_no_effect_and_draws_no_dropout_seeds(batches):
    plain = _make("graph", None, 0.3)
    want = _steps(plain, batches, 3)
    want_state, seeds = _snap(plain), dict(ops._seed_state, epoch=None)
    aug = _make("graph", _none(), 0.3)
    got = _steps(aug, batches, 3)
    assert torch.isfinite(want).all() and torch.equal(want, got), (want, got)
    assert _same(want_state, _snap(aug)) and dict(ops._seed_state, epoch=None) == seeds
    assert aug.augment_step == 3 and plain.augment_step == 0


@pytest.mark.parametrize("feed", ["one batch object", "two alternating batches"])
def test_graph_and_manual_mode_index_the_steps_alike(batches, feed):
    feed = batches[:1] if feed == "one batch object" else batches
    losses = {}
    for mode in ("graph", "manual"):
        tr = _make(mode, EEGTimeTransforms(p_shift=0.6, p_scale=0.6, p_invert=0.3, p_mask=0.6, seed=11), 0.0)
        losses[mode] = _steps(tr, feed, 4)
        assert tr.augment_step == 4                               # (the capture's two warm-up steps consumed none)
    assert torch.isfinite(losses["graph"]).all()
    assert torch.equal(losses["graph"], losses["manual"]), losses


COMBOS = {"alone": (False, False), "with augment=": (True, False), "with fmri_augment=": (False, True), "with both": (True, True)}


def _partners(combo):
    eeg_aug, vol_aug = COMBOS[combo]
    return (EEGTransforms(p=1.0, seed=5) if eeg_aug else None), (VolumeTransforms(p_flip=1.0, p_shift=1.0, seed=7) if vol_aug else None)


@pytest.fixture(scope="module")
def by_hand(batches):
    """manual mode, dropout 0, no augmenter: 3 steps on the plain batches, and per combination 3 steps on the batches that
    `EEGTimeTransforms.batch(eeg, step=k, base=...)` (and `VolumeTransforms.batch`) produce, fed by hand"""
    plain = _steps(_make("manual", None, 0.0), batches, 3)
    out = {}
    for combo in COMBOS:
        base, vol = _partners(combo)
        fed = [(_every().batch(batches[k % 2][0], step=k, base=base),
                batches[k % 2][1] if vol is None else vol.batch(batches[k % 2][1], step=k)) for k in range(3)]
        out[combo] = _steps(_make("manual", None, 0.0), fed, 3)
    return plain, out


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("mode", ["graph", "manual"])
def test_it_augments_and_equals_feeding_the_augmented_batches_by_hand(batches, by_hand, mode, combo):
    plain, want = by_hand
    base, vol = _partners(combo)
    tr = _make(mode, _every(), 0.0, augment=base, fmri_augment=vol)
    got = _steps(tr, batches, 3)
    assert got[0] != plain[0], (got, plain)
    assert torch.equal(got, want[combo]), (got, want[combo])
    assert tr.augment_step == 3 and tr.fmri_augment_step == (3 if vol is not None else 0)


def test_autograd_mode_augments_too(batches):
    base = EEGTransforms(p=1.0, seed=5)
    got = _steps(_make("autograd", _every(), 0.0, augment=EEGTransforms(p=1.0, seed=5)), batches, 2)
    fed = [(_every().batch(batches[k][0], step=k, base=base), batches[k][1]) for k in range(2)]
    assert torch.equal(got, _steps(_make("autograd", None, 0.0), fed, 2)), got


def test_inference_is_untouched(batches):
    eeg, fmri = batches[0]
    a, b = _make("graph", None, 0.3), _make("graph", _every(), 0.3)
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
    mk = lambda: EEGTimeTransforms(p_shift=0.6, p_scale=0.6, p_invert=0.3, p_mask=0.6, seed=9)   # noqa: E731
    a = _make(mode, mk(), 0.3, augment=EEGTransforms(p=0.6, seed=9))
    _steps(a, batches, 3)
    path = str(tmp_path / "ck.pt")
    a.save_checkpoint(path, epoch=1)
    want, want_state = _steps(a, batches, 3, i0=3), _snap(a)
    b = _make(mode, mk(), 0.3, seed=4, augment=EEGTransforms(p=0.6, seed=9))
    ops.set_dropout_seed(77)
    b.load_checkpoint(path)
    assert b.augment_step == 3
    got = _steps(b, batches, 3, i0=3)
    assert torch.isfinite(want).all() and torch.equal(want, got), (want, got)
    assert _same(want_state, _snap(b)) and a.augment_step == b.augment_step == 6
    for other in (None, EEGTimeTransforms(p_shift=0.6, p_scale=0.6, p_invert=0.3, p_mask=0.6, seed=10),
                  EEGTimeTransforms(p_shift=0.6, max_shift=8, p_scale=0.6, p_invert=0.3, p_mask=0.6, seed=9)):
        with pytest.raises(ValueError, match="eeg_time_augment differs"):
            _make(mode, other, 0.3, augment=EEGTransforms(p=0.6, seed=9)).load_checkpoint(path)


@pytest.mark.parametrize("kind", ["power", "stft"])
def test_other_eeg_branches_are_augmented_through_the_fp32_batch(batches, kind):
    from multimodal_eeg_fmri_amd.crossmodal_v4_enhancements import MultiScaleSTFTPowerEncoder
    from multimodal_eeg_fmri_amd.enhanced_models_v4 import EnhancedPowerEncoder

    def step(time_aug, feed):
        ops.set_seed_epoch(None)
        torch.manual_seed(0)
        enc = MultiScaleSTFTPowerEncoder(C, (16, 32), 8, 128, 2, 4, 0.0) if kind == "stft" else EnhancedPowerEncoder(C, 128, 2, 4, 0.0)
        tr = _make("graph", time_aug, 0.0, eeg_encoder=enc)
        assert tr._eeg_kind == kind
        return tr.train_step(*feed)["loss"].item()
    eeg, fmri = batches[0]
    plain, aug = step(None, batches[0]), step(_every(), batches[0])
    assert aug == aug and abs(aug) < float("inf") and aug != plain, (plain, aug)
    assert aug == step(None, (_every().batch(eeg, step=0), fmri))


@pytest.mark.parametrize("kind", ["erp", "stft"])
def test_an_in_place_loader_works(batches, kind):
    """the batch IS the captured step's static `c["eeg"]`: the gather never runs in place"""
    from multimodal_eeg_fmri_amd.crossmodal_v4_enhancements import MultiScaleSTFTPowerEncoder

    def make(time_aug):
        torch.manual_seed(0)
        kw = {"eeg_encoder": MultiScaleSTFTPowerEncoder(C, (16, 32), 8, 128, 2, 4, 0.0)} if kind == "stft" else {}
        return _make("graph", time_aug, 0.0, **kw)
    want = _steps(make(_every()), batches, 3)
    tr = make(_every())
    got = [tr.train_step(*batches[0])["loss"].clone()]
    for k in (1, 2):
        eeg, fmri = batches[k % 2]
        tr._cap["eeg"].copy_(eeg)                                  # the loader writes the static buffer itself
        keep = tr._cap["eeg"].clone()
        got.append(tr.train_step(tr._cap["eeg"], fmri)["loss"].clone())
        if kind == "erp":
            assert torch.equal(tr._cap["eeg"], keep)               # (the packed operand took the augmented batch)
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(got), want), (got, want)


def test_packed_path_refuses_the_trainer(batches):
    tr = _make("graph", EEGTimeTransforms(seed=1), 0.0)
    tr.train_step(*batches[0])
    with pytest.raises(ValueError, match="temporal EEG augmenter"):
        tr.train_step_packed(torch.zeros(tr._cap["in"].numel(), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="temporal EEG augmenter"):
        tr.pack_host_batch(*batches[0])
    with pytest.raises(ValueError, match="temporal EEG augmenter"):
        tr.host_feeder()
