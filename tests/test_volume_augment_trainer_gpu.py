"""GPU: `BridgeTrainer(fmri_augment=VolumeTransforms(...))` - in graph mode the two launches write the captured step's static
fMRI buffer and the EEG batch is staged without the fMRI copy, the three modes index the steps alike, an all-zero augmenter
and every inference entry point leave the trainer's numbers alone, a resumed run continues bit for bit, and a trainer
without a volume augmenter issues the launches it always did."""
import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
from multimodal_eeg_fmri_amd.crossmodal_eeg_scr import EEGTransforms
from multimodal_eeg_fmri_amd.fmri_utils import VolumeTransforms

pytestmark = pytest.mark.gpu

B, C, T = 4, 8, 64
VOLS = [(8, 8, 8), (5, 7, 9)]


@pytest.fixture(autouse=True)
def _no_seed_epoch():
    ops.set_seed_epoch(None)
    yield
    ops.set_seed_epoch(None)


@pytest.fixture(scope="module")
def batches():
    return {vol: [synthetic_pairs(B, C, T, vol, seed=800 + i) for i in range(2)] for vol in VOLS}


def _aug(p=None, **kw):
    """an augmenter that does something to most samples of a 4-sample batch (p: every probability)"""
    probs = dict(p_flip=0.5, p_shift=0.7, p_scale=0.6, p_noise=0.6, p_erase=0.5) if p is None else \
        dict(p_flip=p, p_shift=p, p_scale=p, p_noise=p, p_erase=p)
    return VolumeTransforms(**dict(dict(probs, max_shift=2, seed=13), **kw))


def _make(mode, fmri_augment, dropout, seed=0, **kw):
    ops.set_seed_epoch(None)
    ops.set_dropout_seed(2024)
    torch.manual_seed(seed)
    return BridgeTrainer(eeg_channels=C, dropout=dropout, lr=1e-3, mode=mode, fmri_augment=fmri_augment, **kw).train()


def _steps(tr, feed, k, i0=0):
    out = [tr.train_step(*feed[i % len(feed)])["loss"].clone() for i in range(i0, i0 + k)]
    torch.cuda.synchronize()
    return torch.stack(out)


def _snap(tr):
    b = tr.bucket
    return [t.detach().clone() for t in (b.p, b.m, b.v, b.state)] + [v.detach().clone() for v in tr.state_dict().values()]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("vol", VOLS)
def test_the_static_fmri_buffer_holds_the_augmented_batch(batches, vol):
    feed = batches[vol]
    tr = _make("graph", _aug(), 0.0)
    ref = _aug()
    changed = 0
    for step in range(3):
        eeg, fmri = feed[step % 2]
        keep = fmri.clone()
        loss = tr.train_step(eeg, fmri)["loss"].item()
        assert loss == loss and torch.equal(fmri, keep)               # (the caller's batch is only read)
        want = ref.batch(fmri, step, 0)
        assert torch.equal(_bits(tr.input_buffers()[1]), _bits(want)), step
        changed += int(not torch.equal(want, fmri))
        assert tr.fmri_augment_step == step + 1                      # (the capture's two warm-up steps consumed none)
    assert changed == 3 and tr.augment_step == 0


def test_the_static_buffer_itself_may_be_the_batch(batches):
    feed = batches[VOLS[0]]
    tr = _make("graph", _aug(1.0), 0.0)
    tr.train_step(*feed[0])
    buf = tr.input_buffers()[1]
    buf.copy_(feed[1][1])                                             # an in-place loader
    tr.train_step(feed[1][0], buf)
    torch.cuda.synchronize()
    want = _aug(1.0).batch(feed[1][1], 1, 0)
    assert not torch.equal(want, feed[1][1]) and torch.equal(_bits(buf), _bits(want))
    scratch, plan = tr._cap["fmri_scratch"], tr._cap["fmri_aug_plan"]
    buf.copy_(feed[0][1])                                             # the next step reuses the scratch tensor and the plan
    tr.train_step(feed[0][0], buf)
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(_aug(1.0).batch(feed[0][1], 2, 0)))
    assert tr._cap["fmri_scratch"] is scratch and tr._cap["fmri_aug_plan"] is plan


def test_the_stft_front_end_gets_a_plain_copy_of_the_eeg_batch(monkeypatch):
    """the STFT front end reads the fp32 EEG batch, not a packed operand: after the two volume launches the EEG staging
    is a copy into the static buffer and no further launch"""
    from multimodal_eeg_fmri_amd.crossmodal_v4_enhancements import MultiScaleSTFTPowerEncoder
    feed = [synthetic_pairs(B, C, 256, VOLS[0], seed=850 + i) for i in range(2)]
    ops.set_seed_epoch(None)
    torch.manual_seed(0)
    tr = _make("graph", _aug(1.0), 0.0, eeg_encoder=MultiScaleSTFTPowerEncoder(C, (16, 32), 8, 128, 2, 4, 0.0))
    assert tr._eeg_kind == "stft"
    tr.train_step(*feed[0])
    torch.cuda.synchronize()
    names, real = [], _hip.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(_hip, "call", spy)
    loss = tr.train_step(*feed[1])["loss"].item()
    monkeypatch.setattr(_hip, "call", real)
    assert loss == loss and names == ["mm_volume_augment_plan", "mm_volume_augment"], names
    eeg_buf, fmri_buf = tr.input_buffers()
    assert tr._cap["xb"] is None and torch.equal(eeg_buf, feed[1][0])
    assert torch.equal(_bits(fmri_buf), _bits(_aug(1.0).batch(feed[1][1], 1, 0)))


def test_launches_of_a_replayed_step_and_the_eeg_operand(batches, monkeypatch):
    """the `_hip.call` names of one replayed step: unchanged without a volume augmenter; with one, the two volume launches
    and then the EEG staging without its fMRI copy - whose packed operand is what the EEG-only trainer stages"""
    feed = batches[VOLS[0]]
    names = []
    real = _hip.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)
    want = {"plain": ["mm_stage_inputs"],
            "eeg": ["mm_eeg_augment_plan", "mm_stage_inputs_aug"],
            "volume": ["mm_volume_augment_plan", "mm_volume_augment", "mm_pack_nct_bf16"],
            "both": ["mm_volume_augment_plan", "mm_volume_augment", "mm_eeg_augment_plan", "mm_stage_inputs_aug"]}
    xb = {}
    for kind in want:
        tr = _make("graph", _aug(1.0) if kind in ("volume", "both") else None, 0.0,
                   augment=EEGTransforms(p=1.0, seed=5) if kind in ("eeg", "both") else None)
        tr.train_step(*feed[0])
        torch.cuda.synchronize()
        monkeypatch.setattr(_hip, "call", spy)
        names.clear()
        tr.train_step(*feed[1])
        monkeypatch.setattr(_hip, "call", real)
        torch.cuda.synchronize()
        assert names == want[kind], (kind, names)
        xb[kind] = tr._cap["xb"].clone()
        fm = tr.input_buffers()[1]
        assert torch.equal(fm, feed[1][1]) == (kind in ("plain", "eeg"))
    assert torch.equal(xb["both"].view(torch.int16), xb["eeg"].view(torch.int16))
    assert torch.equal(xb["volume"].view(torch.int16), xb["plain"].view(torch.int16))
    assert not torch.equal(xb["eeg"], xb["plain"])


@pytest.mark.parametrize("vol", VOLS)
def test_graph_and_manual_mode_agree_and_equal_feeding_augmented_volumes_by_hand(batches, vol):
    feed = batches[vol]
    losses = {}
    for mode in ("graph", "manual"):
        tr = _make(mode, _aug(), 0.0)
        losses[mode] = _steps(tr, feed, 3)
        assert tr.fmri_augment_step == 3
    assert torch.isfinite(losses["graph"]).all()
    assert torch.equal(losses["graph"], losses["manual"]), losses
    ref = _aug()
    fed = [(feed[k % 2][0], ref.batch(feed[k % 2][1], k)) for k in range(3)]
    by_hand = _steps(_make("manual", None, 0.0), fed, 3)
    plain = _steps(_make("manual", None, 0.0), feed, 3)
    assert torch.equal(losses["manual"], by_hand) and not torch.equal(by_hand, plain), (losses, by_hand, plain)


def test_autograd_mode_augments_too(batches):
    feed = batches[VOLS[0]]
    got = _steps(_make("autograd", _aug(1.0), 0.0), feed, 2)
    ref = _aug(1.0)
    fed = [(feed[k][0], ref.batch(feed[k][1], k)) for k in range(2)]
    assert torch.equal(got, _steps(_make("autograd", None, 0.0), fed, 2)), got


def test_an_all_zero_augmenter_has_no_effect_and_draws_no_dropout_seeds(batches):
    feed = batches[VOLS[0]]
    plain = _make("graph", None, 0.3)
    want = _steps(plain, feed, 3)
    want_state, seeds = _snap(plain), dict(ops._seed_state, epoch=None)
    aug = _make("graph", _aug(0.0), 0.3)
    got = _steps(aug, feed, 3)
    assert torch.isfinite(want).all() and torch.equal(want, got), (want, got)
    assert _same(want_state, _snap(aug)) and dict(ops._seed_state, epoch=None) == seeds
    assert aug.fmri_augment_step == 3 and plain.fmri_augment_step == 0


def test_inference_is_untouched(batches):
    eeg, fmri = batches[VOLS[0]][0]
    a, b = _make("graph", None, 0.3), _make("graph", _aug(1.0), 0.3)
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
    ra, rb = a.evaluate_retrieval(eeg, fmri, ks=(1, 2)), b.evaluate_retrieval(eeg, fmri, ks=(1, 2))
    assert ra.keys() == rb.keys() and all(_equal(ra[k], rb[k]) for k in ra)
    assert b.fmri_augment_step == 1


def _equal(u, v):
    if torch.is_tensor(u):
        return torch.equal(u, v)
    if isinstance(u, dict):
        return u.keys() == v.keys() and all(_equal(u[k], v[k]) for k in u)
    if isinstance(u, (tuple, list)):
        return len(u) == len(v) and all(_equal(a, b) for a, b in zip(u, v))
    return u == v


def test_resume_continues_bit_for_bit(batches, tmp_path):
    feed = batches[VOLS[0]]
    a = _make("graph", _aug(), 0.3)
    _steps(a, feed, 2)
    path = str(tmp_path / "ck.pt")
    a.save_checkpoint(path, epoch=1)
    want, want_state = _steps(a, feed, 3, i0=2), _snap(a)
    b = _make("graph", _aug(), 0.3, seed=4)
    ops.set_dropout_seed(77)
    b.load_checkpoint(path)
    assert b.fmri_augment_step == 2
    got = _steps(b, feed, 3, i0=2)
    assert torch.isfinite(want).all() and torch.equal(want, got), (want, got)
    assert _same(want_state, _snap(b)) and a.fmri_augment_step == b.fmri_augment_step == 5
    with pytest.raises(ValueError, match="fmri_augment differs"):
        _make("graph", None, 0.3).load_checkpoint(path)
    with pytest.raises(ValueError, match="fmri_augment differs"):
        _make("graph", _aug(seed=14), 0.3).load_checkpoint(path)


def test_packed_path_refuses_a_volume_augmenting_trainer(batches):
    feed = batches[VOLS[0]]
    tr = _make("graph", _aug(), 0.0)
    tr.train_step(*feed[0])
    with pytest.raises(ValueError, match="has a volume augmenter"):
        tr.train_step_packed(torch.zeros(tr._cap["in"].numel(), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="has a volume augmenter"):
        tr.pack_host_batch(*feed[0])
    with pytest.raises(ValueError, match="has a volume augmenter"):
        tr.host_feeder()
