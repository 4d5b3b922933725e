"""CPU: the BridgeTrainer checkpoint container, its AdamW layout, the refusals, the atomic write and the schedule of
`fit` (the trainer constructs on CPU; nothing here launches a kernel)."""
import os

import pytest
import torch

from multimodal_eeg_fmri_amd import ops
from multimodal_eeg_fmri_amd.bridge_checkpoint import CONTAINER_KEYS
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer
from multimodal_eeg_fmri_amd.crossmodal_v4_enhancements import CosineAnnealingWarmup
from multimodal_eeg_fmri_amd.enhanced_models_v4 import EnhancedERPEncoder, EnhancedPowerEncoder
from multimodal_eeg_fmri_amd.fmri_utils import fMRIVolumeEncoder3D


def _trainer(seed=0, **kw):
    torch.manual_seed(seed)
    kw.setdefault("eeg_channels", 8)
    return BridgeTrainer(device="cpu", mode="manual", **kw)


def _fill(tr, seed):
    """distinct values in every slot of the bucket and the optimizer words (as if trained)"""
    g = torch.Generator().manual_seed(seed)
    b = tr.bucket
    with torch.no_grad():
        b.p.copy_(torch.randn(b.n, generator=g))
        b.m.copy_(torch.randn(b.n, generator=g))
        b.v.copy_(torch.rand(b.n, generator=g))
        b.state[0] = 17.0
        tr.set_lr(3e-4)
        for t in tr.buffers():
            if t.is_floating_point():
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
            else:
                t.fill_(5)


def _everything(tr):
    b = tr.bucket
    return ([t.clone() for t in (b.p, b.m, b.v, b.state)] + [v.clone() for v in tr.state_dict().values()],
            dict(ops._seed_state), tr.lr, tr.betas, tr.eps, tr.weight_decay, tr.grad_clip)


def _same(a, b):
    ta, tb = a[0], b[0]
    return len(ta) == len(tb) and all(torch.equal(x, y) for x, y in zip(ta, tb)) and a[1:] == b[1:]


def test_container_keys_and_weights_only_load(tmp_path):
    tr = _trainer()
    _fill(tr, 1)
    path = str(tmp_path / "ck.pt")
    sched = CosineAnnealingWarmup(torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-3), 3, 10)
    sched.step()
    tr.save_checkpoint(path, epoch=4, metrics={"mean_R@1": 0.25}, scheduler=sched)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) == set(CONTAINER_KEYS)
    assert ck["epoch"] == 4 and ck["metrics"] == {"mean_R@1": 0.25}
    assert ck["scheduler_state_dict"]["current_epoch"] == 1
    # model_state_dict is the unchanged nn.Module.state_dict()
    want = tr.state_dict()
    assert list(ck["model_state_dict"]) == list(want)
    assert all(torch.equal(ck["model_state_dict"][k], want[k]) for k in want)
    bts = ck["bridge_trainer_state"]
    assert bts["eeg_kind"] == "erp" and bts["world"] == 1 and bts["bucket_n"] == tr.bucket.n
    assert bts["groups"] == [[n, r, lo, hi] for n, r, lo, hi in tr.groups]
    assert bts["step"] == 17.0 and abs(bts["lr"] - 3e-4) < 1e-10
    assert bts["dropout"]["kind"] == "counter" and bts["fit"] is None
    assert torch.equal(bts["optimizer_words"], tr.bucket.state)
    # a reference-side loader indexes only the keys it knows: the sub-dicts load into stand-alone encoders
    enc = EnhancedERPEncoder(8, 128, 2, 4, 0.3)
    enc.load_state_dict({k[len("eeg_encoder."):]: v for k, v in ck["model_state_dict"].items()
                         if k.startswith("eeg_encoder.")})
    assert all(torch.equal(a, b) for a, b in zip(enc.state_dict().values(), tr.eeg_encoder.state_dict().values()))
    fe = fMRIVolumeEncoder3D(1, 64, dropout=0.3)
    fe.load_state_dict({k[len("fmri_encoder."):]: v for k, v in ck["model_state_dict"].items()
                        if k.startswith("fmri_encoder.")})


def test_optimizer_layout_is_torch_adamw_in_parameters_order(tmp_path):
    tr = _trainer()
    _fill(tr, 2)
    ck = tr.checkpoint_state()
    trainable = [p for p in tr.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(trainable, lr=1.0)
    opt.load_state_dict(ck["optimizer_state_dict"])
    b = tr.bucket
    assert len(opt.state) == len(trainable)
    assert abs(opt.param_groups[0]["lr"] - 3e-4) < 1e-10 and opt.param_groups[0]["betas"] == tr.betas
    for p in trainable:
        # the parameter's own range of the flat bucket, found from its storage (independent of the map)
        off = (p.data_ptr() - b.p.data_ptr()) // 4
        sl = slice(off, off + p.numel())
        st = opt.state[p]
        assert torch.equal(st["exp_avg"], b.m[sl].view(p.shape))
        assert torch.equal(st["exp_avg_sq"], b.v[sl].view(p.shape))
        assert float(st["step"]) == 17.0
    assert any(p is tr.head.logit_scale for p in trainable)
    frozen = [n for n, p in tr.named_parameters() if not p.requires_grad]
    assert frozen and all(n in ck["model_state_dict"] for n in frozen)
    # the bucket is NOT in parameters() order, so the map is not the identity
    assert [id(p) for p in trainable] != [id(p) for p in b.params]
    # and back: a state edited through torch's AdamW loads into the trainer's moments
    for p in trainable:
        opt.state[p]["exp_avg"].mul_(2)
    ck["optimizer_state_dict"] = opt.state_dict()
    tr2 = _trainer(seed=5)
    tr2.load_checkpoint_state(ck)
    assert torch.equal(tr2.bucket.m, 2 * b.m) and torch.equal(tr2.bucket.v, b.v) and torch.equal(tr2.bucket.p, b.p)


def test_load_restores_everything_in_place_and_the_dropout_counter():
    tr = _trainer()
    _fill(tr, 3)
    ops.set_dropout_seed(4242)
    for _ in range(7):
        ops._next_seed()
    ck = tr.checkpoint_state()
    want = _everything(tr)
    tr2 = _trainer(seed=9)
    ptrs = [p.data_ptr() for p in tr2.parameters()]
    ops.set_dropout_seed(1)
    for _ in range(3):
        ops._next_seed()
    tr2.load_checkpoint_state(ck)
    assert [p.data_ptr() for p in tr2.parameters()] == ptrs                 # in place: views of the bucket stay views
    got = _everything(tr2)
    assert _same(want, got)
    assert ops._seed_state["base"] == 4242 and ops._seed_state["step"] == 7


@pytest.mark.parametrize("case", ["eeg_kind", "shapes", "world", "groups", "not a checkpoint"])
def test_refusals_name_the_field_and_touch_nothing(case):
    src = _trainer()
    _fill(src, 4)
    if case == "eeg_kind":
        torch.manual_seed(0)
        other = BridgeTrainer(device="cpu", mode="manual", eeg_encoder=EnhancedPowerEncoder(8, 128, 2, 4, 0.3))
        ck = other.checkpoint_state()
    elif case == "shapes":
        ck = _trainer(eeg_channels=16).checkpoint_state()
    else:
        ck = src.checkpoint_state()
        if case == "world":
            ck["bridge_trainer_state"]["world"] = 2
        elif case == "groups":
            g = ck["bridge_trainer_state"]["groups"]
            g[0][3] += 1
            g[1][2] += 1
        else:
            ck = dict(ck["model_state_dict"])
    tr = _trainer(seed=7)
    _fill(tr, 5)
    ops.set_dropout_seed(31)
    before = _everything(tr)
    with pytest.raises(ValueError) as e:
        tr.load_checkpoint_state(ck)
    field = {"eeg_kind": "eeg_kind", "shapes": "shapes", "world": "world", "groups": "groups",
             "not a checkpoint": "not a BridgeTrainer checkpoint"}[case]
    assert field in str(e.value)
    assert _same(before, _everything(tr))


def test_bare_state_dict_and_reference_container_load_the_model_only(tmp_path):
    src = _trainer()
    _fill(src, 6)
    bare, ref = str(tmp_path / "bare.pt"), str(tmp_path / "ref.pt")
    torch.save(src.state_dict(), bare)
    torch.save({"epoch": 3, "model_state_dict": src.state_dict(), "metrics": {"f1": 0.5}}, ref)
    for path, want in ((bare, (None, None)), (ref, (3, {"f1": 0.5}))):
        tr = _trainer(seed=8)
        m0 = tr.bucket.m.clone()
        assert tr.load_checkpoint(path) == want
        assert all(torch.equal(a, b) for a, b in zip(tr.state_dict().values(), src.state_dict().values()))
        assert torch.equal(tr.bucket.m, m0)


def test_save_is_atomic(tmp_path, monkeypatch):
    tr = _trainer()
    path = str(tmp_path / "last.pt")
    tr.save_checkpoint(path, epoch=1)
    good = open(path, "rb").read()
    _fill(tr, 7)
    real = torch.save

    def dying_save(obj, f, *a, **k):
        f.write(b"partial checkpoint bytes")
        raise RuntimeError("disk full")
    monkeypatch.setattr(torch, "save", dying_save)
    with pytest.raises(RuntimeError, match="disk full"):
        tr.save_checkpoint(path, epoch=2)
    assert open(path, "rb").read() == good                      # the previous file is whole
    assert os.listdir(tmp_path) == ["last.pt"]                  # no temporary left behind
    monkeypatch.setattr(torch, "save", real)
    fresh = str(tmp_path / "sub" / "x.pt")
    os.makedirs(os.path.dirname(fresh))
    monkeypatch.setattr(torch, "save", dying_save)
    with pytest.raises(RuntimeError):
        tr.save_checkpoint(fresh, epoch=2)
    assert os.listdir(os.path.dirname(fresh)) == []              # no partial file at all


def test_fit_schedule_matches_cosine_annealing_warmup(tmp_path):
    """fit steps the package's CosineAnnealingWarmup once per epoch after the epoch's training, as the reference
    does: epoch 1 at the base rate, epoch e at _lr_at(e - 1); the LR word follows (no batches: nothing launches)"""
    tr = _trainer(lr=2e-3)
    hist = tr.fit([], 8, warmup_epochs=3, min_lr=1e-5)
    ref = CosineAnnealingWarmup(torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=2e-3), 3, 8, min_lr=1e-5)
    want = [2e-3] + [ref._lr_at(e) for e in range(1, 8)]
    assert [h["lr"] for h in hist] == want
    assert [h["epoch"] for h in hist] == list(range(1, 9)) and all(h["steps"] == 0 for h in hist)
    assert tr.lr == ref._lr_at(8) and float(tr.bucket.state[2]) == torch.tensor(ref._lr_at(8)).item()
    # resumed at an epoch boundary: the same rates, the same history
    d = str(tmp_path / "run")
    tr2 = _trainer(lr=2e-3)
    with pytest.raises(RuntimeError):
        tr2.fit(lambda e: [] if e <= 5 else (_ for _ in ()).throw(RuntimeError("interrupted")), 8,
                warmup_epochs=3, min_lr=1e-5, checkpoint_dir=d)
    assert torch.load(os.path.join(d, "last.pt"), weights_only=True)["epoch"] == 5
    tr3 = _trainer(seed=3, lr=5.0)
    assert tr3.fit([], 8, warmup_epochs=3, min_lr=1e-5, checkpoint_dir=d, resume=True) == hist
    assert tr3.lr == tr.lr


def test_fit_argument_checks():
    tr = _trainer()
    with pytest.raises(ValueError):
        tr.fit([], 3, warmup_epochs=3)
    with pytest.raises(ValueError):
        tr.fit([], 5, resume=True)
    with pytest.raises(ValueError):
        tr.fit([], 5, eval_every=0)
