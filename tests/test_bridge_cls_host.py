"""Host side of the bridge's supervised classification objective: the header declares the new entry points and `_hip`
maps them, `ops.class_labels` and `ops.bridge_cls_check` reject what the kernels do not serve before any launch, and a
CPU-built `BridgeTrainer` shows the constructor / `train_step` rules, the bucket layout and the checkpoint container
with and without ``classify=True``."""
import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer

CLS_PARTS = ("cross_attn", "fusion", "classifier")


def _cpu_trainer(**kw):
    torch.manual_seed(0)
    return BridgeTrainer(eeg_channels=8, device="cpu", **kw)


def test_header_declares_the_entry_points_and_hip_maps_them():
    sigs = _hip.parse_header()
    for name in ("mm_bridge_cls_fwd", "mm_bridge_cls_bwd", "mm_proj_heads_bwd_da"):
        assert name in sigs, name
        assert set(sigs[name]) <= set("pifu"), (name, sigs[name])
    assert sigs["mm_proj_heads_bwd_da"] == "p" + sigs["mm_proj_heads_bwd"]          # one more input: da
    assert sigs["mm_bridge_cls_fwd"].count("u") == 5 and sigs["mm_bridge_cls_bwd"].count("u") == 3   # dropout seeds
    assert _hip.header_abi_version() == 5


def test_class_labels_converts_host_integers_and_rejects_the_rest():
    out = ops.class_labels(torch.tensor([0, 1, 1, 0], dtype=torch.int64), 4, 2)
    assert out.dtype == torch.int32 and out.tolist() == [0, 1, 1, 0]
    assert ops.class_labels(torch.tensor([2, 0], dtype=torch.uint8), 2, 3).dtype == torch.int32
    assert ops.class_labels(None, 4, 2) is None
    with pytest.raises(ValueError, match="integer"):
        ops.class_labels(torch.tensor([0.0, 1.0]), 2, 2)
    with pytest.raises(ValueError, match="shape"):
        ops.class_labels(torch.tensor([0, 1, 1]), 4, 2)
    with pytest.raises(ValueError, match="shape"):
        ops.class_labels(torch.zeros(4, 1, dtype=torch.int64), 4, 2)
    with pytest.raises(ValueError, match=r"\[0, 2\)"):
        ops.class_labels(torch.tensor([0, 2]), 2, 2)
    with pytest.raises(ValueError, match=r"\[0, 2\)"):
        ops.class_labels(torch.tensor([-1, 1]), 2, 2)
    with pytest.raises(ValueError, match="Tensor"):
        ops.class_labels([0, 1], 2, 2)


def test_shape_check_rejects_what_the_kernels_do_not_serve():
    ops.bridge_cls_check(128, 4, 2)
    ops.bridge_cls_check(32, 16, 16)
    ops.bridge_cls_check(256, 1, 2)
    for dim in (48, 16, 288):
        with pytest.raises(ValueError, match="bridge_dim"):
            ops.bridge_cls_check(dim, 4, 2)
    for heads in (5, 32, 0):
        with pytest.raises(ValueError, match="num_heads"):
            ops.bridge_cls_check(128, heads, 2)
    for classes in (1, 17):
        with pytest.raises(ValueError, match="num_classes"):
            ops.bridge_cls_check(128, 4, classes)


def test_constructor_and_train_step_rules():
    with pytest.raises(ValueError, match="class_weight"):
        _cpu_trainer(class_weight=[1.0, 2.0])                            # without classify
    with pytest.raises(ValueError, match="class_weight"):
        _cpu_trainer(classify=True, class_weight=[1.0, 2.0, 3.0])        # wrong length
    with pytest.raises(ValueError, match="num_classes"):
        _cpu_trainer(classify=True, num_classes=17)
    with pytest.raises(ValueError, match="bridge_dim"):
        _cpu_trainer(classify=True, bridge_dim=48)
    with pytest.raises(ValueError, match="ce_weight"):
        _cpu_trainer(classify=True, ce_weight=-1.0)
    eeg, fmri = torch.zeros(4, 8, 64), torch.zeros(4, 1, 16, 16, 16)
    lab = torch.tensor([0, 1, 0, 1])
    for mode in ("graph", "manual", "autograd"):
        tc = _cpu_trainer(classify=True, mode=mode)
        with pytest.raises(ValueError, match="labels"):
            tc.train_step(eeg, fmri)
        with pytest.raises(ValueError, match=r"\[0, 2\)"):
            tc.train_step(eeg, fmri, labels=torch.tensor([0, 1, 2, 1]))
        td = _cpu_trainer(mode=mode)
        with pytest.raises(ValueError, match="classify=True"):
            td.train_step(eeg, fmri, labels=lab)
    with pytest.raises(ValueError, match="labels"):
        _cpu_trainer(classify=True).evaluate(eeg, fmri)
    with pytest.raises(ValueError, match="classify=True"):
        _cpu_trainer().evaluate(eeg, fmri, labels=lab)
    with pytest.raises(ValueError, match="labels"):
        _cpu_trainer(classify=True).pack_host_batch(eeg, fmri)


def test_default_trainer_has_no_classify_state_and_trains_no_classifier_parameter():
    d = _cpu_trainer()
    assert "classify" not in d.checkpoint_state()["bridge_trainer_state"]
    names = [n for _, n, _, _ in d.optimizer_param_map()]
    assert not [n for n in names if any(part in n for part in CLS_PARTS)]
    assert d._scal.numel() == 4 and d.classify is False
    assert d.head.bridge.classifier[4].weight.shape[0] == 2


def test_classify_trainer_trains_the_whole_bridge_in_the_heads_group():
    d, c = _cpu_trainer(), _cpu_trainer(classify=True, num_classes=3, class_weight=[1.0, 2.0, 0.5], ce_weight=0.25)
    names = {n: sl for _, n, _, sl in c.optimizer_param_map()}
    cls = [n for n in names if any(part in n for part in CLS_PARTS)]
    want = [n for n, _ in c.head.bridge.named_parameters() if any(part in n for part in CLS_PARTS)]
    assert sorted(cls) == sorted("head.bridge." + n for n in want) and len(cls) == 16
    (name, _, lo, hi), = [g for g in c.groups if "heads" in g[0]]
    assert all(lo <= names[n].start and names[n].stop <= hi for n in cls), name
    assert c.bucket.n - d.bucket.n == sum(c.get_parameter(n).numel() for n in cls)
    assert c._scal.numel() == 9 and c.head.bridge.classifier[4].weight.shape[0] == 3
    st = c.checkpoint_state()["bridge_trainer_state"]["classify"]
    assert st == {"ce_weight": 0.25, "num_classes": 3, "class_weight": [1.0, 2.0, 0.5]}
    # the same modules in the same RNG order: the shared parameters start from the same values
    for (n1, p1), (n2, p2) in zip(d.named_parameters(), _cpu_trainer(classify=True).named_parameters()):
        assert n1 == n2 and torch.equal(p1, p2), n1


def test_checkpoint_compatibility_names_the_differing_field():
    c = _cpu_trainer(classify=True, ce_weight=0.5)
    sd = c.checkpoint_state()
    with pytest.raises(ValueError, match="ce_weight"):
        _cpu_trainer(classify=True, ce_weight=1.0)._check_compatible(sd)
    with pytest.raises(ValueError, match="class_weight"):
        _cpu_trainer(classify=True, ce_weight=0.5, class_weight=[1.0, 2.0])._check_compatible(sd)
    with pytest.raises(ValueError, match="classify"):
        _cpu_trainer()._check_compatible(sd)
    with pytest.raises(ValueError, match="classify"):
        c._check_compatible(_cpu_trainer().checkpoint_state())
    _cpu_trainer(classify=True, ce_weight=0.5)._check_compatible(sd)
