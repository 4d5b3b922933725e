"""Host side of `bridge_branches`: the step schedule as a table (`step_schedule`, pinned the way
test_block_plan_host.py pins `ops.block_plan`), which entry of the two branch tables every encoder type selects, the
bucket groups of a CPU-built trainer per EEG kind, and the byte layout of a captured step's static inputs."""
import pytest
import torch

from multimodal_eeg_fmri_amd import ops
from multimodal_eeg_fmri_amd.bridge_branches import (EEG_BRANCHES, FMRI_BRANCHES, StepSchedule, input_layout, select_eeg,
                                                     select_fmri, step_schedule)
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer
from multimodal_eeg_fmri_amd.crossmodal_v4_enhancements import MultiScaleSTFTPowerEncoder
from multimodal_eeg_fmri_amd.enhanced_models_v4 import EnhancedERPEncoder, EnhancedPowerEncoder
from multimodal_eeg_fmri_amd.fmri_utils import fMRIFusionNet, fMRITabularEncoder

HAND_ORDER = (("fmri", "side"), ("handed0", "side"), ("handed1", "side"), ("main", "main"))
PLAIN_ORDER = (("handed0", "main"), ("handed1", "main"), ("main", "main"), ("fmri", "side"))
V32, BIG, BELOW, TAB = (1, 32, 32, 32), (1, 64, 64, 32), (1, 64, 64, 31), (87,)
EEG, FMRI = ("eeg_encoder",), ("fmri_encoder",)

# (EEG kind, fMRI kind, per-sample shape, frozen, fused rows, env) -> (fmri_first, hand, handed_convs); None = not pinned
ROWS = [
    ("erp", "volume", V32, (), True, {}, (False, True, 0)),
    ("erp", "volume", V32, (), False, {}, (False, True, 1)),
    ("erp", "volume", BIG, (), True, {}, (True, False, 0)),                 # exactly 4 * 32^3 voxels
    ("erp", "volume", BIG, (), False, {}, (True, False, 0)),
    ("erp", "volume", BELOW, (), True, {}, (False, None, None)),
    ("erp", "volume", BIG, (), True, {"MM_FMRI_LONGER": "0"}, (False, True, 0)),
    ("erp", "volume", V32, (), True, {"MM_FMRI_LONGER": "1"}, (True, False, 0)),
    ("erp", "tabular", TAB, (), True, {"MM_FMRI_LONGER": "1"}, (False, True, 0)),
    ("erp", "tabular", TAB, (), False, {}, (False, True, 1)),
    ("erp", "volume", V32, (), True, {"MM_CONV_WGRADS_HANDED": "2"}, (False, True, 2)),
    ("erp", "volume", V32, (), False, {"MM_CONV_WGRADS_HANDED": "0"}, (False, True, 0)),
    ("erp", "volume", BIG, (), True, {"MM_CONV_WGRADS_HANDED": "2"}, (True, False, 0)),      # nothing is handed over
    ("erp", "volume", V32, EEG, True, {"MM_CONV_WGRADS_HANDED": "2"}, (False, False, 0)),
    ("erp", "volume", V32, EEG, True, {}, (False, False, 0)),
    ("erp", "volume", V32, FMRI, True, {}, (False, True, 0)),
    ("erp", "volume", BIG, EEG + FMRI, False, {}, (True, False, 0)),
    ("power", "volume", V32, (), False, {}, (False, True, 1)),
    ("power", "volume", V32, (), True, {}, (False, True, 1)),               # only the ERP chain's default depends on it
    ("stft", "volume", V32, (), True, {}, (False, True, 1)),
    ("stft", "tabular", TAB, (), True, {}, (False, True, 1)),
    ("power", "volume", V32, (), True, {"MM_CONV_WGRADS_HANDED": "2"}, (False, True, 2)),
    ("power", "volume", BIG, (), True, {}, (True, False, 0)),
]


@pytest.mark.parametrize("eeg,fmri,shape,frozen,fused,env,want", ROWS)
def test_schedule_table(eeg, fmri, shape, frozen, fused, env, want):
    s = step_schedule(eeg, fmri, frozen, shape, fused, env)
    assert isinstance(s, StepSchedule)
    for got, w in zip((s.fmri_first, s.hand, s.handed_convs), want):
        assert w is None or (got == w and type(got) is type(w)), (s, want)
    assert s.eeg_live == ("eeg_encoder" not in frozen) and s.fmri_live == ("fmri_encoder" not in frozen)
    assert s.hand == (not s.fmri_first and s.eeg_live)
    assert s.handed_convs == 0 or s.hand
    assert s.reduce_order == (HAND_ORDER if s.hand else PLAIN_ORDER)


def test_schedule_reads_only_the_mapping_it_is_given(monkeypatch):
    monkeypatch.setenv("MM_FMRI_LONGER", "1")
    monkeypatch.setenv("MM_CONV_WGRADS_HANDED", "2")
    s = step_schedule("erp", "volume", (), V32, True, {})
    assert (s.fmri_first, s.hand, s.handed_convs) == (False, True, 0)


def _cpu_trainer(**kw):
    torch.manual_seed(0)
    return BridgeTrainer(**{"eeg_channels": 8, "device": "cpu", **kw})


def _eeg_encoder(kind):
    return {"erp": lambda: None, "power": lambda: EnhancedPowerEncoder(8, 128, 2, 4, 0.0),
            "stft": lambda: MultiScaleSTFTPowerEncoder(8, (16, 32), 8, 128, 2, 4, 0.0)}[kind]()


def test_every_encoder_type_selects_its_entry():
    assert select_eeg(EnhancedERPEncoder(8, 128, 2, 4, 0.0)) is EEG_BRANCHES["erp"]
    assert select_eeg(_eeg_encoder("power")) is EEG_BRANCHES["power"]
    assert select_eeg(_eeg_encoder("stft")) is EEG_BRANCHES["stft"]
    assert sorted(EEG_BRANCHES) == ["erp", "power", "stft"] and all(k == b.kind for k, b in EEG_BRANCHES.items())
    assert [k for k, b in EEG_BRANCHES.items() if b.raw_input] == ["stft"]
    assert [k for k, b in EEG_BRANCHES.items() if b.hands_over] == ["erp"]
    enc = fMRITabularEncoder(4, 4, hidden_dim=64)
    assert select_fmri(None, 64) is FMRI_BRANCHES["volume"] and select_fmri(enc, 64) is FMRI_BRANCHES["tabular"]
    assert list(FMRI_BRANCHES) == ["volume", "tabular"]
    assert [b.can_be_longer for b in FMRI_BRANCHES.values()] == [True, False]
    assert [b.augmentable for b in FMRI_BRANCHES.values()] == [True, False]
    assert [b.perturb_default for b in FMRI_BRANCHES.values()] == [("blocks", 8), ("windows", 1)]
    with pytest.raises(TypeError, match="no tape for an EEG encoder of type Linear"):
        select_eeg(torch.nn.Linear(4, 4))
    with pytest.raises(TypeError, match="no tape for an EEG encoder of type Linear"):
        _cpu_trainer(eeg_encoder=torch.nn.Linear(4, 4))
    with pytest.raises(TypeError, match=r"fmri_encoder must be an fMRITabularEncoder or None \(the voxel encoder\), got fMRIFusionNet"):
        _cpu_trainer(fmri_encoder=fMRIFusionNet(4, 4))
    with pytest.raises(ValueError, match="fmri_dim=64 but the fMRITabularEncoder ends in 32 features"):
        _cpu_trainer(fmri_encoder=fMRITabularEncoder(4, 4, hidden_dim=32))
    from multimodal_eeg_fmri_amd.fmri_utils import VolumeTransforms
    with pytest.raises(ValueError, match="fmri_augment augments"):
        _cpu_trainer(fmri_encoder=enc, fmri_augment=VolumeTransforms())


ERP_GROUPS = [("eeg conv block 1", "main"), ("eeg conv blocks 2-3", "handed1"), ("eeg transformer stack + heads", "handed0"),
              ("fmri encoder", "fmri")]
ONE_GROUP = [("eeg encoder + heads", "main"), ("fmri encoder", "fmri")]


@pytest.mark.parametrize("kind", ["erp", "power", "stft"])
@pytest.mark.parametrize("fmri", ["volume", "tabular"])
def test_bucket_groups_per_eeg_kind(kind, fmri):
    def enc_f():
        return fMRITabularEncoder(37, 50, hidden_dim=64, dropout=0.0) if fmri == "tabular" else None
    tr = _cpu_trainer(eeg_encoder=_eeg_encoder(kind), fmri_encoder=enc_f())
    assert (tr._eeg_kind, tr._fmri_kind) == (kind, fmri)
    assert [g[:2] for g in tr.groups] == (ERP_GROUPS if kind == "erp" else ONE_GROUP)
    n_e = sum(p.numel() for p in tr.eeg_encoder.parameters())
    n_f = sum(p.numel() for p in tr.fmri_encoder.parameters())
    n_h = tr.bucket.n - n_e - n_f
    assert n_h > 0 and tr.groups[0][2] == 0 and tr.groups[-1][2:] == (tr.fmri_lo, tr.bucket.n) and tr.bucket.n - tr.fmri_lo == n_f
    assert all(a[3] == b[2] for a, b in zip(tr.groups, tr.groups[1:]))          # contiguous, in bucket order
    if kind == "erp":
        cl = tr.eeg_encoder.conv_layers
        size = lambda idx: sum(p.numel() for i in idx for p in cl[i].parameters())  # noqa: E731
        assert [g[3] - g[2] for g in tr.groups[:2]] == [size((0, 1)), size((4, 5, 9, 10))]
    fz = _cpu_trainer(eeg_encoder=_eeg_encoder(kind), fmri_encoder=enc_f(), freeze=("eeg_encoder",))
    assert [g[:2] for g in fz.groups] == [("heads", "main"), ("fmri encoder", "fmri")]
    assert fz.groups[0][2:] == (0, n_h) and fz.bucket.n == n_h + n_f and fz._eeg_kind == kind


@pytest.mark.parametrize("kind", ["erp", "stft"])
def test_input_layout_is_the_captures_and_the_host_packers(kind):
    B, C, T, vol = 4, 6, 64, (1, 8, 8, 8)
    tr = _cpu_trainer(eeg_encoder=_eeg_encoder(kind) if kind == "stft" else None, eeg_channels=6)
    n_e = B * C * T * 4 if kind == "stft" else B * T * ops.cpad(C) * 2      # raw fp32, else the packed bf16 (B, T, Cp) operand
    n_f = B * 8 ** 3 * 4
    assert ops.cpad(C) > C
    assert input_layout(tr._eeg, (B, C, T), B * 8 ** 3, False) == (n_e, n_f, 0, 0)                 # plain
    assert input_layout(tr._eeg, (B, C, T), B * 8 ** 3, True) == (n_e, n_f, 4 * B, 0)              # grouped
    assert input_layout(tr._eeg, (B, C, T), B * 8 ** 3, False, True) == (n_e, n_f, 0, 4 * B)       # labelled
    assert input_layout(tr._eeg, (B, C, T), B * 8 ** 3, True, True) == (n_e, n_f, 4 * B, 4 * B)
    # the shape of test_trainer_gpu.py's packed step
    assert sum(input_layout(EEG_BRANCHES["erp"], (8, 16, 256), 8 * 16 ** 3, False)) == 8 * 256 * 16 * 2 + 8 * 16 ** 3 * 4
    g = torch.Generator().manual_seed(3)
    eeg, fmri = torch.randn(B, C, T, generator=g), torch.randn(B, *vol, generator=g)
    gid = torch.tensor([0, 0, 1, 1], dtype=torch.int32)
    for groups in (None, gid):
        n = n_e + n_f + (4 * B if groups is not None else 0)
        out = tr.pack_host_batch(eeg, fmri, out=torch.full((n + 8,), 0xAB, dtype=torch.uint8), groups=groups)
        assert bool((out[n:] == 0xAB).all())                                 # exactly n bytes written
        assert torch.equal(out[n_e:n_e + n_f].view(torch.float32).view(fmri.shape), fmri)
        if groups is not None:
            assert torch.equal(out[n_e + n_f:n].view(torch.int32), gid)
        if kind == "stft":
            assert torch.equal(out[:n_e].view(torch.float32).view(eeg.shape), eeg)
        else:
            xb = out[:n_e].view(torch.bfloat16).view(B, T, ops.cpad(C))
            assert torch.equal(xb[:, :, :C], eeg.permute(0, 2, 1).to(torch.bfloat16)) and not xb[:, :, C:].any()
