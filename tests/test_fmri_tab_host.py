"""Host side of the tabular fMRI encoder (`fmri_utils.fMRITabularEncoder`) and of a `BridgeTrainer` built on it: state
dict keys and the copy of a trained `fMRIFusionNet`, every argument check that must fire before a launch, the two
entry points' declarations, and the bucket layout of a CPU-built trainer."""
import inspect

import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
from multimodal_eeg_fmri_amd.bridge_branches import step_schedule
from multimodal_eeg_fmri_amd.bridge_trainer import (BridgeTrainer, synthetic_tabular_pairs,
                                                    synthetic_tabular_subject_pairs)
from multimodal_eeg_fmri_amd.fmri_utils import fMRIFusionNet, fMRITabularEncoder


def _cpu_trainer(enc=None, **kw):
    torch.manual_seed(0)
    return BridgeTrainer(eeg_channels=8, device="cpu", fmri_encoder=enc, **kw)


def test_state_dict_keys_are_the_fusion_nets_without_the_head():
    torch.manual_seed(1)
    net = fMRIFusionNet(37, 50, hidden_dim=64, num_classes=3, dropout=0.4)
    enc = fMRITabularEncoder(37, 50, hidden_dim=64, dropout=0.4)
    want = [k for k in net.state_dict() if not k.startswith("head.")]
    assert list(enc.state_dict()) == want and len(want) == 2 + 5 * 7
    res = enc.load_state_dict(net.state_dict(), strict=False)
    assert not res.missing_keys and sorted(res.unexpected_keys) == sorted(k for k in net.state_dict() if k.startswith("head."))
    assert [n for n, _ in enc.named_buffers()] == [n for n, _ in net.named_buffers()]       # the ticket words are no buffer


def test_from_fusion_net_copies_a_trained_net():
    torch.manual_seed(2)
    net = fMRIFusionNet(5, 9, hidden_dim=32, dropout=0.25).eval()
    with torch.no_grad():
        for q in net.parameters():
            q.add_(torch.randn_like(q) * 0.1)
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.uniform_(-1, 1)
                m.running_var.uniform_(0.5, 2)
                m.num_batches_tracked.fill_(7)
    enc = fMRITabularEncoder.from_fusion_net(net)
    assert (enc.activation_dim, enc.connectivity_dim, enc.hidden_dim, enc.drop_p) == (5, 9, 32, 0.25)
    assert not enc.training and enc.in_dim == 14
    sd = net.state_dict()
    for k, v in enc.state_dict().items():
        assert torch.equal(v, sd[k]) and v.data_ptr() != sd[k].data_ptr(), k
    assert enc.get_fusion_weights() == net.get_fusion_weights()
    assert fMRITabularEncoder.from_fusion_net(net.train()).training
    assert [type(l).__name__ + type(b).__name__ for l, b in enc.layers()] == ["LinearBatchNorm1d"] * 5
    assert [l.weight.shape for l, _ in enc.layers()] == [(64, 5), (32, 64), (64, 9), (32, 64), (32, 64)]


def test_split_gives_the_two_halves():
    enc = fMRITabularEncoder(3, 4, hidden_dim=32)
    x = torch.arange(14.0).view(2, 7)
    act, conn = enc.split(x)
    assert torch.equal(act, x[:, :3]) and torch.equal(conn, x[:, 3:]) and act.data_ptr() == x.data_ptr()


@pytest.mark.parametrize("hidden", [16, 48, 96, 256])
def test_hidden_dim_outside_the_served_set_is_refused(hidden):
    with pytest.raises(ValueError, match="hidden_dim"):
        fMRITabularEncoder(10, 10, hidden_dim=hidden)


def test_input_dims_and_dropout_are_checked():
    with pytest.raises(ValueError, match="activation_dim"):
        fMRITabularEncoder(0, 10)
    with pytest.raises(ValueError, match="connectivity_dim"):
        fMRITabularEncoder(10, 0)
    with pytest.raises(ValueError, match="dropout"):
        fMRITabularEncoder(10, 10, dropout=1.0)
    fMRITabularEncoder(1, 1, hidden_dim=128)


def test_module_checks_the_input_before_any_launch():
    enc = fMRITabularEncoder(7, 3, hidden_dim=32).train()
    with pytest.raises(ValueError, match=r"\(B, 10\)"):
        enc(torch.zeros(4, 11))                                # wrong width
    with pytest.raises(ValueError, match=r"\(B, 10\)"):
        enc(torch.zeros(4, 1, 10))
    with pytest.raises(ValueError, match="2 <= B <= 256"):
        enc(torch.zeros(1, 10))
    with pytest.raises(ValueError, match="2 <= B <= 256"):
        enc(torch.zeros(257, 10))
    with pytest.raises(_hip.HipLibraryError, match="CPU tensor"):
        enc(torch.zeros(4, 10))                                # a good shape on the host: no CPU path
    with pytest.raises(_hip.HipLibraryError, match="CPU tensor"):
        enc.eval()(torch.zeros(1, 10))                         # eval mode takes B = 1 ...
    with pytest.raises(_hip.HipLibraryError, match="CPU tensor"):
        enc.eval()(torch.zeros(300, 10))                       # ... and more than 256 rows


def test_trainer_constructor_rules():
    with pytest.raises(TypeError, match="fMRITabularEncoder"):
        _cpu_trainer(torch.nn.Linear(4, 64))
    with pytest.raises(TypeError, match="fMRITabularEncoder"):
        _cpu_trainer(fMRIFusionNet(4, 4))
    with pytest.raises(ValueError, match="fmri_dim"):
        _cpu_trainer(fMRITabularEncoder(4, 4, hidden_dim=32))              # fmri_dim defaults to 64
    with pytest.raises(ValueError, match="fmri_dim"):
        _cpu_trainer(fMRITabularEncoder(4, 4, hidden_dim=64), fmri_dim=128)
    tr = _cpu_trainer(fMRITabularEncoder(4, 4, hidden_dim=32), fmri_dim=32)
    assert tr._fmri_kind == "tabular" and _cpu_trainer()._fmri_kind == "volume"
    assert inspect.signature(BridgeTrainer.__init__).parameters["fmri_encoder"].default is None


@pytest.mark.parametrize("mode", ["graph", "manual", "autograd"])
def test_trainer_checks_the_fmri_batch_before_any_launch(mode):
    tab = _cpu_trainer(fMRITabularEncoder(37, 50), mode=mode)
    vol = _cpu_trainer(mode=mode)
    eeg = torch.zeros(4, 8, 64)
    with pytest.raises(ValueError, match=r"\(B, 87\)"):
        tab.train_step(eeg, torch.zeros(4, 1, 16, 16, 16))     # a volume batch for a tabular trainer
    with pytest.raises(ValueError, match=r"\(B, 87\)"):
        tab.train_step(eeg, torch.zeros(4, 86))
    with pytest.raises(ValueError, match="volume batch"):
        vol.train_step(eeg, torch.zeros(4, 87))                # a tabular batch for the voxel trainer
    with pytest.raises(ValueError, match="2 <= B <= 256"):
        tab.train_step(torch.zeros(1, 8, 64), torch.zeros(1, 87))
    with pytest.raises(ValueError, match="2 <= B <= 256"):
        tab.train_step(torch.zeros(257, 8, 64), torch.zeros(257, 87))
    for fn in (tab.evaluate, tab.explain):
        with pytest.raises(ValueError, match=r"\(B, 87\)"):
            fn(eeg, torch.zeros(4, 1, 16, 16, 16))
    with pytest.raises(ValueError, match=r"\(B, 87\)"):
        tab.predict(eeg, torch.zeros(4, 88))
    assert tab._cap is None and vol._cap is None


def test_header_declares_the_entry_points_and_hip_maps_them():
    sigs = _hip.parse_header()
    fwd, bwd = sigs["mm_fmri_tab_fwd"], sigs["mm_fmri_tab_bwd"]
    # x, four sizes, 5 x 7 layer pointers, the two scalars, out, save, tickets, train, eps, momentum, drop_p, 5 seeds, epoch
    assert fwd == "p" + "iiii" + "p" * 35 + "pp" + "ppp" + "i" + "fff" + "uuuuu" + "p"
    # dout, x, out, save, four sizes, 5 x (w, gamma), the two scalars, scratch, dx, 5 x 4 + 2 destinations, train, eps, drop_p
    assert bwd == "pppp" + "iiii" + "p" * 10 + "pp" + "pp" + "p" * 22 + "i" + "ff"
    assert _hip.header_abi_version() == 5                       # new entry points: nothing that remains changed
    from multimodal_eeg_fmri_amd import autograd
    src = inspect.getsource(ops._tab_forward_impl) + inspect.getsource(autograd.fmri_tab_bwd)
    assert '"mm_fmri_tab_fwd"' in src and '"mm_fmri_tab_bwd"' in src
    lib = _hip.load()
    assert hasattr(lib, "mm_fmri_tab_fwd") and hasattr(lib, "mm_fmri_tab_bwd")
    assert len(lib.mm_fmri_tab_fwd.argtypes) == len(fwd) + 1 and len(lib.mm_fmri_tab_bwd.argtypes) == len(bwd) + 1


def test_workspace_sizes():
    assert ops.fmri_tab_save_floats(32, 64) == 13 * 32 * 64 + 14 * 64
    assert ops.fmri_tab_scratch_floats(32, 100, 200, 64) == (2 + 4 + 3) * 4 * 32 * 64
    assert ops.fmri_tab_scratch_floats(2, 1, 64, 32) == (1 + 1 + 3) * 4 * 2 * 32
    assert ops.fmri_tab_scratch_floats(2, 65, 129, 32) == (2 + 3 + 3) * 4 * 2 * 32


@pytest.mark.parametrize("kw", [{}, {"loss": "sigmoid"}, {"classify": True}], ids=["infonce", "sigmoid", "classify"])
def test_cpu_trainer_bucket_layout(kw):
    enc = fMRITabularEncoder(37, 50, hidden_dim=64, dropout=0.0)
    tab, vol = _cpu_trainer(enc, **kw), _cpu_trainer(**kw)
    assert [g[:2] for g in tab.groups] == [g[:2] for g in vol.groups]
    assert tab.groups[:-1] == vol.groups[:-1]                   # the EEG side of the bucket is where it was
    name, ready, lo, hi = tab.groups[-1]
    n_enc = sum(q.numel() for q in enc.parameters())
    assert (name, ready) == ("fmri encoder", "fmri") and hi - lo == n_enc and hi == tab.bucket.n and lo == tab.fmri_lo
    assert n_enc == (37 * 128 + 128 * 3) + (128 * 64 + 64 * 3) + (50 * 128 + 128 * 3) + (128 * 64 + 64 * 3) + (128 * 64 + 64 * 3) + 2
    assert tab.fmri_encoder is enc
    for q in enc.parameters():                                  # every parameter and its gradient sink live in the bucket
        assert q._mm_grad.shape == q.shape
        assert tab.bucket.p.data_ptr() <= q.data_ptr() < tab.bucket.p.data_ptr() + 4 * tab.bucket.n
    keys = set(tab.state_dict())
    assert {k for k in keys if k.startswith("fmri_encoder.")} == {"fmri_encoder." + k for k in enc.state_dict()}
    assert {k for k in keys if not k.startswith("fmri_encoder.")} == {k for k in vol.state_dict() if not k.startswith("fmri_encoder.")}
    assert not step_schedule("erp", "tabular", (), (87,), True, {}).fmri_first
    assert not step_schedule("erp", "volume", (), (1, 16, 16, 16), True, {}).fmri_first


def test_synthetic_tabular_helpers():
    eeg, fmri = synthetic_tabular_pairs(6, 8, 64, 37, 50, seed=3, device="cpu")
    assert eeg.shape == (6, 8, 64) and fmri.shape == (6, 87) and fmri.dtype == torch.float32
    eeg2, fmri2 = synthetic_tabular_pairs(6, 8, 64, 37, 50, seed=3, device="cpu")
    assert torch.equal(eeg, eeg2) and torch.equal(fmri, fmri2)
    assert not torch.equal(fmri, synthetic_tabular_pairs(6, 8, 64, 37, 50, seed=4, device="cpu")[1])
    e, f, g = synthetic_tabular_subject_pairs(3, 4, 8, 64, 37, 50, seed=5, device="cpu")
    assert e.shape == (12, 8, 64) and f.shape == (12, 87) and g.dtype == torch.int32
    assert g.tolist() == [0] * 4 + [1] * 4 + [2] * 4
    assert torch.equal(f[0], f[3]) and not torch.equal(f[3], f[4]) and not torch.equal(e[0], e[1])
    with pytest.raises(ValueError, match="subjects"):
        synthetic_tabular_subject_pairs(0, 4, device="cpu")
