"""CPU: the head-dim-generic attention entry points refuse what they do not run before anything launches (null pointers
only: nothing can ever reach the device), ops picks the entry point by head dim and refuses an unsupported
(d_model, nhead) with ValueError, and BridgeTrainer builds at any width and records its head counts in checkpoints."""
import ctypes

import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer
from multimodal_eeg_fmri_amd.enhanced_models_v4 import EnhancedERPEncoder, TemporalTransformerBlock


def _fwd(lib, dh):
    return lib.mm_attn_fwd_hd(None, None, None, 1, 16, 4, dh, ctypes.c_float(0.25), ctypes.c_float(0.0), 0, None, None, 0,
                              None)


def _bwd(lib, dh):
    return lib.mm_attn_bwd_hd(None, None, None, None, None, None, 1, 16, 4, dh, ctypes.c_float(0.25), ctypes.c_float(0.0),
                              0, None, None, 0, None)


@pytest.mark.parametrize("dh", [0, 8, 12, 20, 63, 72, 128])
def test_hd_entry_points_refuse_unsupported_head_dims(dh):
    lib = _hip.load()
    for call in (_fwd, _bwd):
        assert call(lib, dh) == -1
        assert b"head_dim" in lib.mm_last_error()


@pytest.mark.parametrize("dh", [16, 24, 32, 40, 48, 56, 64])
def test_hd_entry_points_refuse_null_pointers_at_supported_head_dims(dh):
    lib = _hip.load()
    for call in (_fwd, _bwd):
        assert call(lib, dh) == -1
        assert b"null" in lib.mm_last_error()


def test_hd_entry_points_refuse_a_bad_dropout_rate():
    lib = _hip.load()
    rc = lib.mm_attn_fwd_hd(None, None, None, 1, 16, 4, 32, ctypes.c_float(0.25), ctypes.c_float(1.0), 0, None, None, 0,
                            None)
    assert rc == -1 and b"drop_p" in lib.mm_last_error()


def test_entry_point_by_head_dim():
    assert ops.ATTN_HEAD_DIMS == (16, 24, 32, 40, 48, 56, 64)
    assert ops.attn_entry(128, 4, "fwd") == "mm_attn_fwd" and ops.attn_entry(128, 4, "bwd") == "mm_attn_bwd"
    assert ops.attn_entry(64, 2, "fwd") == "mm_attn_fwd"
    for d, h in ((64, 4), (96, 4), (256, 4), (128, 8), (512, 8), (160, 4), (48, 2), (56, 1)):
        assert ops.attn_entry(d, h, "fwd") == "mm_attn_fwd_hd"
        assert ops.attn_entry(d, h, "bwd") == "mm_attn_bwd_hd"


@pytest.mark.parametrize("d,h", [(64, 8), (128, 16), (96, 5), (512, 4), (100, 4), (72, 1), (64, 0)])
def test_unsupported_width_raises_value_error_before_launch(d, h):
    with pytest.raises(ValueError, match=r"supported head dims: 16, 24, 32, 40, 48, 56, 64") as e:
        ops.attn_entry(d, h, "fwd")
    assert f"({d}, {h})" in str(e.value)
    # ops.attention checks before it allocates or launches: a CPU tensor never reaches the library
    if h > 0 and d % h == 0:
        with pytest.raises(ValueError, match="head dim"):
            ops.attention(torch.zeros(1, 4, 3 * d, dtype=torch.bfloat16), h, True)


def test_models_of_any_shape_still_build_on_cpu():
    """no construction-time check: a model to load weights into builds for any shape torch accepts"""
    m = EnhancedERPEncoder(8, 64, 2, 8, 0.1)
    assert all(b.nhead == 8 for b in m.transformer_layers)
    TemporalTransformerBlock(96, nhead=12)


@pytest.mark.parametrize("hidden,heads,layers", [(64, 4, 2), (256, 4, 2), (128, 8, 2), (96, 4, 3), (128, 4, 1)])
def test_trainer_builds_at_width_with_consistent_bucket_and_groups(hidden, heads, layers):
    torch.manual_seed(0)
    tr = BridgeTrainer(eeg_channels=8, hidden_dim=hidden, num_heads=heads, num_layers=layers, device="cpu", mode="manual")
    enc = tr.eeg_encoder
    assert len(enc.transformer_layers) == layers and all(b.nhead == heads for b in enc.transformer_layers)
    assert enc.conv_layers[9].out_channels == hidden and enc.output_proj[2].out_features == hidden
    # groups tile the bucket in order; each holds exactly its layer group's trainable parameters
    off = 0
    for _, _, lo, hi in tr.groups:
        assert lo == off and hi >= lo
        off = hi
    assert off == tr.bucket.n
    cl = enc.conv_layers
    n_conv1 = sum(p.numel() for i in (0, 1) for p in cl[i].parameters())
    n_conv23 = sum(p.numel() for i in (4, 5, 9, 10) for p in cl[i].parameters())
    assert tr.groups[0][3] - tr.groups[0][2] == n_conv1
    assert tr.groups[1][3] - tr.groups[1][2] == n_conv23
    assert tr.groups[-1][3] - tr.groups[-1][2] == sum(p.numel() for p in tr.fmri_encoder.parameters())
    assert tr.bucket.n == sum(p.numel() for p in tr.parameters() if p.requires_grad)
    # every trainable parameter is a view of its slice of the bucket
    for _, _, p, sl in tr.optimizer_param_map():
        assert p.numel() == sl.stop - sl.start


def test_default_trainer_is_unchanged():
    torch.manual_seed(0)
    a = BridgeTrainer(eeg_channels=8, device="cpu", mode="manual")
    torch.manual_seed(0)
    b = BridgeTrainer(eeg_channels=8, device="cpu", mode="manual", num_heads=4, num_layers=2)
    assert a.groups == b.groups
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    assert [blk.nhead for blk in a.eeg_encoder.transformer_layers] == [4, 4]


def _trainer(heads, seed=0):
    torch.manual_seed(seed)
    return BridgeTrainer(eeg_channels=8, hidden_dim=128, num_heads=heads, device="cpu", mode="manual")


def test_checkpoint_records_head_counts_and_refuses_other_ones():
    ck = _trainer(8).checkpoint_state()
    assert ck["bridge_trainer_state"]["heads"] == [["eeg_encoder.transformer_layers.0", 8],
                                                   ["eeg_encoder.transformer_layers.1", 8]]
    tr = _trainer(4, seed=3)
    before = [t.clone() for t in (tr.bucket.p, tr.bucket.m, tr.bucket.v, tr.bucket.state)]
    with pytest.raises(ValueError, match="heads differ"):
        tr.load_checkpoint_state(ck)
    assert all(torch.equal(x, y) for x, y in zip(before, (tr.bucket.p, tr.bucket.m, tr.bucket.v, tr.bucket.state)))
    _trainer(8, seed=3).load_checkpoint_state(ck)


def test_checkpoint_without_head_counts_reads_as_four_heads():
    ck = _trainer(4).checkpoint_state()
    del ck["bridge_trainer_state"]["heads"]                  # a checkpoint written before the field existed
    tr = _trainer(4, seed=5)
    tr.load_checkpoint_state(ck)
    assert torch.equal(tr.bucket.p, _trainer(4).bucket.p)
    with pytest.raises(ValueError, match="heads differ"):
        _trainer(8, seed=5).load_checkpoint_state(ck)
