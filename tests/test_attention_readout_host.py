"""CPU: the attention read-out validates before it touches a device - the three C entry points (the library loads
without a GPU, as in test_abi_and_host.py::test_argument_errors_are_reported_not_crashed), ops.encoder_attention's
refusals, and the ERP encoder's token -> sample spreading rule."""
import ctypes

import pytest
import torch

import multimodal_eeg_fmri_amd.crossmodal_v4_enhancements as Cv
import multimodal_eeg_fmri_amd.enhanced_models_v4 as E
from multimodal_eeg_fmri_amd import _hip, ops

P = ctypes.c_void_p(8)          # a non-null pointer no entry point may dereference before it has validated


def test_entry_points_validate_without_a_device():
    lib = _hip.load()
    assert _hip._SIGS["mm_attn_weights"] == "pppiiiifpii" and _hip._SIGS["mm_attn_received"] == "pppfppiiiifpi"
    assert _hip._SIGS["mm_attn_received_ws_floats"] == "iiip"

    def weights(qkv=P, lse=P, w=P, B=1, L=16, H=4, dh=32, per_head=0):
        return lib.mm_attn_weights(qkv, lse, w, B, L, H, dh, 0.1, None, 0, per_head, None)

    def received(qkv=P, lse=P, out=P, ws=P, B=1, L=16, H=4, dh=32, sw=0.0):
        return lib.mm_attn_received(qkv, lse, None, sw, out, ws, B, L, H, dh, 0.1, None, 0, None)
    for fn, name in ((weights, b"attn_weights"), (received, b"attn_received")):
        for dh in (20, 72, 8, 0):
            assert fn(dh=dh) == -1
            assert name + b": head_dim" in lib.mm_last_error()
        for kw in (dict(L=0), dict(B=0), dict(H=0), dict(qkv=None), dict(lse=None)):
            assert fn(**kw) == -1
            assert name + b": null/invalid" in lib.mm_last_error()
    assert weights(w=None) == -1 and b"attn_weights: null/invalid" in lib.mm_last_error()
    assert received(out=None) == -1 and b"attn_received: null/invalid" in lib.mm_last_error()
    assert received(ws=None) == -1 and b"attn_received: null ws" in lib.mm_last_error()
    for ph in (2, -1):
        assert weights(per_head=ph) == -1 and b"attn_weights: per_head" in lib.mm_last_error()
    for sw in (-0.01, 1.01, float("nan"), float("inf")):
        assert received(sw=sw) == -1 and b"attn_received: self_weight" in lib.mm_last_error()
    assert weights(B=70000) == -1 and b"launch grid" in lib.mm_last_error()
    n = ctypes.c_int(-1)
    assert lib.mm_attn_received_ws_floats(3, 130, 4, ctypes.addressof(n), None) == 0 and n.value == 3 * 130 * 4
    assert lib.mm_attn_received_ws_floats(3, 130, 4, None, None) == -1 and b"attn_received_ws_floats" in lib.mm_last_error()
    assert lib.mm_attn_received_ws_floats(3, 0, 4, ctypes.addressof(n), None) == -1
    assert lib.mm_attn_received_ws_floats(1 << 15, 1 << 15, 4, ctypes.addressof(n), None) == -1 and b"overflows" in lib.mm_last_error()


def test_encoder_attention_refusals():
    x = torch.randn(2, 8, 64)
    erp = E.EnhancedERPEncoder(8, 64, 2, 4)
    with pytest.raises(ValueError, match="unknown method 'gradcam'"):
        ops.encoder_attention(erp, x, "gradcam")
    for layer in (2, -1, 7):
        with pytest.raises(ValueError, match="out of range for 2 transformer layers"):
            ops.encoder_attention(erp, x, "received", layer=layer)
    with pytest.raises(ValueError, match="layer applies to method 'received'"):
        ops.encoder_attention(erp, x, "rollout", layer=0)
    for enc in (E.EnhancedERPEncoder(8, 64, 0, 4), E.EnhancedPowerEncoder(8, 64, 0, 4),
                Cv.MultiScaleSTFTPowerEncoder(2, hidden_dim=64, num_transformer_layers=0)):
        with pytest.raises(ValueError, match=f"{type(enc).__name__} has no transformer layers"):
            ops.encoder_attention(enc, x, "rollout")
        with pytest.raises(ValueError, match="no transformer layers"):
            enc.temporal_attention(x)
        with pytest.raises(ValueError, match="no transformer layers"):
            enc.attention_maps(x)
    for other in (torch.nn.Linear(4, 4), Cv.LiteERPEncoder(8, 64, 0.1)):
        with pytest.raises(ValueError, match=type(other).__name__):
            ops.encoder_attention(other, x, "rollout")
    with pytest.raises(ValueError, match="call attention_maps"):
        erp.temporal_attention(x, method="maps")
    with pytest.raises(_hip.HipLibraryError, match="CPU tensor"):      # everything valid: only the device is missing
        ops.encoder_attention(erp, x, "rollout")
    assert erp.training                                                # nothing flipped on the way


def test_host_ops_validate_before_a_launch():
    qkv = torch.zeros(2, 16, 3 * 128, dtype=torch.bfloat16)
    lse = torch.zeros(2, 4, 16)
    with pytest.raises(ValueError, match="head dim"):
        ops.attention_weights(torch.zeros(2, 16, 3 * 80, dtype=torch.bfloat16), lse, 4)          # head dim 20
    with pytest.raises(ValueError, match="bf16"):
        ops.attention_weights(qkv.float(), lse, 4)
    with pytest.raises(ValueError, match="lse must be fp32"):
        ops.attention_received(qkv, lse[:, :2], 4)
    with pytest.raises(ValueError, match="batch \\* heads"):
        ops.attention_weights(qkv, lse, 4, mask=torch.zeros(4, 16, 16))
    with pytest.raises(ValueError, match="expected \\(L, L\\)"):
        ops.attention_received(qkv, lse, 4, mask=torch.zeros(15, 16))
    with pytest.raises(ValueError, match="self_weight"):
        ops.attention_received(qkv, lse, 4, self_weight=-0.5)
    with pytest.raises(_hip.HipLibraryError, match="CPU tensor"):
        ops.attention_weights(qkv, lse, 4)


def test_erp_time_spreads_each_token_over_its_pooled_pair():
    tok = torch.tensor([[1.0, 2.0, 4.0], [0.5, 0.0, 0.25]])
    even = ops.spread_pooled_tokens(tok, 6)
    assert torch.equal(even, torch.tensor([[0.5, 0.5, 1.0, 1.0, 2.0, 2.0], [0.25, 0.25, 0.0, 0.0, 0.125, 0.125]]))
    odd = ops.spread_pooled_tokens(tok, 7)
    assert odd.shape == (2, 7) and torch.equal(odd[:, :6], even) and torch.all(odd[:, 6] == 0)
    assert torch.equal(even.sum(1), tok.sum(1)) and torch.equal(odd.sum(1), tok.sum(1))
    with pytest.raises(ValueError, match="3 tokens do not come from 9 samples"):
        ops.spread_pooled_tokens(tok, 9)
    erp, pw = E.EnhancedERPEncoder(8, 64, 2, 4), E.EnhancedPowerEncoder(8, 64, 2, 4)
    stft = Cv.MultiScaleSTFTPowerEncoder(2, n_ffts=(32,), hop=16, hidden_dim=64)
    assert [ops.encoder_tokens(erp, t) for t in (64, 65, 66)] == [32, 32, 33]
    assert ops.encoder_tokens(pw, 65) == 65 and ops.encoder_tokens(stft, 64) == 5
