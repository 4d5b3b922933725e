"""GPU: `fMRISequenceEncoder3D` at B = 3, F = 3, volumes of 12 x 10 x 9 (odd extents, 9 volumes per batch).  The frame
encoder's part is the volume encoder's own kernels on the (B * F, 1, D, H, W) view, so it is compared bit for bit; the pool
on top is held to the bounds of tests/test_lagpool_kernels_gpu.py against the fp64 formulas; the frame encoder's parameter
gradients to the bound of the volume encoder's gradient tests (5e-2 rel-L2 per tensor, tests/test_models_gpu.py)."""
import copy
import math

import pytest
import torch

from multimodal_eeg_fmri_amd import ops
from multimodal_eeg_fmri_amd.fmri_utils import fMRISequenceEncoder3D, fMRIVolumeEncoder3D

pytestmark = pytest.mark.gpu

B, F, VOL = 3, 3, (12, 10, 9)
POOL_BOUNDS = {"out": 6.1e-7, "attw": 6.0e-7, "dx": 1.4e-5, "dq": 1e-4, "dc": 1e-4}      # test_lagpool_kernels_gpu.BOUNDS
VOLUME_GRAD_BOUND = 5e-2                                                               # test_volume_encoder_train_grads_vs_oracle


def rel_err(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _pool64(x, q, c, dout=None):
    """the pool's formulas in fp64 on fp32 inputs -> out, weights[, dx, dq, dc]"""
    x, q, c = x.double().cpu(), q.double().cpu(), c.double().cpu()
    r = 1.0 / math.sqrt(x.shape[2])
    a = torch.softmax(x @ q * r + c, dim=1)
    out = (a.unsqueeze(-1) * x).sum(dim=1)
    if dout is None:
        return out, a
    dout = dout.double().cpu()
    da = (x * dout.unsqueeze(1)).sum(dim=-1)
    ds = a * (da - (a * da).sum(dim=1, keepdim=True))
    dx = a.unsqueeze(-1) * dout.unsqueeze(1) + ds.unsqueeze(-1) * q * r
    return out, a, dx, (ds.unsqueeze(-1) * x).sum(dim=(0, 1)) * r, ds.sum(dim=0)


@pytest.fixture(scope="module")
def case():
    ops.set_seed_epoch(None)
    torch.manual_seed(3)
    seq = fMRISequenceEncoder3D(F, 64, dropout=0.0).cuda()
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        seq.lag_pool.query.copy_(torch.randn(64, generator=g))
        seq.lag_pool.lag_bias.copy_(torch.randn(F, generator=g))
    x = torch.randn(B, F, *VOL, generator=g).cuda()
    gy = torch.randn(B, 64, generator=g).cuda()
    return seq, x, gy


def test_eval_forward_is_the_frame_encoder_then_the_pool(case):
    seq, x, _ = case
    seq.eval()
    with torch.no_grad():
        out, w = seq(x, return_weights=True)
        feats = seq.frame_encoder(x.view(B * F, 1, *VOL)).view(B, F, 64)
        k_out, k_w = ops.lag_pool_fwd(feats, seq.lag_pool.query, seq.lag_pool.lag_bias)
    assert out.shape == (B, 64) and w.shape == (B, F)
    assert torch.equal(out, k_out) and torch.equal(w, k_w)                # the same kernels on the same view
    want_out, want_w = _pool64(feats, seq.lag_pool.query, seq.lag_pool.lag_bias)
    assert rel_err(out, want_out) <= POOL_BOUNDS["out"], rel_err(out, want_out)
    assert rel_err(w, want_w) <= POOL_BOUNDS["attw"], rel_err(w, want_w)
    assert torch.equal(seq.lag_weights(x), w) and not seq.training
    with torch.no_grad():
        assert torch.equal(seq(x), out)
    seq.train()
    assert torch.equal(seq.lag_weights(x), w) and seq.training and seq.frame_encoder.training      # flags put back


def test_train_backward_is_the_pool_then_the_volume_encoders(case):
    seq, x, gy = case
    seq.train()
    vol = copy.deepcopy(seq.frame_encoder).train()          # same weights, its own BatchNorm buffers
    seq.zero_grad()
    out, w = seq(x, return_weights=True)
    assert out.requires_grad and not w.requires_grad
    out.backward(gy)
    feats = vol(x.view(B * F, 1, *VOL))                     # VolumeEncoderFn on the reshaped batch
    want = _pool64(feats.detach().view(B, F, 64), seq.lag_pool.query.detach(), seq.lag_pool.lag_bias.detach(), gy)
    assert rel_err(out, want[0]) <= POOL_BOUNDS["out"] and rel_err(w, want[1]) <= POOL_BOUNDS["attw"]
    feats.backward(want[2].float().cuda().view(B * F, 64))  # fed the REFERENCE dx
    for (n, p), (_, pv) in zip(seq.frame_encoder.named_parameters(), vol.named_parameters()):
        assert p.grad is not None and pv.grad is not None, n
        if n in ("conv_layers.0.bias", "conv_layers.5.bias", "conv_layers.10.bias"):
            continue                                        # in front of a train-mode BatchNorm: exactly 0, both sides rounding noise
        assert rel_err(p.grad, pv.grad) <= VOLUME_GRAD_BOUND, (n, rel_err(p.grad, pv.grad))
    assert rel_err(seq.lag_pool.query.grad, want[3]) <= POOL_BOUNDS["dq"], rel_err(seq.lag_pool.query.grad, want[3])
    assert rel_err(seq.lag_pool.lag_bias.grad, want[4]) <= POOL_BOUNDS["dc"], rel_err(seq.lag_pool.lag_bias.grad, want[4])
    # both BatchNorm updates saw the same B * F volumes
    for (k, a), (_, b) in zip(seq.frame_encoder.state_dict().items(), vol.state_dict().items()):
        if "running" in k or "num_batches" in k:
            assert torch.equal(a, b), k


@pytest.mark.parametrize("dropout", [0.0, 0.3])
def test_one_frame_is_the_volume_encoder_bit_for_bit(dropout):
    ops.set_seed_epoch(None)
    torch.manual_seed(5)
    vol = fMRIVolumeEncoder3D(1, 64, dropout=dropout).cuda().train()
    seq = fMRISequenceEncoder3D.from_volume_encoder(vol, frames=1)
    g = torch.Generator().manual_seed(6)
    x, gy = torch.randn(4, 1, *VOL, generator=g).cuda(), torch.randn(4, 64, generator=g).cuda()
    ops.set_dropout_seed(77)
    fv = vol(x)
    fv.backward(gy)
    ops.set_dropout_seed(77)
    fs, w = seq(x, return_weights=True)                     # (B, 1, D, H, W) is both a one-channel volume and a one-frame sequence
    fs.backward(gy)
    assert torch.equal(w, torch.ones(4, 1, device="cuda"))
    assert torch.equal(fs, fv)
    for (n, p), (_, pv) in zip(seq.frame_encoder.named_parameters(), vol.named_parameters()):
        assert torch.equal(p.grad, pv.grad), n
    assert not seq.lag_pool.query.grad.any() and not seq.lag_pool.lag_bias.grad.any()
    seq.eval(), vol.eval()
    with torch.no_grad():
        assert torch.equal(seq(x), vol(x))


def test_the_input_gradient_reaches_every_frame(case):
    seq, x, gy = case
    seq.eval()
    xg = x.clone().requires_grad_(True)
    out = seq(xg)
    out.backward(gy)
    assert xg.grad.shape == x.shape and torch.isfinite(xg.grad).all()
    assert all(xg.grad[:, f].abs().max().item() > 0 for f in range(F))
    seq.train()
