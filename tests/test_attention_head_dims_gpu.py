"""GPU: multi-head self-attention at every head dim the kernels run (csrc/attention.hip through mm_attn_fwd_hd /
mm_attn_bwd_hd: dh = 16, 24, ..., 64) against an fp64 reference on the kernels' bf16 operands:
softmax(q k^T / sqrt(dh) + mask) * keep @ v, keep from the host replica of the kernels' dropout block hash
(oracle/dropout_replica.py: attn_keep_scale), and its autograd gradients for the bf16 dout.

Tolerances as in test_kernels_gpu.py::test_attention_fwd_bwd (out 2e-2, lse 1e-3, dqkv rel-L2 < 2e-2 and elementwise
5e-2 / 3e-2) and test_attention_masked_gpu.py (rel-L2 bounds of the masked kernels)."""
import math

import pytest
import torch

from oracle.dropout_replica import attn_keep_scale
from test_kernels_gpu import _hip

pytestmark = pytest.mark.gpu

HEAD_DIMS = [16, 24, 32, 40, 48, 56, 64]
SHAPES = [(2, 512, 4), (3, 125, 4), (1, 300, 2), (2, 32, 1), (2, 1024, 8)]
SEED = 2024


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _inputs(B, L, H, dh, seed):
    g = torch.Generator().manual_seed(seed)
    E = H * dh
    qkv = torch.randn(B, L, 3 * E, generator=g).to(torch.bfloat16).float()
    dout = torch.randn(B, L, E, generator=g).to(torch.bfloat16).float()
    return qkv, dout


def _ref(qkv, dout, B, L, H, dh, mask=None, p=0.0):
    """fp64 attention on the bf16 operands -> out, lse (natural log), dqkv"""
    E = H * dh
    x = qkv.double().requires_grad_(True)
    q, k, v = (t.view(B, L, H, dh).transpose(1, 2) for t in x.split(E, dim=2))
    s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    if mask is not None:
        s = s + (mask.double() if mask.dim() == 2 else mask.double().view(B, H, L, L))
    lse = torch.logsumexp(s, dim=-1)
    pr = torch.exp(s - lse.unsqueeze(-1))
    if p > 0:
        pr = pr * attn_keep_scale(SEED, B * H, L, p).view(B, H, L, L).double()
    o = (pr @ v).transpose(1, 2).reshape(B, L, E)
    o.backward(dout.double())
    return o.detach(), lse.detach(), x.grad


def _run(hip, qkv, dout, B, L, H, dh, mask=None, p=0.0, fwd="mm_attn_fwd_hd", bwd="mm_attn_bwd_hd"):
    E = H * dh
    per_head = int(mask is not None and mask.dim() == 3)
    mg = mask.contiguous().cuda() if mask is not None else None
    qg = qkv.cuda().to(torch.bfloat16)
    out = torch.full((B, L, E), float("nan"), device="cuda").to(torch.bfloat16)
    lse = torch.full((B, H, L), float("nan"), device="cuda")
    hip.call(fwd, qg, out, lse, B, L, H, dh, 1.0 / math.sqrt(dh), p, SEED, None, mg, per_head)
    dqkv = torch.full((B, L, 3 * E), float("nan"), device="cuda").to(torch.bfloat16)
    delta = torch.empty(B, H, L, device="cuda")
    hip.call(bwd, qg, out, dout.cuda().to(torch.bfloat16), lse, dqkv, delta, B, L, H, dh, 1.0 / math.sqrt(dh), p, SEED,
             None, mg, per_head)
    torch.cuda.synchronize()
    return out.float().cpu(), lse.cpu(), dqkv.float().cpu()


@pytest.mark.parametrize("B,L,H", SHAPES)
@pytest.mark.parametrize("dh", HEAD_DIMS)
def test_attention_hd_fwd_bwd_vs_fp64(dh, B, L, H):
    hip = _hip()
    qkv, dout = _inputs(B, L, H, dh, L + dh)
    o_ref, lse_ref, dq_ref = _ref(qkv, dout, B, L, H, dh)
    out, lse, dqkv = _run(hip, qkv, dout, B, L, H, dh)
    torch.testing.assert_close(out, o_ref.float(), rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(lse, lse_ref.float(), rtol=1e-3, atol=1e-3)
    assert _rel(dqkv, dq_ref) < 2e-2, _rel(dqkv, dq_ref)
    torch.testing.assert_close(dqkv, dq_ref.float(), rtol=5e-2, atol=3e-2)


def _mask(kind, B, H, L, g):
    """additive fp32 mask, (L, L) or (B * H, L, L); -inf = not allowed.  Every row keeps at least one key."""
    q = torch.arange(L).view(L, 1)
    k = torch.arange(L).view(1, L)
    if kind == "causal":
        return torch.zeros(L, L).masked_fill(k > q, float("-inf"))
    if kind == "anticausal":                             # queries >= 128: whole leading key chunks masked
        return torch.zeros(L, L).masked_fill(k < q, float("-inf"))
    if kind == "leftpad":                                # per head: whole chunks of keys masked for every query
        m = torch.zeros(B, H, L, L)
        for b in range(B):
            m[b, :, :, :max(1, (b + 2) * L // (B + 3))] = float("-inf")
        return m.view(B * H, L, L)
    return torch.randn(B * H, L, L, generator=g) * 2.0   # random per-head float mask


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("kind", ["causal", "anticausal", "leftpad", "random"])
@pytest.mark.parametrize("dh", [16, 40, 64])
def test_attention_hd_masked_vs_fp64(dh, kind, p):
    hip = _hip()
    B, L, H = 2, 300, 2
    qkv, dout = _inputs(B, L, H, dh, 7 * dh + len(kind))
    mask = _mask(kind, B, H, L, torch.Generator().manual_seed(dh))
    o_ref, lse_ref, dq_ref = _ref(qkv, dout, B, L, H, dh, mask, p)
    out, lse, dqkv = _run(hip, qkv, dout, B, L, H, dh, mask, p)
    assert torch.isfinite(out).all() and torch.isfinite(dqkv).all()
    assert _rel(out, o_ref) < 1e-2, _rel(out, o_ref)
    torch.testing.assert_close(lse, lse_ref.float(), rtol=1e-3, atol=1e-3)
    E = H * dh
    for i, name in enumerate(("dq", "dk", "dv")):
        got, want = dqkv[..., i * E:(i + 1) * E], dq_ref[..., i * E:(i + 1) * E]
        bound = 3e-2 if p > 0 else 2e-2
        assert _rel(got, want) < bound, (name, _rel(got, want))
    if kind == "leftpad":                                # keys no query sees: dK = dV = 0 exactly
        m = mask.view(B, H, L, L)
        for b in range(B):
            dead = torch.isinf(m[b, 0, 0])
            assert torch.all(dqkv[b][dead][:, E:] == 0)


@pytest.mark.parametrize("dh", [24, 64])
def test_attention_hd_bool_mask_equals_minus_inf(dh):
    """ops.additive_attn_mask(bool) + ops.attention (True = not allowed) == the same mask as 0 / -inf floats, bit for bit"""
    from multimodal_eeg_fmri_amd import ops
    B, L, H = 2, 200, 4
    qkv, _ = _inputs(B, L, H, dh, 99)
    allowed = torch.rand(L, L, generator=torch.Generator().manual_seed(5)) < 0.3
    allowed |= torch.eye(L, dtype=torch.bool)
    boolm = (~allowed).cuda()
    addm = torch.zeros(L, L).masked_fill(~allowed, float("-inf")).cuda()
    qg = qkv.cuda().to(torch.bfloat16)
    o1, l1 = ops.attention(qg, H, True, 0.0, 0, ops.additive_attn_mask(boolm, L, qg))
    o2, l2 = ops.attention(qg, H, True, 0.0, 0, addm)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2) and torch.equal(l1, l2)


@pytest.mark.parametrize("dh", [16, 48, 64])
def test_attention_hd_dropout_vs_replica(dh):
    """p = 0.1 without a mask (the DROP instantiations): forward and backward against the fp64 replica of the mask"""
    hip = _hip()
    B, L, H = 2, 384, 4
    qkv, dout = _inputs(B, L, H, dh, 31 + dh)
    o_ref, lse_ref, dq_ref = _ref(qkv, dout, B, L, H, dh, None, 0.1)
    out, lse, dqkv = _run(hip, qkv, dout, B, L, H, dh, None, 0.1)
    assert _rel(out, o_ref) < 1e-2, _rel(out, o_ref)
    torch.testing.assert_close(lse, lse_ref.float(), rtol=1e-3, atol=1e-3)
    assert _rel(dqkv, dq_ref) < 3e-2, _rel(dqkv, dq_ref)
    # and the replica is not vacuous: without the mask the reference is far off
    o_nodrop, _, _ = _ref(qkv, dout, B, L, H, dh)
    assert _rel(out, o_nodrop) > 5 * _rel(out, o_ref)


@pytest.mark.parametrize("dh", [16, 40, 64])
def test_attention_hd_is_bit_reproducible(dh):
    hip = _hip()
    B, L, H = 2, 333, 4
    qkv, dout = _inputs(B, L, H, dh, 3)
    mask = _mask("random", B, H, L, torch.Generator().manual_seed(1))
    for m in (None, mask):
        a = _run(hip, qkv, dout, B, L, H, dh, m, 0.1)
        b = _run(hip, qkv, dout, B, L, H, dh, m, 0.1)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


@pytest.mark.parametrize("B,L,H", [(2, 512, 4), (3, 125, 4)])
def test_attention_hd_at_32_as_tight_as_the_dh32_kernels(B, L, H):
    """head_dim 32 through mm_attn_*_hd: as close to fp64 as mm_attn_fwd / mm_attn_bwd are"""
    hip = _hip()
    qkv, dout = _inputs(B, L, H, 32, 11 + L)
    o_ref, lse_ref, dq_ref = _ref(qkv, dout, B, L, H, 32)
    new = _run(hip, qkv, dout, B, L, H, 32)
    old = _run(hip, qkv, dout, B, L, H, 32, fwd="mm_attn_fwd", bwd="mm_attn_bwd")
    for got, base, want in zip(new, old, (o_ref, lse_ref, dq_ref)):
        assert _rel(got, want) <= 1.05 * _rel(base, want) + 1e-7, (_rel(got, want), _rel(base, want))


def test_attention_hd_refuses_unsupported_head_dims_before_launch():
    hip = _hip()
    for dh in (8, 20, 72):
        for name in ("mm_attn_fwd_hd", "mm_attn_bwd_hd"):
            args = (None, None, None, 1, 4, 1, dh, 1.0, 0.0, 0, None, None, 0) if name.endswith("fwd_hd") else \
                   (None, None, None, None, None, None, 1, 4, 1, dh, 1.0, 0.0, 0, None, None, 0)
            with pytest.raises(hip.HipLibraryError, match="head_dim"):
                hip.call(name, *args)
