"""GPU: multi-head self-attention with an additive attention mask (csrc/attention.hip, the MASK instantiations of the
forward, dq and dkv kernels, with and without attention-probability dropout) against an fp64 reference of the same
operation on the kernels' bf16 operands: softmax(q k^T / sqrt(32) + mask) * keep @ v, keep from the host replica of the
kernels' block hash (oracle/dropout_replica.py: attn_keep_scale), and its autograd gradients for the bf16 dout.

The masks are chosen to reach what the unmasked and the causal / band / random masks of the other tests do not:
  - anti-causal (query q sees keys >= q): every query >= 128 has its first one or more 128-key chunks fully masked, so its
    running maximum is still -inf when the first tiles arrive;
  - left key padding of a different length per batch element (the per-head (B * H, L, L) form): whole chunks of keys masked
    for every query, whose dK and dV must be exactly zero and whose K / V must not reach the output at all;
  - a random finite float mask.
Rows with no allowed key (NaN by contract) are not generated.  Figures are rel-L2 errors ||got - want|| / ||want||
(lse: max abs error in nats); bounds are 3x the worst case measured on the MI355X:

    out 2.6e-3 -> 7.5e-3    lse 1.4e-6 -> 4e-6    dv 2.4e-3 -> 7e-3    dq, dk 3.0e-3 -> 8.5e-3
    (dq, dk with one allowed key per row and dropout: 1.02e-2 -> 2.8e-2, see the test)
Worst cases over every mask, dropout rate and shape; the masked kernels with and without dropout measure alike.
Exact: zero dK / dV for keys no query sees, bit-identical output when such a key's K / V change, and a bool mask equal
to the same mask as additive -inf."""
import math

import pytest
import torch

from oracle.dropout_replica import attn_keep_scale
from test_kernels_gpu import _hip

pytestmark = pytest.mark.gpu

DH = 32
SCALE = 1.0 / math.sqrt(DH)
SEED = 2024


def _mask(kind, B, H, L, g):
    """additive fp32 mask, (L, L) or (B * H, L, L); -inf = not allowed.  Every row keeps at least one key."""
    if kind == "anticausal":
        q = torch.arange(L).view(L, 1)
        k = torch.arange(L).view(1, L)
        return torch.zeros(L, L).masked_fill(k < q, float("-inf"))
    if kind == "leftpad":
        # batch element 0: at least the whole first 128-key chunk (three chunks and a part at L = 512); the others shorter
        pads = [max(128, L - 100) if L > 128 else L // 2] + [min(L - 1, (2 + b) * L // 5) for b in range(1, B)]
        m = torch.zeros(B, H, L, L)
        for b, pad in enumerate(pads):
            m[b, :, :, :pad] = float("-inf")
        return m.view(B * H, L, L)
    return torch.randn(B * H, L, L, generator=g) * 2.0


def _ref(qkv, mask, B, H, L, p, dout):
    """fp64 attention on the bf16 operands; returns out, lse (natural log), dqkv"""
    E = H * DH
    x = qkv.double().requires_grad_(True)
    q, k, v = (t.view(B, L, H, DH).transpose(1, 2) for t in x.split(E, dim=2))
    s = (q @ k.transpose(-1, -2)) * SCALE + (mask.double() if mask.dim() == 2 else mask.double().view(B, H, L, L))
    lse = torch.logsumexp(s, dim=-1)
    pr = torch.exp(s - lse.unsqueeze(-1))
    if p > 0:
        pr = pr * attn_keep_scale(SEED, B * H, L, p).view(B, H, L, L).double()
    o = (pr @ v).transpose(1, 2).reshape(B, L, E)
    o.backward(dout.double())
    return o.detach(), lse.detach(), x.grad


def _run(hip, qkv, mask, B, H, L, p, dout):
    per_head = int(mask.dim() == 3)
    E = H * DH
    qg = qkv.cuda().to(torch.bfloat16)
    mg = mask.contiguous().cuda()
    out = torch.full((B, L, E), float("nan"), device="cuda").to(torch.bfloat16)
    lse = torch.full((B, H, L), float("nan"), device="cuda")
    hip.call("mm_attn_fwd", qg, out, lse, B, L, H, DH, SCALE, p, SEED, None, mg, per_head)
    dqkv = torch.full((B, L, 3 * E), float("nan"), device="cuda").to(torch.bfloat16)
    delta = torch.empty(B, H, L, device="cuda")
    hip.call("mm_attn_bwd", qg, out, dout.cuda().to(torch.bfloat16), lse, dqkv, delta, B, L, H, DH, SCALE, p, SEED,
             None, mg, per_head)
    return out.float().cpu(), lse.cpu(), dqkv.float().cpu()


def _rel(got, want):
    return (got.double() - want).norm().item() / want.norm().item()


CASES = [(L, H, kind, p) for kind in ("anticausal", "leftpad", "random") for p in (0.0, 0.3)
         for L, H in ((129, 4), (256, 1), (320, 4), (512, 1))]


@pytest.mark.parametrize("L,H,kind,p", CASES)
def test_masked_attention_matches_fp64(L, H, kind, p):
    hip = _hip()
    B = 2
    E = H * DH
    g = torch.Generator().manual_seed(L * 10 + H + len(kind) + int(p * 10))
    qkv = (torch.randn(B, L, 3 * E, generator=g) * 0.8).to(torch.bfloat16).float()
    dout = torch.randn(B, L, E, generator=g).to(torch.bfloat16).float()
    mask = _mask(kind, B, H, L, g)
    want_o, want_lse, want_d = _ref(qkv, mask, B, H, L, p, dout)
    out, lse, dqkv = _run(hip, qkv, mask, B, H, L, p, dout)
    # L = 129 left-padded by 128: every query of batch element 0 sees key 128 alone, P = 1 and the exact dS is 0; with
    # dropout the stored bf16 output is keep * v128 rounded, so delta = rowsum(dO * O) misses dP by a bf16 rounding and
    # dq / dk of that element are pure rounding residue (the backward's delta-from-the-output design, not the mask)
    lone = kind == "leftpad" and L <= 129 and p > 0
    figs = {"out": (_rel(out, want_o), 7.5e-3),
            "lse": ((lse.double() - want_lse).abs().max().item(), 4e-6)}
    for i, name in enumerate(("dq", "dk", "dv")):
        figs[name] = (_rel(dqkv[..., i * E:(i + 1) * E], want_d[..., i * E:(i + 1) * E]),
                      7e-3 if name == "dv" else (2.8e-2 if lone else 8.5e-3))
    for name, (e, bound) in figs.items():
        print(f"ERR attn {kind} L{L} H{H} p{p} {name} {e:.3e} (bound {bound:.0e})")
    bad = {k: v for k, v in figs.items() if not v[0] <= v[1]}
    assert not bad, bad
    if kind == "leftpad":
        # keys masked for every query of a batch element: zero gradient, exactly
        m = mask.view(B, H, L, L)
        dead = torch.isinf(m).all(dim=2).all(dim=1)                      # (B, L) keys no query of any head sees
        assert dead.any()
        dk = dqkv[..., E:2 * E][dead]
        dv = dqkv[..., 2 * E:][dead]
        assert torch.all(dk == 0) and torch.all(dv == 0)
        # ... and their K and V do not reach the output: other finite values, the same bits
        qkv2 = qkv.clone()
        pert = (torch.randn(int(dead.sum()), 2 * E, generator=g) * 5).to(torch.bfloat16).float()
        qkv2[..., E:][dead] = pert
        out2, lse2, dqkv2 = _run(hip, qkv2, mask, B, H, L, p, dout)
        assert torch.equal(out2, out) and torch.equal(lse2, lse)
        assert torch.equal(dqkv2[..., :E], dqkv[..., :E])


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_bool_mask_equals_the_additive_minus_inf_mask(p):
    """ops.additive_attn_mask(bool) + ops.attention == the same mask written as 0 / -inf floats, bit for bit, in both
    the shared and the per-head form"""
    from multimodal_eeg_fmri_amd import ops
    _hip()
    B, H, L = 2, 2, 300
    E = H * DH
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(B, L, 3 * E, generator=g).to(torch.bfloat16).cuda()
    k = torch.arange(L).view(1, L)
    shared = k < torch.arange(L).view(L, 1) - 150                     # banned: keys more than 150 behind the query
    per_head = torch.rand(B * H, L, L, generator=g) < 0.5
    per_head[..., 0] = False
    for bm in (shared, per_head):
        fm = torch.zeros(bm.shape).masked_fill(bm, float("-inf")).cuda()
        am = ops.additive_attn_mask(bm, L, qkv)
        assert torch.equal(am, fm)
        o1, l1 = ops.attention(qkv, H, True, p, 5, am)
        o2, l2 = ops.attention(qkv, H, True, p, 5, fm)
        assert torch.equal(o1, o2) and torch.equal(l1, l2)
        assert torch.isfinite(o1.float()).all()
