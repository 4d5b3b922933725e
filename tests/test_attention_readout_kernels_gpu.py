"""GPU: the attention read-out kernels (csrc/attention_readout.hip: mm_attn_weights, mm_attn_received,
mm_attn_received_ws_floats) against an fp64 softmax on the kernels' bf16 operands, as `_ref` of
test_attention_head_dims_gpu.py.  Inputs are randn qkv, scores of order 1 nat (scores of tens of nats and near one-hot rows:
test_attention_sharp_scores_gpu.py); lse comes from the matching mm_attn_fwd (head dim 32) or mm_attn_fwd_hd call.

Tolerances.  The project holds lse to 1e-3 (test_kernels_gpu / test_attention_head_dims_gpu); P = exp(s - lse) inherits
that as a relative error, doubled for the score's own fp32 rounding and the hardware exp: weights rtol 2e-3, atol 1e-6,
every row sums to 1 within 2e-3.  Received: all terms are positive and each within 2e-3, another 1e-3 covers fp32
summation over L <= 257 terms: rtol 3e-3, atol 1e-6.  Received against the fp64 column sum of the `w` that
mm_attn_weights returned: both kernels form every probability with the same instructions, so what is left is fp32
summation of at most 4 * 257 positive terms (n * 2^-24 = 6.1e-5 relative in the worst case) and the head mean's own
roundings in `w`: rtol 1e-4."""
import functools
import math

import pytest
import torch

from multimodal_eeg_fmri_amd import ops
from test_kernels_gpu import _hip

pytestmark = pytest.mark.gpu

# ragged and exact tiles, one and several key / query chunks, both padded widths, the exact (32) and runtime head dims
SHAPES = [(2, 1, 1, 32), (1, 33, 2, 32), (2, 128, 4, 32), (1, 130, 3, 16), (1, 200, 2, 24), (1, 257, 1, 40), (1, 256, 2, 64)]
W_TOL = dict(rtol=2e-3, atol=1e-6)
R_TOL = dict(rtol=3e-3, atol=1e-6)
NEG = float("-inf")


def _probs(qkv, B, L, H, dh, mask=None):
    """fp64 softmax probabilities (B, H, L, L) on the bf16 operands"""
    E = H * dh
    q, k, _ = (t.view(B, L, H, dh).transpose(1, 2) for t in qkv.double().split(E, dim=2))
    s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    if mask is not None:
        s = s + (mask.double() if mask.dim() == 2 else mask.double().view(B, H, L, L))
    return torch.softmax(s, dim=-1)


def _forward_lse(hip, qg, B, L, H, dh, mg=None):
    out = torch.empty(B, L, H * dh, device="cuda", dtype=torch.bfloat16)
    lse = torch.full((B, H, L), float("nan"), device="cuda")
    hip.call("mm_attn_fwd" if dh == 32 else "mm_attn_fwd_hd", qg, out, lse, B, L, H, dh, 1.0 / math.sqrt(dh), 0.0, 0, None, mg,
             int(mg is not None and mg.dim() == 3))
    return lse


@functools.lru_cache(maxsize=None)
def _case(B, L, H, dh, kind=None):
    """operands, the forward's lse and the fp64 probabilities of one shape, computed once and shared (never modified)"""
    hip = _hip()
    g = torch.Generator().manual_seed(1000 * L + dh + H)
    qkv = torch.randn(B, L, 3 * H * dh, generator=g).to(torch.bfloat16)
    qi, ki = torch.arange(L).view(L, 1), torch.arange(L).view(1, L)
    mask = None
    if kind == "causal":
        mask = torch.zeros(L, L).masked_fill(ki > qi, NEG)
    elif kind == "random":                                  # per (batch, head), -inf entries, the diagonal always allowed
        mask = torch.randn(B * H, L, L, generator=g) * 2.0
        mask[(torch.rand(B * H, L, L, generator=g) < 0.3) & (ki != qi)] = NEG
    elif kind == "row":                                     # query row L // 2 fully masked
        mask = torch.zeros(L, L)
        mask[L // 2] = NEG
    elif kind == "onekey":                                  # only key j* = L // 3 allowed, for every query
        mask = torch.full((L, L), NEG)
        mask[:, L // 3] = 0.0
    qg = qkv.cuda()
    mg = mask.cuda() if mask is not None else None
    lse = _forward_lse(hip, qg, B, L, H, dh, mg)
    r = (torch.rand(B, L, generator=g) + 0.1)
    return dict(qkv=qg, lse=lse, mask=mg, P=_probs(qkv.float(), B, L, H, dh, mask), r=r, rg=r.cuda())


def _weights(hip, c, B, L, H, dh, per_head):
    w = torch.full((B, H, L, L) if per_head else (B, L, L), float("nan"), device="cuda")
    m = c["mask"]
    hip.call("mm_attn_weights", c["qkv"], c["lse"], w, B, L, H, dh, 1.0 / math.sqrt(dh), m, int(m is not None and m.dim() == 3),
             int(per_head))
    return w


def _received(hip, c, B, L, H, dh, row_w, sw):
    n = hip.host_int("mm_attn_received_ws_floats", B, L, H)
    assert n == B * H * L
    ws = torch.full((n,), float("nan"), device="cuda")
    out = torch.full((B, L), float("nan"), device="cuda")
    m = c["mask"]
    hip.call("mm_attn_received", c["qkv"], c["lse"], c["rg"] if row_w else None, float(sw), out, ws, B, L, H, dh,
             1.0 / math.sqrt(dh), m, int(m is not None and m.dim() == 3))
    return out


def _received_ref(A, r, sw):
    """A fp64 (B, L, L) head mean, r fp64 (B, L)"""
    return sw * r + (1.0 - sw) * torch.einsum("bi,bij->bj", r, A)


@pytest.mark.parametrize("per_head", [False, True])
@pytest.mark.parametrize("B,L,H,dh", SHAPES)
def test_weights_vs_fp64(B, L, H, dh, per_head):
    hip = _hip()
    c = _case(B, L, H, dh)
    w = _weights(hip, c, B, L, H, dh, per_head).cpu()
    want = c["P"] if per_head else c["P"].mean(dim=1)
    err = ((w.double() - want).abs() / want.clamp_min(1e-30)).max().item()
    print(f"READOUT_FIG weights {(B, L, H, dh)} per_head={per_head}: max rel err {err:.3e}, "
          f"max |rowsum - 1| {(w.double().sum(-1) - 1).abs().max().item():.3e}")
    torch.testing.assert_close(w.double(), want, **W_TOL)
    assert (w.double().sum(-1) - 1).abs().max().item() < 2e-3


@pytest.mark.parametrize("row_w,sw", [(False, 0.0), (True, 0.0), (False, 0.5), (True, 0.5)])
@pytest.mark.parametrize("B,L,H,dh", SHAPES)
def test_received_vs_fp64(B, L, H, dh, row_w, sw):
    hip = _hip()
    c = _case(B, L, H, dh)
    out = _received(hip, c, B, L, H, dh, row_w, sw).cpu().double()
    r = c["r"].double() if row_w else torch.full((B, L), 1.0 / L, dtype=torch.float64)
    want = _received_ref(c["P"].mean(dim=1), r, sw)
    print(f"READOUT_FIG received {(B, L, H, dh)} row_w={row_w} sw={sw}: max rel err "
          f"{((out - want).abs() / want).max().item():.3e}")
    torch.testing.assert_close(out, want, **R_TOL)
    torch.testing.assert_close(out.sum(-1), r.sum(-1), **R_TOL)           # A is row-stochastic: the mass is kept
    w = _weights(hip, c, B, L, H, dh, False).cpu().double()
    torch.testing.assert_close(out, _received_ref(w, r, sw), rtol=1e-4, atol=1e-12)


def test_causal_boolean_mask_through_the_host_ops():
    B, L, H, dh = 1, 130, 2, 32
    c = _case(B, L, H, dh, "causal")
    boolean = torch.triu(torch.ones(L, L, dtype=torch.bool), diagonal=1)
    w = ops.attention_weights(c["qkv"], c["lse"], H, mask=boolean).cpu().double()
    torch.testing.assert_close(w, c["P"].mean(dim=1), **W_TOL)
    assert torch.all(w[:, boolean] == 0)                 # a key after the query gets exactly nothing
    wh = ops.attention_weights(c["qkv"], c["lse"], H, mask=boolean, per_head=True).cpu().double()
    torch.testing.assert_close(wh, c["P"], **W_TOL)
    out = ops.attention_received(c["qkv"], c["lse"], H, mask=boolean).cpu().double()
    torch.testing.assert_close(out, c["P"].mean(dim=(1, 2)), **R_TOL)


def test_random_per_head_additive_mask():
    hip = _hip()
    B, L, H, dh = 2, 64, 2, 32
    c = _case(B, L, H, dh, "random")
    assert torch.isinf(c["mask"]).any() and torch.isfinite(c["lse"]).all()
    torch.testing.assert_close(_weights(hip, c, B, L, H, dh, False).cpu().double(), c["P"].mean(dim=1), **W_TOL)
    torch.testing.assert_close(_weights(hip, c, B, L, H, dh, True).cpu().double(), c["P"], **W_TOL)
    out = _received(hip, c, B, L, H, dh, True, 0.5).cpu().double()
    torch.testing.assert_close(out, _received_ref(c["P"].mean(dim=1), c["r"].double(), 0.5), **R_TOL)


def test_a_fully_masked_row_is_nan_in_that_row_only():
    hip = _hip()
    B, L, H, dh = 1, 33, 2, 32
    c = _case(B, L, H, dh, "row")
    dead = L // 2
    live = [i for i in range(L) if i != dead]
    for per_head in (False, True):
        w = _weights(hip, c, B, L, H, dh, per_head).cpu().double()
        want = c["P"] if per_head else c["P"].mean(dim=1)
        assert torch.isnan(w[..., dead, :]).all() and torch.isfinite(w[..., live, :]).all()
        torch.testing.assert_close(w[..., live, :], want[..., live, :], **W_TOL)
    # every key sums over that query: the whole batch element is NaN
    assert torch.isnan(_received(hip, c, B, L, H, dh, False, 0.0)).all()


def test_a_mask_that_allows_one_key_gives_a_one_hot():
    hip = _hip()
    B, L, H, dh = 1, 130, 2, 32
    c = _case(B, L, H, dh, "onekey")
    j = L // 3
    onehot = torch.zeros(B, L, dtype=torch.float64)
    onehot[:, j] = 1.0
    w = _weights(hip, c, B, L, H, dh, False).cpu().double()
    torch.testing.assert_close(w, onehot.view(B, 1, L).expand(B, L, L), **W_TOL)
    torch.testing.assert_close(_received(hip, c, B, L, H, dh, False, 0.0).cpu().double(), onehot, **R_TOL)


def test_two_calls_give_the_same_bits():
    hip = _hip()
    B, L, H, dh = 2, 128, 4, 32
    c = _case(B, L, H, dh)
    for per_head in (False, True):
        assert torch.equal(_weights(hip, c, B, L, H, dh, per_head), _weights(hip, c, B, L, H, dh, per_head))
    for row_w, sw in ((False, 0.0), (True, 0.5)):
        a, b = _received(hip, c, B, L, H, dh, row_w, sw), _received(hip, c, B, L, H, dh, row_w, sw)
        assert torch.isfinite(a).all() and torch.equal(a, b)
    c = _case(1, 257, 1, 40)
    assert torch.equal(_received(hip, c, 1, 257, 1, 40, True, 0.5), _received(hip, c, 1, 257, 1, 40, True, 0.5))


def test_refusals_before_a_launch():
    hip = _hip()
    B, L, H = 1, 16, 2
    lse = torch.zeros(B, H, L, device="cuda")
    w = torch.zeros(B, L, L, device="cuda")
    out = torch.zeros(B, L, device="cuda")
    ws = torch.zeros(B * H * L, device="cuda")
    q = torch.zeros(B, L, 3 * H * 72, device="cuda", dtype=torch.bfloat16)

    def weights(qkv=q, lse=lse, w=w, L=L, dh=32, per_head=0):
        hip.call("mm_attn_weights", qkv, lse, w, B, L, H, dh, 0.1, None, 0, per_head)

    def received(qkv=q, lse=lse, out=out, ws=ws, L=L, dh=32, sw=0.0):
        hip.call("mm_attn_received", qkv, lse, None, sw, out, ws, B, L, H, dh, 0.1, None, 0)
    for dh in (20, 72):
        with pytest.raises(hip.HipLibraryError, match=r"attn_weights: head_dim"):
            weights(dh=dh)
        with pytest.raises(hip.HipLibraryError, match=r"attn_received: head_dim"):
            received(dh=dh)
    for kw in (dict(L=0), dict(qkv=None), dict(lse=None), dict(w=None)):
        with pytest.raises(hip.HipLibraryError, match=r"attn_weights: null/invalid"):
            weights(**kw)
    for kw in (dict(L=0), dict(qkv=None), dict(lse=None), dict(out=None)):
        with pytest.raises(hip.HipLibraryError, match=r"attn_received: null/invalid"):
            received(**kw)
    with pytest.raises(hip.HipLibraryError, match=r"attn_received: null ws"):
        received(ws=None)
    with pytest.raises(hip.HipLibraryError, match=r"attn_weights: per_head"):
        weights(per_head=2)
    for sw in (-0.1, 1.5, float("nan")):
        with pytest.raises(hip.HipLibraryError, match=r"attn_received: self_weight"):
            received(sw=sw)
    with pytest.raises(hip.HipLibraryError, match=r"attn_received_ws_floats"):
        hip.host_int("mm_attn_received_ws_floats", 0, L, H)
    torch.cuda.synchronize()
    assert torch.all(w == 0) and torch.all(out == 0)                     # nothing was launched
    # host ops: ValueError before a launch
    qkv = torch.zeros(B, L, 3 * H * 32, device="cuda", dtype=torch.bfloat16)
    bad = torch.zeros(B * H + 1, L, L, device="cuda")
    with pytest.raises(ValueError, match="batch \\* heads"):
        ops.attention_weights(qkv, lse, H, mask=bad)
    with pytest.raises(ValueError, match="batch \\* heads"):
        ops.attention_received(qkv, lse, H, mask=bad)
    with pytest.raises(ValueError, match="head dim"):
        ops.attention_weights(torch.zeros(B, L, 3 * H * 20, device="cuda", dtype=torch.bfloat16), lse, H)
    with pytest.raises(ValueError, match="self_weight"):
        ops.attention_received(qkv, lse, H, self_weight=1.5)
    with pytest.raises(ValueError, match="row_w"):
        ops.attention_received(qkv, lse, H, row_w=torch.zeros(B, L + 1, device="cuda"))
