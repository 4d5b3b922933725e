"""GPU: the lag attention pool's kernel pair, "mm_lagpool_fwd" and "mm_lagpool_bwd" (csrc/lagpool.hip), against an fp64
reference on the same fp32 inputs.  Every output is filled with NaN before the launch (each element must be written), dq
and dc are the sums of the per-sample `dparts` rows in ascending b through the batched reduction the step uses
(mm_reduce_many, nrep = -B).

Input families: N(0, 1) everywhere; "sharp" - q scaled until every row's scores spread over more than 80 nats; "shifted" -
c + 1e4 (c a multiple of 1 / 64, so the shift is exact in fp32) must give the UNSHIFTED reference: the exponent is formed
from differences to the row's largest score.

Rel-L2 errors measured on the MI355X, worst over the seven shapes (bound = 3 x that, and never above 1e-4: an all-fp32
kernel with sums of at most 1 024 terms has no business there):
    out 2.02e-7, attw 1.98e-7, dx 4.43e-6, dq 4.84e-5, dc 4.84e-5    (all five worst in the sharp family)
    N(0, 1) and shifted alone (equal to the last digit): out 1.53e-7, attw 9.27e-8, dx 1.28e-7, dq 2.24e-7, dc 1.56e-7
dq / dc at 4.84e-5 is the (3, 2, 64) sharp case: both frames' gradients are e^-81 times an O(1) number, and the exponent -81
is a difference of fp32 scores of size ~100 (ulp 7.6e-6), so e^-81 itself is known to a few 1e-5 relative; 3 x that is
above the cap, so the cap is the bound.
The fp64 reference forms ds = a (da - sum_g a_g da_g) as a_f sum_g a_g (da_f - da_g), as the kernel does: written the first
way, fp64's own rounding of the difference (1e-16) is twenty decades above the dominant frame's true value.
"""
import ctypes
import math
import struct

import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 64), (3, 2, 64), (7, 3, 4), (5, 5, 32), (33, 7, 96), (4, 16, 256), (2, 64, 1024)]
FAMILIES = ["normal", "sharp", "shifted"]
# 3 x the worst measured value per output (docstring), capped at 1e-4
BOUNDS = {"out": 6.1e-7, "attw": 6.0e-7, "dx": 1.4e-5, "dq": 1e-4, "dc": 1e-4}
assert max(BOUNDS.values()) <= 1e-4


def _inputs(B, F, N, family, seed=0):
    """-> (x, q, c, dout) fp32 on the host and the c the reference uses (the unshifted one)"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 13 * F + N)
    x, q, dout = torch.randn(B, F, N, generator=g), torch.randn(N, generator=g), torch.randn(B, N, generator=g)
    c = torch.round(torch.randn(F, generator=g) * 64) / 64
    c_ref = c
    if family == "sharp" and F > 1:
        # the least-spread row ends at 81 nats (e^-81 = 6.6e-36: its gradients stay normal fp32 numbers); fixed-point
        # iteration, because the spread of k u + c is not linear in k
        u, k = x.double() @ q.double() / math.sqrt(N), 1.0
        for _ in range(30):
            s = k * u + c.double()
            k *= 81.0 / (s.max(dim=1).values - s.min(dim=1).values).min().item()
        q = (q.double() * k).float()
    if family == "shifted":
        c = c + 1e4
        assert torch.equal((c.double() - 1e4).float(), c_ref)          # the shift is exact
    return x, q, c, dout, c_ref


def _reference(x, q, c, dout):
    x, q, c, dout = x.double(), q.double(), c.double(), dout.double()
    r = 1.0 / math.sqrt(x.shape[2])
    s = x @ q * r + c
    a = torch.softmax(s, dim=1)
    out = (a.unsqueeze(-1) * x).sum(dim=1)
    da = (x * dout.unsqueeze(1)).sum(dim=-1)
    # = a (da - sum_g a_g da_g), evaluated without its cancellation: behind a softmax that is one-hot to e^-80 the
    # dominant frame's true value (minus the others' sum) is far below fp64's own rounding of the difference
    ds = a * (a.unsqueeze(1) * (da.unsqueeze(2) - da.unsqueeze(1))).sum(dim=2)
    dx = a.unsqueeze(-1) * dout.unsqueeze(1) + ds.unsqueeze(-1) * q * r
    dq = (ds.unsqueeze(-1) * x).sum(dim=(0, 1)) * r
    return dict(out=out, attw=a, dx=dx, dq=dq, dc=ds.sum(dim=0), s=s)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _sum_rows(dparts, B, F, N):
    """dq, dc = the rows of dparts summed in ascending b by the step's batched reduction (descriptors of -B fp32 rows)"""
    dq, dc = torch.zeros(N, device="cuda"), torch.zeros(F, device="cuda")
    raw = struct.pack("<QQqqq", dparts.data_ptr(), dq.data_ptr(), N, -B, N + F) + \
        struct.pack("<QQqqq", dparts.data_ptr() + 4 * N, dc.data_ptr(), F, -B, N + F)
    host = ctypes.create_string_buffer(raw, len(raw))
    _hip.call("mm_reduce_many", ctypes.addressof(host), 2)
    return dq, dc


def _run(x, q, c, dout):
    B, F, N = x.shape
    x, q, c, dout = x.cuda(), q.cuda(), c.cuda(), dout.cuda()
    out, attw, dx, dparts = _nan(B, N), _nan(B, F), _nan(B, F, N), _nan(B, N + F)
    _hip.call("mm_lagpool_fwd", x, q, c, out, attw, B, F, N)
    _hip.call("mm_lagpool_bwd", dout, x, attw, q, dx, dparts, B, F, N)
    dq, dc = _sum_rows(dparts, B, F, N)
    torch.cuda.synchronize()
    return dict(out=out, attw=attw, dx=dx, dq=dq, dc=dc, dparts=dparts)


def _rel_l2(got, want):
    den = want.norm().item()
    err = (got.double().cpu() - want).norm().item()
    return err / den if den > 0 else err


@pytest.fixture(scope="module")
def cases():
    """every (shape, family): inputs, the kernels' outputs and the fp64 reference, computed once"""
    table = {}
    for shape in SHAPES:
        for family in FAMILIES:
            x, q, c, dout, c_ref = _inputs(*shape, family)
            table[shape, family] = ((x, q, c, dout), _run(x, q, c, dout), _reference(x, q, c_ref, dout))
    return table


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_outputs_agree_with_the_fp64_reference(cases, shape, family):
    (x, q, c, dout), got, want = cases[shape, family]
    B, F, N = shape
    if family == "sharp" and F > 1:
        spread = want["s"].max(dim=1).values - want["s"].min(dim=1).values
        assert spread.min().item() > 80
    for k in ("out", "attw", "dx", "dparts"):
        assert torch.isfinite(got[k]).all(), f"{k}: an element was not written"
    errs = {k: _rel_l2(got[k], want[k]) for k in BOUNDS}
    print(f"lagpool {shape} {family}: " + " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    if F == 1:                                            # no softmax gradient: dq and dc are exactly zero, as the reference's
        assert want["dq"].abs().max().item() < 1e-12 and not got["dq"].any() and not got["dc"].any()
        errs.pop("dq"), errs.pop("dc")
    for k, v in errs.items():
        assert v <= BOUNDS[k], (k, v, BOUNDS[k])
    rows = got["attw"].double().sum(dim=1)
    assert (rows - 1).abs().max().item() <= 4 * 2.0 ** -23, (rows - 1).abs().max().item()
    # the parameter rows were summed in ascending b, each rounded once
    acc = got["dparts"][0].clone()
    for b in range(1, B):
        acc = acc + got["dparts"][b]
    assert torch.equal(acc[:N], got["dq"]) and torch.equal(acc[N:], got["dc"])


@pytest.mark.parametrize("shape", [(1, 1, 64), (6, 1, 256)], ids=lambda s: "x".join(map(str, s)))
def test_one_frame_is_the_identity_bit_for_bit(shape):
    x, q, c, dout, _ = _inputs(*shape, "normal", seed=3)
    got = _run(x, q, c, dout)
    assert torch.equal(got["attw"], torch.ones(shape[0], 1, device="cuda"))
    assert torch.equal(got["out"].cpu(), x[:, 0])
    assert torch.equal(got["dx"].cpu()[:, 0], dout)
    assert not got["dparts"].any() and torch.isfinite(got["dparts"]).all()


@pytest.mark.parametrize("shape", [(33, 7, 96), (2, 64, 1024)], ids=lambda s: "x".join(map(str, s)))
def test_two_runs_are_bit_identical(shape):
    x, q, c, dout, _ = _inputs(*shape, "normal", seed=5)
    a, b = _run(x, q, c, dout), _run(x, q, c, dout)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_a_row_does_not_depend_on_its_batch():
    x, q, c, dout, _ = _inputs(33, 7, 96, "normal", seed=9)
    big, small = _run(x, q, c, dout), _run(x[:3].contiguous(), q, c, dout[:3].contiguous())
    for k in ("out", "attw", "dx", "dparts"):
        assert torch.equal(big[k][:3], small[k]), k


def test_bad_shapes_are_refused_by_both_layers():
    x = torch.zeros(2, 3, 8, device="cuda")
    q, c, out, attw = torch.zeros(8, device="cuda"), torch.zeros(3, device="cuda"), _nan(2, 8), _nan(2, 3)
    for B, F, N, word in ((2, 0, 8, "F must be"), (2, 65, 8, "F must be"), (2, 3, 6, "N must be"), (2, 3, 1028, "N must be"),
                          (0, 3, 8, "B must be")):
        with pytest.raises(_hip.HipLibraryError, match=word):
            _hip.call("mm_lagpool_fwd", x, q, c, out, attw, B, F, N)
        with pytest.raises(_hip.HipLibraryError, match=word):
            _hip.call("mm_lagpool_bwd", out, x, attw, q, x, out, B, F, N)
    assert torch.isnan(out).all() and torch.isnan(attw).all()          # nothing was launched
    with pytest.raises(ValueError, match="frames must be"):
        ops.lag_pool_fwd(torch.zeros(2, 65, 8, device="cuda"), q, torch.zeros(65, device="cuda"))
    with pytest.raises(ValueError, match="feature width"):
        ops.lag_pool_bwd(torch.zeros(2, 6, device="cuda"), torch.zeros(2, 3, 6, device="cuda"), attw, torch.zeros(6, device="cuda"))


def test_parameters_may_sit_at_any_float_offset():
    """q and c are views into a trainer's flat bucket: no alignment beyond a float's is asked of them"""
    x, q, c, dout, _ = _inputs(5, 5, 32, "normal", seed=13)
    want = _run(x, q, c, dout)
    flat = torch.zeros(1 + 32 + 5, device="cuda")
    flat[1:33], flat[33:] = q.cuda(), c.cuda()
    assert flat[1:33].data_ptr() % 16 != 0
    got_out, got_w = ops.lag_pool_fwd(x.cuda(), flat[1:33], flat[33:])
    got_dx, got_parts = ops.lag_pool_bwd(dout.cuda(), x.cuda(), got_w, flat[1:33])
    for k, t in (("out", got_out), ("attw", got_w), ("dx", got_dx), ("dparts", got_parts)):
        assert torch.equal(t, want[k]), k


def test_the_ops_pair_and_the_autograd_function_are_the_kernels():
    x, q, c, dout, _ = _inputs(5, 5, 32, "normal", seed=11)
    want = _run(x, q, c, dout)
    xg, qg, cg = (t.cuda().requires_grad_(True) for t in (x, q, c))
    out, w = ops.lag_pool(xg, qg, cg)
    assert not w.requires_grad and torch.equal(out, want["out"]) and torch.equal(w, want["attw"])
    out.backward(dout.cuda())
    assert torch.equal(xg.grad, want["dx"]) and torch.equal(qg.grad, want["dq"]) and torch.equal(cg.grad, want["dc"])
    with torch.no_grad():
        o2, w2 = ops.lag_pool(xg, qg, cg)
    assert torch.equal(o2, want["out"]) and torch.equal(w2, want["attw"])
