"""GPU: the attribution kernels of csrc/xai.hip, called by name through the C ABI.

* mm_xai_interp is BIT-EQUAL to torch's fp32 ``base + alpha * (x - base)`` with alpha = np.linspace(0, 1, n)[s] (each
  operation rounded on its own) for the zero, per-sample and broadcast baselines, odd inner sizes (scalar path),
  unaligned pointers and chunks that start at s0 > 0.
* mm_xai_accum / mm_xai_finish / mm_xai_pair_score against an fp64 host computation.  Bounds from the formats:
  a sum of S fp32 terms added one at a time carries at most (S + 1) * 2^-24 relative to the sum of magnitudes; one
  subtraction, one division and one product round three times (4 * 2^-24 allowed); a mean over T values adds
  (T + 2) * 2^-24 of the mean of magnitudes.  Two runs give the same bits.
* every invalid shape gives a negative return code and leaves the outputs alone."""
import ctypes

import numpy as np
import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _torch_interp(x, base, n_steps, s0, steps):
    alphas = np.linspace(0, 1, n_steps)
    b = torch.zeros_like(x) if base is None else base.expand_as(x)
    return torch.cat([b + float(np.float32(alphas[s])) * (x - b) for s in range(s0, s0 + steps)])


@pytest.mark.parametrize("shape", [(4, 8, 256), (3, 5, 37), (2, 1, 6, 5, 7), (5, 36), (1, 3)])
@pytest.mark.parametrize("kind", ["zero", "per_sample", "broadcast"])
def test_interpolation_is_bit_equal_to_the_fp32_formula(shape, kind):
    x = _randn(11, *shape)
    base = {"zero": None, "per_sample": _randn(12, *shape) * 0.5, "broadcast": x.mean(dim=0, keepdim=True)}[kind]
    rows = {"zero": 0, "per_sample": shape[0], "broadcast": 1}[kind]
    B, inner = shape[0], x.numel() // shape[0]
    for n_steps, s0, steps in ((7, 0, 7), (7, 3, 2), (50, 41, 9), (1, 0, 1), (2, 1, 1)):
        out = torch.full((steps * B,) + tuple(shape[1:]), float("nan"), device="cuda")
        _hip.call("mm_xai_interp", x, base, rows, out, n_steps, s0, steps, B, inner)
        want = _torch_interp(x, base, n_steps, s0, steps)
        assert torch.equal(out, want), (shape, kind, n_steps, s0, (out - want).abs().max().item())
        assert torch.equal(ops.xai_interpolate(x, base, n_steps, s0, steps), want)
    # the first and the last point of the path are the baseline and the input themselves
    ends = ops.xai_interpolate(x, base, 9, 0, 9)
    assert torch.equal(ends[-B:], (torch.zeros_like(x) if base is None else base.expand_as(x)) + (x - (0 if base is None else base)))


def test_interpolation_through_unaligned_pointers_takes_the_scalar_path():
    buf, obuf = _randn(13, 4 * 64 + 1), torch.zeros(3 * 4 * 64 + 1, device="cuda")
    x, out = buf[1:].view(4, 64), obuf[1:]                         # 4-byte aligned only
    _hip.call("mm_xai_interp", x.data_ptr(), None, 0, out.data_ptr(), 5, 1, 3, 4, 64)
    assert torch.equal(out.view(12, 64), _torch_interp(x, None, 5, 1, 3)) and obuf[0].item() == 0.0


@pytest.mark.parametrize("n,steps", [(4 * 8 * 256, 9), (3 * 185, 5), (7, 1), (4096 * 33, 3)])
def test_accumulate_sums_in_ascending_step_order(n, steps):
    g = _randn(21, steps, n)
    acc0 = _randn(22, n)
    acc = acc0.clone()
    _hip.call("mm_xai_accum", g, acc, steps, n)
    want = acc0.double() + g.double().sum(0)
    mag = acc0.double().abs() + g.double().abs().sum(0)
    assert ((acc.double() - want).abs() <= (steps + 1) * EPS * mag).all()
    seq = acc0.clone()                                             # the stated order, exactly
    for s in range(steps):
        seq = seq + g[s]
    assert torch.equal(acc, seq)
    again = acc0.clone()
    _hip.call("mm_xai_accum", g, again, steps, n)
    assert torch.equal(acc, again)
    # cutting the steps into chunks leaves the bits alone
    parts = acc0.clone()
    cut = max(1, steps // 2)
    ops.xai_accumulate(parts, g[:cut], cut)
    if steps > cut:
        ops.xai_accumulate(parts, g[cut:], steps - cut)
    assert torch.equal(parts, acc)


@pytest.mark.parametrize("B,C,T", [(4, 8, 256), (3, 5, 37), (2, 3, 1024), (2, 1, 3001)])
@pytest.mark.parametrize("kind", ["zero", "per_sample", "broadcast"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_finish_against_fp64(B, C, T, kind, mode):
    x, acc = _randn(31, B, C, T), _randn(32, B, C, T) * 3
    base = {"zero": None, "per_sample": _randn(33, B, C, T), "broadcast": _randn(34, 1, C, T)}[kind]
    rows = {"zero": 0, "per_sample": B, "broadcast": 1}[kind]
    n_steps = 20
    xd, ad = x.double(), acc.double()
    bd = torch.zeros_like(xd) if base is None else base.double().expand_as(xd)
    want = {0: ((xd - bd) * ad / n_steps).abs(), 1: ad.abs(), 2: ad.abs() * xd.abs()}[mode]
    for with_chan in (True, False):
        attr = torch.full_like(x, float("nan"))
        chan = torch.full((B, C), float("nan"), device="cuda") if with_chan else None
        _hip.call("mm_xai_finish", x, base, rows, acc, attr, chan, B, C, T, n_steps, mode)
        # mode 0: the subtraction's rounding is relative to |x| + |base|, not to the difference
        tol = 4 * EPS * (want + ((xd.abs() + bd.abs()) * ad.abs() / n_steps if mode == 0 else 0))
        assert ((attr.double() - want).abs() <= tol).all(), (mode, kind, with_chan)
        attr2 = torch.empty_like(x)
        chan2 = torch.empty((B, C), device="cuda") if with_chan else None
        _hip.call("mm_xai_finish", x, base, rows, acc, attr2, chan2, B, C, T, n_steps, mode)
        assert torch.equal(attr, attr2)
        if with_chan:
            mean = attr.double().mean(dim=2)                      # of the fp32 attributions the kernel wrote
            assert ((chan.double() - mean).abs() <= (T + 2) * EPS * mean).all()
            assert torch.equal(chan, chan2)
            first = attr.clone()
        else:
            assert torch.equal(attr, first)                       # the flat and the per-row kernels write the same bits
    a2, c2 = ops.xai_finish(x, base, acc, n_steps, {0: "integrated_gradients", 1: "gradient", 2: "gradient_x_input"}[mode], channels=True)
    assert torch.equal(a2, first) and c2.shape == (B, C)


def test_finish_on_a_volume_and_on_feature_rows():
    for shape in ((2, 1, 6, 5, 7), (5, 36)):
        x, acc = _randn(41, *shape), _randn(42, *shape)
        attr, chan = ops.xai_finish(x, None, acc, 8, "integrated_gradients")
        assert chan is None and attr.shape == x.shape
        want = (x.double() * acc.double() / 8).abs()
        assert ((attr.double() - want).abs() <= 4 * EPS * want).all()
    with pytest.raises(ValueError):
        ops.xai_finish(_randn(43, 5, 36), None, _randn(44, 5, 36), 8, "gradient", channels=True)


@pytest.mark.parametrize("B,N", [(6, 128), (3, 100), (1, 7)])
def test_pair_score_and_seed(B, N):
    z = torch.nn.functional.normalize(_randn(51, B, 2, N), dim=2).reshape(B, 2 * N).contiguous()
    score = torch.full((B,), float("nan"), device="cuda")
    seed = torch.full((B, 2 * N), float("nan"), device="cuda")
    _hip.call("mm_xai_pair_score", z, score, seed, B, N)
    zd = z.double()
    want = (zd[:, :N] * zd[:, N:]).sum(1)
    mag = (zd[:, :N] * zd[:, N:]).abs().sum(1)
    assert ((score.double() - want).abs() <= (N + 2) * EPS * mag).all()
    assert torch.equal(seed[:, :N], z[:, N:]) and torch.equal(seed[:, N:], z[:, :N])
    s2, g2 = ops.xai_pair_score(z)
    assert torch.equal(s2, score) and torch.equal(g2, seed)
    s3, g3 = ops.xai_pair_score(z, want_seed=False)
    assert torch.equal(s3, score) and g3 is None


def test_invalid_shapes_give_negative_codes_and_write_nothing():
    lib = _hip.load()
    x, out = _randn(61, 2, 8), torch.zeros(5 * 2, 8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    L = ctypes.c_int64
    P = lambda t: ctypes.c_void_p(t.data_ptr())              # noqa: E731
    bad = [("mm_xai_interp", (P(x), None, 0, P(out), 5, 3, 3, L(2), L(8), st)),
           ("mm_xai_interp", (P(x), None, 0, P(out), 0, 0, 1, L(2), L(8), st)),
           ("mm_xai_interp", (P(x), None, 0, P(out), 5, 0, 5, L(2), L(0), st)),
           ("mm_xai_interp", (P(x), P(x), 3, P(out), 5, 0, 5, L(2), L(8), st)),
           ("mm_xai_interp", (P(x), None, 0, None, 5, 0, 5, L(2), L(8), st)),
           ("mm_xai_accum", (P(out), P(out), 0, L(16), st)),
           ("mm_xai_accum", (P(out), P(out), 2, L(-1), st)),
           ("mm_xai_finish", (P(x), None, 0, P(x), P(out), None, 2, 1, L(8), 5, 7, st)),
           ("mm_xai_finish", (P(x), None, 0, P(x), P(out), None, 0, 1, L(8), 5, 0, st)),
           ("mm_xai_finish", (P(x), None, 0, P(x), P(out), None, 2, 1, L(8), -1, 0, st)),
           ("mm_xai_finish", (P(x), P(x), 5, P(x), P(out), None, 2, 1, L(8), 5, 0, st)),
           ("mm_xai_pair_score", (P(x), P(out), None, 2, 0, st)),
           ("mm_xai_pair_score", (P(x), None, None, 2, 4, st))]
    for name, args in bad:
        rc = getattr(lib, name)(*args)
        assert rc < 0 and lib.mm_last_error(), (name, rc)
    torch.cuda.synchronize()
    assert out.abs().max().item() == 0.0
    with pytest.raises(_hip.HipLibraryError, match="xai_interp"):
        ops.xai_interpolate(x, None, 5, 4, 3)
    with pytest.raises(ValueError):
        ops.xai_interpolate(x, _randn(62, 3, 8), 5, 0, 5)
