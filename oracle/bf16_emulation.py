"""TEST INFRASTRUCTURE ONLY.  Runs the fp32 oracle with the GEMM operands
(activations and weights of every conv / linear) rounded to bf16, the way the
HIP path feeds its MFMAs (fp32 accumulate), and with the one activation tensor the
HIP path keeps in bf16 where the reference keeps fp32 rounded too: the pre-BatchNorm
output of the pooled 32 -> 64 voxel-encoder layer (csrc/conv3d_wres.hip writes it as
bf16; BatchNorm, the 2x2x2 arg-max and the backward's x-hat all see the rounded
values).  Rounding is straight-through for autograd.  Separates "bf16 operand precision" (expected, and amplified by
max-pool argmax flips in backward) from logic errors: the HIP path is held
tightly to THIS variant and loosely to the pure-fp32 oracle."""
from __future__ import annotations

import contextlib

import torch
import torch.nn.functional as TF

from . import ref_functional as RF


def _r(t):
    if t is None or not t.is_floating_point():
        return t
    return t + (t.to(torch.bfloat16).float() - t).detach()


class _RoundedF:
    def __init__(self, stored_bf16=((64, 32),)):
        self.stored = tuple(stored_bf16)          # (Cout, Cin) of the conv3d layers whose pre-BatchNorm output the HIP path keeps in bf16

    def __getattr__(self, name):
        fn = getattr(TF, name)
        if name in ("conv1d", "linear"):
            def wrapped(x, w, b=None, *a, **k):
                return fn(_r(x), _r(w), b, *a, **k)
            return wrapped
        if name == "conv3d":
            def wrapped3(x, w, b=None, *a, **k):
                out = fn(_r(x), _r(w), b, *a, **k)
                return _r(out) if tuple(w.shape[:2]) in self.stored else out   # layer 2 (and the implicit-GEMM layer 1): stored in bf16
            return wrapped3
        return fn


@contextlib.contextmanager
def bf16_operands(l1_as_gemm: bool = False, widths=(32, 64, 128)):
    """``l1_as_gemm``: the voxel encoder's first layer ran as an ordinary implicit GEMM (a caller asked for d / d volume,
    ops._vol_forward_impl(need_dx=True), or w0 != 32: there is no fused first layer then); that form keeps its pooled
    layer's pre-BatchNorm output in bf16 too.  ``widths``: the voxel encoder's (w0, w1, w2) - the layers whose output is
    stored in bf16 are the POOLED ones, w0 -> w1 and (as a GEMM) 1 -> w0, recognised by their (Cout, Cin); the un-pooled
    last layer keeps fp32 (so its shape must differ from the pooled ones', as it does for the widths the tests use)."""
    w0, w1, w2 = widths
    assert (w2, w1) not in ((w1, w0), (w0, 1)), "the last layer's weight shape must tell it from the pooled layers"
    saved = RF.F
    RF.F = _RoundedF(((w1, w0), (w0, 1)) if l1_as_gemm else ((w1, w0),))
    try:
        yield
    finally:
        RF.F = saved
