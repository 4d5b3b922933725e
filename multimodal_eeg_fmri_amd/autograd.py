"""Backward passes of the HIP path, exposed to torch.autograd as a handful of
coarse ``Function``s (one per encoder / block / head) so the tape stays short.

Parameter gradients are produced without floating-point atomics (per-workgroup slots summed in
order, or fixed-point accumulator workspaces: csrc/common.h), so a step is bit-reproducible.  When a
parameter carries a gradient *sink* (``param._mm_grad``, a view into the
trainer's flat gradient bucket) the kernels accumulate straight into it and
autograd receives ``None``; otherwise a fresh tensor is returned to autograd.
"""
from __future__ import annotations

import os
from typing import Dict, List, NamedTuple, Optional

import torch

from . import _hip
from . import ops
from .ops import ACT, AREPL, REPL, WREP, _BF, _F32, _empty, _zeros


_BAG = {"cur": None}


def _reduce_into(dst, src, K, stride, offset=0, nrep=REPL):
    """dst[k] += sum_rep src[rep*stride + offset + k]   (deferred to GradBag.flush when a bag is active).
    nrep = REPL: ``src`` is a gradient accumulator workspace (zeroed (REPL, ...) fp32-sized buffer holding AREPL
    replicas of 64-bit fixed-point sums; ``stride`` / ``offset`` count its 64-bit elements); nrep = 1: compact fp32."""
    if dst is None:
        return
    if nrep not in (1, REPL):
        raise ValueError("_reduce_into: nrep is 1 (fp32 vector) or REPL (accumulator workspace)")
    bag = _BAG["cur"]
    ptr = src.data_ptr() + (8 if nrep == REPL else 4) * offset
    if bag is not None:
        bag.defer(ptr, dst, K, AREPL if nrep == REPL else 1, stride, keep=src)
    elif nrep == REPL:
        _hip.call("mm_acc_reduce", ptr, dst, K, stride)
    else:
        _hip.call("mm_reduce_replicas", ptr, dst, K, 1, stride)


def _scatter_into(dw, ws, cout, cin, taps, cinp, nrep, window=None):
    """dw[n][c][tap] += sum_rep ws[rep][n][tap][c]   (deferred to GradBag.flush when a bag is active).
    ``window`` = (first output channel, first tap, workspace taps, workspace output channels): ``dw`` (cout, cin, taps) takes
    only that block of a wider workspace (the branches of EnhancedPowerEncoder's merged convolution)."""
    bag = _BAG["cur"]
    if bag is not None:
        bag.defer_scatter(ws, dw, cout, cin, taps, cinp, nrep, window)
    elif window is None:
        _hip.call("mm_wgrad_scatter", ws, dw, cout, cin, taps, cinp, nrep)
    else:
        import ctypes
        import struct
        raw = struct.pack("<QQiiiiii", *scatter_desc(ws, dw, cout, cin, taps, cinp, nrep, window))
        host = ctypes.create_string_buffer(raw, len(raw))
        _hip.call("mm_scatter_many", ctypes.addressof(host), 1)


def scatter_desc(ws, dw, cout, cin, taps, cinp, nrep, window=None):
    """the 40-byte descriptor of mm_scatter_many / mm_flush_many (include/mmeeg_hip.h)"""
    if window is None:
        return (ws.data_ptr(), dw.data_ptr(), cout, cin, taps, cinp, nrep, 0)
    n0, tap0, ws_taps, ws_cout = window
    return (ws.data_ptr() + 4 * n0 * ws_taps * cinp, dw.data_ptr(), cout, cin, taps | (tap0 << 8) | (ws_taps << 16), cinp, nrep, ws_cout)


def _wgrad_slots(dy, x, dw, dbr, B, T, cinp, N, k, pad, cin, parts=None):
    """conv / linear weight gradient without atomics: every row-chunk workgroup stores its partial
    dW[n][tap][c] into its own slot of a workspace; the (deferred, batched) scatter sums the slots
    into the parameter layout."""
    bag = _BAG["cur"]
    grouped = bag is not None and k == 1
    if grouped:
        slots = _hip.host_int("mm_conv1d_wgrad_many_slots", B, T, cinp, N)
    else:
        slots = _hip.host_int("mm_conv1d_wgrad_slots", B, T, cinp, N, k)
    ws = _empty((slots, N, k, cinp), _F32, dy)                   # every element has exactly one writer: no memset
    if grouped:
        # a Linear's weight gradient feeds nothing but the final slot sum: collect it; the bag issues
        # all of them as ONE launch when it is flushed (possibly on another stream, off the chain)
        bag.defer_wgrad(dy, x, ws, dbr, B, T, cinp, N, slots)
    elif bag is not None and bag.defer_conv_wgrads:
        # k > 1 convs: same idea, one launch each at flush time (a trainer hands them to an idle stream)
        bag.calls.append(("mm_conv1d_wgrad", (dy, x, ws, dbr, B, T, cinp, N, k, pad, cinp, k * cinp, 1, cinp,
                                              slots, N * k * cinp, 1)))
    else:
        _hip.call("mm_conv1d_wgrad", dy, x, ws, dbr, B, T, cinp, N, k, pad, cinp, k * cinp, 1, cinp,
                  slots, N * k * cinp, 1)
    if parts is None:
        _scatter_into(dw, ws, N, cin, k, cinp, slots)
    else:            # (gradient tensor, first output channel, output channels, kernel size): centred tap windows of the workspace
        for t, n0, cn, kk in parts:
            if t is not None:
                _scatter_into(t, ws, cn, cin, kk, cinp, slots, window=(n0, (k - kk) // 2, k, N))


class deferred:
    """context: parameter-gradient replica reductions issued inside are collected
    in ``bag`` and executed as one mm_reduce_many launch on exit."""

    def __init__(self, bag, device):
        self.bag, self.device = bag, device

    def __enter__(self):
        self.prev = _BAG["cur"]
        _BAG["cur"] = self.bag
        return self.bag

    def __exit__(self, *exc):
        _BAG["cur"] = self.prev
        if exc[0] is None:
            self.bag.flush(self.device)
        return False


def _ln_param_grads(bag, ln, dgb, D):
    """dgb = replicated [REPL][2][D] {dgamma row, dbeta row}"""
    gw, gb = bag.target(ln.weight), bag.target(ln.bias)
    if gw is not None and gb is not None and gw.data_ptr() + 4 * D == gb.data_ptr():
        _reduce_into(gw, dgb, 2 * D, 2 * D)                                # adjacent in the flat bucket
        return
    _reduce_into(gw, dgb, D, 2 * D, 0)
    _reduce_into(gb, dgb, D, 2 * D, D)


def _compact(rep_buf, K):
    """gradient accumulator workspace of K values per replica -> compact fp32 [K] (one parallel reduction)"""
    out = _zeros((K,), rep_buf)
    _hip.call("mm_acc_reduce", rep_buf, out, K, K)
    return out


def _bn_param_grads(bag, bn, sums, N, nrep=1):
    """sums = [nrep][sum dz (dbeta) | sum dz*xhat (dgamma)]"""
    _reduce_into(bag.target(bn.bias), sums, N, 2 * N, 0, nrep=nrep)
    _reduce_into(bag.target(bn.weight), sums, N, 2 * N, N, nrep=nrep)


# ------------------------------------------------------------ gradient sinks
class GradBag:
    """collects parameter gradients of one backward call.  Replica reductions
    into parameter gradients are deferred and flushed as ONE kernel launch."""

    def __init__(self):
        self.fresh: Dict[int, torch.Tensor] = {}
        self.pending = []            # (src_ptr, dst_ptr, K, nrep, stride)
        self.scatters = []           # (ws_ptr, dw_ptr, Cout, Cin, taps, Cinp, nrep)
        self.wgrads = []             # (dy_ptr, x_ptr, ws_ptr, dbias_ptr, B, T, Cin, Cout, Cin_real, nslots)
        self.calls = []              # (entry point, args): launches postponed to flush time
        self.defer_conv_wgrads = False
        self._keep = []

    def defer(self, src_ptr: int, dst: torch.Tensor, K: int, nrep: int, stride: int, keep=None):
        self.pending.append((src_ptr, dst.data_ptr(), K, nrep, stride))
        self._keep.append((dst, keep))

    def defer_scatter(self, ws: torch.Tensor, dw: torch.Tensor, cout, cin, taps, cinp, nrep, window=None):
        self.scatters.append(scatter_desc(ws, dw, cout, cin, taps, cinp, nrep, window))
        self._keep.append((dw, ws))

    def defer_wgrad(self, dy, x, ws, dbr, B, T, cinp, N, slots):
        self.wgrads.append((dy.data_ptr(), x.data_ptr(), ws.data_ptr(), dbr.data_ptr() if dbr is not None else 0,
                            B, T, cinp, N, cinp, slots))
        self._keep.append((dy, x, ws, dbr))

    def hand_over(self) -> "GradBag":
        """move everything deferred so far into a new bag (to be flushed elsewhere, e.g. on another stream)"""
        other = GradBag()
        other.pending, other.scatters, other.wgrads, other._keep = self.pending, self.scatters, self.wgrads, self._keep
        other.calls = self.calls
        self.pending, self.scatters, self.wgrads, self.calls, self._keep = [], [], [], [], []
        return other

    def flush(self, device):
        import ctypes
        import struct
        for name, args in self.calls:                    # first: the slot sums and bias reductions below read them
            _hip.call(name, *args)
        self._keep.append(self.calls)
        self.calls = []
        if self.wgrads:
            raw = b"".join(struct.pack("<QQQQiiiiiiii", *d, 0, 0) for d in self.wgrads)
            host = ctypes.create_string_buffer(raw, len(raw))
            _hip.call("mm_conv1d_wgrad_many", ctypes.addressof(host), len(self.wgrads))
            self.wgrads = []
        if not self.scatters and not self.pending:
            return
        # slot sums (weight gradients) and accumulator reductions (bias / norm-parameter gradients): one launch
        sraw = b"".join(struct.pack("<QQiiiiii", *d) for d in self.scatters)
        rraw = b"".join(struct.pack("<QQqqq", *d) for d in self.pending)
        shost = ctypes.create_string_buffer(sraw, max(len(sraw), 1))      # descriptors travel as kernel arguments
        rhost = ctypes.create_string_buffer(rraw, max(len(rraw), 1))
        _hip.call("mm_flush_many", ctypes.addressof(shost) if self.scatters else None, len(self.scatters),
                  ctypes.addressof(rhost) if self.pending else None, len(self.pending))
        self.scatters, self.pending = [], []

    def target(self, p: torch.Tensor) -> Optional[torch.Tensor]:
        """fp32 buffer (PyTorch layout of ``p``) the kernels accumulate into."""
        if p is None or not p.requires_grad:
            return None
        sink = getattr(p, "_mm_grad", None)
        if sink is not None:
            return sink
        t = self.fresh.get(id(p))
        if t is None:
            t = torch.zeros_like(p, dtype=_F32, memory_format=torch.contiguous_format)
            self.fresh[id(p)] = t
        return t

    def result(self, p: torch.Tensor) -> Optional[torch.Tensor]:
        return self.fresh.get(id(p))


def _mask_cast(g_f32=None, g_bf16=None, z=None, act="none", drop_p=0.0, seed=0):
    """bf16( g * dropout_mask * act'(z) )"""
    src = g_f32 if g_f32 is not None else g_bf16
    out = _empty(src.shape, _BF, src)
    _hip.call("mm_act_bwd", g_f32, g_bf16, z, out, src.numel(), ACT[act], float(drop_p), int(seed), ops.EP())
    return out


def linear_bwd(bag: GradBag, dy: torch.Tensor, x: torch.Tensor, weight, bias, *, need_dx=True,
               dx_f32=False, below=None):
    """dy (M, N) bf16, x (M, Kp) bf16 -> dx (M, Kp); accumulates dW, db.
    ``below`` = (z, act, drop_p, seed) of the layer that produced ``x``: the data-gradient
    GEMM then returns d(pre-activation z) = (dy W) * act'(z) * dropout_mask directly."""
    M, N = dy.shape
    Kp = x.shape[1]
    K = weight.shape[1]
    dw = bag.target(weight)
    db = bag.target(bias)
    dbr = _zeros((REPL, N), dy) if db is not None else None
    if dw is not None:
        _wgrad_slots(dy, x, dw, dbr, 1, M, Kp, N, 1, 0, K)
    elif db is not None:
        _hip.call("mm_colsum", dy, None, dbr, M, N)
    if db is not None:
        _reduce_into(db, dbr, N, N)
    if not need_dx:
        return None
    _, wd, cinp, coutp = ops.weights.get(weight, True)
    if coutp != N:
        raise _hip.HipLibraryError(f"linear_bwd: dY width {N} != padded out width {coutp}")
    kw = {}
    if below is not None:
        z, act, p, seed = below
        kw = dict(gradz=z, gradz_act=act, drop_p=p, seed=seed)
    r = ops.igemm(dy.view(1, M, N), wd, 1, 0, cinp, out_f32=dx_f32, out_bf16=not dx_f32, **kw)
    return (r["f32"] if dx_f32 else r["bf16"]).view(M, cinp)


_NO_BCAST = bool(os.environ.get("MM_NO_BCAST"))     # A/B knob: the voxel head's gradient as a full (B, V, N) tensor
_NO_GEMM2 = bool(os.environ.get("MM_NO_GEMM2"))     # A/B knob: the out-projection's data gradient as its own launch
_NO_BNRED = bool(os.environ.get("MM_NO_BNRED"))     # A/B knob: the BatchNorm-backward reduce as its own launch
_NO_FFN_ROWS_BWD = bool(os.environ.get("MM_NO_FFN_ROWS_BWD"))   # A/B knob: the FFN-2 data gradient as its own launch


def _bn_bwd_args(s: dict, y):
    B, T, N = y.shape
    d2 = s.get("drop2", (0.0, 0))
    return (B, T, N, ACT[s["act"]], s["pool"], 1 if s["drop_first"] else 0, float(s["drop_p"]), int(s["seed"]),
            float(d2[0]), int(d2[1]), ops.EP())


def conv_bn_act_bwd(bag: GradBag, s: dict, dout_bf16=None, dout_f32=None, need_dx=True, sums=None, below=None):
    """backward of ops.conv_bn_act (train mode). returns dx (B, T, Cinp) bf16.

    ``sums``: this block's BatchNorm-backward sums when the producer of ``dout`` already formed them (skips the
    reduce launch).  ``below`` = the saved dict of the conv block whose output fed this one: the data-gradient GEMM
    then runs that block's reduce pass as its epilogue (mm_conv1d_dgrad_bn_reduce) and the call returns
    ``(dx, sums_below)``; ``sums_below`` is None when the shapes do not allow the fusion (the caller passes it on
    either way)."""
    conv, bn = s["conv"], s["bn"]
    y, out4, xb = s["y"], s["out4"], s["xb"]
    B, T, N = y.shape
    args = _bn_bwd_args(s, y)
    if sums is None:
        sums = _zeros((REPL, 2, N), y)
        _hip.call("mm_bn_act_bwd_reduce", y, out4, dout_bf16, dout_f32, sums, *args)
    dy = _empty((B, T, N), _BF, y)
    # the apply pass sums the 32 replicas itself (no compaction launch between the two passes)
    _hip.call("mm_bn_act_bwd_apply", y, out4, dout_bf16, dout_f32, sums, dy, None, *args,
              1 if s.get("train", True) else 0, REPL)
    _bn_param_grads(bag, bn, sums, N, nrep=REPL)
    k, pad = conv.kernel_size[0], conv.padding[0]
    cin = conv.in_channels
    # a convolution merged from several modules (ops._power_merged_train) sends its slot sums straight into THEIR gradients
    parts = getattr(conv, "parts", None)
    if parts is not None:
        parts = [(bag.target(w), n0, w.shape[0], w.shape[2]) for w, n0 in parts]
        dw = None
    else:
        dw = bag.target(conv.weight)
    if dw is not None or (parts is not None and any(t is not None for t, *_ in parts)):
        cinp_x = xb.shape[2]
        db = bag.target(conv.bias)
        dbr = _zeros((REPL, N), y) if db is not None else None
        _wgrad_slots(dy, xb, dw, dbr, B, T, cinp_x, N, k, pad, cin, parts=parts)
        if db is not None:
            _reduce_into(db, dbr, N, N)
    if not need_dx:
        return None if below is None else (None, None)
    _, wd, cinp, coutp = ops.weights.get(conv.weight, True)
    assert coutp == N
    if below is not None:
        yb = below["y"]
        d2 = below.get("drop2", (0.0, 0))
        if not _NO_BNRED and (k > 1 or cinp <= 64) and yb.shape[2] == cinp and yb.shape[1] == T * below["pool"] and float(d2[0]) == 0.0:
            dx = _empty((B, T, cinp), _BF, y)
            sums_b = _zeros((REPL, 2, cinp), y)
            _hip.call("mm_conv1d_dgrad_bn_reduce", dy, wd, B, T, N, cinp, k, k - 1 - pad, dx, yb, below["out4"], sums_b,
                      ACT[below["act"]], below["pool"], 1 if below["drop_first"] else 0, float(below["drop_p"]),
                      int(below["seed"]), ops.EP())
            return dx, sums_b
        return ops.igemm(dy, wd, k, k - 1 - pad, cinp)["bf16"], None
    return ops.igemm(dy, wd, k, k - 1 - pad, cinp)["bf16"]


class BlockBwdPlan(NamedTuple):
    """which launches a transformer block's backward runs: the forward's ``ops.BlockPlan`` plus this module's knobs"""
    ffn: str            # FFN + norm2 + out-projection data gradient: "ffn_rows" (mm_ffn_rows_bwd) | "ln_gemm2" (.._ln_bwd_gemm2) |
    #                     "ln" (mm_linear_dgrad_ln_bwd) | "generic" (data-gradient GEMM, then LayerNorm backward)
    qkv: str            # QKV projection + norm1: "ln_bn_reduce" (.._ln_bwd_bn_reduce) | "ln" | "generic"
    head_rows: bool     # the head's gradient is accepted as one fp32 row per sample (read by the "ffn_rows" / "ln_gemm2" launch)


def block_bwd_plan(plan: ops.BlockPlan, bn_below: bool = False) -> BlockBwdPlan:
    """``bn_below``: the block's input is the un-pooled 128-wide output of a conv block whose BatchNorm-backward sums the
    last launch can form, and nothing asks for a masked bf16 copy of d(input)"""
    gemm2 = plan.ln_fused and plan.out_proj_128 and not _NO_GEMM2
    if gemm2:
        ffn = "ffn_rows" if plan.ffn_rows_width and not _NO_FFN_ROWS_BWD else "ln_gemm2"
    else:
        ffn = "ln" if plan.ln_fused else "generic"
    qkv = "generic" if not plan.ln_fused else "ln_bn_reduce" if bn_below and not _NO_BNRED else "ln"
    return BlockBwdPlan(ffn, qkv, gemm2)


def _linear_ln_bwd(bag, form, dy, h, weight, bias, x, stat, ln, dres, dx, dx_bf16, dgb, drop_p, seed, bn_below=None, w2=None,
                   res_rows=0):
    """backward of ``Linear(LayerNorm(x))``: weight / bias gradients of the Linear (``h`` = LN(x) bf16 is its
    input), then d x = LN_backward(dy W) + dres.  ``form`` (BlockBwdPlan.ffn / .qkv): "generic" takes two launches, the
    others run the data-gradient GEMM with the LayerNorm backward as its epilogue - "ln_bn_reduce" with the BatchNorm-backward
    sums of the conv block ``bn_below`` (dx is its fp32 d(out)), returned in ``bn_below["sums"]``; "ln_gemm2" with the data
    gradient of the Linear under this LayerNorm's skip path (``w2`` = the attention out-projection's 128 x 128 image),
    computed from dx_bf16 before it leaves the workgroup and returned."""
    M, D = x.shape
    if form == "generic":
        dh = linear_bwd(bag, dy, h, weight, bias)
        _hip.call("mm_layernorm_bwd", dh, None, x, stat, ln.weight, dres, dx, dx_bf16, dgb, M, D, drop_p, seed, ops.EP())
        return None
    linear_bwd(bag, dy, h, weight, bias, need_dx=False)
    _, wd, cinp, coutp = ops.weights.get(weight, True)
    if coutp != dy.shape[1] or cinp != D:
        raise _hip.HipLibraryError(f"linear_ln_bwd: dY width {dy.shape[1]} / LN width {D} != weight image {coutp} x {cinp}")
    if form == "ln_bn_reduce":
        sb = bn_below["s"]
        yb = sb["y"]
        d2 = sb.get("drop2", (0.0, 0))
        bn_below["sums"] = sums_b = _zeros((REPL, 2, 128), yb)
        _hip.call("mm_linear_dgrad_ln_bwd_bn_reduce", dy, wd, M, coutp, x, stat, ln.weight, dres, dx, dgb, ops.EP(),
                  yb, sb["out4"], sums_b, ACT[sb["act"]], float(sb["drop_p"]), int(sb["seed"]), float(d2[0]), int(d2[1]))
        return None
    if form == "ln_gemm2":
        do = _empty((M, 128), _BF, dy)
        _hip.call("mm_linear_dgrad_ln_bwd_gemm2", dy, wd, M, coutp, x, stat, ln.weight, dres, dx, dx_bf16, dgb,
                  drop_p, seed, ops.EP(), w2, do, int(res_rows))
        return do
    _hip.call("mm_linear_dgrad_ln_bwd", dy, wd, M, coutp, x, stat, ln.weight, dres, dx, dx_bf16, dgb,
              drop_p, seed, ops.EP())
    return None


def ffn_rows_bwd_fused(blocks) -> bool:
    """do all these saved transformer blocks take mm_ffn_rows_bwd?  A trainer balances its two streams by it."""
    return bool(blocks) and all(block_bwd_plan(s["plan"]).ffn == "ffn_rows" for s in blocks)


def transformer_block_bwd(bag: GradBag, s: dict, dx2: torch.Tensor, dy2=None, emit_for=None, bn_below=None):
    """dx2 fp32 (M, D) -> (dx0 fp32 (M, D), bf16(dx0 * mask) or None).

    ``dy2`` = bf16(dx2 * dropout_mask(p, s3)) if the producer of dx2 already emitted it;
    ``emit_for`` = (p, seed) of the consumer of dx0 (the FFN2 mask of the block below):
    the last LayerNorm-backward then also writes that masked bf16 operand, so no
    stand-alone cast/mask pass runs between GEMMs.
    ``bn_below`` = {"s": saved dict of the conv block whose output is this block's input}: the last launch also forms
    that block's BatchNorm-backward sums (returned as ``bn_below["sums"]`` when the shapes allow the fusion).
    Which launches run: ``block_bwd_plan`` of the plan the forward saved."""
    blk = s["blk"]
    p = s["p"]
    s1, s2, s3 = s["seeds"]
    B, L = s["B"], s["L"]
    M, D = s["x1"].shape
    at = blk.self_attn
    yb = bn_below["s"]["y"] if bn_below is not None else None
    form = block_bwd_plan(s["plan"], yb is not None and emit_for is None and yb.shape[2] == 128
                          and bn_below["s"]["pool"] == 1 and yb.shape[0] * yb.shape[1] == M)
    res_rows = 0
    if isinstance(dx2, tuple):                          # (one fp32 row per sample (B, D), tokens per sample): pooled_head_bwd
        rows, per = dx2
        if form.head_rows:
            dx2, res_rows = rows, per                   # the LayerNorm-backward launch reads the row (res_rows)
        else:                                           # no consumer for the row form: materialise the token gradients
            dx2 = rows.view(-1, 1, D).expand(-1, per, D).reshape(M, D).contiguous()
    # FFN second linear:  x2 = x1 + drop(g W2^T + b2);  g = drop(act(z))
    if dy2 is None:
        dy2 = _mask_cast(g_f32=dx2, drop_p=p, seed=s3)
    dx1 = _empty((M, D), _F32, dx2)
    dyo = _empty((M, D), _BF, dx2)                      # bf16(dx1 * mask1): out-proj backward operand
    dgb = _zeros((REPL, 2, D), dx2)
    # attention output projection:  x1 = x0 + drop(o Wo^T + bo): at width 128 its data gradient is a second GEMM inside the
    # launch above it (FFN-1 data gradient + norm2 backward), fed by the masked rows before they leave the workgroup
    wd_o = ops.weights.get(at.out_proj.weight, True)[1] if form.ffn in ("ffn_rows", "ln_gemm2") else None
    if form.ffn == "ffn_rows":
        # ... and with an FFN width that fits the workgroup's LDS the FFN-2 data gradient heads the same launch: the dz rows
        # feed the FFN-1 data gradient before they leave the workgroup (mm_ffn_rows_bwd); the three weight gradients as below
        n1 = s["z"].shape[-1]
        _, wd2, cinp2, coutp2 = ops.weights.get(blk.linear2.weight, True)
        _, wd1, cinp1, coutp1 = ops.weights.get(blk.linear1.weight, True)
        if (cinp2, coutp2, cinp1, coutp1) != (n1, D, D, n1):
            raise _hip.HipLibraryError(f"transformer_block_bwd: FFN weight images {cinp2} x {coutp2}, {cinp1} x {coutp1} != width {D}, hidden {n1}")
        linear_bwd(bag, dy2, s["g"], blk.linear2.weight, blk.linear2.bias, need_dx=False)
        dz = _empty((M, n1), _BF, dx2)
        do = _empty((M, D), _BF, dx2)
        _hip.call("mm_ffn_rows_bwd", dy2, wd2, M, n1, s["z"], ACT[blk._act], float(p), int(s2), dz, wd1, s["x1"], s["st2"],
                  blk.norm2.weight, dx2, int(res_rows), dx1, dyo, dgb, float(p), int(s1), ops.EP(), wd_o, do)
        linear_bwd(bag, dz, s["h2"], blk.linear1.weight, blk.linear1.bias, need_dx=False)
    else:
        dz = linear_bwd(bag, dy2, s["g"], blk.linear2.weight, blk.linear2.bias, below=(s["z"], blk._act, p, s2))
        do = _linear_ln_bwd(bag, form.ffn, dz, s["h2"], blk.linear1.weight, blk.linear1.bias, s["x1"], s["st2"], blk.norm2,
                            dx2, dx1, dyo, dgb, float(p), int(s1), w2=wd_o, res_rows=res_rows)
    _ln_param_grads(bag, blk.norm2, dgb, D)
    if do is None:
        do = linear_bwd(bag, dyo, s["o"].view(M, D), at.out_proj.weight, at.out_proj.bias)
    else:
        linear_bwd(bag, dyo, s["o"].view(M, D), at.out_proj.weight, at.out_proj.bias, need_dx=False)
    dqkv = _empty((B, L, 3 * D), _BF, dx2)
    delta = _empty((B, blk.nhead, L), _F32, dx2)
    dh = D // blk.nhead
    pa, sa = s.get("attn_drop", (0.0, 0))
    entry = ops.attn_entry(D, blk.nhead, "bwd")
    _hip.call(entry, s["qkv"], s["o"], do, s["lse"], dqkv, delta, B, L, blk.nhead, dh, float(dh) ** -0.5,
              float(pa), int(sa), ops.EP(), s.get("mask"), ops.attn_mask_per_head(s.get("mask"), B, blk.nhead, L))
    dx0 = _empty((M, D), _F32, dx2)
    emit = _empty((M, D), _BF, dx2) if emit_for is not None else None
    ep, es = emit_for if emit_for is not None else (0.0, 0)
    dgb = _zeros((REPL, 2, D), dx2)
    _linear_ln_bwd(bag, form.qkv, dqkv.view(M, 3 * D), s["h1"], at.in_proj_weight, at.in_proj_bias, s["x"], s["st1"],
                   blk.norm1, dx1, dx0, emit, dgb, float(ep), int(es), bn_below=bn_below)
    _ln_param_grads(bag, blk.norm1, dgb, D)
    return dx0, emit


def pooled_head_bwd(bag: GradBag, s: dict, dout: torch.Tensor, emit_for=None, rows_only=False):
    """dout fp32 (B, H) -> d tokens fp32 (B, L, D); with ``emit_for`` = (p, seed) of the consumer also its
    dropout-masked bf16 copy, returned as a pair (fused head only, else None).
    ``rows_only`` (fused head): returns (d pooled SUM fp32 (B, D), 1 / L) instead - every token's gradient is that row
    times the scale, and a consumer that can take it in this form (mm_bn_act_bwd_*_bcast) saves the (B, L, D) tensor;
    with ``emit_for`` (the chain's form) ((one fp32 row per sample for the consumer's skip path, L), masked bf16 tokens for
    its GEMMs)."""
    lin = s["lin"]
    B, L, D = s["B"], s["L"], s["D"]
    if s.get("fused"):
        N = lin.weight.shape[0]
        dout = dout.contiguous()
        rows = rows_only and not _NO_BCAST
        # only the entry point, the gradient buffer and the token count the kernel spreads it over differ
        if rows and emit_for is not None:
            entry, shape, Lk = "mm_pooled_head_bwd_rows", (B, D), L
        else:
            entry, shape, Lk = "mm_pooled_head_bwd", (B, 1 if rows else L, D), 1 if rows else L
        dz = _empty((B, N), _BF, dout)
        dx = _empty(shape, _F32, dout)
        emit = _empty((B, L, D), _BF, dout) if emit_for is not None else None
        ep, es = emit_for if emit_for is not None else (0.0, 0)
        _hip.call(entry, dout, s["z"], lin.weight, dz, dx, emit, B, Lk, D, N, ACT[s["act"]],
                  float(s["drop_p"]), int(s["seed"]), float(ep), int(es), ops.EP())
        linear_bwd(bag, dz, s["pooled"], lin.weight, lin.bias, need_dx=False)
        if rows:
            return ((dx, L), emit) if emit_for is not None else (dx.view(B, D), 1.0 / L)
        return (dx, emit) if emit_for is not None else dx
    if emit_for is not None:
        return pooled_head_bwd(bag, s, dout), None
    dz = _mask_cast(g_f32=dout.contiguous(), z=s["z"], act=s["act"], drop_p=s["drop_p"], seed=s["seed"])
    dpool = linear_bwd(bag, dz, s["pooled"], lin.weight, lin.bias, dx_f32=True)
    dx = _empty((B, L, D), _F32, dout)
    _hip.call("mm_meanpool_bwd", dpool, dx, B, L, D)
    return dx


def _module_params(m) -> List[torch.nn.Parameter]:
    return [p for p in m.parameters()]


class _ModuleFn(torch.autograd.Function):
    """shared plumbing: forward(ctx, module, x, *params) with params passed only
    so that autograd tracks them."""

    @staticmethod
    def _finish(ctx, bag, params, dx):
        return (None, dx) + tuple(bag.result(p) for p in params)


def erp_encoder_bwd(bag: GradBag, sv: dict, dout: torch.Tensor, need_dx: bool = False, after_blocks=None,
                    after_conv2=None, after_conv3=None):
    """backward of ops._erp_forward_impl (train mode); dout fp32 (B, H).  ``after_blocks()`` is called
    once the transformer stack's backward has been issued, ``after_conv2()`` once the second conv block's
    has (a trainer hands the reductions / weight gradients collected so far to another stream there)."""
    blocks = sv["blocks"]
    dy2 = None
    if blocks:                                       # the head's backward also writes the top block's masked operand
        d, dy2 = pooled_head_bwd(bag, sv["head"], dout, emit_for=(blocks[-1]["p"], blocks[-1]["seeds"][2]), rows_only=True)
    else:
        d = pooled_head_bwd(bag, sv["head"], dout)
    if isinstance(d, tuple):                         # (row per sample, tokens per sample): the top block reads the row
        B, L, D = dy2.shape
    else:
        B, L, D = d.shape
        d = d.view(B * L, D)
    if dy2 is not None:
        dy2 = dy2.view(B * L, D)
    c3, c2, c1 = sv["convs"][2], sv["convs"][1], sv["convs"][0]
    bn3 = {"s": c3}
    for i in range(len(blocks) - 1, -1, -1):
        below = (blocks[i - 1]["p"], blocks[i - 1]["seeds"][2]) if i > 0 else None
        d, dy2 = transformer_block_bwd(bag, blocks[i], d, dy2=dy2, emit_for=below, bn_below=bn3 if i == 0 else None)
    if after_blocks is not None:
        after_blocks()
    g, sm = conv_bn_act_bwd(bag, c3, dout_f32=d.view(B, L, D), sums=bn3.get("sums"), below=c2)
    if after_conv3 is not None:
        after_conv3()
    g, sm = conv_bn_act_bwd(bag, c2, dout_bf16=g, sums=sm, below=c1)
    if after_conv2 is not None:
        after_conv2()
    g = conv_bn_act_bwd(bag, c1, dout_bf16=g, need_dx=need_dx, sums=sm)
    if not need_dx:
        return None
    Bx, C, T = sv["x_shape"]
    dx = _empty((Bx, C, T), _F32, dout)
    _hip.call("mm_unpack_ntc_f32", g, dx, Bx, C, T, g.shape[2])
    return dx


class ErpEncoderFn(_ModuleFn):
    """train mode, or eval mode with a backward to follow (frozen BatchNorm: running statistics,
    no dropout) - the latter serves fine-tuning on a frozen encoder and gradient saliency
    (bridge_utils.py:158-229)."""

    @staticmethod
    def run(m, x):
        return ErpEncoderFn.apply(m, x, *_module_params(m))

    @staticmethod
    def forward(ctx, m, x, *params):
        out, saved = ops._erp_forward_impl(m, x.float(), m.training, True, save=True)
        ctx.m, ctx.saved, ctx.params = m, saved, params
        ctx.need_dx = x.requires_grad
        return out

    @staticmethod
    def backward(ctx, dout):
        bag = GradBag()
        with deferred(bag, dout.device):
            dx = erp_encoder_bwd(bag, ctx.saved, dout, ctx.need_dx)
        return _ModuleFn._finish(ctx, bag, ctx.params, dx)


def power_encoder_bwd(bag: GradBag, sv: dict, dout: torch.Tensor, need_dx: bool = False):
    """backward of ops._power_forward_impl; returns (dx packed bf16 (B, T, Cp) or None, finish) where
    ``finish()`` must run AFTER the bag's deferred reductions were flushed: it slices the merged
    192-channel conv / BatchNorm gradients back into the three conv_scale modules."""
    d = pooled_head_bwd(bag, sv["head"], dout)
    B, L, D = d.shape
    d = d.view(B * L, D)
    blocks = sv["blocks"]
    dy2 = None
    for i in range(len(blocks) - 1, -1, -1):
        below = (blocks[i - 1]["p"], blocks[i - 1]["seeds"][2]) if i > 0 else None
        d, dy2 = transformer_block_bwd(bag, blocks[i], d, dy2=dy2, emit_for=below)
    g = conv_bn_act_bwd(bag, sv["convs"][1], dout_f32=d.view(B, L, D))
    g = conv_bn_act_bwd(bag, sv["convs"][0], dout_bf16=g, need_dx=need_dx)
    conv, bn, seqs = sv["merged"]

    def finish():
        # ONE launch adds the merged bias / BatchNorm gradients' slices into the real parameters' sinks (it was twelve sliced
        # add_); the weight gradients went straight from the slot workspace into the three real tensors (conv_bn_act_bwd)
        tg = lambda ps: [bag.target(p) for p in ps]       # noqa: E731
        none3 = [None] * 3
        ops.power_merge_call(2, (tg([sq[0].weight for sq in seqs]), tg([sq[0].bias for sq in seqs]), tg([sq[1].weight for sq in seqs]),
                                 tg([sq[1].bias for sq in seqs]), none3, none3),
                             [bag.result(conv.weight), bag.result(conv.bias), bag.result(bn.weight), bag.result(bn.bias), None, None],
                             cin=conv.in_channels, ks=[sq[0].kernel_size[0] for sq in seqs])
    return g, finish


class PowerEncoderFn(_ModuleFn):
    """EnhancedPowerEncoder (train, or eval with a backward to follow).  ``packed``: x is already the
    channels-last bf16 (B, T, Cp) image (STFT front-end output) and gets no gradient."""

    @staticmethod
    def run(m, x, packed=False):
        return PowerEncoderFn.apply(m, x, packed, *_module_params(m))

    @staticmethod
    def forward(ctx, m, x, packed, *params):
        xb = x if packed else ops.pack_nct(x.float())
        need_dx = bool(x.requires_grad)                  # packed: the gradient goes back as the packed bf16 image (StftFrontEndFn)
        out, saved = ops._power_forward_impl(m, xb, m.training, need_dx, save=True)
        ctx.saved, ctx.params = saved, params
        ctx.need_dx, ctx.x_shape, ctx.packed = need_dx, tuple(x.shape), bool(packed)
        return out

    @staticmethod
    def backward(ctx, dout):
        bag = GradBag()
        with deferred(bag, dout.device):
            g, finish = power_encoder_bwd(bag, ctx.saved, dout.contiguous(), ctx.need_dx)
        finish()
        dx = None
        if ctx.need_dx and ctx.packed:
            dx = g
        elif ctx.need_dx:
            Bx, C, T = ctx.x_shape
            dx = _empty((Bx, C, T), _F32, dout)
            _hip.call("mm_unpack_ntc_f32", g, dx, Bx, C, T, g.shape[2])
        return (None, dx, None) + tuple(bag.result(p) for p in ctx.params)


class StftFrontEndFn(torch.autograd.Function):
    """multi-scale STFT power front-end [+ per-sample z-score] as a differentiable step: raw EEG (B, C, T) fp32 ->
    channels-last bf16 spectra (B, frames, Cp).  Backward: the gradient w.r.t. the packed spectra -> z-score backward
    (fp32) -> per scale, the gradient of |DFT(window * frame)|^2 gathered back onto the samples (mm_stft_power_bwd) ->
    d / d raw EEG (saliency / integrated gradients on the config-#5 model)."""

    @staticmethod
    def forward(ctx, x, n_ffts, hop, normalize):
        xc = x.float().contiguous()
        out, spec = ops.stft_front_end(xc, n_ffts, hop, normalize, keep_spec=True)
        ctx.save_for_backward(xc, spec if spec is not None else out)
        ctx.cfg = (tuple(n_ffts), int(hop), bool(normalize))
        return out

    @staticmethod
    def backward(ctx, g):
        xc, spec = ctx.saved_tensors
        n_ffts, hop, normalize = ctx.cfg
        B, C, T = xc.shape
        frames, cp = g.shape[1], g.shape[2]
        widths = [C * (n // 2 + 1) for n in n_ffts]
        g = g.contiguous()
        if normalize:
            gp = _empty((B, frames, cp), _F32, g)
            _hip.call("mm_sample_zscore_bwd", spec, g, gp, B, frames, sum(widths), cp, 1e-8)
        else:
            gp = g.float()
        dx = torch.zeros_like(xc)
        off = 0
        for n, wdt in zip(n_ffts, widths):
            _hip.call("mm_stft_power_bwd", xc, gp, dx, B, C, T, int(n), hop, off, cp)
            off += wdt
        return dx, None, None, None


class AddPositionalFn(torch.autograd.Function):
    """stand-alone PositionalEncoding.forward (enhanced_models_v4.py:44-55): dropout(x + pe[:L]);
    backward = the same counter-hash mask on the incoming gradient."""

    @staticmethod
    def forward(ctx, x, pe, p):
        seed = ops._next_seed() if p > 0 else 0
        ctx.p, ctx.seed, ctx.dtype = p, seed, x.dtype
        return ops.add_positional_impl(x, pe, p, seed)

    @staticmethod
    def backward(ctx, dout):
        if ctx.p > 0:
            dx = ops.add_positional_impl(dout, None, ctx.p, ctx.seed, backward=True)
        else:
            dx = dout
        return dx.to(ctx.dtype), None, None


class TransformerBlockFn(_ModuleFn):
    @staticmethod
    def run(blk, x, mask=None):
        return TransformerBlockFn.apply(blk, x, mask, *_module_params(blk))

    @staticmethod
    def forward(ctx, blk, x, mask, *params):
        xf = x.float().contiguous()
        out, saved = ops.transformer_block_fwd(xf, blk, blk.training, True, save=True, mask=mask)
        ctx.blk, ctx.saved, ctx.params = blk, saved, params
        return out

    @staticmethod
    def backward(ctx, dout):
        bag = GradBag()
        B, L, D = dout.shape
        with deferred(bag, dout.device):
            dx, _ = transformer_block_bwd(bag, ctx.saved, dout.contiguous().view(B * L, D).float())
        return (None, dx.view(B, L, D), None) + tuple(bag.result(p) for p in ctx.params)


def conv3d_bn_act_bwd(bag: GradBag, s: dict, dout, need_dx=True):
    """backward of ops.conv3d_bn_act (train, or eval with frozen BatchNorm: ``s["train"]`` False). dout: bf16 pooled
    volume, or fp32 (B, V, N) for the un-pooled last stage.  returns dx bf16 (B,D,H,W,Cinp)."""
    conv, bn = s["conv"], s["bn"]
    y, out4, xv = s["y"], s["out4"], s["xv"]
    B, D, H, W, N = y.shape
    train = 1 if s.get("train", True) else 0
    sums = _zeros((REPL, 2, N), y)
    dy = _empty((B, D, H, W, N), _BF, y)
    gelu = ACT["gelu"]
    if s["pool"]:
        _hip.call("mm_pool3d_bn_act_bwd_reduce", s["ysel"], out4, dout, sums, B, D, H, W, N, gelu,
                  float(s["drop_p"]), int(s["seed"]), ops.EP())
        # the apply passes sum the workspace's replicas themselves (no compaction launch between the two passes)
        _hip.call("mm_pool3d_bn_act_bwd_apply", y, s["arg"], out4, dout, sums, dy, B, D, H, W, N, gelu,
                  float(s["drop_p"]), int(s["seed"]), ops.EP(), train, REPL)
    elif isinstance(dout, tuple):                       # (one fp32 row per sample, scale): pooled_head_bwd(rows_only=True)
        rows, scale = dout
        _hip.call("mm_bn_act_bwd_reduce_bcast", y, out4, rows, float(scale), sums, B, D * H * W, N, gelu,
                  float(s["drop_p"]), int(s["seed"]), ops.EP())
        _hip.call("mm_bn_act_bwd_apply_bcast", y, out4, rows, float(scale), sums, dy, B, D * H * W, N, gelu,
                  float(s["drop_p"]), int(s["seed"]), ops.EP(), train, REPL)
    else:
        args = (B, D * H * W, N, gelu, 1, 1, float(s["drop_p"]), int(s["seed"]), 0.0, 0, ops.EP())
        _hip.call("mm_bn_act_bwd_reduce", y, out4, None, dout, sums, *args)
        _hip.call("mm_bn_act_bwd_apply", y, out4, None, dout, sums, dy, None, *args, train, REPL)
    _bn_param_grads(bag, bn, sums, N, nrep=REPL)
    cin = conv.in_channels
    dw = bag.target(conv.weight)
    if dw is not None:
        cinp_x = xv.shape[4]
        db = bag.target(conv.bias)
        dbr = _zeros((REPL, N), y) if db is not None else None
        slots = _hip.host_int("mm_conv3d_wgrad_slots", B, D, H, W, cinp_x, N)
        ws = _empty((slots, N, 27, cinp_x), _F32, y)           # one writer per element: no atomics, no memset
        end = ops.kernel_timer.bracket(f"conv3d_wgrad_c{cinp_x}")     # (bench.py's roofline_family; off by default)
        _hip.call("mm_conv3d_wgrad", dy, xv, ws, dbr, B, D, H, W, cinp_x, N, cinp_x,
                  27 * cinp_x, 1, cinp_x, slots, N * 27 * cinp_x, 1)
        if end is not None:
            end.record()
        _scatter_into(dw, ws, N, cin, 27, cinp_x, slots)
        if db is not None:
            _reduce_into(db, dbr, N, N)
    if not need_dx:
        return None
    _, wd, cinp, coutp = ops.weights.get(conv.weight, True)
    assert coutp == N
    dx = _empty((B, D, H, W, cinp), _BF, y)
    end = ops.kernel_timer.bracket(f"conv3d_dgrad_c{N}")
    _hip.call("mm_conv3d_fwd", dy, wd, B, D, H, W, N, cinp, None, None, None, dx)
    if end is not None:
        end.record()
    return dx


def conv3d_l1_bwd(bag: GradBag, s: dict, dout: torch.Tensor):
    """backward of ops.conv3d_l1_bn_act (no input gradient: the volume is data; a caller that wants one runs
    layer 1 through conv3d_bn_act, ops._vol_forward_impl(need_dx=True))."""
    conv, bn, x = s["conv"], s["bn"], s["x"]
    B, _, D, H, W = x.shape
    train = 1 if s.get("train", True) else 0
    # one recompute pass: S1 / S2 and A1 = x^T dz; BatchNorm's backward is linear in S1, S2, and its two correction terms
    # come from the forward pass's compact Gram matrix (csrc/conv3d_l1.hip)
    sums = _zeros((REPL, 2, 32), x)
    dw = bag.target(conv.weight)
    if dw is None:                                   # frozen conv weight: the sums alone (BatchNorm gradients)
        _hip.call("mm_conv3d_l1", 2, x, s["wimg"], conv.bias, s["out4"], dout, None, sums, None, None, None,
                  B, D, H, W, train, float(s["drop_p"]), int(s["seed"]), ops.EP())
    else:
        a1 = _zeros((REPL, 27, 32), x)
        _hip.call("mm_conv3d_l1_bwd", x, s["wimg"], conv.bias, s["out4"], dout, sums, a1, s.get("gramc") if train else None,
                  dw, bag.target(conv.bias), B, D, H, W, train, float(s["drop_p"]), int(s["seed"]), ops.EP())
    _bn_param_grads(bag, bn, sums, 32, nrep=REPL)


def volume_encoder_bwd(bag: GradBag, sv: dict, dout: torch.Tensor):
    """backward of ops._vol_forward_impl (train mode, or eval with frozen BatchNorm); dout fp32 (B, out_dim).
    Returns d / d volume (fp32, the input's shape) when the forward was run with need_dx, else None."""
    last = sv["convs"][2]
    d = pooled_head_bwd(bag, sv["head"], dout, rows_only=not last["pool"])     # fp32 (B, V, N), or (row per sample, 1 / V)
    g = conv3d_bn_act_bwd(bag, last, d)
    g = conv3d_bn_act_bwd(bag, sv["convs"][1], g)
    if sv["convs"][0].get("l1"):
        conv3d_l1_bwd(bag, sv["convs"][0], g)
        return None
    need_dx = bool(sv.get("need_dx"))
    dxp = conv3d_bn_act_bwd(bag, sv["convs"][0], g, need_dx=need_dx)
    if not need_dx:
        return None
    Bx, C, D, H, W = sv["x_shape"]
    return dxp[..., :C].permute(0, 4, 1, 2, 3).float().contiguous()      # (B, D, H, W, Cp) bf16 -> (B, C, D, H, W) fp32


class VolumeEncoderFn(_ModuleFn):
    """train mode, or eval mode with a backward to follow (frozen BatchNorm: running statistics, no dropout, no
    statistic update) - fine-tuning on a frozen voxel encoder and gradient saliency / integrated gradients on an
    end-to-end voxel path (the protocol of bridge_utils.py:158-229)."""

    @staticmethod
    def run(m, x):
        return VolumeEncoderFn.apply(m, x, *_module_params(m))

    @staticmethod
    def forward(ctx, m, x, *params):
        ctx.need_dx = bool(x.requires_grad)
        out, saved = ops._vol_forward_impl(m, x.float(), m.training, True, save=True, need_dx=ctx.need_dx)
        ctx.saved, ctx.params = saved, params
        return out

    @staticmethod
    def backward(ctx, dout):
        bag = GradBag()
        with deferred(bag, dout.device):
            dx = volume_encoder_bwd(bag, ctx.saved, dout)
        return _ModuleFn._finish(ctx, bag, ctx.params, dx)


def _lag_param_grads(bag: GradBag, query, lag_bias, dparts: torch.Tensor, B: int, F: int, N: int):
    """dparts (B, N + F) = mm_lagpool_bwd's per-sample rows (dq_b | dc_b): their sums in ascending b go into the two
    parameter gradients with the bag's batched reduction (descriptors of B fp32 rows: no launch of their own)"""
    for p, K, off in ((query, N, 0), (lag_bias, F, N)):
        dst = bag.target(p)
        if dst is not None:
            bag.defer(dparts.data_ptr() + 4 * off, dst, K, -B, N + F, keep=dparts)


class LagPoolFn(torch.autograd.Function):
    """`ops.lag_pool_fwd` on the tape: (x (B, F, N), query, lag_bias) -> (out, weights); the weights are a read-out"""

    @staticmethod
    def forward(ctx, x, query, lag_bias):
        out, attw = ops.lag_pool_fwd(x, query, lag_bias)
        ctx.saved = (x.detach().float().contiguous(), attw, query, lag_bias)
        ctx.mark_non_differentiable(attw)
        return out, attw

    @staticmethod
    def backward(ctx, dout, _dweights):
        x, attw, query, lag_bias = ctx.saved
        B, F, N = x.shape
        dx, dparts = ops.lag_pool_bwd(dout.contiguous(), x, attw, query)
        bag = GradBag()
        with deferred(bag, dout.device):
            _lag_param_grads(bag, query, lag_bias, dparts, B, F, N)
        return dx if ctx.needs_input_grad[0] else None, bag.result(query), bag.result(lag_bias)


def sequence_encoder_bwd(bag: GradBag, sv: dict, dout: torch.Tensor):
    """backward of ops._seq_forward_impl; dout fp32 (B, out_dim): the pool's backward (mm_lagpool_bwd, one launch; its
    parameter rows ride in the bag's reduction), then `volume_encoder_bwd` on the B * F volumes with the pool's dx as its
    dout.  Returns d / d frames (B, F, D, H, W) when the forward was run with need_dx, else None."""
    B, F = sv["B"], sv["F"]
    N = dout.shape[1]
    dx, dparts = ops.lag_pool_bwd(dout.contiguous(), sv["feats"].view(B, F, N), sv["weights"], sv["pool"].query)
    _lag_param_grads(bag, sv["pool"].query, sv["pool"].lag_bias, dparts, B, F, N)
    dvol = volume_encoder_bwd(bag, sv["vol"], dx.view(B * F, N))
    return None if dvol is None else dvol.view(B, F, *dvol.shape[2:])


class SequenceEncoderFn(_ModuleFn):
    """`fMRISequenceEncoder3D` on the tape -> (features, lag weights): train mode, or eval mode with a backward to follow
    (frozen BatchNorm, no dropout, no statistic update), as `VolumeEncoderFn`"""

    @staticmethod
    def run(m, x):
        return SequenceEncoderFn.apply(m, x, *_module_params(m))

    @staticmethod
    def forward(ctx, m, x, *params):
        ctx.need_dx = bool(x.requires_grad)
        out, saved = ops._seq_forward_impl(m, x, m.training, save=True, need_dx=ctx.need_dx)
        ctx.saved, ctx.params = saved, params
        ctx.mark_non_differentiable(saved["weights"])
        return out, saved["weights"]

    @staticmethod
    def backward(ctx, dout, _dweights):
        bag = GradBag()
        with deferred(bag, dout.device):
            dx = sequence_encoder_bwd(bag, ctx.saved, dout)
        return _ModuleFn._finish(ctx, bag, ctx.params, dx)


def fmri_tab_bwd(bag: GradBag, sv: dict, dout: torch.Tensor):
    """backward of ops._tab_forward_impl (train mode, or frozen BatchNorm), ONE launch (mm_fmri_tab_bwd); dout fp32
    (B, hidden_dim).  Every parameter gradient is written into its `GradBag` target with PLAIN stores (the launch is the
    target's only writer: one backward of an encoder per step).  Returns d / d x (B, A + C) when the forward was run
    with need_dx, else None."""
    m, x = sv["enc"], sv["x"]
    B, A, C, H = sv["B"], m.activation_dim, m.connectivity_dim, m.hidden_dim
    layers = m.layers()
    t = bag.target
    scratch = _empty((ops.fmri_tab_scratch_floats(B, A, C, H),), _F32, dout)
    dx = _empty((B, A + C), _F32, dout) if sv.get("need_dx") else None
    ins = [q for lin, bn in layers for q in (lin.weight, bn.weight)]
    outs = [t(q) for lin, bn in layers for q in (lin.weight, lin.bias, bn.weight, bn.bias)]
    _hip.call("mm_fmri_tab_bwd", dout.float().contiguous(), x, sv["out"], sv["save"], B, A, C, H, *ins, m.activation_weight,
              m.connectivity_weight, scratch, dx, *outs, t(m.activation_weight), t(m.connectivity_weight),
              int(sv["train"]), sv["eps"], float(sv["p"]))
    return dx


class FmriTabFn(_ModuleFn):
    """`fMRITabularEncoder` on the autograd tape: train mode, or eval mode with a backward to follow (frozen BatchNorm:
    running statistics, no dropout, no statistic update) - attribution and fine-tuning on a frozen encoder."""

    @staticmethod
    def run(m, x):
        return FmriTabFn.apply(m, x, *_module_params(m))

    @staticmethod
    def forward(ctx, m, x, *params):
        ctx.need_dx = bool(x.requires_grad)
        out, saved = ops._tab_forward_impl(m, x, m.training, True, need_dx=ctx.need_dx)
        ctx.saved, ctx.params = saved, params
        return out

    @staticmethod
    def backward(ctx, dout):
        bag = GradBag()
        with deferred(bag, dout.device):
            dx = fmri_tab_bwd(bag, ctx.saved, dout)
        return _ModuleFn._finish(ctx, bag, ctx.params, dx)


# ------------------------------------------------ projection bridge / loss
def proj_head_bwd(bag: GradBag, s: dict, da: torch.Tensor, need_dx=True):
    lin, ln = s["seq"][0], s["seq"][1]
    B, N = da.shape
    K = lin.weight.shape[1]
    dhn = _empty((B, N), _F32, da)
    _hip.call("mm_act_bwd_f32", da, s["hn"], dhn, B * N, ACT["gelu"], float(s["p"]), int(s["seed"]), ops.EP())
    dz1 = _empty((B, N), _F32, da)
    dgb = _zeros((REPL, 2, N), da)
    _hip.call("mm_layernorm_bwd", None, dhn, s["z1"], s["stat"], ln.weight, None, dz1, None, dgb, B, N, 0.0, 0, None)
    _ln_param_grads(bag, ln, dgb, N)
    dx = _empty((B, K), _F32, da) if need_dx else None
    _hip.call("mm_small_linear_bwd", dz1, s["x"], lin.weight, dx, bag.target(lin.weight), bag.target(lin.bias), B, K, N)
    return dx


def contrastive_embed_bwd(bag: GradBag, s: dict, dz: torch.Tensor, need=(True, True)):
    """dz (B, 2N) packed -> (d eeg_feat (B, eeg_dim), d fmri_feat (B, fmri_dim))"""
    B, N = s["B"], s["N"]
    br = s["bridge"]
    (le, lne), (lf, lnf) = br.eeg_proj[:2], br.fmri_proj[:2]
    xe, xf = s["xe"], s["xf"]
    dxe = _empty(xe.shape, _F32, dz) if need[0] else None
    dxf = _empty(xf.shape, _F32, dz) if need[1] else None
    t = bag.target
    _hip.call("mm_proj_heads_bwd", dz.contiguous(), s["z"], s["nrm"], s["hn"], s["z1"], s["stat"],
              xe, le.weight, lne.weight, xe.shape[1], xf, lf.weight, lnf.weight, xf.shape[1],
              dxe, t(le.weight), t(le.bias), t(lne.weight), t(lne.bias),
              dxf, t(lf.weight), t(lf.bias), t(lnf.weight), t(lnf.bias),
              B, N, float(s["p"]), int(s["seeds"][0]), int(s["seeds"][1]), ops.EP())
    return dxe, dxf


def contrastive_embed_bwd_da(bag: GradBag, s: dict, dz: torch.Tensor, da: torch.Tensor, need=(True, True)):
    """`contrastive_embed_bwd` with ``da`` (2, B, N), a second gradient at the heads' post-dropout activations (the
    classification branch's, `bridge_cls_bwd`): mm_proj_heads_bwd_da in place of mm_proj_heads_bwd"""
    B, N = s["B"], s["N"]
    br = s["bridge"]
    (le, lne), (lf, lnf) = br.eeg_proj[:2], br.fmri_proj[:2]
    xe, xf = s["xe"], s["xf"]
    dxe = _empty(xe.shape, _F32, dz) if need[0] else None
    dxf = _empty(xf.shape, _F32, dz) if need[1] else None
    t = bag.target
    _hip.call("mm_proj_heads_bwd_da", dz.contiguous(), da, s["z"], s["nrm"], s["hn"], s["z1"], s["stat"],
              xe, le.weight, lne.weight, xe.shape[1], xf, lf.weight, lnf.weight, xf.shape[1],
              dxe, t(le.weight), t(le.bias), t(lne.weight), t(lne.bias),
              dxf, t(lf.weight), t(lf.bias), t(lnf.weight), t(lnf.bias),
              B, N, float(s["p"]), int(s["seeds"][0]), int(s["seeds"][1]), ops.EP())
    return dxe, dxf


def bridge_cls_bwd(bag: GradBag, s: dict, loss_in=None, loss_total=None) -> torch.Tensor:
    """backward of ``ce_weight * ce`` through the classification branch (``s``: what `ops.bridge_cls_forward_impl`
    saved, with labels): mm_bridge_cls_bwd's two launches.  Every parameter gradient is ADDED to its `GradBag` target;
    -> da (2, B, N), the gradient of the two tokens (`contrastive_embed_bwd_da`).  ``loss_total`` (1,): receives
    ``loss_in[0] + ce_weight * ce`` (plain store of the rows launch)."""
    if s["labels"] is None:
        raise ValueError("bridge_cls_bwd: the forward ran without labels")
    B, N, H, C = s["B"], s["N"], s["H"], s["C"]
    ps = ops.bridge_cls_params(s["bridge"])
    (in_w, in_b, out_w, out_b, g0_w, g0_b, g3_w, g3_b, fl, temp, c0_w, c0_b, ln_g, ln_b, c4_w, c4_b) = ps
    grad_rows = _empty((_hip.host_int("mm_bridge_cls_ws_floats", B, N, 1),), _F32, s["save"])
    da = _empty((2, B, N), _F32, s["save"])
    pa, sa_, pg, sg, pc, sc = s["drops"]
    for phase in (0, 1):                                     # rows, then weights: one launch each
        _hip.call("mm_bridge_cls_bwd", s["save"], s["logits"], s["loss"], s["labels"], float(s["ce_weight"]),
                  in_w, out_w, g0_w, g3_w, fl, temp, c0_w, ln_g, ln_b, c4_w, grad_rows, da,
                  *[bag.target(p) for p in ps], loss_in, loss_total, phase, B, N, H, C, pa, sa_, pg, sg, pc, sc, ops.EP())
    return da


class ContrastiveEmbedFn(torch.autograd.Function):
    @staticmethod
    def run(bridge, eeg, fmri):
        ps = list(bridge.eeg_proj.parameters()) + list(bridge.fmri_proj.parameters())
        return ContrastiveEmbedFn.apply(bridge, eeg, fmri, *ps)

    @staticmethod
    def forward(ctx, bridge, eeg, fmri, *params):
        z, saved = ops.contrastive_embed_impl(bridge, eeg, fmri, bridge.training)
        ctx.saved, ctx.params = saved, params
        ctx.need = (eeg.requires_grad, fmri.requires_grad)
        return z

    @staticmethod
    def backward(ctx, dz):
        bag = GradBag()
        with deferred(bag, dz.device):
            dxe, dxf = contrastive_embed_bwd(bag, ctx.saved, dz.contiguous(), ctx.need)
        return (None, dxe, dxf) + tuple(bag.result(p) for p in ctx.params)


class ClipLossFn(torch.autograd.Function):
    """z (B, 2N) packed local embeddings -> (loss, acc_e2f, acc_f2e).  With a process group the columns are
    the all-gathered global batch; every rank evaluates all rows of it (``mm_clip_loss_own_rows``), so the
    backward hands out d (sum over ranks of their losses) / d z_local directly - what a reduce-scatter of the
    gathered gradients would deliver - and the usual gradient all-reduce of data parallelism completes it."""

    @staticmethod
    def forward(ctx, z, logit_scale, group, gid=None, radius=0):
        """``gid``: (B,) int32 device group ids (ops.group_ids) -> the grouped loss; gathered like the embeddings.
        ``radius`` > 0: ids within it are ignored keys (``mm_clip_loss_own_rows_masked``)"""
        from . import dp
        z = z.contiguous().float()
        B, N2 = z.shape
        rank = dp.rank(group)
        z_all = dp.gather_embeddings(z, group)
        need_grad = z.requires_grad or logit_scale.requires_grad
        scal = _empty((4,), _F32, z)
        dz = _empty((B, N2), _F32, z) if need_grad else None
        ls = logit_scale.detach().reshape(1).float().contiguous()
        gid_all = None if gid is None else dp.gather_embeddings(gid.view(B, 1), group).view(-1)
        ops.clip_loss_own_rows(z_all, gid_all, ls, scal, dz, B, rank * B, radius)
        if need_grad:
            ctx.save_for_backward(dz, scal)
        return scal[0].clone(), scal[1].clone(), scal[2].clone()

    @staticmethod
    def backward(ctx, g_loss, g_a, g_b):
        dz, scal = ctx.saved_tensors
        return dz * g_loss, (scal[3] * g_loss).reshape(()), None, None, None


class ClipBankLossFn(torch.autograd.Function):
    """`ClipLossFn` against the batch and a cross-batch memory (``mm_clip_bank_loss``): ``bank`` (an `ops.ClipBank`) and its
    state words are constants of the tape - bank rows carry no loss and receive no gradient.  Single process only."""

    @staticmethod
    def forward(ctx, z, logit_scale, bank, gid=None, warmup=0):
        z = z.contiguous().float()
        B, N2 = z.shape
        need_grad = z.requires_grad or logit_scale.requires_grad
        scal = _empty((4,), _F32, z)
        dz = _empty((B, N2), _F32, z) if need_grad else None
        ls = logit_scale.detach().reshape(1).float().contiguous()
        ops.clip_bank_loss(z.detach(), gid, bank, ls, scal, dz, warmup)
        if need_grad:
            ctx.save_for_backward(dz, scal)
        return scal[0].clone(), scal[1].clone(), scal[2].clone()

    @staticmethod
    def backward(ctx, g_loss, g_a, g_b):
        dz, scal = ctx.saved_tensors
        return dz * g_loss, (scal[3] * g_loss).reshape(()), None, None, None


class ClipKeyLossFn(torch.autograd.Function):
    """`ClipBankLossFn` with a momentum key encoder (``mm_clip_key_loss``): the online rows ``q`` are queries only, the key
    rows ``k`` of the same pairs are constants of the tape like the bank - ``k`` carries no gradient."""

    @staticmethod
    def forward(ctx, q, k, logit_scale, bank, gid=None, warmup=0):
        q = q.contiguous().float()
        k = k.detach().contiguous().float()
        B, N2 = q.shape
        need_grad = q.requires_grad or logit_scale.requires_grad
        scal = _empty((4,), _F32, q)
        dq = _empty((B, N2), _F32, q) if need_grad else None
        ls = logit_scale.detach().reshape(1).float().contiguous()
        ops.clip_key_loss(q.detach(), k, gid, bank, ls, scal, dq, warmup)
        if need_grad:
            ctx.save_for_backward(dq, scal)
        return scal[0].clone(), scal[1].clone(), scal[2].clone()

    @staticmethod
    def backward(ctx, g_loss, g_a, g_b):
        dq, scal = ctx.saved_tensors
        return dq * g_loss, None, (scal[3] * g_loss).reshape(()), None, None, None


class SigmoidLossFn(torch.autograd.Function):
    """`ClipLossFn` for the pairwise sigmoid loss (``mm_sigmoid_loss_own_rows``): the same gather of embeddings and ids,
    the same own-rows gradient; one more learnable scalar, ``logit_bias``."""

    @staticmethod
    def forward(ctx, z, logit_scale, logit_bias, group, gid=None, radius=0):
        from . import dp
        z = z.contiguous().float()
        B, N2 = z.shape
        rank = dp.rank(group)
        z_all = dp.gather_embeddings(z, group)
        need_grad = z.requires_grad or logit_scale.requires_grad or logit_bias.requires_grad
        scal = _empty((5,), _F32, z)
        dz = _empty((B, N2), _F32, z) if need_grad else None
        ls = logit_scale.detach().reshape(1).float().contiguous()
        lb = logit_bias.detach().reshape(1).float().contiguous()
        gid_all = None if gid is None else dp.gather_embeddings(gid.view(B, 1), group).view(-1)
        ops.sigmoid_loss_own_rows(z_all, gid_all, ls, lb, scal, dz, B, rank * B, radius)
        if need_grad:
            ctx.save_for_backward(dz, scal)
        return scal[0].clone(), scal[1].clone(), scal[2].clone()

    @staticmethod
    def backward(ctx, g_loss, g_a, g_b):
        dz, scal = ctx.saved_tensors
        return dz * g_loss, (scal[3] * g_loss).reshape(()), (scal[4] * g_loss).reshape(()), None, None, None
