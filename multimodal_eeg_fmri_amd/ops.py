"""Host-side composition of the HIP kernels (``libmmeeg_hip.so``) into the
reference's layers.  PyTorch is used for device memory, streams and autograd
bookkeeping only; every FLOP of the path runs in the C-ABI kernels.

Conventions
-----------
* activations between kernels are channels-last: EEG ``(B, T, C)``, tokens
  ``(B, L, d)``; GEMM operands are bf16, the transformer residual stream, all
  statistics and all parameter gradients are fp32;
* a Linear layer is the ``taps == 1`` case of the 1-D implicit GEMM;
* dropout masks are a counter hash of (seed, element index) recomputed in the
  backward kernels, never stored.
"""
from __future__ import annotations

import functools
import math
import os
import weakref
from typing import Dict, List, NamedTuple, Optional

import torch

from . import _hip, augment_stream

ACT = {"none": 0, "gelu": 1, "relu": 2, "tanh": 3, "sigmoid": 4}
_BF = torch.bfloat16
_F32 = torch.float32


# --------------------------------------------------------------------- helpers
def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _hip.HipLibraryError(
                "multimodal_eeg_fmri_amd runs on the MI355X HIP path only: got a CPU tensor "
                "(no CPU / eager-PyTorch fallback is provided)")
    _hip.load()


def cpad(c: int) -> int:
    """channel count as the MFMA K-chunking wants it: a multiple of 16."""
    c16 = max(16, (c + 15) // 16 * 16)
    return c16


def _empty(shape, dtype, like):
    return torch.empty(shape, dtype=dtype, device=like.device)


REPL = 32          # fp32-sized copies to allocate (and zero) per accumulator workspace (csrc/common.h: MM_REPL) ...
AREPL = 16         # ... which the kernels use as 16 replicas of 64-bit fixed-point sums (MM_ACC_REPL): order-free adds
WREP = 8           # replicas of the conv weight-gradient workspaces
ACC_STAT, ACC_GRAD = 28, 40        # fixed-point fraction bits: activation statistics / gradient sums (csrc/common.h)


def acc_decode(ws: torch.Tensor, k: int) -> torch.Tensor:
    """accumulator workspace (REPL, ...) as the kernels left it -> its fp64 sums (...).  For tests and debugging:
    the product reads workspaces on the device (mm_bn_finalize, mm_acc_reduce, ...)."""
    i = ws.contiguous().flatten().view(torch.int64).view(AREPL, *ws.shape[1:])
    out = i.sum(0).double() * 2.0 ** -k
    # csrc/common.h's overflow contract: a poisoned replica (2^62) or replica magnitudes summing to 2^61 read as NaN
    bad = i.double().abs().sum(0) >= 2.0 ** 61
    return torch.where(bad, torch.full_like(out, float("nan")), out)


def acc_encode(values: torch.Tensor, k: int) -> torch.Tensor:
    """fp sums (...) -> an accumulator workspace (REPL, ...) holding them (replica 0), e.g. to feed mm_bn_finalize"""
    i = torch.zeros((AREPL,) + tuple(values.shape), dtype=torch.int64, device=values.device)
    i[0] = (values.double() * 2.0 ** k).round().long()
    return i.flatten().view(torch.float32).view((REPL,) + tuple(values.shape))


class _Arena:
    """one zeroed fp32 scratch buffer per training step: every accumulator the
    kernels add into (stats, sums, wgrad workspaces ...) is a slice of it, so a
    step pays ONE memset instead of ~40 tiny fill launches."""

    def __init__(self):
        self.buf = None
        self.off = 0
        self.active = False
        self.cleared = 0
        self.high = 0                     # largest offset any step has reached

    def begin(self, device, nfloats: int = 6 << 20, clear: Optional[int] = None, defer_zero: bool = False):
        """``clear``: zero only the first ``clear`` floats (a caller that knows its step's high-water
        mark; slices beyond it fall back to torch.zeros).  ``defer_zero``: the caller zeroes
        ``zero_range()`` itself before the first kernel that uses a slice (the trainer's weight-image launch does)."""
        if self.buf is None or self.buf.device != device or self.buf.numel() < nfloats:
            self.buf = torch.empty(nfloats, dtype=_F32, device=device)
        self.cleared = self.buf.numel() if clear is None else min(int(clear), self.buf.numel())
        self.cleared -= self.cleared % 4
        if not defer_zero:
            self.buf[:self.cleared].zero_()
        self.off = 0
        self.active = True

    def end(self):
        self.active = False

    def zero_range(self):
        """(tensor, floats) a ``begin(defer_zero=True)`` left for the caller to clear"""
        return self.buf, self.cleared

    def take(self, shape, device):
        n = 1
        for d in shape:
            n *= int(d)
        if not self.active or self.buf.device != device or self.off + n > self.cleared:
            return None
        out = self.buf[self.off:self.off + n].view(shape)
        self.off += (n + 63) // 64 * 64
        self.high = max(self.high, self.off)
        return out


arena = _Arena()


def _zeros(shape, like, dtype=_F32):
    if dtype == _F32:
        t = arena.take(tuple(shape), like.device)
        if t is not None:
            return t
    return torch.zeros(shape, dtype=dtype, device=like.device)


_NO_FFN1_FUSE = bool(os.environ.get("MM_NO_FFN1_FUSE"))   # A/B knob: the first FFN Linear as its own launch, not behind the out-projection
_NO_FFN_ROWS = bool(os.environ.get("MM_NO_FFN_ROWS"))     # A/B knob: the second FFN Linear (and its consumers) as its own launch
_NO_QKV_FUSE = bool(os.environ.get("MM_NO_QKV_FUSE"))     # A/B knob: the next block's QKV projection as its own launch
_seed_state = {"base": 0x1234567, "step": 0, "epoch": None}


def set_seed_epoch(t: Optional[torch.Tensor]):
    """device int32 word mixed into every dropout seed ON THE DEVICE; lets a
    hipGraph-captured step draw fresh masks on every replay (None = off)."""
    _seed_state["epoch"] = t


def EP():
    return _seed_state["epoch"]


def set_dropout_seed(seed: int):
    _seed_state["base"] = int(seed) & 0x7FFFFFFF
    _seed_state["step"] = 0


def _next_seed() -> int:
    _seed_state["step"] += 1
    return (_seed_state["base"] * 2654435761 + _seed_state["step"] * 40503) & 0xFFFFFFFF


class _KernelTimer:
    """optional HIP-event bracket around named kernel launches on the current
    stream (bench.py uses it for the roofline line; off by default)."""

    def __init__(self):
        self._ev = {}

    def reset(self, name):
        self._ev[name] = []

    def bracket(self, name):
        lst = self._ev.get(name)
        if lst is None:
            return None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        lst.append((a, b))
        a.record()
        return b

    def all_ms(self, name):
        lst = self._ev.get(name) or []
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in lst]

    def mean_ms(self, name):
        v = self.all_ms(name)
        return sum(v) / len(v) if v else None


kernel_timer = _KernelTimer()


# ------------------------------------------------------------ weight images
class _WeightCache:
    """bf16 MFMA images of fp32 parameters, rebuilt when the parameter changes.

    forward image  ``wf [Cout][k][Cinp]``; data-gradient image
    ``wd [Cinp][k flipped][Coutp]`` (``mm_prep_conv_weight``)."""

    def __init__(self):
        self._gen = 0
        self._store: Dict[int, tuple] = {}
        self._rec = None                      # list of (owner, view shape | None, need_dgrad) while recording

    def invalidate(self):
        self._gen += 1

    # ---- batched preparation: record which images one step asks for, then rebuild them all in
    # ONE launch at the start of every later step (a graph replay otherwise carries ~40 five-
    # microsecond repack nodes on its critical path)
    def start_recording(self):
        self._rec = []

    def stop_recording(self):
        rec, self._rec = self._rec or [], None
        seen, out = {}, []
        for owner, shape, dg in rec:
            k = (id(owner), shape)
            if k in seen:
                out[seen[k]][2] = out[seen[k]][2] or dg
            else:
                seen[k] = len(out)
                out.append([owner, shape, dg])
        return [tuple(e) for e in out]

    @staticmethod
    def _as3d(w: torch.Tensor) -> torch.Tensor:
        wd3 = w.detach()
        if wd3.dim() == 2:
            wd3 = wd3.unsqueeze(-1)
        if wd3.dim() == 5:
            wd3 = wd3.reshape(wd3.shape[0], wd3.shape[1], -1)
        return wd3.contiguous()

    def prepare_all(self, recorded, zero=None):
        """rebuild every recorded image that is out of date with one mm_prep_many launch; ``zero`` = (fp32 tensor,
        floats): the same launch clears that range (the step's accumulator arena)"""
        import ctypes
        import struct
        raw, keep = [], []
        for owner, shape, need_dgrad in recorded:
            w = owner if shape is None else owner.view(shape)
            ver = (owner.data_ptr(), owner._version, self._gen, tuple(w.shape))
            hit = self._store.get(id(owner))
            if hit is not None and hit[5]() is owner and hit[0] == ver and (hit[2] is not None or not need_dgrad):
                continue
            wd3 = self._as3d(w)
            cout, cin, k3 = wd3.shape
            cinp, coutp = cpad(cin), cpad(cout)
            wf = _empty((cout, k3, cinp), _BF, w)
            wd = _empty((cinp, k3, coutp), _BF, w) if need_dgrad else None
            raw.append(struct.pack("<QQQiiiiii", wd3.data_ptr(), wf.data_ptr(), wd.data_ptr() if wd is not None else 0,
                                   cout, cin, k3, cinp, coutp if need_dgrad else 0, 0))
            keep.append(wd3)
            self._store[id(owner)] = (ver, wf, wd, cinp, coutp, weakref.ref(owner))
        if raw:
            buf = b"".join(raw)
            host = ctypes.create_string_buffer(buf, len(buf))
            if zero is not None:
                _hip.call("mm_prep_many_zero", ctypes.addressof(host), len(raw), zero[0], int(zero[1]))
            else:
                _hip.call("mm_prep_many", ctypes.addressof(host), len(raw))
        elif zero is not None:
            zero[0][:int(zero[1])].zero_()

    def seed(self, w: torch.Tensor, wf: torch.Tensor, wd, cinp: int, coutp: int):
        """hand in images that were built elsewhere (mm_power_merge mode 3); ``get(w, ...)`` then returns them as long as
        ``w`` is unchanged and no data-gradient image is asked for that was not handed in"""
        self._store[id(w)] = ((w.data_ptr(), w._version, self._gen, tuple(w.shape)), wf, wd, cinp, coutp, weakref.ref(w))

    def get(self, w: torch.Tensor, need_dgrad: bool, key=None):
        owner = w if key is None else key          # the nn.Parameter the image belongs to
        if self._rec is not None and not getattr(owner, "_mm_transient", False):
            self._rec.append((owner, None if key is None else tuple(w.shape), bool(need_dgrad)))
        k = id(owner)
        ver = (owner.data_ptr(), owner._version, self._gen, tuple(w.shape))
        hit = self._store.get(k)
        # the weak reference rules out a dead parameter whose id/address got reused
        if (hit is not None and hit[5]() is owner and hit[0] == ver
                and (hit[2] is not None or not need_dgrad)):
            return hit[1], hit[2], hit[3], hit[4]
        wd3 = self._as3d(w)
        cout, cin, k3 = wd3.shape
        cinp, coutp = cpad(cin), cpad(cout)
        wf = _empty((cout, k3, cinp), _BF, w)
        wd = _empty((cinp, k3, coutp), _BF, w) if need_dgrad else None
        _hip.call("mm_prep_conv_weight", wd3, wf, wd, cout, cin, k3, cinp, coutp if need_dgrad else 0)
        if len(self._store) > 4096:
            self._store = {i: e for i, e in self._store.items() if e[5]() is not None}
        self._store[k] = (ver, wf, wd, cinp, coutp, weakref.ref(owner))
        return wf, wd, cinp, coutp


weights = _WeightCache()


def weights_changed():
    """call after parameters were updated outside torch's version counter
    (the fused AdamW kernel writes through raw pointers)."""
    weights.invalidate()


# ----------------------------------------------------------- kernel wrappers
def pack_nct(x: torch.Tensor) -> torch.Tensor:
    """(B, C, T) fp32 -> (B, T, Cp) bf16 channels-last, zero-padded channels."""
    B, C, T = x.shape
    cp = cpad(C)
    y = _empty((B, T, cp), _BF, x)
    _hip.call("mm_pack_nct_bf16", x.contiguous(), y, B, C, T, cp)
    return y


# ---- EEG augmentation (csrc/augment.hip; the reference's EEGTransforms).  The stream is counter based and has nothing
# to do with the dropout stream above: no state here, none on the device.
AUG_PURPOSES = augment_stream.PURPOSES["eeg"]


def augment_streams(seed: int, step: int, rank: int = 0) -> tuple:
    """the five 32-bit stream words of one augmentation step, in `AUG_PURPOSES` order: purposes 0..4 of augment_stream.py"""
    return augment_stream.streams("eeg", seed, step, rank)


def _aug_chunks(n: int) -> int:
    """chunks a sample of ``n`` values is summed in: 4096 values each, doubled until there are at most 64 (csrc/aug_stream.h)"""
    chunk = 4096
    while (n + chunk - 1) // chunk > 64:
        chunk *= 2
    return (n + chunk - 1) // chunk


def eeg_augment_check(B: int, C: int, T: int, n_drop: int, who: str = "eeg_augment"):
    """what both the kernels and the CPU path refuse, before anything runs"""
    if min(B, C, T) < 1 or C * T < 2:
        raise ValueError(f"{who}: a sample needs C * T >= 2 values for its standard deviation (got C = {C}, T = {T})")
    if B * C * ((T + 1) // 2) >= 1 << 32:
        raise ValueError(f"{who}: B * C * ceil(T / 2) must stay below 2^32 (the random stream's index)")
    if not 1 <= n_drop <= C:
        raise ValueError(f"{who}: n_drop must lie in [1, {C}] (got {n_drop})")


def eeg_augment_plan_layout(B: int, C: int, T: int):
    """(words, words per sample, chunks per sample) of mm_eeg_augment_plan's buffer (include/mmeeg_hip.h)"""
    stride = (4 + (C + 31) // 32 + 1) & ~1
    nchunk = _aug_chunks(C * T)
    return B * stride + 4 * B * nchunk, stride, nchunk


def eeg_augment_read_plan(plan: torch.Tensor, B: int, C: int, T: int):
    """-> (noise_on bool (B,), drop_mask bool (B, C), std fp32 (B,)) of a plan both launches have written"""
    _, stride, _ = eeg_augment_plan_layout(B, C, T)
    hdr = plan[:B * stride].view(B, stride)
    nw = (C + 31) // 32
    bits = (hdr[:, 4:4 + nw].unsqueeze(-1) >> torch.arange(32, device=plan.device, dtype=torch.int32)) & 1
    return hdr[:, 2] != 0, bits.reshape(B, nw * 32)[:, :C] != 0, hdr[:, 1].contiguous().view(_F32)


# ---- fMRI volume augmentation (csrc/volume_augment.hip), on purposes of its own of the same stream
VOL_AUG_PURPOSES = augment_stream.PURPOSES["volume"]
VOL_AUG_FLAGS = ("flip", "shift", "scale", "noise", "erase")            # bit k of a plan's flag word
_VOL_HDR = 16


def volume_augment_streams(seed: int, step: int, rank: int = 0) -> tuple:
    """the fourteen 32-bit stream words of one volume-augmentation step, in `VOL_AUG_PURPOSES` order: purposes 5..18"""
    return augment_stream.streams("volume", seed, step, rank)


def volume_augment_check(shape, *, p_flip: float, p_shift: float, max_shift: int, p_scale: float, scale_range: float,
                         p_noise: float, noise_factor: float, p_erase: float, erase, fill: float,
                         who: str = "volume_augment"):
    """what both the kernels and the CPU path refuse, before anything runs.  ``shape``: (B, 1, D, H, W); ``erase``: the
    erased cuboid's extents (ed, eh, ew)"""
    if len(shape) != 5:
        raise ValueError(f"{who}: expected a (B, 1, D, H, W) batch, got shape {tuple(shape)}")
    B, C, D, H, W = (int(v) for v in shape)
    if C != 1:
        raise ValueError(f"{who}: volumes have one channel (got C = {C})")
    V = D * H * W
    if min(B, D, H, W) < 1 or V < 2:
        raise ValueError(f"{who}: a sample needs D * H * W >= 2 voxels for its standard deviation (got {D} x {H} x {W})")
    if V >= 1 << 31:
        raise ValueError(f"{who}: D * H * W must stay below 2^31 (the voxel index)")
    if B * ((V + 1) // 2) >= 1 << 32:
        raise ValueError(f"{who}: B * ceil(D * H * W / 2) must stay below 2^32 (the random stream's index)")
    for name, p in (("p_flip", p_flip), ("p_shift", p_shift), ("p_scale", p_scale), ("p_noise", p_noise), ("p_erase", p_erase)):
        if not 0.0 <= p <= 1.0:                                    # (a NaN fails too)
            raise ValueError(f"{who}: {name} must lie in [0, 1] (got {p!r})")
    if int(max_shift) != max_shift or not 0 <= max_shift < min(D, H, W):
        raise ValueError(f"{who}: max_shift must be an integer in [0, min(D, H, W)) = [0, {min(D, H, W)}) (got {max_shift!r})")
    if not 0.0 <= scale_range < 1.0:
        raise ValueError(f"{who}: scale_range must lie in [0, 1) (got {scale_range!r})")
    if not math.isfinite(noise_factor) or not math.isfinite(fill):
        raise ValueError(f"{who}: noise_factor and fill must be finite (got {noise_factor!r}, {fill!r})")
    if len(erase) != 3 or any(int(e) != e or not 1 <= e <= n for e, n in zip(erase, (D, H, W))):
        raise ValueError(f"{who}: the erased cuboid's extents must lie in [1, {D}] x [1, {H}] x [1, {W}] (got {tuple(erase)!r})")


def volume_augment_plan_layout(B: int, D: int, H: int, W: int):
    """(words, words per sample, chunks per sample) of mm_volume_augment_plan's buffer (include/mmeeg_hip.h)"""
    nchunk = _aug_chunks(D * H * W)
    return B * _VOL_HDR + 4 * B * nchunk, _VOL_HDR, nchunk


def _overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def volume_augment_into(x: torch.Tensor, out: torch.Tensor, *, p_flip: float, p_shift: float, max_shift: int, p_scale: float,
                        scale_range: float, p_noise: float, noise_factor: float, p_erase: float, erase, fill: float, seed: int,
                        step: int, rank: int = 0, plan: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the two launches: the plan of batch ``x`` (B, 1, D, H, W) fp32, then the augmented batch into ``out`` (same shape,
    fp32, contiguous, NOT overlapping ``x``: the shift is a gather).  ``plan``: a buffer of `volume_augment_plan_layout`
    words to reuse (a training loop keeps one per batch shape).  -> the plan buffer (int32 words)."""
    kw = dict(p_flip=p_flip, p_shift=p_shift, max_shift=max_shift, p_scale=p_scale, scale_range=scale_range, p_noise=p_noise,
              noise_factor=noise_factor, p_erase=p_erase, erase=erase, fill=fill)
    volume_augment_check(x.shape, **kw)
    if x.dtype != _F32 or out.dtype != _F32 or tuple(out.shape) != tuple(x.shape):
        raise ValueError(f"volume_augment_into: fp32 batches of one shape (got {x.dtype} {tuple(x.shape)} -> {out.dtype} {tuple(out.shape)})")
    if _overlap(x, out):
        raise ValueError("volume_augment_into: source and destination overlap (the shift is a gather: augment into another buffer)")
    _need_gpu(x, out)
    B, _, D, H, W = x.shape
    words, _, _ = volume_augment_plan_layout(B, D, H, W)
    if plan is None:
        plan = torch.empty(words, dtype=torch.int32, device=x.device)
    s = dict(zip(VOL_AUG_PURPOSES, volume_augment_streams(seed, step, rank)))
    _hip.call("mm_volume_augment_plan", x, plan, words, B, D, H, W, p_flip, p_shift, int(max_shift), p_scale, scale_range, p_noise,
              p_erase, int(erase[0]), int(erase[1]), int(erase[2]), s["flip_decision"], s["shift_decision"], s["shift_z"],
              s["shift_y"], s["shift_x"], s["scale_decision"], s["scale_u"], s["noise_decision"], s["erase_decision"],
              s["erase_z"], s["erase_y"], s["erase_x"])
    _hip.call("mm_volume_augment", x, plan, words, out, B, D, H, W, noise_factor, fill, s["gauss_a"], s["gauss_b"])
    return plan


def volume_augment_read_plan(plan: torch.Tensor, B: int, D: int, H: int, W: int) -> dict:
    """a plan both launches have written -> {"flags": {flip, shift, scale, noise, erase: bool (B,)}, "shift": int32 (B, 3)
    = (dz, dy, dx), "factor": fp32 (B,), "erase_box": int32 (B, 6) = (ez, ey, ex, ed, eh, ew; zeros when off), "std":
    fp32 (B,), "noise_scale": fp32 (B,)}"""
    hdr = plan[:B * _VOL_HDR].view(B, _VOL_HDR)
    return {"flags": {name: (hdr[:, 0] >> k) & 1 != 0 for k, name in enumerate(VOL_AUG_FLAGS)},
            "shift": hdr[:, 1:4].contiguous(), "factor": hdr[:, 4].contiguous().view(_F32),
            "erase_box": hdr[:, 5:11].contiguous(), "std": hdr[:, 12].contiguous().view(_F32),
            "noise_scale": hdr[:, 11].contiguous().view(_F32)}


def volume_augment(x: torch.Tensor, *, step: int, rank: int = 0, return_plan: bool = False, **kw):
    """VolumeTransforms on a device batch (B, 1, D, H, W): flip, shift, scale, noise and erase per sample (the keywords of
    `volume_augment_into`); the draws are a function of (seed, step, rank) alone.  -> the augmented fp32 batch (a new
    tensor); with ``return_plan`` also `volume_augment_read_plan`'s dict."""
    _need_gpu(x)
    x = x.contiguous().float()
    out = torch.empty_like(x)
    plan = volume_augment_into(x, out, step=step, rank=rank, **kw)
    return (out, volume_augment_read_plan(plan, x.shape[0], *x.shape[2:])) if return_plan else out


# ---- temporal EEG augmentation (csrc/augment.hip's mm_stage_inputs_taug), on purposes of its own of the same stream
EEG_TIME_AUG_PURPOSES = augment_stream.PURPOSES["eeg_time"]
EEG_TIME_AUG_FLAGS = ("shift", "scale", "invert", "mask")              # bit k of a time plan's flag word
_TIME_HDR = 8


def eeg_time_augment_streams(seed: int, step: int, rank: int = 0) -> tuple:
    """the seven 32-bit stream words of one temporal-augmentation step, in `EEG_TIME_AUG_PURPOSES` order: purposes 19..25"""
    return augment_stream.streams("eeg_time", seed, step, rank)


def eeg_time_augment_check(B: int, C: int, T: int, *, p_shift: float, max_shift: int, p_scale: float, scale_range: float,
                           p_invert: float, p_mask: float, mask_len: int, n_drop: Optional[int] = None,
                           who: str = "eeg_time_augment"):
    """what both the kernel and the CPU path refuse, before anything runs.  ``mask_len``: the masked window's samples;
    ``n_drop``: that of an `EEGTransforms` riding along (its shape limits then hold too), None without one"""
    if min(B, C, T) < 1:
        raise ValueError(f"{who}: expected a non-empty (B, C, T) batch (got {B} x {C} x {T})")
    if B * C >= 1 << 32:
        raise ValueError(f"{who}: B * C must stay below 2^32 (the kernel's row index)")
    for name, p in (("p_shift", p_shift), ("p_scale", p_scale), ("p_invert", p_invert), ("p_mask", p_mask)):
        if not 0.0 <= p <= 1.0:                                    # (a NaN fails too)
            raise ValueError(f"{who}: {name} must lie in [0, 1] (got {p!r})")
    if int(max_shift) != max_shift or not 0 <= max_shift < T:
        raise ValueError(f"{who}: max_shift must be an integer in [0, T) = [0, {T}) (got {max_shift!r})")
    if not 0.0 <= scale_range < 1.0:
        raise ValueError(f"{who}: scale_range must lie in [0, 1) (got {scale_range!r})")
    if int(mask_len) != mask_len or not 1 <= mask_len <= T:
        raise ValueError(f"{who}: the masked window must lie in [1, T] = [1, {T}] samples (got {mask_len!r})")
    if n_drop is not None:
        eeg_augment_check(B, C, T, n_drop, who)


def eeg_time_augment_read_plan(time_plan: torch.Tensor) -> dict:
    """a (B, 8) int32 time plan mm_stage_inputs_taug has written -> {"flags": {shift, scale, invert, mask: bool (B,)},
    "shift": int32 (B,), "gain": fp32 (B,), "mask_start": int32 (B,), "mask_len": int32 (B,) (0 when off)}"""
    hdr = time_plan.view(-1, _TIME_HDR)
    return {"flags": {name: (hdr[:, 0] >> k) & 1 != 0 for k, name in enumerate(EEG_TIME_AUG_FLAGS)},
            "shift": hdr[:, 1].contiguous(), "gain": hdr[:, 2].contiguous().view(_F32), "mask_start": hdr[:, 3].contiguous(),
            "mask_len": hdr[:, 4].contiguous()}


# ---- the ONE host call of both EEG augmenters: `eeg_augment*` and `eeg_time_augment*` below are its public spellings
def eeg_augmenters_into(x: torch.Tensor, xb: Optional[torch.Tensor], out: Optional[torch.Tensor], *, base_args: Optional[dict] = None,
                        time_args: Optional[dict] = None, step: int, rank: int = 0, fmri_dst: Optional[torch.Tensor] = None,
                        fmri_src: Optional[torch.Tensor] = None, plan: Optional[torch.Tensor] = None,
                        time_plan: Optional[torch.Tensor] = None):
    """batch ``x`` (B, C, T) fp32 through an `EEGTransforms` (``base_args`` = its `kernel_args(C)`), an `EEGTimeTransforms`
    (``time_args`` = its `kernel_args(T)`) or both, into the packed bf16 operand ``xb`` (B, T, cpad(C)) and / or the fp32
    ``out`` (B, C, T), with the fMRI copy of mm_stage_inputs when given.  The launches: base only - mm_eeg_augment_plan, then
    mm_stage_inputs_aug; time only - mm_stage_inputs_taug alone (its draws need no plan); both - the plan, then
    mm_stage_inputs_taug with the noise and the channel drop in the same launch.  With ``time_args`` ``out`` must not overlap
    ``x``: the shift is a gather.  ``plan``: a buffer of `eeg_augment_plan_layout` words to reuse (a training loop keeps one
    per batch shape); ``time_plan``: (B, 8) int32 for the per-sample time draws (`eeg_time_augment_read_plan`), or None.
    -> the EEG plan buffer (int32 words; None without ``base_args``)."""
    if base_args is None and time_args is None:
        raise ValueError("eeg_augmenters_into: neither base_args nor time_args")
    n_drop = None if base_args is None else base_args["n_drop"]
    if time_args is None:
        _need_gpu(x)
        B, C, T = x.shape
        eeg_augment_check(B, C, T, n_drop)
    else:
        B, C, T = x.shape
        t = {k: v for k, v in time_args.items() if k != "seed"}
        eeg_time_augment_check(B, C, T, n_drop=n_drop, **t)
        if x.dtype != _F32 or (out is not None and (out.dtype != _F32 or tuple(out.shape) != (B, C, T))):
            raise ValueError("eeg_time_augment_into: fp32 batches of one shape")
        if out is not None and _overlap(x, out):
            raise ValueError("eeg_time_augment_into: source and destination overlap (the shift is a gather: augment into another buffer)")
        _need_gpu(x)
    words, s, noise_factor = 0, (0, 0, 0, 0, 0), 0.0
    if base_args is None:
        plan = None
    else:
        words, _, _ = eeg_augment_plan_layout(B, C, T)
        if plan is None:
            plan = torch.empty(words, dtype=torch.int32, device=x.device)
        s = augment_streams(base_args["seed"], step, rank)
        noise_factor = base_args["noise_factor"]
        _hip.call("mm_eeg_augment_plan", x, plan, words, B, C, T, base_args["p_noise"], base_args["p_drop"], n_drop, s[0], s[1], s[2])
    stage = (x, plan, words, xb, out, B, C, T, cpad(C), noise_factor, s[3], s[4])
    fmri = (fmri_dst, fmri_src, 0 if fmri_src is None else fmri_src.numel())
    if time_args is None:
        _hip.call("mm_stage_inputs_aug", *stage, *fmri)
    else:
        _hip.call("mm_stage_inputs_taug", *stage, t["p_shift"], int(t["max_shift"]), t["p_scale"], t["scale_range"], t["p_invert"],
                  t["p_mask"], int(t["mask_len"]), *eeg_time_augment_streams(time_args["seed"], step, rank), time_plan, *fmri)
    return plan


def eeg_augmenters(x: torch.Tensor, *, base_args: Optional[dict] = None, time_args: Optional[dict] = None, step: int,
                   rank: int = 0, packed: bool = False, return_plan: bool = False):
    """`eeg_augmenters_into` on a device batch (B, C, T); the draws are a function of (seed, step, rank) alone.  -> the
    augmented fp32 batch (a new tensor); with ``packed`` also its channels-last bf16 image (B, T, cpad(C)), the first
    convolution's operand; with ``return_plan`` also what the launches drew: `eeg_augment_read_plan`'s tuple without
    ``time_args``, else `eeg_time_augment_read_plan`'s dict (plus "base": that tuple when ``base_args`` is given)."""
    _need_gpu(x)
    x = x.contiguous().float()
    B, C, T = x.shape
    out = _empty((B, C, T), _F32, x)
    xb = _empty((B, T, cpad(C)), _BF, x) if packed else None
    tp = torch.empty(B, _TIME_HDR, dtype=torch.int32, device=x.device) if return_plan and time_args is not None else None
    plan = eeg_augmenters_into(x, xb, out, base_args=base_args, time_args=time_args, step=step, rank=rank, time_plan=tp)
    res = (out, xb) if packed else out
    if not return_plan:
        return res
    base = None if plan is None else eeg_augment_read_plan(plan, B, C, T)
    if tp is None:
        return res, base
    info = eeg_time_augment_read_plan(tp)
    if base is not None:
        info["base"] = base
    return res, info


def eeg_augment_into(x: torch.Tensor, xb: Optional[torch.Tensor], out: Optional[torch.Tensor], *, p_noise: float, p_drop: float,
                     noise_factor: float, n_drop: int, seed: int, step: int, rank: int = 0,
                     fmri_dst: Optional[torch.Tensor] = None, fmri_src: Optional[torch.Tensor] = None,
                     plan: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`eeg_augmenters_into` with an `EEGTransforms` alone, its `kernel_args(C)` as keywords: the two launches"""
    return eeg_augmenters_into(x, xb, out, base_args=dict(p_noise=p_noise, p_drop=p_drop, noise_factor=noise_factor, n_drop=n_drop, seed=seed),
                               step=step, rank=rank, fmri_dst=fmri_dst, fmri_src=fmri_src, plan=plan)


def eeg_augment(x: torch.Tensor, *, p_noise: float, p_drop: float, noise_factor: float, n_drop: int, seed: int, step: int,
                rank: int = 0, packed: bool = False, return_plan: bool = False):
    """EEGTransforms on a device batch (B, C, T): per sample, with probability ``p_noise``, Gaussian noise of
    ``noise_factor`` x the sample's standard deviation, then with probability ``p_drop`` ``n_drop`` channels zeroed
    (`eeg_augmenters`; with ``return_plan`` also (noise_on, drop_mask, std))"""
    return eeg_augmenters(x, base_args=dict(p_noise=p_noise, p_drop=p_drop, noise_factor=noise_factor, n_drop=n_drop, seed=seed),
                          step=step, rank=rank, packed=packed, return_plan=return_plan)


# (the time spellings take the same keywords: `time_args`, optionally `base_args`)
eeg_time_augment_into, eeg_time_augment = eeg_augmenters_into, eeg_augmenters


def igemm(x: torch.Tensor, wf: torch.Tensor, taps: int, pad: int, cout: int, *,
          scale=None, shift=None, act="none", residual=None, pe=None, pool=1, stats=None,
          out_f32=False, out_bf16=True, out_pre=False, drop_p=0.0, seed=0, gradz=None, gradz_act="none"):
    """x (B, T, Cin) bf16 -> dict(out_f32, out_bf16, out_pre) of (B, T/pool, cout)."""
    B, T, cin = x.shape
    res = {}
    of = _empty((B, T // pool, cout), _F32, x) if out_f32 else None
    ob = _empty((B, T // pool, cout), _BF, x) if out_bf16 else None
    op = _empty((B, T, cout), _BF, x) if out_pre else None
    args = (x, wf, B, T, cin, cout, taps, pad, scale, shift, ACT[act], residual, pe,
            pool, stats, of, ob, op, float(drop_p), int(seed), EP(), gradz, ACT[gradz_act])
    nsplit, ws_floats = _splitk_plan(B, T, cin, cout, taps)
    if nsplit > 1:                # few output tiles, long reduction (config #5's merged conv): channel slices + an epilogue launch
        _hip.call("mm_conv1d_fwd_splitk", *args, _empty((ws_floats,), _F32, x), nsplit)
    else:
        _hip.call("mm_conv1d_fwd", *args)
    res["f32"], res["bf16"], res["pre"] = of, ob, op
    return res


_SPLITK_PLANS: Dict[tuple, tuple] = {}


def _splitk_plan(B: int, T: int, cin: int, cout: int, taps: int):
    """(slices, workspace floats) of mm_conv1d_fwd_splitk_plan, cached per shape"""
    if taps == 1:
        return 1, 0
    key = (B, T, cin, cout, taps)
    plan = _SPLITK_PLANS.get(key)
    if plan is None:
        import ctypes
        n, ws = ctypes.c_int(0), ctypes.c_int64(0)
        _hip.call("mm_conv1d_fwd_splitk_plan", B, T, cin, cout, taps, ctypes.addressof(n), ctypes.addressof(ws))
        plan = _SPLITK_PLANS[key] = (n.value, ws.value)
    return plan


def clip_loss_ws_floats(B: int, Bg: int, grouped: bool = False) -> int:
    """floats of the scratch of mm_clip_loss_own_rows (``grouped``: mm_clip_loss_own_rows_grouped) for B own rows of a
    Bg-row gathered batch; the kernel file owns the layout"""
    return _hip.host_int("mm_clip_loss_grouped_ws_floats" if grouped else "mm_clip_loss_ws_floats", B, Bg)


def clip_loss_grouped_ws_floats(B: int, Bg: int) -> int:
    """clip_loss_ws_floats(B, Bg, grouped=True) under its earlier name (tests/test_clip_groups_gpu.py and callers of the previous version use it)"""
    return clip_loss_ws_floats(B, Bg, grouped=True)


def clip_loss_masked_ws_floats(B: int, Bg: int) -> int:
    """floats of the scratch of mm_clip_loss_own_rows_masked for B own rows of a Bg-row gathered batch"""
    return _hip.host_int("mm_clip_loss_masked_ws_floats", B, Bg)


def _loss_radius(radius, gid_all, who: str) -> int:
    """``radius`` of the loss entry points as an int >= 0; a radius > 0 needs ids: ``ValueError`` otherwise"""
    radius = int(radius)
    if radius < 0:
        raise ValueError(f"{who}: radius must be >= 0 (got {radius})")
    if radius > 0 and gid_all is None:
        raise ValueError(f"{who}: radius={radius} needs group ids (groups=): the ids are the timeline positions")
    return radius


def clip_loss_own_rows(z_all, gid_all, logit_scale1, scal, dz, B: int, row0: int, radius: int = 0):
    """symmetric InfoNCE of rows [row0, row0 + B) of the gathered batch z_all (Bg, 2N) -> scal (4,), dz (B, 2N) or None;
    gid_all (Bg,) int32 group ids: the grouped loss, None: pair i is its own positive.  ``radius`` > 0: keys whose id is
    within ``radius`` of the query's (and not equal) are ignored (mm_clip_loss_own_rows_masked).  Allocates the workspace."""
    Bg, N2 = z_all.shape
    if _loss_radius(radius, gid_all, "clip_loss_own_rows"):
        ws = _empty((clip_loss_masked_ws_floats(B, Bg),), _F32, z_all)
        _hip.call("mm_clip_loss_own_rows_masked", z_all, gid_all, logit_scale1, scal, dz, ws, B, Bg, N2 // 2, row0, int(radius))
        return
    ws = _empty((clip_loss_ws_floats(B, Bg, gid_all is not None),), _F32, z_all)
    if gid_all is None:
        _hip.call("mm_clip_loss_own_rows", z_all, logit_scale1, scal, dz, ws, B, Bg, N2 // 2, row0)
    else:
        _hip.call("mm_clip_loss_own_rows_grouped", z_all, gid_all, logit_scale1, scal, dz, ws, B, Bg, N2 // 2, row0)


def sigmoid_loss_ws_floats(B: int, Bg: int) -> int:
    """floats of the scratch of mm_sigmoid_loss_own_rows for B own rows of a Bg-row gathered batch (plain and grouped alike)"""
    return _hip.host_int("mm_sigmoid_loss_ws_floats", B, Bg)


def sigmoid_loss_masked_ws_floats(B: int, Bg: int) -> int:
    """floats of the scratch of mm_sigmoid_loss_own_rows_masked for B own rows of a Bg-row gathered batch"""
    return _hip.host_int("mm_sigmoid_loss_masked_ws_floats", B, Bg)


def sigmoid_loss_own_rows(z_all, gid_all, logit_scale1, logit_bias1, scal, dz, B: int, row0: int, radius: int = 0):
    """pairwise sigmoid loss of rows [row0, row0 + B) of the gathered batch z_all (Bg, 2N) -> scal (5,), dz (B, 2N) or None;
    gid_all (Bg,) int32 group ids: pairs with equal ids are positives, None: pair i only.  ``radius`` > 0: pairs whose ids
    differ by at most ``radius`` are ignored (mm_sigmoid_loss_own_rows_masked).  Allocates the workspace."""
    Bg, N2 = z_all.shape
    if _loss_radius(radius, gid_all, "sigmoid_loss_own_rows"):
        ws = _empty((sigmoid_loss_masked_ws_floats(B, Bg),), _F32, z_all)
        _hip.call("mm_sigmoid_loss_own_rows_masked", z_all, gid_all, logit_scale1, logit_bias1, scal, dz, ws, B, Bg, N2 // 2,
                  row0, int(radius))
        return
    ws = _empty((sigmoid_loss_ws_floats(B, Bg),), _F32, z_all)
    _hip.call("mm_sigmoid_loss_own_rows", z_all, gid_all, logit_scale1, logit_bias1, scal, dz, ws, B, Bg, N2 // 2, row0)


def clip_bank_check(B: int, K: int, N: int, warmup: int = 0, who: str = "clip_bank"):
    """the shape rules of mm_clip_bank_loss / mm_clip_bank_push (csrc/clip_bank.hip), before any launch: ``ValueError``"""
    if K < 1:
        raise ValueError(f"{who}: the bank needs at least one row (K={K})")
    if N < 4 or N % 4:
        raise ValueError(f"{who}: the embedding width must be a positive multiple of 4 (N={N})")
    if warmup < 0:
        raise ValueError(f"{who}: warmup must be >= 0 (got {warmup})")
    if B < 1 or B > K:
        raise ValueError(f"{who}: a batch of {B} rows does not fit a bank of {K} (need 1 <= B <= K)")


class ClipBank:
    """the cross-batch memory of the InfoNCE loss (mm_clip_bank_loss / mm_clip_bank_push): device storage the caller owns,
    allocated before any capture.  ``bank`` (K, 2N) fp32 rows [ze | zf]; ``gid`` (K,) int32 ids of the rows (``grouped``
    banks only, else None); ``state`` (4,) int32 = {head, filled, pushes, 0} - zero it to empty the bank."""

    def __init__(self, K: int, N: int, grouped: bool = False, device="cuda"):
        clip_bank_check(1, K, N, 0, "ClipBank")
        self.K, self.N, self.grouped = int(K), int(N), bool(grouped)
        self.bank = torch.zeros(self.K, 2 * self.N, dtype=_F32, device=device)
        self.gid = torch.zeros(self.K, dtype=torch.int32, device=device) if grouped else None
        self.state = torch.zeros(4, dtype=torch.int32, device=device)

    def reset(self):
        self.state.zero_()

    def tensors(self):
        return [t for t in (self.bank, self.gid, self.state) if t is not None]


def clip_bank_ws_floats(B: int, K: int, N: int) -> int:
    """floats of the scratch of mm_clip_bank_loss (the 2 B (B + K) scores + the key chunks' partials)"""
    return _hip.host_int("mm_clip_bank_ws_floats", B, K, N)


def _bank_args(z, gid, bank: ClipBank, who: str):
    B, N2 = z.shape
    if N2 != 2 * bank.N:
        raise ValueError(f"{who}: rows of {N2} floats, the bank holds rows of {2 * bank.N}")
    if (gid is not None) != bank.grouped:
        raise ValueError(f"{who}: the bank {'carries' if bank.grouped else 'carries no'} group ids, the batch "
                         f"{'has none' if gid is None else 'has some'}")
    return B


def clip_bank_loss(z, gid, bank: ClipBank, logit_scale1, scal, dz, warmup: int = 0):
    """symmetric InfoNCE of the B rows of z (B, 2N) against themselves and the valid rows of ``bank`` -> scal (4,), dz
    (B, 2N) or None; gid (B,) int32 or None (the bank must have been built alike).  The number of valid bank rows is read
    on the device (``pushes >= warmup ? filled : 0``).  Allocates the workspace; the bank is not written."""
    B = _bank_args(z, gid, bank, "clip_bank_loss")
    clip_bank_check(B, bank.K, bank.N, warmup, "clip_bank_loss")
    ws = _empty((clip_bank_ws_floats(B, bank.K, bank.N),), _F32, z)
    _hip.call("mm_clip_bank_loss", z, gid, bank.bank, bank.gid, bank.state, logit_scale1, scal, dz, ws, B, bank.K, bank.N,
              int(warmup))


def clip_key_ws_floats(B: int, K: int, N: int) -> int:
    """floats of the scratch of mm_clip_key_loss (scores, the key chunks' partials, the folded normalisers and - with more
    than one key tile - the tiles' dq sums and their tickets)"""
    return _hip.host_int("mm_clip_key_ws_floats", B, K, N)


def clip_key_loss(q, k, gid, bank: ClipBank, logit_scale1, scal, dq, warmup: int = 0):
    """`clip_bank_loss` with the batch's keys taken from ``k`` (B, 2N), a momentum key encoder's rows of the same pairs:
    the online rows ``q`` (B, 2N) are queries only, ``k`` and the bank are constants -> scal (4,), dq (B, 2N) or None = the
    gradient w.r.t. ``q`` (there is no key term).  Allocates the workspace; neither ``k`` nor the bank is written
    (mm_clip_key_loss)."""
    B = _bank_args(q, gid, bank, "clip_key_loss")
    if tuple(k.shape) != tuple(q.shape):
        raise ValueError(f"clip_key_loss: {tuple(q.shape)} query rows but key rows of {tuple(k.shape)} (one key row per pair)")
    if q.dtype != _F32 or k.dtype != _F32:
        raise ValueError(f"clip_key_loss: q and k must be float32 (got {q.dtype}, {k.dtype})")
    clip_bank_check(B, bank.K, bank.N, warmup, "clip_key_loss")
    ws = _empty((clip_key_ws_floats(B, bank.K, bank.N),), _F32, q)
    _hip.call("mm_clip_key_loss", q, k, gid, bank.bank, bank.gid, bank.state, logit_scale1, scal, dq, ws, B, bank.K, bank.N,
              int(warmup))


def clip_bank_push(z, gid, bank: ClipBank):
    """the B rows of z (and their ids) into the ring, then the state words advance (mm_clip_bank_push)"""
    B = _bank_args(z, gid, bank, "clip_bank_push")
    clip_bank_check(B, bank.K, bank.N, 0, "clip_bank_push")
    _hip.call("mm_clip_bank_push", z, gid, bank.bank, bank.gid, bank.state, B, bank.K, bank.N)


def group_ids(groups, n: int, device=None, who: str = "groups") -> Optional[torch.Tensor]:
    """Validate a (n,) vector of group ids (e.g. subject indices; compared for equality only) -> int32 on ``device``, or
    None for None.  A host tensor of any integer dtype is range-checked and converted; a device tensor must already be
    int32 (checking its values would synchronise a replayed step).  Anything else raises ValueError before any launch."""
    if groups is None:
        return None
    if not isinstance(groups, torch.Tensor):
        raise ValueError(f"{who}: group ids must be a torch.Tensor (got {type(groups).__name__})")
    if groups.dim() != 1 or groups.shape[0] != n:
        raise ValueError(f"{who}: group ids must have shape ({n},) (got {tuple(groups.shape)})")
    if groups.dtype.is_floating_point or groups.dtype.is_complex or groups.dtype == torch.bool:
        raise ValueError(f"{who}: group ids must be an integer tensor (got {groups.dtype})")
    if groups.is_cuda:
        if groups.dtype != torch.int32:
            raise ValueError(f"{who}: group ids on the device must be int32 (got {groups.dtype}); host tensors of any integer "
                             "dtype are converted")
        if device is not None and groups.device != torch.device(device):
            raise ValueError(f"{who}: group ids are on {groups.device}, the batch on {device}")
        return groups.contiguous()
    if n and groups.dtype != torch.int32:
        g64 = groups.long()
        if bool((g64 < -2 ** 31).any()) or bool((g64 >= 2 ** 31).any()):
            raise ValueError(f"{who}: group ids must fit in int32")
    g32 = groups.to(torch.int32).contiguous()
    return g32 if device is None else g32.to(device)


def linear_rows(x2d: torch.Tensor, weight: torch.Tensor, bias, *, act="none", residual=None,
                out_f32=False, out_bf16=True, out_pre=False, drop_p=0.0, seed=0, need_dgrad=False):
    """(M, K) bf16 @ weight(N, K)^T + bias with a fused epilogue (taps == 1)."""
    M, K = x2d.shape
    wf, _, cinp, _ = weights.get(weight, need_dgrad)
    if cinp != K:
        raise _hip.HipLibraryError(f"linear: activation width {K} != padded weight width {cinp}")
    r = igemm(x2d.view(1, M, K), wf, 1, 0, weight.shape[0], shift=bias, act=act,
              residual=residual, out_f32=out_f32, out_bf16=out_bf16, out_pre=out_pre,
              drop_p=drop_p, seed=seed)
    return {k: (v.view(-1, v.shape[-1]) if v is not None else None) for k, v in r.items()}


def bn_fold_eval(bn, conv_bias) -> torch.Tensor:
    """[4][N] = scale, shift (conv bias folded), mean, rstd from running stats."""
    n = bn.num_features
    out4 = _empty((4, n), _F32, bn.weight)
    _hip.call("mm_bn_finalize", None, bn.weight, bn.bias, bn.running_mean, bn.running_var,
              conv_bias, out4, n, 1.0, 0.0, float(bn.eps), 1, None)
    return out4


def bn_finalize_train(bn, stats, count) -> torch.Tensor:
    n = bn.num_features
    out4 = _empty((4, n), _F32, bn.weight)
    mom = 0.1 if bn.momentum is None else float(bn.momentum)
    _hip.call("mm_bn_finalize", stats, bn.weight, bn.bias, bn.running_mean, bn.running_var,
              None, out4, n, float(count), mom, float(bn.eps), 0, bn.num_batches_tracked)
    return out4


def bn_fin_desc(bn, stats, count):
    """host-side mm_bn_fin_t for the `*_fin` apply passes (the train-mode finalize runs in their prologue) ->
    (ctypes buffer to pass as ``bn_fin_host``, out4 tensor the launch will write, objects to keep alive)"""
    import ctypes
    import struct
    n = bn.num_features
    out4 = _empty((4, n), _F32, bn.weight)
    mom = 0.1 if bn.momentum is None else float(bn.momentum)
    nb = bn.num_batches_tracked
    raw = struct.pack("<QQQQQQQfffi", stats.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                      bn.running_var.data_ptr(), out4.data_ptr(), nb.data_ptr() if nb is not None else 0,
                      float(count), mom, float(bn.eps), 0)
    buf = ctypes.create_string_buffer(raw, len(raw))
    return buf, out4


def layernorm(x2d: torch.Tensor, ln, want_stat: bool):
    M, D = x2d.shape
    out = _empty((M, D), _BF, x2d)
    stat = _empty((M, 2), _F32, x2d) if want_stat else None
    _hip.call("mm_layernorm_fwd", x2d, ln.weight, ln.bias, out, None, stat, M, D, float(ln.eps))
    return out, stat


def attn_effective_dropout(p: float) -> float:
    """the attention-probability dropout rate the kernels apply for a requested ``p``: csrc/attention.hip decides a 2 x 2 block
    of scores with one 32-bit hash and 8-bit fields, so the rate is quantised to round(256 p) / 256 (p = 0.1 -> 0.1016,
    the keep scale is that of the quantised rate: the mask stays unbiased); 0 < p < 1/512 rounds to NO dropout"""
    return round(256.0 * float(p)) / 256.0


def attention(qkv: torch.Tensor, nhead: int, want_lse: bool, drop_p: float = 0.0, seed: int = 0, mask=None):
    if 0.0 < float(drop_p) < 1.0 / 512.0:
        import warnings
        warnings.warn(f"attention dropout p = {drop_p} is below the kernels' resolution (1/256): no attention-probability dropout "
                      "is applied (nn.MultiheadAttention(dropout=p) would drop with probability p)")
    B, L, E3 = qkv.shape
    E = E3 // 3
    entry = attn_entry(E, nhead, "fwd")
    dh = E // nhead
    out = _empty((B, L, E), _BF, qkv)
    lse = _empty((B, nhead, L), _F32, qkv) if want_lse else None
    _hip.call(entry, qkv, out, lse, B, L, nhead, dh, 1.0 / math.sqrt(dh), float(drop_p), int(seed), EP(), mask,
              attn_mask_per_head(mask, B, nhead, L))
    return out, lse


ATTN_HEAD_DIMS = tuple(range(16, 65, 8))        # the head widths the self-attention kernels run (16, 24, ..., 64)


def attn_entry(d_model: int, nhead: int, which: str) -> str:
    """the C-ABI entry point of the self-attention ``which`` pass ("fwd" / "bwd") for a ``d_model``-wide, ``nhead``-head
    layer: head_dim 32 (the default model) runs the kernels of csrc/attention.hip compiled for exactly that width
    (mm_attn_fwd / mm_attn_bwd), every other supported head_dim runs the same kernels with a runtime head_dim
    (mm_attn_fwd_hd / mm_attn_bwd_hd).  Anything else raises ValueError before a launch."""
    dh = d_model // nhead if nhead > 0 else 0
    if nhead <= 0 or d_model % nhead or dh not in ATTN_HEAD_DIMS:
        raise ValueError(f"self-attention: (d_model, nhead) = ({d_model}, {nhead}) gives a head dim the kernels do not run; "
                         f"supported head dims: {', '.join(map(str, ATTN_HEAD_DIMS))}")
    return f"mm_attn_{which}" if dh == 32 else f"mm_attn_{which}_hd"


def attn_mask_per_head(mask, B: int, nhead: int, L: int) -> int:
    """0: ``mask`` is None or the shared (L, L) matrix; 1: the (B * nhead, L, L) form - its leading size is checked
    here, where the batch is known"""
    if mask is None or mask.dim() == 2:
        return 0
    if tuple(mask.shape) != (B * nhead, L, L):
        raise ValueError(f"attn_mask: the 3-D form must be (batch * heads, L, L) = ({B * nhead}, {L}, {L}), got {tuple(mask.shape)}")
    return 1


def additive_attn_mask(mask, L: int, like: torch.Tensor):
    """nn.MultiheadAttention's ``attn_mask`` (enhanced_models_v4.py:98) as the additive fp32 matrix the kernels take -
    (L, L) shared by all heads (the only form the reference passes) or (batch * heads, L, L): a boolean mask marks
    NOT-allowed positions with True (-> -inf)."""
    if mask is None:
        return None
    if mask.dim() not in (2, 3) or tuple(mask.shape[-2:]) != (L, L):
        raise ValueError(f"attn_mask: expected (L, L) or (batch * heads, L, L) with L = {L}, got {tuple(mask.shape)}")
    if mask.dtype == torch.bool:
        m = torch.zeros(tuple(mask.shape), dtype=_F32, device=like.device)
        m.masked_fill_(mask.to(like.device), float("-inf"))
        return m
    return mask.to(device=like.device, dtype=_F32).contiguous()


# ------------------------------------------------------- attention read-out
def _attn_readout_args(qkv: torch.Tensor, lse: torch.Tensor, nhead: int, mask, who: str):
    """what ``attention_weights`` / ``attention_received`` check alike, before a launch: the packed bf16 (B, L, 3E)
    projections, the fp32 (B, nhead, L) log-sum-exp, the head-dim rule of ``attn_entry`` and the two mask forms"""
    if qkv.dim() != 3 or qkv.dtype != _BF or qkv.shape[2] % 3 or min(qkv.shape) < 1:
        raise ValueError(f"{who}: qkv must be a non-empty bf16 (B, L, 3 E) tensor, got {qkv.dtype} {tuple(qkv.shape)}")
    B, L, E3 = qkv.shape
    attn_entry(E3 // 3, nhead, "fwd")
    if lse.dtype != _F32 or tuple(lse.shape) != (B, nhead, L):
        raise ValueError(f"{who}: lse must be fp32 (B, heads, L) = ({B}, {nhead}, {L}), got {lse.dtype} {tuple(lse.shape)}")
    mask = additive_attn_mask(mask, L, qkv)
    per = attn_mask_per_head(mask, B, nhead, L)
    return B, L, E3 // 3 // nhead, mask, per


def attention_weights(qkv: torch.Tensor, lse: torch.Tensor, nhead: int, mask=None, per_head: bool = False) -> torch.Tensor:
    """the eval-mode attention probabilities of a forward that kept ``qkv`` and ``lse`` (``transformer_block_fwd``'s
    ``saved['qkv']`` / ``saved['lse']``): fp32 (B, L, L), the mean over the heads - what nn.MultiheadAttention returns
    with ``need_weights=True`` - or (B, nhead, L, L) with ``per_head``.  One launch of mm_attn_weights."""
    B, L, dh, mask, per = _attn_readout_args(qkv, lse, nhead, mask, "attention_weights")
    _need_gpu(qkv, lse)
    w = _empty((B, nhead, L, L) if per_head else (B, L, L), _F32, qkv)
    _hip.call("mm_attn_weights", qkv.contiguous(), lse.contiguous(), w, B, L, nhead, dh, 1.0 / math.sqrt(dh), mask, per,
              1 if per_head else 0)
    return w


def attention_received(qkv: torch.Tensor, lse: torch.Tensor, nhead: int, row_w: Optional[torch.Tensor] = None,
                       self_weight: float = 0.0, mask=None) -> torch.Tensor:
    """fp32 (B, L): ``self_weight * r + (1 - self_weight) * r @ A`` with A the head-averaged attention matrix of
    ``attention_weights`` - never stored - and r = ``row_w`` (B, L), or 1 / L everywhere.  The defaults give the attention
    every time step receives; ``self_weight = 0.5`` is one step of attention rollout (mm_attn_received)."""
    B, L, dh, mask, per = _attn_readout_args(qkv, lse, nhead, mask, "attention_received")
    if not 0.0 <= float(self_weight) <= 1.0:
        raise ValueError(f"attention_received: self_weight must lie in [0, 1], got {self_weight}")
    if row_w is not None:
        if tuple(row_w.shape) != (B, L):
            raise ValueError(f"attention_received: row_w must be (B, L) = ({B}, {L}), got {tuple(row_w.shape)}")
        row_w = row_w.to(_F32).contiguous()
    _need_gpu(qkv, lse, row_w)
    out = _empty((B, L), _F32, qkv)
    ws = _empty((max(_hip.host_int("mm_attn_received_ws_floats", B, L, nhead), 1),), _F32, qkv)
    _hip.call("mm_attn_received", qkv.contiguous(), lse.contiguous(), row_w, float(self_weight), out, ws, B, L, nhead, dh,
              1.0 / math.sqrt(dh), mask, per)
    return out


ATTN_READOUT_METHODS = ("received", "rollout", "maps")


def _attention_encoder(encoder):
    """(kind, the module that owns ``transformer_layers``) of an encoder ``encoder_attention`` serves"""
    from .crossmodal_v4_enhancements import MultiScaleSTFTPowerEncoder
    from .enhanced_models_v4 import EnhancedERPEncoder, EnhancedPowerEncoder
    if isinstance(encoder, EnhancedERPEncoder):
        return "erp", encoder
    if isinstance(encoder, EnhancedPowerEncoder):
        return "power", encoder
    if isinstance(encoder, MultiScaleSTFTPowerEncoder):
        return "stft", encoder.encoder
    raise ValueError(f"encoder_attention: {type(encoder).__name__} is not an EEG transformer encoder (EnhancedERPEncoder, "
                     "EnhancedPowerEncoder, MultiScaleSTFTPowerEncoder): it has no temporal attention to read out")


def encoder_tokens(encoder, T: int) -> int:
    """tokens the transformer stack of ``encoder`` sees for a ``T``-sample input: the ERP encoder pools by 2, the power
    encoder keeps every step, the STFT front end makes T // hop + 1 frames"""
    kind, _ = _attention_encoder(encoder)
    return T // 2 if kind == "erp" else T if kind == "power" else T // encoder.hop + 1


def spread_pooled_tokens(tokens: torch.Tensor, T: int) -> torch.Tensor:
    """(B, L) token weights of the ERP encoder -> (B, T) sample weights: token i came out of MaxPool1d(2) over samples
    2i, 2i + 1 (the convolutions keep the length), which share its weight equally; an odd last sample fed no token and
    gets 0.  The sum over time is the sum over tokens."""
    B, L = tokens.shape
    if L != T // 2:
        raise ValueError(f"spread_pooled_tokens: {L} tokens do not come from {T} samples (expected {T // 2})")
    time = tokens.new_zeros((B, T))
    time[:, :2 * L] = (0.5 * tokens).repeat_interleave(2, dim=1)
    return time


def encoder_attention(encoder, x: torch.Tensor, method: str, layer: Optional[int] = None, mask=None):
    """What the transformer stack of an EEG encoder attends to over time.  ONE eval-mode forward (frozen BatchNorm, no
    dropout, no seed drawn: the module's own train / eval flags are not consulted and not touched) keeps every block's
    ``qkv`` and ``lse``; the read-out kernels do the rest.
      "maps":     the list of per-layer head-averaged (B, L, L) matrices;
      "received": (B, L), the mean over the queries of layer ``layer``'s matrix (default: the last layer);
      "rollout":  (B, L), attention rollout (Abnar & Zuidema 2020) to the mean-pooled feature: r_N = 1 / L,
                  r_{l-1} = r_l (0.5 A_l + 0.5 I) - a chain of N vector steps, no L x L product is formed."""
    if method not in ATTN_READOUT_METHODS:
        raise ValueError(f"encoder_attention: unknown method {method!r} (one of {', '.join(ATTN_READOUT_METHODS)})")
    kind, inner = _attention_encoder(encoder)
    n = len(inner.transformer_layers)
    if n == 0:
        raise ValueError(f"encoder_attention: this {type(encoder).__name__} has no transformer layers")
    if layer is not None and method != "received":
        raise ValueError(f"encoder_attention: layer applies to method 'received' only, not to {method!r}")
    li = n - 1 if layer is None else int(layer)
    if not 0 <= li < n:
        raise ValueError(f"encoder_attention: layer {layer} out of range for {n} transformer layers")
    if x.dim() != 3:
        raise ValueError(f"encoder_attention: expected (batch, channels, time), got {tuple(x.shape)}")
    _need_gpu(x)
    nhead = inner.transformer_layers[0].nhead
    with torch.no_grad():
        mask = additive_attn_mask(mask, encoder_tokens(encoder, x.shape[2]), x)
        if kind == "erp":
            saved = _erp_forward_impl(inner, x.float(), False, True, save=True, mask=mask)[1]
        else:
            xb = pack_nct(x.float()) if kind == "power" else stft_front_end(x, encoder.n_ffts, encoder.hop, encoder.normalize)
            saved = _power_forward_impl(inner, xb, False, True, save=True, mask=mask)[1]
        recs = [(s["qkv"].view(s["B"], s["L"], -1), s["lse"]) for s in saved["blocks"]]
        if method == "maps":
            return [attention_weights(q, l, nhead, mask) for q, l in recs]
        if method == "received":
            return attention_received(*recs[li], nhead, mask=mask)
        r = None
        for q, l in reversed(recs):
            r = attention_received(q, l, nhead, row_w=r, self_weight=0.5, mask=mask)
        return r


def encoder_temporal_attention(encoder, x: torch.Tensor, method: str = "rollout", layer: Optional[int] = None) -> dict:
    """``encoder_attention`` as the encoders' ``temporal_attention`` returns it: {"tokens": (B, L)} plus "time": (B, T)
    where the token-to-sample map is fixed - the ERP encoder's pooled pairs, the power encoder's identity; STFT frames
    overlap, so there is none."""
    if method == "maps":
        raise ValueError("temporal_attention: method 'maps' has no per-step form; call attention_maps")
    tokens = encoder_attention(encoder, x, method, layer)
    out = {"tokens": tokens}
    kind, _ = _attention_encoder(encoder)
    if kind == "erp":
        out["time"] = spread_pooled_tokens(tokens, x.shape[2])
    elif kind == "power":
        out["time"] = tokens
    return out


def block_attention_weights(blk, x: torch.Tensor, mask=None, average_attn_weights: bool = True) -> torch.Tensor:
    """TemporalTransformerBlock.attention_weights: norm1, in-projection, attention forward with lse, mm_attn_weights"""
    if x.dim() != 3:
        raise ValueError(f"attention_weights: expected (batch, seq, d_model), got {tuple(x.shape)}")
    _need_gpu(x)
    B, L, D = x.shape
    with torch.no_grad():
        mask = additive_attn_mask(mask, L, x)
        h1, _ = layernorm(x.float().contiguous().view(B * L, D), blk.norm1, False)
        qkv = linear_rows(h1, blk.self_attn.in_proj_weight, blk.self_attn.in_proj_bias)["bf16"].view(B, L, 3 * D)
        _, lse = attention(qkv, blk.nhead, True, mask=mask)
        return attention_weights(qkv, lse, blk.nhead, mask, per_head=not average_attn_weights)


# ------------------------------------------------------------------- stages
def conv_bn_act(xb: torch.Tensor, conv, bn, *, act="gelu", pool=1, training=False, drop_p=0.0,
                drop_first=True, pe=None, pe_drop_p=0.0, want_f32=False, want_bf16=True, need_dgrad=False,
                save=None, next_norm=None):
    """Conv1d -> BatchNorm1d -> act [-> MaxPool(2)] [-> Dropout] on (B, T, Cp) bf16.

    eval : one kernel (BN folded into the GEMM epilogue).
    train: GEMM (+bias, per-channel sum/sumsq) -> finalize -> BN/act/pool apply.
    eval with ``save`` (a backward will follow: frozen BatchNorm, saliency maps): the
    train-shaped pipeline with the RUNNING statistics and no statistic update.
    ``next_norm`` (a LayerNorm(128) that consumes the fp32 output row-wise - the transformer stack's first norm1):
    computed by the same launch when the block is 128 wide and un-pooled; the result comes back as ``out["prenorm"]``
    = (bf16 rows, mean / rstd or None).
    Returns (out dict, saved-for-backward dict or None)."""
    save = training if save is None else save
    k = conv.kernel_size[0]
    pad = conv.padding[0]
    cout = conv.out_channels
    wf, _, cinp, _ = weights.get(conv.weight, need_dgrad)
    assert xb.shape[2] == cinp, (xb.shape, cinp)
    B, T, _ = xb.shape
    if not save:
        out4 = bn_fold_eval(bn, conv.bias)
        r = igemm(xb, wf, k, pad, cout, scale=out4[0], shift=out4[1], act=act, pe=pe, pool=pool,
                  out_f32=want_f32, out_bf16=want_bf16)
        return r, None
    stats = _zeros((REPL, 2, cout), xb) if training else None
    y = igemm(xb, wf, k, pad, cout, shift=conv.bias, stats=stats, out_f32=True, out_bf16=False)["f32"]
    # train mode, GELU, <= 256 channels: the finalize (mean / rstd / running statistics) runs in the apply pass's prologue
    fold = training and act == "gelu" and cout <= 256 and isinstance(bn.running_mean, torch.Tensor)
    fin = None
    if fold:
        fin, out4 = bn_fin_desc(bn, stats, B * T)
    else:
        out4 = bn_finalize_train(bn, stats, B * T) if training else bn_fold_eval(bn, None)
    if not training:
        drop_p = pe_drop_p = 0.0
    seed = _next_seed() if drop_p > 0 else 0
    seed2 = _next_seed() if pe_drop_p > 0 else 0
    of = _empty((B, T // pool, cout), _F32, xb) if want_f32 else None
    ob = _empty((B, T // pool, cout), _BF, xb) if want_bf16 else None
    prenorm = None
    if next_norm is not None and cout == 128 and pool == 1 and want_f32 and not want_bf16 and drop_first \
            and tuple(next_norm.normalized_shape) == (128,):
        hn = _empty((B * T, cout), _BF, xb)
        stn = _empty((B * T, 2), _F32, xb)
        if fold:
            import ctypes
            _hip.call("mm_bn_act_fwd_ln_fin", y, ctypes.addressof(fin), pe, of, B, T, ACT[act], float(drop_p), seed,
                      float(pe_drop_p), seed2, EP(), next_norm.weight, next_norm.bias, float(next_norm.eps), hn, stn)
        else:
            _hip.call("mm_bn_act_fwd_ln", y, out4[0], out4[1], pe, of, B, T, ACT[act], float(drop_p), seed,
                      float(pe_drop_p), seed2, EP(), next_norm.weight, next_norm.bias, float(next_norm.eps), hn, stn)
        prenorm = (hn, stn)
    elif fold:
        import ctypes
        _hip.call("mm_bn_act_fwd_fin", y, ctypes.addressof(fin), pe, ob, of, B, T, cout, ACT[act], pool,
                  1 if drop_first else 0, float(drop_p), seed, float(pe_drop_p), seed2, EP())
    else:
        _hip.call("mm_bn_act_fwd", y, out4[0], out4[1], pe, ob, of, B, T, cout, ACT[act], pool,
                  1 if drop_first else 0, float(drop_p), seed, float(pe_drop_p), seed2, EP())
    saved = dict(xb=xb, y=y, out4=out4, act=act, pool=pool, drop_p=drop_p, seed=seed,
                 drop2=(float(pe_drop_p), seed2), drop_first=drop_first, conv=conv, bn=bn, train=training)
    return {"f32": of, "bf16": ob, "pre": None, "prenorm": prenorm}, saved


class BlockPlan(NamedTuple):
    """which launches one transformer block runs, decided from shapes, consumers and the A/B knobs alone (``block_plan``).
    ``transformer_block_fwd`` dispatches on it and saves it; the backward reads it (``autograd.block_bwd_plan``)."""
    ln_fused: bool          # width 128, rows in groups of 32: the LayerNorms ride in the epilogue of the GEMM above them
    front: str              # out-projection .. first FFN Linear: "rows" (mm_ffn_rows_fwd: the tail and its consumers too) |
    #                         "ln_gemm2_act" (mm_linear_fwd_ln_gemm2_act) | "ln" (mm_linear_fwd_ln + a GEMM) | "generic" (3 launches)
    tail: str               # second FFN Linear: "rows" (ran in the front's launch) | "meanpool" (mm_linear_fwd_meanpool) |
    #                         "ln_gemm2" (mm_linear_fwd_ln_gemm2) | "ln" (mm_linear_fwd_ln) | "generic"
    qkv_fused: bool         # the next block's QKV projection runs on its norm1 rows in this block's last launch
    out_proj_128: bool      # the out-projection's images are 128 x 128 (the backward can run its data gradient as a second GEMM)
    ffn_rows_width: bool    # the FFN width is a multiple of 128 up to 512 (the hidden tile fits the workgroup's LDS)


def block_plan(D: int, M: int, n1: int, *, pool_out: bool = False, next_norm: bool = False, next_nq: int = 0) -> BlockPlan:
    """the plan of a ``D``-wide block with FFN width ``n1`` on ``M`` = B * L rows.  ``pool_out`` / ``next_norm``: which consumer
    the finished rows have; ``next_nq``: the width of the next block's packed QKV projection (0 = no next block).  Pure: the
    weight images' padded widths are ``cpad`` of the Linear shapes, nothing is built or recorded; the knobs are read here.
    The QKV projection rides along only with ``M * next_nq < 2**32``, from either launch: the rule in front of
    mm_linear_fwd_ln_gemm2 once lacked that guard, but the kernel was never safe beyond it (no test reaches that size)."""
    ln_fused = D == 128 and M % 32 == 0
    k128 = cpad(D) == 128       # the images that take D-wide rows (out-projection, first FFN Linear, QKV projection) are 128 wide
    ffn1 = ln_fused and k128 and n1 % 128 == 0 and M * n1 < (1 << 32) and not _NO_FFN1_FUSE
    rows = ffn1 and n1 <= 512 and cpad(n1) == n1 and not _NO_FFN_ROWS and (pool_out or next_norm)
    qkv = bool(ln_fused and k128 and next_norm and not pool_out and next_nq > 0 and next_nq % 128 == 0
               and M * next_nq < (1 << 32) and not _NO_QKV_FUSE)
    front = "rows" if rows else "ln_gemm2_act" if ffn1 else "ln" if ln_fused else "generic"
    if rows or pool_out:
        tail = "rows" if rows else "meanpool"
    else:
        tail = ("ln_gemm2" if qkv else "ln") if next_norm and ln_fused else "generic"
    return BlockPlan(ln_fused, front, tail, qkv, k128, n1 % 128 == 0 and n1 <= 512)


def _ln_front_begin(blk, x2, save, need_dgrad):
    """the three LayerNorm-fused fronts: out-projection and first FFN Linear images, buffers of x1, norm2(x1) and its statistics"""
    M, D = x2.shape
    wf, _, cinp, _ = weights.get(blk.self_attn.out_proj.weight, need_dgrad)
    x1 = _empty((M, D), _F32, x2)
    h2 = _empty((M, D), _BF, x2)
    st2 = _empty((M, 2), _F32, x2) if save else None
    w1 = weights.get(blk.linear1.weight, need_dgrad)[0]
    return wf, cinp, w1, x1, h2, st2


def _next_rows(x2, save, next_blk, qkv_fused, need_dgrad):
    """the next block's norm1 rows and statistics, with ``qkv_fused`` its QKV image, bias, width and q | k | v buffer too"""
    M, D = x2.shape
    hn = _empty((M, D), _BF, x2)
    stn = _empty((M, 2), _F32, x2) if save else None
    if not qkv_fused:
        return hn, stn, None, None, 0, None
    at = next_blk.self_attn
    wq, _, cq, _ = weights.get(at.in_proj_weight, need_dgrad)
    if cq != D:
        raise _hip.HipLibraryError(f"transformer block: the next block's QKV image is {cq} wide, the rows {D}")
    nq = at.in_proj_weight.shape[0]
    return hn, stn, wq, at.in_proj_bias, nq, _empty((M, nq), _BF, x2)


def _ffn1_rows(blk, h2, p, s2, save, need_dgrad):
    """the first FFN Linear as its own GEMM -> (hidden bf16, pre-activation or None)"""
    f1 = linear_rows(h2, blk.linear1.weight, blk.linear1.bias, act=blk._act, out_pre=save, drop_p=p, seed=s2, need_dgrad=need_dgrad)
    return f1["bf16"], f1["pre"]


def _block_rows(blk, o, x2, p, seeds, save, need_dgrad, plan, L, pool_out, next_norm, next_blk):
    """front "rows": everything after attention is ONE launch - out-projection, norm2, both FFN Linears on the hidden tile the
    workgroup still holds, and the consumers of the finished rows (the mean over time, or the next block's norm1 and QKV
    projection); without a backward the hidden tensor is never written -> (x1, h2, st2, g, z, x2o, next_prenorm)"""
    M, D = x2.shape
    s1, s2, s3 = seeds
    n1 = blk.linear1.weight.shape[0]
    wf, cinp, w1, x1, h2, st2 = _ln_front_begin(blk, x2, save, need_dgrad)
    z1 = _empty((M, n1), _BF, x2) if save else None
    w2 = weights.get(blk.linear2.weight, need_dgrad)[0]
    g1 = _empty((M, n1), _BF, x2) if save else None
    x2o = _empty((M, D), _F32, x2)
    hn = stn = wq = bq = qn = nxt = None
    nq = 0
    if pool_out is None:
        hn, stn, wq, bq, nq, qn = _next_rows(x2, save, next_blk, plan.qkv_fused, need_dgrad)
        nxt = (hn, stn, qn) if qn is not None else (hn, stn)
    _hip.call("mm_ffn_rows_fwd", o, wf, M, cinp, blk.self_attn.out_proj.bias, x2, x1, float(p), int(s1),
              EP(), blk.norm2.weight, blk.norm2.bias, float(blk.norm2.eps), h2, st2, w1, blk.linear1.bias, n1, g1, z1,
              ACT[blk._act], float(p), int(s2), w2, blk.linear2.bias, x2o, float(p), int(s3),
              None if hn is None else next_norm.weight, None if hn is None else next_norm.bias,
              float(next_norm.eps) if hn is not None else 0.0, hn, stn, wq, bq, nq, qn, pool_out,
              L if pool_out is not None else 0)
    return x1, h2, st2, g1, z1, x2o, nxt


def _front_ln_gemm2_act(blk, o, x2, p, s1, s2, save, need_dgrad):
    """front "ln_gemm2_act": the first FFN Linear (GELU, Dropout, pre-activation copy) runs on norm2's rows inside the
    out-projection's launch -> (x1, h2, st2, g, z)"""
    M = x2.shape[0]
    n1 = blk.linear1.weight.shape[0]
    wf, cinp, w1, x1, h2, st2 = _ln_front_begin(blk, x2, save, need_dgrad)
    z1 = _empty((M, n1), _BF, x2) if save else None
    weights.get(blk.linear2.weight, need_dgrad)             # (requested with the other two: a cold cache builds all three here)
    g1 = _empty((M, n1), _BF, x2)
    _hip.call("mm_linear_fwd_ln_gemm2_act", o, wf, M, cinp, blk.self_attn.out_proj.bias, x2, x1, float(p),
              int(s1), EP(), blk.norm2.weight, blk.norm2.bias, float(blk.norm2.eps), h2, st2, w1, blk.linear1.bias,
              n1, g1, z1, ACT[blk._act], float(p), int(s2))
    return x1, h2, st2, g1, z1


def _front_ln(blk, o, x2, p, s1, s2, save, need_dgrad):
    """front "ln": norm2 in the out-projection's epilogue, the first FFN Linear as its own GEMM -> (x1, h2, st2, g, z)"""
    wf, cinp, _, x1, h2, st2 = _ln_front_begin(blk, x2, save, need_dgrad)
    _hip.call("mm_linear_fwd_ln", o, wf, x2.shape[0], cinp, blk.self_attn.out_proj.bias, x2, x1, float(p), int(s1),
              EP(), blk.norm2.weight, blk.norm2.bias, float(blk.norm2.eps), h2, st2)
    return (x1, h2, st2) + _ffn1_rows(blk, h2, p, s2, save, need_dgrad)


def _front_generic(blk, o, x2, p, s1, s2, save, need_dgrad):
    """front "generic": out-projection, norm2 and the first FFN Linear as three launches -> (x1, h2, st2, g, z)"""
    at = blk.self_attn
    x1 = linear_rows(o, at.out_proj.weight, at.out_proj.bias, residual=x2, out_f32=True, out_bf16=False, drop_p=p, seed=s1,
                     need_dgrad=need_dgrad)["f32"]
    h2, st2 = layernorm(x1, blk.norm2, save)
    return (x1, h2, st2) + _ffn1_rows(blk, h2, p, s2, save, need_dgrad)


_BLOCK_FRONTS = {"ln_gemm2_act": _front_ln_gemm2_act, "ln": _front_ln, "generic": _front_generic}


def _tail_meanpool(blk, g, x1, p, s3, need_dgrad, L, pool_out):
    """tail "meanpool": the second FFN Linear also accumulates the mean over time of its output rows -> x2o"""
    M, D = x1.shape
    wf, _, cinp, _ = weights.get(blk.linear2.weight, need_dgrad)
    x2o = _empty((M, D), _F32, x1)
    _hip.call("mm_linear_fwd_meanpool", g, wf, M, cinp, blk.linear2.bias, x1, x2o, float(p), int(s3), EP(), pool_out, L)
    return x2o


def _tail_ln(blk, g, x1, p, s3, need_dgrad, save, next_norm, next_blk, qkv_fused):
    """tails "ln" / "ln_gemm2": the next block's norm1 in the second FFN Linear's epilogue, with ``qkv_fused`` followed by that
    block's QKV projection as a second GEMM of the launch -> (x2o, next_prenorm)"""
    M, D = x1.shape
    wf, _, cinp, _ = weights.get(blk.linear2.weight, need_dgrad)
    x2o = _empty((M, D), _F32, x1)
    hn, stn, wq, bq, nq, qn = _next_rows(x1, save, next_blk, qkv_fused, need_dgrad)
    args = (g, wf, M, cinp, blk.linear2.bias, x1, x2o, float(p), int(s3), EP(), next_norm.weight, next_norm.bias,
            float(next_norm.eps), hn, stn)
    if qkv_fused:
        _hip.call("mm_linear_fwd_ln_gemm2", *args, wq, bq, nq, qn)
        return x2o, (hn, stn, qn)
    _hip.call("mm_linear_fwd_ln", *args)
    return x2o, (hn, stn)


def transformer_block_fwd(x: torch.Tensor, blk, training: bool, need_dgrad: bool = False,
                          save: Optional[bool] = None, pool_out: Optional[torch.Tensor] = None,
                          prenorm=None, next_norm=None, mask=None, next_blk=None):
    """x fp32 (B, L, d) -> fp32 (B, L, d); returns (out, saved).  ``training``
    switches dropout on; ``save`` (default = training) keeps what backward needs.
    ``pool_out`` (zeroed fp32 (B, d)): the second FFN Linear also accumulates the mean over time of
    the block's output there (the encoder's pooling step, fused into that GEMM's epilogue).
    Width 128: every LayerNorm but the stack's first is computed in the epilogue of the GEMM that produces
    its input (``prenorm`` = (norm1(x) bf16, stats) handed in by the block below, ``next_norm`` = the next
    block's norm1, whose output is then returned in ``saved['next_prenorm']`` / as third result).  With ``next_blk`` the
    same launch also runs that block's QKV projection on those rows (a second GEMM: the third result then carries the
    packed q | k | v as its third element).  Which launches run is decided once, by ``block_plan``; the plan is kept in
    ``saved['plan']``.  norm1 / QKV projection and attention first, then the plan's front and tail."""
    B, L, D = x.shape
    M = B * L
    save = training if save is None else save
    p = blk.dropout.p if training else 0.0
    pa = float(blk.self_attn.dropout) if training else 0.0      # attention-probability dropout
    plan = block_plan(D, M, blk.linear1.weight.shape[0], pool_out=pool_out is not None, next_norm=next_norm is not None,
                      next_nq=next_blk.self_attn.in_proj_weight.shape[0] if next_blk is not None else 0)
    sa = _next_seed() if pa > 0 else 0
    s1, s2, s3 = (_next_seed(), _next_seed(), _next_seed()) if p > 0 else (0, 0, 0)
    x2 = x.view(M, D)
    h1, st1 = prenorm[:2] if prenorm is not None else layernorm(x2, blk.norm1, save)
    if prenorm is not None and len(prenorm) > 2:            # the block below already projected its fused LayerNorm rows
        qkv = prenorm[2]
    else:
        qkv = linear_rows(h1, blk.self_attn.in_proj_weight, blk.self_attn.in_proj_bias,
                          need_dgrad=need_dgrad)["bf16"]
    o, lse = attention(qkv.view(B, L, 3 * D), blk.nhead, save, pa, sa, mask)
    o2 = o.view(M, D)
    nxt = None
    if plan.front == "rows":
        x1, h2, st2, g, z, x2o, nxt = _block_rows(blk, o2, x2, p, (s1, s2, s3), save, need_dgrad, plan, L, pool_out,
                                                  next_norm, next_blk)
    else:
        x1, h2, st2, g, z = _BLOCK_FRONTS[plan.front](blk, o2, x2, p, s1, s2, save, need_dgrad)
        if plan.tail == "meanpool":
            x2o = _tail_meanpool(blk, g, x1, p, s3, need_dgrad, L, pool_out)
        elif plan.tail in ("ln", "ln_gemm2"):
            x2o, nxt = _tail_ln(blk, g, x1, p, s3, need_dgrad, save, next_norm, next_blk, plan.qkv_fused)
        else:
            x2o = linear_rows(g, blk.linear2.weight, blk.linear2.bias, residual=x1, out_f32=True,
                              out_bf16=False, drop_p=p, seed=s3, need_dgrad=need_dgrad)["f32"]
    saved = None
    if save:
        saved = dict(x=x2, h1=h1, st1=st1, qkv=qkv, o=o, lse=lse, x1=x1, h2=h2, st2=st2,
                     z=z, g=g, p=p, seeds=(s1, s2, s3), attn_drop=(pa, sa), B=B, L=L, blk=blk,
                     mask=mask, plan=plan)
    if next_norm is not None:
        return x2o.view(B, L, D), saved, nxt
    return x2o.view(B, L, D), saved


def pooled_head_fwd(x: torch.Tensor, lin, *, act="gelu", training=False, drop_p=0.0,
                    need_dgrad=False, save=None, pooled_f32=None):
    """mean over L of fp32 (B, L, d) -> Linear -> act [-> dropout]: fp32 (B, out).
    ``pooled_f32``: the mean, when the producer of ``x`` already accumulated it (transformer_block_fwd): a
    (B, 2 d) buffer holding the 64-bit fixed-point accumulator the GEMM epilogue added into."""
    B, L, D = x.shape
    pooled_acc = pooled_f32 is not None
    save = training if save is None else save
    p = drop_p if training else 0.0
    seed = _next_seed() if p > 0 else 0
    if D % 16 == 0 and D <= 1024:                    # fp32 head kernel: one small launch instead of a 1-workgroup GEMM
        if pooled_f32 is None:
            pooled_f32 = _empty((B, D), _F32, x)
            _hip.call("mm_meanpool_fwd", x, pooled_f32, None, B, L, D)
        N = lin.weight.shape[0]
        out = _empty((B, N), _F32, x)
        z = _empty((B, N), _BF, x) if save else None
        pooled = _empty((B, D), _BF, x) if save else None
        _hip.call("mm_pooled_head_fwd", None if pooled_acc else pooled_f32, pooled_f32 if pooled_acc else None,
                  lin.weight, lin.bias, out, z, pooled, B, D, N, ACT[act], float(p), int(seed), EP())
        saved = dict(pooled=pooled, z=z, seed=seed, drop_p=p, B=B, L=L, D=D, lin=lin, act=act, fused=True) if save else None
        return out, saved
    pooled = _empty((B, D), _BF, x)
    _hip.call("mm_meanpool_fwd", x, None, pooled, B, L, D)
    r = linear_rows(pooled, lin.weight, lin.bias, act=act, out_f32=True, out_bf16=False,
                    out_pre=save, drop_p=p, seed=seed, need_dgrad=need_dgrad)
    saved = dict(pooled=pooled, z=r["pre"], seed=seed, drop_p=p, B=B, L=L, D=D, lin=lin,
                 act=act) if save else None
    return r["f32"], saved


def pe_table(pos_encoder, L: int) -> torch.Tensor:
    """(L, d) fp32 view of the sinusoid buffer (max_len, 1, d)."""
    pe = pos_encoder.pe
    if L > pe.shape[0]:
        raise ValueError(f"sequence length {L} exceeds PositionalEncoding max_len {pe.shape[0]}")
    return pe[:L, 0, :].contiguous()


# ------------------------------------------------------------ EEG encoders
def _encoder_tail_impl(m, h, training: bool, need_dgrad: bool, save: bool, prenorm=None, stages=None, mask=None):
    """shared tail of both EEG encoders: transformer stack -> mean pool -> Linear -> GELU.
    ``prenorm``: (norm1(h) bf16, stats) of the FIRST block when the producer of ``h`` already formed it.
    ``stages`` (dict, inspection only): receives a copy of the residual stream after every block (``block<i>``).
    ``mask`` (additive fp32, ``additive_attn_mask``): every block's attn_mask; the encoders' own forward passes none."""
    blocks = []
    B, L, D = h.shape
    nblk = len(m.transformer_layers)
    # 64-bit fixed-point mean accumulator (one replica): the last block's GEMM epilogue adds into it
    pooled = _zeros((B, 2 * D), h) if nblk and L % 32 == 0 and D == 128 else None
    layers = list(m.transformer_layers)
    for i, blk in enumerate(layers):
        if i < nblk - 1:                                 # the next block's norm1 rides in this block's last GEMM
            h, s, prenorm = transformer_block_fwd(h, blk, training, need_dgrad, save=save, prenorm=prenorm,
                                                  next_norm=layers[i + 1].norm1, next_blk=layers[i + 1], mask=mask)
        else:
            h, s = transformer_block_fwd(h, blk, training, need_dgrad, save=save, pool_out=pooled, prenorm=prenorm, mask=mask)
        blocks.append(s)
        if stages is not None:
            stages[f"block{i}"] = h.clone()
    out, s = pooled_head_fwd(h, m.output_proj[2], training=training, drop_p=m.drop_p, need_dgrad=need_dgrad,
                             save=save, pooled_f32=pooled)
    return out, blocks, s, h


def _erp_forward_impl(m, x: torch.Tensor, training: bool, need_dgrad: bool, save=None, xb=None, stages=None, mask=None):
    """EnhancedERPEncoder forward; returns (features fp32 (B, H), saved list).
    ``save`` (default = training): keep what a backward needs (eval + save = frozen BatchNorm).
    ``xb``: ``pack_nct(x)`` when the caller already holds it (a trainer stages its inputs packed).
    ``stages`` (dict, inspection only - the parity tests hold the HIP path's intermediate activations against the
    reference's, enhanced_models_v4.py:169-193): receives channels-last copies of what the path materialises - ``conv1``
    / ``conv2`` (bf16 (B, T, C)), ``pos`` (fp32, conv block 3 + positional table, one launch) and ``block<i>`` - plus
    ``conv3``, which the fused launch never forms: one EXTRA launch of the same kernel without the table."""
    cl = m.conv_layers
    save = training if save is None else save
    p = m.drop_p if training else 0.0
    if xb is None:
        xb = pack_nct(x)
    saved = []
    saved_in = []                                        # conv block outputs (for ``stages``)
    r, s = conv_bn_act(xb, cl[0], cl[1], training=training, drop_p=p, need_dgrad=need_dgrad, save=save)
    saved.append(s)
    saved_in.append(r["bf16"])
    r, s = conv_bn_act(r["bf16"], cl[4], cl[5], pool=2, training=training, drop_p=p,
                       drop_first=False, need_dgrad=need_dgrad, save=save)
    saved.append(s)
    saved_in.append(r["bf16"])
    L = r["bf16"].shape[1]
    r, s = conv_bn_act(r["bf16"], cl[9], cl[10], training=training, drop_p=p,
                       pe=pe_table(m.pos_encoder, L), pe_drop_p=(m.pos_encoder.dropout.p if training else 0.0),
                       want_f32=True, want_bf16=False, need_dgrad=need_dgrad, save=save,
                       next_norm=m.transformer_layers[0].norm1 if len(m.transformer_layers) else None)
    saved.append(s)
    if stages is not None:
        stages["conv1"], stages["conv2"] = saved_in[0].clone(), saved_in[1].clone()
        stages["pos"] = r["f32"].clone()
        if not save:                                     # (the fused eval launch: BatchNorm folded into the GEMM epilogue)
            wf3 = weights.get(cl[9].weight, need_dgrad)[0]
            o4 = bn_fold_eval(cl[10], cl[9].bias)
            stages["conv3"] = igemm(saved_in[1], wf3, cl[9].kernel_size[0], cl[9].padding[0], cl[9].out_channels,
                                    scale=o4[0], shift=o4[1], act="gelu", out_f32=True, out_bf16=False)["f32"]
    out, blocks, s, h = _encoder_tail_impl(m, r["f32"], training, need_dgrad, save, prenorm=r.get("prenorm"), stages=stages,
                                           mask=mask)
    return out, dict(convs=saved, blocks=blocks, head=s, x_shape=tuple(x.shape), tokens=h)


def erp_encoder_forward(m, x: torch.Tensor) -> torch.Tensor:
    _need_gpu(x)
    if m.training or _wants_grad(m, x):
        from .autograd import ErpEncoderFn
        return ErpEncoderFn.run(m, x)
    with torch.no_grad():
        return _erp_forward_impl(m, x.float(), False, False)[0]


def _wants_grad(m, x) -> bool:
    """a backward may follow: autograd is on and the input or a parameter asks for a gradient"""
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in m.parameters()))


def add_positional(x, pe, drop_p, training):
    """PositionalEncoding.forward on the fp32 stream (reference quirk kept, enhanced_models_v4.py:49:
    a 3-D input is batch-first unless ``x.size(1) == 1``, which is read as (seq, batch=1, d))."""
    _need_gpu(x)
    if x.dim() != 3:
        raise ValueError("PositionalEncoding: expected a 3-D input (batch, seq, d_model) or (seq, 1, d_model)")
    L = x.size(1) if x.size(1) != 1 else x.size(0)
    if L > pe.shape[0]:
        raise ValueError(f"sequence length {L} exceeds PositionalEncoding max_len {pe.shape[0]}")
    from .autograd import AddPositionalFn
    return AddPositionalFn.apply(x, pe, float(drop_p) if training else 0.0)


def add_positional_impl(x, pe, p: float, seed: int, backward: bool = False):
    """one mm_add_pe launch; x (B, L, D) batch-first or (L, 1, D); ``backward``: mask only."""
    shape = x.shape
    if x.size(1) != 1:
        B, L, D = shape
    else:
        L, B, D = shape[0], 1, shape[2]
    xf = x.float().contiguous()
    tab = None if backward else pe[:L, 0, :].contiguous()
    out = _empty(tuple(shape), _F32, xf)
    _hip.call("mm_add_pe", xf, tab, out, None, B, L, D, float(p), int(seed), EP())
    return out


def transformer_block(x, blk, training, mask=None):
    _need_gpu(x)
    mask = additive_attn_mask(mask, x.shape[1], x)
    if training or (torch.is_grad_enabled() and x.requires_grad):
        from .autograd import TransformerBlockFn
        return TransformerBlockFn.run(blk, x, mask)
    with torch.no_grad():
        return transformer_block_fwd(x.float().contiguous(), blk, False, mask=mask)[0]


# --------------------------------------------------------- 3-D voxel encoder
def pack_volume(x: torch.Tensor) -> torch.Tensor:
    """(B, 1, D, H, W) fp32 -> (B, D, H, W, 16) bf16 (channel 0 = voxel)."""
    B, C, D, H, W = x.shape
    if C != 1:
        raise _hip.HipLibraryError("fMRIVolumeEncoder3D: single-channel volumes only")
    y = _empty((B, D, H, W, 16), _BF, x)
    _hip.call("mm_pack_volume_bf16", x.contiguous(), y, B * D * H * W, 16)
    return y


def conv3d_bn_act(xv: torch.Tensor, conv, bn, *, pool: bool, training: bool, drop_p: float,
                  need_dgrad: bool, save=None):
    """Conv3d(k3,p1) -> BatchNorm3d -> GELU [-> MaxPool3d(2)] [-> Dropout] on
    channels-last bf16 volumes.  Returns (out, saved).  A pooled layer keeps its pre-BatchNorm
    tensor in bf16 (half the traffic of the conv's output, the pooling pass and the backward; the
    statistics come from the fp32 accumulators); the un-pooled last layer keeps fp32.
    eval with ``save`` (a backward will follow: frozen BatchNorm - fine-tuning on a frozen encoder, saliency):
    the train-shaped pipeline with the RUNNING statistics, no statistic update, no dropout."""
    save = training if save is None else save
    B, D, H, W, cinp = xv.shape
    cout = conv.out_channels
    wf, _, cp, _ = weights.get(conv.weight, need_dgrad)
    assert cp == cinp, (cp, cinp)
    y = _empty((B, D, H, W, cout), _BF if pool else _F32, xv)
    yf, yb = (None, y) if pool else (y, None)
    fin = None
    if training:
        stats = _zeros((REPL, 2, cout), xv)
        cal = kernel_timer.bracket(f"event_pair_c{cinp}")    # an EMPTY bracket on the same stream: what a pair of
        if cal is not None:                                  # HIP event records costs by itself (calibration)
            cal.record()
        end = kernel_timer.bracket(f"conv3d_fwd_c{cinp}")
        _hip.call("mm_conv3d_fwd", xv, wf, B, D, H, W, cinp, cout, conv.bias, stats, yf, yb)
        if end is not None:
            end.record()
        if cout <= 256:                                # the finalize runs in the prologue of the apply pass below
            fin, out4 = bn_fin_desc(bn, stats, B * D * H * W)
        else:
            out4 = bn_finalize_train(bn, stats, B * D * H * W)
    elif save:
        _hip.call("mm_conv3d_fwd", xv, wf, B, D, H, W, cinp, cout, conv.bias, None, yf, yb)
        out4 = bn_fold_eval(bn, None)
    else:
        _hip.call("mm_conv3d_fwd", xv, wf, B, D, H, W, cinp, cout, None, None, yf, yb)
        out4 = bn_fold_eval(bn, conv.bias)
    seed = _next_seed() if (training and drop_p > 0) else 0
    p = drop_p if training else 0.0
    ysel = arg = None
    fold = training and fin is not None
    if pool:
        out = _empty((B, D // 2, H // 2, W // 2, cout), _BF, xv)
        if save:                                       # the window winners: all that BN-backward's reduction needs
            ysel = _empty(out.shape, _BF, xv)
            arg = _empty(out.shape, torch.uint8, xv)
        if fold:
            import ctypes
            _hip.call("mm_pool3d_bn_act_fwd_fin", y, ctypes.addressof(fin), out, ysel, arg, B, D, H, W, cout, ACT["gelu"], float(p), seed, EP())
        else:
            _hip.call("mm_pool3d_bn_act_fwd", y, out4, out, ysel, arg, B, D, H, W, cout, ACT["gelu"], float(p), seed, EP())
    else:
        out = _empty((B, D * H * W, cout), _F32, xv)
        if fold:
            import ctypes
            _hip.call("mm_bn_act_fwd_fin", y, ctypes.addressof(fin), None, None, out, B, D * H * W, cout,
                      ACT["gelu"], 1, 1, float(p), seed, 0.0, 0, EP())
        else:
            _hip.call("mm_bn_act_fwd", y, out4[0], out4[1], None, None, out, B, D * H * W, cout,
                      ACT["gelu"], 1, 1, float(p), seed, 0.0, 0, EP())
    saved = dict(xv=xv, y=y, out4=out4, pool=pool, drop_p=p, seed=seed, conv=conv, bn=bn,
                 ysel=ysel, arg=arg, train=training) if save else None
    return out, saved


def conv3d_l1_bn_act(x: torch.Tensor, conv, bn, *, training: bool, drop_p: float, save=None, winners=None):
    """fused first layer on the raw fp32 volume (B, 1, D, H, W); see conv3d_l1.hip.  ``save`` without ``training``:
    frozen BatchNorm (running statistics), a backward will follow.  ``winners`` (list, inspection only): receives the
    u8 (B, D/2, H/2, W/2, 32) tensor of pooling-window winners the forward launch then also writes."""
    save = training if save is None else save
    B, _, D, H, W = x.shape
    wimg = weights.get(conv.weight.view(32, 27, 1), False, key=conv.weight)[0]
    out = _empty((B, D // 2, H // 2, W // 2, 32), _BF, x)
    p = drop_p if training else 0.0
    seed = _next_seed() if p > 0 else 0
    gramc = fin = None
    if training:
        # BatchNorm statistics from the Gram matrix of the im2col matrix (no per-channel pass over the convolution):
        # csrc/conv3d_l1.hip.  The workspace is kept: the backward's weight-gradient correction terms come from it.
        gram = _zeros((REPL, 32, 32), x)
        stats = _zeros((REPL, 2, 32), x)
        _hip.call("mm_conv3d_l1_gram", x, wimg, conv.bias, gram, stats, B, D, H, W)
        gramc = gram                                   # (the accumulator workspace itself: the backward's combine step reads it)
        if winners is None:                            # the finalize runs in the forward kernel's prologue
            fin, out4 = bn_fin_desc(bn, stats, B * D * H * W)
        else:
            out4 = bn_finalize_train(bn, stats, B * D * H * W)
        bias = conv.bias
    elif save:
        out4 = bn_fold_eval(bn, None)                  # the backward recomputes conv + bias and needs mean / rstd apart
        bias = conv.bias
    else:
        out4 = bn_fold_eval(bn, conv.bias)
        bias = None
    if training and fin is not None:
        import ctypes
        _hip.call("mm_conv3d_l1_fwd_fin", x, wimg, bias, ctypes.addressof(fin), out, B, D, H, W, float(p), seed, EP())
    elif winners is not None:
        arg = _empty(tuple(out.shape), torch.uint8, x)
        _hip.call("mm_conv3d_l1_fwd_winners", x, wimg, bias, out4, out, arg, B, D, H, W, 1 if training else 0, float(p), seed, EP())
        winners.append(arg)
    else:
        _hip.call("mm_conv3d_l1", 1, x, wimg, bias, out4, None, None, None, out, None, None,
                  B, D, H, W, 1 if training else 0, float(p), seed, EP())
    saved = dict(l1=True, x=x, wimg=wimg, out4=out4, drop_p=p, seed=seed, conv=conv, bn=bn, train=training, gramc=gramc) if save else None
    return out, saved


def check_volume_shape(shape):
    """(B, C, D, H, W) with every spatial extent >= 4: the encoder's two MaxPool3d(2) floor odd extents, as torch, and
    an axis shorter than 4 leaves the second pool empty (torch raises on it too)."""
    if len(shape) != 5:
        raise ValueError(f"fMRIVolumeEncoder3D: expected a (B, C, D, H, W) volume batch, got shape {tuple(shape)}")
    if min(shape[2:]) < 4:
        raise ValueError(f"fMRIVolumeEncoder3D: every spatial extent must be >= 4 (two MaxPool3d(2) layers), "
                         f"got D, H, W = {tuple(shape[2:])}")


VOLUME_WIDTH_MAX = 1024


def volume_width_ok(w) -> bool:
    """a channel width the voxel encoder's kernels take on both sides of a convolution: 16, or a multiple of 32 up to
    `VOLUME_WIDTH_MAX`.  A layer's output is the next layer's unpadded channels-last input and, in the backward, the
    data-gradient GEMM's input: mm_conv3d_fwd reads Cin = 16 or a multiple of 32 (one 16-channel or whole 32-channel LDS
    chunks), `cpad` pads weight images to multiples of 16 only, mm_conv3d_wgrad wants multiples of 8, and the
    BatchNorm / pool passes and the pooled head stop at 1 024 channels."""
    try:
        w = w.__index__()
    except (AttributeError, TypeError):
        return False
    return w == 16 or (w % 32 == 0 and 32 <= w <= VOLUME_WIDTH_MAX)


def check_volume_widths(widths):
    """``fMRIVolumeEncoder3D(widths=(w0, w1, w2))``: refuse what the kernels cannot run with a ValueError, before any
    launch (a width of 48 used to die on an assert in the backward pass only)."""
    try:
        ws = tuple(widths)
    except TypeError:
        ws = ()
    if len(ws) != 3 or not all(volume_width_ok(w) for w in ws):
        raise ValueError(f"fMRIVolumeEncoder3D: widths must be three channel counts, each 16 or a multiple of 32 up to "
                         f"{VOLUME_WIDTH_MAX} (16, 32, 64, 96, 128, ...), got {widths!r}")


def _vol_forward_impl(m, x: torch.Tensor, training: bool, need_dgrad: bool, save=None, need_dx: bool = False, winners=None):
    """``save`` (default = training): keep what a backward needs; eval + save = frozen BatchNorm.  ``need_dx``: the
    caller wants d / d volume - layer 1 then runs as an ordinary implicit GEMM on the channel-padded volume (the
    fused layer-1 kernels never form its data gradient).  ``winners`` (list, inspection only; needs ``save``): receives
    the two max-pool layers' window winners, u8 channels-last, j = (dd << 2) | (hh << 1) | ww."""
    save = training if save is None else save
    cl = m.conv_layers
    p = m.drop_p
    saved = []
    B, C, D, H, W = x.shape
    check_volume_shape(x.shape)
    x = x.contiguous()
    if C == 1 and cl[0].out_channels == 32 and not need_dx:
        h, s = conv3d_l1_bn_act(x, cl[0], cl[1], training=training, drop_p=p, save=save, winners=winners)
    else:
        h, s = conv3d_bn_act(pack_volume(x), cl[0], cl[1], pool=True, training=training, drop_p=p,
                             need_dgrad=need_dgrad or need_dx, save=save)
    saved.append(s)
    h, s = conv3d_bn_act(h, cl[5], cl[6], pool=True, training=training, drop_p=p, need_dgrad=need_dgrad, save=save)
    saved.append(s)
    if winners is not None:
        if len(winners) == 0:                            # layer 1 took the generic path: its winners are saved like layer 2's
            winners.append(saved[0]["arg"])
        winners.append(s["arg"])
    h, s = conv3d_bn_act(h, cl[10], cl[11], pool=False, training=training, drop_p=p, need_dgrad=need_dgrad, save=save)
    saved.append(s)
    out, hs = pooled_head_fwd(h, m.output_proj[2], training=training, drop_p=p, need_dgrad=need_dgrad, save=save)
    return out, dict(convs=saved, head=hs, x_shape=tuple(x.shape), need_dx=need_dx)


def volume_encoder_forward(m, x: torch.Tensor) -> torch.Tensor:
    check_volume_shape(x.shape)
    _need_gpu(x)
    if m.training or _wants_grad(m, x):
        from .autograd import VolumeEncoderFn
        return VolumeEncoderFn.run(m, x)
    with torch.no_grad():
        return _vol_forward_impl(m, x.float(), False, False)[0]


# ------------------------- lag attention pooling over fMRI frame sequences (fp32, csrc/lagpool.hip: one launch each way)
LAG_MAX_FRAMES = 64
LAG_MAX_DIM = 1024


def lag_pool_check(frames, dim, who: str = "lag_pool"):
    """what mm_lagpool_fwd / mm_lagpool_bwd take, checked before any launch: 1 <= F <= 64 frames of N features, N a
    multiple of 4 in 4..1024"""
    if not 1 <= int(frames) <= LAG_MAX_FRAMES:
        raise ValueError(f"{who}: frames must be in 1..{LAG_MAX_FRAMES}, got {frames}")
    if int(dim) % 4 != 0 or not 4 <= int(dim) <= LAG_MAX_DIM:
        raise ValueError(f"{who}: the feature width must be a multiple of 4 in 4..{LAG_MAX_DIM}, got {dim}")


def _lag_pool_args(x, q, c, who: str):
    if x.dim() != 3:
        raise ValueError(f"{who}: expected (B, F, N) frame features, got shape {tuple(x.shape)}")
    B, F, N = x.shape
    lag_pool_check(F, N, who)
    if B < 1:
        raise ValueError(f"{who}: empty batch")
    if q.numel() != N or (c is not None and c.numel() != F):
        raise ValueError(f"{who}: query must have N = {N} elements and lag_bias F = {F}, got {q.numel()}"
                         f"{'' if c is None else f' and {c.numel()}'}")
    return B, F, N


def _chunked(t: torch.Tensor) -> torch.Tensor:
    """fp32, contiguous and 16-byte aligned, as the lag pool's kernels read activations (a copy only when it is not)"""
    t = t.detach().float().contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def lag_pool_fwd(x: torch.Tensor, query: torch.Tensor, lag_bias: torch.Tensor):
    """x (B, F, N) fp32 frame features -> (out (B, N), weights (B, F)): weights = softmax over the frames of
    (x . query) / sqrt(N) + lag_bias, out = the weighted sum of the frames (mm_lagpool_fwd, one launch)"""
    B, F, N = _lag_pool_args(x, query, lag_bias, "lag_pool_fwd")
    _need_gpu(x, query, lag_bias)
    xc = _chunked(x)
    out, attw = _empty((B, N), _F32, xc), _empty((B, F), _F32, xc)
    _hip.call("mm_lagpool_fwd", xc, query.detach().float().contiguous(), lag_bias.detach().float().contiguous(), out, attw, B, F, N)
    return out, attw


def lag_pool_bwd(dout: torch.Tensor, x: torch.Tensor, weights: torch.Tensor, query: torch.Tensor):
    """-> (dx (B, F, N), dparts (B, N + F)): the gradient of `lag_pool_fwd` w.r.t. the frames and the per-sample rows
    (d query | d lag_bias), whose sums in ascending b are the two parameter gradients (mm_lagpool_bwd, one launch)"""
    B, F, N = _lag_pool_args(x, query, None, "lag_pool_bwd")
    if tuple(dout.shape) != (B, N) or tuple(weights.shape) != (B, F):
        raise ValueError(f"lag_pool_bwd: dout must be {(B, N)} and weights {(B, F)}, got {tuple(dout.shape)} and {tuple(weights.shape)}")
    _need_gpu(dout, x, weights, query)
    xc = _chunked(x)
    dx, dparts = _empty((B, F, N), _F32, xc), _empty((B, N + F), _F32, xc)
    _hip.call("mm_lagpool_bwd", _chunked(dout), xc, weights.detach().float().contiguous(),
              query.detach().float().contiguous(), dx, dparts, B, F, N)
    return dx, dparts


def lag_pool(x: torch.Tensor, query: torch.Tensor, lag_bias: torch.Tensor):
    """`lag_pool_fwd` on the autograd tape (`autograd.LagPoolFn`) -> (out (B, N), weights (B, F)); the weights are a
    read-out and carry no gradient"""
    _lag_pool_args(x, query, lag_bias, "lag_pool")
    _need_gpu(x, query, lag_bias)
    if torch.is_grad_enabled() and (x.requires_grad or query.requires_grad or lag_bias.requires_grad):
        from .autograd import LagPoolFn
        return LagPoolFn.apply(x, query, lag_bias)
    with torch.no_grad():
        return lag_pool_fwd(x, query, lag_bias)


def check_sequence_shape(m, shape, who: str = "fMRISequenceEncoder3D"):
    """(B, F, D, H, W) with F = the encoder's frame count and every spatial extent >= 4 (`check_volume_shape`)"""
    if len(shape) != 5:
        raise ValueError(f"{who}: expected a (B, F, D, H, W) batch of fMRI frame sequences, got shape {tuple(shape)}")
    if shape[1] != m.frames:
        raise ValueError(f"{who}: the encoder pools F = {m.frames} frames, the batch has {shape[1]} (shape {tuple(shape)})")
    if min(shape[2:]) < 4:
        raise ValueError(f"{who}: every spatial extent must be >= 4 (two MaxPool3d(2) layers), got D, H, W = {tuple(shape[2:])}")
    if shape[0] < 1:
        raise ValueError(f"{who}: empty batch")


def _seq_forward_impl(m, x: torch.Tensor, live: bool, save=None, need_dx: bool = False):
    """`fMRISequenceEncoder3D` forward: the (B, F, D, H, W) batch is viewed as B * F single-channel volumes
    (B * F, 1, D, H, W), run through `_vol_forward_impl` on ``m.frame_encoder`` and pooled over the frames
    (mm_lagpool_fwd).  BY DEFINITION the train-mode BatchNorm statistics are those of all B * F volumes - every frame of
    every sample counts alike, and the running statistics are updated once per step with them.
    ``live`` False = the frozen form (eval kernels, no dropout seed drawn, nothing saved unless ``save``); ``save`` (default
    = live) keeps what `autograd.sequence_encoder_bwd` needs; ``need_dx``: the caller wants d / d frames.
    -> (features (B, out_dim), saved); saved["weights"] (B, F) are the lag weights of this pass."""
    save = live if save is None else save
    check_sequence_shape(m, x.shape)
    B, F, D, H, W = x.shape
    vols = x.float().contiguous().view(B * F, 1, D, H, W)
    feats, sv = _vol_forward_impl(m.frame_encoder, vols, live, save, save=save, need_dx=need_dx)
    pool = m.lag_pool
    out, attw = lag_pool_fwd(feats.view(B, F, -1), pool.query, pool.lag_bias)
    if not save:
        return out, dict(weights=attw)
    return out, dict(vol=sv, feats=feats, weights=attw, pool=pool, B=B, F=F, need_dx=need_dx)


def sequence_encoder_forward(m, x: torch.Tensor, return_weights: bool = False):
    check_sequence_shape(m, x.shape)
    _need_gpu(x)
    if m.training or _wants_grad(m, x):
        from .autograd import SequenceEncoderFn
        out, attw = SequenceEncoderFn.run(m, x)
    else:
        with torch.no_grad():
            out, sv = _seq_forward_impl(m, x, False)
            attw = sv["weights"]
    return (out, attw) if return_weights else out


# ------------------------------------------------- projection bridge (fp32)
def small_linear(x: torch.Tensor, lin, *, act="none", drop_p=0.0, seed=0, want_pre=False, bn=None,
                 weight=None, bias=None):
    """fp32 (B, K) -> (B, N): dropout(act((x W^T + b) * scale + shift)); scale/shift
    = eval-mode BatchNorm1d ``bn`` folded; optional pre-activation copy."""
    W = lin.weight if weight is None else weight
    bvec = (lin.bias if lin is not None else None) if bias is None else bias
    B, K = x.shape
    N = W.shape[0]
    y = _empty((B, N), _F32, x)
    pre = _empty((B, N), _F32, x) if want_pre else None
    sc = sh = None
    if bn is not None:
        out4 = bn_fold_eval(bn, None)
        sc, sh = out4[0], out4[1]
    _hip.call("mm_small_linear_fwd", x, W, bvec, sc, sh, y, pre, B, K, N, ACT[act], float(drop_p), int(seed), EP())
    return y, pre


def proj_head_fwd(seq, x: torch.Tensor, training: bool, drop_p: float):
    """Linear -> LayerNorm -> GELU -> Dropout (bridge_utils.py:34-45) in fp32."""
    lin, ln = seq[0], seq[1]
    B = x.shape[0]
    N = lin.weight.shape[0]
    z1, _ = small_linear(x, lin)
    hn = _empty((B, N), _F32, x)
    stat = _empty((B, 2), _F32, x)
    _hip.call("mm_layernorm_fwd", z1, ln.weight, ln.bias, None, hn, stat, B, N, float(ln.eps))
    p = drop_p if training else 0.0
    seed = _next_seed() if p > 0 else 0
    a = _empty((B, N), _F32, x)
    _hip.call("mm_act_f32", hn, a, B * N, ACT["gelu"], float(p), seed, EP())
    return a, dict(x=x, z1=z1, hn=hn, stat=stat, p=p, seed=seed, seq=seq)


def contrastive_embed_impl(bridge, eeg: torch.Tensor, fmri: torch.Tensor, training: bool):
    """-> packed L2-normalised embeddings z (B, 2N) = [ze | zf], saved."""
    B = eeg.shape[0]
    N = bridge.bridge_dim
    xe, xf = eeg.float().contiguous(), fmri.float().contiguous()
    (le, lne), (lf, lnf) = bridge.eeg_proj[:2], bridge.fmri_proj[:2]
    assert lne.eps == lnf.eps
    p = float(bridge.drop_p) if training else 0.0
    se, sf = (_next_seed(), _next_seed()) if p > 0 else (0, 0)
    z = _empty((B, 2 * N), _F32, eeg)
    nrm = _empty((2, B), _F32, eeg)
    z1 = _empty((2, B, N), _F32, eeg)
    hn = _empty((2, B, N), _F32, eeg)
    stat = _empty((2, B, 2), _F32, eeg)
    _hip.call("mm_proj_heads_fwd", xe, le.weight, le.bias, lne.weight, lne.bias, xe.shape[1],
              xf, lf.weight, lf.bias, lnf.weight, lnf.bias, xf.shape[1],
              z1, hn, stat, z, nrm, B, N, float(lne.eps), p, se, sf, EP())
    return z, dict(xe=xe, xf=xf, z1=z1, hn=hn, stat=stat, z=z, nrm=nrm, B=B, N=N, p=p, seeds=(se, sf), bridge=bridge)


def proj_embed_one(bridge, x: torch.Tensor, modality: str) -> torch.Tensor:
    """eval-mode L2-normalised embedding (B, bridge_dim) of ONE modality's encoder features.  mm_proj_heads_fwd
    unchanged, with that modality's head in both halves: each half is computed on its own, so the result is the
    same bits as the same half of the paired embedding (contrastive_embed_impl); no dropout, no seed drawn."""
    _need_gpu(x)
    if modality not in ("eeg", "fmri"):
        raise ValueError(f"proj_embed_one: modality must be 'eeg' or 'fmri', got {modality!r}")
    B = x.shape[0]
    N = bridge.bridge_dim
    xc = x.detach().float().contiguous()
    lin, ln = (bridge.eeg_proj if modality == "eeg" else bridge.fmri_proj)[:2]
    z = _empty((B, 2 * N), _F32, x)
    nrm = _empty((2, B), _F32, x)
    z1 = _empty((2, B, N), _F32, x)
    hn = _empty((2, B, N), _F32, x)
    stat = _empty((2, B, 2), _F32, x)
    _hip.call("mm_proj_heads_fwd", xc, lin.weight, lin.bias, ln.weight, ln.bias, xc.shape[1],
              xc, lin.weight, lin.bias, ln.weight, ln.bias, xc.shape[1],
              z1, hn, stat, z, nrm, B, N, float(ln.eps), 0.0, 0, 0, EP())
    return z[:, :N].contiguous()


# ------------------------------------------- classification branch of the bridge (fp32, csrc/bridge_cls.hip)
CLS_MAX_CLASSES = 16


def bridge_cls_check(bridge_dim: int, num_heads: int, num_classes: int, who: str = "bridge_cls"):
    """the shapes mm_bridge_cls_fwd / _bwd serve (the same test as their MM_REQUIRE): ValueError before any launch"""
    if bridge_dim % 32 != 0 or not 32 <= bridge_dim <= 256:
        raise ValueError(f"{who}: bridge_dim must be a multiple of 32 in [32, 256] (got {bridge_dim})")
    if not 1 <= num_heads <= 16 or bridge_dim % num_heads != 0:
        raise ValueError(f"{who}: num_heads must be <= 16 and divide bridge_dim {bridge_dim} (got {num_heads})")
    if not 2 <= num_classes <= CLS_MAX_CLASSES:
        raise ValueError(f"{who}: num_classes must be in [2, {CLS_MAX_CLASSES}] (got {num_classes})")


def class_labels(labels, B: int, C: int, device=None, who: str = "labels") -> Optional[torch.Tensor]:
    """Validate a (B,) vector of class labels -> int32 on ``device``, or None for None.  A host tensor of any integer
    dtype is checked against [0, C) and converted; a device tensor must already be int32 (checking its values would
    synchronise a replayed step: the kernel gives a row whose label is outside [0, C) weight 0)."""
    if labels is None:
        return None
    if not isinstance(labels, torch.Tensor):
        raise ValueError(f"{who}: class labels must be a torch.Tensor (got {type(labels).__name__})")
    if labels.dim() != 1 or labels.shape[0] != B:
        raise ValueError(f"{who}: class labels must have shape ({B},) (got {tuple(labels.shape)})")
    if labels.dtype.is_floating_point or labels.dtype.is_complex or labels.dtype == torch.bool:
        raise ValueError(f"{who}: class labels must be an integer tensor (got {labels.dtype})")
    if labels.is_cuda:
        if labels.dtype != torch.int32:
            raise ValueError(f"{who}: class labels on the device must be int32 (got {labels.dtype}); host tensors of any "
                             "integer dtype are converted")
        if device is not None and labels.device != torch.device(device):
            raise ValueError(f"{who}: class labels are on {labels.device}, the batch on {device}")
        return labels.contiguous()
    if B:
        l64 = labels.long()
        if bool((l64 < 0).any()) or bool((l64 >= C).any()):
            raise ValueError(f"{who}: class labels must lie in [0, {C}) (got {int(l64.min())}..{int(l64.max())})")
    l32 = labels.to(torch.int32).contiguous()
    return l32 if device is None else l32.to(device)


def bridge_cls_params(bridge):
    """the parameters of the classification branch in the order of the entry points' arguments"""
    ca, fu, cl = bridge.cross_attn, bridge.fusion, bridge.classifier
    return (ca.in_proj_weight, ca.in_proj_bias, ca.out_proj.weight, ca.out_proj.bias, fu.gate_net[0].weight,
            fu.gate_net[0].bias, fu.gate_net[3].weight, fu.gate_net[3].bias, fu.fusion_logits, fu.temperature,
            cl[0].weight, cl[0].bias, cl[1].weight, cl[1].bias, cl[4].weight, cl[4].bias)


def bridge_cls_forward_impl(bridge, sv_h: dict, training: bool, labels=None, class_weight=None, ce_weight: float = 1.0,
                            loss_out=None, ticket=None):
    """the classification branch on the rows of `contrastive_embed_impl` (``sv_h``: what it saved), ONE launch
    (mm_bridge_cls_fwd) -> (logits (B, C), fusion_w (B, 2), attn_w (B, 2), saved).  ``labels`` int32 (B,) on the device
    (`class_labels`): ``loss_out`` (4,) = {ce, rows classified right, sum of the row weights, ce_weight * ce} is
    written (allocated here when None); without labels it is not touched.  ``ticket``: the int32 word in which
    the launch's workgroups count themselves off (the last one sums the rows' loss terms and leaves it zero) - the
    caller's own zeroed word, which no launch that may run at the same time shares (a trainer keeps one, allocated outside
    any capture); None: a fresh zeroed word for this call (one fill; inside a capture it is a node of that graph).
    Training draws one seed per dropout site whose p > 0: attention probabilities, gate hidden, classifier hidden - the order of `bridge_forward`'s train branch."""
    hn = sv_h["hn"]
    B, N = sv_h["B"], sv_h["N"]
    H = int(bridge.num_heads)
    ps = bridge_cls_params(bridge)
    C = ps[14].shape[0]
    bridge_cls_check(N, H, C)
    if tuple(ps[4].shape) != (N, 2 * N) or tuple(ps[10].shape) != (N // 2, N):
        raise ValueError("bridge_cls: the fusion gate / classifier widths are not those of EEGfMRIBridgeFusionNet")
    if class_weight is not None and (class_weight.dtype != _F32 or tuple(class_weight.shape) != (C,)):
        raise ValueError(f"bridge_cls: class_weight must be fp32 of shape ({C},)")
    pa = float(bridge.cross_attn.dropout) if training else 0.0
    pg = float(bridge.fusion.gate_net[2].p) if training else 0.0
    pc = float(bridge.drop_p) if training else 0.0
    sa_, sg, sc = (_next_seed() if p > 0 else 0 for p in (pa, pg, pc))
    logits = _empty((B, C), _F32, hn)
    fw = _empty((B, 2), _F32, hn)
    aw = _empty((B, 2), _F32, hn)
    save = _empty((_hip.host_int("mm_bridge_cls_ws_floats", B, N, 0),), _F32, hn)
    if labels is None:
        ticket = None
    else:
        if loss_out is None:
            loss_out = _empty((4,), _F32, hn)
        if ticket is None:
            ticket = torch.zeros(1, dtype=torch.int32, device=hn.device)
        elif ticket.dtype != torch.int32 or ticket.numel() != 1 or ticket.device != hn.device:
            raise ValueError("bridge_cls: ticket must be one int32 word on the batch's device")
    eps = float(bridge.classifier[1].eps)
    _hip.call("mm_bridge_cls_fwd", hn, float(sv_h["p"]), int(sv_h["seeds"][0]), int(sv_h["seeds"][1]), *ps,
              labels, class_weight, float(ce_weight), logits, fw, aw, save, loss_out if labels is not None else None,
              ticket, B, N, H, C, eps, pa, sa_, pg, sg, pc, sc, EP())
    saved = dict(save=save, logits=logits, loss=loss_out, labels=labels, ticket=ticket, ce_weight=float(ce_weight), B=B, N=N, H=H, C=C,
                 drops=(pa, sa_, pg, sg, pc, sc), bridge=bridge)
    return logits, fw, aw, saved


def retrieval_ws_floats(nq: int, ng: int, d: int, k: int) -> int:
    """floats of mm_retrieval's scratch (mm_retrieval_ws_floats: the kernel file owns the layout)"""
    return _hip.host_int("mm_retrieval_ws_floats", nq, ng, d, k)


@functools.lru_cache(maxsize=None)
def retrieval_kmax() -> int:
    import re
    m = re.search(r"^#define\s+MM_RETRIEVAL_KMAX\s+(\d+)", open(_hip.header_path()).read(), flags=re.M)
    return int(m.group(1))


def retrieval_grouped_ws_floats(nq: int, ng: int, d: int) -> int:
    """floats of mm_retrieval_grouped's scratch (mm_retrieval_grouped_ws_floats)"""
    return _hip.host_int("mm_retrieval_grouped_ws_floats", nq, ng, d)


def retrieval_masked_ws_floats(nq: int, ng: int, d: int, k: int) -> int:
    """floats of mm_retrieval_masked's scratch (mm_retrieval_masked_ws_floats)"""
    return _hip.host_int("mm_retrieval_masked_ws_floats", nq, ng, d, k)


def retrieval(q: torch.Tensor, g: torch.Tensor, positives: Optional[torch.Tensor] = None, k: int = 0,
              ranks: bool = True, q_groups: Optional[torch.Tensor] = None, g_groups: Optional[torch.Tensor] = None,
              radius: int = 0, return_negatives: bool = False):
    """Rank of each query's positive among all gallery rows and / or its top-k matches (mm_retrieval), without an
    Nq x Ng score matrix.  q (Nq, D), g (Ng, D): contiguous fp32 on the GPU (L2-normalised rows for cosine retrieval).
    positives: int tensor (Nq,) of gallery indices (None: query i's positive is gallery row i).  Scores are exact fp32
    dot products; a tie with the positive counts AGAINST the query (rank = 1 + #{j != pos : s_j >= s_pos}).
    -> (ranks int64 (Nq,) | None, topk_idx int64 (Nq, k) | None, topk_score fp32 (Nq, k) | None); top-k is score
    descending, equal scores by lower index, unfilled slots (-1, -inf).
    q_groups (Nq,) / g_groups (Ng,) integer group ids (both or neither; not with ``positives``; ranks only, k = 0): every
    gallery row of the query's group is a positive, and the rank is that of the best-placed one (mm_retrieval_grouped:
    1 + #{j outside the group : s_j >= max over the group}; a query without a positive ranks Ng).
    ``radius`` > 0 (needs both id vectors): the ids are timeline positions (`bridge_utils.timeline_ids`) and a gallery row
    within ``radius`` of the query's id, not equal to it, is ignored - it never counts against the rank and never enters
    the top-k (mm_retrieval_masked; ``k > 0`` and ``ranks=False`` are allowed here).  ``return_negatives=True`` (needs the
    ids; also mm_retrieval_masked) appends the int64 (Nq,) number of gallery rows further than ``radius`` from each query
    to the tuple.  ``radius=0`` without it: the calls above, unchanged."""
    grouped = q_groups is not None or g_groups is not None
    radius = int(radius)
    if radius < 0:
        raise ValueError(f"retrieval: radius must be >= 0 (got {radius})")
    if radius > 0 and (q_groups is None or g_groups is None):
        raise ValueError(f"retrieval: radius={radius} needs group ids (q_groups and g_groups: positions on a timeline)")
    if return_negatives and (q_groups is None or g_groups is None):
        raise ValueError("retrieval: return_negatives=True needs group ids (q_groups and g_groups)")
    masked = radius > 0 or bool(return_negatives)          # radius = 0 without the count: today's calls
    if grouped:
        if q_groups is None or g_groups is None:
            raise ValueError("retrieval: give both q_groups and g_groups, or neither")
        if positives is not None:
            raise ValueError("retrieval: positives and group ids are exclusive")
        if not masked and (not ranks or int(k) != 0):
            raise ValueError("retrieval: with group ids only ranks are computed (ranks=True, k = 0; top-k does not depend on groups)")
    for name, t in (("q", q), ("g", g)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError(f"retrieval: {name} must be a 2-D tensor")
        if not t.is_cuda:
            raise _hip.HipLibraryError(f"retrieval: {name} is a CPU tensor; the HIP path has no CPU fallback")
        if t.dtype != torch.float32:
            raise ValueError(f"retrieval: {name} must be float32 (got {t.dtype})")
        if not t.is_contiguous():
            raise ValueError(f"retrieval: {name} must be contiguous")
    _hip.load()
    nq, d = q.shape
    ng = g.shape[0]
    if g.shape[1] != d:
        raise ValueError(f"retrieval: q has D = {d}, g has D = {g.shape[1]}")
    if q.device != g.device:
        raise ValueError("retrieval: q and g are on different devices")
    if masked:
        k = int(k)
        if not 0 <= k <= min(retrieval_kmax(), ng):
            raise ValueError(f"retrieval: k must be in [0, min({retrieval_kmax()}, Ng = {ng})] (got {k})")
        if not ranks and k == 0:
            raise ValueError("retrieval: nothing to compute (ranks=False and k = 0)")
        qg = group_ids(q_groups, nq, q.device, "retrieval: q_groups")
        gg = group_ids(g_groups, ng, q.device, "retrieval: g_groups")
        ws = torch.empty(retrieval_masked_ws_floats(nq, ng, d, k), dtype=_F32, device=q.device)
        r32 = torch.empty(nq, dtype=torch.int32, device=q.device) if ranks else None
        n32 = torch.empty(nq, dtype=torch.int32, device=q.device) if return_negatives else None
        ti = torch.empty((nq, k), dtype=torch.int32, device=q.device) if k else None
        ts = torch.empty((nq, k), dtype=_F32, device=q.device) if k else None
        with torch.cuda.device(q.device):
            _hip.call("mm_retrieval_masked", q, g, qg, gg, radius, r32, n32, ti, ts, ws, nq, ng, d, k)
        out = (r32.long() if ranks else None, ti.long() if k else None, ts)
        return out + (n32.long(),) if return_negatives else out
    if grouped:
        qg = group_ids(q_groups, nq, q.device, "retrieval: q_groups")
        gg = group_ids(g_groups, ng, q.device, "retrieval: g_groups")
        ws = torch.empty(retrieval_grouped_ws_floats(nq, ng, d), dtype=_F32, device=q.device)
        r32 = torch.empty(nq, dtype=torch.int32, device=q.device)
        with torch.cuda.device(q.device):
            _hip.call("mm_retrieval_grouped", q, g, qg, gg, r32, ws, nq, ng, d)
        return r32.long(), None, None
    k = int(k)
    if not 0 <= k <= min(retrieval_kmax(), ng):
        raise ValueError(f"retrieval: k must be in [0, min({retrieval_kmax()}, Ng = {ng})] (got {k})")
    if not ranks and k == 0:
        raise ValueError("retrieval: nothing to compute (ranks=False and k = 0)")
    pos = None
    if ranks:
        if positives is None:
            if nq > ng:
                raise ValueError(f"retrieval: without positives query i pairs with gallery row i, so Nq ({nq}) <= Ng ({ng})")
        else:
            if positives.shape != (nq,):
                raise ValueError(f"retrieval: positives must have shape ({nq},)")
            if positives.dtype.is_floating_point or positives.dtype == torch.bool:
                raise ValueError("retrieval: positives must be an integer tensor")
            pos = positives.to(device=q.device, dtype=torch.int32).contiguous()
            if nq and bool(((pos < 0) | (pos >= ng)).any()):
                raise ValueError(f"retrieval: positives must lie in [0, {ng})")
    ws = torch.empty(retrieval_ws_floats(nq, ng, d, k), dtype=_F32, device=q.device)
    r32 = torch.empty(nq, dtype=torch.int32, device=q.device) if ranks else None
    ti = torch.empty((nq, k), dtype=torch.int32, device=q.device) if k else None
    ts = torch.empty((nq, k), dtype=_F32, device=q.device) if k else None
    with torch.cuda.device(q.device):
        _hip.call("mm_retrieval", q, g, pos, r32, ti, ts, ws, nq, ng, d, k)
    return (r32.long() if ranks else None, ti.long() if k else None, ts)


def contrastive_embed(bridge, eeg, fmri, training):
    _need_gpu(eeg, fmri)
    from .autograd import ContrastiveEmbedFn
    z = ContrastiveEmbedFn.run(bridge, eeg, fmri)
    N = bridge.bridge_dim
    return z[:, :N], z[:, N:]


def clip_loss(ze, zf, logit_scale, group=None, groups=None, radius: int = 0):
    """symmetric InfoNCE over the (all-gathered) batch -> (loss, top1 e->f, top1 f->e).  ``groups`` (B,) integer ids
    (``group_ids``): pairs with equal ids are positives of each other (mm_clip_loss_own_rows_grouped); None: pair i is
    the only positive of query i.  ``radius`` > 0 (needs ``groups``): the ids are timeline positions
    (`bridge_utils.timeline_ids`) and a key within ``radius`` of the query, not equal to it, is ignored: neither positive
    nor negative, no gradient (mm_clip_loss_own_rows_masked)."""
    _need_gpu(ze)
    gid = group_ids(groups, ze.shape[0], ze.device, "clip_loss")
    radius = _loss_radius(radius, gid, "clip_loss")
    from .autograd import ClipLossFn
    return ClipLossFn.apply(_packed_pair(ze, zf), logit_scale, group, gid, radius)


def clip_loss_bank(ze, zf, logit_scale, bank: ClipBank, groups=None, warmup: int = 0):
    """`clip_loss` against the batch and the valid rows of ``bank`` (mm_clip_bank_loss; single process only) -> (loss,
    top1 e->f, top1 f->e).  The bank is a constant of the tape and is NOT pushed to: follow with `clip_bank_push`."""
    _need_gpu(ze)
    gid = group_ids(groups, ze.shape[0], ze.device, "clip_loss_bank")
    from .autograd import ClipBankLossFn
    return ClipBankLossFn.apply(_packed_pair(ze, zf), logit_scale, bank, gid, warmup)


def clip_loss_key(ze, zf, keys, logit_scale, bank: ClipBank, groups=None, warmup: int = 0):
    """`clip_loss_bank` with a momentum key encoder (mm_clip_key_loss): ``keys`` (B, 2N) = [ke | kf], the key encoder's
    rows of the same pairs, are the batch's keys and constants of the tape like the bank - the gradient reaches ``ze``,
    ``zf`` and ``logit_scale`` only.  NOT pushed to the bank: follow with `clip_bank_push` of ``keys``."""
    _need_gpu(ze)
    gid = group_ids(groups, ze.shape[0], ze.device, "clip_loss_key")
    from .autograd import ClipKeyLossFn
    return ClipKeyLossFn.apply(_packed_pair(ze, zf), keys, logit_scale, bank, gid, warmup)


def sigmoid_loss(ze, zf, logit_scale, logit_bias, group=None, groups=None, radius: int = 0):
    """pairwise sigmoid loss over the (all-gathered) batch (mm_sigmoid_loss_own_rows) -> (loss, top1 e->f, top1 f->e).
    ``groups`` as in `clip_loss`: pairs with equal ids are positives of each other; ``radius`` as there: pairs within it
    are ignored (mm_sigmoid_loss_own_rows_masked)."""
    _need_gpu(ze)
    gid = group_ids(groups, ze.shape[0], ze.device, "sigmoid_loss")
    radius = _loss_radius(radius, gid, "sigmoid_loss")
    from .autograd import SigmoidLossFn
    return SigmoidLossFn.apply(_packed_pair(ze, zf), logit_scale, logit_bias, group, gid, radius)


def _packed_pair(ze: torch.Tensor, zf: torch.Tensor) -> torch.Tensor:
    """(B, 2N) [ze | zf]: the shared base when ze / zf are EXACTLY its two column halves (what
    contrastive_embed returns), a concatenation for anything else (row subsets, other views)."""
    base = ze._base
    if (base is not None and base is zf._base and base.dim() == 2 and base.is_contiguous()
            and ze.dim() == 2 and ze.shape == zf.shape and base.shape == (ze.shape[0], 2 * ze.shape[1])
            and ze.stride() == base.stride() and zf.stride() == base.stride()
            and ze.storage_offset() == base.storage_offset()
            and zf.storage_offset() == base.storage_offset() + ze.shape[1]):
        return base
    return torch.cat([ze, zf], dim=1)



# ----------------------------------------------------- small models (forward)
def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().float().contiguous()


def learned_fusion(m, feats: List[torch.Tensor], training: bool, autograd: bool = False):
    """LearnedFusionModule.forward -> (fused (B, H), weights (B, M)).  ``autograd``: differentiable
    composition even in eval mode (its gate dropout is then off)."""
    _need_gpu(*feats)
    if training or autograd or attribution_active():
        from . import small_autograd as sa
        g = sa.linear(torch.cat(list(feats), dim=1), m.gate_net[0], "gelu", m.gate_net[2].p if training else 0.0)
        dyn = sa.linear(g, m.gate_net[3])
        return sa.LearnedFusionFn.apply(dyn, m.fusion_logits, m.temperature, *feats)
    M = len(feats)
    fs = [_f32c(f) for f in feats]
    B, H = fs[0].shape
    g, _ = small_linear(torch.cat(fs, dim=1), m.gate_net[0], act="gelu")
    dyn, _ = small_linear(g, m.gate_net[3])
    fused = _empty((B, H), _F32, fs[0])
    w = _empty((B, M), _F32, fs[0])
    _hip.call("mm_learned_fusion", fs[0], fs[1], fs[2] if M > 2 else None, dyn, _f32c(m.fusion_logits),
              _f32c(m.temperature).reshape(1), fused, w, B, H, M)
    return fused, w


def bridge_forward(m, eeg, fmri):
    """EEGfMRIBridgeFusionNet.forward -> (logits, fused, fusion_w (B,2), attn_w (B,1,2))."""
    _need_gpu(eeg, fmri)
    # eval mode with a backward to follow (gradient saliency / integrated gradients,
    # bridge_utils.py:158-229): the autograd composition with every dropout off - the bridge has
    # LayerNorms only, so that IS the eval forward
    wants = torch.is_grad_enabled() and (eeg.requires_grad or fmri.requires_grad)
    if m.training or wants:
        from . import small_autograd as sa
        p = m.drop_p if m.training else 0.0
        ca = m.cross_attn
        ep = sa.proj_head(eeg, m.eeg_proj, p)
        fp = sa.proj_head(fmri, m.fmri_proj, p)
        pe = sa.SmallLinearFn.apply(ep, ca.in_proj_weight, ca.in_proj_bias, "none", 0.0)
        pf = sa.SmallLinearFn.apply(fp, ca.in_proj_weight, ca.in_proj_bias, "none", 0.0)
        ctx, attw = sa.Attn1x2Fn.apply(pe, pf, m.num_heads, float(ca.dropout) if m.training else 0.0)
        att = sa.linear(ctx, ca.out_proj)
        fused, fw = learned_fusion(m.fusion, [att, fp], m.training, autograd=True)
        c = m.classifier
        h = sa.ActFn.apply(sa.LayerNormFn.apply(sa.linear(fused, c[0]), c[1].weight, c[1].bias, c[1].eps), "relu", p)
        return sa.linear(h, c[4]), fused, fw, attw.view(-1, 1, 2)
    with torch.no_grad():
        ep, _ = proj_head_fwd(m.eeg_proj, _f32c(eeg), False, 0.0)
        fp, _ = proj_head_fwd(m.fmri_proj, _f32c(fmri), False, 0.0)
        B, E = ep.shape
        ca = m.cross_attn
        pe, _ = small_linear(ep, None, weight=ca.in_proj_weight, bias=ca.in_proj_bias)
        pf, _ = small_linear(fp, None, weight=ca.in_proj_weight, bias=ca.in_proj_bias)
        ctx = _empty((B, E), _F32, ep)
        attw = _empty((B, 2), _F32, ep)
        _hip.call("mm_attn_1x2", pe, pf, ctx, attw, B, E, m.num_heads)
        att, _ = small_linear(ctx, ca.out_proj)
        fused, fw = learned_fusion(m.fusion, [att, fp], False)
        h1, _ = small_linear(fused, m.classifier[0])
        ln = m.classifier[1]
        hn = _empty(h1.shape, _F32, h1)
        _hip.call("mm_layernorm_fwd", h1, ln.weight, ln.bias, None, hn, None, B, h1.shape[1], float(ln.eps))
        hr = _empty(h1.shape, _F32, h1)
        _hip.call("mm_act_f32", hn, hr, hn.numel(), ACT["relu"], 0.0, 0, None)
        logits, _ = small_linear(hr, m.classifier[4])
    return logits, fused, fw, attw.view(B, 1, 2)


def bridge_cls_rows(m, ep, fp):
    """the classification half of `bridge_forward`'s differentiable branch on rows that are already projected
    (ep, fp = the post-dropout outputs of the two projection heads) -> (logits, fusion_w (B, 2), attn_w (B, 2)).
    These are the lines of `bridge_forward`'s train branch after its two projections (that function stays as it is;
    test_bridge_cls_rows_is_bridge_forwards_train_branch holds the two to the same bits).
    The small_autograd composition, one launch per op: the independent path the fused kernels (csrc/bridge_cls.hip)
    are compared with; dropout follows ``m.training`` and draws its seeds in their order."""
    from . import small_autograd as sa
    p = m.drop_p if m.training else 0.0
    ca = m.cross_attn
    pe = sa.SmallLinearFn.apply(ep, ca.in_proj_weight, ca.in_proj_bias, "none", 0.0)
    pf = sa.SmallLinearFn.apply(fp, ca.in_proj_weight, ca.in_proj_bias, "none", 0.0)
    ctx, attw = sa.Attn1x2Fn.apply(pe, pf, m.num_heads, float(ca.dropout) if m.training else 0.0)
    att = sa.linear(ctx, ca.out_proj)
    fused, fw = learned_fusion(m.fusion, [att, fp], m.training, autograd=True)
    c = m.classifier
    h = sa.ActFn.apply(sa.LayerNormFn.apply(sa.linear(fused, c[0]), c[1].weight, c[1].bias, c[1].eps), "relu", p)
    return sa.linear(h, c[4]), fw, attw


def _mlp_bn_act(x, lin, bn, act, drop_p, training):
    """Linear -> BatchNorm1d -> act -> Dropout on fp32 rows (eval: BN folded into the linear)."""
    if training:
        from . import small_autograd as sa
        return sa.linear_bn_act(x, lin, bn, act, drop_p)
    if torch.is_grad_enabled() and (x.requires_grad or lin.weight.requires_grad):
        # eval mode with a backward to follow: frozen BatchNorm (running statistics, no update), dropout off
        from . import small_autograd as sa
        return sa.linear_bn_act(x, lin, bn, act, 0.0, frozen=True)
    return small_linear(_f32c(x), lin, act=act, bn=bn)[0]


def small_autograd_linear(x, lin, act="none", drop_p=0.0):
    """differentiable fp32 Linear (+ activation, dropout) on (B, K) rows: small_autograd.linear"""
    from . import small_autograd as sa
    return sa.linear(x, lin, act, drop_p)


def _v4_classifier(cl, fused, p, training):
    from . import small_autograd as sa
    h = _mlp_bn_act(fused, cl[0], cl[1], "gelu", p, training)
    h = _mlp_bn_act(h, cl[4], cl[5], "gelu", p, training)
    return sa.linear(h, cl[8])


def trimodal_v4_forward(m, erp, pw, conn):
    """EnhancedTriModalFusionNetV4.forward (crossmodal_v4_enhancements.py:338-388)
    -> (logits, fusion weights (B, 3), fused (B, H))"""
    _need_gpu(erp, pw, conn)
    from . import small_autograd as sa
    tr, p = m.training, m.drop_p
    e = m.erp_encoder(erp)
    w = m.pw_encoder(pw)
    c = conn.reshape(conn.size(0), -1) if conn.dim() > 2 else conn
    ce = m.conn_encoder
    c = _mlp_bn_act(c, ce[0], ce[1], "gelu", p, tr)
    c = _mlp_bn_act(c, ce[4], ce[5], "gelu", p, tr)
    enh, _ = sa.mha_1xk(m.cross_attn, [e, w, c], tr)
    fused, weights = learned_fusion(m.fusion, [enh, w, c], tr)
    return _v4_classifier(m.classifier, fused, p, tr), weights, fused


def bidirectional_cross_attention_forward(m, e, w):
    """BiDirectionalCrossAttention.forward (crossmodal_v4_enhancements.py:436-466)"""
    _need_gpu(e, w)
    from . import small_autograd as sa
    tr = m.training
    p = m.dropout.p if tr else 0.0
    ea, _ = sa.mha_1xk(m.erp_to_pw_attn, [e, w], tr)
    wa, _ = sa.mha_1xk(m.pw_to_erp_attn, [w, e], tr)       # softmax over the same two keys: order is immaterial

    def gated(feat, att, gate, norm):
        # (attribution: the gate reads the feature with its tape, so d / d input holds every path of the reference)
        g = sa.linear(torch.cat([feat.float() if attribution_active() else _f32c(feat), att], dim=1), gate[0], "sigmoid")
        upd = sa.ActFn.apply(sa.MulFn.apply(g, att), "none", p)
        return sa.LayerNormFn.apply(sa.AddFn.apply(feat, upd), norm.weight, norm.bias, norm.eps)
    return gated(e, ea, m.erp_gate, m.norm_erp), gated(w, wa, m.pw_gate, m.norm_pw)


def smart_fusion_v4_forward(m, erp, pw):
    """EnhancedSmartFusionNetV4.forward (crossmodal_v4_enhancements.py:537-570)"""
    _need_gpu(erp, pw)
    e = m.erp_encoder(erp)
    w = m.pw_encoder(pw)
    if m.use_cross_attention:
        e, w = m.cross_attention(e, w)
    fused, weights = learned_fusion(m.fusion, [e, w], m.training)
    return _v4_classifier(m.classifier, fused, m.drop_p, m.training), weights, fused


def fmri_mlp_forward(seq, x, drop_p, training):
    """Linear-BN-ReLU-Drop x2 (fmri_utils.py:26-35); eval-mode BN is folded."""
    _need_gpu(x)
    if training:
        from . import small_autograd as sa
        h = sa.linear_bn_act(x, seq[0], seq[1], "relu", drop_p)
        return sa.linear_bn_act(h, seq[4], seq[5], "relu", drop_p)
    h, _ = small_linear(_f32c(x), seq[0], act="relu", bn=seq[1])
    h, _ = small_linear(h, seq[4], act="relu", bn=seq[5])
    return h


def fmri_single_forward(m, x):
    """fMRIActivationOnly / fMRIConnectivityOnly (run_fmri_v11.py:311-370): encoder MLP -> Linear-ReLU-Dropout-Linear."""
    _need_gpu(x)
    if m.training:
        from . import small_autograd as sa
        p = m.drop_p
        feat = fmri_mlp_forward(m.encoder.encoder, x, p, True)
        return sa.linear(sa.linear(feat, m.head[0], "relu", p), m.head[3])
    with torch.no_grad():
        feat = fmri_mlp_forward(m.encoder.encoder, x, 0.0, False)
        h, _ = small_linear(feat, m.head[0], act="relu")
        out, _ = small_linear(h, m.head[3])
    return out


def fmri_fusion_forward(m, activation, connectivity):
    _need_gpu(activation, connectivity)
    if m.training:
        from . import small_autograd as sa
        p = m.drop_p
        a = fmri_mlp_forward(m.activation_encoder.encoder, activation, p, True)
        c = fmri_mlp_forward(m.connectivity_encoder.encoder, connectivity, p, True)
        comb = sa.Softmax2ConcatFn.apply(a, c, m.activation_weight, m.connectivity_weight)
        fused = sa.linear_bn_act(comb, m.fusion[0], m.fusion[1], "relu", p)
        return sa.linear(sa.linear(fused, m.head[0], "relu", p), m.head[3]), fused
    with torch.no_grad():
        a = fmri_mlp_forward(m.activation_encoder.encoder, activation, 0.0, False)
        c = fmri_mlp_forward(m.connectivity_encoder.encoder, connectivity, 0.0, False)
        B, H = a.shape
        comb = _empty((B, 2 * H), _F32, a)
        _hip.call("mm_softmax2_concat", a, c, _f32c(m.activation_weight), _f32c(m.connectivity_weight), comb, B, H, H)
        fused, _ = small_linear(comb, m.fusion[0], act="relu", bn=m.fusion[1])
        h, _ = small_linear(fused, m.head[0], act="relu")
        out, _ = small_linear(h, m.head[3])
    return out, fused


# ------------------------------------------- tabular fMRI encoder (fp32, csrc/fmri_tab.hip: one launch each way)
def fmri_tab_check(m, shape, training: bool, who: str = "fMRITabularEncoder"):
    """the input of an `fMRITabularEncoder`, checked before any launch: (B, activation_dim + connectivity_dim); train mode
    (batch statistics) 2 <= B <= 256 - B = 1 has no variance, as torch says, and one workgroup holds a feature's whole
    batch - eval mode any B >= 1"""
    if len(shape) != 2 or shape[1] != m.in_dim:
        raise ValueError(f"{who}: expected a (B, {m.in_dim}) batch [activation ({m.activation_dim}) | connectivity "
                         f"({m.connectivity_dim})], got shape {tuple(shape)}")
    B = shape[0]
    if training and not 2 <= B <= m.MAX_TRAIN_BATCH:
        raise ValueError(f"{who}: train mode (batch statistics) takes 2 <= B <= {m.MAX_TRAIN_BATCH} rows, got {B}")
    if B < 1:
        raise ValueError(f"{who}: empty batch")


def fmri_tab_save_floats(B: int, H: int) -> int:
    """floats of mm_fmri_tab_fwd's save buffer (include/mmeeg_hip.h)"""
    return 13 * B * H + 14 * H


def fmri_tab_scratch_floats(B: int, A: int, C: int, H: int) -> int:
    """floats of mm_fmri_tab_bwd's scratch: 4 B H per workgroup"""
    return ((A + 63) // 64 + (C + 63) // 64 + 3) * 4 * B * H


def _tab_forward_impl(m, x: torch.Tensor, training: bool, save=None, need_dx: bool = False):
    """`fMRITabularEncoder` forward, ONE launch (mm_fmri_tab_fwd).  ``training`` False = frozen BatchNorm (running
    statistics, no dropout, nothing updated).  What a backward needs is always kept (13 B H + 14 H floats; ``save`` is accepted
    for symmetry with the other encoders).  Train mode draws five dropout seeds, in layer order.  -> (fused (B, H), saved)"""
    fmri_tab_check(m, x.shape, training)
    x = x.float().contiguous()
    B, A, C, H = x.shape[0], m.activation_dim, m.connectivity_dim, m.hidden_dim
    p = float(m.drop_p) if training else 0.0
    seeds = tuple(_next_seed() for _ in range(5)) if p > 0 else (0,) * 5
    out = _empty((B, H), _F32, x)
    sv = _empty((fmri_tab_save_floats(B, H),), _F32, x)
    layers = m.layers()
    bn0 = layers[0][1]
    args = []
    for lin, bn in layers:
        assert bn.eps == bn0.eps and bn.momentum == bn0.momentum
        args += [lin.weight, lin.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked]
    _hip.call("mm_fmri_tab_fwd", x, B, A, C, H, *args, m.activation_weight, m.connectivity_weight, out, sv,
              m.tickets(x.device), int(training), float(bn0.eps), float(bn0.momentum), p, *seeds, EP())
    return out, dict(enc=m, x=x, out=out, save=sv, B=B, train=bool(training), p=p, seeds=seeds, need_dx=need_dx,
                     eps=float(bn0.eps))


def fmri_tab_forward(m, x: torch.Tensor) -> torch.Tensor:
    fmri_tab_check(m, x.shape, m.training)
    _need_gpu(x)
    if m.training or attribution_active() or _wants_grad(m, x):    # (eval mode on the tape: frozen BatchNorm, no dropout)
        from .autograd import FmriTabFn
        return FmriTabFn.run(m, x)
    with torch.no_grad():
        return _tab_forward_impl(m, x, False)[0]


# ------------------ the fMRI notebook's transformer encoders (fp32, csrc/fmri_tx.hip: one launch forward, two backward)
TAB_TX_HIDDEN_DIMS = (32, 64, 128)
TAB_TX_MAX_LAYERS = 8
TAB_TX_ROW_TILE = 16          # rows a workgroup of mm_tab_tx_fwd owns
_TX_LAYER_PARAMS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                    "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias",
                    "norm2.weight", "norm2.bias")


def tab_tx_check(hidden_dim: int, num_layers: int, in_dims=(), dropout: float = 0.0, nhead: int = 4, who: str = "tab_tx"):
    """what mm_tab_tx_fwd / mm_tab_tx_bwd take, checked before any launch; names the offending argument"""
    if hidden_dim not in TAB_TX_HIDDEN_DIMS:
        raise ValueError(f"{who}: hidden_dim must be one of {TAB_TX_HIDDEN_DIMS}, got {hidden_dim}")
    if not 1 <= int(num_layers) <= TAB_TX_MAX_LAYERS:
        raise ValueError(f"{who}: num_layers must be in 1..{TAB_TX_MAX_LAYERS}, got {num_layers}")
    if len(in_dims) > 2:
        raise ValueError(f"{who}: one or two stacks, got {len(in_dims)}")
    for d in in_dims:
        if int(d) < 1:
            raise ValueError(f"{who}: in_dim must be >= 1, got {d}")
    if not 0.0 <= float(dropout) < 1.0:
        raise ValueError(f"{who}: dropout must be in [0, 1), got {dropout}")
    if nhead != 4:
        raise ValueError(f"{who}: nhead must be 4 (the notebook's encoder layers), got {nhead}")


def tab_tx_save_floats(nstacks: int, B: int, H: int, L: int) -> int:
    """floats of mm_tab_tx_fwd's save buffer (include/mmeeg_hip.h)"""
    return nstacks * (1 + 9 * L) * B * H


def tab_tx_scratch_floats(nstacks: int, B: int, H: int, L: int) -> int:
    """floats of mm_tab_tx_bwd's scratch"""
    return nstacks * (3 + 11 * L) * B * H


def tab_tx_params(enc) -> List[torch.Tensor]:
    """an encoder's 4 + 12 L parameters in the kernels' order (= its parameters() order)"""
    ps = [enc.project.weight, enc.project.bias]
    for layer in enc.transformer.layers:
        named = dict(layer.named_parameters())
        ps += [named[k] for k in _TX_LAYER_PARAMS]
    return ps + [enc.norm.weight, enc.norm.bias]


def host_table(values, ctype):
    """a host array the C ABI reads during the call (pointer tables, seed lists): keep the returned object alive until the
    call has returned"""
    import ctypes
    return (ctype * max(len(values), 1))(*values)


def tab_tx_forward_impl(encs, xs, training: bool, save: bool):
    """one or two notebook encoders (``crossmodal_fmri_scr.ActivationEncoder`` / ``ConnectivityEncoder``) on their inputs
    (B, in_dim), ONE launch (mm_tab_tx_fwd).  Train mode draws 4 L dropout seeds per stack (layer order, then attention,
    dropout1, FFN middle, dropout2), stack by stack.  ``save`` False: nothing but the outputs is written.
    -> ([feat (B, H)], saved)"""
    import ctypes
    n = len(encs)
    e0 = encs[0]
    H, L = e0.hidden_dim, e0.num_layers
    tab_tx_check(H, L, [e.in_dim for e in encs], e0.drop_p, who="tab_tx_forward")
    for e, x in zip(encs, xs):
        if (e.hidden_dim, e.num_layers, e.drop_p) != (H, L, e0.drop_p):
            raise ValueError("tab_tx_forward: the stacks of one launch share hidden_dim, num_layers and dropout")
        if x.dim() != 2 or x.shape[1] != e.in_dim or x.shape[0] != xs[0].shape[0] or x.shape[0] < 1:
            raise ValueError(f"tab_tx_forward: expected a (B, {e.in_dim}) batch with B >= 1 rows in every stack, got shape "
                             f"{tuple(x.shape)}")
    _need_gpu(*xs)
    xs = [x.float().contiguous() for x in xs]
    B = xs[0].shape[0]
    p = float(e0.drop_p) if training else 0.0
    seeds = [_next_seed() for _ in range(n * 4 * L)] if p > 0 else []
    params = [q for e in encs for q in tab_tx_params(e)]
    ptab = host_table([_hip._ptr(q) for q in params], ctypes.c_void_p)
    stab = host_table(seeds, ctypes.c_uint32)
    outs = [_empty((B, H), _F32, xs[0]) for _ in range(n)]
    sv = _empty((tab_tx_save_floats(n, B, H, L),), _F32, xs[0]) if save else None
    _hip.call("mm_tab_tx_fwd", xs[0], xs[1] if n > 1 else None, n, B, encs[0].in_dim, encs[1].in_dim if n > 1 else 0, H, L,
              ctypes.addressof(ptab), outs[0], outs[1] if n > 1 else None, sv, p, ctypes.addressof(stab) if seeds else None, EP())
    return outs, dict(encs=list(encs), xs=xs, save=sv, B=B, H=H, L=L, p=p, seeds=seeds, params=params)


def conn_encoder_forward(m, x):
    _need_gpu(x)
    if m.training or attribution_active():                   # (attribution: eval mode on the tape - frozen BatchNorm, no dropout)
        from . import small_autograd as sa
        p, fz = (m.drop_p, False) if m.training else (0.0, True)
        h = sa.linear_bn_act(x, m.proj1[0], m.proj1[1], "gelu", p, frozen=fz)
        h = sa.linear_bn_act(h, m.proj2[0], m.proj2[1], "gelu", p, frozen=fz)
        gate = sa.linear(sa.linear(h, m.attention[0], "tanh"), m.attention[2], "sigmoid")
        return sa.linear_bn_act(sa.MulFn.apply(h, gate), m.output[0], m.output[1], "gelu", p, frozen=fz)
    with torch.no_grad():
        h, _ = small_linear(_f32c(x), m.proj1[0], act="gelu", bn=m.proj1[1])
        h, _ = small_linear(h, m.proj2[0], act="gelu", bn=m.proj2[1])
        t, _ = small_linear(h, m.attention[0], act="tanh")
        g, _ = small_linear(t, m.attention[2], act="sigmoid")
        hg = torch.empty_like(h)
        _hip.call("mm_mul_f32", h, g, hg, h.numel())
        out, _ = small_linear(hg, m.output[0], act="gelu", bn=m.output[1])
    return out


# ------------------------------------------------- GATv2 over one static graph (csrc/gnn.hip)
class GatGraph:
    """the graph ``mm_gatv2_fwd`` / ``mm_gatv2_bwd`` read, int32 on the device of the ``edge_index`` it came from:
    CSR by target (``rowptr`` (N + 1), ``col`` (E') = source) and the CSC view of the same edges (``colptr`` (N + 1),
    ``row`` (E') = target, ``perm`` (E') = CSR position; CSR order within a source).

    For edge attributes, whose rows come aligned with the listed ``edge_index`` (``mm_gatv2_edge_pack`` / ``_pack_bwd``):
    ``eid`` (E') = listed edge of each CSR position, -1 for an appended self-loop; ``indeg`` (N) = in-degree without
    loops; ``pos`` (E) = CSR position of each listed edge, -1 for a dropped self-loop; ``tgt`` (E) = its target.
    For attention output in torch_geometric's edge order (the listed non-loop edges, then the N self-loops):
    ``attn_edge_index`` (2, E') int64 and ``attn_pos`` (E') int64 = the CSR position of each of those edges."""

    def __init__(self, num_nodes, rowptr, col, colptr, row, perm, eid=None, indeg=None, pos=None, tgt=None,
                 attn_edge_index=None, attn_pos=None):
        self.num_nodes, self.num_edges = int(num_nodes), int(col.numel())
        self.rowptr, self.col, self.colptr, self.row, self.perm = rowptr, col, colptr, row, perm
        self.eid, self.indeg, self.pos, self.tgt = eid, indeg, pos, tgt
        self.num_listed = None if pos is None else int(pos.numel())
        self.attn_edge_index, self.attn_pos = attn_edge_index, attn_pos


def _build_gat_graph(edge_index: torch.Tensor, num_nodes: int) -> GatGraph:
    N = int(num_nodes)
    if N < 1:
        raise ValueError(f"gat_graph: num_nodes={num_nodes}")
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError(f"gat_graph: edge_index must be (2, E), got {tuple(edge_index.shape)}")
    if edge_index.is_floating_point() or edge_index.dtype == torch.bool:
        raise ValueError(f"gat_graph: edge_index must hold integers, got {edge_index.dtype}")
    ei = edge_index.detach().to("cpu", torch.int64)
    if ei.numel() and (int(ei.min()) < 0 or int(ei.max()) >= N):
        raise ValueError(f"gat_graph: edge_index must lie in [0, {N}), got [{int(ei.min())}, {int(ei.max())}]")
    # GATv2Conv(add_self_loops=True): listed self-loops go, one per node is appended; duplicates stay
    keep = ei[0] != ei[1]
    loops = torch.arange(N, dtype=torch.int64)
    src = torch.cat([ei[0][keep], loops])
    dst = torch.cat([ei[1][keep], loops])
    order = torch.sort(dst, stable=True).indices                    # CSR by target, listed order within a target
    col, tgt = src[order], dst[order]
    perm = torch.sort(col, stable=True).indices                     # CSC: by source, CSR order within a source

    def ptr(keys):
        out = torch.zeros(N + 1, dtype=torch.int64)
        out[1:] = torch.cumsum(torch.bincount(keys, minlength=N), 0)
        return out
    # edge attributes: listed rows <-> CSR positions
    kept = keep.nonzero().flatten()
    eid = torch.cat([kept, torch.full((N,), -1, dtype=torch.int64)])[order]
    inv = torch.empty_like(order)
    inv[order] = torch.arange(order.numel())                        # [listed non-loop edges, then loops] -> CSR position
    pos = torch.full((ei.size(1),), -1, dtype=torch.int64)
    pos[kept] = inv[:kept.numel()]
    indeg = torch.bincount(ei[1][keep], minlength=N)
    dev = edge_index.device
    i32 = [t.to(torch.int32).contiguous().to(dev) for t in (ptr(tgt), col, ptr(col), tgt[perm], perm, eid, indeg, pos, ei[1])]
    return GatGraph(N, *i32, attn_edge_index=torch.stack([src, dst]).to(dev), attn_pos=inv.to(dev))


def gat_graph(edge_index: torch.Tensor, num_nodes: int) -> GatGraph:
    """``GatGraph`` of ``edge_index`` (2, E) = [source; target] with GATv2Conv's self-loop rule, built once per
    ``edge_index`` tensor (and again only after an in-place change of it).  ValueError for a malformed graph."""
    key = (int(num_nodes), edge_index._version)
    hit = getattr(edge_index, "_mm_gat_graph", None)
    if hit is not None and hit[0] == key:
        return hit[1]
    g = _build_gat_graph(edge_index, num_nodes)
    edge_index._mm_gat_graph = (key, g)
    return g


def _gat_cat(conv):
    """W_l | W_r stacked, so that both linear images of the node features come from one launch"""
    W = torch.cat([conv.lin_l.weight, conv.lin_r.weight], dim=0)
    b = torch.cat([conv.lin_l.bias, conv.lin_r.bias], dim=0) if conv.lin_l.bias is not None else None
    return W, b


def _gat_edge_args(w_edge, ea_csr):
    """what an ``mm_gatv2_edge_*`` call takes beyond its plain twin: ((w_edge, edge_attr, ea_batched), (D,)); a plain
    layer (``ea_csr`` None): ((), ())"""
    return ((), ()) if ea_csr is None else ((w_edge, ea_csr, int(ea_csr.size(0) != 1)), (ea_csr.size(2),))


def _fill_args(fill_value):
    """(fill_mean, constant) of GATv2EdgeConv's ``fill_value``: 'mean' or a number"""
    if isinstance(fill_value, str):
        if fill_value != "mean":
            raise ValueError(f"GATv2EdgeConv: fill_value must be 'mean' or a number, got '{fill_value}'")
        return 1, 0.0
    if isinstance(fill_value, bool) or not isinstance(fill_value, (int, float)):
        raise ValueError(f"GATv2EdgeConv: fill_value must be 'mean' or a number, got {fill_value!r}")
    return 0, float(fill_value)


def gat_edge_attr(edge_attr, graph: GatGraph, B: int, edge_dim: int) -> torch.Tensor:
    """``edge_attr`` (E,), (E, D) [shared by the batch] or (B, E, D) [per sample], rows aligned with the listed
    ``edge_index`` -> (1 | B, E, D).  ValueError, before any launch, for a missing tensor, D outside 1..8 or not the
    layer's ``edge_dim``, another E than the graph lists or another B than ``x`` has."""
    if edge_attr is None:
        raise ValueError(f"GATv2EdgeConv: this layer has edge_dim={edge_dim}, edge_attr is required")
    if not torch.is_tensor(edge_attr) or not edge_attr.is_floating_point() or edge_attr.dim() not in (1, 2, 3):
        raise ValueError("GATv2EdgeConv: edge_attr must be a floating-point (E,), (E, D) or (B, E, D) tensor")
    ea = edge_attr.reshape(1, -1, 1) if edge_attr.dim() == 1 else edge_attr.unsqueeze(0) if edge_attr.dim() == 2 else edge_attr
    Bo, El, D = ea.shape
    if not 1 <= D <= 8:
        raise ValueError(f"GATv2EdgeConv: edge_attr has D={D} features per edge, supported 1..8")
    if D != edge_dim:
        raise ValueError(f"GATv2EdgeConv: edge_attr has D={D} features per edge, the layer edge_dim={edge_dim}")
    if El != graph.num_listed:
        raise ValueError(f"GATv2EdgeConv: edge_attr has {El} rows, edge_index lists {graph.num_listed} edges")
    if edge_attr.dim() == 3 and Bo != B:
        raise ValueError(f"GATv2EdgeConv: edge_attr is for a batch of {Bo}, x for a batch of {B}")
    return ea


def gat_edge_pack(ea: torch.Tensor, graph: GatGraph, fill_value="mean") -> torch.Tensor:
    """listed attributes (1 | B, E, D) -> CSR order with the self-loop rows filled (1 | B, E', D): ``mm_gatv2_edge_pack``"""
    fill_mean, fill = _fill_args(fill_value)
    _need_gpu(ea, graph.col)
    ea = _f32c(ea)
    Bo, El, D = ea.shape
    csr = _empty((Bo, graph.num_edges, D), _F32, ea)
    _hip.call("mm_gatv2_edge_pack", ea if El else None, graph.eid, graph.rowptr, graph.indeg, csr, Bo, graph.num_nodes,
              El, graph.num_edges, D, fill_mean, fill)
    return csr


def gatv2_forward(conv, x: torch.Tensor, graph: GatGraph, act: str = "none", ea_csr=None, sink=None) -> torch.Tensor:
    """inference path of one GATv2Conv / GATv2EdgeConv layer: x (B, N, in) fp32 -> act(out) (B, N, heads * out_channels).
    ``ea_csr`` (1 | B, E', D): the packed edge attributes of an edge layer; ``sink``: a list that receives the
    softmax alpha (B, H, E'), CSR order."""
    if (ea_csr is None) != (getattr(conv, "edge_dim", None) is None):
        raise ValueError("gatv2_forward: packed edge attributes go with an edge layer (GATv2EdgeConv), and only with one")
    _need_gpu(x, graph.col)
    B, N, F = x.shape
    if N != graph.num_nodes:
        raise ValueError(f"gatv2_forward: x has {N} nodes, the graph {graph.num_nodes}")
    H, C = conv.heads, conv.out_channels
    with torch.no_grad():
        W, b = _gat_cat(conv)
        xlr, _ = small_linear(_f32c(x).view(B * N, F), None, weight=W, bias=b)
        out = _empty((B, N, H * C), _F32, x)
        alpha = _empty((B, H, graph.num_edges), _F32, x)
        att, bias = _f32c(conv.att), None if conv.bias is None else _f32c(conv.bias)
        edge, D = _gat_edge_args(None if ea_csr is None else _f32c(conv.lin_edge.weight), ea_csr)
        _hip.call("mm_gatv2_edge_fwd" if edge else "mm_gatv2_fwd", xlr, xlr.data_ptr() + 4 * H * C, 2 * H * C, att, bias,
                  *edge, graph.rowptr, graph.col, out, None, alpha, B, N, H, C, graph.num_edges, *D,
                  float(conv.negative_slope), ACT[act], 0.0, 0, None)
    if sink is not None:
        sink.append(alpha)
    return out


def gat_attention_output(graph: GatGraph, alpha: torch.Tensor):
    """the softmax alpha (B, H, E') of a layer, CSR order -> (edge_index' (2, E'), alpha (B, E', H)) in torch_geometric's
    edge order: the listed non-loop edges in listed order, then the N self-loops.  Output formatting: an index copy."""
    return graph.attn_edge_index, alpha.detach().permute(0, 2, 1)[:, graph.attn_pos].contiguous()


def gatv2_conv_forward(conv, x, edge_index, edge_attr=None, return_attention_weights=None):
    """GATv2Conv / GATv2EdgeConv.forward: x (N, in) or (B, N, in) -> (N, H*C) / (B, N, H*C); the autograd path in train
    mode and whenever a gradient can be asked for (an input or a parameter requires one), the inference path
    otherwise.  With ``return_attention_weights`` -> (out, (edge_index', alpha (E', H) / (B, E', H)))."""
    if x.dim() not in (2, 3):
        raise ValueError(f"GATv2Conv: x must be (N, in) or (B, N, in), got {tuple(x.shape)}")
    x3 = x.unsqueeze(0) if x.dim() == 2 else x
    graph = gat_graph(edge_index, x3.size(1))
    edge_dim = getattr(conv, "edge_dim", None)
    ea = None
    if edge_dim is not None:                                    # refusals first: they need no GPU
        ea = gat_edge_attr(edge_attr, graph, x3.size(0), edge_dim)
        _fill_args(conv.fill_value)
    _need_gpu(x, edge_index, ea)
    sink = [] if return_attention_weights else None
    tape = conv.training or (torch.is_grad_enabled() and (x.requires_grad or (ea is not None and ea.requires_grad)
                                                          or any(q.requires_grad for q in conv.parameters())))
    if tape:
        from . import small_autograd as sa
        ea_csr = None if ea is None else sa.gat_edge_pack(ea, graph, conv.fill_value)
        out = sa.gatv2(conv, x3, graph, "none", conv.training, sink=sink, ea_csr=ea_csr)
    else:
        out = gatv2_forward(conv, x3, graph, ea_csr=None if ea is None else gat_edge_pack(ea, graph, conv.fill_value), sink=sink)
    out = out.squeeze(0) if x.dim() == 2 else out
    if not return_attention_weights:
        return out
    ei, alpha = gat_attention_output(graph, sink[0])
    return out, (ei, alpha.squeeze(0) if x.dim() == 2 else alpha)


def gnn_conn_encoder_forward(m, x, edge_index, edge_attr=None, attn_sink=None):
    """GNNConnectivityEncoder.forward (enhanced_models_v4.py:367-413): node_proj per node row -> GATv2 + GELU layers ->
    mean over nodes -> output_proj.  The reference applies node_proj sample by sample, so in train mode its
    BatchNorm1d takes statistics over the N nodes of ONE sample and updates the running statistics B times in
    sequence: kept, as a loop over samples (the GAT layers run the whole batch per launch).
    With ``edge_dim``: the layers take ``edge_attr``, or - without one - every sample's own connectivity
    ea[b, e, :] = x[b, source e, target e, :] (plain indexing: on the tape the gradient reaches ``x`` through it too).
    ``attn_sink``: a list that receives every layer's softmax alpha (B, H, E'), CSR order."""
    B, N = x.size(0), m.num_nodes
    graph = gat_graph(edge_index, N)
    edge_dim = getattr(m, "edge_dim", None)
    ea = None
    if edge_dim is not None:
        if edge_attr is None:
            if x.dim() != 4 or tuple(x.shape[1:]) != (N, N, edge_dim):
                raise ValueError(f"GNNConnectivityEncoder: edge features from the connectivity itself need x of shape "
                                 f"(B, {N}, {N}, {edge_dim}) [edge_dim == connectivity types], got {tuple(x.shape)}")
            edge_attr = x[:, edge_index[0], edge_index[1], :]
        ea = gat_edge_attr(edge_attr, graph, B, edge_dim)
    elif edge_attr is not None:
        raise ValueError("GNNConnectivityEncoder: edge_attr needs an encoder built with edge_dim")
    _need_gpu(x, edge_index, ea)
    x = x.reshape(B, N, -1)
    lin, bn = m.node_proj[0], m.node_proj[1]
    if m.training or attribution_active() or (torch.is_grad_enabled() and (x.requires_grad or (ea is not None and ea.requires_grad))):
        from . import small_autograd as sa
        p, fz = (m.drop_p, False) if m.training else (0.0, True)   # eval on the tape: frozen BatchNorm, no dropout
        if m.training:
            h = torch.stack([sa.linear_bn_act(x[i], lin, bn, "gelu", p) for i in range(B)], dim=0)
        else:
            h = sa.linear_bn_act(x.reshape(B * N, -1), lin, bn, "gelu", 0.0, frozen=True).view(B, N, -1)
        ea_csr = None if ea is None else sa.gat_edge_pack(ea, graph, "mean")          # once, for every layer
        for conv in m.gat_layers:
            h = sa.gatv2(conv, h, graph, "gelu", m.training, sink=attn_sink, ea_csr=ea_csr)
        return sa.linear_bn_act(sa.MeanRowsFn.apply(h), m.output_proj[0], m.output_proj[1], "gelu", p, frozen=fz)
    with torch.no_grad():
        h, _ = small_linear(_f32c(x).view(B * N, -1), lin, act="gelu", bn=bn)
        h = h.view(B, N, -1)
        ea_csr = None if ea is None else gat_edge_pack(ea, graph, "mean")
        for conv in m.gat_layers:
            h = gatv2_forward(conv, h, graph, "gelu", ea_csr=ea_csr, sink=attn_sink)
        pooled = _empty((B, h.shape[2]), _F32, h)
        _hip.call("mm_meanpool_fwd", h, pooled, None, B, N, h.shape[2])
        out, _ = small_linear(pooled, m.output_proj[0], act="gelu", bn=m.output_proj[1])
    return out


def trimodal_forward(m, erp, pw, conn):
    """EnhancedTriModalFusionNet.forward (enhanced_models_v4.py:590-657) -> (logits, fusion weights (B, 3), fused (B, H))"""
    _need_gpu(erp, pw, conn)
    from . import small_autograd as sa
    tr, p = m.training, m.drop_p
    e = m.erp_encoder(erp)
    w = m.pw_encoder(pw)
    if m.use_gnn:
        if m.edge_index is None:                                 # the graph comes from the first batch's first sample (:614-624)
            c0 = conn.detach()
            cm = c0[0, :, :, 0] if c0.dim() == 4 else c0[0].reshape(c0.size(1), c0.size(1))
            m.edge_index = m.conn_encoder.create_graph_from_connectivity(cm.unsqueeze(0))[0].to(conn.device)
        c = m.conn_encoder(conn, m.edge_index)
    else:
        ce = m.conn_encoder
        c = _mlp_bn_act(conn.reshape(conn.size(0), -1), ce[0], ce[1], "gelu", p, tr)
        c = _mlp_bn_act(c, ce[4], ce[5], "gelu", p, tr)
    tape = torch.is_grad_enabled() and any(t.requires_grad for t in (e, w, c))
    enh, _ = sa.mha_1xk(m.cross_attn, [e, w, c], tr)
    fused, weights = learned_fusion(m.fusion, [enh, w, c], tr, autograd=tape)
    return _v4_classifier(m.classifier, fused, p, tr), weights, fused


def hybrid_fusion_forward(m, erp, pw, conn):
    _need_gpu(erp, pw, conn)
    if m.training or attribution_active():
        from . import small_autograd as sa
        p, fz = (m.drop_p, False) if m.training else (0.0, True)
        g = sa.linear(sa.linear(torch.cat([erp, pw], dim=1), m.erp_pw_gate[0], "gelu", p), m.erp_pw_gate[3])
        comb, gate = sa.Gate2MixFn.apply(g, erp, pw, conn, float(m.conn_boost))
        return sa.linear_bn_act(comb, m.late_fusion[0], m.late_fusion[1], "gelu", p, frozen=fz), gate
    with torch.no_grad():
        e, p, c = _f32c(erp), _f32c(pw), _f32c(conn)
        B, H = e.shape
        g1, _ = small_linear(torch.cat([e, p], dim=1), m.erp_pw_gate[0], act="gelu")
        g2, _ = small_linear(g1, m.erp_pw_gate[3])
        comb = _empty((B, 2 * H), _F32, e)
        gate = _empty((B, 2), _F32, e)
        _hip.call("mm_gate2_mix", g2, e, p, c, comb, gate, B, H, float(m.conn_boost))
        fused, _ = small_linear(comb, m.late_fusion[0], act="gelu", bn=m.late_fusion[1])
    return fused, gate


def bn_classifier_forward(seq, fused, drop_p, training):
    """Linear-BN-GELU-Drop-Linear (crossmodal_v4_enhancements.py:909-915)."""
    _need_gpu(fused)
    if training:
        from . import small_autograd as sa
        return sa.linear(sa.linear_bn_act(fused, seq[0], seq[1], "gelu", drop_p), seq[4])
    if torch.is_grad_enabled() and (fused.requires_grad or seq[0].weight.requires_grad):
        from . import small_autograd as sa                   # eval + backward: frozen BatchNorm, dropout off
        return sa.linear(sa.linear_bn_act(fused, seq[0], seq[1], "gelu", 0.0, frozen=True), seq[4])
    with torch.no_grad():
        h, _ = small_linear(_f32c(fused), seq[0], act="gelu", bn=seq[1])
        out, _ = small_linear(h, seq[4])
    return out


def lite_encoder_forward(m, x):
    """LiteERPEncoder / LitePowerEncoder (crossmodal_v4_enhancements.py:817-877)."""
    _need_gpu(x)
    if m.training or attribution_active():
        from . import small_autograd as sa
        pooled = sa.LiteConvFn.apply(m, x, *list(m.conv_layers.parameters()))
        return sa.linear(pooled, m.output[1], "gelu", m.drop_p if m.training else 0.0)
    with torch.no_grad():
        cl = m.conv_layers
        xb = pack_nct(x.float())
        r, _ = conv_bn_act(xb, cl[0], cl[1], pool=2, training=False)
        r, _ = conv_bn_act(r["bf16"], cl[5], cl[6], training=False)
        h = r["bf16"]
        B, T, N = h.shape
        pooled = _empty((B, N), _F32, h)
        _hip.call("mm_meanpool_bf16", h, pooled, B, T, N)
        out, _ = small_linear(pooled, m.output[1], act="gelu")
    return out


# ---- the EEG notebook's single-modality baselines (crossmodal_eeg_scr.py: ERPOnlyNet / PWOnlyNet; csrc/timepool.hip)
TIMEPOOL_K = 128                 # the width the tail kernels read: the encoders' fixed third conv block
TIMEPOOL_P_MAX = 512             # projection widths served: the multiples of 16 up to this


def timepool_check(P: int, K: int, L: int, who: str = "timepool"):
    """the sizes mm_timepool_* serve, refused with ValueError before any launch"""
    if K != TIMEPOOL_K:
        raise ValueError(f"{who}: the projection reads {K} channels; the time-pool kernels serve {TIMEPOOL_K}")
    if P < 16 or P > TIMEPOOL_P_MAX or P % 16:
        raise ValueError(f"{who}: projection width {P} is not served (a multiple of 16 up to {TIMEPOOL_P_MAX})")
    if L < 1:
        raise ValueError(f"{who}: {L} time steps reach the projection (at least 1)")


def _baseline_parts(m, kind: str):
    """(encoder, its 1 x 1 projection) of a baseline net or of a stand-alone encoder"""
    if kind == "erp":
        enc = getattr(m, "erp_enc", m)
        return enc, enc.step_proj
    if kind == "pw":
        enc = getattr(m, "pw_enc", m)
        return enc, enc.proj
    raise ValueError(f"eeg baseline: kind is 'erp' or 'pw' (got {kind!r})")


def eeg_baseline_check(m, x, kind: str, head: bool = True):
    """shape rules of the baselines, before any launch.  The two MaxPool1d(2) run in the BatchNorm apply pass, which
    pools even lengths only: T % 4 == 0 (the floor MaxPool1d takes on an odd length is not served)."""
    enc, proj = _baseline_parts(m, kind)
    who = type(m).__name__
    if x is None or x.dim() != 3:
        raise ValueError(f"{who}: expected a (B, C, T) batch, got {None if x is None else tuple(x.shape)}")
    B, C, T = x.shape
    if C != enc.conv1.in_channels:
        raise ValueError(f"{who}: the batch has {C} channels, the encoder takes {enc.conv1.in_channels}")
    if T < 4 or T % 4:
        raise ValueError(f"{who}: T = {T} is not served: the two MaxPool1d(2) need T % 4 == 0 (and T >= 4)")
    if head and m.training and B < 2:
        raise ValueError(f"{who}: BatchNorm1d of the head needs at least 2 samples in train mode (got {B})")
    timepool_check(proj.out_channels, enc.conv3.out_channels, T // 4, who)


def _baseline_blocks_eval(enc, x, last_f32: bool):
    """the three Conv-BN-ReLU[-MaxPool2] blocks, BatchNorm folded into the GEMM epilogue: one launch per block"""
    r, _ = conv_bn_act(pack_nct(x.float()), enc.conv1, enc.bn1, act="relu", pool=2, training=False)
    r, _ = conv_bn_act(r["bf16"], enc.conv2, enc.bn2, act="relu", pool=2, training=False)
    r, _ = conv_bn_act(r["bf16"], enc.conv3, enc.bn3, act="relu", training=False, want_f32=last_f32, want_bf16=not last_f32)
    return r["f32" if last_f32 else "bf16"]


def timepool_max(h, proj, drop_p: float = 0.0, seed: int = 0):
    """(B, L, 128) bf16 -> (max over time of the dropped-out projection (B, P) fp32, arg-max (B, P) int32, weight image)"""
    B, L, K = h.shape
    P = proj.out_channels
    wf = weights.get(proj.weight, False)[0]
    pooled, arg = _empty((B, P), _F32, h), _empty((B, P), torch.int32, h)
    _hip.call("mm_timepool_max_fwd", h, wf, proj.bias, pooled, arg, B, L, K, P, float(drop_p), int(seed), EP())
    return pooled, arg, wf


def timepool_avg(h, proj, bins: int):
    """(B, L, 128) fp32 -> (Flatten(AdaptiveAvgPool1d(bins)(projection)) (B, P * bins), the bin means (B, bins, 128))"""
    B, L, K = h.shape
    P = proj.out_channels
    xbin, pooled = _empty((B, bins, K), _F32, h), _empty((B, P * bins), _F32, h)
    _hip.call("mm_timepool_avg_fwd", h, proj.weight.detach().reshape(P, K), proj.bias, xbin, pooled, B, L, K, P, bins)
    return pooled, xbin


def eeg_baseline_forward(m, x, kind: str):
    """ERPOnlyNet (kind "erp") / PWOnlyNet ("pw") -> logits.  Train mode: the tape with batch statistics and dropout;
    eval with a backward to follow (autograd on and something asks for a gradient, or an attribution): the same tape
    with frozen BatchNorm and dropout off; otherwise the folded eval launches, detached."""
    eeg_baseline_check(m, x, kind)
    _need_gpu(x)
    enc, proj = _baseline_parts(m, kind)
    p_head = float(m.head[4].p)
    if m.training or attribution_active() or _wants_grad(m, x):
        from . import small_autograd as sa
        fn = sa.PWOnlyFn if kind == "pw" else sa.ERPOnlyFn
        pooled = fn.apply(m, x, *list(enc.parameters()))
        return bn_classifier_forward(m.head[1:], pooled, p_head, m.training)
    with torch.no_grad():
        if kind == "pw":
            pooled = timepool_max(_baseline_blocks_eval(enc, x, False), proj)[0]
        else:
            pooled = timepool_avg(_baseline_blocks_eval(enc, x, True), proj, int(m.pool.output_size))[0]
        return bn_classifier_forward(m.head[1:], pooled, p_head, False)


def eeg_step_encoder_forward(enc, x, kind: str):
    """the notebook's ERPEncoder / PowerEncoder on their own: (B, C, T) -> (B, T / 4, out_dim) fp32, the projection as
    the taps = 1 GEMM (PowerEncoder: its dropout in the epilogue, train mode only)"""
    eeg_baseline_check(enc, x, kind, head=False)
    _need_gpu(x)
    if enc.training or attribution_active() or _wants_grad(enc, x):
        from . import small_autograd as sa
        return sa.StepEncoderFn.apply(enc, kind, x, *list(enc.parameters()))
    _, proj = _baseline_parts(enc, kind)
    with torch.no_grad():
        h = _baseline_blocks_eval(enc, x, False)
        B, L, K = h.shape
        r = linear_rows(h.view(B * L, K), proj.weight, proj.bias, out_f32=True, out_bf16=False)
        return r["f32"].view(B, L, -1)


def _power_merged(m, device):
    """the three parallel Conv1d(C->64, k in {3,5,7}) as ONE k=7 conv with 192
    outputs (shorter kernels zero-padded around the centre tap) + folded BN."""
    ws, bs, o4 = [], [], []
    for seq in (m.conv_scale1, m.conv_scale2, m.conv_scale3):
        w = seq[0].weight.detach()
        k = w.shape[2]
        ws.append(torch.nn.functional.pad(w, ((7 - k) // 2, (7 - k) // 2)))
        o4.append(bn_fold_eval(seq[1], seq[0].bias))
    return torch.cat(ws, dim=0).contiguous(), torch.cat(o4, dim=1).contiguous()


def stft_front_end(x: torch.Tensor, n_ffts, hop: int, normalize: bool = False, keep_spec: bool = False):
    """(B, C, T) fp32 -> channels-last bf16 (B, frames, Cp) multi-scale STFT power,
    channel order [scale][c][f] as torch.cat([stft_power(x, n) ...], dim=1).
    ``normalize``: z-score every sample's spectra (the reference's normalize_modality on its power
    features, run_training_lite.py:48-51, 162) in fp32 before the bf16 cast."""
    B, C, T = x.shape
    widths = [C * (n // 2 + 1) for n in n_ffts]
    total = sum(widths)
    cp = cpad(total)
    frames = T // hop + 1
    xc = x.float().contiguous()
    if normalize:
        spec = torch.zeros((B, frames, cp), dtype=_F32, device=x.device) if cp != total else _empty((B, frames, cp), _F32, x)
        out = _empty((B, frames, cp), _BF, x)
    else:
        spec = None
        out = torch.zeros((B, frames, cp), dtype=_BF, device=x.device) if cp != total else _empty((B, frames, cp), _BF, x)
    off = 0
    for n, wdt in zip(n_ffts, widths):
        _hip.call("mm_stft_power", xc, None if normalize else out, spec, B, C, T, int(n), int(hop), off, cp)
        off += wdt
    if normalize:
        _hip.call("mm_sample_zscore_bf16", spec, out, _empty((64 * B,), torch.float64, x), B, frames, total, cp, 1e-8)
    return (out, spec) if keep_spec else out


def stft_power_encoder_forward(m, x):
    """MultiScaleSTFTPowerEncoder: STFT power front-end -> EnhancedPowerEncoder.  The front-end has no parameters; when
    the raw EEG asks for a gradient it is differentiated too (autograd.StftFrontEndFn)."""
    _need_gpu(x)
    enc = m.encoder
    if enc.training or _wants_grad(enc, x):
        from .autograd import PowerEncoderFn, StftFrontEndFn
        if x.requires_grad and torch.is_grad_enabled():           # d / d raw EEG: the front-end joins the tape
            spec = StftFrontEndFn.apply(x, m.n_ffts, m.hop, m.normalize)
        else:
            with torch.no_grad():
                spec = stft_front_end(x, m.n_ffts, m.hop, m.normalize)
        return PowerEncoderFn.run(enc, spec, packed=True)
    with torch.no_grad():
        return _power_forward_ntc(enc, stft_front_end(x, m.n_ffts, m.hop, m.normalize))


def power_encoder_forward(m, x):
    """EnhancedPowerEncoder (enhanced_models_v4.py:258-285)."""
    _need_gpu(x)
    if m.training or _wants_grad(m, x):
        from .autograd import PowerEncoderFn
        return PowerEncoderFn.run(m, x)
    with torch.no_grad():
        return _power_forward_ntc(m, pack_nct(x.float()))


class _Merged:
    """attribute bag standing in for an nn.Conv1d / nn.BatchNorm1d built from several modules"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def power_merge_call(mode: int, parts, merged, tracked=(None, None, None), cin: int = 0, ks=(3, 5, 7), cinp: int = 0):
    """mm_power_merge: ``parts`` = six triples (conv weight, conv bias, BN weight, BN bias, running mean, running var) of
    fp32 tensors or None, ``merged`` = the six merged tensors or None (include/mmeeg_hip.h: mm_power_merge_t)"""
    import ctypes
    import struct
    ptr = lambda t: 0 if t is None else t.data_ptr()      # noqa: E731
    flat = [ptr(t) for trip in parts for t in trip] + [ptr(t) for t in tracked] + [ptr(t) for t in merged]
    buf = struct.pack("<27Q6i", *flat, int(cin), *[int(k) for k in ks], int(cinp), 0)
    host = ctypes.create_string_buffer(buf, len(buf))
    _hip.call("mm_power_merge", ctypes.addressof(host), int(mode))


def _power_merged_train(m, need_dgrad: bool = True):
    """the three conv scales as ONE Conv1d(C -> 192, k=7, p=3) + BatchNorm1d(192) whose tensors are
    fresh leaves (requires_grad as the parts'), so the generic conv/BN forward+backward applies;
    autograd.power_encoder_bwd adds their gradients back into the six real parameters.  Built by ONE launch
    (mm_power_merge mode 0: the pads / cats of the three branches were ~20 tiny torch launches per step).
    ``need_dgrad`` False (no gradient w.r.t. the input: the trainers): the merged weight exists only as the forward
    kernel's bf16 image (mode 3), handed to the weight cache - its fp32 tensor is a never-read placeholder."""
    seqs = (m.conv_scale1, m.conv_scale2, m.conv_scale3)
    ref = seqs[0][0].weight
    cin = seqs[0][0].in_channels
    ks = tuple(s[0].kernel_size[0] for s in seqs)
    assert all(s[0].out_channels == 64 and s[0].in_channels == cin and s[0].weight.dtype == _F32 for s in seqs), "three 64-channel branches"
    w = _empty((192, cin, 7), _F32, ref)
    vec = [_empty((192,), _F32, ref) for _ in range(5)]
    parts = ([s[0].weight.detach() for s in seqs], [s[0].bias.detach() for s in seqs], [s[1].weight.detach() for s in seqs],
             [s[1].bias.detach() for s in seqs], [s[1].running_mean for s in seqs], [s[1].running_var for s in seqs])
    if need_dgrad:
        power_merge_call(0, parts, [w] + vec, cin=cin, ks=ks)
    else:
        cinp = cpad(cin)
        wf = _empty((192, 7, cinp), _BF, ref)
        power_merge_call(3, parts, [wf] + vec, cin=cin, ks=ks, cinp=cinp)
        weights.seed(w, wf, None, cinp, cpad(192))
    w._mm_transient = True        # rebuilt every step: a trainer's recorded weight list must not hold on to this one
    conv = _Merged(weight=w.requires_grad_(any(s[0].weight.requires_grad for s in seqs)),
                   bias=vec[0].requires_grad_(any(s[0].bias.requires_grad for s in seqs)),
                   kernel_size=(7,), padding=(3,), in_channels=cin, out_channels=192,
                   parts=[(s[0].weight, 64 * i) for i, s in enumerate(seqs)])        # (real weight, its first merged output channel)
    bn = _Merged(weight=vec[1].requires_grad_(any(s[1].weight.requires_grad for s in seqs)),
                 bias=vec[2].requires_grad_(any(s[1].bias.requires_grad for s in seqs)),
                 running_mean=vec[3], running_var=vec[4],
                 num_batches_tracked=None, num_features=192, eps=seqs[0][1].eps, momentum=seqs[0][1].momentum)
    assert all(s[1].eps == bn.eps and s[1].momentum == bn.momentum for s in seqs)
    return conv, bn, seqs


def _power_forward_impl(m, xb: torch.Tensor, training: bool, need_dgrad: bool, save=None, mask=None):
    """EnhancedPowerEncoder on packed (B, T, Cp) bf16 input, train / frozen-BN forms."""
    save = training if save is None else save
    conv, bn, seqs = _power_merged_train(m, need_dgrad)
    r, s0 = conv_bn_act(xb, conv, bn, training=training, need_dgrad=need_dgrad, save=save)
    if training:                                  # running statistics live in the three real modules: handed back in one launch
        none3 = [None] * 3
        power_merge_call(1, (none3, none3, none3, none3, [sq[1].running_mean for sq in seqs], [sq[1].running_var for sq in seqs]),
                         [None, None, None, None, bn.running_mean, bn.running_var],
                         tracked=[sq[1].num_batches_tracked for sq in seqs], cin=conv.in_channels,
                         ks=[sq[0].kernel_size[0] for sq in seqs])
    T = xb.shape[1]
    p = m.drop_p if training else 0.0
    r, s1 = conv_bn_act(r["bf16"], m.fusion[0], m.fusion[1], training=training, drop_p=p,
                        pe=pe_table(m.pos_encoder, T), pe_drop_p=(m.pos_encoder.dropout.p if training else 0.0),
                        want_f32=True, want_bf16=False, need_dgrad=True, save=save)
    out, blocks, sh, h = _encoder_tail_impl(m, r["f32"], training, True, save, mask=mask)
    return out, dict(convs=[s0, s1], blocks=blocks, head=sh, merged=(conv, bn, seqs), tokens=h)


def _power_forward_ntc(m, xb):
    B, T, cp = xb.shape
    w192, o4 = _power_merged(m, xb.device)
    wf = _empty((192, 7, cp), _BF, xb)
    _hip.call("mm_prep_conv_weight", w192, wf, None, 192, w192.shape[1], 7, cp, 0)
    h = igemm(xb, wf, 7, 3, 192, scale=o4[0], shift=o4[1], act="gelu")["bf16"]
    r, _ = conv_bn_act(h, m.fusion[0], m.fusion[1], training=False, pe=pe_table(m.pos_encoder, T),
                       want_f32=True, want_bf16=False)
    tok = r["f32"]
    for blk in m.transformer_layers:
        tok, _ = transformer_block_fwd(tok, blk, False)
    out, _ = pooled_head_fwd(tok, m.output_proj[2])
    return out


def weighted_cross_entropy(logits, target, weight=None):
    """nn.CrossEntropyLoss(weight=...) on the HIP path (_test_bridge.py:858)."""
    _need_gpu(logits, target)
    from . import small_autograd as sa
    w = weight.float().contiguous() if weight is not None else None
    return sa.WeightedCEFn.apply(logits, target, w)


def focal_loss(logits, target, alpha=0.25, gamma=2.0, reduction="mean"):
    """FocalLoss of the EEG notebook (CrossModal_EEG_scr.ipynb cell 20) on the HIP path."""
    _need_gpu(logits, target)
    from . import small_autograd as sa
    return sa.FocalLossFn.apply(logits, target, float(alpha), float(gamma), reduction)


def drop_path(x, drop_prob):
    """training-mode stochastic depth (crossmodal_v4_enhancements.py:639-650) in one launch"""
    _need_gpu(x)
    from . import small_autograd as sa
    return sa.DropPathFn.apply(x, float(drop_prob))


def smoothed_cross_entropy(pred, target, smoothing):
    _need_gpu(pred, target)
    from . import small_autograd as sa
    return sa.SmoothedCEFn.apply(pred, target, float(smoothing))


# ------------------------------------------------- attribution (EEG_CODE/eeg_xai_analysis.py:88-236)
_ATTRIBUTION = {"depth": 0}


class attribution_mode:
    """context of the attribution engine: an EVAL-mode forward issued inside keeps a differentiable tape from the
    logits down to the raw inputs in the glue layers that otherwise run their no-grad eval kernels (learned fusion,
    gated cross attention, connectivity / Lite encoders, hybrid fusion): frozen BatchNorm, every dropout off.

    Why a context and not the test this file uses elsewhere (``torch.is_grad_enabled() and x.requires_grad``, as in
    `_mlp_bn_act` / `bn_classifier_forward`): at a glue layer that test cannot tell an attribution from an ordinary eval
    forward.  The encoders put their output on the tape whenever a PARAMETER asks for a gradient (`_wants_grad`), so in
    eval mode with autograd on - every evaluation not wrapped in no_grad - the features reaching the fusion layers
    already require grad.  Switching on that would move those existing calls from the fused eval kernels to the
    differentiable compositions, i.e. change what they compute today.  The context is entered in ONE place
    (`integrated_gradients`) and read in five forwards; nothing changes outside it or in train mode.
    Supported models = those whose eval forward reaches the inputs on a tape inside the context: the V4 / V4-Lite
    classifiers, the bridge net, the encoders and `BridgeTrainer`.  A model that detaches on the way (the tabular fMRI nets,
    the notebook classes) is refused by the engine - it raises when an input gets no gradient - not attributed as zero."""

    def __enter__(self):
        _ATTRIBUTION["depth"] += 1
        return self

    def __exit__(self, *exc):
        _ATTRIBUTION["depth"] -= 1
        return False


def attribution_active() -> bool:
    return _ATTRIBUTION["depth"] > 0


def xai_alphas(n_steps: int):
    """the interpolation constants of mm_xai_interp as the kernel forms them: ``np.linspace(0, 1, n_steps)`` - arange(n)
    times the fp64 step 1 / (n - 1), the last point exactly 1, a single point 0 - rounded to fp32"""
    import numpy as np
    if n_steps < 1:
        raise ValueError("xai_alphas: n_steps must be >= 1")
    if n_steps == 1:
        return np.zeros(1, dtype=np.float32)
    step = 1.0 / float(n_steps - 1)
    a = [float(s) * step for s in range(n_steps)]
    a[-1] = 1.0
    return np.asarray(a, dtype=np.float64).astype(np.float32)


XAI_BUDGET_BYTES = 2 << 30


def ig_chunk_steps(n_steps: int, step_bytes: int, budget_bytes: int = XAI_BUDGET_BYTES) -> int:
    """THE MEMORY RULE of the batched integrated-gradients engine: how many interpolation steps S_c go through the
    model as one batch of S_c * B rows.  ``step_bytes`` = the device memory ONE step needs at its peak (its B
    interpolated rows of every input, their gradients, and everything the model's tape keeps for the backward);
    eval mode has no batch statistics, so k steps need k times that.  S_c = floor(budget / step_bytes), at least 1
    (a single step always runs) and at most n_steps.  It does not depend on n_steps otherwise: 50 steps of a
    (32, 64, 1024) input are 419 MB in fp32 for that one interpolated tensor alone, before any activation.
    `integrated_gradients` measures ``step_bytes`` on its first step (alpha = 0, run on its own)."""
    if n_steps < 1 or step_bytes < 1 or budget_bytes < 1:
        raise ValueError("ig_chunk_steps: n_steps, step_bytes and budget_bytes must be positive")
    return max(1, min(int(n_steps), int(budget_bytes) // int(step_bytes)))


def ig_chunks(n_steps: int, chunk_steps: int, first_alone: bool = False):
    """[(s0, steps), ...] covering [0, n_steps) in ascending order; ``first_alone``: step 0 is its own chunk (the
    engine measures one step's memory there) and the rule's S_c applies from step 1 on"""
    out, s = [], 0
    if first_alone and n_steps > 0:
        out.append((0, 1))
        s = 1
    while s < n_steps:
        k = min(chunk_steps, n_steps - s)
        out.append((s, k))
        s += k
    return out


def _xai_base(x: torch.Tensor, base):
    """(baseline tensor or None, base_rows) for the kernels: None | (B, ...) | (1, ...) / (...) broadcast"""
    if base is None:
        return None, 0
    b = base.detach().to(x.device).float().contiguous()
    if b.numel() == x.numel():
        return b, x.shape[0]
    if b.numel() * x.shape[0] == x.numel():
        return b, 1
    raise ValueError(f"attribution baseline of shape {tuple(base.shape)} for an input of shape {tuple(x.shape)}")


def xai_interpolate(x: torch.Tensor, base, n_steps: int, s0: int, steps: int) -> torch.Tensor:
    """(steps * B, ...) fp32: rows [k * B, (k + 1) * B) = base + alpha_{s0 + k} * (x - base) (mm_xai_interp)"""
    _need_gpu(x)
    xc = x.detach().float().contiguous()
    b, rows = _xai_base(xc, base)
    B = xc.shape[0]
    out = _empty((steps * B,) + tuple(xc.shape[1:]), _F32, xc)
    _hip.call("mm_xai_interp", xc, b, rows, out, int(n_steps), int(s0), int(steps), B, xc.numel() // B)
    return out


def xai_accumulate(acc: torch.Tensor, grad: torch.Tensor, steps: int):
    """acc (B, ...) += the ``steps`` slices of grad (steps * B, ...), in ascending step order (mm_xai_accum)"""
    g = grad.detach().float().contiguous()
    if g.numel() != steps * acc.numel():
        raise ValueError(f"xai_accumulate: {steps} steps of {tuple(acc.shape)} against a gradient of {tuple(grad.shape)}")
    _hip.call("mm_xai_accum", g, acc, int(steps), acc.numel())
    return acc


XAI_MODES = {"integrated_gradients": 0, "gradient": 1, "gradient_x_input": 2}


def xai_finish(x: torch.Tensor, base, acc: torch.Tensor, n_steps: int, method: str, channels: bool = False):
    """-> (attr like x, chan (B, C) or None): mm_xai_finish.  ``channels``: x is (B, C, T) and the per-channel means
    over T are wanted as well."""
    _need_gpu(x, acc)
    xc = x.detach().float().contiguous()
    b, rows = _xai_base(xc, base)
    B = xc.shape[0]
    if channels:
        if xc.dim() != 3:
            raise ValueError("xai_finish: per-channel means need a (B, C, T) input")
        C, T = xc.shape[1], xc.shape[2]
    else:
        C, T = 1, xc.numel() // B
    attr = torch.empty_like(xc)
    chan = _empty((B, C), _F32, xc) if channels else None
    _hip.call("mm_xai_finish", xc, b, rows, acc.contiguous(), attr, chan, B, C, T, int(n_steps), XAI_MODES[method])
    return attr, chan


def xai_pair_score(z: torch.Tensor, want_seed: bool = True):
    """z (B, 2N) packed [ze | zf] -> (score (B,) = ze . zf per pair, seed (B, 2N) = [zf | ze] = d score / d z)"""
    zc = z.detach().float().contiguous()
    B, N2 = zc.shape
    score = _empty((B,), _F32, zc)
    seed = torch.empty_like(zc) if want_seed else None
    _hip.call("mm_xai_pair_score", zc, score, seed, B, N2 // 2)
    return score, seed


def _release_tape(out: torch.Tensor):
    """The module-level autograd functions keep what their backward needs as plain Python attributes of the graph node
    (``ctx.saved = ...``), the node's own output among it: node -> attribute -> output -> node, a reference cycle that
    only Python's garbage collector frees - and it does not count device bytes, so chunk after chunk of activations
    would pile up behind the engine's memory rule (15.9 GiB instead of 1.9 GiB at the C2 shape).  Once the chunk's
    backward has run the tape is dead: EVERY Python attribute of every custom node is dropped, whatever its name (built-in
    nodes have no attribute dictionary and free their saved tensors themselves)."""
    stack, seen = [out.grad_fn], set()
    while stack:
        fn = stack.pop()
        if fn is None or id(fn) in seen:
            continue
        seen.add(id(fn))
        stack.extend(n for n, _ in fn.next_functions)
        attrs = getattr(fn, "__dict__", None)
        if attrs:
            attrs.clear()


def integrated_gradients(forward, inputs, baselines, n_steps: int, seed_fn, constants=(), chunk_steps: Optional[int] = None,
                         budget_bytes: int = XAI_BUDGET_BYTES):
    """The batched integrated-gradients engine.  The reference (eeg_xai_analysis.py:196-221) runs ``n_steps``
    forward/backward passes one at a time and carries every gradient to the host; here S_c steps are interpolated
    into ONE batch of S_c * B rows (mm_xai_interp), go through ``forward`` and its backward once, and the input
    gradients are folded into one device accumulator per input (mm_xai_accum).  Eval mode has no batch statistics,
    so the rows of the big batch are independent.

    ``forward(*interpolated, *repeated_constants)`` -> the model output (S_c * B, ...) on the autograd tape;
    ``seed_fn(output detached, s0, steps)`` -> the gradient the backward starts from (same shape) - it sees the chunks
    in ascending order, the first one starting at alpha = 0 (where the reference fixes its target class);
    ``inputs`` / ``baselines``: tensors (B, ...) and None | (B, ...) | (1, ...); ``constants``: inputs that are NOT
    interpolated (the reference's connectivity features): repeated for every step, their gradient accumulated alike.
    ``chunk_steps``: S_c given by the caller; None: step 0 runs alone, its peak memory is measured, and
    `ig_chunk_steps` (the memory rule) sizes the remaining chunks - that measurement calls
    ``torch.cuda.reset_peak_memory_stats``, so the caller's peak-memory statistics of this device start over.  Parameter
    ``.grad`` fields are not touched.  An input (or constant) the output does not depend on through the tape RAISES: a model
    that detaches on the way would otherwise be attributed as all zeros.
    -> (accumulators for inputs + constants: the SUM over the steps of d output . seed / d input, chunks [(s0, steps)])."""
    inputs = [t.detach().float().contiguous() for t in inputs]
    constants = [t.detach().float().contiguous() for t in constants]
    _need_gpu(*inputs, *constants)
    if n_steps < 1:
        raise ValueError("integrated_gradients: n_steps must be >= 1")
    accs = [torch.zeros_like(t) for t in inputs + constants]
    dev = inputs[0].device
    floor = torch.cuda.memory_allocated(dev)                 # what is held before the first chunk
    probe = chunk_steps is None
    plan = ig_chunks(n_steps, 1 if probe else int(chunk_steps), first_alone=probe)
    done = []
    i = 0
    while i < len(plan):
        s0, k = plan[i]
        if probe and i == 0:
            torch.cuda.synchronize(dev)
            before = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
        xs = [xai_interpolate(x, b, n_steps, s0, k).requires_grad_(True) for x, b in zip(inputs, baselines)]
        cs = [c.repeat((k,) + (1,) * (c.dim() - 1)).requires_grad_(True) for c in constants]
        with torch.enable_grad(), attribution_mode():
            out = forward(*xs, *cs)
            seed = seed_fn(out.detach(), s0, k)
            grads = torch.autograd.grad(out, xs + cs, seed, allow_unused=True)
        missing = [i for i, g in enumerate(grads) if g is None]
        if missing:
            raise _hip.HipLibraryError(
                f"attribution: input(s) {missing} of {len(grads)} get no gradient - the model's eval-mode forward detaches "
                "before it reaches them (no differentiable HIP path for this model; see ops.attribution_mode)")
        for acc, g in zip(accs, grads):
            xai_accumulate(acc, g, k)
        _release_tape(out)
        del out, seed, grads, xs, cs
        if torch.cuda.memory_allocated(dev) - floor > budget_bytes:     # other cycles left activations behind: collect them
            import gc
            gc.collect()
        done.append((s0, k))
        if probe and i == 0:
            torch.cuda.synchronize(dev)
            step_bytes = max(1, torch.cuda.max_memory_allocated(dev) - before)
            plan = plan[:1] + [(s + 1, n) for s, n in ig_chunks(n_steps - 1, ig_chunk_steps(n_steps, step_bytes, budget_bytes))]
        i += 1
    return accs, done


# ------------------------------------------------- perturbation attribution (csrc/perturb.hip; EEG_CODE/
# CrossModal_EEG_scr.ipynb, InterpretabilityAnalyzer.compute_channel_importance)
PERTURB_KINDS = {"rows": 0, "windows": 1, "blocks": 2}


def _perturb_geometry(kind, shape, size, who: str = "perturb"):
    """-> (kind code, n0, n1, n2, n3, size, U) of mm_perturb_expand for ONE sample of ``shape``: "rows" of a (C, T)
    sample, "windows" of ``size`` along T of a (C, T) or a tabular (F,) sample, "blocks" of ``size``^3 of a
    (Cv, D, H, W) volume.  ValueError for anything else."""
    code = PERTURB_KINDS.get(kind) if isinstance(kind, str) else None
    if code is None:
        raise ValueError(f"{who}: kind must be one of {sorted(PERTURB_KINDS)}, got {kind!r}")
    if isinstance(size, bool) or not isinstance(size, int) or size < 1:
        raise ValueError(f"{who}: size must be an integer >= 1, got {size!r}")
    shape = tuple(int(s) for s in shape)
    if any(s < 1 for s in shape):
        raise ValueError(f"{who}: empty sample shape {shape}")
    if code == 2:
        if len(shape) != 4:
            raise ValueError(f"{who}: blocks need a (Cv, D, H, W) sample, got {shape}")
        n0, n1, n2, n3 = shape
        units = -(-n1 // size) * -(-n2 // size) * -(-n3 // size)
    else:
        if code == 1 and len(shape) == 1:
            shape = (1,) + shape
        if len(shape) != 2:
            raise ValueError(f"{who}: {'rows' if code == 0 else 'windows'} need a (C, T) sample"
                             f"{' or a tabular (F,) one' if code == 1 else ''}, got {shape}")
        (n0, n1), n2, n3 = shape, 1, 1
        units = n0 if code == 0 else -(-n1 // size)
    return code, n0, n1, n2, n3, size, units


def perturb_units(kind, shape, size: int = 1) -> int:
    """U = how many units one sample of ``shape`` has: its rows, ceil(T / size) windows, or ceil(D / size) *
    ceil(H / size) * ceil(W / size) blocks (the unit table of DESIGN.md 5p); host only"""
    return _perturb_geometry(kind, shape, size, "perturb_units")[6]


def _perturb_masks(masks: torch.Tensor, units: int, who: str) -> torch.Tensor:
    if masks.dim() != 2 or masks.shape[1] != units or masks.shape[0] < 1:
        raise ValueError(f"{who}: masks must be (M >= 1, U = {units}), got {tuple(masks.shape)}")
    return masks


def perturb_expand(x: torch.Tensor, base, masks: torch.Tensor, units, m0: int = 0, m: Optional[int] = None) -> torch.Tensor:
    """(m * B, ...) fp32, mask-major: row j * B + b = sample b with every unit that ``masks[m0 + j]`` marks 0 replaced by
    the baseline (mm_perturb_expand).  ``units`` = (kind, size); ``masks`` (M, U) int32 on x's device, 1 = keep;
    ``base``: None (zeros) | (B, ...) | (1, ...) / (...) broadcast, as for `xai_interpolate`."""
    xc = x.detach().float().contiguous()
    code, n0, n1, n2, n3, size, U = _perturb_geometry(units[0], xc.shape[1:], units[1], "perturb_expand")
    _perturb_masks(masks, U, "perturb_expand")
    m = masks.shape[0] - m0 if m is None else int(m)
    if m0 < 0 or m < 1 or m0 + m > masks.shape[0]:
        raise ValueError(f"perturb_expand: masks [{m0}, {m0} + {m}) of {masks.shape[0]}")
    b, rows = _xai_base(xc, base)
    _need_gpu(xc, masks)
    if masks.dtype != torch.int32 or not masks.is_contiguous():
        raise ValueError("perturb_expand: masks must be a contiguous int32 tensor")
    B = xc.shape[0]
    out = _empty((m * B,) + tuple(xc.shape[1:]), _F32, xc)
    _hip.call("mm_perturb_expand", xc, b, rows, masks, out, B, code, n0, n1, n2, n3, size, U, int(m0), m)
    return out


def perturb_pair_scores(z: torch.Tensor, z_other: torch.Tensor) -> torch.Tensor:
    """z (m * B, N) embeddings of the perturbed rows, z_other (B, N) the intact other modality -> (m, B) fp32:
    v[j][b] = z[j * B + b] . z_other[b] (mm_perturb_pair_scores)"""
    zc, oc = z.detach().float().contiguous(), z_other.detach().float().contiguous()
    B, N = oc.shape
    if zc.dim() != 2 or zc.shape[1] != N or zc.shape[0] % B != 0 or zc.shape[0] < B:
        raise ValueError(f"perturb_pair_scores: rows {tuple(zc.shape)} against {tuple(oc.shape)}")
    _need_gpu(zc, oc)
    m = zc.shape[0] // B
    v = _empty((m, B), _F32, zc)
    _hip.call("mm_perturb_pair_scores", zc, oc, v, B, m, N)
    return v


def _check_permutations(perm: torch.Tensor, who: str) -> torch.Tensor:
    """(P >= 1, U >= 1) integer table, every row a permutation of 0 .. U - 1 -> int64 on the host"""
    if not isinstance(perm, torch.Tensor) or perm.dim() != 2 or perm.shape[0] < 1 or perm.shape[1] < 1 \
            or perm.dtype.is_floating_point or perm.dtype == torch.bool:
        raise ValueError(f"{who}: permutations must be a (P, U) integer tensor")
    p = perm.detach().cpu().long()
    if not torch.equal(p.sort(dim=1).values, torch.arange(p.shape[1]).expand_as(p)):
        raise ValueError(f"{who}: every row must be a permutation of 0 .. {p.shape[1] - 1}")
    return p


def shapley_masks(perm: torch.Tensor):
    """The coalitions a (P, U) table of permutations asks for, host only -> (masks (P * (U - 1), U) int32, pos (P, U)
    int32): row q * (U - 1) + k - 1 keeps exactly the first k units of permutation q (k = 1 .. U - 1; the empty and the
    full coalition are shared by all permutations and not repeated), pos[q][u] in 1 .. U = the place of unit u in
    permutation q (the inverse permutation plus one): what mm_perturb_shapley reads."""
    p = _check_permutations(perm, "shapley_masks")
    P, U = p.shape
    place = torch.argsort(p, dim=1)                                    # unit -> 0-based place
    k = torch.arange(1, U).view(1, U - 1, 1)
    masks = (place.view(P, 1, U) < k).to(torch.int32).reshape(P * (U - 1), U)
    return masks, (place + 1).to(torch.int32)


def perturb_shapley(v, v_empty: torch.Tensor, v_full: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """phi (B, U) fp32 = the mean over the P permutations of every unit's marginal contribution (mm_perturb_shapley).
    ``v`` (P * (U - 1), B) or (P, U - 1, B) coalition scores in `shapley_masks` order (None when U == 1), ``v_empty`` /
    ``v_full`` (B,), ``pos`` (P, U) from `shapley_masks`."""
    if pos.dim() != 2 or pos.dtype.is_floating_point:
        raise ValueError("perturb_shapley: pos must be a (P, U) integer tensor")
    P, U = pos.shape
    B = v_full.numel()
    if v_empty.numel() != B or (U > 1 and (v is None or v.numel() != P * (U - 1) * B)):
        raise ValueError(f"perturb_shapley: P={P} U={U} B={B} against v of {None if v is None else tuple(v.shape)}, "
                         f"v_empty of {tuple(v_empty.shape)}")
    hp = pos.detach().cpu()
    if int(hp.min()) < 1 or int(hp.max()) > U:
        raise ValueError(f"perturb_shapley: places must lie in 1 .. {U}")
    _need_gpu(v_full, v_empty, v if U > 1 else None)
    fe, ff = v_empty.detach().float().contiguous(), v_full.detach().float().contiguous()
    vc = v.detach().float().contiguous() if U > 1 else None
    pc = pos.detach().to(ff.device, torch.int32).contiguous()
    phi = _empty((B, U), _F32, ff)
    _hip.call("mm_perturb_shapley", vc, fe, ff, pc, phi, B, U, P)
    return phi


def perturb_scores(score_rows, x: torch.Tensor, base, masks: torch.Tensor, units, chunk_masks: Optional[int] = None,
                   budget_bytes: int = XAI_BUDGET_BYTES) -> torch.Tensor:
    """The batched perturbation engine -> (M, B) fp32: the score of every sample under every mask.  The reference loop
    (one clone, one forward and one host synchronisation per knocked-out channel) becomes: k masks at a time are expanded
    into ONE batch of k * B rows (mm_perturb_expand), ``score_rows(rows)`` -> k * B scores (mask-major; any shape with
    that many elements) runs under ``torch.no_grad()``, and the (k, B) scores land in the result on the device.  In eval
    mode the rows of a batch are independent (frozen BatchNorm, no dropout), so chunking changes nothing but the kernels'
    batch size.
    ``units`` = (kind, size), kind "rows" | "windows" | "blocks" (`perturb_units`); ``masks`` (M, U) integers, 1 = keep,
    0 = replace by ``base`` (None = zeros | (B, ...) | (1, ...)).
    The plan and the memory rule are the gradient engine's (`ig_chunks`, `ig_chunk_steps`; one mask = one "step"):
    ``chunk_masks`` = k given by the caller; None: the first mask runs alone, its peak memory is measured and
    floor(budget / that) masks form every later chunk.  As in `integrated_gradients`, that measurement calls
    ``torch.cuda.reset_peak_memory_stats``: the caller's peak-memory statistics of this device start over.
    Argument errors raise ValueError before any launch."""
    xc = x.detach().float().contiguous()
    if not isinstance(units, (tuple, list)) or len(units) != 2:
        raise ValueError(f"perturb_scores: units must be (kind, size), got {units!r}")
    U = _perturb_geometry(units[0], xc.shape[1:], units[1], "perturb_scores")[6]
    if not isinstance(masks, torch.Tensor) or masks.dtype.is_floating_point:
        raise ValueError("perturb_scores: masks must be an integer tensor")
    _perturb_masks(masks, U, "perturb_scores")
    if chunk_masks is not None and int(chunk_masks) < 1:
        raise ValueError("perturb_scores: chunk_masks must be >= 1")
    if budget_bytes < 1:
        raise ValueError("perturb_scores: budget_bytes must be positive")
    b, _ = _xai_base(xc, base)
    _need_gpu(xc)
    dev = xc.device
    mk = masks.detach().to(dev, torch.int32).contiguous()
    M, B = mk.shape[0], xc.shape[0]
    out = _empty((M, B), _F32, xc)
    probe = chunk_masks is None
    plan = ig_chunks(M, 1 if probe else int(chunk_masks), first_alone=probe)
    i = 0
    while i < len(plan):
        m0, k = plan[i]
        if probe and i == 0:
            torch.cuda.synchronize(dev)
            before = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
        with torch.no_grad():
            rows = perturb_expand(xc, b, mk, units, m0, k)
            s = score_rows(rows)
            if s.numel() != k * B:
                raise ValueError(f"perturb_scores: score_rows returned {tuple(s.shape)} for {k * B} rows")
            out[m0:m0 + k] = s.detach().float().reshape(k, B)
        del rows, s
        if probe and i == 0:
            torch.cuda.synchronize(dev)
            mask_bytes = max(1, torch.cuda.max_memory_allocated(dev) - before)
            plan = plan[:1] + [(s0 + 1, n) for s0, n in ig_chunks(M - 1, ig_chunk_steps(M, mask_bytes, budget_bytes))]
        i += 1
    return out
