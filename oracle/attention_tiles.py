"""TEST INFRASTRUCTURE ONLY (CPU).  The forward attention kernel's lazy online softmax (csrc/attention.hip:
attn_fwd_kernel) replayed in fp64 on the host, inputs that make it rescale, and an emulation of the forward and
backward kernels that rounds where they round.

The kernel walks a (batch, head)'s keys in 32-key tiles (128-key chunks of four tiles are staged in LDS).  One wave owns
32 queries, groups starting at multiples of 32 from row 0 of each 128-query block, i.e. at multiples of 32.  It works in
log2 units (s2 = score * log2 e) and keeps a LAZY running maximum m: accumulators o and l are rescaled by
alpha = exp2(m - max(m, mx)) only in a tile where SOME row of the wave has a tile maximum mx > m + 8 (a wave-uniform
branch, taken by ballot); every row of the wave is rescaled then, rows whose maximum did not grow by alpha = 1.  In every
other tile p = exp2(s2 - m) may reach 2^8.  Padded queries (rows L .. 32 ceil(L / 32) - 1) hold q = 0: they see score 0 on
every key (with an additive mask: the mask row of query L - 1) and vote in the ballot; padded keys are -inf.

score_profiles  builders of bf16-representable qkv (B, L, 3 H dh) whose scores make the kernel rescale
rescale_events  the replay: how often, and where, a score matrix makes the kernel rescale by a finite factor
emulate         fp64 attention forward / backward on the same lazy tiled loop with the kernels' rounding points, and,
                on request, one of six plausible kernel mistakes
plain_fp64      the textbook fp64 attention (the reference of tests/test_attention_head_dims_gpu.py, restated for the
                CPU-only tests)"""
from __future__ import annotations

import math
from typing import Callable, Dict, NamedTuple, Optional

import torch

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
TILE = 32                                # keys per tile, queries per wave
CHUNK = 128                              # keys staged per chunk
THRESH = 8.0                             # log2 units a row's maximum may grow before the wave rescales
D64 = torch.float64
NEG = float("-inf")

MISTAKES = ("no_l_rescale", "no_o_rescale", "alpha_from_tile_max", "alpha_one", "no_max", "eager_threshold_wrong_units")


# ---------------------------------------------------------------------------------------------------------- inputs
def _bf16(x):
    return x.to(torch.bfloat16).float()


def _rows(B, L, H, period=3):
    """(B, H, L) row class (b + h + i) % period: which rows take the rank-one component, varied over batch and head"""
    i = torch.arange(L).view(1, 1, L)
    return (i + torch.arange(H).view(1, H, 1) + torch.arange(B).view(B, 1, 1)) % period


def _draw(B, L, H, dh, seed):
    g = torch.Generator().manual_seed(seed)
    return _bf16(torch.randn(B, L, 3 * H * dh, generator=g))


def _set_rank_one(qkv, H, dh, a, c, gain):
    """coordinate 0 of every head's q and k replaced by a rank-one pair (the randn draw there is dropped), so that
    the head's scores gain a[b, h, i] * c[j] nats: q0 = a * Q0, k0 = c * sqrt(dh) / Q0, Q0 = bf16(gain * sqrt(dh)).  The
    magnitude sits in q (gain > 1): a large common component of K would be multiplied by the rounding error of dS in dQ."""
    B, L, _ = qkv.shape
    E = H * dh
    q0 = float(_bf16(torch.tensor(gain * math.sqrt(dh))))
    x = qkv.clone().view(B, L, 3, H, dh)
    x[:, :, 0, :, 0] = (a.float() * q0).permute(0, 2, 1)
    x[:, :, 1, :, 0] = (c.float() * (math.sqrt(dh) / q0)).view(1, L, 1)
    return _bf16(x.view(B, L, 3 * E))


def _randn(B, L, H, dh, seed):
    """the control: what every other attention test draws"""
    return _draw(B, L, H, dh, seed)


def _ramp(B, L, H, dh, seed):
    """score ~ a_i c_j + N(0, 1): c_j = (j - (L - 1)) ln 2 nats, one log2 unit per key, 32 per tile; a_i = -1 on every
    third row of the first 128 queries, +1 otherwise.  Rising rows climb from -(L - 1) log2 units to 0 and rescale at
    every tile, falling rows hold their maximum (up to +(L - 1) log2 units) in the first tile; the waves of the first
    128 queries hold both kinds, the later ones rising rows only.  Slope and sign are what eager_threshold_wrong_units
    needs to show: an unscaled comparison fires late only while a wave's scores are all negative, and costs nothing
    until p = exp2(s2 - m) leaves fp32 at 2^128; the falling rows' positive scores are what no_max overflows on."""
    falling = (_rows(B, L, H) == 2) & (torch.arange(L) < CHUNK)
    a = torch.where(falling, -1.0, 1.0)
    c = (torch.arange(L, dtype=D64) - (L - 1)) * LN2
    return _set_rank_one(_draw(B, L, H, dh, seed), H, dh, a, c, 32.0)


def _spike(B, L, H, dh, seed):
    """randn, plus for two rows in three the last key (in the partial tile of a ragged L) at +40 nats
    and the first key of the second 128-key chunk at +15 nats"""
    a = (_rows(B, L, H) != 2).double()
    c = torch.zeros(L, dtype=D64)
    c[CHUNK], c[L - 1] = 15.0, 40.0
    return _set_rank_one(_draw(B, L, H, dh, seed), H, dh, a, c, 4.0)


def _sharp(B, L, H, dh, seed):
    """q and k of a randn draw times sqrt(8): scores of standard deviation 8 nats, rows close to one-hot"""
    E = H * dh
    x = _draw(B, L, H, dh, seed)
    x[..., :2 * E] *= math.sqrt(8.0)
    return _bf16(x)


def _offset(sign):
    def build(B, L, H, dh, seed):
        """every score of every row at sign * 100 nats + N(0, 1)"""
        a = torch.ones(B, H, L, dtype=D64)
        return _set_rank_one(_draw(B, L, H, dh, seed), H, dh, a, torch.full((L,), sign * 100.0, dtype=D64), 50.0)
    return build


score_profiles: Dict[str, Callable[[int, int, int, int, int], torch.Tensor]] = {
    "randn": _randn, "ramp": _ramp, "spike": _spike, "sharp": _sharp, "offset+": _offset(1.0), "offset-": _offset(-1.0)}


# seeds of the sharp draws whose last, partial tile (one key at L = 257) would otherwise rescale nobody; chosen on the
# fp64 scores, as every condition on these inputs is (tests/test_attention_sharp_scores_host.py asserts them)
_SEED_BUMP: Dict[tuple, int] = {("sharp", 257, 32): 1, ("sharp", 257, 64): 13}


def case_inputs(profile, B, L, H, dh):
    """the (qkv, dout) of one test case, bf16-representable fp32: one seeded draw per (profile, L, dh)"""
    seed = 1000 * L + dh + _SEED_BUMP.get((profile, L, dh), 0)
    dout = _bf16(torch.randn(B, L, H * dh, generator=torch.Generator().manual_seed(seed + 7919)))
    return score_profiles[profile](B, L, H, dh, seed), dout


def rel_l2(got, want):
    return ((got.double() - want.double()).norm() / want.double().norm().clamp_min(1e-30)).item()


def tensor_bound(e_emu):
    """rel-L2 bound of a bf16 output against fp64: the worst relative cost of the final bf16 rounding, and three times
    the error of emulate() on the same case"""
    return 2.0 ** -9 + 3.0 * e_emu


def lse_bound(lse64):
    """elementwise |lse - lse64| bound: the masked-attention bound at |lse| of order 1, and eight fp32 roundings at
    the magnitude of the lse"""
    return 4e-6 + 8.0 * 2.0 ** -24 * lse64.abs()


def split3(dqkv, E):
    return dqkv[..., :E], dqkv[..., E:2 * E], dqkv[..., 2 * E:]


def _split(qkv, H, dh):
    B, L, _ = qkv.shape
    return tuple(t.reshape(B, L, H, dh).transpose(1, 2) for t in qkv.double().split(H * dh, dim=2))      # (B, H, L, dh)


def _mask4(mask, B, H, L):
    if mask is None:
        return None
    return mask.view(1, 1, L, L).expand(B, H, L, L) if mask.dim() == 2 else mask.view(B, H, L, L)


def scores_nats(qkv, H, dh, mask=None):
    """(B, H, L, L) fp64 scores q k^T / sqrt(dh) + mask of the bf16 operands"""
    q, k, _ = _split(qkv, H, dh)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    m = _mask4(mask, *s.shape[:3])
    return s if m is None else s + m.double()


def plain_fp64(qkv, dout, H, dh, mask=None, keep=None):
    """textbook fp64 attention on the bf16 operands -> out (B, L, E), lse (B, H, L) in nats, dqkv; `keep`
    (B * H, L, L) is the scaled keep mask of oracle.dropout_replica.attn_keep_scale"""
    B, L, _ = qkv.shape
    E = H * dh
    x = qkv.double().requires_grad_(True)
    q, k, v = (t.view(B, L, H, dh).transpose(1, 2) for t in x.split(E, dim=2))
    s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    if mask is not None:
        s = s + _mask4(mask, B, H, L).double()
    lse = torch.logsumexp(s, dim=-1)
    pr = torch.exp(s - lse.unsqueeze(-1))
    if keep is not None:
        pr = pr * keep.view(B, H, L, L).double()
    o = (pr @ v).transpose(1, 2).reshape(B, L, E)
    o.backward(dout.double())
    return o.detach(), lse.detach(), x.grad


# ------------------------------------------------------------------------------------------------ the lazy tiled loop
def _f32(x):
    return x.float().double()


def _exp2_hw(x):
    """v_exp_f32: an fp32 result, results below 2^-126 flushed to zero, above 2^128 -> inf"""
    p = _f32(torch.exp2(x))
    return torch.where(p < 2.0 ** -126, torch.zeros_like(p), p)


def _to_bf16(x):
    return x.float().to(torch.bfloat16).double()         # fp32 first, as the kernels' registers are


class _Walk(NamedTuple):
    o: Optional[torch.Tensor]            # (Lq, dh) unnormalised P V
    l: torch.Tensor                      # (Lq,)
    m: torch.Tensor                      # (Lq,) lazy maximum, log2 units
    events: int
    mixed: int
    chunk_first: int
    partial: int
    max_log2_p: float


def _walk(s2, pad_row, v=None, keep01=None, mistake=None, sc2=None):
    """one (batch, head): s2 (Lq, L) fp64 scores in log2 units with the mask added, pad_row (L,) what a padded query sees"""
    Lq, L = s2.shape
    Lp, Kp = -(-Lq // TILE) * TILE, -(-L // TILE) * TILE
    S = torch.full((Lp, Kp), NEG, dtype=D64)
    S[:Lq, :L] = s2
    S[Lq:, :L] = pad_row
    real = torch.arange(Lp) < Lq
    m = torch.full((Lp,), 0.0 if mistake == "no_max" else NEG, dtype=D64)
    l = torch.zeros(Lp, dtype=D64)
    o = torch.zeros(Lp, v.shape[1], dtype=D64) if v is not None else None
    if v is not None:
        vp = torch.zeros(Kp, v.shape[1], dtype=D64)
        vp[:L] = v
        kp = torch.ones(Lp, Kp, dtype=torch.bool)
        if keep01 is not None:
            kp[:Lq, :L] = keep01
    ev_n = mixed_n = first_n = part_n = 0
    max_lp = NEG
    for kt in range(0, Kp, TILE):
        st = S[:, kt:kt + TILE]
        mx = st.max(dim=1).values
        if mistake != "no_max":
            fire = (mx / sc2 if mistake == "eager_threshold_wrong_units" else mx) > m + THRESH
            wave = fire.view(-1, TILE).any(dim=1).repeat_interleave(TILE)
            m_new = torch.maximum(m, mx)
            top = mx if mistake == "alpha_from_tile_max" else m_new
            d = m - torch.where(top == NEG, torch.zeros_like(top), top)   # all keys so far masked: subtract 0
            d = torch.where(m == NEG, torch.full_like(d, NEG), d)
            alpha = _exp2_hw(d)
            if mistake == "alpha_one":
                alpha = torch.ones_like(alpha)
            a = torch.where(wave, alpha, torch.ones_like(alpha))
            if mistake != "no_l_rescale":
                l = l * a
            if o is not None and mistake != "no_o_rescale":
                o = o * a.unsqueeze(1)
            m = torch.where(wave, m_new, m)
            # the statistics are those of the correct rule
            finite = wave & real & (alpha > 0) & (alpha < 1)
            ones = wave & real & (alpha == 1)
            ev_n += int(finite.sum())
            mixed_n += int((finite.view(-1, TILE).any(dim=1) & ones.view(-1, TILE).any(dim=1)).sum())
            if kt > 0 and kt % CHUNK == 0:
                first_n += int(finite.sum())
            if kt + TILE > L:
                part_n += int(finite.sum())
        m_sub = torch.where(m == NEG, torch.zeros_like(m), m)
        e = st - m_sub.unsqueeze(1)
        max_lp = max(max_lp, float(e[:Lq].max()))
        p = _exp2_hw(e)
        l = l + p.sum(dim=1)
        if o is not None:
            pb = _to_bf16(torch.where(kp[:, kt:kt + TILE], p, torch.zeros_like(p)))
            o = o + pb @ vp[kt:kt + TILE]
    return _Walk(None if o is None else o[:Lq], l[:Lq], m[:Lq], ev_n, mixed_n, first_n, part_n, max_lp)


class RescaleEvents(NamedTuple):
    events: int                          # (row, tile) pairs rescaled by 0 < alpha < 1
    mixed_tiles: int                     # (wave, tile) pairs in which such rows and rows with alpha == 1 are rescaled together
    chunk_first: int                     # events on the first tile of a key chunk with k0 > 0
    partial_tile: int                    # events in a partial last tile
    max_p: float                         # largest exp2(s2 - m_lazy) the kernel forms


def rescale_events(scores_nats, pad_row=None):
    """Replay of the kernel's rule on (..., Lq, L) fp64 scores in nats, additive mask already added.  `pad_row`
    (broadcastable to (..., L)): the scores a padded query row sees - 0 without a mask (the default), the mask row of
    query L - 1 with one.  Only real rows are counted; padded rows vote."""
    Lq, L = scores_nats.shape[-2:]
    s = scores_nats.double().reshape(-1, Lq, L)
    pad = torch.zeros(s.shape[0], L, dtype=D64) if pad_row is None else \
        pad_row.double().expand(*scores_nats.shape[:-2], L).reshape(-1, L)
    tot = [0, 0, 0, 0]
    mp = NEG
    for i in range(s.shape[0]):
        w = _walk(s[i] * LOG2E, pad[i] * LOG2E)
        tot = [t + x for t, x in zip(tot, (w.events, w.mixed, w.chunk_first, w.partial))]
        mp = max(mp, w.max_log2_p)
    return RescaleEvents(*tot, float(2.0 ** mp))


# ------------------------------------------------------------------------------------------------------- emulation
def emulate(qkv, dout, H, dh, mask=None, keep=None, mistake=None):
    """fp64 attention that rounds where the kernels round -> out (B, L, E), lse (B, H, L) nats, dqkv (B, L, 3E).

    Forward (attn_fwd_kernel): the lazy tiled loop above; the unnormalised p = exp2(s2 - m_lazy) is an fp32 value, l sums
    it before the keep mask, P V takes it zeroed by the keep mask and rounded to bf16; out = o dinv / l rounded to
    bf16, lse = (m + log2 l) ln 2 in fp32.  With a mask s2 = fp32(s scale_log2) + fp32(mask log2 e), in fp32.
    Backward (attn_bwd_dq_kernel, attn_bwd_dkv_kernel): p = exp2(s scale_log2 - lse2) in fp32 from the stored fp32 lse,
    delta = sum dO o O of the stored bf16 O, dS = p (keep dinv dP - delta) rounded to bf16, dQ = scale dS K,
    dK = scale dS^T Q, dV = dinv bf16(p keep)^T dO, each rounded to bf16.  Products and sums are fp64 (the kernels': fp32).
    `keep` is attn_keep_scale's (B * H, L, L) scaled mask; `mistake` is one of MISTAKES (forward only: the backward
    kernels have no running maximum and are emulated as they are, on the mistaken forward's out and lse)."""
    assert mistake is None or mistake in MISTAKES, mistake
    B, L, _ = qkv.shape
    E = H * dh
    q, k, v = _split(qkv, H, dh)
    do = dout.double().view(B, L, H, dh).transpose(1, 2)
    scale = 1.0 / math.sqrt(dh)
    sc2 = float(_f32(torch.tensor(scale * LOG2E, dtype=D64)))
    m4 = _mask4(mask, B, H, L)
    dinv = 1.0 if keep is None else float(keep.max())
    k4 = None if keep is None else (keep.view(B, H, L, L) > 0)
    out = torch.empty(B, H, L, dh, dtype=D64)
    lse = torch.empty(B, H, L, dtype=D64)
    dq, dk, dv = (torch.empty(B, H, L, dh, dtype=D64) for _ in range(3))
    for b in range(B):
        for h in range(H):
            raw = q[b, h] @ k[b, h].t()
            if m4 is None:
                s2, pad = raw * sc2, torch.zeros(L, dtype=D64)
            else:
                ml2 = _f32(m4[b, h].double() * LOG2E)
                s2, pad = _f32(_f32(raw * sc2) + ml2), ml2[L - 1]
            kb = None if k4 is None else k4[b, h]
            w = _walk(s2, pad, v[b, h], kb, mistake, sc2)
            ob = _to_bf16(w.o * (dinv / w.l).unsqueeze(1))
            ls = _f32(_f32(w.m + torch.log2(w.l)) * LN2)
            out[b, h], lse[b, h] = ob, ls
            # backward
            p = _exp2_hw(s2 - _f32(ls * LOG2E).unsqueeze(1))
            delta = _f32((do[b, h] * ob).sum(dim=1))
            dp = do[b, h] @ v[b, h].t()
            if kb is not None:
                dp = torch.where(kb, dp * dinv, torch.zeros_like(dp))
            ds = _to_bf16(p * (dp - delta.unsqueeze(1)))
            pk = _to_bf16(p if kb is None else torch.where(kb, p, torch.zeros_like(p)))
            dq[b, h] = _to_bf16(scale * (ds @ k[b, h]))
            dk[b, h] = _to_bf16(scale * (ds.t() @ q[b, h]))
            dv[b, h] = _to_bf16(dinv * (pk.t() @ do[b, h]))

    def flat(t):
        return t.transpose(1, 2).reshape(B, L, E)
    return flat(out), lse, torch.cat([flat(dq), flat(dk), flat(dv)], dim=2)
