"""CPU: the inputs and the reference of tests/test_attention_sharp_scores_gpu.py (oracle/attention_tiles.py).

What is pinned here, without a GPU and never on a kernel's output:
  - rescale_events, the replay of the forward kernel's lazy running maximum, on score matrices whose events are counted by
    hand;
  - that every (profile, L, dh) the GPU file runs makes the kernel rescale by a finite factor, in a wave that also holds rows
    that need no rescale, on the first tile of a later key chunk and (ragged L) in the partial last tile, that the
    unnormalised probability stays <= 2^8 and comes close to it, and that the randn inputs of every older attention test
    do none of this;
  - that emulate(), the fp64 attention that rounds where the kernels round, is inside the GPU file's bounds of the plain fp64
    reference, and that each of six plausible kernel mistakes is more than 10 bounds away on the new inputs while the randn
    control cannot tell it from the correct kernel.

eager_threshold_wrong_units is the one mistake the randn control is not bit-identical for: comparing the unscaled tile
maximum (1 / scale_log2 ~ 4 x larger) against m + 8 makes the kernel rescale MORE often where scores are positive, which
moves m_lazy and with it the fp32 / bf16 roundings of p, but not the mathematics - like no_max it is asserted to stay
inside the bounds there.  It fires LATE only in a wave whose scores are all negative: the later waves of `ramp`."""
import functools
import math

import pytest
import torch

from oracle import attention_tiles as AT
from oracle.dropout_replica import attn_keep_scale

SEED = 2024
SHARP = ("ramp", "spike", "sharp")
# (profile, B, L, H, dh) of every case of the GPU file
FWD_BWD = [(pr, 1, L, 2, dh) for pr in SHARP + ("offset+", "offset-") for dh in (32, 24, 64) for L in (256, 300)]
BATCHED = [("sharp", 2, 300, 3, dh) for dh in (16, 40)]
READOUT = [(pr, 1, L, 2, dh) for pr in ("spike", "sharp") for dh in (32, 24, 64) for L in (256, 257)]
CASES = FWD_BWD + BATCHED + [c for c in READOUT if c not in FWD_BWD]


@functools.lru_cache(maxsize=None)
def _events(profile, B, L, H, dh):
    qkv, _ = AT.case_inputs(profile, B, L, H, dh)
    s = AT.scores_nats(qkv, H, dh)
    return AT.rescale_events(s), float(s.min()), float(s.max())


def test_rescale_events_on_hand_written_scores():
    # 64 queries (two waves) x 96 keys (three tiles), log2 units, every score 0 but the ones named.  Tile 0 takes every row
    # from m = -inf (alpha = 0: not an event).
    s = torch.zeros(64, 96, dtype=torch.float64)
    s[0, 40] = 20.0      # tile 1, wave 0: row 0 fires the wave, alpha = 2^-20                            -> event
    s[1, 41] = 3.0       # tile 1, wave 0: below the threshold, but rescaled with the wave, alpha = 2^-3  -> event
    #                      rows 2 .. 31 of wave 0 are rescaled by alpha = 1                               -> one mixed tile
    s[2, 70] = 7.5       # tile 2, wave 0: below the threshold and nobody fires: p = 2^7.5, no event
    s[32:, 64] = 10.0    # tile 2, wave 1: all 32 rows fire, alpha = 2^-10                                -> 32 events, not mixed
    ev = AT.rescale_events(s * AT.LN2)
    assert ev[:4] == (34, 1, 0, 0)
    assert ev.max_p == pytest.approx(2.0 ** 7.5, rel=1e-12)
    # 40 queries (the second wave has 24 padded rows, score 0) x 140 keys: tile 4 = keys 128 .. 139 is the first of the second
    # chunk and partial
    s = torch.zeros(40, 140, dtype=torch.float64)
    s[33, 130] = 9.0     # wave 1 fires: row 33 alpha = 2^-9, rows 32, 34 .. 39 alpha = 1; padded rows are not counted
    s[5, 100] = 8.5      # tile 3, wave 0: row 5 alpha = 2^-8.5, others 1; not a chunk's first tile
    ev = AT.rescale_events(s * AT.LN2)
    assert ev[:4] == (2, 2, 1, 1) and ev.max_p == 1.0
    # a padded query votes: with a mask its scores are the mask row of the last query.  12 real rows see nothing new in tile
    # 1, the padded rows' +9 fires the wave: every real row is rescaled by 1 - no event, and p stays 1
    s = torch.zeros(12, 64, dtype=torch.float64)
    pad = torch.zeros(64, dtype=torch.float64)
    pad[40] = 9.0 * AT.LN2
    assert AT.rescale_events(s, pad)[:4] == (0, 0, 0, 0)
    s[3, 50] = 5.0 * AT.LN2                              # ... but a row that grew by less than the threshold is now an event
    assert AT.rescale_events(s, pad)[:4] == (1, 1, 0, 0) and AT.rescale_events(s)[:4] == (0, 0, 0, 0)
    assert AT.rescale_events(s).max_p == pytest.approx(32.0, rel=1e-12)


@pytest.mark.parametrize("profile,B,L,H,dh", CASES)
def test_inputs_make_the_kernel_rescale(profile, B, L, H, dh):
    ev, smin, smax = _events(profile, B, L, H, dh)
    print(f"EVENTS {profile} B{B} L{L} H{H} dh{dh}: {tuple(ev)} scores {smin:.1f} .. {smax:.1f} nats")
    assert ev.max_p <= 256.0
    if profile in SHARP:
        assert ev.events >= 100 and ev.mixed_tiles >= 1 and ev.chunk_first >= 1, ev
        if L % AT.TILE:
            assert ev.partial_tile >= 1, ev
    elif profile == "offset+":
        assert smin >= 90.0
    else:
        assert smax <= -90.0


def test_some_case_comes_close_to_the_largest_probability():
    assert max(_events(*c)[0].max_p for c in CASES) > 128.0


@pytest.mark.parametrize("B,L,H,dh", sorted({c[1:] for c in CASES}))
def test_randn_inputs_never_rescale(B, L, H, dh):
    assert _events("randn", B, L, H, dh)[0][:4] == (0, 0, 0, 0)         # the gap the GPU file closes


def test_sharp_rows_are_close_to_one_hot():
    qkv, _ = AT.case_inputs("sharp", 1, 300, 2, 32)
    top = torch.softmax(AT.scores_nats(qkv, 2, 32), dim=-1).max(dim=-1).values
    assert 0.6 < top.mean().item() < 0.9


def _distance(got, ref, emu):
    """how many bounds `got` is from the fp64 reference: (out, lse); a non-finite result is infinitely far"""
    o = AT.rel_l2(got[0], ref[0]) / AT.tensor_bound(AT.rel_l2(emu[0], ref[0]))
    ls = ((got[1] - ref[1]).abs() / AT.lse_bound(ref[1])).max().item()
    return tuple(x if math.isfinite(x) else math.inf for x in (o, ls))


@functools.lru_cache(maxsize=None)
def _triple(profile, B, L, H, dh, p=0.0, mask_kind=None):
    qkv, dout = AT.case_inputs(profile, B, L, H, dh)
    keep = attn_keep_scale(SEED, B * H, L, p) if p > 0 else None
    mask = None
    if mask_kind == "causal":
        mask = torch.zeros(L, L).masked_fill(torch.arange(L).view(1, L) > torch.arange(L).view(L, 1), float("-inf"))
    elif mask_kind is not None:                          # anti-causal, a finite negative in place of -inf
        mask = torch.zeros(L, L).masked_fill(torch.arange(L).view(1, L) < torch.arange(L).view(L, 1), mask_kind)
    return qkv, dout, mask, keep, AT.plain_fp64(qkv, dout, H, dh, mask, keep), AT.emulate(qkv, dout, H, dh, mask, keep)


@pytest.mark.parametrize("profile,B,L,H,dh,p,mask_kind", [
    ("ramp", 1, 300, 2, 24, 0.25, None), ("spike", 1, 256, 2, 32, 0.0, None), ("sharp", 1, 300, 2, 64, 0.25, None),
    ("offset+", 1, 256, 2, 64, 0.0, None), ("offset-", 1, 300, 2, 32, 0.0, None), ("sharp", 2, 300, 3, 16, 0.25, None),
    ("sharp", 1, 300, 2, 24, 0.25, "causal"), ("sharp", 1, 300, 2, 32, 0.0, -1e4), ("sharp", 1, 300, 2, 64, 0.25, -1e9),
    ("sharp", 1, 300, 2, 24, 0.0, torch.finfo(torch.float32).min)])
def test_emulation_is_inside_the_bounds(profile, B, L, H, dh, p, mask_kind):
    _, _, mask, _, ref, emu = _triple(profile, B, L, H, dh, p, mask_kind)
    E = H * dh
    assert all(torch.isfinite(t).all() for t in emu)
    d_out, d_lse = _distance(emu, ref, emu)
    e = [AT.rel_l2(emu[0], ref[0])] + [AT.rel_l2(g, w) for g, w in zip(AT.split3(emu[2], E), AT.split3(ref[2], E))]
    print(f"EMU {profile} L{L} dh{dh} p{p} mask {mask_kind}: e_emu out dq dk dv " + " ".join(f"{x:.2e}" for x in e)
          + f", lse {d_lse:.2f} of its bound")
    assert d_out <= 1.0 and d_lse <= 1.0
    if mask is not None:                                 # masked: the loop really rescales under the mask as well
        pad = mask[L - 1].double()
        qkv = _triple(profile, B, L, H, dh, p, mask_kind)[0]
        assert AT.rescale_events(AT.scores_nats(qkv, H, dh, mask), pad).events >= 100


MUT_SHAPES = [(1, 300, 2, 24), (1, 256, 2, 32), (1, 256, 2, 64)]


@pytest.mark.parametrize("mistake", AT.MISTAKES)
def test_reference_separates_wrong_kernels(mistake):
    for B, L, H, dh in MUT_SHAPES:
        far = {}
        for profile in SHARP + ("offset+", "offset-"):
            qkv, dout, _, _, ref, emu = _triple(profile, B, L, H, dh)
            far[profile] = _distance(AT.emulate(qkv, dout, H, dh, mistake=mistake), ref, emu)
        print(f"MISTAKE {mistake} L{L} dh{dh}: " + ", ".join(f"{k} out {v[0]:.3g} lse {v[1]:.3g}" for k, v in far.items()))
        assert max(max(far[pr]) for pr in SHARP) > 10.0, far
        if mistake == "no_max":
            for pr in ("offset+", "offset-"):
                got = AT.emulate(*_triple(pr, B, L, H, dh)[:2], H, dh, mistake=mistake)
                assert max(far[pr]) > 10.0 and not torch.isfinite(got[0]).any()
        # ... and the inputs every older test uses cannot see it
        qkv, dout, _, _, ref, emu = _triple("randn", B, L, H, dh)
        got = AT.emulate(qkv, dout, H, dh, mistake=mistake)
        if mistake in ("no_max", "eager_threshold_wrong_units"):         # (module docstring)
            assert max(_distance(got, ref, emu)) <= 1.0
        else:
            assert torch.equal(got[0], emu[0]) and torch.equal(got[1], emu[1])
