"""CPU: the shape table of tests/test_power_front_gpu.py's STFT-backward test tells a wrong reflection from a right one.
Importing that module does not touch the GPU.

A plain fp32 torch restatement of mm_stft_power_bwd (windowed frames by index, the DFT as matmuls, the gradient of the
windowed frame, index_add back onto the samples) passes the GPU test's bounds against its fp64 reference at every shape
with T <= 1100, and four broken variants of it each fail them at every shape they apply to:

    drop_left / drop_right    the reads through the left / right reflect padding are not scattered back
    twice_first / twice_last  sample 0 / T - 1 (its own mirror image) is counted once more per direct read

drop_* apply where a frame reaches past that end, twice_* where a frame reads that sample directly.  A shape none of the
four fails at would not belong in the table.  The z-score tables' claims (which loop trips, which form, which side of the
host's switch) are checked by arithmetic."""
import math

import pytest
import torch

from test_power_front_gpu import (CH_OFF, FRONT_CASES, STFT_BWD_SHAPES, STFT_CEIL, ZS_BWD_CEIL, ZS_BWD_SHAPES, ZS_FWD_SHAPES,
                                  _peak, _rel, stft_bwd_case, stft_bwd_lds, stft_bwd_ref64)

HOST_SHAPES = [s for s in STFT_BWD_SHAPES if s[2] <= 1100]
VARIANTS = ("drop_left", "drop_right", "twice_first", "twice_last")


def _raw_index(T, nfft, hop):
    """sample position of element n of every frame before the reflection, (frames, nfft)"""
    frames = T // hop + 1
    return torch.arange(frames).view(-1, 1) * hop + torch.arange(nfft).view(1, -1) - nfft // 2


def applies(variant, T, nfft, hop):
    raw = _raw_index(T, nfft, hop)
    return bool({"drop_left": raw < 0, "drop_right": raw >= T, "twice_first": raw == 0, "twice_last": raw == T - 1}[variant].any())


def stft_bwd_fp32(x, gP, nfft, hop, off, variant=None):
    """fp32 d / dx of sum(|DFT(window * frame)|^2 * gP[..., off : off + C * F]) for x (B, C, T)"""
    B, C, T = x.shape
    F_ = nfft // 2 + 1
    raw = _raw_index(T, nfft, hop)
    frames = raw.shape[0]
    idx = raw.abs()
    idx = torch.where(idx >= T, 2 * (T - 1) - idx, idx)
    assert 0 <= int(idx.min()) and int(idx.max()) < T
    n = torch.arange(nfft, dtype=torch.float64)
    win = (0.5 - 0.5 * torch.cos(2 * math.pi * n / nfft)).float()
    ang = 2 * math.pi * torch.outer(n, torch.arange(F_, dtype=torch.float64)) / nfft
    cm, sm = torch.cos(ang).float(), torch.sin(ang).float()                     # (nfft, F)
    fr = x[:, :, idx] * win                                                     # (B, C, frames, nfft)
    re, im = fr @ cm, -(fr @ sm)                                                # (B, C, frames, F)
    g2 = 2.0 * gP[:, :, off:off + C * F_].reshape(B, frames, C, F_).permute(0, 2, 1, 3)
    dv = ((re * g2) @ cm.t() - (im * g2) @ sm.t()) * win                        # d / d x[idx]
    weight = torch.ones(frames, nfft)
    if variant == "drop_left":
        weight[raw < 0] = 0.0
    elif variant == "drop_right":
        weight[raw >= T] = 0.0
    elif variant == "twice_first":
        weight[raw == 0] = 2.0
    elif variant == "twice_last":
        weight[raw == T - 1] = 2.0
    else:
        assert variant is None
    dx = torch.zeros(B, C, T)
    dx.index_add_(2, idx.reshape(-1), (dv * weight).reshape(B, C, frames * nfft))
    return dx


def _figures(shape, variant=None):
    B, C, T, nfft, hop = shape
    x, gP = stft_bwd_case(*shape)
    got = stft_bwd_fp32(x, gP, nfft, hop, CH_OFF, variant)
    want = stft_bwd_ref64(shape)
    return _rel(got, want), _peak(got, want)


@pytest.mark.parametrize("shape", HOST_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_fp32_restatement_passes_the_gpu_bounds(shape):
    rel, peak = _figures(shape)
    print(f"ERR host stft_bwd {shape} rel {rel:.3e} peak {peak:.3e}")
    b_rel, b_peak = STFT_BWD_SHAPES[shape]
    assert rel <= b_rel and peak <= b_peak, (rel, peak)


@pytest.mark.parametrize("shape", HOST_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_every_broken_reflection_fails_the_gpu_bounds(shape):
    B, C, T, nfft, hop = shape
    b_rel, b_peak = STFT_BWD_SHAPES[shape]
    caught = 0
    for variant in VARIANTS:
        if not applies(variant, T, nfft, hop):
            continue
        rel, peak = _figures(shape, variant)
        print(f"ERR host stft_bwd {shape} {variant} rel {rel:.3e} peak {peak:.3e}")
        assert rel > b_rel or peak > b_peak, (variant, rel, peak)
        # and by a margin no bound under the ceilings could close
        assert rel > 100 * STFT_CEIL[0] or peak > 100 * STFT_CEIL[1], (variant, rel, peak)
        caught += 1
    assert caught >= 1


def test_the_table_reaches_what_it_claims():
    shapes = list(STFT_BWD_SHAPES)
    assert {s[3] for s in shapes} == {8, 16, 32, 64, 128, 256, 512, 1024}
    for B, C, T, nfft, hop in shapes:
        assert T > nfft // 2 and nfft & (nfft - 1) == 0 and stft_bwd_lds(T, nfft) <= 160 * 1024
    both = [s for s in shapes if (lambda r, T: bool(((r < 0).any(dim=1) & (r >= T).any(dim=1)).any()))(_raw_index(*s[2:]), s[2])]
    assert {(2, 3, 5, 8, 2), (1, 2, 129, 256, 64), (1, 2, 257, 512, 128), (1, 2, 513, 1024, 256)} <= set(both)
    lds = sorted(stft_bwd_lds(s[2], s[3]) for s in shapes)
    assert lds[-1] == 160672 and 66976 in lds and 79940 in lds and sum(v > 64 * 1024 for v in lds) == 4
    assert stft_bwd_lds(41000, 8) > 160 * 1024                                 # the refused launch of the GPU test
    assert any(T % 256 and (T // hop + 1) % 8 for _, _, T, _, hop in shapes)
    assert any(T % hop and nfft % hop for _, _, T, nfft, hop in shapes)
    assert any(2 * hop == nfft for *_, nfft, hop in shapes)
    for variant in VARIANTS:
        assert sum(applies(variant, *s[2:]) for s in shapes) >= len(shapes) - 1


def test_the_zscore_tables_reach_what_they_claim():
    one_wg = [s for s, chunked in ZS_FWD_SHAPES.items() if not chunked]
    many_wg = [s for s, chunked in ZS_FWD_SHAPES.items() if chunked]
    for B, rows, chv, cht in ZS_FWD_SHAPES:
        n = rows * cht
        assert ZS_FWD_SHAPES[(B, rows, chv, cht)] == (chv == cht and n % 4 == 0 and n >= 65536)
    # one workgroup of 1024 threads: float4 sweeps with a ragged last trip, the general path unpadded (sample base not
    # 16-byte aligned) and padded, all with more than one trip
    assert any(chv == cht and cht % 4 == 0 and 2048 < rows * cht // 4 and rows * cht // 4 % 1024 for _, rows, chv, cht in one_wg)
    assert any(chv == cht and cht % 4 and rows * cht % 4 and rows * cht > 1024 for _, rows, chv, cht in one_wg)
    assert any(chv < cht and rows * cht > 2048 and rows * cht % 1024 for _, rows, chv, cht in one_wg)
    # both sides of the host's switch, the nearest sizes a float4 layout has
    assert max(rows * cht for _, rows, _, cht in one_wg) == 65536 - 64 and min(rows * cht for _, rows, _, cht in many_wg) == 65536
    # 32 chunks: borders n4 * c / 32 all fractional in one shape
    assert any(all((rows * cht // 4 * c) % 32 for c in range(1, 32)) for _, rows, _, cht in many_wg)
    assert any(B > 1 for B, *_ in many_wg)
    # backward: padded and unpadded, one trip and many, a ragged last trip
    assert any(chv < cht for _, _, chv, cht in ZS_BWD_SHAPES) and any(chv == cht for _, _, chv, cht in ZS_BWD_SHAPES)
    assert any(rows * cht <= 1024 for _, rows, _, cht in ZS_BWD_SHAPES)
    assert any(rows * cht > 65536 and rows * cht % 1024 for _, rows, _, cht in ZS_BWD_SHAPES)
    assert all(b <= ZS_BWD_CEIL for b in ZS_BWD_SHAPES.values())
    assert all(r <= STFT_CEIL[0] and p <= STFT_CEIL[1] for r, p in list(STFT_BWD_SHAPES.values()) + list(FRONT_CASES.values()))
