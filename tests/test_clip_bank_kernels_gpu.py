"""Cross-batch memory InfoNCE (mm_clip_bank_loss, mm_clip_bank_push, mm_clip_bank_ws_floats; csrc/clip_bank.hip) against
an fp64 restatement of the contract in include/mmeeg_hip.h: keys of own row r are the batch rows and the n valid bank rows,
P(r) = the batch key r (gid NULL) or every batch / bank key with r's id, l_dir(r) = LSE_all - LSE_P, loss = mean_r of the two
directions' mean; dz = d loss / d z by autograd, bank rows constants.  The push is held against a ring model on the host.
Tolerances: those of the project's loss-kernel tests (tests/test_sigmoid_loss_gpu.py)."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from multimodal_eeg_fmri_amd import _hip, ops

pytestmark = pytest.mark.gpu

KC = 64                                                   # the kernel's key chunk (csrc/clip_bank.hip)
# N in {16, 128} x B in {2, 6, 32} x K in {8, 64, 200}, B <= K
SHAPES = [(N, B, K) for N in (16, 128) for B in (2, 6, 32) for K in (8, 64, 200) if B <= K]
# every other path of the kernels: N > 128 (keys reloaded per query) | five full query tiles (B = 6 and 2 above: one partial
# tile, 32: four) | more fold tasks than threads | more keys than one coefficient tile
EXTRA_SHAPES = [(132, 6, 64), (16, 40, 64), (16, 160, 200), (16, 6, 1100)]
# (s, correlated pairs): initial temperature of the sigmoid loss | the InfoNCE initialisation 1 / 0.07 | a trained regime
POINTS = {"init": (10.0, False), "tau": (1 / 0.07, False), "trained": (30.0, True)}
FILLS = ("empty", "partial", "full")
NINF = torch.tensor(-math.inf, dtype=torch.float64)


def fill_level(fill, B, K):
    """-> state words {head, filled, pushes, 0}: empty | partly filled, neither n nor B + n a multiple of the key chunk | full
    after wrapping, head != 0"""
    if fill == "empty":
        return [0, 0, 0, 0]
    if fill == "partial":
        n = {8: 5, 64: 37, 200: 131, 1100: 1031}[K]
        assert n % KC and (B + n) % KC and n < K
        return [n % K, n, 3, 0]
    return [3 % K if K > 3 else 1, K, 9, 0]


def ref_bank(z, gid, bank, bank_gid, n, ls):
    """fp64 -> ((loss, top1 e->f, top1 f->e, d loss / d logit_scale), d loss / d z, the smallest top-1 margin)"""
    z = z.double().clone().requires_grad_(True)
    lso = torch.tensor(float(ls), dtype=torch.float64, requires_grad=True)
    B, N = z.shape[0], z.shape[1] // 2
    bk = bank[:n].double()
    ze, zf = z[:, :N], z[:, N:]
    xe = ze @ torch.cat([zf, bk[:, N:]]).T                  # e->f: [B][B + n]
    xf = zf @ torch.cat([ze, bk[:, :N]]).T                  # f->e
    if gid is None:
        pos = torch.cat([torch.eye(B, dtype=torch.bool), torch.zeros(B, n, dtype=torch.bool)], dim=1)
    else:
        pos = gid[:, None] == torch.cat([gid, bank_gid[:n]])[None, :]
    s = lso.exp()
    l = sum(torch.logsumexp(s * x, 1) - torch.logsumexp(torch.where(pos, s * x, NINF), 1) for x in (xe, xf))
    loss = (0.5 * l).mean()
    dz, dls = torch.autograd.grad(loss, (z, lso))
    tops, margin = [], math.inf
    for x in (xe.detach(), xf.detach()):
        best_pos, best_neg = torch.where(pos, x, NINF).max(1).values, torch.where(pos, NINF, x).max(1).values
        tops.append((best_pos >= x.max(1).values).double().mean())
        margin = min(margin, (best_pos - best_neg).abs().min().item())
    return torch.stack([loss.detach(), tops[0], tops[1], dls]), dz, margin


def _rows(n, N, correlated, gen):
    ze = F.normalize(torch.randn(n, N, generator=gen, dtype=torch.float64), dim=1)
    noise = F.normalize(torch.randn(n, N, generator=gen, dtype=torch.float64), dim=1)
    zf = F.normalize(0.9 * ze + math.sqrt(1 - 0.81) * noise, dim=1) if correlated else noise
    return torch.cat([ze, zf], dim=1).float()


def _group_ids(B, K):
    """ids that repeat inside the batch (pairs), inside the bank (pairs) and across both (the bank cycles through the batch's
    ids and three more)"""
    gid = torch.arange(B) // 2 * 5 - 7
    bank_gid = (torch.arange(K) // 2) % ((B + 1) // 2 + 3) * 5 - 7
    return gid.to(torch.int32), bank_gid.to(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(N, B, K, point, grouped):
    """-> (z, gid, bank, bank_gid, ln s as the fp32 value the kernel reads, {fill: (state words, want4, dz)}); computed once
    and shared by every test that needs the case, on the host"""
    s, correlated = POINTS[point]
    gid, bank_gid = _group_ids(B, K) if grouped else (None, None)
    ls = torch.tensor([math.log(s)]).float().item()
    # the seed: the first of a fixed sequence whose top-1 decisions are unambiguous at every fill level (no score within 1e-4
    # of a tie between the best positive and the best negative), judged on the fp64 oracle alone
    for salt in range(16):
        gen = torch.Generator().manual_seed(N * 7919 + B * 131 + K + len(point) * 17 + int(grouped) + 100003 * salt)
        z, bank = _rows(B, N, correlated, gen), _rows(K, N, correlated, gen)
        refs, margin = {}, math.inf
        for fill in FILLS:
            words = fill_level(fill, B, K)
            want, dz, m = ref_bank(z, gid, bank, bank_gid, words[1], ls)
            refs[fill], margin = (words, want, dz), min(margin, m)
        if margin > 1e-4:
            break
    assert margin > 1e-4, f"top-1 margin {margin:.2e} of case {(N, B, K, point, grouped)}: no seed of the sequence is unambiguous"
    return z, gid, bank, bank_gid, ls, refs


def _dev(t, dtype=None):
    return None if t is None else (t if dtype is None else t.to(dtype)).cuda()


def _run(z, gid, bank, bank_gid, state, ls, K, warmup=0, grad=True, ws_fill=None):
    B, N2 = z.shape
    dz = torch.full((B, N2), float("nan"), device="cuda") if grad else None
    scal = torch.full((4,), float("nan"), device="cuda")
    ws = torch.empty(ops.clip_bank_ws_floats(B, K, N2 // 2), device="cuda")
    if ws_fill is not None:
        ws.fill_(ws_fill)
    _hip.call("mm_clip_bank_loss", z, gid, bank, bank_gid, state, ls, scal, dz, ws, B, K, N2 // 2, warmup)
    return scal, dz


def _device_case(case):
    z, gid, bank, bank_gid, ls, refs = case
    return _dev(z), _dev(gid), _dev(bank), _dev(bank_gid), torch.tensor([ls], device="cuda")


def _check(scal, dz, want, g, what):
    got = scal.cpu().double()
    print(f"{what}: scal {got.tolist()} want {want.tolist()} "
          f"dz max err {(dz.cpu().double() - g).abs().max().item():.3e} of {g.abs().max().item():.3e}")
    torch.testing.assert_close(dz.cpu().double(), g, rtol=1e-5, atol=max(1e-5 * g.abs().max().item(), 1e-6))
    torch.testing.assert_close(got[[0, 3]], want[[0, 3]], rtol=1e-5, atol=1e-6)
    assert torch.equal(scal[1:3].cpu(), want[1:3].float()), (scal, want)         # exact: count / B rounded to fp32 once


def test_workspace_size():
    c = ctypes.c_int(0)
    _hip.call("mm_clip_bank_ws_floats", 32, 4096, 128, ctypes.addressof(c))
    assert c.value == ops.clip_bank_ws_floats(32, 4096, 128) >= 2 * 32 * (32 + 4096)


@pytest.mark.parametrize("N,B,K", SHAPES)
@pytest.mark.parametrize("point", list(POINTS))
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_bank_loss_matches_fp64(N, B, K, point, grouped):
    case = _case(N, B, K, point, grouped)
    z, gid, bank, bank_gid, ls = _device_case(case)
    for fill, (words, want, g) in case[5].items():
        state = torch.tensor(words, dtype=torch.int32, device="cuda")
        before = bank.clone()
        scal, dz = _run(z, gid, bank, bank_gid, state, ls, K)
        _check(scal, dz, want, g, f"{fill} n={words[1]}")
        assert torch.equal(bank, before)                                     # bank rows are constants: never written
        assert torch.equal(state.cpu(), torch.tensor(words, dtype=torch.int32))
        scal2, dz2 = _run(z, gid, bank, bank_gid, state, ls, K, ws_fill=float("nan"))
        assert torch.equal(dz, dz2) and torch.equal(scal, scal2)             # bit-reproducible; ws needs no initialisation
        scal3, _ = _run(z, gid, bank, bank_gid, state, ls, K, grad=False)    # scalars only: the same scalars
        assert torch.equal(scal, scal3)


@pytest.mark.parametrize("N,B,K", EXTRA_SHAPES)
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_bank_loss_other_kernel_paths(N, B, K, grouped):
    case = _case(N, B, K, "tau", grouped)
    z, gid, bank, bank_gid, ls = _device_case(case)
    for fill in ("partial", "full") if K == 1100 else ("full",):
        words, want, g = case[5][fill]
        state = torch.tensor(words, dtype=torch.int32, device="cuda")
        scal, dz = _run(z, gid, bank, bank_gid, state, ls, K)
        _check(scal, dz, want, g, f"{fill} n={words[1]}")


@pytest.mark.parametrize("N,B,K", [(16, 6, 8), (128, 32, 64), (128, 2, 200)])
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_empty_bank_is_the_in_batch_loss(N, B, K, grouped):
    """n = 0: mm_clip_loss_own_rows / _grouped at Bg = B, within 1e-6 absolute"""
    case = _case(N, B, K, "tau", grouped)
    z, gid, bank, bank_gid, ls = _device_case(case)
    state = torch.zeros(4, dtype=torch.int32, device="cuda")
    scal, dz = _run(z, gid, bank, bank_gid, state, ls, K)
    scal0, dz0 = torch.empty(4, device="cuda"), torch.empty_like(dz)
    ops.clip_loss_own_rows(z, gid, ls, scal0, dz0, B, 0)
    print(f"scal {scal.tolist()} in-batch {scal0.tolist()} dz diff {(dz - dz0).abs().max().item():.3e}")
    assert (scal - scal0).abs().max().item() <= 1e-6 and (dz - dz0).abs().max().item() <= 1e-6


@pytest.mark.parametrize("fill", ["empty", "partial"])
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_rows_beyond_the_fill_level_are_never_read(fill, grouped):
    N, B, K = 128, 6, 200
    case = _case(N, B, K, "tau", grouped)
    z, gid, bank, bank_gid, ls = _device_case(case)
    words = case[5][fill][0]
    n = words[1]
    state = torch.tensor(words, dtype=torch.int32, device="cuda")
    clean, dirty = bank.clone(), bank.clone()
    clean[n:] = 0
    dirty[n:] = float("nan")
    ids_clean = ids_dirty = None
    if grouped:
        ids_clean, ids_dirty = bank_gid.clone(), bank_gid.clone()
        ids_clean[n:] = 0
        ids_dirty[n:] = gid[0]                                               # garbage that would count as a positive
    s0, d0 = _run(z, gid, clean, ids_clean, state, ls, K)
    s1, d1 = _run(z, gid, dirty, ids_dirty, state, ls, K)
    assert torch.isfinite(s1).all() and torch.isfinite(d1).all()
    assert torch.equal(s0, s1) and torch.equal(d0, d1)


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_warmup_gate(grouped):
    """pushes < warmup: a full bank does not count (the bits of the empty bank); at pushes == warmup it does"""
    N, B, K = 128, 6, 64
    case = _case(N, B, K, "tau", grouped)
    z, gid, bank, bank_gid, ls = _device_case(case)
    full = torch.tensor([3, K, 9, 0], dtype=torch.int32, device="cuda")
    empty = torch.zeros(4, dtype=torch.int32, device="cuda")
    s_empty, d_empty = _run(z, gid, bank, bank_gid, empty, ls, K)
    s_full, d_full = _run(z, gid, bank, bank_gid, full, ls, K)
    assert not torch.equal(s_empty, s_full)
    s, d = _run(z, gid, bank, bank_gid, full, ls, K, warmup=10)
    assert torch.equal(s, s_empty) and torch.equal(d, d_empty)
    s, d = _run(z, gid, bank, bank_gid, full, ls, K, warmup=9)
    assert torch.equal(s, s_full) and torch.equal(d, d_full)


# ---------------------------------------------------------------- push
def ring_push(words, B, K):
    """the documented push on the host: -> (the slots of rows 0..B-1, the new words)"""
    head, filled, pushes = words[:3]
    return [(head + i) % K for i in range(B)], [(head + B) % K, min(filled + B, K), pushes + 1, 0]


def _push_sequence(B, K, N, steps, grouped):
    gen = torch.Generator().manual_seed(B * 100 + K)
    bank = torch.full((K, 2 * N), -5.0, device="cuda")
    ids = torch.full((K,), -1, dtype=torch.int32, device="cuda") if grouped else None
    state = torch.zeros(4, dtype=torch.int32, device="cuda")
    m_bank, m_ids, words = bank.cpu().clone(), torch.full((K,), -1, dtype=torch.int32), [0, 0, 0, 0]
    for step in range(steps):
        z = torch.randn(B, 2 * N, generator=gen)
        g = torch.randint(0, 50, (B,), generator=gen, dtype=torch.int32) if grouped else None
        _hip.call("mm_clip_bank_push", z.cuda(), _dev(g), bank, ids, state, B, K, N)
        slots, words = ring_push(words, B, K)
        m_bank[slots] = z
        if grouped:
            m_ids[slots] = g
        assert state.cpu().tolist() == words, (step, state.cpu().tolist(), words)
        assert torch.equal(bank.cpu(), m_bank), step
        if grouped:
            assert torch.equal(ids.cpu(), m_ids), step
    return words


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_push_follows_the_ring_model(grouped):
    words = _push_sequence(6, 16, 16, 7, grouped)          # wraps inside the third push; 42 rows through 16 slots
    assert words == [42 % 16, 16, 7, 0]
    assert _push_sequence(8, 8, 128, 3, grouped) == [0, 8, 3, 0]               # B = K: every push replaces the bank


def test_captured_push_replays_like_eager_pushes():
    B, K, N = 6, 16, 16
    z = torch.randn(B, 2 * N, device="cuda")
    g = torch.arange(B, dtype=torch.int32, device="cuda")
    banks = []
    for captured in (False, True):
        bank = torch.zeros(K, 2 * N, device="cuda")
        ids = torch.zeros(K, dtype=torch.int32, device="cuda")
        state = torch.zeros(4, dtype=torch.int32, device="cuda")
        zs = z.clone()

        def push():
            _hip.call("mm_clip_bank_push", zs, g, bank, ids, state, B, K, N)
        if captured:
            graph = torch.cuda.CUDAGraph()                                   # (the eager round before loaded the kernel)
            with torch.cuda.graph(graph):
                push()
        for i in range(5):
            zs.copy_(z + i)                                                  # (a replay reads the static input's current rows)
            graph.replay() if captured else push()
        torch.cuda.synchronize()
        banks.append((bank.cpu(), ids.cpu(), state.cpu()))
    for a, b in zip(*banks):
        assert torch.equal(a, b)
    assert banks[0][2].tolist() == [30 % 16, 16, 5, 0]


def test_bad_arguments_are_refused():
    z = torch.zeros(8, 8, device="cuda")
    bank = torch.zeros(16, 8, device="cuda")
    ids = torch.zeros(16, dtype=torch.int32, device="cuda")
    state = torch.zeros(4, dtype=torch.int32, device="cuda")
    ls = torch.zeros(1, device="cuda")
    scal = torch.empty(4, device="cuda")
    ws = torch.empty(ops.clip_bank_ws_floats(8, 16, 4), device="cuda")
    with pytest.raises(Exception, match="clip_bank_loss: null"):
        _hip.call("mm_clip_bank_loss", z, None, bank, None, None, ls, scal, None, ws, 8, 16, 4, 0)
    with pytest.raises(Exception, match="bank_gid is null"):
        _hip.call("mm_clip_bank_loss", z, ids[:8], bank, None, state, ls, scal, None, ws, 8, 16, 4, 0)
    with pytest.raises(Exception, match="multiple of 4"):
        _hip.call("mm_clip_bank_loss", z, None, bank, None, state, ls, scal, None, ws, 8, 16, 6, 0)
    with pytest.raises(Exception, match="1 <= B <= K"):
        _hip.call("mm_clip_bank_loss", z, None, bank, None, state, ls, scal, None, ws, 8, 4, 4, 0)
    with pytest.raises(Exception, match="1 <= B <= K"):
        _hip.call("mm_clip_bank_push", z, None, bank, None, state, 8, 4, 4)
    with pytest.raises(Exception, match="warmup"):
        _hip.call("mm_clip_bank_loss", z, None, bank, None, state, ls, scal, None, ws, 8, 16, 4, -1)
    with pytest.raises(ValueError, match="does not fit"):
        ops.clip_bank_loss(torch.zeros(32, 8, device="cuda"), None, ops.ClipBank(16, 4), ls, scal, None)
