"""InfoNCE with a momentum key encoder (mm_clip_key_loss, mm_clip_key_ws_floats; csrc/clip_bank.hip) against `ref_key`, the
fp64 restatement of the contract in include/mmeeg_hip.h (tests/test_clip_key_host.py): queries q, keys k (batch) and the n
valid bank rows, no key term; dq = d loss / d q and d / d logit_scale by autograd.  Tolerances: those of the project's
loss-kernel tests (tests/test_clip_bank_kernels_gpu.py): dq rtol 1e-5, atol max(1e-5 max|g|, 1e-6); loss and d / d
logit_scale rtol 1e-5, atol 1e-6; the two top-1 words exact.

The branches of the three launches and the shape that reaches each:
  scores (bank_scores_kernel, shared with mm_clip_bank_loss): key rows in registers (N <= 128: the grid) | reloaded per
    query (N = 132) | one partial query tile (B = 2, 6) | full tiles (B = 32) | full tiles and a partial one (B = 44)
  fold (key_fold_kernel, one wave per (direction, query)): fewer chunks than lanes (every K <= 200: 1-4 chunks) | the last
    workgroup partly filled (B = 6, 2 B = 12 = 3 x 4) | more chunks than lanes, a lane folds two (N = 16, B = 6, K = 4200: 66)
  dq (key_dq_kernel, one workgroup per (query tile, slab of 32 columns, tile of 512 keys)): a slab of one direction
    (N = 128: four slabs per direction) | a slab holding both directions (N = 16: one slab = [dqe | dqf]; N = 132: columns
    128..159 straddle) | a slab with idle lanes past the row's end (N = 132: 264 = 8 x 32 + 8) | one partial query tile
    (B = 2, 6) | several full tiles and a partial one (B = 44) | ONE key tile by capacity, B + K <= 512: its sums are dq,
    no ticket (every shape of the grid) | several key tiles, their sums met by the last arriver behind the ticket: a full
    tile and a partly filled one (K = 1100 full: 1106 = 2 x 512 + 82; K = 4200: 9 tiles), key tiles past the valid keys
    that only take their ticket (K = 1100 empty and partial, K = 4200 at n = 4133)"""
import ctypes

import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
from test_clip_key_host import FILLS, KC, POINTS, fill_level, key_case, ref_key

pytestmark = pytest.mark.gpu

SHAPES = [(N, B, K) for N in (16, 128) for B in (2, 6, 32) for K in (8, 64, 200) if B <= K]
EXTRA_SHAPES = [(132, 6, 64), (16, 44, 64), (16, 6, 1100), (16, 6, 4200)]


def _dev(t, dtype=None):
    return None if t is None else (t if dtype is None else t.to(dtype)).cuda()


def _run(q, k, gid, bank, bank_gid, state, ls, K, warmup=0, grad=True, ws_fill=None):
    B, N2 = q.shape
    dq = torch.full((B, N2), float("nan"), device="cuda") if grad else None
    scal = torch.full((4,), float("nan"), device="cuda")
    ws = torch.empty(ops.clip_key_ws_floats(B, K, N2 // 2), device="cuda")
    if ws_fill is not None:
        ws.fill_(ws_fill)
    _hip.call("mm_clip_key_loss", q, k, gid, bank, bank_gid, state, ls, scal, dq, ws, B, K, N2 // 2, warmup)
    return scal, dq


def _device_case(case):
    q, k, gid, bank, bank_gid, ls, refs = case
    return _dev(q), _dev(k), _dev(gid), _dev(bank), _dev(bank_gid), torch.tensor([ls], device="cuda")


def _check(scal, dq, want, g, what):
    got = scal.cpu().double()
    print(f"{what}: scal {got.tolist()} want {want.tolist()} "
          f"dq max err {(dq.cpu().double() - g).abs().max().item():.3e} of {g.abs().max().item():.3e}")
    torch.testing.assert_close(dq.cpu().double(), g, rtol=1e-5, atol=max(1e-5 * g.abs().max().item(), 1e-6))
    torch.testing.assert_close(got[[0, 3]], want[[0, 3]], rtol=1e-5, atol=1e-6)
    assert torch.equal(scal[1:3].cpu(), want[1:3].float()), (scal, want)         # exact: count / B rounded to fp32 once


def test_workspace_size():
    c = ctypes.c_int(0)
    _hip.call("mm_clip_key_ws_floats", 32, 4096, 128, ctypes.addressof(c))
    assert c.value == ops.clip_key_ws_floats(32, 4096, 128) > ops.clip_bank_ws_floats(32, 4096, 128)


@pytest.mark.parametrize("N,B,K", SHAPES)
@pytest.mark.parametrize("point", list(POINTS))
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_key_loss_matches_fp64(N, B, K, point, grouped):
    case = key_case(N, B, K, point, grouped)
    q, k, gid, bank, bank_gid, ls = _device_case(case)
    for fill, (words, want, g) in case[6].items():
        state = torch.tensor(words, dtype=torch.int32, device="cuda")
        before, k_before = bank.clone(), k.clone()
        scal, dq = _run(q, k, gid, bank, bank_gid, state, ls, K)
        _check(scal, dq, want, g, f"{fill} n={words[1]}")
        assert torch.equal(bank, before) and torch.equal(k, k_before)        # keys are constants: never written
        assert torch.equal(state.cpu(), torch.tensor(words, dtype=torch.int32))
        scal2, dq2 = _run(q, k, gid, bank, bank_gid, state, ls, K, ws_fill=float("nan"))
        assert torch.equal(dq, dq2) and torch.equal(scal, scal2)             # two runs, identical bits; ws needs no initialisation
        scal3, _ = _run(q, k, gid, bank, bank_gid, state, ls, K, grad=False)     # dq = NULL: the same scalars
        assert torch.equal(scal, scal3)


@pytest.mark.parametrize("N,B,K", EXTRA_SHAPES)
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_key_loss_other_kernel_paths(N, B, K, grouped):
    """K = 4200 (its only purpose: 66 chunks, a fold lane with two) is not in `fill_level`'s table: a full ring and a
    partial one of 4133 rows (neither it nor B + it a multiple of the chunk), against `ref_key` computed here"""
    if K == 4200:
        gen = torch.Generator().manual_seed(4200 + int(grouped))
        from test_clip_key_host import _group_ids, _key_rows, _rows
        q64 = _rows(B, N, False, gen)
        q, k, bank = q64.float(), _key_rows(q64, N, gen).float(), _rows(K, N, False, gen).float()
        gid, bank_gid = _group_ids(B, K) if grouped else (None, None)
        ls = torch.tensor([POINTS["tau"][0]]).log().item()
        dev = (_dev(q), _dev(k), _dev(gid), _dev(bank), _dev(bank_gid), torch.tensor([ls], device="cuda"))
        for n in (4133, K):
            assert n == K or (n % KC and (B + n) % KC)
            want, g, margin = ref_key(q, k, gid, bank, bank_gid, n, ls)
            assert margin > 1e-4
            state = torch.tensor([5, n, 9, 0], dtype=torch.int32, device="cuda")
            scal, dq = _run(*dev[:5], state, dev[5], K)
            _check(scal, dq, want, g, f"n={n}")
        return
    case = key_case(N, B, K, "tau", grouped)
    q, k, gid, bank, bank_gid, ls = _device_case(case)
    for fill in FILLS:
        words, want, g = case[6][fill]
        state = torch.tensor(words, dtype=torch.int32, device="cuda")
        scal, dq = _run(q, k, gid, bank, bank_gid, state, ls, K)
        _check(scal, dq, want, g, f"{fill} n={words[1]}")


@pytest.mark.parametrize("N,B,K", [(16, 6, 8), (128, 32, 64), (128, 2, 200)])
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_with_k_equal_q_the_loss_is_the_bank_kernels(N, B, K, grouped):
    """k = q (the same rows): loss, top-1 and d / d logit_scale of mm_clip_bank_loss on the same inputs, at the tolerance
    both kernels are held to against fp64"""
    case = key_case(N, B, K, "tau", grouped)
    q, _, gid, bank, bank_gid, ls = _device_case(case)
    for fill in FILLS:
        state = torch.tensor(fill_level(fill, B, K), dtype=torch.int32, device="cuda")
        scal, _ = _run(q, q, gid, bank, bank_gid, state, ls, K)
        scal0 = torch.empty(4, device="cuda")
        ws = torch.empty(ops.clip_bank_ws_floats(B, K, N), device="cuda")
        _hip.call("mm_clip_bank_loss", q, gid, bank, bank_gid, state, ls, scal0, None, ws, B, K, N, 0)
        print(f"{fill}: key {scal.tolist()} bank {scal0.tolist()}")
        torch.testing.assert_close(scal[[0, 3]], scal0[[0, 3]], rtol=1e-5, atol=1e-6)
        assert torch.equal((scal[1:3] * B).round(), (scal0[1:3] * B).round())    # the same rows counted (that kernel multiplies by fl(1 / B))


@pytest.mark.parametrize("fill", ["empty", "partial"])
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_rows_beyond_the_fill_level_are_never_read(fill, grouped):
    N, B, K = 128, 6, 200
    case = key_case(N, B, K, "tau", grouped)
    q, k, gid, bank, bank_gid, ls = _device_case(case)
    words = case[6][fill][0]
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
    s0, d0 = _run(q, k, gid, clean, ids_clean, state, ls, K)
    s1, d1 = _run(q, k, gid, dirty, ids_dirty, state, ls, K, ws_fill=float("nan"))
    assert torch.isfinite(s1).all() and torch.isfinite(d1).all()
    assert torch.equal(s0, s1) and torch.equal(d0, d1)


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_warmup_gate(grouped):
    """pushes < warmup: a full bank does not count (the bits of the empty bank); at pushes == warmup it does"""
    N, B, K = 128, 6, 64
    case = key_case(N, B, K, "tau", grouped)
    q, k, gid, bank, bank_gid, ls = _device_case(case)
    full = torch.tensor([3, K, 9, 0], dtype=torch.int32, device="cuda")
    empty = torch.zeros(4, dtype=torch.int32, device="cuda")
    s_empty, d_empty = _run(q, k, gid, bank, bank_gid, empty, ls, K)
    s_full, d_full = _run(q, k, gid, bank, bank_gid, full, ls, K)
    assert not torch.equal(s_empty, s_full)
    s, d = _run(q, k, gid, bank, bank_gid, full, ls, K, warmup=10)
    assert torch.equal(s, s_empty) and torch.equal(d, d_empty)
    s, d = _run(q, k, gid, bank, bank_gid, full, ls, K, warmup=9)
    assert torch.equal(s, s_full) and torch.equal(d, d_full)


@pytest.mark.parametrize("K", [40, 1040])
def test_one_captured_graph_serves_a_growing_then_wrapping_bank(K):
    """loss + push of the keys, captured once and replayed over six steps (K = 40, B = 16: the ring wraps inside the third
    push), against the same calls issued eagerly: bit for bit, every step.  K = 1040: three key tiles by capacity - the
    replays run the ticketed path, the tickets zeroed by every replay's own fold launch - of which the growing bank fills
    only the first"""
    N, B = 16, 16
    gen = torch.Generator().manual_seed(77)
    steps = [(torch.nn.functional.normalize(torch.randn(B, 2, N, generator=gen), dim=2).reshape(B, 2 * N).cuda(),
              torch.nn.functional.normalize(torch.randn(B, 2, N, generator=gen), dim=2).reshape(B, 2 * N).cuda(),
              torch.randint(0, 12, (B,), generator=gen, dtype=torch.int32).cuda()) for _ in range(6)]
    ls = torch.tensor([2.3], device="cuda")
    runs = []
    for captured in (False, True):
        bank = ops.ClipBank(K, N, True)
        q, k, gid = (t.clone() for t in steps[0])
        scal, dq = torch.zeros(4, device="cuda"), torch.zeros(B, 2 * N, device="cuda")
        ws = torch.empty(ops.clip_key_ws_floats(B, K, N), device="cuda")

        def step():
            _hip.call("mm_clip_key_loss", q, k, gid, bank.bank, bank.gid, bank.state, ls, scal, dq, ws, B, K, N, 1)
            _hip.call("mm_clip_bank_push", k, gid, bank.bank, bank.gid, bank.state, B, K, N)
        if captured:
            graph = torch.cuda.CUDAGraph()                                   # (the eager round before loaded the kernels)
            with torch.cuda.graph(graph):
                step()
        out = []
        for sq, sk, sg in steps:
            q.copy_(sq), k.copy_(sk), gid.copy_(sg)
            graph.replay() if captured else step()
            out.append((scal.clone(), dq.clone()))
        torch.cuda.synchronize()
        runs.append((out, bank))
    (eager, bank_e), (replayed, bank_g) = runs
    for i, ((s0, d0), (s1, d1)) in enumerate(zip(eager, replayed)):
        assert torch.equal(s0, s1) and torch.equal(d0, d1), i
    for a, b in zip(bank_e.tensors(), bank_g.tensors()):
        assert torch.equal(a, b)
    assert bank_g.state.tolist() == [6 * B % K, min(6 * B, K), 6, 0]
    losses = [s[0].item() for s, _ in eager]
    assert len(set(losses)) == 6 and all(x == x for x in losses)


def test_bad_arguments_are_refused():
    q = torch.zeros(8, 8, device="cuda")
    bank = torch.zeros(16, 8, device="cuda")
    ids = torch.zeros(16, dtype=torch.int32, device="cuda")
    state = torch.zeros(4, dtype=torch.int32, device="cuda")
    ls = torch.zeros(1, device="cuda")
    scal = torch.full((4,), 7.0, device="cuda")
    ws = torch.empty(ops.clip_key_ws_floats(8, 16, 4), device="cuda")
    with pytest.raises(Exception, match="clip_key_loss: null"):
        _hip.call("mm_clip_key_loss", q, None, None, bank, None, state, ls, scal, None, ws, 8, 16, 4, 0)
    with pytest.raises(Exception, match="clip_key_loss: null"):
        _hip.call("mm_clip_key_loss", q, q, None, bank, None, None, ls, scal, None, ws, 8, 16, 4, 0)
    with pytest.raises(Exception, match="bank_gid is null"):
        _hip.call("mm_clip_key_loss", q, q, ids[:8], bank, None, state, ls, scal, None, ws, 8, 16, 4, 0)
    with pytest.raises(Exception, match="multiple of 4"):
        _hip.call("mm_clip_key_loss", q, q, None, bank, None, state, ls, scal, None, ws, 8, 16, 6, 0)
    with pytest.raises(Exception, match="1 <= B <= K"):
        _hip.call("mm_clip_key_loss", q, q, None, bank, None, state, ls, scal, None, ws, 8, 4, 4, 0)
    with pytest.raises(Exception, match="warmup"):
        _hip.call("mm_clip_key_loss", q, q, None, bank, None, state, ls, scal, None, ws, 8, 16, 4, -1)
    with pytest.raises(Exception, match="16-byte aligned"):
        _hip.call("mm_clip_key_loss", q, q.view(-1)[1:9], None, bank, None, state, ls, scal, None, ws, 1, 16, 4, 0)
    c = ctypes.c_int(0)
    with pytest.raises(Exception, match="1 <= B <= K"):
        _hip.call("mm_clip_key_ws_floats", 8, 4, 4, ctypes.addressof(c))
    with pytest.raises(ValueError, match="does not fit"):
        ops.clip_key_loss(torch.zeros(32, 8, device="cuda"), torch.zeros(32, 8, device="cuda"), None, ops.ClipBank(16, 4), ls, scal, None)
    torch.cuda.synchronize()
    assert scal.tolist() == [7.0] * 4                                        # nothing was launched
