"""CPU: the case tables of tests/test_igemm1d_gpu.py cover what they claim to.  Importing that module does not touch the
GPU; its dispatch mirror (fwd_cell) only labels shapes."""
from test_igemm1d_gpu import (BIG_EPI, BNRED_CASES, DGRAD_CASES, EPI_CASES, EPI_SHAPES, FWD_CASES, REACHABLE_CELLS,
                              WGRAD_CASES, WGRAD_TAPS, WMANY_CASES, fwd_cell)


def test_every_reachable_forward_cell_is_covered():
    cells = {fwd_cell(B, T, Cin, Cout, k) for B, T, Cin, Cout, k, _ in FWD_CASES}
    assert set(REACHABLE_CELLS) <= cells, sorted(set(REACHABLE_CELLS) - cells)
    assert len(REACHABLE_CELLS) == 12
    # the mirror: a k > 1 convolution always takes the 64 x 64 tile, KCT 128 needs taps 1
    assert fwd_cell(1, 64, 128, 384, 3) == ("64x64", 64) and fwd_cell(1, 64, 128, 384, 1) == ("32x128", 128)
    assert fwd_cell(171, 64, 128, 384, 1) == ("64x128", 128) and fwd_cell(170, 64, 128, 384, 1) == ("32x128", 128)


def test_forward_edges_are_covered():
    taps = {}
    for B, T, Cin, Cout, k, pad in FWD_CASES:
        assert 0 <= pad < k <= 9 and Cin % 16 == 0 and Cout % 4 == 0
        taps.setdefault(k, set()).add(pad)
    assert set(taps) == set(range(1, 10))
    assert all(len(taps[k]) >= 2 for k in (2, 4, 6, 8))
    Ts = {c[1] for c in FWD_CASES}
    assert {1, 31, 33, 64, 65} <= Ts and any(T % 64 and T > 65 for T in Ts)
    assert {4, 12, 20, 48, 132, 384} <= {c[3] for c in FWD_CASES}
    assert {16, 32, 96, 128, 1088} <= {c[2] for c in FWD_CASES}
    assert max(B * -(-T // 64) for B, T, *_ in FWD_CASES) > 512


def test_every_epilogue_step_is_covered():
    acts = {c.get("act", 0) for c in EPI_CASES}
    gz = {c["gz"] for c in EPI_CASES if "gz" in c}
    assert acts == {0, 1, 2, 3, 4} and gz == {0, 1, 2, 3, 4}
    for step in ("scale", "shift", "stats", "res", "pe", "pre", "p"):
        assert any(c.get(step) for c in EPI_CASES), step
        assert any(c.get(step) and c.get("pool") == 2 for c in EPI_CASES), step
    assert any(c.get("p") and c.get("res") and c.get("pool", 1) == 1 for c in EPI_CASES)      # dropped = the residual
    for p in {c["p"] for c in EPI_CASES if c.get("p")}:
        assert (p * 2 ** 32).is_integer() and p in (0.125, 0.25, 0.5)
    assert {fwd_cell(*s[:4], s[4]) for s in EPI_SHAPES.values()} == {("64x64", 64), ("32x128", 128)}
    assert all(fwd_cell(*s[:4], s[4]) == ("64x128", 128) for _, s in BIG_EPI)


def test_gradient_tables_are_covered():
    assert {c[4] for c in WGRAD_CASES} == set(WGRAD_TAPS) == {1, 3, 5, 7}
    assert {c[7] for c in WGRAD_CASES} == {"param", "ws"}
    assert any(c[6] < c[2] for c in WGRAD_CASES)                                        # Cin_real < Cin
    assert {1, 63, 65} <= {c[1] for c in WGRAD_CASES}
    assert any(c[4] > 1 and c[5] != c[4] // 2 for c in WGRAD_CASES)
    assert any(c[2] % 64 and c[3] % 64 for c in WGRAD_CASES if c[4] > 1)
    assert len(WMANY_CASES) > 12 and any(c[2] % 128 and c[3] % 128 for c in WMANY_CASES)
    assert any(c[4] < c[2] for c in WMANY_CASES)
    assert {c[5] for c in BNRED_CASES} == {1, 2} and {c[6] for c in BNRED_CASES} == {1, 2}
    assert any(c[2] % 16 for c in DGRAD_CASES) and any(c[3] % 16 for c in DGRAD_CASES)
