"""mm_adamw_clip_groups / mm_adamw_clip_groups_ema (csrc/optim.hip: adamw_groups_kernel<false / true>) and optim.FusedAdamW
with parameter groups.

Exact by contract (torch.equal): for every distinct (multiplier, weight decay) pair of a table, the elements of that pair's
segments carry the p, m, v, g (and ema) bits that mm_adamw_clip (mm_adamw_clip_ema) writes on a copy of the WHOLE bucket
when called with state[2] = fl32(lr * multiplier) and that weight decay - so one mis-assigned element, in a one-element
segment included, fails; state[0..5) and state[5] are the plain entry points' bits; state[6..8) is never written (NaN
canary); a multiplier of 0 keeps p's bits while m and v move; a second run's bits; a NaN-filled tail behind the table's
n_seg values changes nothing.
fp64: three chained steps against ref_adamw_groups (tests/test_param_groups_host.py, checked there against
torch.optim.AdamW with parameter groups) within the rel-L2 bounds of tests/test_adamw_kernels_gpu.py (BOUND: p 3e-7,
m 4e-7, v 8e-7): the per-element arithmetic is the same, the one extra rounding of lr * multiplier is 2^-24 relative on a
term of size ~lr.  ERR lines print every figure before it is asserted.

Sizes 1, 255, 2049 and 2048 * 256 + 3 (a second, ragged sweep of the grid-stride loop); tables: one segment, every element
its own segment, 1024 segments of lengths 1, 2, 3 cycling, ends at odd offsets, an end at exactly 2048 * 256 and another
one element later."""
import functools

import pytest
import torch

from multimodal_eeg_fmri_amd import _hip
from multimodal_eeg_fmri_amd.optim import FusedAdamW
from test_adamw_kernels_gpu import BOUND
from test_param_groups_host import ref_adamw_groups

pytestmark = pytest.mark.gpu

SWEEP = 2048 * 256
MULTS, WDS = (0.0, 0.1, 1.0, 10.0), (0.0, 0.02, 0.3)
HYPER = dict(b1=0.9, b2=0.999, eps=1e-8, max_norm=1.0, grad_scale=1.0)
LR, STEP0 = 3e-3, 3


def f32(x):
    return torch.tensor(float(x), dtype=torch.float32).item()


def fl_mul(a, b):
    """fl32(a * b) of two fp32 values"""
    return (torch.tensor(a, dtype=torch.float32) * torch.tensor(b, dtype=torch.float32)).item()


def _cycling_1024():
    ends, off = [], 0
    for s in range(1024):
        off += 1 + s % 3
        ends.append(off)
    ends[-1] = 2049                                                          # (the last segment takes the remainder: 3 elements)
    assert ends[-2] < 2049
    return ends


TABLES = {
    "one element": (1, [1]),
    "255 one segment": (255, [255]),
    "255 every element its own segment": (255, list(range(1, 256))),
    "2049 one segment": (2049, [2049]),
    "2049 1024 segments of 1, 2, 3": (2049, _cycling_1024()),
    "2049 odd offsets": (2049, [3, 257, 1025, 1027, 2049]),
    "sweep + 3 one segment": (SWEEP + 3, [SWEEP + 3]),
    "sweep + 3 ends at the sweep": (SWEEP + 3, [12345, SWEEP, SWEEP + 1, SWEEP + 3]),
}


def _values(n_seg, shift=0):
    """segment s gets pair (s + shift) mod 12 of the 4 multipliers x 3 decays"""
    pairs = [(f32(MULTS[k % 4]), f32(WDS[k // 4])) for k in range(12)]
    return [pairs[(s + shift) % 12] for s in range(n_seg)]


def _state(lr, step0=STEP0):
    st = torch.zeros(8 + 1024, device="cuda")                               # MM_OPT_STATE_FLOATS
    st[0], st[2] = float(step0), lr
    st[5:8] = float("nan")
    return st


def _inputs(n):
    gen = torch.Generator().manual_seed(4243 + n % 9973)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 1.5                                 # |g| > max_norm at every size but n = 1: clipping
    m = torch.randn(n, generator=gen) * 0.1                                 # non-zero starting moments
    v = torch.rand(n, generator=gen) * 0.01
    shadow = p + torch.randn(n, generator=gen) * 0.3 + 0.05
    if n == 1:
        g = g.sign() * 2.5
    return {"p": p, "g": g, "m": m, "v": v, "ema": shadow}


def _device(n, lr):
    t = {k: x.cuda() for k, x in _inputs(n).items()}
    t["state"] = _state(f32(lr))
    return t


def _table(ends, vals, tail=0):
    """device arrays of the table; `tail` more entries behind the n_seg values: NaN (and -1 ends), never to be read"""
    nan = [float("nan")] * tail
    return (torch.tensor(list(ends) + [-1] * tail, dtype=torch.int64, device="cuda"),
            torch.tensor([a for a, _ in vals] + nan, dtype=torch.float32, device="cuda"),
            torch.tensor([b for _, b in vals] + nan, dtype=torch.float32, device="cuda"))


def _head(t):
    h = HYPER
    return (t["p"], t["g"], t["m"], t["v"], t["state"], t["p"].numel(), f32(h["b1"]), f32(h["b2"]), f32(h["eps"]))


def _plain_step(t, wd, ema: bool, zero_grad=1, epoch=None):
    h = HYPER
    _hip.call("mm_sumsq", t["g"], t["state"], t["p"].numel())
    args = (*_head(t), wd, f32(h["max_norm"]), f32(h["grad_scale"]), zero_grad, epoch)
    if ema:
        _hip.call("mm_adamw_clip_ema", *args, t["ema"], f32(0.9), 1)
    else:
        _hip.call("mm_adamw_clip", *args)


def _groups_step(t, table, n_seg, ema: bool, zero_grad=1, epoch=None):
    h = HYPER
    _hip.call("mm_sumsq", t["g"], t["state"], t["p"].numel())
    args = (*_head(t), f32(h["max_norm"]), f32(h["grad_scale"]), zero_grad, epoch, *table, n_seg)
    if ema:
        _hip.call("mm_adamw_clip_groups_ema", *args, t["ema"], f32(0.9), 1)
    else:
        _hip.call("mm_adamw_clip_groups", *args)


def _cpu(t):
    return {k: x.cpu() for k, x in t.items()}


@functools.lru_cache(maxsize=None)
def _grouped(name, ema, tail=0):
    n, ends = TABLES[name]
    vals = _values(len(ends))
    t = _device(n, LR)
    _groups_step(t, _table(ends, vals, tail), len(ends), ema)
    torch.cuda.synchronize()
    return _cpu(t)


@functools.lru_cache(maxsize=None)
def _plain(n, mult, wd, ema):
    """mm_adamw_clip[_ema] on the whole bucket with the scalar learning rate fl32(lr * mult) (computed once per pair)"""
    t = _device(n, fl_mul(f32(LR), mult))
    _plain_step(t, wd, ema)
    torch.cuda.synchronize()
    return _cpu(t)


def _segments_of(ends, vals):
    by_pair, lo = {}, 0
    for end, pair in zip(ends, vals):
        by_pair.setdefault(pair, []).append((lo, end))
        lo = end
    return by_pair


@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("name", list(TABLES))
def test_every_segment_carries_the_plain_kernels_bits(name, ema):
    n, ends = TABLES[name]
    vals = _values(len(ends))
    got = _grouped(name, ema)
    p0 = _inputs(n)["p"]
    keys = ("p", "m", "v", "g") + (("ema",) if ema else ())
    by_pair = _segments_of(ends, vals)
    if len(ends) >= 12:
        assert len(by_pair) == 12                                            # every multiplier with every decay
    for (mult, wd), segs in by_pair.items():
        want = _plain(n, mult, wd, ema)
        idx = torch.cat([torch.arange(lo, hi) for lo, hi in segs])
        for k in keys:
            assert torch.equal(got[k][idx], want[k][idx]), (k, mult, wd)
        # the bucket's words do not depend on the pair: step count, sum of squares, clip coefficient, norm (and the decay word)
        assert torch.equal(got["state"][:2], want["state"][:2]) and torch.equal(got["state"][3:5], want["state"][3:5])
        assert torch.equal(got["state"][8:], want["state"][8:])
        if ema:
            assert got["state"][5].item() == want["state"][5].item()
        if mult == 0.0:                                                      # torch's lr = 0 group: held, the moments move
            assert torch.equal(got["p"][idx], p0[idx])
            assert not torch.equal(got["m"][idx], _inputs(n)["m"][idx]) and not torch.equal(got["v"][idx], _inputs(n)["v"][idx])
    st = got["state"]
    assert st[0].item() == STEP0 + 1 and st[2].item() == f32(LR) and st[3].item() < 1.0     # clipping was active
    assert torch.isnan(st[6:8]).all() and (torch.isfinite(st[5]) if ema else torch.isnan(st[5]))
    assert torch.equal(got["g"], torch.zeros(n))                             # zero_grad = 1
    if not ema:
        assert torch.equal(got["ema"], _inputs(n)["ema"])                    # never touched


@pytest.mark.parametrize("name", ["255 every element its own segment", "2049 1024 segments of 1, 2, 3", "sweep + 3 ends at the sweep"])
def test_second_run_and_a_nan_tail_behind_the_table_give_the_same_bits(name):
    first = {ema: _grouped(name, ema) for ema in (False, True)}
    _grouped.cache_clear()
    for ema in (False, True):
        again, tailed = _grouped(name, ema), _grouped(name, ema, 7)
        for k in ("p", "m", "v", "g", "ema"):
            assert torch.equal(first[ema][k], again[k]) and torch.equal(first[ema][k], tailed[k]), (k, ema)
        assert torch.equal(first[ema]["state"][:5], again["state"][:5]) and torch.equal(first[ema]["state"][:5], tailed["state"][:5])


def test_kept_gradients_and_the_epoch_word():
    n, ends = TABLES["2049 odd offsets"]
    t = _device(n, LR)
    g0 = t["g"].clone()
    ep = torch.tensor([41], dtype=torch.int32, device="cuda")
    _groups_step(t, _table(ends, _values(len(ends))), len(ends), False, zero_grad=0, epoch=ep)
    assert torch.equal(t["g"], g0) and int(ep.item()) == 42
    assert torch.equal(t["p"].cpu(), _grouped("2049 odd offsets", False)["p"])


@pytest.mark.parametrize("name", list(TABLES))
def test_three_chained_steps_against_fp64(name):
    n, ends = TABLES[name]
    h = {k: f32(x) for k, x in HYPER.items()}
    lr = f32(LR)
    src = _inputs(n)
    t = _device(n, lr)
    rp, rm, rv = src["p"].double(), src["m"].double(), src["v"].double()
    gen = torch.Generator().manual_seed(99 + n % 9973)
    worst = {}
    for i in range(3):
        vals = _values(len(ends), shift=5 * i)                               # the table's values change between the steps
        g = torch.randn(n, generator=gen) * (1.5 + i)
        t["g"].copy_(g)
        rp, rm, rv, sumsq, clip, norm = ref_adamw_groups(rp, g, rm, rv, STEP0 + i, lr, h["b1"], h["b2"], h["eps"], h["max_norm"],
                                                         h["grad_scale"], ends, [a for a, _ in vals], [b for _, b in vals])
        _groups_step(t, _table(ends, vals), len(ends), False)
        assert t["state"][0].item() == STEP0 + i + 1
        errs = {k: ((t[k].cpu().double() - r).norm() / r.norm()).item() for k, r in (("p", rp), ("m", rm), ("v", rv))}
        errs["clip"] = abs(t["state"][3].item() - clip)
        for k, e in errs.items():
            worst[k] = max(worst.get(k, 0.0), e)
    for k, e in worst.items():
        print(f"ERR adamw_groups {name} n {n} {k} {e:.3e}")
    bad = {k: e for k, e in worst.items() if not e <= BOUND[k]}
    assert not bad, bad


@pytest.mark.parametrize("bad", ["n_seg 0", "n_seg 1025", "null ends", "null multipliers", "null decays", "null ema"])
def test_argument_errors_launch_nothing(bad):
    n, ends = TABLES["2049 odd offsets"]
    t = _device(n, LR)
    before = {k: x.clone() for k, x in t.items()}
    end, mult, wd = _table(ends, _values(len(ends)))
    n_seg = {"n_seg 0": 0, "n_seg 1025": 1025}.get(bad, len(ends))
    table = (None if bad == "null ends" else end, None if bad == "null multipliers" else mult, None if bad == "null decays" else wd)
    h = HYPER
    args = (*_head(t), f32(h["max_norm"]), f32(h["grad_scale"]), 1, None, *table, n_seg)
    with pytest.raises(_hip.HipLibraryError, match="adamw_clip_groups"):
        if bad == "null ema":
            _hip.call("mm_adamw_clip_groups_ema", *args, None, 0.9, 1)
        else:
            _hip.call("mm_adamw_clip_groups", *args)
    torch.cuda.synchronize()
    for k in ("p", "m", "v", "g"):
        assert torch.equal(t[k], before[k])
    assert t["state"][0].item() == STEP0 and torch.isnan(t["state"][5:8]).all()


@pytest.mark.parametrize("ema_decay", [0.0, 0.9])
def test_fused_adamw_with_two_dict_groups_against_fp64(ema_decay):
    """five parameters (7, 300, 1025 | 33, 2 x 5 elements) in two groups - the second at a tenth of the rate without weight
    decay - for three steps, the base rate changed through every group's 'lr' after step 2; and the single-group optimizer
    built from the same tensors launches what it always did"""
    gen = torch.Generator().manual_seed(17)
    shapes, split = [(7,), (3, 100), (1025,), (33,), (2, 5)], 3
    lr, b1, b2, eps, wd = f32(2e-3), f32(0.9), f32(0.999), f32(1e-8), f32(0.05)
    init = [torch.randn(s, generator=gen) for s in shapes]
    params = [torch.nn.Parameter(x.cuda()) for x in init]
    opt = FusedAdamW([{"params": params[:split]}, {"params": params[split:], "lr_scale": f32(0.1), "weight_decay": 0.0}],
                     lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, max_grad_norm=1.0, ema_decay=ema_decay)
    n0 = sum(x.numel() for x in init[:split])
    ends, mults, wds = [n0, opt.bucket.n], [1.0, f32(0.1)], [wd, 0.0]
    assert opt._host_table() == (ends, mults, wds)
    calls = []
    real = _hip.call
    _hip.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        flat = lambda xs: torch.cat([x.detach().reshape(-1) for x in xs])
        rp = flat(init).double()
        rm, rv = torch.zeros_like(rp), torch.zeros_like(rp)
        worst = {}
        for step in range(3):
            if step == 2:
                lr = f32(5e-4)
                for gr in opt.param_groups:
                    gr["lr"] = lr
            opt.zero_grad()
            gs = [torch.randn(s, generator=gen) * (0.5 + step) for s in shapes]
            for q, g in zip(params, gs):
                q.grad = g.cuda()
            opt.step()
            rp, rm, rv, _, clip, norm = ref_adamw_groups(rp, flat(gs), rm, rv, step, lr, b1, b2, eps, 1.0, 1.0, ends, mults, wds)
            assert clip < 1.0 and abs(opt.last_grad_norm - norm) <= BOUND["norm_rel"] * norm
            b = opt.bucket
            for k, got, ref in (("p", b.p, rp), ("m", b.m, rm), ("v", b.v, rv)):
                worst[k] = max(worst.get(k, 0.0), ((got.cpu().double() - ref).norm() / ref.norm()).item())
            assert torch.equal(flat(params), b.p)                            # the parameters are views of the bucket
    finally:
        _hip.call = real
    for k, e in worst.items():
        print(f"ERR adamw_groups FusedAdamW ema_decay {ema_decay} {k} {e:.3e}")
    assert all(e <= BOUND[k] for k, e in worst.items()), worst
    update = "mm_adamw_clip_groups_ema" if ema_decay else "mm_adamw_clip_groups"
    assert calls == ["mm_sumsq", update] * 3
    single = FusedAdamW([torch.nn.Parameter(x.cuda()) for x in init], lr=lr, weight_decay=wd, ema_decay=ema_decay)
    for q in single.bucket.params:
        q.grad = torch.ones_like(q)
    _hip.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        del calls[:]
        single.step()
    finally:
        _hip.call = real
    assert calls == ["mm_sumsq", "mm_adamw_clip_ema" if ema_decay else "mm_adamw_clip"]
