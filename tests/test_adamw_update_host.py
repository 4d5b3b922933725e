"""`optim.adamw_update`, the one host call of the fused clip + AdamW step (CPU, with a recording stand-in for `_hip.call`):
for a scalar weight decay or a SegmentTable, with or without averaged weights, it emits exactly ``mm_sumsq`` and then the
one matching entry point, the arguments in the order of include/mmeeg_hip.h - as many as the header declares, each of the
declared kind - and `FusedAdamW.step` picks the plain kernel for one segment of multiplier 1."""
import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, optim

BETAS, EPS, MAX_NORM, GRAD_SCALE, WD = (0.8, 0.95), 1e-7, 1.5, 0.5, 0.02
EMA_DECAY, EMA_WARMUP = 0.99, False


@pytest.fixture
def calls(monkeypatch):
    out = []
    monkeypatch.setattr(_hip, "call", lambda name, *args: out.append((name, args)))
    return out


def _bucket(ema):
    return optim.FlatBucket([torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 3))], ema=ema)


def _check_kinds(name, args):
    sig = _hip.parse_header()[name]
    assert len(args) == len(sig), (name, len(args), sig)
    for a, c in zip(args, sig):
        if c == "p":
            assert a is None or isinstance(a, torch.Tensor), (name, a)
        elif c == "f":
            assert type(a) is float, (name, a)
        else:
            assert type(a) is int, (name, a)


def _same(got, want):
    assert len(got) == len(want)
    for a, w in zip(got, want):
        assert (a is w) if isinstance(w, torch.Tensor) or w is None else (type(a) is type(w) and a == w), (a, w)


@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("grouped", [False, True], ids=["scalar", "table"])
def test_sumsq_then_the_matching_entry_point_in_header_order(calls, grouped, ema):
    b = _bucket(ema)
    table = optim.SegmentTable([5, 11], [1.0, 0.1], [WD, 0.0], "cpu")
    epoch = torch.zeros(1, dtype=torch.int32)
    optim.adamw_update(b, BETAS, EPS, MAX_NORM, GRAD_SCALE, 1, epoch, table if grouped else WD, EMA_DECAY, EMA_WARMUP)
    want_name = {(False, False): "mm_adamw_clip", (False, True): "mm_adamw_clip_ema",
                 (True, False): "mm_adamw_clip_groups", (True, True): "mm_adamw_clip_groups_ema"}[grouped, ema]
    assert [name for name, _ in calls] == ["mm_sumsq", want_name]
    for name, args in calls:
        _check_kinds(name, args)
    _same(calls[0][1], [b.g, b.state, b.n])
    head = [b.p, b.g, b.m, b.v, b.state, b.n, BETAS[0], BETAS[1], EPS]
    tail = [MAX_NORM, GRAD_SCALE, 1, epoch]
    want = head + ([] if grouped else [WD]) + tail + ([table.end, table.mult, table.wd, 2] if grouped else [])
    want += [b.ema, EMA_DECAY, 0] if ema else []
    _same(calls[1][1], want)
    sigs = _hip.parse_header()
    assert sigs[want_name] == "ppppplfff" + ("" if grouped else "f") + "ffip" + ("pppi" if grouped else "") + ("pfi" if ema else "")


@pytest.mark.parametrize("ema_decay", [0.0, 0.9])
def test_fused_adamw_step_goes_through_it(calls, monkeypatch, ema_decay):
    """a plain list, and groups that make one segment of multiplier 1: the plain entry point with the one decay; anything
    else: the table, built once and rewritten in place"""
    monkeypatch.setattr(optim.ops, "weights_changed", lambda: None)
    suffix = "_ema" if ema_decay else ""
    ps = [torch.nn.Parameter(torch.randn(4)), torch.nn.Parameter(torch.randn(3))]
    opt = optim.FusedAdamW([{"params": ps[:1]}, {"params": ps[1:]}], lr=1e-3, weight_decay=0.05, max_grad_norm=2, ema_decay=ema_decay)
    opt.step()
    assert [name for name, _ in calls] == ["mm_sumsq", "mm_adamw_clip" + suffix]
    args = calls[1][1]
    _check_kinds(*calls[1])
    assert args[9] == 0.05 and args[10:14] == (2.0, 1.0, 0, None)
    del calls[:]
    opt.param_groups[1]["lr_scale"] = 0.5
    opt.step()
    opt.param_groups[1]["weight_decay"] = 0.0
    opt.step()
    assert [name for name, _ in calls] == ["mm_sumsq", "mm_adamw_clip_groups" + suffix] * 2
    for name, args in calls:
        _check_kinds(name, args)
    t = opt._table
    assert calls[1][1][13:17] == (t.end, t.mult, t.wd, 2) and calls[3][1][13] is t.end      # the same device arrays
    assert t.ends == [4, 7] and t.mult.tolist() == [1.0, 0.5] and t.wd.tolist() == [torch.tensor(0.05).item(), 0.0]
