"""mm_adamw_clip_ema (csrc/optim.hip: adamw_kernel<true>, adamw_finish_kernel<true>) and the averaged-weights surface of
optim.FusedAdamW.

Exact by contract (torch.equal / ==): p, m, v, g and state[0..5) are mm_adamw_clip's bits on copies of the same inputs;
state[6..8) is never written (NaN canary); the shadow keeps its bits where it equals p; a second run's bits; the decay word
without warm-up; `averaged()` restores the live bits.
Bounds, none of them taken from the kernel's output:
  decay word state[5]   relative 2^-23 of the fp64 schedule: the integer sums 1 + t and 10 + t are exact in fp32, the
                        quotient is one rounding (2^-24 relative), doubled
  one step              |ema - ref64| <= 8 * 2^-24 * max(|p_new|, |ema_old|) elementwise, ref64 = e + (1 - d)(p - e) in fp64
                        with the d read back from state[5] and the kernel's own p: the rounding of 1 - d (<= 2^-25 absolute,
                        times |p - e| <= 2 M), of the difference (<= 2^-24 * 2 M) and of the fused multiply-add's result
                        (<= 2^-24 * M) add up to less than 4 * 2^-24 * M; doubled as margin
  t chained steps       the per-step error e_t obeys e_t <= d e_(t-1) + (one step's error), so it stays below
                        (one step's error) * min(t, 1 / (1 - d)): 8 * 2^-24 * M * min(t, 1 / (1 - d)), M the largest |p| or
                        |ema| met so far
ERR lines print the worst ratio error / bound of every case before it is asserted."""
import functools

import pytest
import torch

from multimodal_eeg_fmri_amd import _hip
from multimodal_eeg_fmri_amd.optim import FusedAdamW
from test_ema_host import ema_decay_schedule, ema_reference

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 2049, 2048 * 256 + 3]          # the last: a second, ragged grid-stride sweep of adamw_kernel
U = 2.0 ** -24
HYPER = dict(b1=0.9, b2=0.999, eps=1e-8, wd=0.02, max_norm=1.0, grad_scale=1.0)


def f32(x):
    return torch.tensor(float(x), dtype=torch.float32).item()


def _state(lr, step0=0):
    st = torch.zeros(8 + 1024, device="cuda")                               # MM_OPT_STATE_FLOATS
    st[0], st[2] = float(step0), lr
    st[5:8] = float("nan")
    return st


def _inputs(n, seed=0):
    gen = torch.Generator().manual_seed(7919 * seed + n % 9973)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 0.5
    m = torch.randn(n, generator=gen) * 0.1
    v = torch.rand(n, generator=gen) * 0.01
    shadow = p + torch.randn(n, generator=gen) * 0.3 + 0.05                 # different from p
    return p, g, m, v, shadow


def _step(t, ema=None, decay=0.0, warmup=0, zero_grad=1, wd=HYPER["wd"], epoch=None):
    """one optimizer step on the dict of device tensors `t` (the learning rate is state[2]); ema None: mm_adamw_clip"""
    h = HYPER
    n = t["p"].numel()
    _hip.call("mm_sumsq", t["g"], t["state"], n)
    args = (t["p"], t["g"], t["m"], t["v"], t["state"], n, f32(h["b1"]), f32(h["b2"]), f32(h["eps"]), f32(wd),
            f32(h["max_norm"]), f32(h["grad_scale"]), zero_grad, epoch)
    if ema is None:
        _hip.call("mm_adamw_clip", *args)
    else:
        _hip.call("mm_adamw_clip_ema", *args, ema, f32(decay), warmup)


def _device(n, seed, step0, lr=3e-3):
    p, g, m, v, shadow = _inputs(n, seed)
    return {"p": p.cuda(), "g": g.cuda(), "m": m.cuda(), "v": v.cuda(), "state": _state(f32(lr), step0)}, shadow


@functools.lru_cache(maxsize=None)
def _pair(n, step0=0, decay=0.999, warmup=1, seed=0):
    """the same inputs through mm_adamw_clip and through mm_adamw_clip_ema, one step each -> CPU results (computed once)"""
    plain, shadow0 = _device(n, seed, step0)
    fused, _ = _device(n, seed, step0)
    ema = shadow0.cuda()
    _step(plain)
    _step(fused, ema, decay, warmup)
    torch.cuda.synchronize()
    cpu = lambda t: {k: x.cpu() for k, x in t.items()}
    return cpu(plain), cpu(fused), shadow0, ema.cpu()


@pytest.mark.parametrize("n", SIZES)
def test_update_is_mm_adamw_clip_to_the_bit(n):
    plain, fused, _, _ = _pair(n)
    for k in ("p", "m", "v", "g"):
        assert torch.equal(plain[k], fused[k]), k
    assert torch.equal(fused["g"], torch.zeros(n))                          # zero_grad = 1
    assert torch.equal(plain["state"][:5], fused["state"][:5]) and fused["state"][0].item() == 1.0
    assert torch.equal(plain["state"][8:], fused["state"][8:])
    assert torch.isnan(fused["state"][6:8]).all() and torch.isnan(plain["state"][5:8]).all()
    assert torch.isfinite(fused["state"][5])


@pytest.mark.parametrize("n", SIZES)
def test_one_step_average_against_fp64(n):
    _, fused, shadow0, ema = _pair(n)
    d = fused["state"][5].double().item()
    ref = ema_reference(shadow0, fused["p"], d)
    bound = 8 * U * torch.maximum(fused["p"].abs(), shadow0.abs()).double()
    err = (ema.double() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"ERR adamw_ema one step n {n} worst err/bound {ratio:.3f} max err {err.max().item():.3e}")
    assert bool((err <= bound).all())
    assert not torch.equal(ema, shadow0)                                    # (the average did move)


@pytest.mark.parametrize("step0,warmup", [(0, 1), (7, 1), (9999, 1), (0, 0), (7, 0)])
def test_decay_word_follows_the_schedule(step0, warmup):
    """t = 1 and 8 lie below the cap 0.999 ((1 + t) / (10 + t) = 2/11, 1/2), t = 10 000 above it (10001 / 10010)"""
    decay = f32(0.999)
    _, fused, shadow0, ema = _pair(2049, step0, 0.999, warmup)
    want = ema_decay_schedule(step0, decay, bool(warmup))
    got = fused["state"][5].item()
    print(f"ERR adamw_ema decay word step0 {step0} warmup {warmup} got {got!r} want {want!r} rel {abs(got - want) / want:.3e}")
    assert fused["state"][0].item() == step0 + 1
    assert abs(got - want) <= 2.0 ** -23 * want
    if not warmup or step0 == 9999:
        assert got == decay                                                 # the cap itself: no arithmetic at all
    else:
        assert got < 0.6
    ref = ema_reference(shadow0, fused["p"], float(got))                    # and the average used THAT decay
    assert bool(((ema.double() - ref).abs() <= 8 * U * torch.maximum(fused["p"].abs(), shadow0.abs()).double()).all())


def test_twenty_chained_steps_against_the_fp64_recursion():
    n, d = 2049, f32(0.9)
    t, shadow0 = _device(n, 1, 0)
    ema = shadow0.cuda()
    ref = shadow0.double()
    gen = torch.Generator().manual_seed(11)
    M, worst = shadow0.abs().max().item(), 0.0
    for step in range(1, 21):
        t["g"].copy_(torch.randn(n, generator=gen) * 0.5)
        _step(t, ema, 0.9, 0)
        p = t["p"].cpu()
        assert t["state"][5].item() == d and t["state"][0].item() == step
        ref = ema_reference(ref, p, d)
        M = max(M, p.abs().max().item(), ema.abs().max().item())
        bound = 8 * U * M * min(step, 1.0 / (1.0 - d))
        err = (ema.cpu().double() - ref).abs().max().item()
        worst = max(worst, err / bound)
        assert err <= bound, (step, err, bound)
    print(f"ERR adamw_ema 20 chained steps worst err/bound {worst:.3f}")


def test_shadow_equal_to_p_stays_equal_to_the_bit():
    """lr = 0, weight_decay = 0: p keeps its bits, the difference p - ema is exactly 0 and the fused multiply-add returns
    ema itself, while m and v move"""
    n = 2049
    t, _ = _device(n, 2, 0, lr=0.0)
    p0 = t["p"].clone()
    ema = p0.clone()
    m0, v0 = t["m"].clone(), t["v"].clone()
    gen = torch.Generator().manual_seed(12)
    for step in range(5):
        t["g"].copy_(torch.randn(n, generator=gen))
        m_before = t["m"].clone()
        _step(t, ema, 0.9, 1, wd=0.0)
        assert torch.equal(t["p"], p0) and torch.equal(ema, p0)
        assert not torch.equal(t["m"], m_before)
    assert not torch.equal(t["m"], m0) and not torch.equal(t["v"], v0) and t["state"][0].item() == 5.0


def test_bit_reproducible():
    a = _pair(2048 * 256 + 3)
    _pair.cache_clear()
    b = _pair(2048 * 256 + 3)
    assert torch.equal(a[3], b[3]) and torch.equal(a[1]["p"], b[1]["p"])
    assert torch.equal(a[1]["state"][:6], b[1]["state"][:6])


@pytest.mark.parametrize("bad", ["null", "decay 1", "decay < 0"])
def test_argument_errors_launch_nothing(bad):
    t, shadow0 = _device(257, 3, 4)
    ema = shadow0.cuda()
    before = {k: x.clone() for k, x in t.items()}
    shadow, decay = {"null": (None, 0.9), "decay 1": (ema, 1.0), "decay < 0": (ema, -0.25)}[bad]
    with pytest.raises(_hip.HipLibraryError, match="adamw_clip_ema"):
        _hip.call("mm_adamw_clip_ema", t["p"], t["g"], t["m"], t["v"], t["state"], 257, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, 1,
                  None, shadow, decay, 1)
    torch.cuda.synchronize()
    for k in ("p", "m", "v"):
        assert torch.equal(t[k], before[k])
    assert t["state"][0].item() == 4.0 and torch.isnan(t["state"][5:8]).all() and torch.equal(ema.cpu(), shadow0)


def _fused_and_reference(ema_decay=0.9):
    gen = torch.Generator().manual_seed(7)
    shapes = [(7,), (3, 100), (1025,)]
    lr, b1, b2, eps, wd = f32(2e-3), f32(0.9), f32(0.999), f32(1e-8), f32(0.01)
    init = [torch.randn(s, generator=gen) for s in shapes]
    params = [torch.nn.Parameter(x.cuda()) for x in init]
    refs = [torch.nn.Parameter(x.double()) for x in init]
    opt = FusedAdamW(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, ema_decay=ema_decay)
    ropt = torch.optim.AdamW(refs, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    return gen, params, refs, opt, ropt


def test_fused_adamw_average_against_fp64_adamw_and_fp64_ema():
    """three parameters in one bucket, four steps, warm-up on (the default): the shadow against torch.optim.AdamW in
    fp64 followed by the fp64 average with the schedule's decay"""
    gen, params, refs, opt, ropt = _fused_and_reference(0.9)
    flat = lambda ps: torch.cat([q.detach().reshape(-1) for q in ps])
    assert torch.equal(opt.bucket.ema, opt.bucket.p) and opt.bucket.ema.data_ptr() != opt.bucket.p.data_ptr()
    ref = flat(refs).clone()
    M, worst = ref.abs().max().item(), 0.0
    for step in range(4):
        opt.zero_grad()
        for q, r in zip(params, refs):
            g = torch.randn(q.shape, generator=gen) * (0.3 + step)
            q.grad, r.grad = g.cuda(), g.double()
        ropt.step()
        opt.step()
        d = ema_decay_schedule(step, f32(0.9), True)
        assert abs(opt.bucket.state[5].item() - d) <= 2.0 ** -23 * d
        ref = ema_reference(ref, flat(refs), d)
        M = max(M, flat(refs).abs().max().item(), ref.abs().max().item())
        bound = 8 * U * M * min(step + 1, 1.0 / (1.0 - f32(0.9)))
        err = (opt.bucket.ema.cpu().double() - ref).abs().max().item()
        worst = max(worst, err / bound)
        assert err <= bound, (step, err, bound)
    print(f"ERR adamw_ema FusedAdamW 4 steps worst err/bound {worst:.3f}")


def test_averaged_exposes_the_average_through_the_parameter_views_and_restores_the_live_bits():
    gen, params, refs, opt, _ = _fused_and_reference(0.9)
    for step in range(2):
        opt.zero_grad()
        for q in params:
            q.grad = torch.randn(q.shape, generator=gen).cuda()
        opt.step()
    b = opt.bucket
    live, shadow = b.p.clone(), b.ema.clone()
    ptrs = [q.data_ptr() for q in params]
    assert not torch.equal(live, shadow)
    with opt.averaged():
        assert torch.equal(torch.cat([q.detach().reshape(-1) for q in params]), shadow)
        assert torch.equal(b.ema, live) and [q.data_ptr() for q in params] == ptrs
        with pytest.raises(RuntimeError, match="averaged"):
            opt.step()
    assert torch.equal(b.p, live) and torch.equal(b.ema, shadow) and [q.data_ptr() for q in params] == ptrs
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups", "ema"} and torch.equal(sd["ema"]["shadow"], shadow)
    opt.sync_ema()
    assert torch.equal(b.ema, live)
    opt.load_state_dict(sd)
    assert torch.equal(b.ema, shadow)
    plain = FusedAdamW([torch.nn.Parameter(torch.zeros(5, device="cuda"))])
    assert set(plain.state_dict()) == {"state", "param_groups"} and plain.bucket.ema is None
