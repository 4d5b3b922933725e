"""mm_sumsq + mm_adamw_clip (csrc/optim.hip: sumsq_kernel, adamw_kernel, adamw_finish_kernel) and optim.FusedAdamW against
ref_adamw, the fp64 restatement of the kernel file's header (tests/test_clip_loss_refs_host.py, checked there against
torch.optim.AdamW in fp64): every argument the entry points take, one at a time from a base case and all at once; sizes
around the grid caps (1024 x 256 elements per sweep of sumsq_kernel, 2048 x 256 of adamw_kernel: one element past each makes
the grid-stride loops take a second, ragged sweep); the learning rate through state[2]; a restored step counter; a small
bucket after a large one on the same state.  Three steps with a different gradient each, unless stated.  The kernels take
fp32 scalars, so the hyper-parameters are rounded to fp32 first and both sides see the same values.

ERR lines (worst over the steps of a case): p, m, v = rel-L2 against the fp64 trajectory; clip = absolute error of
state[3]; sumsq / norm = error of state[1] / state[4], absolute as for every scalar and (`_rel`) relative, because the values
run from 1e-1 (n = 1) to 3e6 (n = 524 365) and an absolute bound alone would check nothing at the small sizes.  Measured
worst cases on the MI355X and the bounds (2x .. 4x the worst; BOUND below):
  p          9.86e-8 (zero gradient, n = 1000)       3e-7     (tests/test_kernels_gpu.py asserts 2e-6)
  m          1.41e-7 (max_norm 10, n = 1000)         4e-7
  v          2.80e-7 (max_norm 10, n = 1000)         8e-7
  clip       1.32e-7 (grad_scale 1/3, n = 1000)      4e-7
  sumsq      7.57e-2 of 3.3e6 (n = 524 365)          0.2      sumsq_rel  6.88e-8 (n = 262 145)     2e-7
  norm       4.68e-5 of 1.3e3 (n = 262 145)          1.4e-4   norm_rel   1.12e-7 (grad_scale 1/3)  3.5e-7
Exact by contract, asserted with torch.equal / ==: step and epoch counters, a clip coefficient of 1, kept or zeroed
gradients, state[5..8) (never written: NaN canary), p under lr = 0, m = v = 0 under a zero gradient, a second run's bits."""
import math

import pytest
import torch

from multimodal_eeg_fmri_amd import _hip
from multimodal_eeg_fmri_amd.optim import FusedAdamW
from test_clip_loss_refs_host import ref_adamw

pytestmark = pytest.mark.gpu

SUMSQ_SWEEP, ADAMW_SWEEP = 1024 * 256, 2048 * 256
BOUND = {"p": 3e-7, "m": 4e-7, "v": 8e-7, "clip": 4e-7, "sumsq": 0.2, "sumsq_rel": 2e-7, "norm": 1.4e-4, "norm_rel": 3.5e-7}
assert BOUND["p"] <= 2e-6                                                    # tests/test_kernels_gpu.py's bound on p


def f32(x):
    return torch.tensor(float(x), dtype=torch.float32).item()


def _rel(a, b):
    return ((a.double() - b).norm() / b.norm()).item()


def _state(lr, step0=0):
    st = torch.zeros(8 + 1024, device="cuda")                               # MM_OPT_STATE_FLOATS
    st[0], st[2] = float(step0), lr
    st[5:8] = float("nan")                                                   # never written
    return st


def _drive(tag, n, steps=3, lrs=(3e-3,), betas=(0.9, 0.999), eps=1e-8, wd=0.02, max_norm=1.0, grad_scale=1.0,
           zero_grad=1, epoch=True, step0=0, moments=False, gmul=1.0, seed=0):
    """`steps` kernel steps next to the fp64 trajectory; prints the ERR lines, asserts the bounds and everything exact;
    -> (device tensors after the last step, the reference's clip coefficients)"""
    gen = torch.Generator().manual_seed(1000 * seed + n % 9973)
    b1, b2, eps, wd, max_norm, grad_scale = f32(betas[0]), f32(betas[1]), f32(eps), f32(wd), f32(max_norm), f32(grad_scale)
    p0 = torch.randn(n, generator=gen)
    m0 = torch.randn(n, generator=gen) * 0.1 if moments else torch.zeros(n)
    v0 = torch.rand(n, generator=gen) * 0.01 if moments else torch.zeros(n)
    rp, rm, rv = p0.double(), m0.double(), v0.double()
    p, m, v = p0.cuda(), m0.cuda(), v0.cuda()
    state = _state(lrs[0], step0)
    ep = torch.tensor([41], dtype=torch.int32, device="cuda") if epoch else None
    worst, clips = {}, []
    for i in range(steps):
        lr = f32(lrs[min(i, len(lrs) - 1)])
        state[2] = lr                                                        # the host's way to change the learning rate
        g = torch.randn(n, generator=gen) * ((0.5 + i) * gmul)
        gd = g.cuda()
        rp, rm, rv, sumsq, clip, norm = ref_adamw(rp, g, rm, rv, step0 + i, lr, b1, b2, eps, wd, max_norm, grad_scale)
        clips.append(clip)
        _hip.call("mm_sumsq", gd, state, n)
        _hip.call("mm_adamw_clip", p, gd, m, v, state, n, b1, b2, eps, wd, max_norm, grad_scale, zero_grad, ep)
        st = state[:8].cpu()
        assert st[0].item() == step0 + i + 1 and st[2].item() == lr and torch.isnan(st[5:8]).all()
        if ep is not None:
            assert int(ep.item()) == 41 + i + 1
        assert torch.equal(gd.cpu(), torch.zeros(n) if zero_grad else g)
        if clip == 1.0:
            assert st[3].item() == 1.0                                       # max_norm <= 0, or a norm below max_norm
        if norm == 0.0:
            assert st[4].item() == 0.0 and st[1].item() == 0.0
        errs = {"p": _rel(p.cpu(), rp), "m": _rel(m.cpu(), rm) if rm.norm() > 0 else m.abs().max().item(),
                "v": _rel(v.cpu(), rv) if rv.norm() > 0 else v.abs().max().item(),
                "clip": abs(st[3].item() - clip), "sumsq": abs(st[1].item() - sumsq), "norm": abs(st[4].item() - norm),
                "sumsq_rel": abs(st[1].item() - sumsq) / sumsq if sumsq else 0.0,
                "norm_rel": abs(st[4].item() - norm) / norm if norm else 0.0}
        for k, e in errs.items():
            worst[k] = max(worst.get(k, 0.0), e)
    for k, e in worst.items():
        print(f"ERR adamw {tag} n {n} {k} {e:.3e}")
    bad = {k: e for k, e in worst.items() if not e <= BOUND[k]}
    assert not bad, bad
    return {"p": p, "m": m, "v": v, "state": state[:8].clone(), "g": gd}, clips


@pytest.mark.parametrize("n", [1, 255, 257, 1000, SUMSQ_SWEEP + 1, ADAMW_SWEEP + 77])
def test_sizes(n):
    """one element, below and above one workgroup, one workgroup's trainer-test size, one past a full sweep of each grid"""
    _drive("size", n)


@pytest.mark.parametrize("max_norm", [0.0, -1.0, 1.0, 1e9])
def test_max_norm(max_norm):
    """<= 0: no clip (FusedAdamW's default); 1 with |g| ~ 16 .. 80: clipping; 1e9: a clip that is inactive"""
    _, clips = _drive(f"max_norm {max_norm}", 1000, max_norm=max_norm)
    assert all(c < 0.1 for c in clips) if max_norm == 1.0 else clips == [1.0, 1.0, 1.0]


@pytest.mark.parametrize("grad_scale", [1.0, 0.25, 1 / 3])
def test_grad_scale_enters_norm_and_update(grad_scale):
    """the 1 / world of a data-parallel run: state[4] = |g| grad_scale, and the clip is decided on THAT norm: |g| = 16, 47, 79
    against max_norm = 10 clips every step at scale 1 and leaves the first step alone at 0.25 and 1/3"""
    _, clips = _drive(f"grad_scale {grad_scale:.3f}", 1000, max_norm=10.0, grad_scale=grad_scale)
    assert [c == 1.0 for c in clips] == ([False] * 3 if grad_scale == 1.0 else [True, False, False])
    _drive(f"grad_scale {grad_scale:.3f} max_norm 1", 1000, grad_scale=grad_scale)


@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("epoch", [False, True])
def test_zero_grad_and_epoch_word(zero_grad, epoch):
    """zero_grad = 0 (FusedAdamW.step): g keeps its bits, 1: g is cleared; seed_epoch NULL or incremented once per step"""
    _drive(f"zero_grad {zero_grad} epoch {int(epoch)}", 257, zero_grad=zero_grad, epoch=epoch)


@pytest.mark.parametrize("kw", [dict(wd=0.0), dict(eps=1e-3), dict(betas=(0.8, 0.95)), dict(betas=(0.0, 0.5))],
                         ids=["wd0", "eps1e-3", "betas.8-.95", "betas0-.5"])
def test_hyper_parameters(kw):
    _drive(f"hyper {kw}", 1000, **kw)


def test_every_argument_changed_at_once():
    _, clips = _drive("all", SUMSQ_SWEEP + 1, lrs=(1e-2, 5e-4, 2e-3), betas=(0.8, 0.95), eps=1e-3, wd=0.0, max_norm=250.0,
                      grad_scale=1 / 3, zero_grad=0, epoch=False, step0=17, moments=True, seed=1)
    assert [c == 1.0 for c in clips] == [True, False, False]                 # |g| / 3 = 85, 256, 427


def test_learning_rate_through_state():
    """state[2] rewritten between the steps; with lr = 0 p keeps its bits while m, v and the step counter advance"""
    _drive("lr schedule", 1000, lrs=(3e-3, 1e-4, 2e-2))
    a, _ = _drive("lr 0 after 2", 1000, steps=2, seed=2)
    b, _ = _drive("lr 0 at 3", 1000, steps=3, lrs=(3e-3, 3e-3, 0.0), seed=2)
    assert torch.equal(a["p"], b["p"]) and b["state"][0].item() == 3.0
    assert not torch.equal(a["m"], b["m"]) and not torch.equal(a["v"], b["v"])


def test_resume_at_step_10000():
    """state[0] = 9999 with non-zero moments, as a checkpoint restores them: one step == the reference at t = 10000"""
    out, _ = _drive("resume", 1000, steps=1, step0=9999, moments=True, seed=3)
    assert out["state"][0].item() == 10000.0


def test_zero_gradient():
    """norm exactly 0, clip coefficient exactly 1 (1 / 1e-6 capped), m = v = 0: p changes by its decay only"""
    out, clips = _drive("zero gradient", 1000, gmul=0.0, seed=4)
    assert clips == [1.0, 1.0, 1.0]
    assert out["state"][4].item() == 0.0 and out["state"][3].item() == 1.0
    assert torch.count_nonzero(out["m"]).item() == 0 and torch.count_nonzero(out["v"]).item() == 0


def test_small_bucket_after_a_large_one():
    """mm_sumsq over 300 000 elements fills 1024 partial-sum slots; the next bucket of 100 elements writes one and must
    see the others cleared: state[1] and state[4] are those of the 100 elements"""
    gen = torch.Generator().manual_seed(5)
    state = _state(3e-3)
    big = (torch.randn(300_000, generator=gen) * 3).cuda()
    _hip.call("mm_sumsq", big, state, 300_000)
    torch.cuda.synchronize()
    assert torch.count_nonzero(state[8:]).item() == 1024
    n = 100
    g = torch.randn(n, generator=gen)
    p0 = torch.randn(n, generator=gen)
    p, m, v, gd = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), g.cuda()
    _hip.call("mm_sumsq", gd, state, n)
    _hip.call("mm_adamw_clip", p, gd, m, v, state, n, f32(0.9), f32(0.999), f32(1e-8), f32(0.02), 1.0, 1.0, 1, None)
    rp, rm, rv, sumsq, clip, norm = ref_adamw(p0, g, torch.zeros(n), torch.zeros(n), 0, f32(3e-3), f32(0.9), f32(0.999),
                                              f32(1e-8), f32(0.02), 1.0, 1.0)
    st = state[:8].cpu()
    errs = {"p": _rel(p.cpu(), rp), "m": _rel(m.cpu(), rm), "v": _rel(v.cpu(), rv), "clip": abs(st[3].item() - clip),
            "sumsq": abs(st[1].item() - sumsq), "sumsq_rel": abs(st[1].item() - sumsq) / sumsq,
            "norm": abs(st[4].item() - norm), "norm_rel": abs(st[4].item() - norm) / norm}
    for k, e in errs.items():
        print(f"ERR adamw stale n {n} {k} {e:.3e}")
    bad = {k: e for k, e in errs.items() if not e <= BOUND[k]}
    assert not bad, bad
    assert torch.count_nonzero(state[8:]).item() == 1 and st[0].item() == 1.0


def test_bit_reproducible():
    a, _ = _drive("twice", SUMSQ_SWEEP + 1, seed=6)
    b, _ = _drive("twice", SUMSQ_SWEEP + 1, seed=6)
    for k in ("p", "m", "v"):
        assert torch.equal(a[k], b[k])
    assert torch.equal(a["state"][:5], b["state"][:5]) and torch.isnan(a["state"][5:]).all()


@pytest.mark.parametrize("max_grad_norm", [0.0, 0.5])
def test_fused_adamw_surface(max_grad_norm):
    """optim.FusedAdamW over three parameters (7, 300, 1025 elements: one flat bucket) for four steps against fp64
    clip_grad_norm_ + torch.optim.AdamW, the learning rate changed through param_groups[0]['lr'] after step 2"""
    gen = torch.Generator().manual_seed(7)
    shapes = [(7,), (3, 100), (1025,)]
    lr, b1, b2, eps, wd = f32(2e-3), f32(0.9), f32(0.999), f32(1e-8), f32(0.01)
    init = [torch.randn(s, generator=gen) for s in shapes]
    params = [torch.nn.Parameter(x.cuda()) for x in init]
    refs = [torch.nn.Parameter(x.double()) for x in init]
    opt = FusedAdamW(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, max_grad_norm=max_grad_norm)
    ropt = torch.optim.AdamW(refs, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    worst = {}
    for step in range(4):
        if step == 2:
            opt.param_groups[0]["lr"] = ropt.param_groups[0]["lr"] = f32(5e-4)
        opt.zero_grad()
        for q, r in zip(params, refs):
            g = torch.randn(q.shape, generator=gen) * (0.3 + step)
            q.grad, r.grad = g.cuda(), g.double()
        norm = torch.linalg.vector_norm(torch.cat([r.grad.reshape(-1) for r in refs])).item()
        if max_grad_norm > 0:
            assert abs(torch.nn.utils.clip_grad_norm_(refs, max_grad_norm).item() - norm) <= 1e-12 * norm
        ropt.step()
        opt.step()
        b = opt.bucket
        assert b.state[0].item() == step + 1 and all(q.grad is None for q in params)
        if max_grad_norm <= 0:
            assert b.state[3].item() == 1.0
        rflat = lambda key: torch.cat([ropt.state[r][key].reshape(-1) for r in refs])
        errs = {"p": _rel(torch.cat([q.detach().reshape(-1) for q in params]).cpu(), torch.cat([r.detach().reshape(-1) for r in refs])),
                "m": _rel(b.m.cpu(), rflat("exp_avg")), "v": _rel(b.v.cpu(), rflat("exp_avg_sq")),
                "norm": abs(opt.last_grad_norm - norm), "norm_rel": abs(opt.last_grad_norm - norm) / norm}
        for k, e in errs.items():
            worst[k] = max(worst.get(k, 0.0), e)
    for k, e in worst.items():
        print(f"ERR adamw FusedAdamW max_grad_norm {max_grad_norm} {k} {e:.3e}")
    bad = {k: e for k, e in worst.items() if not e <= BOUND[k]}
    assert not bad, bad
