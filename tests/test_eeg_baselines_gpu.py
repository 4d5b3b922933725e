"""The EEG notebook's single-modality baselines (crossmodal_eeg_scr.py: ERPOnlyNet / PWOnlyNet) on the GPU: eval logits
against the notebook's own classes (tests/golden/g1_eeg_baselines.npz, tools/make_eeg_baseline_golden.py), train-mode
logits, loss, every parameter gradient and d / d input against a functional replica in fp64 with the conv / 1 x 1 operands
rounded to bf16 (straight-through; the avg tail pool-first in full precision, as the kernels compute it), the frozen-
BatchNorm tape of eval mode, the launches a step makes, and short FlexibleTrainer runs.

Shape: B = 8, C = 5, T = 44 (11 steps reach the tails; avg bins [0,3) [2,6) [5,9) [8,11)), widths 32 / 16.

These nets stack two MaxPool1d(2), a ReLU and (PWOnlyNet) a global arg-max: a near-tie flips a winner and moves a gradient
by 1e-1.  The seeds are therefore chosen so that the replica ITSELF is stable - run in fp32 and in fp64 (both with bf16
operands) its logits and all gradients agree to 1e-4 - and the tests assert that precondition.

Upper bounds are the project's for the same conv kernels (tests/test_models_gpu.py::test_a7_trimodal_lite_*: logits 3e-2,
gradients 8e-2, parameters with a gradient norm < 1e-5 skipped); the asserted ones are 4 x the values measured on MI355X,
listed in `MEASURED`.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import multimodal_eeg_fmri_amd.crossmodal_eeg_scr as Nb
from multimodal_eeg_fmri_amd import _hip, ops
from oracle.fixtures import build, seeded_randn

pytestmark = pytest.mark.gpu

B, C, T, OUT_DIM, HIDDEN = 8, 5, 44, 32, 16
MODELS = {"erponly": (Nb.ERPOnlyNet, 72), "pwonly": (Nb.PWOnlyNet, 71)}          # class, seed (stable: see the docstring)
LOGIT_CAP, GRAD_CAP = 3e-2, 8e-2                                                  # the project's bounds for bf16 conv encoders
# measured on MI355X: rel-L2 of (eval logits vs the golden, train logits, worst parameter gradient, d / d input,
# eval-mode d / d input) - the asserted bounds are min(cap, 4 x these)
MEASURED = {"erponly": dict(eval=2.08e-4, logits=6.9e-7, grad=5.15e-3, dx=4.11e-3, eval_dx=4.33e-3),
            "pwonly": dict(eval=8.47e-4, logits=5.6e-6, grad=5.71e-3, dx=4.30e-3, eval_dx=4.68e-3)}
# (worst gradients: erp_enc.bn1.weight / pw_enc.bn2.bias; the fp32 half - projection, head - sits at 1e-7 ... 1e-5.  Loss
# differences 2e-8 / 4e-7.  Eval + grad, worst parameter gradient 3.6e-3 / 4.8e-3.  Informational, against the pure-fp32
# golden: train logits 6.5e-3 / 1.8e-2, gradient norms within 1.3e-2 / 1.5e-2.)


def rel_err(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return ((got - want).norm() / want.norm().clamp_min(1e-30)).item()


def _bound(tag, key, cap):
    m = MEASURED[tag][key]
    return cap if m is None else min(cap, 4.0 * m)


def _net(tag, dropout=None):
    cls, seed = MODELS[tag]
    m = build(cls, seed, C, OUT_DIM, HIDDEN, 2)
    if dropout is not None:
        for q in m.modules():
            if isinstance(q, nn.Dropout):
                q.p = dropout
    return m


def _inputs(tag):
    seed = MODELS[tag][1]
    x = seeded_randn(seed + 100, B, C, T)
    y = torch.randint(0, 2, (B,), generator=torch.Generator().manual_seed(seed + 200))
    return x, y


def _call(m, tag, x):
    return m(erp=x) if tag == "erponly" else m(pw=x)


# ------------------------------------------------------------------ the replica
def _r(t):
    """bf16 rounding of a GEMM operand, straight-through for autograd, in the tensor's own dtype"""
    return t + (t.to(torch.bfloat16).to(t.dtype) - t).detach()


def _bn(h, sd, pre, train, dims):
    shape = [1, -1] + [1] * (h.dim() - 2)
    if train:
        mean, var = h.mean(dims), h.var(dims, unbiased=False)
    else:
        mean, var = sd[pre + "running_mean"], sd[pre + "running_var"]
    return (h - mean.view(shape)) / torch.sqrt(var.view(shape) + 1e-5) * sd[pre + "weight"].view(shape) + sd[pre + "bias"].view(shape)


def replica(sd, x, tag, train):
    erp = tag == "erponly"
    enc = "erp_enc." if erp else "pw_enc."
    h = x
    for i, pad in enumerate((3, 2, 1) if erp else (1, 1, 1), 1):
        h = F.conv1d(_r(h), _r(sd[enc + f"conv{i}.weight"]), sd[enc + f"conv{i}.bias"], padding=pad)
        h = torch.relu(_bn(h, sd, enc + f"bn{i}.", train, (0, 2)))
        if i < 3:
            h = F.max_pool1d(h, 2)
    if erp:                                  # bins averaged first, in full precision, then projected
        L = h.shape[2]
        spans = [((i * L) // 4, -((-(i + 1) * L) // 4)) for i in range(4)]
        xbin = torch.stack([h[:, :, a:e].mean(2) for a, e in spans], dim=2)                 # (B, 128, 4)
        pooled = torch.einsum("bki,pk->bpi", xbin, sd[enc + "step_proj.weight"][:, :, 0]) + sd[enc + "step_proj.bias"][None, :, None]
        pooled = pooled.flatten(1)
    else:
        pooled = F.conv1d(_r(h), _r(sd[enc + "proj.weight"]), sd[enc + "proj.bias"]).max(dim=2).values
    z = F.linear(pooled, sd["head.1.weight"], sd["head.1.bias"])
    z = F.gelu(_bn(z, sd, "head.2.", train, (0,)))
    return F.linear(z, sd["head.5.weight"], sd["head.5.bias"])


@functools.lru_cache(maxsize=None)
def _oracle(tag, train, dtype):
    """replica forward + backward in ``dtype`` -> (logits, loss, {parameter: gradient}, d / d input); computed once"""
    m = _net(tag)
    x, y = _inputs(tag)
    sd = {k: (v.detach().to(dtype).requires_grad_(True) if v.is_floating_point() else v) for k, v in m.state_dict().items()}
    xo = x.to(dtype).requires_grad_(True)
    logits = replica(sd, xo, tag, train)
    loss = F.cross_entropy(logits, y)
    loss.backward()
    grads = {k: v.grad.detach() for k, v in sd.items() if v.is_floating_point() and v.grad is not None}
    return logits.detach(), loss.detach(), grads, xo.grad.detach()


def _assert_replica_is_stable(tag, train):
    l32, _, g32, dx32 = _oracle(tag, train, torch.float32)
    l64, _, g64, dx64 = _oracle(tag, train, torch.float64)
    worst = max([rel_err(l32, l64), rel_err(dx32, dx64)] + [rel_err(g32[k], g64[k]) for k in g64 if g64[k].norm() >= 1e-5])
    assert worst < 1e-4, f"{tag}: the replica in fp32 and in fp64 differ by {worst:.2e}: a near-tie; choose another seed"


# ------------------------------------------------------------------------ tests
@pytest.mark.parametrize("tag", sorted(MODELS))
def test_eval_logits_vs_the_notebook_golden(golden, tag):
    fx = golden("g1_eeg_baselines.npz")
    assert int(fx[tag + "/seed"]) == MODELS[tag][1]
    m = _net(tag).eval().cuda()
    x, _ = _inputs(tag)
    with torch.no_grad():
        logits = _call(m, tag, x.cuda())
    assert logits.shape == (B, 2) and not logits.requires_grad
    e = rel_err(logits, torch.as_tensor(fx[tag + "/eval_logits"]))
    print(f"{tag} eval logits vs golden: {e:.3e}")
    assert e < _bound(tag, "eval", LOGIT_CAP)
    if tag == "erponly":                     # a time-major batch is transposed first, as in the notebook
        with torch.no_grad():
            assert torch.equal(m(erp=x.transpose(1, 2).contiguous().cuda()), logits)


@pytest.mark.parametrize("tag", sorted(MODELS))
def test_train_logits_loss_and_every_gradient_vs_the_replica(golden, tag):
    _assert_replica_is_stable(tag, True)
    logits_o, loss_o, grads_o, dx_o = _oracle(tag, True, torch.float64)
    m = _net(tag, dropout=0.0).train().cuda()
    x, y = _inputs(tag)
    xg = x.cuda().requires_grad_(True)
    logits = _call(m, tag, xg)
    loss = F.cross_entropy(logits, y.cuda())
    loss.backward()
    e_log = rel_err(logits, logits_o)
    errs = {}
    for n, p in m.named_parameters():
        w = grads_o.get(n)
        if w is None or w.norm() < 1e-5:
            continue
        assert p.grad is not None, n
        errs[n] = rel_err(p.grad, w)
    e_dx = rel_err(xg.grad, dx_o)
    worst = max(errs, key=errs.get)
    print(f"{tag} train vs replica: logits {e_log:.3e} loss {abs(loss.item() - loss_o.item()):.3e} "
          f"worst gradient {worst} {errs[worst]:.3e} d/dx {e_dx:.3e}")
    print("  " + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    fx = golden("g1_eeg_baselines.npz")         # informational: the pure-fp32 notebook run (bf16 emulation alone sits far from it)
    gn = dict(zip([str(k) for k in fx[tag + "/gnames"]], fx[tag + "/gnorms"]))
    print(f"  vs the fp32 golden (informational): logits {rel_err(logits, torch.as_tensor(fx[tag + '/train_logits'])):.3e} "
          f"worst gradient-norm ratio off by {max(abs(m.get_parameter(k).grad.norm().item() / v - 1) for k, v in gn.items() if v > 1e-5):.3e}")
    assert e_log < _bound(tag, "logits", LOGIT_CAP)
    assert abs(loss.item() - loss_o.item()) < 2e-2
    assert errs[worst] < _bound(tag, "grad", GRAD_CAP), (worst, errs[worst])
    assert e_dx < _bound(tag, "dx", GRAD_CAP)
    # the running statistics moved (momentum 0.1 from the perturbed start) and the batch counters advanced
    enc = m.erp_enc if tag == "erponly" else m.pw_enc
    assert int(enc.bn1.num_batches_tracked) == 1 and int(m.head[2].num_batches_tracked) == 1
    assert not torch.equal(enc.bn3.running_mean.cpu(), _net(tag).state_dict()[("erp_enc." if tag == "erponly" else "pw_enc.") + "bn3.running_mean"])


@pytest.mark.parametrize("tag", sorted(MODELS))
def test_eval_mode_with_grad_runs_the_frozen_tape(tag):
    _assert_replica_is_stable(tag, False)
    logits_o, _, grads_o, dx_o = _oracle(tag, False, torch.float64)
    m = _net(tag).eval().cuda()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    x, y = _inputs(tag)
    xg = x.cuda().requires_grad_(True)
    logits = _call(m, tag, xg)
    assert logits.requires_grad
    F.cross_entropy(logits, y.cuda()).backward()
    assert float(xg.grad.abs().max()) > 0
    e_log, e_dx = rel_err(logits, logits_o), rel_err(xg.grad, dx_o)
    errs = {n: rel_err(p.grad, grads_o[n]) for n, p in m.named_parameters() if grads_o[n].norm() >= 1e-5}
    worst = max(errs, key=errs.get)
    print(f"{tag} eval + grad vs frozen replica: logits {e_log:.3e} d/dx {e_dx:.3e} worst gradient {worst} {errs[worst]:.3e}")
    assert e_log < LOGIT_CAP and e_dx < _bound(tag, "eval_dx", GRAD_CAP) and errs[worst] < GRAD_CAP
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), f"{k} changed in eval mode"
    with torch.no_grad():                    # the folded launches compute the same function
        assert rel_err(_call(m, tag, x.cuda()), logits) < 2e-2


@pytest.mark.parametrize("tag", sorted(MODELS))
def test_a_train_step_runs_the_fused_tail_once_each_way(monkeypatch, tag):
    m = _net(tag).train().cuda()
    x, y = _inputs(tag)
    calls = []
    real = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    F.cross_entropy(_call(m, tag, x.cuda()), y.cuda()).backward()
    monkeypatch.setattr(_hip, "call", real)
    names = [n for n, _ in calls]
    fwd, bwd = ("mm_timepool_avg_fwd", "mm_timepool_avg_bwd") if tag == "erponly" else ("mm_timepool_max_fwd", "mm_timepool_max_bwd")
    assert names.count(fwd) == 1 and names.count(bwd) == 1
    assert not [n for n in names if n.startswith("mm_timepool") and n not in (fwd, bwd)]
    # no taps = 1 GEMM of the projection's width: (x, wf, B, T, cin, cout, taps, ...)
    assert not [a for n, a in calls if n == "mm_conv1d_fwd" and a[6] == 1 and a[5] == OUT_DIM]
    assert names.count("mm_conv1d_fwd") >= 3


def _toy_loader(tag, n=32, seed=5):
    """separable: the class shifts every channel's mean; 5-tuples through collate_trimodal, batches of 8"""
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(n) % 2
    erp = torch.randn(n, C, T, generator=g) + (y.float() * 2 - 1)[:, None, None] * 0.8
    pw = torch.randn(n, C, T, generator=g) + (y.float() * 2 - 1)[:, None, None] * 0.8
    conn = torch.zeros(n, 3)
    items = [(erp[i], pw[i], conn[i], i, int(y[i])) for i in range(n)]
    return [Nb.collate_trimodal(items[i:i + 8]) for i in range(0, n, 8)]


def _fit(tag, epochs=5):
    ops.set_dropout_seed(1234)
    torch.manual_seed(3)
    m = MODELS[tag][0](C, OUT_DIM, HIDDEN, 2)
    tr = Nb.FlexibleTrainer(m, lr=3e-3, modality=tag)
    loader = _toy_loader(tag)
    start = {k: v.detach().clone() for k, v in m.named_parameters()}
    losses = [tr.train_one_epoch(loader, grad_clip=1.0) for _ in range(epochs)]
    return tr, loader, start, losses


@pytest.mark.parametrize("tag", sorted(MODELS))
def test_flexible_trainer_fits_a_separable_set(tmp_path, tag):
    tr, loader, start, losses = _fit(tag)
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    for k, v in tr.model.named_parameters():
        assert not torch.equal(v.detach(), start[k]), f"{k} did not move"
    out = tr.evaluate(loader, 2)
    assert len(out) == 6
    metrics, targets, probs = out[0], out[1], out[2]
    assert set(metrics) >= {"Accuracy", "F1"} and probs.shape == (32, 2) and len(targets) == 32
    _, _, _, losses2 = _fit(tag)
    assert losses2 == losses, "two runs from the same seeds differ"
    path = str(tmp_path / f"best_{tag}_fold0.pt")
    tr.save_checkpoint(path, 4, metrics)
    fresh = Nb.FlexibleTrainer(MODELS[tag][0](C, OUT_DIM, HIDDEN, 2), lr=3e-3, modality=tag)
    epoch, got = fresh.load_checkpoint(path)                                   # load_state_dict is strict
    assert epoch == 4 and got["Accuracy"] == metrics["Accuracy"]
    for (k, a), (_, b) in zip(tr.model.state_dict().items(), fresh.model.state_dict().items()):
        assert torch.equal(a, b), k
    assert np.array_equal(fresh.evaluate(loader, 2)[2], probs)


@pytest.mark.parametrize("tag", sorted(MODELS))
def test_stand_alone_encoder_returns_every_step(tag):
    """ERPEncoder / PowerEncoder alone: (B, T / 4, out_dim) fp32 through the taps = 1 GEMM; pooling it on the host gives the
    net's own pooled features (eval mode), and a backward reaches the input"""
    m = _net(tag).eval().cuda()
    enc = m.erp_enc if tag == "erponly" else m.pw_enc
    x, _ = _inputs(tag)
    with torch.no_grad():
        steps = enc(x.cuda())
    assert steps.shape == (B, T // 4, OUT_DIM) and steps.dtype == torch.float32
    sd = {k: v.double() for k, v in _net(tag).state_dict().items()}
    pre = "erp_enc." if tag == "erponly" else "pw_enc."
    h = x.double()
    for i, pad in enumerate((3, 2, 1) if tag == "erponly" else (1, 1, 1), 1):
        h = torch.relu(_bn(F.conv1d(_r(h), _r(sd[pre + f"conv{i}.weight"]), sd[pre + f"conv{i}.bias"], padding=pad), sd, pre + f"bn{i}.", False, (0, 2)))
        h = F.max_pool1d(h, 2) if i < 3 else h
    name = "step_proj" if tag == "erponly" else "proj"
    want = F.conv1d(_r(h), _r(sd[pre + name + ".weight"]), sd[pre + name + ".bias"]).permute(0, 2, 1)
    assert rel_err(steps, want) < 2e-2
    xg = x.cuda().requires_grad_(True)
    enc.train()
    enc(xg).square().mean().backward()
    assert torch.isfinite(xg.grad).all() and float(xg.grad.abs().max()) > 0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in enc.parameters())
