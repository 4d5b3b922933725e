"""GPU: the tabular fMRI encoder as one forward and one backward launch (csrc/fmri_tab.hip: mm_fmri_tab_fwd,
mm_fmri_tab_bwd) against fp64 on the host.

Reference at dropout 0: `oracle.ref_functional.fmri_fusion_net(sd, act, conn, train=True)[1]`; at dropout > 0 a
restatement (`_replica`) with an explicit `oracle.dropout_replica.keep_scale` mask after each of the five BN-ReLU sites
(element index b * width + f, seeds in layer order a1, a2, c1, c2, f), differentiated by torch autograd in fp64; the
restatement with every mask off must be the oracle's function (asserted to 1e-12), and it also yields the batch
statistics the running buffers are checked against.  Loss = sum(fused * R) with a fixed random R; every parameter and
running statistic is moved off its initial value first.

Tolerances are those of this fp32 head family (tests/test_bridge_cls_kernels_gpu.py): outputs and statistics rtol 1e-4 /
atol 1e-5, d x rtol 1e-3 / atol 1e-5, parameter gradients rtol 2e-3 / atol 2e-5; a gradient tensor whose fp64 norm is
below 1e-5 is compared with the atol alone, and WHICH tensors those are is asserted per shape (`SMALL`): in train mode
every Linear bias (BatchNorm removes the batch mean: its gradient is rounding noise) and, on these inputs, nothing else -
at B = 2, where BatchNorm maps a feature's two rows to nearly -1 / +1 whatever they were, the gradients in front of it
are small but their fp64 norms stay above the line."""
import pytest
import torch
import torch.nn.functional as F

from multimodal_eeg_fmri_amd import _hip, autograd, ops
from multimodal_eeg_fmri_amd.fmri_utils import fMRIFusionNet, fMRITabularEncoder
from oracle import ref_functional as RF
from oracle.dropout_replica import keep_scale

pytestmark = pytest.mark.gpu

SHAPES = [(2, 7, 3, 32), (5, 1, 1, 128), (8, 100, 200, 64), (33, 130, 1225, 64), (256, 64, 64, 64)]
FROZEN_SHAPES = [(1, 7, 3, 32), (300, 37, 50, 64)]
_ENC = ("activation_encoder.encoder.", "connectivity_encoder.encoder.")
LAYERS = [(_ENC[0] + "0.", _ENC[0] + "1."), (_ENC[0] + "4.", _ENC[0] + "5."), (_ENC[1] + "0.", _ENC[1] + "1."),
          (_ENC[1] + "4.", _ENC[1] + "5."), ("fusion.0.", "fusion.1.")]
BIASES = {lin + "bias" for lin, _ in LAYERS}
# gradient tensors whose fp64 norm is below 1e-5 (train mode, dropout 0), from the fp64 oracle alone
SMALL = {
    (2, 7, 3, 32): BIASES,
    (5, 1, 1, 128): BIASES,
    (8, 100, 200, 64): BIASES,
    (33, 130, 1225, 64): BIASES,
    (256, 64, 64, 64): BIASES,
}


@pytest.fixture(autouse=True)
def _no_seed_epoch():
    ops.set_seed_epoch(None)
    yield
    ops.set_seed_epoch(None)


class Case:
    """an `fMRIFusionNet` with every parameter and running statistic moved off its initial value, the
    `fMRITabularEncoder` copied from it on the device, an input and the loss's fixed random R"""

    def __init__(self, shape, p=0.0, seed=0):
        B, A, C, H = shape
        self.shape, self.p = shape, p
        torch.manual_seed(300 + seed + B + A)
        net = fMRIFusionNet(A, C, hidden_dim=H, dropout=p)
        g = torch.Generator().manual_seed(11 + seed)
        with torch.no_grad():
            for q in net.parameters():               # zero-mean biases, unit gammas and equal fusion scalars hide terms
                q.add_(torch.randn(q.shape, generator=g) * 0.05)
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm1d):
                    m.running_mean.copy_(torch.rand(m.running_mean.shape, generator=g) - 0.5)
                    m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
                    m.num_batches_tracked.fill_(3)
        self.net = net
        self.sd = {k: v.clone() for k, v in net.state_dict().items()}
        self._enc = None
        self.x = torch.randn(B, A + C, generator=g)
        self.R = torch.randn(B, H, generator=g)

    @property
    def enc(self):
        if self._enc is None:
            self._enc = fMRITabularEncoder.from_fusion_net(self.net).cuda().train()
            self.reset()
        return self._enc

    def reset(self):
        self.enc.load_state_dict(self.sd, strict=False)

    def sd64(self):
        return {k: (v.double().requires_grad_(True) if v.is_floating_point() else v.clone()) for k, v in self.sd.items()}


def _replica(sd, x, A, seeds, p, train):
    """fp64 restatement with explicit masks -> (fused, [(batch mean, unbiased batch var)] x 5 in layer order)"""
    stats = {}

    def layer(i, h):
        lin, bn = LAYERS[i]
        pre = F.linear(h, sd[lin + "weight"], sd[lin + "bias"])
        stats[i] = (pre.mean(0).detach(), pre.var(0, unbiased=True).detach() if pre.shape[0] > 1 else None)
        z = torch.relu(RF._bn(sd, bn, pre, train))
        return z * keep_scale(seeds[i], z.numel(), p).view(z.shape).double()
    a = layer(1, layer(0, x[:, :A]))
    c = layer(3, layer(2, x[:, A:]))
    w = torch.softmax(torch.stack([sd["activation_weight"], sd["connectivity_weight"]]), dim=0)
    fused = layer(4, torch.cat([a * w[0], c * w[1]], dim=1))
    return fused, [stats[i] for i in range(5)]


def _oracle(case, train=True, seeds=None):
    """``seeds`` None: every mask off -> RF.fmri_fusion_net (and the restatement must agree with it)"""
    B, A, C, H = case.shape
    sd = case.sd64()
    x = case.x.double().requires_grad_(True)
    fused, stats = _replica(sd, x, A, seeds or (0,) * 5, case.p if seeds else 0.0, train)
    if seeds is None:
        ref = RF.fmri_fusion_net(sd, x[:, :A], x[:, A:], train=train)[1]
        torch.testing.assert_close(fused.detach(), ref.detach(), rtol=0, atol=1e-12)
        fused = ref
    (fused * case.R.double()).sum().backward()
    grads = {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in sd.items()
             if t.is_floating_point() and not k.startswith("head.") and "running" not in k}
    run = {}
    for (lin, bn), (mean, var) in zip(LAYERS, stats):
        rm, rv = case.sd[bn + "running_mean"].double(), case.sd[bn + "running_var"].double()
        run[bn + "running_mean"] = 0.9 * rm + 0.1 * mean if train else rm
        run[bn + "running_var"] = 0.9 * rv + 0.1 * var if train else rv
    return dict(out=fused.detach(), dx=x.grad, grads=grads, run=run)


def _device(case, training=True, dropout_seed=1234, sync=True):
    """the tape functions from the case's initial state: one forward launch, one backward launch.  Gradient targets are
    pre-filled with NaN: the launch writes every element with a plain store."""
    enc = case.enc
    case.reset()
    ops.set_dropout_seed(dropout_seed)
    with torch.no_grad():
        out, sv = ops._tab_forward_impl(enc, case.x.cuda(), training, True, need_dx=True)
        bag = autograd.GradBag()
        tg = {}
        for n, q in enc.named_parameters():
            tg[n] = bag.target(q)
            tg[n].fill_(float("nan"))
        dx = autograd.fmri_tab_bwd(bag, sv, case.R.cuda())
        bag.flush(out.device)
    if sync:
        torch.cuda.synchronize()
    return dict(out=out, dx=dx, grads=tg, save=sv["save"], seeds=sv["seeds"], sv=sv,
                state={k: v.clone() for k, v in enc.state_dict().items()})


def _compare(case, got, want, small=None, train=True):
    torch.testing.assert_close(got["out"].cpu().double(), want["out"], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(got["dx"].cpu().double(), want["dx"], rtol=1e-3, atol=1e-5)
    under = set()
    assert set(got["grads"]) == set(want["grads"])
    for n, g in got["grads"].items():
        w = want["grads"][n]
        assert torch.isfinite(g).all(), n
        tiny = w.norm().item() < 1e-5
        if tiny:
            under.add(n)
        torch.testing.assert_close(g.cpu().double(), w, rtol=0.0 if tiny else 2e-3, atol=2e-5, msg=lambda t, n=n: n + ": " + t)
    if small is not None:
        assert under == small, sorted(under ^ small)
    for k, w in want["run"].items():
        torch.testing.assert_close(got["state"][k].cpu().double(), w, rtol=1e-4, atol=1e-5, msg=lambda t, k=k: k + ": " + t)
    for _, bn in LAYERS:
        assert got["state"][bn + "num_batches_tracked"].item() == 3 + (1 if train else 0), bn
    assert case.enc.tickets("cuda")[:3].tolist() == [0, 0, 0]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_train_mode_equals_the_fp64_oracle_without_dropout(shape):
    case = Case(shape)
    _compare(case, _device(case), _oracle(case), small=SMALL[shape])


@pytest.mark.parametrize("shape", SHAPES[2:4], ids=lambda s: "x".join(map(str, s)))
def test_dropout_equals_the_fp64_replica_and_depends_on_the_seed(shape):
    case = Case(shape, p=0.3)
    got = _device(case)
    assert len(set(got["seeds"])) == 5 and 0 not in got["seeds"]
    _compare(case, got, _oracle(case, seeds=got["seeds"]))
    assert (got["out"] == 0).float().mean().item() > 0.3            # ReLU and the mask both zero elements
    other = _device(case, dropout_seed=4321)
    assert not torch.equal(other["out"], got["out"]) and not torch.equal(other["dx"], got["dx"])


@pytest.mark.parametrize("shape", FROZEN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_frozen_batchnorm_equals_the_fp64_oracle(shape):
    case = Case(shape, p=0.3)                                       # (a frozen forward draws no mask whatever p is)
    case.enc.eval()
    got = _device(case, training=False)
    assert got["seeds"] == (0,) * 5
    _compare(case, got, _oracle(case, train=False), train=False)
    for k, v in got["state"].items():                               # nothing is updated
        assert torch.equal(v.cpu(), case.sd[k]), k
    with torch.no_grad():                                           # the module's eval forward is the same launch
        assert torch.equal(case.enc(case.x.cuda()), got["out"])


def test_agrees_with_the_fusion_nets_own_train_path_on_the_gpu():
    """the independent on-GPU path: `fMRIFusionNet` in train mode (ops.fmri_fusion_forward, the small_autograd chain)"""
    case = Case(SHAPES[2])
    B, A, C, H = case.shape
    net = case.net.cuda().train()
    x, R = case.x.cuda(), case.R.cuda()
    _, fused = net(x[:, :A].contiguous(), x[:, A:].contiguous(), return_features=True)
    (fused * R).sum().backward()
    enc = case.enc
    case.reset()
    xg = x.clone().requires_grad_(True)
    out = enc(xg)
    (out * R).sum().backward()
    torch.cuda.synchronize()
    torch.testing.assert_close(out.detach(), fused.detach(), rtol=1e-4, atol=1e-5)
    ref = dict(net.named_parameters())
    for n, q in enc.named_parameters():
        assert q.grad is not None and ref[n].grad is not None, n
        torch.testing.assert_close(q.grad, ref[n].grad, rtol=2e-3, atol=2e-5, msg=lambda t, n=n: n + ": " + t)
    nsd = net.state_dict()
    for k, v in enc.state_dict().items():
        if "running" in k:
            torch.testing.assert_close(v, nsd[k], rtol=0, atol=1e-6, msg=lambda t, k=k: k + ": " + t)
        elif "num_batches" in k:
            assert v.item() == nsd[k].item() == 4


def test_two_runs_are_bit_identical_and_a_second_launch_follows_at_once():
    case = Case(SHAPES[3], p=0.3)
    a = _device(case)
    b = _device(case, sync=False)
    c = _device(case, sync=False)                                   # right behind b: the ticket words were left at zero
    torch.cuda.synchronize()
    for other in (b, c):
        for k in ("out", "dx", "save"):
            assert torch.equal(a[k], other[k]), k
        for n in a["grads"]:
            assert torch.equal(a["grads"][n], other["grads"][n]), n
        for k in a["state"]:
            assert torch.equal(a["state"][k], other["state"][k]), k
    assert case.enc.tickets("cuda")[:3].tolist() == [0, 0, 0]


def test_autograd_surface_is_the_tape_bit_for_bit():
    case = Case(SHAPES[2], p=0.3)
    tape = _device(case)
    case.reset()
    ops.set_dropout_seed(1234)
    enc = case.enc
    x = case.x.cuda().requires_grad_(True)
    out = enc(x)
    ps = list(enc.parameters())
    grads = torch.autograd.grad(out, [x] + ps, case.R.cuda())
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), tape["out"]) and torch.equal(grads[0], tape["dx"])
    for (n, _), g in zip(enc.named_parameters(), grads[1:]):
        assert torch.equal(g, tape["grads"][n]), n
    for k, v in enc.state_dict().items():
        assert torch.equal(v, tape["state"][k]), k


def test_each_direction_is_one_launch(monkeypatch):
    case = Case(SHAPES[0])
    names = []
    real = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    _device(case)
    assert names == ["mm_fmri_tab_fwd", "mm_fmri_tab_bwd"]


def test_unsupported_arguments_are_refused_before_any_launch():
    case = Case(SHAPES[0])
    enc, x = case.enc, case.x.cuda()
    with pytest.raises(ValueError, match="2 <= B <= 256"):
        enc(x[:1])
    with pytest.raises(ValueError, match=r"\(B, 10\)"):
        enc(x[:, :9])
    with pytest.raises(_hip.HipLibraryError, match="CPU tensor"):
        enc(case.x)
    enc.hidden_dim = 48                                             # (what the constructor refuses, forced past it)
    with pytest.raises(_hip.HipLibraryError, match="hidden_dim"):
        ops._tab_forward_impl(enc, x, True)
    torch.cuda.synchronize()
