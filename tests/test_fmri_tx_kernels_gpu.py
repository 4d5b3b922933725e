"""GPU: the fMRI notebook's transformer encoders as one forward launch and one two-launch backward call
(csrc/fmri_tx.hip: "mm_tab_tx_fwd", "mm_tab_tx_bwd") against fp64 on the host.

Oracle at dropout 0: torch's own modules in double precision - the encoder's ``project``, ``nn.TransformerEncoder`` and
``norm`` containers, deep-copied with the same weights and called as the notebook calls them (train mode, so torch takes
its plain path).  At dropout > 0: a restatement (`_replica`) with an explicit `oracle.dropout_replica.keep_scale` mask at
each of the four sites of a layer (attention: one value per (row, head), index b * 4 + head; dropout1 / dropout2: b * H + f;
FFN middle: b * 4H + f; seeds in layer order then site order, stack by stack), differentiated by torch autograd in fp64;
with every mask off the restatement must be torch's function (asserted to 1e-12).  Loss = sum(feat * R) per stack with a
fixed random R; every parameter is moved off its initial value first.

Tolerances are those of the fp32 head family (tests/test_fmri_tab_kernels_gpu.py): outputs rtol 1e-4 / atol 1e-5, d x
rtol 1e-3 / atol 1e-5, parameter gradients rtol 2e-3 / atol 2e-5; a gradient tensor whose fp64 norm is below 1e-5 is
compared with the atol alone.  WHICH tensors those are is asserted: the query / key rows of every ``in_proj_weight`` /
``in_proj_bias`` (torch leaves rounding noise there; the kernel must write exact zeros) and nothing else."""
import copy

import pytest
import torch
import torch.nn.functional as F

from multimodal_eeg_fmri_amd import _hip, autograd, ops
from multimodal_eeg_fmri_amd import small_autograd as sa
from multimodal_eeg_fmri_amd.crossmodal_fmri_scr import ActivationEncoder
from oracle.dropout_replica import keep_scale

pytestmark = pytest.mark.gpu

ROW = ops.TAB_TX_ROW_TILE
# (B, in_dims per stack, H, L): B in {1, 8, row tile + 1}, in_dim in {1, 33, 131}, every H, L in {1, 3}, one and two stacks
CASES = [(1, (1,), 32, 1), (8, (33, 131), 64, 3), (ROW + 1, (131, 1), 128, 1), (8, (33,), 128, 3), (ROW + 1, (1, 33), 32, 3),
         (1, (131, 33), 64, 1)]


@pytest.fixture(autouse=True)
def _no_seed_epoch():
    ops.set_seed_epoch(None)
    yield
    ops.set_seed_epoch(None)


class Case:
    """one or two encoders with every parameter moved off its initial value, inputs and the loss's fixed random R"""
    _cache = {}

    def __init__(self, B, in_dims, H, L, p=0.0):
        self.B, self.in_dims, self.H, self.L, self.p = B, in_dims, H, L, p
        torch.manual_seed(700 + B + H + L + sum(in_dims))
        g = torch.Generator().manual_seed(17 + B + L)
        self.encs = [ActivationEncoder(L, d, H, p) for d in in_dims]
        with torch.no_grad():
            for e in self.encs:
                for q in e.parameters():             # zero biases and unit gammas hide terms
                    q.add_(torch.randn(q.shape, generator=g) * 0.05)
        self.xs = [torch.randn(B, d, generator=g) for d in in_dims]
        self.Rs = [torch.randn(B, H, generator=g) for _ in in_dims]
        self._dev = None

    @classmethod
    def get(cls, *key):
        if key not in cls._cache:
            cls._cache[key] = cls(*key)
        return cls._cache[key]

    @property
    def dev(self):
        if self._dev is None:
            self._dev = [copy.deepcopy(e).cuda().train() for e in self.encs]
        return self._dev

    def names(self, s):
        return [n for n, _ in self.encs[s].named_parameters()]


def _replica(e, x, seeds, p):
    """fp64 restatement of one encoder (module ``e`` in double) with explicit masks"""
    B, H = x.shape[0], e.hidden_dim
    ln = lambda t, m: F.layer_norm(t, (H,), m.weight, m.bias, 1e-5)       # noqa: E731
    ks = lambda seed, shape: keep_scale(seed, shape[0] * shape[1], p).view(shape).double()     # noqa: E731
    h = e.project(x)
    for l, layer in enumerate(e.transformer.layers):
        s = seeds[4 * l:4 * l + 4]
        W, b = layer.self_attn.in_proj_weight, layer.self_attn.in_proj_bias
        v = F.linear(h, W[2 * H:], b[2 * H:])
        keep = ks(s[0], (B, 4)).unsqueeze(-1).expand(B, 4, H // 4).reshape(B, H)
        att = layer.self_attn.out_proj(v * keep)
        h = ln(h + att * ks(s[1], (B, H)), layer.norm1)
        mid = torch.relu(layer.linear1(h)) * ks(s[2], (B, 4 * H))
        h = ln(h + layer.linear2(mid) * ks(s[3], (B, H)), layer.norm2)
    return ln(h, e.norm)


def _oracle(case, seeds=None):
    """``seeds`` None: torch's own modules (and the restatement with every mask off must agree with them)"""
    res = []
    n4 = 4 * case.L
    for s, (enc, x, R) in enumerate(zip(case.encs, case.xs, case.Rs)):
        e = copy.deepcopy(enc).double().train()
        x = x.double().requires_grad_(True)
        if seeds is None:
            assert all(layer.dropout.p == 0.0 for layer in e.transformer.layers)
            out = e.norm(e.transformer(e.project(x).unsqueeze(1)).squeeze(1))
            torch.testing.assert_close(_replica(e, x, [0] * n4, 0.0).detach(), out.detach(), rtol=0, atol=1e-12)
        else:
            out = _replica(e, x, seeds[s * n4:(s + 1) * n4], case.p)
        (out * R.double()).sum().backward()
        res.append(dict(out=out.detach(), dx=x.grad, grads={n: q.grad for n, q in e.named_parameters()}))
    return res


def _device(case, need_dx=True, dropout_seed=1234, fill=float("nan")):
    """the forward launch and the backward call from the case's state.  Gradient targets are pre-filled with ``fill``: the
    launch writes every element with a plain store."""
    encs = case.dev
    ops.set_dropout_seed(dropout_seed)
    with torch.no_grad():
        outs, sv = ops.tab_tx_forward_impl(encs, [x.cuda() for x in case.xs], True, True)
        bag = autograd.GradBag()
        tg = []
        for e in encs:
            tg.append({n: bag.target(q) for n, q in e.named_parameters()})
            for t in tg[-1].values():
                t.fill_(fill)
        dxs = sa.tab_tx_bwd(bag, sv, [R.cuda() for R in case.Rs], [need_dx] * len(encs))
    torch.cuda.synchronize()
    return [dict(out=o, dx=dx, grads=g) for o, dx, g in zip(outs, dxs, tg)], sv


def _qk(name, H):
    return slice(0, 2 * H) if name.endswith(("in_proj_weight", "in_proj_bias")) else None


def _compare(case, got, want):
    H = case.H
    for s, (g, w) in enumerate(zip(got, want)):
        torch.testing.assert_close(g["out"].cpu().double(), w["out"], rtol=1e-4, atol=1e-5)
        if g["dx"] is not None:
            torch.testing.assert_close(g["dx"].cpu().double(), w["dx"], rtol=1e-3, atol=1e-5)
        small = set()
        for n in case.names(s):
            have, ref = g["grads"][n].cpu().double(), w["grads"][n]
            qk = _qk(n, H)
            if qk is not None:                       # query / key rows: below the line in fp64, exact zeros on the device
                assert ref[qk].norm().item() < 1e-5, (n, ref[qk].norm().item())
                assert torch.count_nonzero(have[qk]).item() == 0, n
                torch.testing.assert_close(have[qk], ref[qk], rtol=0, atol=2e-5)
                have, ref = have[2 * H:], ref[2 * H:]
            if ref.norm().item() < 1e-5:
                small.add(n)
                torch.testing.assert_close(have, ref, rtol=0, atol=2e-5, msg=lambda m: f"stack {s} {n}: {m}")
            else:
                torch.testing.assert_close(have, ref, rtol=2e-3, atol=2e-5, msg=lambda m: f"stack {s} {n}: {m}")
        assert small == set(), small                 # nothing but the query / key rows falls under the atol-alone rule


@pytest.mark.parametrize("need_dx", [True, False])
@pytest.mark.parametrize("shape", CASES, ids=str)
def test_forward_and_every_gradient_against_fp64(shape, need_dx):
    case = Case.get(*shape)
    got, sv = _device(case, need_dx=need_dx)
    assert sv["seeds"] == []                         # dropout 0 draws nothing
    if not need_dx:
        assert all(g["dx"] is None for g in got)
    _compare(case, got, _oracle(case))


def test_qk_rows_are_written_as_zeros_over_garbage():
    case = Case.get(8, (33, 131), 64, 3)
    got, _ = _device(case, fill=123.25)
    H = case.H
    for s, g in enumerate(got):
        for n in case.names(s):
            t = g["grads"][n]
            assert not (t == 123.25).any().item(), n          # every element has a writer
            if _qk(n, H) is not None:
                assert torch.count_nonzero(t[:2 * H]).item() == 0 and torch.count_nonzero(t[2 * H:]).item() > 0, n


def test_no_save_writes_only_the_output():
    case = Case.get(ROW + 1, (131, 1), 128, 1)
    with torch.no_grad():
        outs, sv = ops.tab_tx_forward_impl(case.dev, [x.cuda() for x in case.xs], False, False)
    assert sv["save"] is None
    for o, w in zip(outs, _oracle(case)):
        torch.testing.assert_close(o.cpu().double(), w["out"], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("shape", [(8, (33, 131), 64, 3), (ROW + 1, (1,), 32, 1)], ids=str)
def test_dropout_forward_and_backward_equal_the_mask_replica(shape):
    case = Case.get(*shape, 0.3)
    got, sv = _device(case, dropout_seed=77)
    B, H, L, n = case.B, case.H, case.L, len(case.in_dims)
    assert len(sv["seeds"]) == n * 4 * L and len(set(sv["seeds"])) == n * 4 * L
    _compare(case, got, _oracle(case, seeds=sv["seeds"]))
    # the attention mask is one value per (row, head): the saved keep * v is zero over whole heads, and over those the
    # replica's mask says
    save = sv["save"].cpu().view(n, -1)
    for s in range(n):
        for l in range(L):
            mv = save[s, (1 + 9 * l) * B * H:(2 + 9 * l) * B * H].view(B, 4, H // 4)
            dropped = (mv == 0).all(dim=2)
            assert ((mv == 0).any(dim=2) == dropped).all()
            want = keep_scale(sv["seeds"][s * 4 * L + 4 * l], B * 4, 0.3).view(B, 4) == 0
            assert torch.equal(dropped, want)
    assert any((keep_scale(sd, B * 4, 0.3) == 0).any() for sd in sv["seeds"][::4])
    # another seed, another mask
    other, sv2 = _device(case, dropout_seed=78)
    assert sv2["seeds"] != sv["seeds"]
    assert not torch.equal(other[0]["out"], got[0]["out"])


def test_eval_draws_no_seed():
    case = Case.get(8, (33, 131), 64, 3, 0.3)
    enc = case.dev[0].eval()
    try:
        ops.set_dropout_seed(5)
        before = dict(ops._seed_state)
        with torch.no_grad():
            a = enc(case.xs[0].cuda())
            b = enc(case.xs[0].cuda())
        assert dict(ops._seed_state) == before
        assert torch.equal(a, b)
    finally:
        enc.train()


def test_save_flag_is_off_in_eval_and_under_no_grad(monkeypatch):
    case = Case.get(8, (33, 131), 64, 3, 0.3)
    enc, x = case.dev[0], case.xs[0].cuda()
    flags = []
    real = ops.tab_tx_forward_impl

    def spy(encs, xs, training, save):
        flags.append((bool(training), bool(save)))
        outs, sv = real(encs, xs, training, save)
        assert (sv["save"] is not None) == bool(save)
        return outs, sv

    monkeypatch.setattr(ops, "tab_tx_forward_impl", spy)
    try:
        enc(x)                                           # train mode, autograd on
        with torch.no_grad():
            enc(x)                                       # train mode under no_grad: dropout, but nothing saved
            enc.eval()
            enc(x)
        enc(x)                                           # eval mode on the tape (attribution, fine-tuning)
    finally:
        enc.train()
    assert flags == [(True, True), (True, False), (False, False), (False, True)]


def test_eval_mode_input_gradient_through_autograd():
    """tabular attribution: eval mode, only the input asks for a gradient"""
    case = Case.get(8, (33, 131), 64, 3)
    want = _oracle(case)
    for s, enc in enumerate(case.dev):
        enc.eval()
        try:
            x = case.xs[s].cuda().requires_grad_(True)
            out = enc(x)
            out.backward(case.Rs[s].cuda())
        finally:
            enc.train()
            for q in enc.parameters():
                q.grad = None
        torch.testing.assert_close(out.detach().cpu().double(), want[s]["out"], rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(x.grad.cpu().double(), want[s]["dx"], rtol=1e-3, atol=1e-5)


def test_two_calls_give_identical_bits():
    case = Case.get(ROW + 1, (1, 33), 32, 3, 0.3)
    a, _ = _device(case, dropout_seed=9)
    b, _ = _device(case, dropout_seed=9)
    for s, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u["out"], v["out"]) and torch.equal(u["dx"], v["dx"])
        for n in case.names(s):
            assert torch.equal(u["grads"][n], v["grads"][n]), n


def test_unsupported_shapes_are_refused_before_a_launch():
    import ctypes
    case = Case.get(8, (33,), 128, 3)
    enc = case.dev[0]
    x = case.xs[0].cuda()
    out = torch.full((8, 128), 7.0, device="cuda")
    ptab = ops.host_table([_hip._ptr(q) for q in ops.tab_tx_params(enc)], ctypes.c_void_p)
    for H, L in ((48, 3), (128, 0), (128, 9), (256, 3)):
        with pytest.raises(_hip.HipLibraryError, match="tab_tx_fwd"):
            _hip.call("mm_tab_tx_fwd", x, None, 1, 8, 33, 0, H, L, ctypes.addressof(ptab), out, None, None, 0.0, None, None)
        with pytest.raises(_hip.HipLibraryError, match="tab_tx_bwd"):
            _hip.call("mm_tab_tx_bwd", out, None, x, None, 1, 8, 33, 0, H, L, ctypes.addressof(ptab), ctypes.addressof(ptab),
                      out, out, None, None, 0.0, None, None)
    for bad in (dict(nstacks=3), dict(B=0), dict(in0=0)):
        a = dict(nstacks=1, B=8, in0=33)
        a.update(bad)
        with pytest.raises(_hip.HipLibraryError, match="tab_tx_fwd"):
            _hip.call("mm_tab_tx_fwd", x, None, a["nstacks"], a["B"], a["in0"], 0, 128, 3, ctypes.addressof(ptab), out, None, None,
                      0.0, None, None)
    torch.cuda.synchronize()
    assert (out == 7.0).all().item()                 # nothing was launched
    with pytest.raises(ValueError, match="hidden_dim"):
        ops.tab_tx_check(48, 2, [10])
    with pytest.raises(ValueError, match="num_layers"):
        ops.tab_tx_check(64, 0, [10])
    with pytest.raises(ValueError, match="num_layers"):
        ops.tab_tx_check(64, 9, [10])
    with pytest.raises(ValueError, match="in_dim"):
        ops.tab_tx_check(64, 2, [0])
    with pytest.raises(ValueError, match=r"\(B, 33\)"):
        ops.tab_tx_forward_impl([enc], [torch.zeros(8, 34, device="cuda")], False, False)
