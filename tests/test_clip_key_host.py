"""Host side of the momentum key encoder (`BridgeTrainer(key_encoder=True)`, mm_clip_key_loss): the header declares the
entry points; the constructor names each missing partner before any allocation; `ops.clip_key_loss` refuses bad arguments
before any launch; the key twins are unregistered views into ``bucket.ema``; the checkpoint records ``key_encoder``; and
the fp64 oracle `ref_key` - which the kernel test holds the kernels against - is checked against itself: with k = q its loss
is the loss of `ref_bank` (the oracle of tests/test_clip_bank_kernels_gpu.py, restated here) and its dq is that oracle's
gradient with the key term removed."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from multimodal_eeg_fmri_amd import _hip, dp, ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer

KC = 64                                                   # the kernels' key chunk (csrc/clip_bank.hip)
POINTS = {"init": (10.0, False), "tau": (1 / 0.07, False), "trained": (30.0, True)}     # (s, correlated pairs): the bank test's
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


def _positives(gid, bank_gid, B, n):
    if gid is None:
        return torch.cat([torch.eye(B, dtype=torch.bool), torch.zeros(B, n, dtype=torch.bool)], dim=1)
    return gid[:, None] == torch.cat([gid, bank_gid[:n]])[None, :]


def _tops(xs, pos):
    tops, margin = [], math.inf
    for x in xs:
        best_pos, best_neg = torch.where(pos, x, NINF).max(1).values, torch.where(pos, NINF, x).max(1).values
        tops.append((best_pos >= x.max(1).values).double().mean())
        margin = min(margin, (best_pos - best_neg).abs().min().item())
    return tops, margin


def ref_key(q, k, gid, bank, bank_gid, n, ls):
    """the contract of mm_clip_key_loss in fp64 -> ((loss, top1 e->f, top1 f->e, d loss / d logit_scale), d loss / d q, the
    smallest top-1 margin).  k and the bank are constants: autograd differentiates w.r.t. q and logit_scale only."""
    q = q.double().clone().requires_grad_(True)
    lso = torch.tensor(float(ls), dtype=torch.float64, requires_grad=True)
    B, N = q.shape[0], q.shape[1] // 2
    k, bk = k.double(), bank[:n].double()
    xe = q[:, :N] @ torch.cat([k[:, N:], bk[:, N:]]).T      # e->f: qe_r over kf_t, [B][B + n]
    xf = q[:, N:] @ torch.cat([k[:, :N], bk[:, :N]]).T      # f->e: qf_r over ke_t
    pos = _positives(gid, bank_gid, B, n)
    s = lso.exp()
    l = sum(torch.logsumexp(s * x, 1) - torch.logsumexp(torch.where(pos, s * x, NINF), 1) for x in (xe, xf))
    loss = (0.5 * l).mean()
    dq, dls = torch.autograd.grad(loss, (q, lso))
    tops, margin = _tops((xe.detach(), xf.detach()), pos)
    return torch.stack([loss.detach(), tops[0], tops[1], dls]), dq, margin


def ref_bank(z, gid, bank, bank_gid, n, ls, key_term=True):
    """the oracle of mm_clip_bank_loss (tests/test_clip_bank_kernels_gpu.py), restated: the rows are queries AND keys.
    ``key_term`` False: the batch keys are detached copies - the gradient that is left is the query term."""
    z = z.double().clone().requires_grad_(True)
    lso = torch.tensor(float(ls), dtype=torch.float64, requires_grad=True)
    B, N = z.shape[0], z.shape[1] // 2
    bk = bank[:n].double()
    ze, zf = z[:, :N], z[:, N:]
    ke, kf = (ze, zf) if key_term else (ze.detach(), zf.detach())
    xe = ze @ torch.cat([kf, bk[:, N:]]).T
    xf = zf @ torch.cat([ke, bk[:, :N]]).T
    pos = _positives(gid, bank_gid, B, n)
    s = lso.exp()
    l = sum(torch.logsumexp(s * x, 1) - torch.logsumexp(torch.where(pos, s * x, NINF), 1) for x in (xe, xf))
    loss = (0.5 * l).mean()
    dz, dls = torch.autograd.grad(loss, (z, lso))
    tops, margin = _tops((xe.detach(), xf.detach()), pos)
    return torch.stack([loss.detach(), tops[0], tops[1], dls]), dz, margin


def _rows(n, N, correlated, gen):
    ze = F.normalize(torch.randn(n, N, generator=gen, dtype=torch.float64), dim=1)
    noise = F.normalize(torch.randn(n, N, generator=gen, dtype=torch.float64), dim=1)
    zf = F.normalize(0.9 * ze + math.sqrt(1 - 0.81) * noise, dim=1) if correlated else noise
    return torch.cat([ze, zf], dim=1)


def _key_rows(q, N, gen):
    """a slowly moving encoder's rows of the same pairs: each half of q turned a little and normalised again"""
    halves = [F.normalize(h + 0.3 * F.normalize(torch.randn(h.shape, generator=gen, dtype=torch.float64), dim=1), dim=1)
              for h in (q[:, :N], q[:, N:])]
    return torch.cat(halves, dim=1)


def _group_ids(B, K):
    """ids that repeat inside the batch (pairs), inside the bank (pairs) and across both (the bank cycles through the batch's
    ids and three more)"""
    gid = torch.arange(B) // 2 * 5 - 7
    bank_gid = (torch.arange(K) // 2) % ((B + 1) // 2 + 3) * 5 - 7
    return gid.to(torch.int32), bank_gid.to(torch.int32)


@functools.lru_cache(maxsize=None)
def key_case(N, B, K, point, grouped):
    """-> (q, k, gid, bank, bank_gid, ln s as the fp32 value the kernel reads, {fill: (state words, want4, dq)}); computed once
    and shared by every test that needs the case, on the host.  The seed: the first of a fixed sequence whose top-1
    decisions are unambiguous at every fill level (no score within 1e-4 of a tie between the best positive and the best
    negative), judged on the fp64 oracle alone."""
    s, correlated = POINTS[point]
    gid, bank_gid = _group_ids(B, K) if grouped else (None, None)
    ls = torch.tensor([math.log(s)]).float().item()
    for salt in range(16):
        gen = torch.Generator().manual_seed(N * 7919 + B * 131 + K + len(point) * 17 + int(grouped) + 100003 * salt + 5)
        q64 = _rows(B, N, correlated, gen)
        q, k, bank = q64.float(), _key_rows(q64, N, gen).float(), _rows(K, N, correlated, gen).float()
        refs, margin = {}, math.inf
        for fill in FILLS:
            words = fill_level(fill, B, K)
            want, dq, m = ref_key(q, k, gid, bank, bank_gid, words[1], ls)
            refs[fill], margin = (words, want, dq), min(margin, m)
        if margin > 1e-4:
            break
    assert margin > 1e-4, f"top-1 margin {margin:.2e} of case {(N, B, K, point, grouped)}: no seed of the sequence is unambiguous"
    return q, k, gid, bank, bank_gid, ls, refs


# ---------------------------------------------------------------- the oracle against itself
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
@pytest.mark.parametrize("N,B,K", [(16, 6, 8), (128, 6, 64), (16, 32, 200)])
def test_ref_key_with_k_equal_q_is_ref_bank_without_its_key_term(N, B, K, grouped):
    q, k, gid, bank, bank_gid, ls, refs = key_case(N, B, K, "tau", grouped)
    for fill, (words, _, _) in refs.items():
        n = words[1]
        want, dz, _ = ref_bank(q, gid, bank, bank_gid, n, ls)
        _, dz_query, _ = ref_bank(q, gid, bank, bank_gid, n, ls, key_term=False)
        got, dq, _ = ref_key(q, q, gid, bank, bank_gid, n, ls)
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-14)          # loss, both top-1 and d / d logit_scale
        torch.testing.assert_close(dq, dz_query, rtol=1e-12, atol=1e-14)
        assert (dq - dz).abs().max().item() > 1e-4                             # (the key term is not nothing)
        # and the closed form: dqe_r = sum_t G_e2f[r][t] kf_t with G = 0.5 s / B (softmax - [t in P] softmax over P)
        s = math.exp(ls)
        keys = torch.cat([q.double(), bank[:n].double()])
        x = q.double()[:, :N] @ keys[:, N:].T
        pos = _positives(gid, bank_gid, B, n)
        G = 0.5 * s / B * (torch.softmax(s * x, 1) - torch.softmax(torch.where(pos, s * x, NINF), 1))
        torch.testing.assert_close(dq[:, :N], G @ keys[:, N:], rtol=1e-10, atol=1e-13)


def test_ref_key_gives_the_keys_and_the_bank_no_gradient_and_sees_the_keys():
    q, k, gid, bank, bank_gid, ls, refs = key_case(16, 6, 8, "tau", True)
    want, dq, _ = refs["full"][1], refs["full"][2], None
    other, _, _ = ref_key(q, q, gid, bank, bank_gid, 8, ls)
    assert abs(other[0].item() - want[0].item()) > 1e-3                        # k != q changes the loss
    assert dq.shape == q.shape and torch.isfinite(dq).all()


# ---------------------------------------------------------------- header, ops, constructor
@pytest.fixture
def no_launch(monkeypatch):
    """any library call fails the test: the rules must raise before a launch"""
    def refuse(name, *a):
        raise AssertionError(f"{name} was called")
    monkeypatch.setattr(_hip, "call", refuse)


def _cpu_trainer(**kw):
    torch.manual_seed(0)
    return BridgeTrainer(eeg_channels=8, device="cpu", **kw)


def test_header_declares_the_entry_points_and_hip_maps_them():
    sigs = _hip.parse_header()
    assert sigs["mm_clip_key_loss"] == "p" * 10 + "iiii"           # q k gid bank bank_gid state logit_scale scal4 dq ws | B K N warmup
    assert sigs["mm_clip_key_ws_floats"] == "iiip"
    assert sigs["mm_clip_bank_loss"] == "p" * 9 + "iiii" and sigs["mm_clip_bank_push"] == "p" * 5 + "iii"      # unchanged


def test_ops_argument_checks_come_before_any_launch(no_launch):
    bank = ops.ClipBank(16, 4, False, "cpu")
    grouped = ops.ClipBank(16, 4, True, "cpu")
    q, ls, scal = torch.zeros(8, 8), torch.zeros(1), torch.zeros(4)
    ids = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(ValueError, match="one key row per pair"):
        ops.clip_key_loss(q, torch.zeros(6, 8), None, bank, ls, scal, None)
    with pytest.raises(ValueError, match="rows of 12 floats"):
        ops.clip_key_loss(torch.zeros(8, 12), torch.zeros(8, 12), None, bank, ls, scal, None)
    with pytest.raises(ValueError, match="carries no group ids"):
        ops.clip_key_loss(q, q, ids, bank, ls, scal, None)
    with pytest.raises(ValueError, match="carries group ids"):
        ops.clip_key_loss(q, q, None, grouped, ls, scal, None)
    with pytest.raises(ValueError, match="float32"):
        ops.clip_key_loss(q, q.double(), None, bank, ls, scal, None)
    with pytest.raises(ValueError, match="does not fit"):
        ops.clip_key_loss(torch.zeros(32, 8), torch.zeros(32, 8), None, bank, ls, scal, None)
    with pytest.raises(ValueError, match="warmup"):
        ops.clip_key_loss(q, q, None, bank, ls, scal, None, warmup=-1)


def test_constructor_names_each_missing_partner(no_launch, monkeypatch):
    with pytest.raises(ValueError, match=r"key_encoder=True needs bank_size > 0"):
        _cpu_trainer(key_encoder=True, ema_decay=0.99)
    with pytest.raises(ValueError, match=r"key_encoder=True needs ema_decay > 0"):
        _cpu_trainer(key_encoder=True, bank_size=64)
    with pytest.raises(ValueError, match=r"key_encoder=True needs loss='infonce'"):
        _cpu_trainer(key_encoder=True, bank_size=64, ema_decay=0.99, loss="sigmoid")
    monkeypatch.setattr(dp, "world_size", lambda group: 2 if group is not None else 1)
    with pytest.raises(ValueError, match=r"key_encoder=True needs a world size of 1"):
        _cpu_trainer(key_encoder=True, bank_size=64, ema_decay=0.99, group=object())
    assert _cpu_trainer()._key_encoder is False and _cpu_trainer()._key is None


def test_key_twins_are_unregistered_views_into_the_average(no_launch):
    kw = dict(bank_size=64, ema_decay=0.99)
    tr, plain = _cpu_trainer(key_encoder=True, **kw), _cpu_trainer(**kw)
    assert list(tr.state_dict()) == list(plain.state_dict())
    assert [tuple(p.shape) for p in tr.parameters()] == [tuple(p.shape) for p in plain.parameters()]
    assert tr.bucket.n == plain.bucket.n and tr.groups == plain.groups
    assert set(tr._key) == {"eeg_encoder", "fmri_encoder", "bridge"}
    b = tr.bucket
    pairs = [(tr.eeg_encoder, tr._key["eeg_encoder"]), (tr.fmri_encoder, tr._key["fmri_encoder"]),
             (tr.head.bridge.eeg_proj, tr._key["bridge"].eeg_proj), (tr.head.bridge.fmri_proj, tr._key["bridge"].fmri_proj)]
    for online, twin in pairs:
        assert not twin.training
        for (name, p), (tname, tp) in zip(online.named_parameters(), twin.named_parameters()):
            assert name == tname and tp is not p and not tp.requires_grad and not hasattr(tp, "_mm_grad") and tp.grad is None
            assert tp.data_ptr() - b.ema.data_ptr() == p.data_ptr() - b.p.data_ptr() and tp.shape == p.shape
        for (name, buf), (tname, tbuf) in zip(online.named_buffers(), twin.named_buffers()):
            assert name == tname and tbuf is buf                # the running statistics are the online module's own tensors
    b.ema.fill_(3.0)                                             # the twins see the average, the online modules the weights
    assert tr._key["eeg_encoder"].conv_layers[0].weight.min().item() == 3.0 and tr.eeg_encoder.conv_layers[0].weight.min().item() != 3.0
    frozen = _cpu_trainer(key_encoder=True, freeze=("fmri_encoder",), **kw)
    assert set(frozen._key) == {"eeg_encoder", "bridge"}         # a frozen encoder has no twin


def test_checkpoint_records_key_encoder_and_a_mismatch_raises(no_launch):
    kw = dict(bank_size=32, ema_decay=0.99)
    key, plain = _cpu_trainer(key_encoder=True, **kw), _cpu_trainer(**kw)
    assert key.checkpoint_state()["bridge_trainer_state"]["bank"]["key_encoder"] is True
    assert "key_encoder" not in plain.checkpoint_state()["bridge_trainer_state"]["bank"]      # the container is unchanged
    _cpu_trainer(key_encoder=True, **kw).load_checkpoint_state(key.checkpoint_state())
    with pytest.raises(ValueError, match=r"bank\.key_encoder differs"):
        _cpu_trainer(**kw).load_checkpoint_state(key.checkpoint_state())
    with pytest.raises(ValueError, match=r"bank\.key_encoder differs"):
        _cpu_trainer(key_encoder=True, **kw).load_checkpoint_state(plain.checkpoint_state())


def test_a_step_on_the_averaged_weights_is_refused(no_launch):
    tr = _cpu_trainer(key_encoder=True, bank_size=32, ema_decay=0.99, mode="manual")
    with tr.ema_weights():
        with pytest.raises(RuntimeError, match="ema_weights"):
            tr.train_step(torch.zeros(8, 8, 128), torch.zeros(8, 1, 16, 16, 16))
