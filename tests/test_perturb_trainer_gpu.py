"""GPU: BridgeTrainer.perturb - occlusion drops and permutation-sampled Shapley values of each pair's eval-mode cosine
similarity ze_i . zf_i, from forward scores alone (ops.perturb_scores, csrc/perturb.hip).

* occlusion with chunk_masks=1 agrees with the reference protocol written here on the trainer's public modules - clone,
  zero one channel / window / block, head.embed, (ze * zf).sum(1) - within rtol 1e-5, atol 1e-6 (the tolerance the existing
  tests give `scores` against that torch sum), for the ERP, Power and STFT encoders, the voxel encoder and a tabular one;
  "scores" equals explain(method="gradient")["scores"] within the same tolerance.  The loop calls the modules as the
  `explain` tests do (eval mode, autograd on): that is the forward `perturb` runs; `embed`'s no_grad forward differs
  from it by bf16 rounding (1.69e-5 in the similarity at this shape).
* chunking: chunk_masks=None (the memory rule) and 3 against 1.  The largest absolute difference of the drops, measured on
  the MI355X, is 0.0 for both modalities (every row of the big batch comes out with the bits it has in a batch of B), so the
  test asserts torch.equal; the figure is printed first.
* a channel whose first-layer weights are zero has an occlusion drop and a Shapley value of exactly 0.0.
* Shapley over the 4 windows of 64 samples with all 24 orders equals the textbook value computed in fp64 from the 16
  coalition scores, and sums to scores - empty_scores (efficiency) within the kernel test's bound.
* the same seed gives the same bits, another seed other values.
* train_step, perturb, train_step leaves the same bits as train_step, train_step (the assertion of the explain tests)."""
import itertools
import math

import pytest
import torch

from multimodal_eeg_fmri_amd import ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs, synthetic_tabular_pairs
from multimodal_eeg_fmri_amd.fmri_utils import fMRITabularEncoder

pytestmark = pytest.mark.gpu


def _trainer(kind="erp", C=8, **kw):
    import multimodal_eeg_fmri_amd.crossmodal_v4_enhancements as Cv
    import multimodal_eeg_fmri_amd.enhanced_models_v4 as E
    ops.set_seed_epoch(None)
    torch.manual_seed(0)
    enc = {"erp": None, "power": lambda: E.EnhancedPowerEncoder(C, dropout=0.3),
           "stft": lambda: Cv.MultiScaleSTFTPowerEncoder(C, dropout=0.3)}[kind]
    kw.setdefault("mode", "manual")
    return BridgeTrainer(eeg_channels=C, dropout=0.3, eeg_encoder=None if enc is None else enc(), **kw).train()


def _loop(tr, eeg, fmri, knock_eeg=(), knock_fmri=()):
    """the reference protocol on the public modules, one knocked-out unit per forward: -> (scores, drops_e, drops_f);
    ``knock_*``: functions that zero one unit of a clone in place.  The modules are called as the `explain` tests call
    them - eval mode, autograd on, the inputs asking for a gradient: the forward `explain` differentiates."""
    tr.eval()

    def score(e, f):
        ze, zf = tr.head.embed(tr.eeg_encoder(e.requires_grad_(True)), tr.fmri_encoder(f.requires_grad_(True)))
        return (ze * zf).sum(dim=1).detach()
    full = score(eeg.clone(), fmri.clone())
    de, df = [], []
    for knock in knock_eeg:
        e = eeg.clone()
        knock(e)
        de.append(full - score(e, fmri.clone()))
    for knock in knock_fmri:
        f = fmri.clone()
        knock(f)
        df.append(full - score(eeg.clone(), f))
    tr.train()
    return full, (torch.stack(de, dim=1) if de else None), (torch.stack(df, dim=1) if df else None)


def _zero_channel(c):
    def knock(e):
        e[:, c] = 0
    return knock


def _zero_window(k, w):
    def knock(e):
        e[..., k * w:(k + 1) * w] = 0
    return knock


def _zero_block(d, h, w, s):
    def knock(f):
        f[:, :, d * s:(d + 1) * s, h * s:(h + 1) * s, w * s:(w + 1) * s] = 0
    return knock


BLOCKS_8_OF_16 = [_zero_block(d, h, w, 8) for d in range(2) for h in range(2) for w in range(2)]       # unit (d * 2 + h) * 2 + w


@pytest.fixture(scope="module")
def erp_case():
    tr = _trainer("erp")
    eeg, fmri = synthetic_pairs(4, 8, 256, (16, 16, 16), seed=21)
    return tr, eeg, fmri


def test_occlusion_equals_the_loop_on_the_public_modules(erp_case):
    tr, eeg, fmri = erp_case
    full, de, df = _loop(tr, eeg, fmri, [_zero_channel(c) for c in range(8)], BLOCKS_8_OF_16)
    out = tr.perturb(eeg, fmri, fmri_units=("blocks", 8), chunk_masks=1)
    assert tr.training and set(out) == {"eeg", "fmri", "scores"}
    assert out["eeg"].shape == (4, 8) and out["fmri"].shape == (4, 8) and out["scores"].shape == (4,)
    assert all(t.dtype == torch.float32 and t.is_cuda for t in out.values())
    print("PERTURB_FIG occlusion vs loop: channels", (out["eeg"] - de).abs().max().item(), "blocks", (out["fmri"] - df).abs().max().item(),
          "largest drops", de.abs().max().item(), df.abs().max().item())
    assert de.abs().max().item() > 0 and df.abs().max().item() > 0
    torch.testing.assert_close(out["eeg"], de, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(out["fmri"], df, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(out["scores"], full, rtol=1e-5, atol=1e-6)
    assert torch.equal(tr.perturb(eeg, fmri, chunk_masks=1)["fmri"], out["fmri"])             # blocks of 8 are the default
    _, dw, _ = _loop(tr, eeg, fmri, [_zero_window(k, 64) for k in range(4)])
    win = tr.perturb(eeg, fmri, eeg_units=("windows", 64), chunk_masks=1)
    assert win["eeg"].shape == (4, 4)
    torch.testing.assert_close(win["eeg"], dw, rtol=1e-5, atol=1e-6)
    # the 'mean' baseline replaces a channel by the batch mean
    mean = tr.perturb(eeg, fmri, baseline="mean", chunk_masks=1)
    m = eeg.mean(dim=0, keepdim=True)

    def mean_channel(c):
        def knock(e):
            e[:, c] = m[:, c]
        return knock
    _, dm, _ = _loop(tr, eeg, fmri, [mean_channel(c) for c in range(8)])
    torch.testing.assert_close(mean["eeg"], dm, rtol=1e-5, atol=1e-6)


def test_scores_equal_the_scores_of_explain(erp_case):
    """"scores" is the number `explain` attributes: `perturb` runs the encoders through the forward `explain`
    differentiates (eval mode, autograd on).  The package's other eval forward - under ``torch.no_grad()``, as in `embed`:
    one kernel per convolution block, BatchNorm and bias folded into the GEMM epilogue (ops.conv_bn_act, save=False) -
    forms the values each block rounds to bf16 in another order; its similarities measured 1.69e-5 (absolute) / 6.82e-5
    (relative) away at this shape (printed below, not bounded)."""
    tr, eeg, fmri = erp_case
    got = tr.perturb(eeg, fmri, chunk_masks=1)["scores"]
    want = tr.explain(eeg, fmri, method="gradient")["scores"]
    print("PERTURB_FIG scores vs explain's scores: max abs", (got - want).abs().max().item(), "max rel", ((got - want).abs() / want.abs()).max().item())
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)
    ze, zf = tr.embed(eeg, fmri)
    print("PERTURB_FIG scores vs embed's similarities (recorded, not bounded): max abs", (got - (ze * zf).sum(dim=1)).abs().max().item())


@pytest.mark.parametrize("kind", ["power", "stft"])
def test_occlusion_with_the_other_eeg_encoders(kind):
    tr = _trainer(kind)
    eeg, fmri = synthetic_pairs(2, 8, 512 if kind == "stft" else 256, (16, 16, 16), seed=23)
    full, de, df = _loop(tr, eeg, fmri, [_zero_channel(c) for c in range(8)], BLOCKS_8_OF_16)
    out = tr.perturb(eeg, fmri, chunk_masks=1)
    assert de.abs().max().item() > 0
    torch.testing.assert_close(out["eeg"], de, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(out["fmri"], df, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(out["scores"], full, rtol=1e-5, atol=1e-6)


def test_occlusion_with_a_tabular_fmri_encoder():
    A, CF = 37, 50
    ops.set_seed_epoch(None)
    torch.manual_seed(0)
    tr = BridgeTrainer(eeg_channels=8, dropout=0.3, mode="manual", fmri_encoder=fMRITabularEncoder(A, CF, hidden_dim=64, dropout=0.3)).train()
    eeg, fmri = synthetic_tabular_pairs(4, 8, 128, A, CF, seed=25)
    full, de, df = _loop(tr, eeg, fmri, [_zero_channel(c) for c in range(8)], [_zero_window(k, 1) for k in range(A + CF)])
    out = tr.perturb(eeg, fmri, chunk_masks=1)                                   # windows of 1 feature are the default
    assert out["fmri"].shape == (4, A + CF) and df.abs().max().item() > 0
    torch.testing.assert_close(out["eeg"], de, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(out["fmri"], df, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(out["scores"], full, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        tr.perturb(eeg, fmri, fmri_units=("blocks", 8))


def test_chunking_leaves_the_drops_as_they_are(erp_case):
    """measured on the MI355X: the largest absolute difference of the drops between chunk_masks=1 and chunk_masks=3 / None
    is 0.0 for both modalities, so equality is asserted"""
    tr, eeg, fmri = erp_case
    one = tr.perturb(eeg, fmri, chunk_masks=1)
    for chunk in (None, 3):
        got = tr.perturb(eeg, fmri, chunk_masks=chunk)
        for k in ("eeg", "fmri"):
            print(f"PERTURB_FIG chunk_masks={chunk} vs 1: {k} max_abs_diff={(got[k] - one[k]).abs().max().item():.3e}")
        assert torch.equal(got["eeg"], one["eeg"]) and torch.equal(got["fmri"], one["fmri"]) and torch.equal(got["scores"], one["scores"])


def test_a_channel_the_model_cannot_see_gets_exactly_zero():
    tr = _trainer("erp")
    eeg, fmri = synthetic_pairs(4, 8, 256, (16, 16, 16), seed=27)
    with torch.no_grad():
        tr.eeg_encoder.conv_layers[0].weight[:, 2] = 0
    occ = tr.perturb(eeg, fmri, chunk_masks=1)
    shap = tr.perturb(eeg, fmri, method="shapley", n_permutations=3, seed=5, chunk_masks=1)
    for out in (occ, shap):
        assert (out["eeg"][:, 2] == 0).all(), out["eeg"][:, 2]
        others = torch.cat([out["eeg"][:, :2], out["eeg"][:, 3:]], dim=1)
        assert (others != 0).any(dim=1).all()


def test_shapley_over_all_orders_is_the_textbook_value():
    tr, U = _trainer("erp"), 4
    eeg, fmri = synthetic_pairs(4, 8, 256, (16, 16, 16), seed=29)
    orders = torch.tensor(list(itertools.permutations(range(U))))
    out = tr.perturb(eeg, fmri, method="shapley", eeg_units=("windows", 64), permutations={"eeg": orders}, n_permutations=2,
                     chunk_masks=1)
    assert set(out) == {"eeg", "fmri", "scores", "empty_scores"} and set(out["empty_scores"]) == {"eeg", "fmri"}
    assert out["eeg"].shape == (4, U) and out["fmri"].shape == (4, 8) and out["empty_scores"]["eeg"].shape == (4,)
    # the 16 coalition scores, mask s keeps window u iff bit u of s is set, at the same batch size
    masks = torch.tensor([[(s >> u) & 1 for u in range(U)] for s in range(1 << U)], dtype=torch.int32)
    br = tr.head.bridge
    tr.eval()

    def features(enc, x):                    # the forward `perturb` runs: eval mode, autograd on, the input asking for a gradient
        with torch.enable_grad():
            return enc(x.clone().requires_grad_(True)).detach()
    zf = ops.proj_embed_one(br, features(tr.fmri_encoder, fmri), "fmri")
    v = ops.perturb_scores(lambda rows: ops.perturb_pair_scores(ops.proj_embed_one(br, features(tr.eeg_encoder, rows), "eeg"), zf),
                           eeg, None, masks, ("windows", 64), chunk_masks=1).double().cpu()
    tr.train()
    assert torch.equal(v[(1 << U) - 1].float(), out["scores"].cpu()) and torch.equal(v[0].float(), out["empty_scores"]["eeg"].cpu())
    want = torch.zeros(4, U, dtype=torch.float64)
    for u in range(U):
        for s in range(1 << U):
            if not (s >> u) & 1:
                k = bin(s).count("1")
                want[:, u] += math.factorial(k) * math.factorial(U - k - 1) / math.factorial(U) * (v[s | (1 << u)] - v[s])
    print("PERTURB_FIG exact shapley max_abs_err", (out["eeg"].cpu().double() - want).abs().max().item(), "largest", want.abs().max().item())
    assert want.abs().max().item() > 0
    torch.testing.assert_close(out["eeg"].cpu().double(), want, rtol=1e-6, atol=1e-9)
    for k, n in (("eeg", U), ("fmri", 8)):
        phi = out[k].cpu().double()
        gap = out["scores"].cpu().double() - out["empty_scores"][k].cpu().double()
        scale = torch.maximum(phi.abs().max(dim=1).values, gap.abs())
        assert ((phi.sum(dim=1) - gap).abs() <= (n + 1) * 2.0 ** -24 * scale).all(), (k, phi.sum(dim=1) - gap, scale)


def test_the_seed_fixes_the_permutations(erp_case):
    tr, eeg, fmri = erp_case
    a = tr.perturb(eeg, fmri, method="shapley", n_permutations=2, seed=3)
    b = tr.perturb(eeg, fmri, method="shapley", n_permutations=2, seed=3)
    c = tr.perturb(eeg, fmri, method="shapley", n_permutations=2, seed=4)
    assert torch.equal(a["eeg"], b["eeg"]) and torch.equal(a["fmri"], b["fmri"]) and torch.equal(a["scores"], b["scores"])
    assert not torch.equal(a["eeg"], c["eeg"]) and not torch.equal(a["fmri"], c["fmri"])
    assert torch.equal(a["scores"], c["scores"]) and torch.equal(a["empty_scores"]["eeg"], c["empty_scores"]["eeg"])


@pytest.mark.parametrize("mode", ["graph", "manual"])
def test_perturb_between_two_steps_leaves_the_training_state_bit_for_bit(mode):
    batches = [synthetic_pairs(8, 8, 256, (16, 16, 16), seed=300 + i) for i in range(2)]

    def run(with_perturb):
        ops.set_seed_epoch(None)
        ops.set_dropout_seed(4242)
        tr = _trainer("erp", lr=1e-3, mode=mode)
        losses = [tr.train_step(*batches[0])["loss"].clone()]
        if with_perturb:
            torch.cuda.synchronize()
            b = tr.bucket
            before = [t.clone() for t in (b.p, b.g, b.m, b.v, b.state)] + [t.clone() for t in tr.buffers()]
            seeds = dict(ops._seed_state)
            cap = tr._cap
            for kw in (dict(method="occlusion", baseline="mean"), dict(method="shapley", n_permutations=2, eeg_units=("windows", 64))):
                out = tr.perturb(*batches[1], **kw)
                assert torch.isfinite(out["eeg"]).all() and torch.isfinite(out["fmri"]).all()
            torch.cuda.synchronize()
            after = [b.p, b.g, b.m, b.v, b.state] + list(tr.buffers())
            assert all(torch.equal(x, y) for x, y in zip(before, after))
            assert {k: v for k, v in ops._seed_state.items() if k != "epoch"} == {k: v for k, v in seeds.items() if k != "epoch"}
            assert ops._seed_state["epoch"] is seeds["epoch"] and tr._cap is cap and tr.training
            assert all(p.grad is None for p in tr.parameters())
        losses.append(tr.train_step(*batches[1])["loss"].clone())
        losses.append(tr.train_step(*batches[0])["loss"].clone())
        torch.cuda.synchronize()
        b = tr.bucket
        state = [t.clone() for t in (b.p, b.m, b.v, b.state)] + [t.detach().clone() for t in tr.buffers()]
        ops.set_seed_epoch(None)
        return torch.stack(losses), state
    l1, s1 = run(True)
    l2, s2 = run(False)
    assert torch.isfinite(l1).all() and torch.equal(l1, l2), (l1, l2)
    assert len(s1) == len(s2) and all(torch.equal(a, b) for a, b in zip(s1, s2))
