"""Host side of the fMRI frame-sequence branch (no GPU): `LagAttentionPool` and `fMRISequenceEncoder3D` as modules, the
pool's CPU composition against the hand-written formulas in fp64, the "sequence" entry of the branch tables, its shape
checks and place in the step schedule, and the refusals that come before any launch."""
import math

import pytest
import torch

from multimodal_eeg_fmri_amd import ops
from multimodal_eeg_fmri_amd.bridge_branches import FMRI_BRANCHES, FMRI_SEQUENCE_BRANCH, fmri_branch, select_fmri, step_schedule
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs, synthetic_sequence_pairs
from multimodal_eeg_fmri_amd.fmri_utils import (LagAttentionPool, VolumeTransforms, fMRISequenceEncoder3D, fMRITabularEncoder,
                                                fMRIVolumeEncoder3D)


def test_constructors_validate_their_arguments():
    for frames in (0, 65, -1):
        with pytest.raises(ValueError, match="frames must be in 1..64"):
            LagAttentionPool(frames, 64)
        with pytest.raises(ValueError, match="frames must be in 1..64"):
            fMRISequenceEncoder3D(frames)
    for dim in (6, 0, 1028, 2):
        with pytest.raises(ValueError, match="multiple of 4 in 4..1024"):
            LagAttentionPool(3, dim)
        with pytest.raises(ValueError, match="multiple of 4 in 4..1024"):
            fMRISequenceEncoder3D(3, out_dim=dim)
    with pytest.raises(ValueError, match="widths must be"):
        fMRISequenceEncoder3D(3, widths=(32, 48, 128))
    pool = LagAttentionPool(64, 1024)
    assert pool.query.shape == (1024,) and pool.lag_bias.shape == (64,)
    assert not pool.query.any() and not pool.lag_bias.any()
    with pytest.raises(ValueError, match=r"expected \(B, 64, 1024\)"):
        pool(torch.zeros(2, 3, 1024))


def test_state_dict_keys_and_the_copy_of_a_volume_encoder():
    torch.manual_seed(0)
    vol = fMRIVolumeEncoder3D(1, 32, widths=(32, 32, 64), dropout=0.1).eval()
    with torch.no_grad():
        for p in vol.parameters():
            p.add_(torch.randn_like(p))
        vol.conv_layers[1].running_mean.normal_()
        vol.conv_layers[6].num_batches_tracked.fill_(7)
    seq = fMRISequenceEncoder3D.from_volume_encoder(vol, frames=5)
    assert list(seq.state_dict()) == [f"frame_encoder.{k}" for k in vol.state_dict()] + ["lag_pool.query", "lag_pool.lag_bias"]
    assert (seq.frames, seq.out_dim, seq.drop_p, seq.training) == (5, 32, 0.1, False)
    for k, v in vol.state_dict().items():
        got = seq.state_dict()[f"frame_encoder.{k}"]
        assert torch.equal(got, v) and got.data_ptr() != v.data_ptr(), k
    assert not seq.lag_pool.query.any() and not seq.lag_pool.lag_bias.any()
    assert fMRISequenceEncoder3D.from_volume_encoder(vol.train(), 2).training
    with pytest.raises(ValueError, match="1 input channel"):
        fMRISequenceEncoder3D.from_volume_encoder(fMRIVolumeEncoder3D(2, 32), 3)


def _by_hand(x, q, c, dout):
    """the formulas of DESIGN.md section 5x, written out with loops over b and f"""
    B, F, N = x.shape
    r = 1.0 / math.sqrt(N)
    out, a_all = torch.zeros(B, N, dtype=x.dtype), torch.zeros(B, F, dtype=x.dtype)
    dx, dq, dc = torch.zeros_like(x), torch.zeros_like(q), torch.zeros_like(c)
    for b in range(B):
        s = torch.stack([x[b, f] @ q * r + c[f] for f in range(F)])
        e = torch.exp(s - s.max())
        a = e / e.sum()
        a_all[b] = a
        out[b] = sum(a[f] * x[b, f] for f in range(F))
        da = torch.stack([dout[b] @ x[b, f] for f in range(F)])
        ds = a * (da - (a * da).sum())
        for f in range(F):
            dx[b, f] = a[f] * dout[b] + ds[f] * q * r
            dq += r * ds[f] * x[b, f]
        dc += ds
    return out, a_all, dx, dq, dc


@pytest.mark.parametrize("shape", [(1, 1, 8), (3, 4, 12), (5, 7, 64)])
def test_the_cpu_pool_is_the_hand_written_math_in_fp64(shape):
    B, F, N = shape
    g = torch.Generator().manual_seed(sum(shape))
    x, dout = torch.randn(B, F, N, generator=g, dtype=torch.float64), torch.randn(B, N, generator=g, dtype=torch.float64)
    pool = LagAttentionPool(F, N).double()
    with torch.no_grad():
        pool.query.copy_(torch.randn(N, generator=g, dtype=torch.float64))
        pool.lag_bias.copy_(torch.randn(F, generator=g, dtype=torch.float64))
    xg = x.clone().requires_grad_(True)
    out, w = pool(xg, return_weights=True)
    out.backward(dout)
    want = _by_hand(x, pool.query.detach(), pool.lag_bias.detach(), dout)
    for name, got, ref in zip(("out", "weights", "dx", "dq", "dc"), (out, w, xg.grad, pool.query.grad, pool.lag_bias.grad), want):
        assert (got.detach() - ref).abs().max().item() <= 1e-12, name
    assert torch.equal(pool(x), out.detach())


def test_the_pool_starts_as_the_mean_over_frames_and_the_query_learns_at_once():
    x = torch.randn(4, 6, 16, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    pool = LagAttentionPool(6, 16).double()
    out, w = pool(x, return_weights=True)
    assert torch.equal(w, torch.full((4, 6), 1 / 6, dtype=torch.float64))
    assert (out - x.mean(dim=1)).abs().max().item() <= 1e-15
    out.square().sum().backward()
    assert pool.query.grad.abs().max().item() > 0


def test_select_fmri_and_the_sequence_entry():
    seq = fMRISequenceEncoder3D(4, 64)
    b = select_fmri(seq, 64)
    assert b is FMRI_SEQUENCE_BRANCH and b is fmri_branch("sequence") and b.kind == "sequence"
    assert fmri_branch("volume") is FMRI_BRANCHES["volume"] and fmri_branch("tabular") is FMRI_BRANCHES["tabular"]
    assert b.can_be_longer and not b.augmentable and b.capture_words is None
    assert b.perturb_default == ("rows", 1) and b.perturb_kinds == ("rows", "blocks")
    assert b.perturb_shape("rows", (4, 8, 9, 10)) == (4, 720) and b.perturb_shape("blocks", (4, 8, 9, 10)) == (4, 8, 9, 10)
    assert b.checkpoint_tag(seq) == {"frames": 4}
    with pytest.raises(ValueError, match="fmri_dim=64 but the fMRISequenceEncoder3D ends in 32 features"):
        select_fmri(fMRISequenceEncoder3D(4, 32), 64)
    with pytest.raises(ValueError, match="fmri_dim=64 but the fMRISequenceEncoder3D ends in 32 features"):
        BridgeTrainer(eeg_channels=8, device="cpu", fmri_encoder=fMRISequenceEncoder3D(4, 32))


def test_the_branch_check_refuses_bad_batches_before_any_launch():
    seq = fMRISequenceEncoder3D(3, 64)
    check = FMRI_SEQUENCE_BRANCH.check
    check(seq, (2, 3, 4, 5, 6), True, "train_step")
    with pytest.raises(ValueError, match=r"train_step \(fMRI sequence encoder\): expected a \(B, F, D, H, W\) batch"):
        check(seq, (2, 3, 8, 8), True, "train_step")
    with pytest.raises(ValueError, match="pools F = 3 frames, the batch has 4"):
        check(seq, (2, 4, 8, 8, 8), True, "train_step")
    with pytest.raises(ValueError, match="every spatial extent must be >= 4"):
        check(seq, (2, 3, 8, 3, 8), False, "embed")
    tr = BridgeTrainer(eeg_channels=8, device="cpu", fmri_encoder=seq)
    eeg = torch.zeros(2, 8, 64)
    for call in (tr.train_step, tr.evaluate, tr.explain, tr.perturb, tr.predict):
        with pytest.raises(ValueError, match="pools F = 3 frames"):
            call(eeg, torch.zeros(2, 2, 8, 8, 8))
    with pytest.raises(ValueError, match="fmri_units must be"):
        tr.perturb(eeg, torch.zeros(2, 3, 8, 8, 8), fmri_units=("windows", 2))


def test_the_sequence_branch_in_the_step_schedule():
    assert step_schedule("erp", "sequence", (), (4, 32, 32, 32), True, {}).fmri_first is True
    assert step_schedule("erp", "sequence", (), (2, 32, 32, 32), True, {}).fmri_first is False
    s = step_schedule("erp", "sequence", (), (2, 32, 32, 32), True, {})
    assert s == step_schedule("erp", "volume", (), (1, 32, 32, 32), True, {})        # below the threshold: the volume branch's row
    assert step_schedule("erp", "sequence", (), (2, 32, 32, 32), True, {"MM_FMRI_LONGER": "1"}).fmri_first is True


def test_the_trainer_takes_a_sequence_encoder_and_refuses_volume_augmentation():
    torch.manual_seed(0)
    seq = fMRISequenceEncoder3D(3, 64, dropout=0.0)
    with pytest.raises(ValueError, match="fmri_augment augments .* same for all frames of a sample"):
        BridgeTrainer(eeg_channels=8, device="cpu", fmri_encoder=seq, fmri_augment=VolumeTransforms())
    tr = BridgeTrainer(eeg_channels=8, device="cpu", fmri_encoder=seq)
    assert tr._fmri_kind == "sequence" and tr.fmri_encoder is seq
    # the pool's two parameters are the tail of the fMRI encoder's bucket group: same group list, same ready points
    plain = BridgeTrainer(eeg_channels=8, device="cpu")
    assert [g[:2] for g in tr.groups] == [g[:2] for g in plain.groups]
    assert [g[2:] for g in tr.groups[:-1]] == [g[2:] for g in plain.groups[:-1]]
    assert tr.bucket.n == plain.bucket.n + 64 + 3 and tr.groups[-1][2:] == (tr.fmri_lo, tr.bucket.n)
    assert [id(p) for p in tr.bucket.params[-2:]] == [id(seq.lag_pool.query), id(seq.lag_pool.lag_bias)]
    assert tr._param_component[-2:] == ["fmri_encoder", "fmri_encoder"]
    ck = tr.checkpoint_state()
    assert ck["bridge_trainer_state"]["fmri_branch"] == {"kind": "sequence", "frames": 3}
    assert "fmri_branch" not in plain.checkpoint_state()["bridge_trainer_state"]     # the default container is unchanged
    other = BridgeTrainer(eeg_channels=8, device="cpu", fmri_encoder=fMRISequenceEncoder3D(2, 64, dropout=0.0))
    with pytest.raises(ValueError, match=r"fmri_branch differs: checkpoint \[kind='sequence', frames=3\], trainer \[kind='sequence', frames=2\]"):
        other.load_checkpoint_state(ck)
    with pytest.raises(ValueError, match=r"fmri_branch differs: checkpoint \[kind='sequence', frames=3\], trainer \[one fMRI item per pair"):
        plain.load_checkpoint_state(ck)
    tab = BridgeTrainer(eeg_channels=8, device="cpu", fmri_encoder=fMRITabularEncoder(4, 4))
    with pytest.raises(ValueError, match="fmri_branch differs"):
        tr.load_checkpoint_state(tab.checkpoint_state())


def test_lag_pool_ops_refuse_bad_shapes_before_any_launch(monkeypatch):
    from multimodal_eeg_fmri_amd import _hip
    monkeypatch.setattr(_hip, "call", lambda *a: pytest.fail("a launch was issued"))
    monkeypatch.setattr(_hip, "load", lambda: pytest.fail("the library was asked for"))
    for F, N, word in ((0, 8, "frames must be"), (65, 8, "frames must be"), (3, 6, "feature width"), (3, 1028, "feature width")):
        x = torch.zeros(2, F, N)
        with pytest.raises(ValueError, match=word):
            ops.lag_pool_fwd(x, torch.zeros(N), torch.zeros(F))
        with pytest.raises(ValueError, match=word):
            ops.lag_pool_bwd(torch.zeros(2, N), x, torch.zeros(2, F), torch.zeros(N))
        with pytest.raises(ValueError, match=word):
            ops.lag_pool(x, torch.zeros(N), torch.zeros(F))
    with pytest.raises(ValueError, match=r"expected \(B, F, N\)"):
        ops.lag_pool_fwd(torch.zeros(3, 8), torch.zeros(8), torch.zeros(3))
    with pytest.raises(ValueError, match="query must have N = 8"):
        ops.lag_pool_fwd(torch.zeros(2, 3, 8), torch.zeros(4), torch.zeros(3))
    with pytest.raises(ValueError, match="dout must be"):
        ops.lag_pool_bwd(torch.zeros(2, 4), torch.zeros(2, 3, 8), torch.zeros(2, 3), torch.zeros(8))
    with pytest.raises(ValueError, match="pools F = 3 frames"):
        ops._seq_forward_impl(fMRISequenceEncoder3D(3), torch.zeros(2, 4, 8, 8, 8), False)


def test_synthetic_sequence_pairs_plant_the_latent_in_one_frame():
    eeg, fmri = synthetic_sequence_pairs(6, 4, 2, 8, 64, (8, 8, 8), seed=5, device="cpu")
    e0, f0 = synthetic_pairs(6, 8, 64, (8, 8, 8), seed=5, device="cpu")
    assert eeg.shape == (6, 8, 64) and fmri.shape == (6, 4, 8, 8, 8) and torch.equal(eeg, e0)
    gm = torch.Generator().manual_seed(99)
    torch.randn(8, 16, generator=gm)
    A_f = torch.randn(512, 16, generator=gm) / 4.0
    z = torch.randn(6, 16, generator=torch.Generator().manual_seed(5))
    signal = (z @ A_f.t()).view(6, 8, 8, 8)
    corr = [torch.corrcoef(torch.stack([fmri[:, f].flatten(), signal.flatten()]))[0, 1].item() for f in range(4)]
    assert corr[2] > 0.5 and all(abs(corr[f]) < 0.1 for f in (0, 1, 3)), corr
    for bad in ((0, 0), (4, 4), (4, -1)):
        with pytest.raises(ValueError):
            synthetic_sequence_pairs(2, *bad, device="cpu")
