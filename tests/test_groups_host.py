"""Host checks of subject-grouped positives (no GPU): group ids are validated before any launch, the id tail of a packed
host batch, and the synthetic subject data."""
import pytest
import torch

from multimodal_eeg_fmri_amd import ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_subject_pairs


def test_group_ids_are_validated_and_converted():
    assert ops.group_ids(None, 4) is None
    for dt in (torch.int64, torch.int16, torch.uint8, torch.int32):
        g = ops.group_ids(torch.tensor([3, 1, 3, 0], dtype=dt), 4)
        assert g.dtype == torch.int32 and g.tolist() == [3, 1, 3, 0]
    assert ops.group_ids(torch.tensor([-(2 ** 31), 2 ** 31 - 1]), 2).tolist() == [-(2 ** 31), 2 ** 31 - 1]
    with pytest.raises(ValueError, match="integer"):
        ops.group_ids(torch.zeros(4), 4)
    with pytest.raises(ValueError, match="integer"):
        ops.group_ids(torch.zeros(4, dtype=torch.bool), 4)
    with pytest.raises(ValueError, match="shape"):
        ops.group_ids(torch.zeros(5, dtype=torch.int64), 4)
    with pytest.raises(ValueError, match="shape"):
        ops.group_ids(torch.zeros(4, 1, dtype=torch.int64), 4)
    with pytest.raises(ValueError, match="int32"):
        ops.group_ids(torch.tensor([0, 2 ** 31]), 2)
    with pytest.raises(ValueError, match="int32"):
        ops.group_ids(torch.tensor([-(2 ** 31) - 1, 0]), 2)
    with pytest.raises(ValueError, match="torch.Tensor"):
        ops.group_ids([0, 1], 2)


def test_retrieval_group_arguments_are_checked_first():
    q, g = torch.zeros(4, 8), torch.zeros(6, 8)
    ids_q, ids_g = torch.arange(4), torch.arange(6)
    with pytest.raises(ValueError, match="both"):
        ops.retrieval(q, g, q_groups=ids_q)
    with pytest.raises(ValueError, match="both"):
        ops.retrieval(q, g, g_groups=ids_g)
    with pytest.raises(ValueError, match="exclusive"):
        ops.retrieval(q, g, torch.arange(4), q_groups=ids_q, g_groups=ids_g)
    with pytest.raises(ValueError, match="only ranks"):
        ops.retrieval(q, g, k=2, q_groups=ids_q, g_groups=ids_g)
    with pytest.raises(ValueError, match="only ranks"):
        ops.retrieval(q, g, ranks=False, q_groups=ids_q, g_groups=ids_g)


def test_trainer_refuses_bad_ids_before_any_launch():
    tr = BridgeTrainer(eeg_channels=8, device="cpu", mode="manual")
    eeg, fmri = torch.zeros(4, 8, 64), torch.zeros(4, 1, 16, 16, 16)
    for bad in (torch.zeros(4), torch.zeros(3, dtype=torch.int64), torch.tensor([0, 1, 2, 2 ** 40])):
        with pytest.raises(ValueError):
            tr.train_step(eeg, fmri, bad)
        with pytest.raises(ValueError):
            tr.pack_host_batch(eeg, fmri, out=torch.empty(10 ** 6, dtype=torch.uint8), groups=bad)


def test_packed_host_batch_appends_the_ids_and_keeps_the_ungrouped_layout():
    tr = BridgeTrainer(eeg_channels=8, device="cpu", mode="graph")
    eeg, fmri = torch.randn(4, 8, 64), torch.randn(4, 1, 16, 16, 16)
    n = 4 * 64 * ops.cpad(8) * 2 + fmri.numel() * 4
    plain = tr.pack_host_batch(eeg, fmri, out=torch.empty(n, dtype=torch.uint8))
    grouped = tr.pack_host_batch(eeg, fmri, out=torch.empty(n + 16, dtype=torch.uint8),
                                 groups=torch.tensor([7, 7, -1, 2 ** 31 - 1]))
    assert torch.equal(grouped[:n], plain)
    assert grouped[n:].view(torch.int32).tolist() == [7, 7, -1, 2 ** 31 - 1]


def test_synthetic_subject_pairs_share_one_volume_per_subject():
    eeg, fmri, groups = synthetic_subject_pairs(3, 4, eeg_channels=8, samples=32, vol=(4, 4, 4), device="cpu")
    assert eeg.shape == (12, 8, 32) and fmri.shape == (12, 1, 4, 4, 4)
    assert groups.dtype == torch.int32 and groups.tolist() == [0] * 4 + [1] * 4 + [2] * 4
    for s in range(3):
        rows = (groups == s).nonzero().flatten()
        assert all(torch.equal(fmri[rows[0]], fmri[r]) for r in rows)
        assert not torch.equal(eeg[rows[0]], eeg[rows[1]])
    assert not torch.equal(fmri[0], fmri[4])
