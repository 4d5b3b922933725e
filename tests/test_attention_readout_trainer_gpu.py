"""GPU: BridgeTrainer.temporal_attention between graph-mode training steps - chunking gives the same result within the
read-out kernels' tolerance (layers x 3e-3 relative, test_attention_readout_kernels_gpu.py), a repeated call the same bits,
and losses, parameters, Adam moments and BatchNorm buffers afterwards are bit-identical to a twin trainer that never
called it (the assertion of test_perturb_trainer_gpu.py for `perturb`)."""
import pytest
import torch

from multimodal_eeg_fmri_amd import ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs

pytestmark = pytest.mark.gpu


def _trainer(mode):
    ops.set_seed_epoch(None)
    ops.set_dropout_seed(4242)
    torch.manual_seed(0)
    return BridgeTrainer(eeg_channels=8, dropout=0.3, lr=1e-3, mode=mode).train()


def test_temporal_attention_between_graph_steps_leaves_the_training_state_bit_for_bit():
    batches = [synthetic_pairs(8, 8, 256, (16, 16, 16), seed=300 + i) for i in range(2)]

    def run(readout):
        tr = _trainer("graph")
        losses = [tr.train_step(*batches[i % 2])["loss"].clone() for i in range(3)]
        if readout:
            torch.cuda.synchronize()
            b = tr.bucket
            before = [t.clone() for t in (b.p, b.g, b.m, b.v, b.state)] + [t.clone() for t in tr.buffers()]
            seeds = dict(ops._seed_state)
            cap = tr._cap
            eeg = batches[1][0]
            a3 = tr.temporal_attention(eeg, batch_size=3)
            a8 = tr.temporal_attention(eeg.cuda(), batch_size=8)
            assert set(a3) == {"tokens", "time"} and a3["tokens"].shape == (8, 128) and a3["time"].shape == (8, 256)
            layers = len(tr.eeg_encoder.transformer_layers)
            for k in a3:
                assert a3[k].dtype == torch.float32 and a3[k].is_cuda and torch.isfinite(a3[k]).all()
                torch.testing.assert_close(a3[k], a8[k], rtol=layers * 3e-3, atol=1e-9)
                torch.testing.assert_close(a3[k].sum(-1), torch.ones(8, device="cuda"), rtol=layers * 3e-3, atol=0)
            again = tr.temporal_attention(eeg, batch_size=3)
            assert all(torch.equal(again[k], a3[k]) for k in a3)
            rec = tr.temporal_attention(eeg, method="received", layer=0, batch_size=8)
            assert rec["tokens"].shape == (8, 128) and not torch.equal(rec["tokens"], a8["tokens"])
            with pytest.raises(ValueError, match="batch_size"):
                tr.temporal_attention(eeg, batch_size=0)
            torch.cuda.synchronize()
            after = [b.p, b.g, b.m, b.v, b.state] + list(tr.buffers())
            assert all(torch.equal(x, y) for x, y in zip(before, after))
            assert {k: v for k, v in ops._seed_state.items() if k != "epoch"} == {k: v for k, v in seeds.items() if k != "epoch"}
            assert ops._seed_state["epoch"] is seeds["epoch"] and tr._cap is cap and tr.training
            assert all(p.grad is None for p in tr.parameters())
        losses += [tr.train_step(*batches[i % 2])["loss"].clone() for i in range(3)]
        torch.cuda.synchronize()
        b = tr.bucket
        state = [t.clone() for t in (b.p, b.m, b.v, b.state)] + [t.detach().clone() for t in tr.buffers()]
        ops.set_seed_epoch(None)
        return torch.stack(losses), state
    l1, s1 = run(True)
    l2, s2 = run(False)
    assert torch.isfinite(l1).all() and torch.equal(l1, l2), (l1, l2)
    assert len(s1) == len(s2) and all(torch.equal(a, b) for a, b in zip(s1, s2))
