"""BridgeTrainer with subject-grouped positives (train_step / evaluate / pack_host_batch / HostFeeder / fit with group
ids) at a small shape, dropout 0: the graph replay and the eager tape train bit-identically, a grouped capture and an
ungrouped one alternate correctly, the eval loss is the fp64 grouped loss, all-distinct ids train as the ungrouped step,
and a short fit on several epochs per subject goes below the floor the ungrouped loss cannot pass."""
import math

import pytest
import torch

from multimodal_eeg_fmri_amd import ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_subject_pairs
from test_clip_groups_gpu import ref_grouped

pytestmark = pytest.mark.gpu

C, T, VOL = 8, 256, (16, 16, 16)


def _trainer(mode, lr=1e-3):
    ops.set_seed_epoch(None)
    torch.manual_seed(0)
    return BridgeTrainer(eeg_channels=C, dropout=0.0, lr=lr, mode=mode).train()


def _batches(n=3, subjects=4, per_subject=4):
    out = []
    for i in range(n):
        eeg, fmri, g = synthetic_subject_pairs(subjects, per_subject, C, T, VOL, seed=900 + i)
        perm = torch.randperm(eeg.shape[0], generator=torch.Generator().manual_seed(i))
        out.append((eeg[perm.cuda()].contiguous(), fmri[perm.cuda()].contiguous(), (g.cpu()[perm] * 10 + i).to(torch.int32)))
    return out


def _finish(tr, losses):
    torch.cuda.synchronize()
    p = tr.bucket.p.detach().clone()
    ops.set_seed_epoch(None)
    return torch.stack(losses), p


def test_graph_and_manual_grouped_steps_are_bit_identical_and_recapture_on_switch():
    batches = _batches()
    # grouped x3, then an ungrouped batch, then grouped again: two switches, each a new capture in graph mode
    plan = [(0, True), (1, True), (2, True), (0, False), (1, True)]

    def run(mode):
        tr = _trainer(mode)
        losses, kinds = [], []
        for i, grouped in plan:
            e, f, g = batches[i]
            losses.append(tr.train_step(e, f, g if grouped else None)["loss"].clone())
            if mode == "graph":
                kinds.append(tr._cap["grouped"])
        l, p = _finish(tr, losses)
        return l, p, kinds
    lm, pm, _ = run("manual")
    lg, pg, kinds = run("graph")
    assert kinds == [g for _, g in plan]
    assert torch.isfinite(lm).all()
    assert torch.equal(lm, lg), (lm - lg).abs().max().item()
    assert torch.equal(pm, pg)
    # device int32 ids are taken as they are
    tr = _trainer("graph")
    e, f, g = batches[0]
    a = tr.train_step(e, f, g)["loss"].item()
    tr2 = _trainer("graph")
    assert tr2.train_step(e, f, g.cuda())["loss"].item() == a


def test_evaluate_equals_the_fp64_grouped_loss():
    tr = _trainer("graph")
    batches = _batches()
    for e, f, g in batches:
        tr.train_step(e, f, g)
    e, f, g = batches[1]
    out = tr.evaluate(e, f, g)
    ze, zf = tr.embed(e, f)
    want, _ = ref_grouped(torch.cat([ze, zf], 1).cpu(), g.long(), tr.head.logit_scale.item(), e.shape[0], 0)
    assert abs(out["loss"].item() - want[0].item()) <= 1e-5 * max(1.0, abs(want[0].item()))
    assert out["top1_e2f"].item() == want[1].item() and out["top1_f2e"].item() == want[2].item()


def test_distinct_ids_train_as_the_ungrouped_step():
    batches = _batches()

    def run(grouped):
        tr = _trainer("graph")
        losses = []
        for i in range(3):
            e, f, _ = batches[i]
            ids = torch.arange(e.shape[0], dtype=torch.int32) * 3 - 5 if grouped else None
            losses.append(tr.train_step(e, f, ids)["loss"].clone())
        return _finish(tr, losses)
    lu, pu = run(False)
    lg, pg = run(True)
    # the two loss kernels agree to <= 1e-6 per step (test_clip_groups_gpu); three AdamW steps keep that small
    assert (lu - lg).abs().max().item() <= 1e-5
    assert (pu - pg).abs().max().item() <= 1e-5


def test_packed_host_batches_and_the_feeder_carry_the_ids():
    batches = _batches()

    def run(how):
        tr = _trainer("graph")
        losses = [tr.train_step(*batches[0])["loss"].clone()]                 # captures the grouped step
        if how == "feeder":
            feeder = tr.host_feeder()
            hosts = [tr.pack_host_batch(*batches[i % 3][:2], groups=batches[i % 3][2]) for i in range(1, 5)]
            feeder.upload(hosts[0])
            for i in range(4):
                if i + 1 < 4:
                    feeder.upload(hosts[i + 1])
                losses.append(feeder.step()["loss"].clone())
        else:
            for i in range(1, 5):
                e, f, g = batches[i % 3]
                if how == "packed":
                    host = tr.pack_host_batch(e, f, groups=g)
                    assert host.numel() == tr._cap["in"].numel()
                    assert torch.equal(host[-4 * e.shape[0]:].view(torch.int32), g)
                    losses.append(tr.train_step_packed(host.cuda())["loss"].clone())
                else:
                    losses.append(tr.train_step(e, f, g)["loss"].clone())
        return _finish(tr, losses)
    l0, p0 = run("steps")
    l1, p1 = run("packed")
    l2, p2 = run("feeder")
    assert torch.isfinite(l0).all()
    assert torch.equal(l0, l1) and torch.equal(p0, p1)
    assert torch.equal(l0, l2) and torch.equal(p0, p2)


def test_fit_on_subject_epochs_goes_below_the_ungrouped_floor():
    k = 4                                                   # epochs (and copies of the volume) per subject in a batch
    eeg, fmri, groups = synthetic_subject_pairs(16, k, C, T, VOL, seed=31, epoch_noise=0.3)
    train = [(eeg[i:i + 16], fmri[i:i + 16], groups[i:i + 16]) for i in range(0, 64, 16)]
    val = synthetic_subject_pairs(16, k, C, T, VOL, seed=32, epoch_noise=0.3)
    tr = _trainer("graph")
    E = 20
    hist = tr.fit(train, E, val=val, warmup_epochs=1, patience=100)
    assert len(hist) == E and all(h["val"] is not None for h in hist)
    floor = 0.5 * math.log(k)
    grouped = [tr.evaluate(*b)["loss"].item() for b in train]
    ungrouped = [tr.evaluate(*b[:2])["loss"].item() for b in train]
    # k identical volumes per batch: no ungrouped loss can pass 1/2 log k; the grouped one does
    assert min(ungrouped) >= floor - 1e-5, ungrouped
    assert sum(grouped) / len(grouped) < floor, (grouped, [h["train_loss"] for h in hist])
    # the history carries the grouped R@k; the restored best state reproduces its entry
    best = max(range(E), key=lambda i: (hist[i]["monitor"], -i))
    again = tr.evaluate_retrieval(val[0], val[1], groups=val[2])
    assert again == hist[best]["val"]
    assert set(again["eeg_to_fmri"]) >= {"R@1", "R@5", "R@10", "median_rank", "mrr"}
    # the ungrouped ranks count the subject's copies of the volume against the query: R@1 = 0 there
    assert tr.evaluate_retrieval(*val[:2])["eeg_to_fmri"]["R@1"] == 0.0 < again["eeg_to_fmri"]["R@1"]
