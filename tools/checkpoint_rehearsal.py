"""Checkpoint / resume and `fit` of the data-parallel bridge trainer: two ranks on ONE GPU, collectives over gloo
(the staging shim of tools/dp_rehearsal.py; RCCL refuses two ranks on one device).  Checks:
  * rank 0 saves, both ranks load: the resumed parameters are bit-identical across ranks and equal the
    uninterrupted world-2 run (losses, parameters, Adam moments, optimizer words);
  * `fit` stops at the same epoch on both ranks (rank 0 validates and decides; rank 1's own monitor would never stop).
usage: python tools/checkpoint_rehearsal.py [world]        (spawns its own ranks)
"""
import os
import socket
import sys
import tempfile

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _worker(rank, world, port, tmp, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from multimodal_eeg_fmri_amd import ops
        from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
        from tools import gloo_staging
        gloo_staging.install()
        torch.cuda.set_device(0)
        ops.set_seed_epoch(None)
        ops.set_dropout_seed(555)
        batches = [synthetic_pairs(8, 16, 256, (16, 16, 16), seed=1000 + 10 * rank + i) for i in range(3)]

        def make(seed):
            torch.manual_seed(seed)
            return BridgeTrainer(eeg_channels=16, dropout=0.3, lr=1e-3, group=dist.group.WORLD).train()

        def steps(tr, i0, k):
            out = []
            for i in range(i0, i0 + k):
                out.append(tr.train_step(*batches[i % 3])["loss"].item())
            torch.cuda.synchronize()
            return out

        def snap(tr):
            b = tr.bucket
            return [t.detach().cpu().clone() for t in (b.p, b.m, b.v, b.state)]

        path = os.path.join(tmp, "ck.pt")
        a = make(0)
        steps(a, 0, 5)
        a.save_checkpoint(path, epoch=1)
        la = steps(a, 5, 5)
        ref = snap(a)
        b = make(3 + rank)
        for _ in range(4 + rank):                      # unrelated seeds drawn before the load
            ops._next_seed()
        b.load_checkpoint(path)
        lb = steps(b, 5, 5)
        got = snap(b)
        gathered = [torch.zeros_like(got[0]) for _ in range(world)]
        dist.all_gather(gathered, got[0])
        res = {"losses_equal": la == lb, "state_equal": all(torch.equal(x, y) for x, y in zip(ref, got)),
               "same_params_across_ranks": all(torch.equal(gathered[0], g) for g in gathered),
               "capture_mode": b.capture_mode}

        # fit: only rank 0's monitor decides (rank 1's scores keep rising and would never stop)
        scripted = iter([0.1, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5] if rank == 0 else [0.1 * i for i in range(1, 9)])
        val = synthetic_pairs(16, 16, 256, (16, 16, 16), seed=77)
        c = make(0)
        hist = c.fit(lambda e: batches, 8, val=val, warmup_epochs=1, patience=2, monitor=lambda m: next(scripted),
                     checkpoint_dir=os.path.join(tmp, "fit"))
        res["stop_epoch"] = hist[-1]["epoch"] if hist[-1]["stop"] else None
        res["history_monitor"] = [h["monitor"] for h in hist]
        p = c.bucket.p.detach().cpu().clone()
        gathered = [torch.zeros_like(p) for _ in range(world)]
        dist.all_gather(gathered, p)
        res["fit_same_params_across_ranks"] = all(torch.equal(gathered[0], g) for g in gathered)
        best = torch.load(os.path.join(tmp, "fit", "best.pt"), map_location="cpu", weights_only=True)
        res["best_epoch"] = best["epoch"]
        res["restored_is_best"] = all(torch.equal(best["model_state_dict"][n], t.detach().cpu())
                                      for n, t in c.named_parameters())
        res_all = [None] * world
        dist.all_gather_object(res_all, res)
        if rank == 0:
            q.put(res_all)
    finally:
        dist.destroy_process_group()


def run(world=2, timeout=600):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as tmp:
        procs = [ctx.Process(target=_worker, args=(r, world, port, tmp, q)) for r in range(world)]
        for p in procs:
            p.start()
        try:
            res = q.get(timeout=timeout)
        finally:
            for p in procs:
                p.join(timeout=120)
                if p.is_alive():
                    p.kill()
        for p in procs:
            assert p.exitcode == 0, p.exitcode
    return res


if __name__ == "__main__":
    print(run(int(sys.argv[1]) if len(sys.argv) > 1 else 2))
