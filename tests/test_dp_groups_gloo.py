"""CPU, world size 2, gloo: the grouped loss under data parallelism.  The group ids are all-gathered like the
embeddings (dp.gather_embeddings on a (B, 1) int32 view, what ClipLossFn and the trainer do); every rank evaluates all
rows of the gathered batch with the grouped InfoNCE and keeps the gradient rows of its own pairs.  With groups that span
the two ranks this reproduces the single-process global-batch loss and gradient.  A torch restatement of the kernel's
math stands in for the HIP kernel (which needs a GPU)."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import ref_functional as RF

W, B, N = 2, 6, 16
IDS = torch.tensor([0, 1, 1, 2, 0, 3, 3, 1, 4, 0, 2, 5], dtype=torch.int32)     # groups 0 - 3 span both ranks


def grouped_clip_loss(z_all, gid_all, scale, row0, B):
    """mean over rows [row0, row0 + B) of (l_row + l_col) / 2, P(r) = {j : gid_j = gid_r} (mm_clip_loss_own_rows_grouped)"""
    N = z_all.shape[1] // 2
    L = scale * z_all[:, :N] @ z_all[:, N:].T
    same = gid_all[:, None] == gid_all[None, :]
    ninf = torch.tensor(float("-inf"))
    l_row = torch.logsumexp(L, 1) - torch.logsumexp(torch.where(same, L, ninf), 1)
    l_col = torch.logsumexp(L, 0) - torch.logsumexp(torch.where(same, L, ninf), 0)
    return (0.5 * (l_row + l_col))[row0:row0 + B].mean()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, port, out_q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=W)
    from multimodal_eeg_fmri_amd import dp
    try:
        g = torch.Generator().manual_seed(7)
        h_all = torch.randn(W * B, 2 * N, generator=g)
        w = torch.randn(2 * N, generator=g)
        scale = torch.tensor(3.0)
        h = (h_all[rank * B:(rank + 1) * B] * w).requires_grad_(True)
        z = torch.cat([RF.l2_normalize(h[:, :N]), RF.l2_normalize(h[:, N:])], dim=1)
        gid = IDS[rank * B:(rank + 1) * B].clone()
        z_all = dp.gather_embeddings(z.detach(), dist.group.WORLD)
        gid_all = dp.gather_embeddings(gid.view(B, 1), dist.group.WORLD).view(-1)
        assert gid_all.dtype == torch.int32 and torch.equal(gid_all, IDS)
        za = z_all.clone().requires_grad_(True)
        total, loss_r = 0.0, None
        for r in range(W):
            lr_ = grouped_clip_loss(za, gid_all, scale, r * B, B)
            total = total + lr_
            if r == rank:
                loss_r = lr_
        total.backward()
        z.backward(za.grad[rank * B:(rank + 1) * B])
        flat = (h.grad * h_all[rank * B:(rank + 1) * B]).sum(0)
        dp.allreduce_sum_(flat, dist.group.WORLD)
        flat /= W
        losses = [torch.zeros(()) for _ in range(W)]
        dist.all_gather(losses, loss_r.detach())
        if rank == 0:
            out_q.put((flat, torch.stack(losses).mean()))
    finally:
        dist.destroy_process_group()


def test_grouped_dp_step_equals_global_batch():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, q)) for r in range(W)]
    for p in procs:
        p.start()
    got_grad, got_loss = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    g = torch.Generator().manual_seed(7)
    h_all = torch.randn(W * B, 2 * N, generator=g)
    w = torch.randn(2 * N, generator=g).requires_grad_(True)
    h = h_all * w
    z = torch.cat([RF.l2_normalize(h[:, :N]), RF.l2_normalize(h[:, N:])], dim=1)
    loss = grouped_clip_loss(z, IDS, torch.tensor(3.0), 0, W * B)
    loss.backward()
    assert abs(got_loss.item() - loss.item()) < 1e-6
    torch.testing.assert_close(got_grad, w.grad, rtol=1e-5, atol=1e-6)
    # the groups matter: the ungrouped loss of the same batch differs
    assert abs(loss.item() - RF.clip_loss(z[:, :N], z[:, N:], z[:, :N], z[:, N:], torch.tensor(3.0))[0].item()) > 1e-3
