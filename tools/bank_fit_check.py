#!/usr/bin/env python3
"""One observation, not a test: does a cross-batch negative bank help a small-batch fit?  The synthetic fit of bench.py's
untimed half (fresh shared-latent pairs every step, 5 % warm-up + cosine schedule, dropout 0.1) at B pairs per step, once
without a bank, once with ``bank_size`` rows and once with the bank filled by a momentum key encoder (``key_encoder=True``,
``ema_decay`` 0.999), equal steps and seeds; then gallery-scale retrieval (R@1, both directions) over held-out pairs no run
has seen.
Usage: python tools/bank_fit_check.py [steps=3000] [B=8] [bank_size=1024] [held_out=256]"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_eeg_fmri_amd import ops  # noqa: E402
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs  # noqa: E402

C, T, VOL, LR = 64, 1024, (32, 32, 32), 3e-4


def fit(steps, B, bank_size, held, key_encoder=False):
    torch.manual_seed(0)
    ops.set_seed_epoch(None)
    ops.set_dropout_seed(20260)
    tr = BridgeTrainer(eeg_channels=C, dropout=0.1, lr=LR, bank_size=bank_size,
                       **(dict(key_encoder=True, ema_decay=0.999) if key_encoder else {})).train()
    gm = torch.Generator().manual_seed(99)                       # the fixed mixing matrices of synthetic_pairs()
    A_e = torch.randn(C, 16, generator=gm).cuda()
    A_f = (torch.randn(VOL[0] * VOL[1] * VOL[2], 16, generator=gm) / 4.0).cuda()
    gg = torch.Generator(device="cuda").manual_seed(7)
    warm = max(1, steps // 20)
    for i in range(steps):
        if i % 50 == 0:
            f = (i + 50) / warm if i < warm else 0.01 + 0.99 * 0.5 * (1.0 + math.cos(math.pi * (i - warm) / max(1, steps - warm)))
            tr.set_lr(LR * min(1.0, f))
        z = torch.randn(B, 16, device="cuda", generator=gg)
        e = (z @ A_e.t()).unsqueeze(-1) * 0.5 + torch.randn(B, C, T, device="cuda", generator=gg)
        v = (z @ A_f.t()).view(B, 1, *VOL) + torch.randn(B, 1, *VOL, device="cuda", generator=gg)
        out = tr.train_step(e, v)
    m = tr.evaluate_retrieval(*held, batch_size=64)
    return out["loss"].item(), m["eeg_to_fmri"]["R@1"], m["fmri_to_eeg"]["R@1"], m["eeg_to_fmri"]["mrr"], tr.bank_filled


def main():
    a = [int(x) for x in sys.argv[1:]]
    steps, B, K, n = (a + [3000, 8, 1024, 256][len(a):])[:4]
    held = synthetic_pairs(n, C, T, VOL, seed=900)
    print(f"synthetic fit, {steps} steps of B={B} fresh pairs, lr {LR} (warm-up + cosine), dropout 0.1; {n} held-out pairs, chance R@1 {1 / n:.4f}")
    for size, key in ((0, False), (K, False), (K, True)):
        loss, r_ef, r_fe, mrr, filled = fit(steps, B, size, held, key)
        print(f"bank_size={size:5d}{' key_encoder' if key else '':12s} (filled {filled:5d}): last train loss {loss:.4f}  held-out R@1 e->f {r_ef:.4f}  f->e {r_fe:.4f}  "
              f"mean {(r_ef + r_fe) / 2:.4f}  MRR e->f {mrr:.4f}")


if __name__ == "__main__":
    main()
