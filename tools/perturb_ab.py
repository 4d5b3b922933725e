#!/usr/bin/env python3
"""One timing, recorded in DESIGN.md section 5p and asserted nowhere: `BridgeTrainer.perturb(method="occlusion")` against
the same drops computed one mask at a time through the trainer's public modules - clone, zero one channel / one 8^3 block,
both encoders, head.embed, (ze * zf).sum(1) - the reference notebook's protocol, the modules called the way `perturb` and
`explain` run them (eval mode, autograd on).  Both are warmed, both end in a synchronise, device events bracket each, and
they alternate in one process.  Also prints the largest difference between the two results, the same loop under no_grad
(the package's other eval forward: another result, bf16-rounding away) and the expansion kernel's own rate.
Usage: python tools/perturb_ab.py [B=32] [reps=5]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_eeg_fmri_amd import ops  # noqa: E402
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs  # noqa: E402

C, T, VOL, S = 64, 1024, (32, 32, 32), 8


def loop(tr, eeg, fmri, taped=True):
    """``taped``: the modules as `explain` (and `perturb`) run them - eval mode, autograd on, the inputs asking for a
    gradient; False: under no_grad, as the notebook's loop and `embed` (another forward: bf16-rounding away)"""
    tr.eval()
    with torch.set_grad_enabled(taped):
        def score(e, f):
            if taped:
                e, f = e.detach().requires_grad_(True), f.detach().requires_grad_(True)
            ze, zf = tr.head.embed(tr.eeg_encoder(e), tr.fmri_encoder(f))
            s = (ze * zf).sum(dim=1).detach()
            if taped:
                ops._release_tape(ze)            # (the tape's reference cycles would keep every forward's activations)
            return s
        full = score(eeg, fmri)
        de, df = [], []
        for c in range(C):
            e = eeg.clone()
            e[:, c] = 0
            de.append(full - score(e, fmri))
        g = VOL[0] // S
        for d in range(g):
            for h in range(g):
                for w in range(g):
                    f = fmri.clone()
                    f[:, :, d * S:(d + 1) * S, h * S:(h + 1) * S, w * S:(w + 1) * S] = 0
                    df.append(full - score(eeg, f))
    tr.train()
    return torch.stack(de, dim=1), torch.stack(df, dim=1)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    torch.manual_seed(0)
    ops.set_seed_epoch(None)
    tr = BridgeTrainer(eeg_channels=C, dropout=0.3, mode="manual").train()
    eeg, fmri = synthetic_pairs(B, C, T, VOL, seed=5)
    engine = lambda: tr.perturb(eeg, fmri, fmri_units=("blocks", S))      # noqa: E731
    for _ in range(2):                                                      # warm both
        out = engine()
        ref = loop(tr, eeg, fmri)
    torch.cuda.synchronize()
    print(f"largest |engine - loop|: channels {(out['eeg'] - ref[0]).abs().max().item():.3e} blocks "
          f"{(out['fmri'] - ref[1]).abs().max().item():.3e}; largest drops {ref[0].abs().max().item():.3e} {ref[1].abs().max().item():.3e}")
    plain = loop(tr, eeg, fmri, taped=False)
    torch.cuda.synchronize()
    print(f"largest |engine - no_grad loop|: channels {(out['eeg'] - plain[0]).abs().max().item():.3e} blocks "
          f"{(out['fmri'] - plain[1]).abs().max().item():.3e}")
    te, tl, tn = [], [], []
    for _ in range(reps):                                                   # alternate
        te.append(timed(engine)[0])
        tl.append(timed(lambda: loop(tr, eeg, fmri))[0])
        tn.append(timed(lambda: loop(tr, eeg, fmri, taped=False))[0])
    med = lambda v: sorted(v)[len(v) // 2]                                  # noqa: E731
    print(f"B={B} EEG {C}x{T}, volumes {VOL}, {C} channel masks + {(VOL[0] // S) ** 3} block masks")
    print("engine ms", [round(t, 2) for t in te], "loop ms", [round(t, 2) for t in tl], "no_grad loop ms", [round(t, 2) for t in tn])
    print(f"median: engine {med(te):.2f} ms, loop {med(tl):.2f} ms, ratio {med(tl) / med(te):.2f}x; "
          f"no_grad loop (another forward) {med(tn):.2f} ms")
    # the expansion alone: 64 masks of the EEG batch (B x 64 x 1024 x 64 x 4 bytes written, B x 64 x 1024 x 4 read per mask)
    masks = (1 - torch.eye(C, dtype=torch.int32)).cuda()
    ops.perturb_expand(eeg, None, masks, ("rows", 1))
    torch.cuda.synchronize()
    ts = [timed(lambda: ops.perturb_expand(eeg, None, masks, ("rows", 1)))[0] for _ in range(reps)]
    wrote = C * eeg.numel() * 4
    print(f"mm_perturb_expand {C} masks of ({B}, {C}, {T}): {med(ts):.3f} ms (includes the allocation), {wrote / 1e6:.0f} MB written, "
          f"{wrote / med(ts) / 1e6:.0f} GB/s of writes")


if __name__ == "__main__":
    main()
