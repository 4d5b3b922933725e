#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/g1_eeg_baselines.npz from the reference's EEG notebook.

At generation time only, the notebook (``EEG_CODE/CrossModal_EEG_scr.ipynb`` under the reference checkout given on the
command line) is opened, the five code cells that define the single-modality baselines are selected by content (each
marker matches exactly one code cell) and executed in a namespace of ``{torch, nn, F, Optional}``; the classes are
instantiated on the CPU and run in fp32.  Only arrays are stored - no reference text - and this script carries none.

Shape: B = 8, C = 5, T = 44 (so 11 time steps reach the projection and the four AdaptiveAvgPool1d bins are [0,3) [2,6)
[5,9) [8,11)), erp_out = pw_out = 32, hidden = 16, two classes.  The weights are ``oracle.fixtures.build(cls, seed, ...)``
on both sides, so only the seed and ``checksum`` are stored.

Contents, per model m in (erponly, pwonly):
  m/seed, m/input_seed, m/label_seed      build seed; the input is seeded_randn(input_seed, B, C, T)
  m/sd_names, m/sd_shapes, m/checksum     state_dict keys, shapes ("32,5,7") and oracle.fixtures.checksum
  m/labels
  m/eval_logits                           eval mode
  m/train_logits, m/train_loss            train mode, every nn.Dropout.p of the instance set to 0; cross entropy (mean)
  m/gnames, m/gnorms, m/gsums, m/ghead::<parameter>      oracle.fixtures.grad_summary of that backward

Run:  python tools/make_eeg_baseline_golden.py <reference checkout>
"""
from __future__ import annotations

import json
import os
import sys
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.fixtures import build, checksum, grad_summary, seeded_randn  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g1_eeg_baselines.npz")
NOTEBOOK = os.path.join("EEG_CODE", "CrossModal_EEG_scr.ipynb")
CELLS = ("class BaseEEGModel(", "class PowerEncoder(", "class PWOnlyNet(", "class ERPEncoder(", "class ERPOnlyNet(")
B, C, T, OUT_DIM, HIDDEN = 8, 5, 44, 32, 16
MODELS = {"erponly": ("ERPOnlyNet", 72), "pwonly": ("PWOnlyNet", 71)}        # class, build seed (input seed = seed + 100)


def notebook_classes(reference_root):
    cells = json.load(open(os.path.join(reference_root, NOTEBOOK)))["cells"]
    ns = {"torch": torch, "nn": nn, "F": F, "Optional": Optional}
    for marker in CELLS:
        src = ["".join(c["source"]) for c in cells if c["cell_type"] == "code" and marker in "".join(c["source"])]
        assert len(src) == 1, (marker, len(src))
        exec(compile(src[0], marker, "exec"), ns)
    return ns


def shapes(sd):
    return np.array([",".join(str(d) for d in v.shape) for v in sd.values()])


def main(reference_root):
    ns = notebook_classes(reference_root)
    out = {}
    for tag, (cls, seed) in MODELS.items():
        def make():
            return build(ns[cls], seed, C, OUT_DIM, HIDDEN, 2)
        x = seeded_randn(seed + 100, B, C, T)
        y = torch.randint(0, 2, (B,), generator=torch.Generator().manual_seed(seed + 200))
        kw = {"erp": x} if tag == "erponly" else {"pw": x}
        net = make()
        sd = net.state_dict()
        out.update({f"{tag}/seed": np.int64(seed), f"{tag}/input_seed": np.int64(seed + 100),
                    f"{tag}/label_seed": np.int64(seed + 200), f"{tag}/sd_names": np.array(list(sd)),
                    f"{tag}/sd_shapes": shapes(sd), f"{tag}/checksum": checksum(net), f"{tag}/labels": y.numpy()})
        with torch.no_grad():
            out[f"{tag}/eval_logits"] = net.eval()(**kw).numpy()
        net = make().train()
        for mod in net.modules():
            if isinstance(mod, nn.Dropout):
                mod.p = 0.0
        logits = net(**kw)
        loss = F.cross_entropy(logits, y)
        loss.backward()
        out[f"{tag}/train_logits"] = logits.detach().numpy()
        out[f"{tag}/train_loss"] = loss.detach().numpy()
        out.update({f"{tag}/{k}": v for k, v in grad_summary(net).items()})
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
