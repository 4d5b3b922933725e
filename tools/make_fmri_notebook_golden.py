#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/f5_fmri_notebook.npz from the reference's fMRI notebook.

At generation time only, the notebook (``fMRI_CODE/CrossModal_fmri_scr.ipynb`` under the reference checkout given on the
command line) is opened, its three model cells are selected by their first line and executed in a namespace of
``{torch, nn, F}``; the classes they define are instantiated on the CPU and run in fp32.  Only arrays are stored - no
reference text - and this script carries none.

Shape: H = 32, L = 2, activation_dim = 30, connectivity_dim = 21, B = 8 (59 572 parameters).  ONE set of weights serves
every model: the classification fusion net's ``state_dict`` (every parameter and running statistic moved off its initial
value); the single-branch models take ``activation_encoder.*`` / ``connectivity_encoder.*`` as ``encoder.*`` and the same
``head.*``; the regression models replace ``head.3`` by ``reg_head3_{weight,bias}``.

Contents:
  sd_names, sd_shapes            the fusion net's state_dict keys (73) and shapes ("32,30"), in order
  single_names, single_shapes    the single-branch models' keys (32) and shapes
  w/<key>                        the weights; reg_head3_weight, reg_head3_bias
  activation, connectivity, class_labels, reg_labels          the inputs
  per task t in (classification, regression):
    t/fusion_output, t/fusion_fused, t/activation_only_output, t/connectivity_only_output        eval mode
    t/train_loss, t/grad/<parameter>          train mode, dropout 0 (cross entropy / MSE, mean), fusion net

Run:  python tools/make_fmri_notebook_golden.py <reference checkout>
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "f5_fmri_notebook.npz")
NOTEBOOK = os.path.join("fMRI_CODE", "CrossModal_fmri_scr.ipynb")
CELLS = ("# ENCODER BLOCKS", "class fMRIActivationOnly", "# FUSION MODEL")
H, L, A, C, B = 32, 2, 30, 21, 8


def notebook_classes(reference_root):
    cells = json.load(open(os.path.join(reference_root, NOTEBOOK)))["cells"]
    ns = {"torch": torch, "nn": nn, "F": F}
    for first in CELLS:
        src = ["".join(c["source"]) for c in cells if c["cell_type"] == "code" and "".join(c["source"]).startswith(first)]
        assert len(src) == 1, (first, len(src))
        exec(compile(src[0], first, "exec"), ns)
    return ns


def shapes(sd):
    return np.array([",".join(str(d) for d in v.shape) for v in sd.values()])


def main(reference_root):
    ns = notebook_classes(reference_root)
    g = torch.Generator().manual_seed(2605)
    torch.manual_seed(5)
    fusion = ns["fMRIFusionNet"](A, C, hidden_dim=H, num_classes=2, dropout=0.0, num_transformer_layers=L)
    with torch.no_grad():
        for q in fusion.parameters():                 # zero biases, unit gammas and equal fusion scalars hide terms
            q.add_(torch.randn(q.shape, generator=g) * 0.05)
        bn = fusion.fusion[1]
        bn.running_mean.copy_(torch.rand(H, generator=g) - 0.5)
        bn.running_var.copy_(torch.rand(H, generator=g) + 0.5)
        bn.num_batches_tracked.fill_(3)
    sd = {k: v.clone() for k, v in fusion.state_dict().items()}
    reg_w, reg_b = torch.randn(1, H // 2, generator=g) * 0.2, torch.randn(1, generator=g) * 0.2
    act, conn = torch.randn(B, A, generator=g), torch.randn(B, C, generator=g)
    cls_y, reg_y = torch.randint(0, 2, (B,), generator=g), torch.randn(B, generator=g)
    single = ns["fMRIActivationOnly"](A, hidden_dim=H, num_classes=2, dropout=0.0, num_layers=L)
    out = {"sd_names": np.array(list(sd)), "sd_shapes": shapes(sd),
           "single_names": np.array(list(single.state_dict())), "single_shapes": shapes(single.state_dict()),
           "reg_head3_weight": reg_w.numpy(), "reg_head3_bias": reg_b.numpy(),
           "activation": act.numpy(), "connectivity": conn.numpy(), "class_labels": cls_y.numpy(), "reg_labels": reg_y.numpy()}
    out.update({"w/" + k: v.numpy() for k, v in sd.items()})

    def weights(task, prefix=None):
        w = dict(sd)
        if task == "regression":
            w["head.3.weight"], w["head.3.bias"] = reg_w, reg_b
        if prefix is None:
            return w
        return {("encoder." + k[len(prefix):] if k.startswith(prefix) else k): v for k, v in w.items()
                if k.startswith(prefix) or k.startswith("head.")}

    for task in ("classification", "regression"):
        kw = dict(hidden_dim=H, num_classes=2, dropout=0.0, task=task)
        net = ns["fMRIFusionNet"](A, C, num_transformer_layers=L, **kw)
        net.load_state_dict(weights(task))
        a_only = ns["fMRIActivationOnly"](A, num_layers=L, **kw)
        a_only.load_state_dict(weights(task, "activation_encoder."))
        c_only = ns["fMRIConnectivityOnly"](C, num_layers=L, **kw)
        c_only.load_state_dict(weights(task, "connectivity_encoder."))
        with torch.no_grad():
            o, fused = net.eval()(act, conn, return_features=True)
            out[task + "/fusion_output"], out[task + "/fusion_fused"] = o.numpy(), fused.numpy()
            out[task + "/activation_only_output"] = a_only.eval()(act, conn).numpy()
            out[task + "/connectivity_only_output"] = c_only.eval()(act, conn).numpy()
        net.train()
        o = net(act, conn)
        loss = F.cross_entropy(o, cls_y) if task == "classification" else F.mse_loss(o, reg_y)
        loss.backward()
        out[task + "/train_loss"] = loss.detach().numpy()
        for k, q in net.named_parameters():
            out[task + "/grad/" + k] = q.grad.numpy()
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {sum(v.numel() for v in fusion.parameters())} parameters")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
