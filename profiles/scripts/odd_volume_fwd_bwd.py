"""train fwd + bwd of the voxel encoder (dropout 0.3) at B = 8 on one volume shape, e.g. 91x109x91: the workload of
profiles/odd_volume_*_kernels.txt, run under `rocprofv3 --kernel-trace --stats -- python3 profiles/scripts/odd_volume_fwd_bwd.py 91x109x91 10`"""
import sys

import torch

sys.path.insert(0, ".")
from oracle.fixtures import build  # noqa: E402
import multimodal_eeg_fmri_amd.fmri_utils as Fm  # noqa: E402

shape = tuple(int(v) for v in sys.argv[1].split("x"))
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
torch.cuda.set_device(0)
m = build(Fm.fMRIVolumeEncoder3D, 1, dropout=0.3).train().cuda()
g = torch.Generator().manual_seed(3)
x = torch.randn(8, 1, *shape, generator=g).cuda()
gy = torch.randn(8, 64, generator=g).cuda()
for _ in range(iters):
    y = m(x)
    y.backward(gy)
    m.zero_grad(set_to_none=True)
torch.cuda.synchronize()
print("done", shape, float(y.float().sum()))
