#!/usr/bin/env python3
"""Micro-benchmark of individual C-ABI kernels at the C2 training-step shapes
(HIP events, interleaved rounds, median).  Usage: python tools/kbench.py [filter]"""
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_eeg_fmri_amd import _hip, ops  # noqa: E402

BF = torch.bfloat16


def timeit(fn, iters=20, rounds=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    meds = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        meds.append(a.elapsed_time(b) / iters * 1e3)
    return statistics.median(meds)


def linear_case(M, K, N, out_f32=False, residual=False, act="none"):
    x = torch.randn(M, K, device="cuda").to(BF)
    w = torch.randn(N, K, device="cuda") / math.sqrt(K)
    b = torch.randn(N, device="cuda")
    wf = torch.empty(N, 1, K, dtype=BF, device="cuda")
    _hip.call("mm_prep_conv_weight", w.view(N, K, 1).contiguous(), wf, None, N, K, 1, K, 0)
    res = torch.randn(M, N, device="cuda") if residual else None
    of = torch.empty(M, N, device="cuda") if out_f32 else None
    ob = None if out_f32 else torch.empty(M, N, dtype=BF, device="cuda")

    def fn():
        _hip.call("mm_conv1d_fwd", x, wf, 1, M, K, N, 1, 0, None, b, ops.ACT[act], res, None, 1, None, of, ob, None, 0.0, 0, None, None, 0)
    us = timeit(fn)
    fl = 2.0 * M * K * N
    print(f"linear M={M} K={K} N={N} f32={out_f32} res={residual} act={act}: {us:8.1f} us  {fl / us / 1e6:8.1f} TF/s")


def conv1d_case(B, T, Cin, Cout, k):
    x = torch.randn(B, T, Cin, device="cuda").to(BF)
    w = torch.randn(Cout, Cin, k, device="cuda") / math.sqrt(Cin * k)
    wf = torch.empty(Cout, k, Cin, dtype=BF, device="cuda")
    _hip.call("mm_prep_conv_weight", w.contiguous(), wf, None, Cout, Cin, k, Cin, 0)
    of = torch.empty(B, T, Cout, device="cuda")
    stats = torch.zeros(32, 2, Cout, device="cuda")
    b = torch.randn(Cout, device="cuda")

    def fn():
        _hip.call("mm_conv1d_fwd", x, wf, B, T, Cin, Cout, k, k // 2, None, b, 0, None, None, 1, stats, of, None, None, 0.0, 0, None, None, 0)
    us = timeit(fn)
    fl = 2.0 * B * T * Cin * Cout * k
    print(f"conv1d B={B} T={T} Cin={Cin} Cout={Cout} k={k}: {us:8.1f} us  {fl / us / 1e6:8.1f} TF/s")


def conv1d_wgrad_case(B, T, Cin, Cout, k):
    x = torch.randn(B, T, Cin, device="cuda").to(BF)
    dy = torch.randn(B, T, Cout, device="cuda").to(BF)
    ws = torch.zeros(8, Cout, k, Cin, device="cuda")
    db = torch.zeros(32, Cout, device="cuda")

    def fn():
        _hip.call("mm_conv1d_wgrad", dy, x, ws, db, B, T, Cin, Cout, k, k // 2, Cin, k * Cin, 1, Cin, 8, Cout * k * Cin, 0)
    us = timeit(fn)
    fl = 2.0 * B * T * Cin * Cout * k
    print(f"wgrad1d B={B} T={T} Cin={Cin} Cout={Cout} k={k}: {us:8.1f} us  {fl / us / 1e6:8.1f} TF/s")


def conv3d_dims_case(B, D, H, W, Cin, Cout, dgrad=False):
    """layer-2-shaped forward at arbitrary volume dims (BASELINE config #4: 64x64x48 input -> 32x32x24 here)"""
    x = torch.randn(B, D, H, W, Cin, device="cuda").to(BF)
    w = torch.randn(Cout, Cin, 27, device="cuda") / math.sqrt(Cin * 27)
    wf = torch.empty(Cout, 27, Cin, dtype=BF, device="cuda")
    _hip.call("mm_prep_conv_weight", w.contiguous(), wf, None, Cout, Cin, 27, Cin, 0)
    wres = (Cin == 32 and Cout == 64) or dgrad           # the weight-resident kernel writes bf16 only; so do data gradients
    of = torch.empty(B, D, H, W, Cout, device="cuda", dtype=BF if wres else torch.float32)
    stats = None if dgrad else torch.zeros(32, 2, Cout, device="cuda")
    b = None if dgrad else torch.randn(Cout, device="cuda")

    def fn():
        _hip.call("mm_conv3d_fwd", x, wf, B, D, H, W, Cin, Cout, b, stats, None if wres else of, of if wres else None)
    us = graph_time(fn, n=10)
    fl = 2.0 * B * D * H * W * Cin * Cout * 27
    print(f"conv3d B={B} {D}x{H}x{W} Cin={Cin} Cout={Cout}: {us:8.1f} us  {fl / us / 1e6:8.1f} TF/s "
          f"({fl / us / 1e6 / 2500:.3f} of 2.5 PF; graph-replayed)")


def wres_sustained_case(B, D, H, W, launches=400):
    """the roofline kernel (layer 2, 32 -> 64 channels) as `launches` back-to-back eager launches with no host
    synchronisation in between - sustained clocks, the condition bench.py's roofline_c2_standalone / roofline_c4 time it
    under; run under `rocprofv3 --kernel-trace --stats` for the per-launch mean the bench line must agree with"""
    Cin, Cout = 32, 64
    x = torch.randn(B, D, H, W, Cin, device="cuda").to(BF)
    w = torch.randn(Cout, Cin, 27, device="cuda") / math.sqrt(Cin * 27)
    wf = torch.empty(Cout, 27, Cin, dtype=BF, device="cuda")
    _hip.call("mm_prep_conv_weight", w.contiguous(), wf, None, Cout, Cin, 27, Cin, 0)
    of = torch.empty(B, D, H, W, Cout, device="cuda", dtype=BF)
    stats = torch.zeros(32, 2, Cout, device="cuda")
    b = torch.randn(Cout, device="cuda")
    for _ in range(10):
        _hip.call("mm_conv3d_fwd", x, wf, B, D, H, W, Cin, Cout, b, stats, None, of)
    torch.cuda.synchronize()
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(int(4.0e6))
    a.record()
    for _ in range(launches):
        _hip.call("mm_conv3d_fwd", x, wf, B, D, H, W, Cin, Cout, b, stats, None, of)
    e.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(e) / launches * 1e3
    fl = 2.0 * B * D * H * W * Cin * Cout * 27
    print(f"conv3d_wres sustained B={B} {D}x{H}x{W}: {launches} launches, {us:8.2f} us each  {fl / us / 1e6:8.1f} TF/s "
          f"({fl / us / 1e6 / 2500:.3f} of 2.5 PF; HIP events, gaps included)")


def conv3d_case(B, S, Cin, Cout, wgrad=True, fwd=True):
    x = torch.randn(B, S, S, S, Cin, device="cuda").to(BF)
    w = torch.randn(Cout, Cin, 27, device="cuda") / math.sqrt(Cin * 27)
    wf = torch.empty(Cout, 27, Cin, dtype=BF, device="cuda")
    _hip.call("mm_prep_conv_weight", w.contiguous(), wf, None, Cout, Cin, 27, Cin, 0)
    wres = Cin == 32 and Cout == 64                      # the weight-resident kernel writes bf16 only
    of = torch.empty(B, S, S, S, Cout, device="cuda", dtype=BF if wres else torch.float32)
    stats = torch.zeros(32, 2, Cout, device="cuda")
    b = torch.randn(Cout, device="cuda")

    def fn():
        _hip.call("mm_conv3d_fwd", x, wf, B, S, S, S, Cin, Cout, b, stats, None if wres else of, of if wres else None)
    fl = 2.0 * B * S ** 3 * Cin * Cout * 27
    if fwd:
        us = graph_time(fn)
        print(f"conv3d B={B} {S}^3 Cin={Cin} Cout={Cout}: {us:8.1f} us  {fl / us / 1e6:8.1f} TF/s (graph-replayed)")
    if not wgrad:
        return
    dy = torch.randn(B, S, S, S, Cout, device="cuda").to(BF)
    import ctypes
    n = ctypes.c_int(0)
    _hip.call("mm_conv3d_wgrad_slots", B, S, S, S, Cin, Cout, ctypes.addressof(n))
    ws = torch.zeros(n.value, Cout, 27, Cin, device="cuda")           # slot mode, as in the training step

    def fn2():
        _hip.call("mm_conv3d_wgrad", dy, x, ws, None, B, S, S, S, Cin, Cout, Cin, 27 * Cin, 1, Cin, n.value, Cout * 27 * Cin, 1)
    us = graph_time(fn2)
    print(f"wgrad3d B={B} {S}^3 Cin={Cin} Cout={Cout}: {us:8.1f} us  {fl / us / 1e6:8.1f} TF/s ({fl / us / 1e6 / 2500:.3f} of 2.5 PF; "
          f"{n.value} slots, graph-replayed)")


def attn_case(B=32, L=512, H=4, p=0.1, head_dim=32):
    """self-attention forward / backward at ``head_dim`` (16, 24, ..., 64): the entry point the model would call
    (mm_attn_* at 32, mm_attn_*_hd otherwise)"""
    from multimodal_eeg_fmri_amd import ops
    E = H * head_dim
    fwd, bwd = ops.attn_entry(E, H, "fwd"), ops.attn_entry(E, H, "bwd")
    qkv = (torch.randn(B, L, 3 * E, device="cuda") * 0.5).to(BF)
    out = torch.empty(B, L, E, dtype=BF, device="cuda")
    lse = torch.empty(B, H, L, device="cuda")
    dout = torch.randn(B, L, E, device="cuda").to(BF)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty(B, H, L, device="cuda")
    sc = 1 / math.sqrt(head_dim)
    f = timeit(lambda: _hip.call(fwd, qkv, out, lse, B, L, H, head_dim, sc, p, 77, None, None, 0))
    b = timeit(lambda: _hip.call(bwd, qkv, out, dout, lse, dqkv, delta, B, L, H, head_dim, sc, p, 77, None, None, 0))
    fl = 4.0 * B * H * L * L * head_dim
    print(f"attention B={B} L={L} H={H} dh={head_dim} p={p} ({fwd}): fwd {f:6.1f} us ({fl / f / 1e6:6.1f} TF/s)   "
          f"bwd (dq + dkv) {b:6.1f} us")


def attnmap_case(B=32, L=512, H=4, head_dim=32):
    """the attention read-out (csrc/attention_readout.hip) next to the forward it reads from: head-mean weights, received,
    and the route it replaces - per-head weights materialised, then reduced by torch"""
    E = H * head_dim
    fwd = ops.attn_entry(E, H, "fwd")
    qkv = (torch.randn(B, L, 3 * E, device="cuda") * 0.5).to(BF)
    out = torch.empty(B, L, E, dtype=BF, device="cuda")
    lse = torch.empty(B, H, L, device="cuda")
    sc = 1 / math.sqrt(head_dim)
    _hip.call(fwd, qkv, out, lse, B, L, H, head_dim, sc, 0.0, 0, None, None, 0)
    w = torch.empty(B, L, L, device="cuda")
    wh = torch.empty(B, H, L, L, device="cuda")
    rec = torch.empty(B, L, device="cuda")
    ws = torch.empty(_hip.host_int("mm_attn_received_ws_floats", B, L, H), device="cuda")
    f = timeit(lambda: _hip.call(fwd, qkv, out, lse, B, L, H, head_dim, sc, 0.0, 0, None, None, 0))
    tw = timeit(lambda: _hip.call("mm_attn_weights", qkv, lse, w, B, L, H, head_dim, sc, None, 0, 0))
    tr = timeit(lambda: _hip.call("mm_attn_received", qkv, lse, None, 0.0, rec, ws, B, L, H, head_dim, sc, None, 0))

    def materialise():
        _hip.call("mm_attn_weights", qkv, lse, wh, B, L, H, head_dim, sc, None, 0, 1)
        return wh.mean(dim=(1, 2))
    tm = timeit(materialise)
    print(f"attnmap B={B} L={L} H={H} dh={head_dim}: fwd (p=0) {f:7.1f} us | weights (head mean) {tw:7.1f} us, writes "
          f"{w.numel() * 4 / 1e6:.1f} MB | received {tr:7.1f} us, writes {(ws.numel() + rec.numel()) * 4 / 1e6:.2f} MB | "
          f"per-head weights + torch mean {tm:7.1f} us, writes {wh.numel() * 4 / 1e6:.1f} MB")


def floor_case():
    x = torch.zeros(64, device="cuda")
    y = torch.zeros(64, device="cuda")
    act = ops.ACT["none"]
    us = timeit(lambda: _hip.call("mm_act_f32", x, y, 64, act, 0.0, 0, None))
    print(f"harness floor (64-element copy through _hip.call): {us:8.1f} us")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _hip.call("mm_act_f32", x, y, 64, act, 0.0, 0, None)
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        for _ in range(20):
            _hip.call("mm_act_f32", x, y, 64, act, 0.0, 0, None)
    us = timeit(g.replay, iters=5) / 20
    print(f"same, 20 launches per hipGraph replay: {us:8.1f} us per kernel")


def graph_time(fn, n=20):
    """per-launch time of fn when n launches are replayed from one hipGraph"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    return timeit(g.replay, iters=5) / n


def bn_bwd_case(R, S, N, pool, f32_dout):
    """the two BatchNorm+act backward passes at an EEG conv layer's shape (graph-replayed launches)"""
    y = torch.randn(R, S, N, device="cuda")
    out4 = torch.stack([torch.rand(N, device="cuda") + 0.5, torch.randn(N, device="cuda") * 0.1,
                        torch.zeros(N, device="cuda"), torch.ones(N, device="cuda")]).contiguous()
    So = S // pool
    dout = torch.randn(R, So, N, device="cuda")
    db = None if f32_dout else dout.to(BF)
    df = dout if f32_dout else None
    sums = torch.zeros(32, 2, N, device="cuda")
    dy = torch.empty(R, S, N, dtype=BF, device="cuda")
    args = (R, S, N, ops.ACT["gelu"], pool, 0, 0.3, 1234, 0.0, 0, None)
    red = graph_time(lambda: _hip.call("mm_bn_act_bwd_reduce", y, out4, db, df, sums, *args))
    app = graph_time(lambda: _hip.call("mm_bn_act_bwd_apply", y, out4, db, df, sums, dy, None, *args, 1, 32))
    mb = (y.numel() * 4 + dout.numel() * (4 if f32_dout else 2)) / 1e6
    print(f"bn_bwd R={R} S={S} N={N} pool={pool} dout={'f32' if f32_dout else 'bf16'}: reduce {red:6.1f} us "
          f"({mb / red:5.2f} TB/s of {mb:.1f} MB)  apply {app:6.1f} us")


def split_case():
    """does running two half-batch chains on two streams beat one full-batch chain?  (linear + attention)"""
    import math as _m

    def mk(M):
        B = M // 512
        x = torch.randn(M, 128, device="cuda").to(BF)
        w = torch.randn(384, 128, device="cuda") / _m.sqrt(128)
        wf = torch.empty(384, 1, 128, dtype=BF, device="cuda")
        _hip.call("mm_prep_conv_weight", w.view(384, 128, 1).contiguous(), wf, None, 384, 128, 1, 128, 0)
        qkv = torch.empty(M, 384, dtype=BF, device="cuda")
        o = torch.empty(M, 128, dtype=BF, device="cuda")
        lse = torch.empty(B, 4, 512, device="cuda")
        w2 = torch.randn(128, 128, device="cuda") / _m.sqrt(128)
        wf2 = torch.empty(128, 1, 128, dtype=BF, device="cuda")
        _hip.call("mm_prep_conv_weight", w2.view(128, 128, 1).contiguous(), wf2, None, 128, 128, 1, 128, 0)
        res = torch.randn(M, 128, device="cuda")
        out = torch.empty(M, 128, device="cuda")

        def chain():
            for _ in range(4):
                _hip.call("mm_conv1d_fwd", x, wf, 1, M, 128, 384, 1, 0, None, None, 0, None, None, 1, None, None, qkv, None, 0.0, 0, None, None, 0)
                _hip.call("mm_attn_fwd", qkv, o, lse, B, 512, 4, 32, 1.0 / _m.sqrt(32), 0.1, 5, None, None, 0)
                _hip.call("mm_conv1d_fwd", o, wf2, 1, M, 128, 128, 1, 0, None, None, 0, res, None, 1, None, out, None, None, 0.1, 7, None, None, 0)
        return chain
    full = mk(16384)
    h1, h2 = mk(8192), mk(8192)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def two():
        cur = torch.cuda.current_stream()
        s1.wait_stream(cur); s2.wait_stream(cur)
        with torch.cuda.stream(s1):
            h1()
        with torch.cuda.stream(s2):
            h2()
        cur.wait_stream(s1); cur.wait_stream(s2)
    for name, fn in (("one stream, B=32", full), ("one stream, B=16 twice", lambda: (h1(), h2())), ("two streams, B=16 each", two)):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        print(f"{name:28s} {timeit(g.replay, iters=10):8.1f} us  (4 x [QKV linear, attention fwd, out-proj])")


def l1_case(B=32, D=32, H=32, W=32, p=0.3):
    """the three training passes of the fused first voxel layer (conv3d_l1.hip) at the C2 shape: statistics (mode 0),
    forward (mode 1), one-pass backward (mode 4 + combine).  FLOPs per pass = 2 * 27 * 32 * voxels = 1.81 GF at C2;
    compulsory bytes: 4.2 MB fp32 volume in (+ 8.4 MB bf16 pooled output for the forward / pooled gradient in for the backward)."""
    import multimodal_eeg_fmri_amd.fmri_utils as Fm
    torch.manual_seed(0)
    enc = Fm.fMRIVolumeEncoder3D(1, 64, dropout=p).cuda().train()
    conv, bn = enc.conv_layers[0], enc.conv_layers[1]
    x = torch.randn(B, 1, D, H, W, device="cuda")
    out, s = ops.conv3d_l1_bn_act(x, conv, bn, training=True, drop_p=p)
    wimg, out4 = s["wimg"], s["out4"]
    stats = torch.zeros(32, 2, 32, device="cuda")
    dout = torch.randn(out.shape, device="cuda").to(BF)
    sums, a1 = torch.zeros(32, 2, 32, device="cuda"), torch.zeros(32, 27, 32, device="cuda")
    gram = torch.zeros(32, 32, 32, device="cuda")
    gramc = s["gramc"].clone()
    dw, db = torch.zeros(32, 1, 3, 3, 3, device="cuda"), torch.zeros(32, device="cuda")
    fl = 2.0 * 27 * 32 * B * D * H * W
    tg = timeit(lambda: _hip.call("mm_conv3d_l1_gram", x, wimg, conv.bias, gram, stats, B, D, H, W))
    t0 = timeit(lambda: _hip.call("mm_conv3d_l1", 0, x, wimg, conv.bias, None, None, None, stats, None, None, None,
                                  B, D, H, W, 1, 0.0, 0, None))
    t1 = timeit(lambda: _hip.call("mm_conv3d_l1", 1, x, wimg, conv.bias, out4, None, None, None, out, None, None,
                                  B, D, H, W, 1, float(p), 123, None))
    t4 = timeit(lambda: _hip.call("mm_conv3d_l1_bwd", x, wimg, conv.bias, out4, dout, sums, a1, gramc, dw, db,
                                  B, D, H, W, 1, float(p), 123, None))
    inb, outb = x.numel() * 4, out.numel() * 2
    for name, t, byts in (("Gram matrix + BatchNorm sums", tg, inb),
                          ("stats by recompute (mode 0, ABI)", t0, inb), ("forward (mode 1)", t1, inb + outb),
                          ("backward (mode 4 + combine)", t4, inb + outb)):
        print(f"conv3d_l1 {name:34s} B={B} {D}x{H}x{W}: {t:7.1f} us  {fl / t / 1e6:6.1f} TF/s (of 157 fp32 / 2500 bf16)  "
              f"{byts / 1e6:5.1f} MB compulsory -> {byts / t / 1e6:6.2f} TB/s of 8")


def step_case(config="c2", steps=4):
    """the captured training step itself, a few replays: the PMC collector (profiles/run_pmc_kernels.sh <tag> step "")
    reads counters for EVERY kernel of the step (the profiler serialises them: stand-alone figures in the step's order)"""
    from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
    torch.manual_seed(0)
    enc = None
    if config == "c5":
        from multimodal_eeg_fmri_amd.crossmodal_v4_enhancements import MultiScaleSTFTPowerEncoder
        enc = MultiScaleSTFTPowerEncoder(64, (64, 128), 32, 128, 2, 4, 0.3)
    tr = BridgeTrainer(eeg_channels=64, dropout=0.3, eeg_encoder=enc).train()
    eeg, fmri = synthetic_pairs(32, 64, 1024, (32, 32, 32), seed=1234)
    for _ in range(steps):
        out = tr.train_step(eeg, fmri)
    torch.cuda.synchronize()
    print(f"step case {config}: {steps} steps, loss {out['loss'].item():.4f}")


FP32_MFMA_PEAK_TF = 157.3      # MI355X fp32-input MFMA peak (MI355X_MICROARCH.md)


def retr_case(nq, ng, d, k, vs_torch=False):
    """mm_retrieval (ranks + top-k): time, TF/s = 2 Nq Ng D / time, share of the fp32 MFMA peak.  vs_torch: also the
    torch composition (fp32 q @ g.T, comparison, topk) and a check that its ranks agree within the fp64 tie band"""
    gen = torch.Generator(device="cuda").manual_seed(7)
    q = torch.nn.functional.normalize(torch.randn(nq, d, device="cuda", generator=gen), dim=1).contiguous()
    g = torch.nn.functional.normalize(torch.randn(ng, d, device="cuda", generator=gen), dim=1).contiguous()
    us = timeit(lambda: ops.retrieval(q, g, k=k), iters=5, rounds=3)
    tf = 2.0 * nq * ng * d / (us * 1e-6) / 1e12
    print(f"retr Nq={nq} Ng={ng} D={d} k={k}: {us:9.1f} us  {tf:6.1f} TF/s  {tf / FP32_MFMA_PEAK_TF:5.3f} of fp32 MFMA peak")
    # where the time goes: the same launch with one epilogue only
    ur = timeit(lambda: ops.retrieval(q, g), iters=5, rounds=3)
    uk = timeit(lambda: ops.retrieval(q, g, k=k, ranks=False), iters=5, rounds=3)
    print(f"  ranks only: {ur:9.1f} us ({2.0 * nq * ng * d / (ur * 1e-6) / 1e12:6.1f} TF/s)   top-k only: {uk:9.1f} us")
    if not vs_torch:
        return

    def torch_way():
        s = q @ g.T
        sp = s.diagonal()
        r = 1 + (s >= sp[:, None]).sum(1) - 1
        return r, s.topk(k, dim=1)
    ut = timeit(torch_way, iters=5, rounds=3)
    print(f"  torch composition (fp32 GEMM + compare + topk): {ut:9.1f} us  -> kernel {ut / us:4.2f}x faster")
    r, _, _ = ops.retrieval(q, g)
    rt, _ = torch_way()
    rows = torch.arange(0, nq, max(1, nq // 512), device="cuda")
    S = q[rows].double() @ g.double().T
    sp = S[torch.arange(len(rows), device="cuda"), rows]
    lo = 1 + (S > sp[:, None] + 1e-6).sum(1)
    hi = (S >= sp[:, None] - 1e-6).sum(1)
    ok = all(((x[rows] >= lo) & (x[rows] <= hi)).all().item() for x in (r, rt))
    print(f"  ranks of kernel and torch within the fp64 tie band on {len(rows)} queries: {ok}; "
          f"equal on {(r == rt).float().mean().item():.6f} of all queries")
    assert ok


def loss_lines():
    """the loss launches (graph-replayed) at (B, Bg, N) = (32, 32, 128) and (32, 256, 128): the InfoNCE kernel pair and the
    pairwise sigmoid loss, each plain and grouped, in the same run"""
    for B, Bg, N in ((32, 32, 128), (32, 256, 128)):
        z = torch.nn.functional.normalize(torch.randn(Bg, 2 * N, device="cuda"), dim=1).contiguous()
        gid = (torch.arange(Bg, device="cuda", dtype=torch.int32) // 4).contiguous()
        ls = torch.full((1,), math.log(1 / 0.07), device="cuda")
        scal, dz = torch.empty(5, device="cuda"), torch.empty(B, 2 * N, device="cuda")
        ws_u = torch.empty(ops.clip_loss_ws_floats(B, Bg), device="cuda")
        ws_g = torch.empty(ops.clip_loss_ws_floats(B, Bg, grouped=True), device="cuda")
        tu = graph_time(lambda: _hip.call("mm_clip_loss_own_rows", z, ls, scal, dz, ws_u, B, Bg, N, 0))
        tg = graph_time(lambda: _hip.call("mm_clip_loss_own_rows_grouped", z, gid, ls, scal, dz, ws_g, B, Bg, N, 0))
        print(f"clip loss B={B} Bg={Bg} N={N}: ungrouped {tu:7.2f} us  grouped {tg:7.2f} us  (+{tg - tu:5.2f} us)")
        lsig, lb = torch.full((1,), math.log(10.0), device="cuda"), torch.full((1,), -10.0, device="cuda")
        ws_s = torch.empty(ops.sigmoid_loss_ws_floats(B, Bg), device="cuda")
        su = graph_time(lambda: _hip.call("mm_sigmoid_loss_own_rows", z, None, lsig, lb, scal, dz, ws_s, B, Bg, N, 0))
        sg = graph_time(lambda: _hip.call("mm_sigmoid_loss_own_rows", z, gid, lsig, lb, scal, dz, ws_s, B, Bg, N, 0))
        print(f"sigmoid loss B={B} Bg={Bg} N={N}: ungrouped {su:7.2f} us  grouped {sg:7.2f} us  "
              f"({su - tu:+5.2f} / {sg - tg:+5.2f} us vs clip loss)")


def sigmoid_case(step_iters=30):
    """the pairwise sigmoid loss vs InfoNCE: the loss launches (`loss_lines`) and the C2 graph step (B = 32) with each
    loss, interleaved rounds"""
    loss_lines()
    from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
    eeg, fmri = synthetic_pairs(32, 64, 1024, (32, 32, 32))
    trs = []
    for loss in ("infonce", "sigmoid"):
        ops.set_seed_epoch(None)
        torch.manual_seed(0)
        tr = BridgeTrainer(eeg_channels=64, dropout=0.3, loss=loss).train()
        tr.train_step(eeg, fmri)
        trs.append(tr)
    times = ([], [])
    for _ in range(5):
        for i, tr in enumerate(trs):
            times[i].append(timeit(lambda: tr.train_step(eeg, fmri), iters=step_iters, rounds=1))
    ti, ts = statistics.median(times[0]), statistics.median(times[1])
    print(f"C2 graph step B=32: infonce {ti:7.1f} us  sigmoid {ts:7.1f} us  ({100 * (ts / ti - 1):+.2f} %)")


def groups_case(step_iters=30):
    """subject-grouped positives vs the ungrouped path: the loss launches (`loss_lines`), the rank pass at Nq = Ng = 8192 and
    65536 (D = 128), and the C2 graph step (B = 32: 8 subjects x 4 epochs) with and without ids, interleaved rounds"""
    loss_lines()
    for n in (8192, 65536):
        q = torch.nn.functional.normalize(torch.randn(n, 128, device="cuda"), dim=1).contiguous()
        g = torch.nn.functional.normalize(torch.randn(n, 128, device="cuda"), dim=1).contiguous()
        ids = torch.randint(0, n // 8, (n,), device="cuda", dtype=torch.int32)
        tu = timeit(lambda: ops.retrieval(q, g), iters=5, rounds=5)
        tg = timeit(lambda: ops.retrieval(q, g, q_groups=ids, g_groups=ids), iters=5, rounds=5)
        print(f"ranks Nq=Ng={n} D=128: ungrouped {tu:9.1f} us  grouped {tg:9.1f} us  ({tg / tu:4.2f}x)")
    from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_subject_pairs
    eeg, fmri, groups = synthetic_subject_pairs(8, 4, 64, 1024, (32, 32, 32))
    trs = []
    for grouped in (False, True):
        ops.set_seed_epoch(None)
        torch.manual_seed(0)
        tr = BridgeTrainer(eeg_channels=64, dropout=0.3).train()
        tr.train_step(eeg, fmri, groups if grouped else None)
        trs.append((tr, groups if grouped else None))
    times = ([], [])
    for _ in range(5):
        for i, (tr, gr) in enumerate(trs):
            times[i].append(timeit(lambda: tr.train_step(eeg, fmri, gr), iters=step_iters, rounds=1))
    tu, tg = statistics.median(times[0]), statistics.median(times[1])
    print(f"C2 graph step B=32: ungrouped {tu:7.1f} us  grouped {tg:7.1f} us  ({100 * (tg / tu - 1):+.2f} %)")


def neighbours_case(rounds=5):
    """ignored temporal neighbours: the masked launches against the same build's grouped launches of both losses at the C2
    loss shape (B = Bg = 32, N = 128) and at Bg = 256, graph-replayed in the same run, medians of interleaved rounds.
    Timeline ids (a shuffled 0 .. Bg - 1), radius 2: 2 to 4 ignored keys per row; the grouped launches get the same ids"""
    for B, Bg, N in ((32, 32, 128), (32, 256, 128)):
        z = torch.nn.functional.normalize(torch.randn(Bg, 2 * N, device="cuda"), dim=1).contiguous()
        gid = torch.randperm(Bg, device="cuda").to(torch.int32).contiguous()
        ls = torch.full((1,), math.log(1 / 0.07), device="cuda")
        lsig, lb = torch.full((1,), math.log(10.0), device="cuda"), torch.full((1,), -10.0, device="cuda")
        scal, dz = torch.empty(5, device="cuda"), torch.empty(B, 2 * N, device="cuda")
        ws_g = torch.empty(ops.clip_loss_ws_floats(B, Bg, grouped=True), device="cuda")
        ws_m = torch.empty(ops.clip_loss_masked_ws_floats(B, Bg), device="cuda")
        ws_s = torch.empty(ops.sigmoid_loss_ws_floats(B, Bg), device="cuda")
        ws_t = torch.empty(ops.sigmoid_loss_masked_ws_floats(B, Bg), device="cuda")
        cases = [
            ("clip grouped", lambda: _hip.call("mm_clip_loss_own_rows_grouped", z, gid, ls, scal, dz, ws_g, B, Bg, N, 0)),
            ("clip masked", lambda: _hip.call("mm_clip_loss_own_rows_masked", z, gid, ls, scal, dz, ws_m, B, Bg, N, 0, 2)),
            ("sigmoid grouped", lambda: _hip.call("mm_sigmoid_loss_own_rows", z, gid, lsig, lb, scal, dz, ws_s, B, Bg, N, 0)),
            ("sigmoid masked", lambda: _hip.call("mm_sigmoid_loss_own_rows_masked", z, gid, lsig, lb, scal, dz, ws_t, B, Bg, N, 0, 2))]
        times = {name: [] for name, _ in cases}
        for _ in range(rounds):
            for name, fn in cases:
                times[name].append(graph_time(fn))
        for name, _ in cases:
            print(f"neighbours B={B} Bg={Bg} N={N}: {name:16s} {_spread(times[name])}")
        for kind in ("clip", "sigmoid"):
            g, m = statistics.median(times[f"{kind} grouped"]), statistics.median(times[f"{kind} masked"])
            print(f"neighbours B={B} Bg={Bg} N={N}: {kind} masked - grouped {m - g:+6.2f} us")


def retrieval_masked_case(rounds=5, iters=10):
    """retrieval with ignored temporal neighbours: mm_retrieval_masked against the same build's mm_retrieval_grouped (ranks
    only, k = 0) and mm_retrieval (top-k only, k = 10) at (Nq, Ng, D) = (4096, 4096, 128) and (512, 65536, 128), on
    preallocated buffers (the entry points alone), HIP events, medians of interleaved rounds [min .. max].  Timeline ids (a
    shuffled 0 .. Ng - 1; the queries take the first Nq), radius 2: 2 to 4 ignored rows per query; the grouped launch
    gets the same ids, the ungrouped one needs none"""
    for nq, ng, d in ((4096, 4096, 128), (512, 65536, 128)):
        gen = torch.Generator(device="cuda").manual_seed(7)
        q = torch.nn.functional.normalize(torch.randn(nq, d, device="cuda", generator=gen), dim=1).contiguous()
        g = torch.nn.functional.normalize(torch.randn(ng, d, device="cuda", generator=gen), dim=1).contiguous()
        gg = torch.randperm(ng, device="cuda").to(torch.int32).contiguous()
        qg = gg[:nq].contiguous()
        k = 10
        r, n = (torch.empty(nq, dtype=torch.int32, device="cuda") for _ in range(2))
        ti, ts = torch.empty(nq, k, dtype=torch.int32, device="cuda"), torch.empty(nq, k, device="cuda")
        ws_g = torch.empty(ops.retrieval_grouped_ws_floats(nq, ng, d), device="cuda")
        ws_u = torch.empty(ops.retrieval_ws_floats(nq, ng, d, k), device="cuda")
        ws_m = torch.empty(ops.retrieval_masked_ws_floats(nq, ng, d, k), device="cuda")
        cases = [
            ("ranks grouped", lambda: _hip.call("mm_retrieval_grouped", q, g, qg, gg, r, ws_g, nq, ng, d)),
            ("ranks masked", lambda: _hip.call("mm_retrieval_masked", q, g, qg, gg, 2, r, None, None, None, ws_m, nq, ng, d, 0)),
            ("ranks+neg masked", lambda: _hip.call("mm_retrieval_masked", q, g, qg, gg, 2, r, n, None, None, ws_m, nq, ng, d, 0)),
            ("top-k ungrouped", lambda: _hip.call("mm_retrieval", q, g, None, None, ti, ts, ws_u, nq, ng, d, k)),
            ("top-k masked", lambda: _hip.call("mm_retrieval_masked", q, g, qg, gg, 2, None, None, ti, ts, ws_m, nq, ng, d, k)),
            ("all masked", lambda: _hip.call("mm_retrieval_masked", q, g, qg, gg, 2, r, n, ti, ts, ws_m, nq, ng, d, k))]
        times = {name: [] for name, _ in cases}
        for _ in range(rounds):
            for name, fn in cases:
                times[name].append(timeit(fn, iters=iters, rounds=1))
        tag = f"retrieval_masked Nq={nq} Ng={ng} D={d}"
        for name, _ in cases:
            print(f"{tag}: {name:16s} {_spread(times[name])}")
        med = {name: statistics.median(t) for name, t in times.items()}
        print(f"{tag}: ranks masked - grouped {med['ranks masked'] - med['ranks grouped']:+7.1f} us "
              f"({100 * (med['ranks masked'] / med['ranks grouped'] - 1):+.2f} %), with negatives "
              f"{med['ranks+neg masked'] - med['ranks grouped']:+7.1f} us; top-k (k = {k}) masked - ungrouped "
              f"{med['top-k masked'] - med['top-k ungrouped']:+7.1f} us ({100 * (med['top-k masked'] / med['top-k ungrouped'] - 1):+.2f} %); "
              f"ranks, negatives and top-k in one call {med['all masked']:7.1f} us against "
              f"{med['ranks grouped'] + med['top-k ungrouped']:7.1f} us for the grouped and the ungrouped call")


def bank_case(B=32, N=128, step_iters=30, rounds=5):
    """the cross-batch negative bank: the loss section's launches, graph-replayed in the same run - the in-batch InfoNCE
    pair against mm_clip_bank_loss + mm_clip_bank_push on a full bank of K = 1024 and 4096 rows (and the loss's two
    launches alone) - and the C2 graph step (B = 32) without a bank and with bank_size = 4096 (full), interleaved rounds"""
    z = torch.nn.functional.normalize(torch.randn(B, 2 * N, device="cuda"), dim=1).contiguous()
    ls = torch.full((1,), math.log(1 / 0.07), device="cuda")
    scal, dz = torch.empty(4, device="cuda"), torch.empty(B, 2 * N, device="cuda")
    ws_u = torch.empty(ops.clip_loss_ws_floats(B, B), device="cuda")
    cases = [("in-batch clip loss", lambda: _hip.call("mm_clip_loss_own_rows", z, ls, scal, dz, ws_u, B, B, N, 0))]
    for K in (1024, 4096):
        bank = ops.ClipBank(K, N, False, "cuda")
        bank.bank.copy_(torch.nn.functional.normalize(torch.randn(K, 2 * N, device="cuda"), dim=1))
        bank.state.copy_(torch.tensor([0, K, K // B, 0], dtype=torch.int32))
        ws = torch.empty(ops.clip_bank_ws_floats(B, K, N), device="cuda")

        def loss(bank=bank, ws=ws, K=K):
            _hip.call("mm_clip_bank_loss", z, None, bank.bank, None, bank.state, ls, scal, dz, ws, B, K, N, 0)

        def both(bank=bank, loss=loss, K=K):
            loss()
            _hip.call("mm_clip_bank_push", z, None, bank.bank, None, bank.state, B, K, N)
        cases += [(f"bank loss K={K}", loss), (f"bank loss + push K={K}", both)]
    times = {name: [] for name, _ in cases}
    for _ in range(rounds):
        for name, fn in cases:
            times[name].append(graph_time(fn))
    for name, _ in cases:
        print(f"loss section B={B} N={N}: {name:26s} {_spread(times[name])}")
    from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
    eeg, fmri = synthetic_pairs(32, 64, 1024, (32, 32, 32))
    trs = []
    for K in (0, 4096):
        ops.set_seed_epoch(None)
        torch.manual_seed(0)
        tr = BridgeTrainer(eeg_channels=64, dropout=0.3, bank_size=K).train()
        for _ in range(K // 32 + 1):                          # fill the bank: the timed steps see all K rows
            tr.train_step(eeg, fmri)
        trs.append(tr)
    steps = ([], [])
    for _ in range(rounds):
        for i, tr in enumerate(trs):
            steps[i].append(timeit(lambda: tr.train_step(eeg, fmri), iters=step_iters, rounds=1))
    t0, t1 = statistics.median(steps[0]), statistics.median(steps[1])
    print(f"C2 graph step B=32: no bank {_spread(steps[0])}   bank_size=4096 (filled {trs[1].bank_filled}) {_spread(steps[1])}   "
          f"({t1 - t0:+.1f} us, {100 * (t1 / t0 - 1):+.2f} %)")


def key_case(B=32, N=128, step_iters=30, rounds=5, stamps=True):
    """the momentum key encoder: mm_clip_key_loss (+ push) against mm_clip_bank_loss (+ push) on a full bank of K = 1024 and
    4096 rows - eager launches between HIP events and graph-replayed launches, interleaved rounds in the same run - then the
    C2 graph step (B = 32, bank_size = 4096 full, ema_decay = 0.999) without and with key_encoder=True, the eval forward of
    both encoders alone (what the key pass adds to each stream), and both steps' phase stamps"""
    q = torch.nn.functional.normalize(torch.randn(B, 2, N, device="cuda"), dim=2).reshape(B, 2 * N).contiguous()
    k = torch.nn.functional.normalize(q.view(B, 2, N) + 0.3 * torch.randn(B, 2, N, device="cuda"), dim=2).reshape(B, 2 * N).contiguous()
    ls = torch.full((1,), math.log(1 / 0.07), device="cuda")
    scal, dz = torch.empty(4, device="cuda"), torch.empty(B, 2 * N, device="cuda")
    cases = []
    for K in (1024, 4096):
        bank = ops.ClipBank(K, N, False, "cuda")
        bank.bank.copy_(torch.nn.functional.normalize(torch.randn(K, 2, N, device="cuda"), dim=2).reshape(K, 2 * N))
        bank.state.copy_(torch.tensor([0, K, K // B, 0], dtype=torch.int32))
        ws_b = torch.empty(ops.clip_bank_ws_floats(B, K, N), device="cuda")
        ws_k = torch.empty(ops.clip_key_ws_floats(B, K, N), device="cuda")

        def bank_loss(bank=bank, ws=ws_b, K=K):
            _hip.call("mm_clip_bank_loss", q, None, bank.bank, None, bank.state, ls, scal, dz, ws, B, K, N, 0)

        def key_loss(bank=bank, ws=ws_k, K=K):
            _hip.call("mm_clip_key_loss", q, k, None, bank.bank, None, bank.state, ls, scal, dz, ws, B, K, N, 0)

        def push(bank=bank, K=K):
            _hip.call("mm_clip_bank_push", k, None, bank.bank, None, bank.state, B, K, N)
        cases += [(f"bank loss K={K}", bank_loss), (f"key loss K={K}", key_loss),
                  (f"bank loss + push K={K}", lambda a=bank_loss, b=push: (a(), b())),
                  (f"key loss + push K={K}", lambda a=key_loss, b=push: (a(), b()))]
    eager, replayed = {name: [] for name, _ in cases}, {name: [] for name, _ in cases}
    for _ in range(rounds):
        for name, fn in cases:
            eager[name].append(timeit(fn, iters=20, rounds=1))
            replayed[name].append(graph_time(fn))
    for name, _ in cases:
        print(f"loss section B={B} N={N}: {name:26s} eager {_spread(eager[name])}   graph {_spread(replayed[name])}")
    from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
    eeg, fmri = synthetic_pairs(32, 64, 1024, (32, 32, 32))
    trs = []
    for key in (False, True):
        ops.set_seed_epoch(None)
        torch.manual_seed(0)
        tr = BridgeTrainer(eeg_channels=64, dropout=0.3, bank_size=4096, ema_decay=0.999, key_encoder=key).train()
        for _ in range(4096 // 32 + 1):                       # fill the bank: the timed steps see all K rows
            tr.train_step(eeg, fmri)
        trs.append(tr)
    steps = ([], [])
    for _ in range(rounds):
        for i, tr in enumerate(trs):
            steps[i].append(timeit(lambda: tr.train_step(eeg, fmri), iters=step_iters, rounds=1))
    t0, t1 = statistics.median(steps[0]), statistics.median(steps[1])
    print(f"C2 graph step B=32 bank_size=4096 ema_decay=0.999: no key encoder {_spread(steps[0])}   key_encoder=True {_spread(steps[1])}   "
          f"({t1 - t0:+.1f} us, {100 * (t1 / t0 - 1):+.2f} %)")
    tr = trs[1]
    xb = ops.pack_nct(eeg)
    with torch.no_grad():
        fwd = {"EEG eval forward": lambda: tr._eeg.forward(tr._key["eeg_encoder"], eeg, xb, False),
               "fMRI eval forward": lambda: tr._fmri.forward(tr._key["fmri_encoder"], fmri, False),
               "twin heads": lambda: tr._key_embed(torch.zeros(32, 128, device="cuda"), torch.zeros(32, 64, device="cuda"))}
        for name, fn in fwd.items():
            print(f"key pass alone, graph-replayed: {name:18s} {_spread([graph_time(fn, n=5) for _ in range(rounds)])}")
    if stamps:
        for name, key in (("no key encoder", False), ("key_encoder=True", True)):
            ops.set_seed_epoch(None)
            torch.manual_seed(0)
            tr = BridgeTrainer(eeg_channels=64, dropout=0.3, bank_size=4096, ema_decay=0.999, key_encoder=key).train()
            tr.stamps = torch.zeros(16, dtype=torch.int64, device="cuda")
            acc = torch.zeros(16, dtype=torch.float64)
            for _ in range(5):
                tr.train_step(eeg, fmri)
            for _ in range(20):
                tr.train_step(eeg, fmri)
                torch.cuda.synchronize()
                s = tr.stamps.cpu().double()
                acc += (s - s[0]) / 100.0
            order = sorted((i for i in range(len(tr.STAMP_NAMES)) if key or i < 14), key=lambda i: acc[i].item())
            print(f"stamps, {name} (us after step start, graph step): " +
                  "; ".join(f"{tr.STAMP_NAMES[i]} {acc[i].item() / 20:.1f}" for i in order))


def lagpool_case(B=32, F=8, N=64, step_iters=30, rounds=5, stamps=True):
    """the lag attention pool.  (a) mm_lagpool_fwd / mm_lagpool_bwd at B = 32, F = 8, N = 64 against the same operation as a
    chain of torch ops (matmul, softmax, bmm; the backward is their autograd) - eager launches between HIP events and the
    kernels graph-replayed, interleaved rounds in the same run, median [min .. max].  (b) the C2 graph step (B = 32,
    64 ch x 1024, 32^3 voxels) of the default trainer against `fMRISequenceEncoder3D(frames=1)`: the difference is the
    pool's two graph nodes.  (c) the step at F = 4 (128 volumes of 32^3 per step: `step_schedule` issues the fMRI branch
    first) and the phase stamps of both streams at F = 1 and F = 4."""
    torch.manual_seed(0)
    x = torch.randn(B, F, N, device="cuda")
    q, c, dout = torch.randn(N, device="cuda"), torch.randn(F, device="cuda"), torch.randn(B, N, device="cuda")
    out, attw = torch.empty(B, N, device="cuda"), torch.empty(B, F, device="cuda")
    dx, dparts = torch.empty(B, F, N, device="cuda"), torch.empty(B, N + F, device="cuda")
    r = 1.0 / math.sqrt(N)
    xt, qt, ct = (t.clone().requires_grad_(True) for t in (x, q, c))

    def torch_fwd():
        a = torch.softmax(torch.matmul(xt, qt) * r + ct, dim=1)
        return torch.bmm(a.unsqueeze(1), xt).squeeze(1)

    def torch_fwd_bwd():
        xt.grad = qt.grad = ct.grad = None
        torch_fwd().backward(dout)

    def k_fwd():
        _hip.call("mm_lagpool_fwd", x, q, c, out, attw, B, F, N)

    def k_bwd():
        _hip.call("mm_lagpool_bwd", dout, x, attw, q, dx, dparts, B, F, N)
    k_fwd()
    # (x, q and c ask for no gradient: this forward keeps no tape)
    plain_fwd = lambda: torch.bmm(torch.softmax(torch.matmul(x, q) * r + c, dim=1).unsqueeze(1), x)   # noqa: E731
    cases = [("torch chain, forward (no tape)", plain_fwd), ("torch chain, forward + autograd backward", torch_fwd_bwd),
             ("mm_lagpool_fwd", k_fwd), ("mm_lagpool_bwd", k_bwd)]
    eager = {name: [] for name, _ in cases}
    replayed = {"mm_lagpool_fwd": [], "mm_lagpool_bwd": []}
    for _ in range(rounds):
        for name, fn in cases:
            eager[name].append(timeit(fn, iters=20, rounds=1))
        replayed["mm_lagpool_fwd"].append(graph_time(k_fwd))
        replayed["mm_lagpool_bwd"].append(graph_time(k_bwd))
    for name, _ in cases:
        tail = f"   graph {_spread(replayed[name])}" if name in replayed else ""
        print(f"lag pool B={B} F={F} N={N}: {name:42s} eager {_spread(eager[name])}{tail}")
    tf, tfb = statistics.median(eager[cases[0][0]]), statistics.median(eager[cases[1][0]])
    print(f"lag pool B={B} F={F} N={N}: torch chain backward alone (fwd + bwd minus the forward without a tape): {tfb - tf:.1f} us")
    from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
    from multimodal_eeg_fmri_amd.fmri_utils import fMRISequenceEncoder3D
    eeg, fmri = synthetic_pairs(32, 64, 1024, (32, 32, 32))
    seq4 = torch.randn(32, 4, 32, 32, 32, device="cuda")

    def trainer(frames):
        ops.set_seed_epoch(None)
        torch.manual_seed(0)
        enc = None if frames is None else fMRISequenceEncoder3D(frames, 64, dropout=0.3)
        return BridgeTrainer(eeg_channels=64, dropout=0.3, fmri_encoder=enc).train()
    trs = [("default trainer", trainer(None), fmri), ("sequence encoder, frames=1", trainer(1), fmri),
           ("sequence encoder, frames=4", trainer(4), seq4)]
    for _, tr, f in trs:
        tr.train_step(eeg, f)
    steps = [[] for _ in trs]
    for _ in range(rounds):
        for i, (_, tr, f) in enumerate(trs):
            steps[i].append(timeit(lambda: tr.train_step(eeg, f), iters=step_iters, rounds=1))
    t0, t1 = statistics.median(steps[0]), statistics.median(steps[1])
    for (name, tr, _), t in zip(trs, steps):
        print(f"C2 graph step B=32: {name:28s} {_spread(t)}   fmri_first={tr.schedule.fmri_first}")
    print(f"C2 graph step B=32: frames=1 against the default trainer {t1 - t0:+.1f} us ({100 * (t1 / t0 - 1):+.2f} %)")
    if stamps:
        for name, frames, f in (("frames=1", 1, fmri), ("frames=4", 4, seq4)):
            tr = trainer(frames)
            tr.stamps = torch.zeros(16, dtype=torch.int64, device="cuda")
            acc = torch.zeros(16, dtype=torch.float64)
            for _ in range(5):
                tr.train_step(eeg, f)
            for _ in range(20):
                tr.train_step(eeg, f)
                torch.cuda.synchronize()
                s = tr.stamps.cpu().double()
                acc += (s - s[0]) / 100.0
            order = sorted(range(14), key=lambda i: acc[i].item())
            print(f"stamps, sequence encoder {name}, fmri_first={tr.schedule.fmri_first} (us after step start, graph step): " +
                  "; ".join(f"{tr.STAMP_NAMES[i]} {acc[i].item() / 20:.1f}" for i in order))


def ema_case(step_iters=30, rounds=5):
    """averaged weights in the update kernel, at the default C2 trainer's bucket size, graph-replayed launches in the same
    run, interleaved rounds: mm_adamw_clip, mm_adamw_clip_ema (the same update + the average: 10 streams over the bucket
    against 8) and mm_adamw_clip followed by a separate torch ``lerp_`` of the same buffers (the two-launch form); then the
    C2 graph step (B = 32) without and with ema_decay"""
    from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
    trs = []
    for d in (0.0, 0.999):
        ops.set_seed_epoch(None)
        torch.manual_seed(0)
        trs.append(BridgeTrainer(eeg_channels=64, dropout=0.3, ema_decay=d).train())
    n = trs[0].bucket.n
    p, g, m, ema = (torch.randn(n, device="cuda") * s for s in (1.0, 0.1, 0.01, 1.0))
    v = torch.rand(n, device="cuda") * 1e-3
    state = torch.zeros(8 + 1024, device="cuda")
    state[2] = 1e-4
    _hip.call("mm_sumsq", g, state, n)
    args = (p, g, m, v, state, n, 0.9, 0.999, 1e-8, 1e-4, 1.0, 1.0, 0, None)

    def plain():
        _hip.call("mm_adamw_clip", *args)

    def fused():
        _hip.call("mm_adamw_clip_ema", *args, ema, 0.999, 1)

    def two():
        _hip.call("mm_adamw_clip", *args)
        ema.lerp_(p, 1e-3)
    cases = [("mm_adamw_clip", plain), ("mm_adamw_clip_ema", fused), ("mm_adamw_clip + torch lerp_", two)]
    times = {name: [] for name, _ in cases}
    for _ in range(rounds):
        for name, fn in cases:
            times[name].append(graph_time(fn))
    for name, _ in cases:
        print(f"update n={n} ({4 * n / 1e6:.2f} MB per stream): {name:28s} {_spread(times[name])}")
    t0, t1, t2 = (statistics.median(times[name]) for name, _ in cases)
    print(f"fused / plain {t1 / t0:.3f}x (traffic: 10 / 8 streams = 1.25x)   fused / two-launch {t1 / t2:.3f}x")
    eeg, fmri = synthetic_pairs(32, 64, 1024, (32, 32, 32))
    for tr in trs:
        for _ in range(3):
            tr.train_step(eeg, fmri)
    steps = ([], [])
    for _ in range(rounds):
        for i, tr in enumerate(trs):
            steps[i].append(timeit(lambda: tr.train_step(eeg, fmri), iters=step_iters, rounds=1))
    s0, s1 = statistics.median(steps[0]), statistics.median(steps[1])
    print(f"C2 graph step B=32: no average {_spread(steps[0])}   ema_decay=0.999 {_spread(steps[1])}   "
          f"({s1 - s0:+.1f} us, {100 * (s1 / s0 - 1):+.2f} %)")


def param_groups_case(step_iters=30, rounds=5):
    """parameter groups in the update kernel, at the default C2 trainer's bucket size, graph-replayed launches in the same
    run, interleaved rounds: mm_adamw_clip against mm_adamw_clip_groups with 1, 8 and ~200 segments (the same 8 streams over
    the bucket; the difference is the staging of the table in LDS and the per-element search); then the C2 graph step
    (B = 32) of the default trainer, with no_decay=True (the trainer's own table), and with the fMRI encoder / both encoders
    frozen"""
    from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
    setups = [("default", {}), ("no_decay", {"no_decay": True}), ("freeze fmri", {"freeze": ("fmri_encoder",)}),
              ("freeze both", {"freeze": ("eeg_encoder", "fmri_encoder")})]
    trs = []
    for _, kw in setups:
        ops.set_seed_epoch(None)
        torch.manual_seed(0)
        trs.append(BridgeTrainer(eeg_channels=64, dropout=0.3, **kw).train())
    n = trs[0].bucket.n
    p, g, m = (torch.randn(n, device="cuda") * s for s in (1.0, 0.1, 0.01))
    v = torch.rand(n, device="cuda") * 1e-3
    state = torch.zeros(8 + 1024, device="cuda")
    state[2] = 1e-4
    _hip.call("mm_sumsq", g, state, n)
    head = (p, g, m, v, state, n, 0.9, 0.999, 1e-8)
    cases = [("mm_adamw_clip", lambda: _hip.call("mm_adamw_clip", *head, 1e-4, 1.0, 1.0, 0, None))]
    for n_seg in dict.fromkeys((1, 8, 200, trs[1]._table.n_seg)):
        if n_seg == trs[1]._table.n_seg:
            ends = list(trs[1]._table.ends)
        else:
            ends = [n * (s + 1) // n_seg for s in range(n_seg)]
        end = torch.tensor(ends, dtype=torch.int64, device="cuda")
        mult = torch.tensor([(1.0, 0.1)[s % 2] for s in range(n_seg)], device="cuda")
        wd = torch.tensor([(1e-4, 0.0)[s % 2] for s in range(n_seg)], device="cuda")
        cases.append((f"mm_adamw_clip_groups {n_seg} segments",
                      lambda end=end, mult=mult, wd=wd, n_seg=n_seg: _hip.call("mm_adamw_clip_groups", *head, 1.0, 1.0, 0, None,
                                                                              end, mult, wd, n_seg)))
    times = {name: [] for name, _ in cases}
    for _ in range(rounds):
        for name, fn in cases:
            times[name].append(graph_time(fn))
    t0 = statistics.median(times["mm_adamw_clip"])
    for name, _ in cases:
        print(f"update n={n} ({4 * n / 1e6:.2f} MB per stream): {name:36s} {_spread(times[name])}  "
              f"({statistics.median(times[name]) / t0:.3f}x)")
    eeg, fmri = synthetic_pairs(32, 64, 1024, (32, 32, 32))
    for tr in trs:
        for _ in range(3):
            tr.train_step(eeg, fmri)
    steps = [[] for _ in trs]
    for _ in range(rounds):
        for i, tr in enumerate(trs):
            steps[i].append(timeit(lambda: tr.train_step(eeg, fmri), iters=step_iters, rounds=1))
    s0 = statistics.median(steps[0])
    for (name, _), tr, xs in zip(setups, trs, steps):
        print(f"C2 graph step B=32: {name:12s} bucket {tr.bucket.n:8d}  segments {tr._table.n_seg:4d}  {_spread(xs)}  "
              f"({statistics.median(xs) - s0:+.1f} us)")


def _spread(xs):
    return f"{statistics.median(xs):7.1f} us  [{min(xs):.1f} .. {max(xs):.1f}]"


def cls_case(B=32, N=128, step_iters=30, rounds=5):
    """the bridge's classification objective.  (a) the section at B = 32, bridge_dim = 128, train mode (dropout 0.3): the
    fused launches (mm_proj_heads_fwd, mm_bridge_cls_fwd, mm_bridge_cls_bwd x 2, mm_proj_heads_bwd_da; and the three
    classification launches alone) against the eager composition they stand in for - EEGfMRIBridgeFusionNet's train
    forward + WeightedCrossEntropy + backward - in the same run, interleaved rounds, median [min .. max].
    (b) the C2 graph step with classify=True against the default step of the same build."""
    from multimodal_eeg_fmri_amd import autograd
    from multimodal_eeg_fmri_amd.bridge_utils import EEGfMRIBridgeFusionNet, WeightedCrossEntropy
    torch.manual_seed(0)
    m = EEGfMRIBridgeFusionNet(128, 64, N, 2, 4, dropout=0.3).cuda().train()
    xe, xf = torch.randn(B, 128, device="cuda"), torch.randn(B, 64, device="cuda")
    y64 = torch.randint(0, 2, (B,), device="cuda")
    y32 = y64.to(torch.int32)
    cw = torch.tensor([0.8, 1.3], device="cuda")
    ce = WeightedCrossEntropy(cw).cuda()
    dz = torch.randn(B, 2 * N, device="cuda") * 0.01

    def eager():
        for q in m.parameters():
            q.grad = None
        ce(m(xe, xf), y64).backward()

    bag, keep = autograd.GradBag(), {}

    def fused(heads=True):
        with torch.no_grad():
            if heads or "sv_h" not in keep:
                keep["z"], keep["sv_h"] = ops.contrastive_embed_impl(m, xe, xf, True)
            sv_c = ops.bridge_cls_forward_impl(m, keep["sv_h"], True, y32, cw, 1.0)[3]
            da = autograd.bridge_cls_bwd(bag, sv_c)
            if heads:
                autograd.contrastive_embed_bwd_da(bag, keep["sv_h"], dz, da)

    cases = [("eager composition (model fwd + CE + bwd)", eager), ("fused section incl. both heads launches", fused),
             ("fused classification launches alone (3)", lambda: fused(False))]
    times = [[] for _ in cases]
    for _ in range(rounds):
        for i, (_, fn) in enumerate(cases):
            times[i].append(timeit(fn, iters=step_iters, rounds=1))
    print(f"classification section B={B} bridge_dim={N} (eager launches from the host, stream time):")
    for (name, _), t in zip(cases, times):
        print(f"  {name:44s} {_spread(t)}")
    g = [[] for _ in cases[1:]]
    for _ in range(rounds):
        for i, (_, fn) in enumerate(cases[1:]):
            g[i].append(graph_time(fn))
    for (name, _), t in zip(cases[1:], g):
        print(f"  {name:44s} {_spread(t)}  (graph-replayed)")
    from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
    eeg, fmri = synthetic_pairs(32, 64, 1024, (32, 32, 32))
    lab = torch.randint(0, 2, (32,), dtype=torch.int32, device="cuda")
    trs = []
    for classify in (False, True):
        ops.set_seed_epoch(None)
        torch.manual_seed(0)
        tr = BridgeTrainer(eeg_channels=64, dropout=0.3, classify=classify).train()
        args = (eeg, fmri, None, lab) if classify else (eeg, fmri)
        tr.train_step(*args)
        trs.append((tr, args))
    times = ([], [])
    for _ in range(rounds):
        for i, (tr, args) in enumerate(trs):
            times[i].append(timeit(lambda: tr.train_step(*args), iters=step_iters, rounds=1))
    td, tc = statistics.median(times[0]), statistics.median(times[1])
    print(f"C2 graph step B=32: default {_spread(times[0])}  classify {_spread(times[1])}  ({tc - td:+.1f} us, {100 * (tc / td - 1):+.2f} %)")


def tabfmri_case(step_iters=30, rounds=5):
    """the tabular fMRI encoder.  (a) forward + backward of the feature path at three shapes, train mode (dropout 0.3): the
    two fused launches (mm_fmri_tab_fwd, mm_fmri_tab_bwd) against the path they stand beside - `fMRIFusionNet`'s train-mode
    ``return_features`` forward (ops.fmri_fusion_forward, the small_autograd chain) + its autograd backward from the
    fused feature - in the same run, interleaved rounds, median [min .. max]; eager launches from the host (stream
    time), then the fused pair graph-replayed.  (b) the C2-shaped graph step (B = 32, 64 ch x 1024) with the tabular
    branch at (100, 200) against the volume branch at 32^3."""
    from multimodal_eeg_fmri_amd import autograd
    from multimodal_eeg_fmri_amd.fmri_utils import fMRIFusionNet, fMRITabularEncoder
    for B, A, C, H in ((32, 100, 200, 64), (32, 500, 4096, 64), (256, 100, 200, 64)):
        torch.manual_seed(0)
        net = fMRIFusionNet(A, C, hidden_dim=H, dropout=0.3).cuda().train()
        enc = fMRITabularEncoder.from_fusion_net(net).train()
        x = torch.randn(B, A + C, device="cuda")
        act, conn = (t.contiguous() for t in enc.split(x))
        R = torch.randn(B, H, device="cuda")
        feat = [q for n, q in net.named_parameters() if not n.startswith("head.")]

        def existing():
            for q in feat:
                q.grad = None
            net(act, conn, return_features=True)[1].backward(R)

        bag = autograd.GradBag()

        def fused():
            with torch.no_grad():
                _, sv = ops._tab_forward_impl(enc, x, True, True)
                autograd.fmri_tab_bwd(bag, sv, R)

        cases = [("fMRIFusionNet train fwd (features) + autograd bwd", existing), ("fused pair (2 launches)", fused)]
        times = [[] for _ in cases]
        for _ in range(rounds):
            for i, (_, fn) in enumerate(cases):
                times[i].append(timeit(fn, iters=step_iters, rounds=1))
        g = [graph_time(fused) for _ in range(rounds)]
        print(f"tabular fMRI feature path B={B} A={A} C={C} H={H} (fwd + bwd):")
        for (name, _), t in zip(cases, times):
            print(f"  {name:52s} {_spread(t)}")
        print(f"  {'fused pair, graph-replayed':52s} {_spread(g)}")
    from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs, synthetic_tabular_pairs
    trs = []
    for tab in (False, True):
        ops.set_seed_epoch(None)
        torch.manual_seed(0)
        enc = fMRITabularEncoder(100, 200, 64, dropout=0.3) if tab else None
        tr = BridgeTrainer(eeg_channels=64, dropout=0.3, fmri_encoder=enc).train()
        args = synthetic_tabular_pairs(32, 64, 1024, 100, 200) if tab else synthetic_pairs(32, 64, 1024, (32, 32, 32))
        tr.train_step(*args)
        trs.append((tr, args))
    times = ([], [])
    for _ in range(rounds):
        for i, (tr, args) in enumerate(trs):
            times[i].append(timeit(lambda: tr.train_step(*args), iters=step_iters, rounds=1))
    print(f"C2 graph step B=32: volume branch (32^3) {_spread(times[0])}  tabular branch (100, 200) {_spread(times[1])}")


def tabtx_case(step_iters=30, rounds=5, H=64, L=2, A=100, C=200, p=0.4):
    """the fMRI notebook's two transformer encoders (crossmodal_fmri_scr), forward + backward of both stacks, train mode at
    the notebook's dropout 0.4, at B = 8 (the notebook's batch) and B = 256: the fused path (mm_tab_tx_fwd, one launch,
    and mm_tab_tx_bwd, two launches) against torch's own eager modules - the encoders' ``project`` / ``nn.TransformerEncoder`` /
    ``norm`` containers called as the notebook calls them, autograd backward - on the same GPU in the same run:
    interleaved rounds, median [min .. max] of HIP-event times; then the fused path graph-replayed."""
    from multimodal_eeg_fmri_amd import autograd
    from multimodal_eeg_fmri_amd import small_autograd as sa
    from multimodal_eeg_fmri_amd.crossmodal_fmri_scr import ActivationEncoder, ConnectivityEncoder
    for B in (8, 256):
        torch.manual_seed(0)
        encs = [ActivationEncoder(L, A, H, p).cuda().train(), ConnectivityEncoder(L, C, H, p).cuda().train()]
        xs = [torch.randn(B, A, device="cuda"), torch.randn(B, C, device="cuda")]
        Rs = [torch.randn(B, H, device="cuda") for _ in encs]
        params = [q for e in encs for q in e.parameters()]

        def eager():
            for q in params:
                q.grad = None
            outs = [e.norm(e.transformer(e.project(x).unsqueeze(1)).squeeze(1)) for e, x in zip(encs, xs)]
            torch.autograd.backward(outs, Rs)

        bag = autograd.GradBag()

        def fused():
            with torch.no_grad():
                _, sv = ops.tab_tx_forward_impl(encs, xs, True, True)
                sa.tab_tx_bwd(bag, sv, Rs, [False, False])

        def fused_fwd():
            with torch.no_grad():
                ops.tab_tx_forward_impl(encs, xs, True, True)

        cases = [("torch eager nn.TransformerEncoder fwd + autograd bwd", eager), ("fused (1 + 2 launches)", fused),
                 ("fused, forward launch alone", fused_fwd)]
        times = [[] for _ in cases]
        for _ in range(rounds):
            for i, (_, fn) in enumerate(cases):
                times[i].append(timeit(fn, iters=step_iters, rounds=1))
        g = [graph_time(fused) for _ in range(rounds)]
        print(f"notebook transformer encoders, two stacks B={B} in=({A}, {C}) H={H} L={L} p={p} (fwd + bwd):")
        for (name, _), t in zip(cases, times):
            print(f"  {name:56s} {_spread(t)}")
        print(f"  {'fused, graph-replayed':56s} {_spread(g)}")


def timepool_case(B=32, L=256, P=128, p=0.2, step_iters=30, rounds=5):
    """tails of the EEG baselines (csrc/timepool.hip) at the notebook's widths, T = 1024 (256 steps reach the tail), train
    mode, forward + backward: the fused pair (max tail: projection, dropout and max over time in one launch, the backward a
    gather; avg tail: bins averaged first, four rows projected) against torch's eager form of what the notebook computes -
    Linear over every step, dropout, amax / adaptive_avg_pool1d, autograd backward - in fp32 on the same GPU in the same
    run: interleaved rounds, median [min .. max] of HIP-event times; then the fused pairs graph-replayed."""
    import torch.nn.functional as F
    K = 128
    torch.manual_seed(0)
    h32 = torch.randn(B, L, K, device="cuda")
    hb = h32.to(BF)
    proj = torch.nn.Conv1d(K, P, 1).cuda()
    W2 = proj.weight.detach().reshape(P, K)
    wf = ops.weights.get(proj.weight, False)[0]
    R, R4 = torch.randn(B, P, device="cuda"), torch.randn(B, 4 * P, device="cuda")
    pooled, arg = torch.empty(B, P, device="cuda"), torch.empty(B, P, dtype=torch.int32, device="cuda")
    pooled4, xbin = torch.empty(B, 4 * P, device="cuda"), torch.empty(B, 4, K, device="cuda")
    dhb, dh32 = torch.empty_like(hb), torch.empty_like(h32)
    dw, db = torch.zeros(P, K, device="cuda"), torch.zeros(P, device="cuda")
    hg = h32.clone().requires_grad_(True)
    Wg, bg = W2.clone().requires_grad_(True), proj.bias.detach().clone().requires_grad_(True)

    def max_fused():
        _hip.call("mm_timepool_max_fwd", hb, wf, proj.bias, pooled, arg, B, L, K, P, p, 7, None)
        _hip.call("mm_timepool_max_bwd", R, arg, hb, wf, dhb, dw, db, B, L, K, P, p, 7, None)

    def avg_fused():
        _hip.call("mm_timepool_avg_fwd", h32, W2, proj.bias, xbin, pooled4, B, L, K, P, 4)
        _hip.call("mm_timepool_avg_bwd", R4, xbin, W2, dh32, dw, db, B, L, K, P, 4)

    def max_eager():
        hg.grad = Wg.grad = bg.grad = None
        F.dropout(F.linear(hg, Wg, bg), p, True).amax(1).backward(R)

    def avg_eager():
        hg.grad = Wg.grad = bg.grad = None
        F.adaptive_avg_pool1d(F.linear(hg, Wg, bg).transpose(1, 2), 4).flatten(1).backward(R4)

    cases = [("max tail, torch eager (Linear, dropout, amax; autograd)", max_eager), ("max tail, fused (1 + 2 launches)", max_fused),
             ("avg tail, torch eager (Linear, adaptive_avg_pool1d; autograd)", avg_eager), ("avg tail, fused (1 + 2 launches)", avg_fused)]
    times = [[] for _ in cases]
    for _ in range(rounds):
        for i, (_, fn) in enumerate(cases):
            times[i].append(timeit(fn, iters=step_iters, rounds=1))
    g = [[graph_time(fn) for _ in range(rounds)] for fn in (max_fused, avg_fused)]
    print(f"baseline tails B={B} L={L} K={K} P={P} p={p} (fwd + bwd; the projected tensor would be {B * L * P * 4 / 1e6:.1f} MB in fp32):")
    for (name, _), t in zip(cases, times):
        print(f"  {name:62s} {_spread(t)}")
    print(f"  {'max tail, fused, graph-replayed':62s} {_spread(g[0])}")
    print(f"  {'avg tail, fused, graph-replayed':62s} {_spread(g[1])}")


def aug_case(B=32, C=64, T=1024, vol=(32, 32, 32), step_iters=30):
    """EEG augmentation (csrc/augment.hip) at the C2 shape: mm_stage_inputs alone against the plan + mm_stage_inputs_aug pair
    at p = 0.3 and p = 1 - issued eagerly (what a training loop pays: host issue included) and replayed from a hipGraph
    (the kernels alone), HIP events, interleaved rounds; bytes: the EEG batch read once / twice, the bf16 operand and the
    fMRI batch written, the fMRI batch read - then the C2 graph step with and without an augmenter"""
    from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
    from multimodal_eeg_fmri_amd.crossmodal_eeg_scr import EEGTransforms
    eeg, fmri = synthetic_pairs(B, C, T, vol)
    cp = ops.cpad(C)
    xb, fdst = torch.empty(B, T, cp, dtype=BF, device="cuda"), torch.empty_like(fmri)
    step = [0]
    plan = torch.empty(ops.eeg_augment_plan_layout(B, C, T)[0], dtype=torch.int32, device="cuda")

    def aug(p):
        step[0] += 1
        ops.eeg_augment_into(eeg, xb, None, p_noise=p, p_drop=p, noise_factor=0.05, n_drop=max(1, int(0.1 * C)), seed=1,
                             step=step[0], fmri_dst=fdst, fmri_src=fmri, plan=plan)
    cases = [("mm_stage_inputs", lambda: _hip.call("mm_stage_inputs", eeg, xb, None, B, C, T, cp, fdst, fmri, fmri.numel()), 1),
             ("plan + mm_stage_inputs_aug p = 0.3", lambda: aug(0.3), 2), ("plan + mm_stage_inputs_aug p = 1", lambda: aug(1.0), 2)]
    times, gtimes = [[] for _ in cases], [[] for _ in cases]
    for _ in range(5):
        for i, (_, fn, _) in enumerate(cases):
            times[i].append(timeit(fn, iters=200, rounds=1))
            gtimes[i].append(graph_time(fn, n=50))
    for (name, _, reads), t, gt in zip(cases, times, gtimes):
        us, gus = statistics.median(t), statistics.median(gt)
        nbytes = reads * eeg.numel() * 4 + xb.numel() * 2 + 2 * fmri.numel() * 4
        print(f"{name:38s} eager {us:6.2f} us (min {min(t):5.2f}, max {max(t):5.2f})  in a graph {gus:6.2f} us (min {min(gt):5.2f}, "
              f"max {max(gt):5.2f})  {nbytes / 1e6:5.1f} MB  {nbytes / gus / 1e6:5.2f} TB/s")
    trs = []
    for augment in (None, EEGTransforms(p=0.3, seed=1), EEGTransforms(p=1.0, seed=1)):
        ops.set_seed_epoch(None)
        torch.manual_seed(0)
        tr = BridgeTrainer(eeg_channels=C, dropout=0.3, augment=augment).train()
        tr.train_step(eeg, fmri)
        trs.append(tr)
    times = [[] for _ in trs]
    for _ in range(5):
        for i, tr in enumerate(trs):
            times[i].append(timeit(lambda: tr.train_step(eeg, fmri), iters=step_iters, rounds=1))
    base = statistics.median(times[0])
    for name, t in zip(("no augmenter", "augment p = 0.3", "augment p = 1"), times):
        us = statistics.median(t)
        print(f"C2 graph step B={B}: {name:16s} {us:7.1f} us  (min {min(t):6.1f}, max {max(t):6.1f})  {100 * (us / base - 1):+.2f} %")


def taug_case(B=32, C=64, T=1024, vol=(32, 32, 32), step_iters=30):
    """temporal EEG augmentation (csrc/augment.hip's mm_stage_inputs_taug) at the C2 shape, in one run: the
    parent's mm_stage_inputs and plan + mm_stage_inputs_aug pair against the time-only launch and plan + mm_stage_inputs_taug -
    issued eagerly and replayed from a hipGraph, HIP events, interleaved rounds - then the C2 graph step with and without the
    augmenter"""
    from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
    from multimodal_eeg_fmri_amd.crossmodal_eeg_scr import EEGTimeTransforms, EEGTransforms
    eeg, fmri = synthetic_pairs(B, C, T, vol)
    cp = ops.cpad(C)
    xb, fdst = torch.empty(B, T, cp, dtype=BF, device="cuda"), torch.empty_like(fmri)
    step = [0]
    plan = torch.empty(ops.eeg_augment_plan_layout(B, C, T)[0], dtype=torch.int32, device="cuda")
    default, every = EEGTimeTransforms(seed=1), EEGTimeTransforms(p_shift=1.0, p_scale=1.0, p_invert=1.0, p_mask=1.0, seed=1)
    base = EEGTransforms(p=0.3, seed=1)

    def aug():
        step[0] += 1
        ops.eeg_augment_into(eeg, xb, None, step=step[0], fmri_dst=fdst, fmri_src=fmri, plan=plan, **base.kernel_args(C))

    def taug(time_aug, with_base):
        step[0] += 1
        ops.eeg_time_augment_into(eeg, xb, None, time_args=time_aug.kernel_args(T), base_args=base.kernel_args(C) if with_base else None,
                                  step=step[0], fmri_dst=fdst, fmri_src=fmri, plan=plan)
    cases = [("mm_stage_inputs", lambda: _hip.call("mm_stage_inputs", eeg, xb, None, B, C, T, cp, fdst, fmri, fmri.numel()), 1),
             ("plan + mm_stage_inputs_aug p = 0.3", aug, 2),
             ("mm_stage_inputs_taug defaults", lambda: taug(default, False), 1),
             ("mm_stage_inputs_taug every p = 1", lambda: taug(every, False), 1),
             ("plan + mm_stage_inputs_taug p = 0.3", lambda: taug(default, True), 2)]
    times, gtimes = [[] for _ in cases], [[] for _ in cases]
    for _ in range(5):
        for i, (_, fn, _) in enumerate(cases):
            times[i].append(timeit(fn, iters=200, rounds=1))
            gtimes[i].append(graph_time(fn, n=50))
    for (name, _, reads), t, gt in zip(cases, times, gtimes):
        us, gus = statistics.median(t), statistics.median(gt)
        nbytes = reads * eeg.numel() * 4 + xb.numel() * 2 + 2 * fmri.numel() * 4
        print(f"{name:38s} eager {us:6.2f} us (min {min(t):5.2f}, max {max(t):5.2f})  in a graph {gus:6.2f} us (min {min(gt):5.2f}, "
              f"max {max(gt):5.2f})  {nbytes / 1e6:5.1f} MB  {nbytes / gus / 1e6:5.2f} TB/s")
    # After the graph captures above, the FOURTH trainer built in this process replays its step ~210 us slower whatever its
    # configuration (measured with an augmenter-free trainer, `augment=` alone and both augmenters in that place; the
    # trainers before and after it are not affected, nor is a fourth trainer in a process without those captures - DESIGN.md
    # 5u; the cause was not looked for).  So the fourth place holds a second augmenter-free trainer, which shows the effect.
    trs, names = [], ("no augmenter", "eeg_time_augment defaults", "eeg_time_augment p = 1", "no augmenter, 4th trainer",
                      "augment p = 0.3", "defaults + augment p = 0.3")
    for time_aug, eaug in ((None, None), (default, None), (every, None), (None, None), (None, base), (default, base)):
        ops.set_seed_epoch(None)
        torch.manual_seed(0)
        tr = BridgeTrainer(eeg_channels=C, dropout=0.3, augment=eaug, eeg_time_augment=time_aug).train()
        tr.train_step(eeg, fmri)
        trs.append(tr)
    times = [[] for _ in trs]
    for _ in range(5):
        for i, tr in enumerate(trs):
            times[i].append(timeit(lambda: tr.train_step(eeg, fmri), iters=step_iters, rounds=1))
    ref = statistics.median(times[0])
    for name, t in zip(names, times):
        us = statistics.median(t)
        print(f"C2 graph step B={B}: {name:28s} {us:7.1f} us  (min {min(t):6.1f}, max {max(t):6.1f})  {100 * (us / ref - 1):+.2f} %")


def volaug_case(B=32, C=64, T=1024, vol=(32, 32, 32), odd=(91, 109, 91), step_iters=30):
    """fMRI volume augmentation (csrc/volume_augment.hip) at the C2 shape: mm_stage_inputs alone against the staging sequences
    of a trainer with a volume augmenter - the kernel pair + mm_pack_nct_bf16, and the kernel pair + the EEG augmenter's pair
    without its fMRI copy - issued eagerly and replayed from a hipGraph, HIP events, interleaved rounds; the kernel pair alone
    on a batch of odd MNI volumes; then the C2 graph step with and without `fmri_augment`"""
    from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
    from multimodal_eeg_fmri_amd.crossmodal_eeg_scr import EEGTransforms
    from multimodal_eeg_fmri_amd.fmri_utils import VolumeTransforms
    eeg, fmri = synthetic_pairs(B, C, T, vol)
    cp = ops.cpad(C)
    xb, fdst = torch.empty(B, T, cp, dtype=BF, device="cuda"), torch.empty_like(fmri)
    step = [0]
    eplan = torch.empty(ops.eeg_augment_plan_layout(B, C, T)[0], dtype=torch.int32, device="cuda")
    vplan = torch.empty(ops.volume_augment_plan_layout(B, *vol)[0], dtype=torch.int32, device="cuda")
    default, every = VolumeTransforms(seed=1), VolumeTransforms(1.0, 1.0, 2, 1.0, 0.1, 1.0, 0.05, 1.0, seed=1)

    def pair(aug, src=fmri, dst=fdst, plan=vplan):
        step[0] += 1
        ops.volume_augment_into(src, dst, step=step[0], plan=plan, **aug.kernel_args(src.shape))

    def vol_then_pack(aug):
        pair(aug)
        _hip.call("mm_pack_nct_bf16", eeg, xb, B, C, T, cp)

    def vol_then_eeg(aug, p):
        pair(aug)
        ops.eeg_augment_into(eeg, xb, None, p_noise=p, p_drop=p, noise_factor=0.05, n_drop=max(1, int(0.1 * C)), seed=1,
                             step=step[0], plan=eplan)
    nf, ne = fmri.numel() * 4, eeg.numel() * 4
    cases = [("mm_stage_inputs", lambda: _hip.call("mm_stage_inputs", eeg, xb, None, B, C, T, cp, fdst, fmri, fmri.numel()), ne + xb.numel() * 2 + 2 * nf),
             ("volume pair alone, defaults", lambda: pair(default), 3 * nf),
             ("volume pair alone, every p = 1", lambda: pair(every), 3 * nf),
             ("volume pair (defaults) + mm_pack_nct_bf16", lambda: vol_then_pack(default), ne + xb.numel() * 2 + 3 * nf),
             ("volume pair (p = 1) + mm_pack_nct_bf16", lambda: vol_then_pack(every), ne + xb.numel() * 2 + 3 * nf),
             ("volume pair (defaults) + EEG pair p = 0.3", lambda: vol_then_eeg(default, 0.3), 2 * ne + xb.numel() * 2 + 3 * nf)]
    times, gtimes = [[] for _ in cases], [[] for _ in cases]
    for _ in range(5):
        for i, (_, fn, _) in enumerate(cases):
            times[i].append(timeit(fn, iters=200, rounds=1))
            gtimes[i].append(graph_time(fn, n=50))
    for (name, _, nbytes), t, gt in zip(cases, times, gtimes):
        us, gus = statistics.median(t), statistics.median(gt)
        print(f"{name:44s} eager {us:6.2f} us (min {min(t):5.2f}, max {max(t):5.2f})  in a graph {gus:6.2f} us (min {min(gt):5.2f}, "
              f"max {max(gt):5.2f})  {nbytes / 1e6:5.1f} MB  {nbytes / gus / 1e6:5.2f} TB/s")
    # the odd MNI volume: the kernel pair alone (scalar loads in the plan, rows that start at any address)
    g = torch.Generator().manual_seed(3)
    big = torch.randn(4, 1, *odd, generator=g).cuda()
    bdst, bplan = torch.empty_like(big), torch.empty(ops.volume_augment_plan_layout(4, *odd)[0], dtype=torch.int32, device="cuda")
    for name, aug in (("defaults", default), ("every p = 1", every)):
        t = [timeit(lambda: pair(aug, big, bdst, bplan), iters=100, rounds=1) for _ in range(5)]
        gt = [graph_time(lambda: pair(aug, big, bdst, bplan), n=50) for _ in range(5)]
        nbytes = 3 * big.numel() * 4
        print(f"volume pair alone, B = 4 of {odd[0]}x{odd[1]}x{odd[2]}, {name:12s} eager {statistics.median(t):6.2f} us (min {min(t):5.2f}, max "
              f"{max(t):5.2f})  in a graph {statistics.median(gt):6.2f} us (min {min(gt):5.2f}, max {max(gt):5.2f})  {nbytes / 1e6:5.1f} MB  "
              f"{nbytes / statistics.median(gt) / 1e6:5.2f} TB/s")
    trs, names = [], ("no augmenter", "fmri_augment defaults", "fmri_augment p = 1", "fmri_augment defaults + augment p = 0.3")
    for vaug, eaug in ((None, None), (default, None), (every, None), (default, EEGTransforms(p=0.3, seed=1))):
        ops.set_seed_epoch(None)
        torch.manual_seed(0)
        tr = BridgeTrainer(eeg_channels=C, dropout=0.3, augment=eaug, fmri_augment=vaug).train()
        tr.train_step(eeg, fmri)
        trs.append(tr)
    times = [[] for _ in trs]
    for _ in range(5):
        for i, tr in enumerate(trs):
            times[i].append(timeit(lambda: tr.train_step(eeg, fmri), iters=step_iters, rounds=1))
    base = statistics.median(times[0])
    for name, t in zip(names, times):
        us = statistics.median(t)
        print(f"C2 graph step B={B}: {name:40s} {us:7.1f} us  (min {min(t):6.1f}, max {max(t):6.1f})  {100 * (us / base - 1):+.2f} %")


def xai_case(B=32, C=64, T=1024, vol=(32, 32, 32), n_steps=50, rounds=5):
    """attribution (csrc/xai.hip, BridgeTrainer.explain) at the C2 shape.  (1) the three streaming kernels alone: GB/s of
    the bytes each must move, beside the ~6.3 TB/s a float4 copy reaches on this part.  (2) integrated gradients of the
    matching score, n_steps points, through the SAME trainer: the reference's protocol (eeg_xai_analysis.py:196-225: one
    forward/backward per step, every gradient carried to the host as numpy, mean and |.| on the host) against the batched
    engine; HIP events, the two forms interleaved round by round, medians."""
    import numpy as np
    from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer, synthetic_pairs
    HBM = 6.3e3                                                  # GB/s, achievable (float4 copy)
    n = B * C * T
    base = torch.randn(1, C, T, device="cuda")

    def ring(make, nbytes):
        """enough copies that a pass over them all is well beyond the 256 MB Infinity Cache: every launch reads and writes
        buffers the previous ~1 GiB of launches did not touch, so the figure is an HBM figure"""
        return [make() for _ in range(max(2, int(math.ceil((1 << 30) / nbytes))))]

    def rotating(call, *rings):
        state = {"i": 0}

        def fn():
            i = state["i"]
            state["i"] = i + 1
            call(*[r[i % len(r)] for r in rings])
        return fn
    xs = ring(lambda: torch.randn(B, C, T, device="cuda"), n * 4)
    for S in (1, 9, 25):
        outs = ring(lambda: torch.empty(S * B, C, T, device="cuda"), S * n * 4)
        us = timeit(rotating(lambda x, out: _hip.call("mm_xai_interp", x, base, 1, out, n_steps, 0, S, B, C * T), xs, outs))
        gb = (S + 1) * n * 4 / 1e9
        print(f"xai_interp  S={S:2d} ({B},{C},{T}) mean baseline, {len(xs)} / {len(outs)} rotating buffers: {us:8.1f} us  {gb / us * 1e6:7.0f} GB/s ({gb / us * 1e6 / HBM * 100:4.1f} % of {HBM:.0f})")
        accs = ring(lambda: torch.zeros(B, C, T, device="cuda"), n * 4)
        us = timeit(rotating(lambda out, acc: _hip.call("mm_xai_accum", out, acc, S, n), outs, accs))
        gb = (S + 2) * n * 4 / 1e9
        print(f"xai_accum   S={S:2d}: {us:8.1f} us  {gb / us * 1e6:7.0f} GB/s ({gb / us * 1e6 / HBM * 100:4.1f} %)")
        del outs
    accs = ring(lambda: torch.randn(B, C, T, device="cuda"), n * 4)
    attrs = ring(lambda: torch.empty(B, C, T, device="cuda"), n * 4)
    chan = torch.empty(B, C, device="cuda")
    for label, ch in (("rows + channel means", chan), ("flat", None)):
        us = timeit(rotating(lambda x, acc, attr: _hip.call("mm_xai_finish", x, base, 1, acc, attr, ch, B, C, T, n_steps, 0), xs, accs, attrs))
        gb = 3 * n * 4 / 1e9
        print(f"xai_finish  {label}: {us:8.1f} us  {gb / us * 1e6:7.0f} GB/s ({gb / us * 1e6 / HBM * 100:4.1f} %)")
    del xs, accs, attrs
    torch.manual_seed(0)
    tr = BridgeTrainer(eeg_channels=C, dropout=0.3, mode="manual").train()
    eeg, fmri = synthetic_pairs(B, C, T, vol)

    def reference_protocol():
        tr.eval()
        ops.weights_changed()
        g0 = tr.bucket.g.clone()
        ge, gf = [], []
        for alpha in np.linspace(0, 1, n_steps):
            e = (float(alpha) * eeg).requires_grad_(True)
            f = (float(alpha) * fmri).requires_grad_(True)
            ze, zf = tr.head.embed(tr.eeg_encoder(e), tr.fmri_encoder(f))
            z = ops._packed_pair(ze, zf)
            a, b = torch.autograd.grad(z, [e, f], ops.xai_pair_score(z)[1])
            ge.append(a.detach().cpu().numpy())
            gf.append(b.detach().cpu().numpy())
        res = np.abs(eeg.cpu().numpy() * np.mean(ge, axis=0)), np.abs(fmri.cpu().numpy() * np.mean(gf, axis=0))
        tr.train()
        tr.bucket.g.copy_(g0)
        return res

    def batched():
        out = tr.explain(eeg, fmri, n_steps=n_steps)
        return out["eeg"].cpu().numpy(), out["fmri"].cpu().numpy()
    ra, rb = reference_protocol(), batched()                     # warm-up of both, and the two results side by side
    for k, name in enumerate(("eeg", "fmri")):
        print(f"batched vs per-step result, {name}: rel-L2 {np.linalg.norm(ra[k] - rb[k]) / np.linalg.norm(ra[k]):.2e}")
    import gc

    def peak_of(fn):
        """peak allocation of one call above what is held before it (the per-step protocol's dead tapes collected first)"""
        gc.collect()
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - held) / 2 ** 20
    for cs in (1, 2, 4, 8):
        print(f"batched, chunk_steps={cs}: peak {peak_of(lambda: tr.explain(eeg, fmri, n_steps=n_steps, chunk_steps=cs)):.0f} MiB above what was held")
    print(f"batched, memory rule (budget {ops.XAI_BUDGET_BYTES / 2 ** 20:.0f} MiB per chunk): peak {peak_of(batched):.0f} MiB above what was held")
    times = {"per-step + host round trips": [], "batched engine": []}
    for _ in range(rounds):
        for label, fn in (("per-step + host round trips", reference_protocol), ("batched engine", batched)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[label].append(a.elapsed_time(b))
    for label, t in times.items():
        print(f"integrated gradients B={B} {C}x{T} {vol} n_steps={n_steps}, {label}: median {statistics.median(t):8.1f} ms  (rounds {[round(v, 1) for v in t]})")
    m = {k: statistics.median(v) for k, v in times.items()}
    print(f"speed-up of the batched engine: {m['per-step + host round trips'] / m['batched engine']:.2f} x")


def gat_case(B=32, N=64, H=4, C=32, dense=True):
    """one GATv2 layer (csrc/gnn.hip) on the all-pairs graph, forward and backward, the W_l | W_r linear beside it, the
    edge variant at D = 1 and D = 3 with its ratio to the plain kernels, and a GNNConnectivityEncoder eval forward for the whole batch vs one sample per call (the reference's loop shape)"""
    import multimodal_eeg_fmri_amd.enhanced_models_v4 as E
    adj = ~torch.eye(N, dtype=torch.bool) if dense else torch.rand(N, N) < 0.1
    ei = adj.nonzero().t().contiguous().cuda()
    g = ops.gat_graph(ei, N)
    HC, Eg = H * C, g.num_edges
    x = torch.randn(B * N, HC, device="cuda")
    W = torch.randn(2 * HC, HC, device="cuda") / math.sqrt(HC)
    b = torch.randn(2 * HC, device="cuda")
    att = torch.randn(H, C, device="cuda") / math.sqrt(C)
    bias = torch.randn(HC, device="cuda")
    xlr = torch.empty(B * N, 2 * HC, device="cuda")
    out, pre, dout = (torch.empty(B, N, HC, device="cuda") for _ in range(3))
    dout.normal_()
    alpha, ds = torch.empty(B, H, Eg, device="cuda"), torch.empty(B, H, Eg, device="cuda")
    dz, part = torch.empty(B, N, HC, device="cuda"), torch.empty(B, 2, HC, device="cuda")
    dxlr, dx = torch.empty_like(xlr), torch.empty_like(x)
    dW, db, datt, dbias = torch.zeros_like(W), torch.zeros_like(b), torch.zeros_like(att), torch.zeros_like(bias)
    xr, dxr = xlr.data_ptr() + 4 * HC, dxlr.data_ptr() + 4 * HC
    act = ops.ACT["gelu"]

    def lin_f():
        _hip.call("mm_small_linear_fwd", x, W, b, None, None, xlr, None, B * N, HC, 2 * HC, 0, 0.0, 0, None)

    def lin_b():
        _hip.call("mm_small_linear_bwd", dxlr, x, W, dx, dW, db, B * N, HC, 2 * HC)

    def fwd(p=0.0):
        _hip.call("mm_gatv2_fwd", xlr, xr, 2 * HC, att, bias, g.rowptr, g.col, out, pre, alpha, B, N, H, C, Eg, 0.2, act, p, 7, None)

    def bwd(p=0.0):
        _hip.call("mm_gatv2_bwd", dout, pre, xlr, xr, 2 * HC, att, alpha, g.rowptr, g.col, g.colptr, g.row, g.perm, dxlr,
                  dxr, datt, dbias, ds, dz, part, B, N, H, C, Eg, 0.2, act, p, 7, None)
    lin_f()
    tag = f"gat B={B} N={N} H={H} C={C} E'={Eg}"
    rows = B * N * HC * 4
    fb = 2 * rows + 2 * rows + B * H * Eg * 4                        # xl, xr in; out, pre out; alpha out
    bb = 2 * rows + 2 * rows + 2 * rows + 2 * rows + 3 * B * H * Eg * 4   # xl, xr, dout, pre in; dz, dxl, dxr out (+ dz back in); alpha in, ds out + in
    plain = {}
    for name, fn, nbytes in (("linear W_l|W_r fwd", lin_f, B * N * 3 * HC * 4), ("gatv2 fwd p=0", fwd, fb),
                             ("gatv2 fwd p=0.3", lambda: fwd(0.3), fb), ("gatv2 bwd p=0", bwd, bb),
                             ("gatv2 bwd p=0.3", lambda: bwd(0.3), bb), ("linear W_l|W_r bwd", lin_b, B * N * 4 * HC * 4)):
        us = timeit(fn)
        plain[name] = us
        print(f"{tag} {name:22s}: {us:8.1f} us   {nbytes / 1e6:6.2f} MB moved  {nbytes / us / 1e3:7.1f} GB/s")
    # edge variant (mm_gatv2_edge_*): per-sample attributes, D raw features per edge projected inside the score loop
    for D in (1, 3):
        we = torch.randn(HC, D, device="cuda") / math.sqrt(D)
        listed = torch.randn(B, ei.shape[1], D, device="cuda")
        ea, dea, dlisted = torch.empty(B, Eg, D, device="cuda"), torch.empty(B, Eg, D, device="cuda"), torch.empty_like(listed)
        dwe, wpart, epart = torch.zeros_like(we), torch.empty(B, HC, D, device="cuda"), torch.empty(B, H, Eg, D, device="cuda")

        def pack():
            _hip.call("mm_gatv2_edge_pack", listed, g.eid, g.rowptr, g.indeg, ea, B, N, ei.shape[1], Eg, D, 1, 0.0)

        def pack_b():
            _hip.call("mm_gatv2_edge_pack_bwd", dea, g.pos, g.tgt, g.rowptr, g.indeg, dlisted, B, N, ei.shape[1], Eg, D, 1)

        def efwd():
            _hip.call("mm_gatv2_edge_fwd", xlr, xr, 2 * HC, att, bias, we, ea, 1, g.rowptr, g.col, out, pre, alpha, B, N, H, C,
                      Eg, D, 0.2, act, 0.0, 7, None)

        def ebwd(with_dea=True):
            _hip.call("mm_gatv2_edge_bwd", dout, pre, xlr, xr, 2 * HC, att, we, ea, 1, alpha, g.rowptr, g.col, g.colptr, g.row,
                      g.perm, dxlr, dxr, datt, dbias, dwe, dea if with_dea else None, ds, dz, part, wpart,
                      epart if with_dea else None, B, N, H, C, Eg, D, 0.2, act, 0.0, 7, None)
        pack()
        eb = B * Eg * D * 4
        for name, fn, nbytes, ref in ((f"edge D={D} pack", pack, 2 * eb, None), (f"edge D={D} fwd p=0", efwd, fb + eb, "gatv2 fwd p=0"),
                                      (f"edge D={D} bwd p=0", ebwd, bb + 3 * eb + 2 * H * eb, "gatv2 bwd p=0"),
                                      (f"edge D={D} bwd no d ea", lambda: ebwd(False), bb + 2 * eb, "gatv2 bwd p=0"),
                                      (f"edge D={D} pack bwd", pack_b, 2 * eb, None)):
            us = timeit(fn)
            ratio = f"  {us / plain[ref]:5.2f} x plain" if ref else ""
            print(f"{tag} {name:22s}: {us:8.1f} us   {nbytes / 1e6:6.2f} MB moved  {nbytes / us / 1e3:7.1f} GB/s{ratio}")
    enc = E.GNNConnectivityEncoder(num_nodes=N, num_conn_types=3, hidden_dim=HC, num_heads=H).cuda().eval()
    conn = torch.rand(B, N, N, 3, device="cuda")
    with torch.no_grad():
        whole = timeit(lambda: enc(conn, ei), iters=5)
        singles = [conn[i:i + 1].contiguous() for i in range(B)]
        loop = timeit(lambda: [enc(c1, ei) for c1 in singles], iters=2)
    print(f"{tag} encoder eval forward: whole batch {whole:8.1f} us   one sample per call x {B} {loop:8.1f} us   ({loop / whole:.1f} x)")


def ffnbwd_case(M=16384, n1=512, p=0.3):
    """a transformer block's row-wise backward at the C2 shape: the two launches (FFN-2 data gradient, then FFN-1 data
    gradient + norm2 backward + out-projection data gradient) against mm_ffn_rows_bwd, and the traffic each form moves"""
    g = torch.Generator().manual_seed(5)

    def img(cout, cin):                      # data-gradient weight image of a Linear(cin -> cout): cin rows of cout
        wd = torch.empty(cin, 1, cout, dtype=BF, device="cuda")
        wf = torch.empty(cout, 1, cin, dtype=BF, device="cuda")
        w = (torch.randn(cout, cin, 1, generator=g) / math.sqrt(cin)).cuda()
        _hip.call("mm_prep_conv_weight", w, wf, wd, cout, cin, 1, cin, cout)
        return wd
    w2d, w1d, wod = img(128, n1), img(n1, 128), img(128, 128)
    dy2 = (torch.randn(M, 128, generator=g) * 0.1).cuda().to(BF)
    z = torch.randn(M, n1, generator=g).cuda().to(BF)
    x1 = torch.randn(M, 128, generator=g).cuda()
    stat = torch.stack([x1.mean(1), (x1.var(1, unbiased=False) + 1e-5).rsqrt()], 1).contiguous()
    gam = (0.5 + torch.rand(128, generator=g)).cuda()
    dres = (torch.randn(M, 128, generator=g) * 0.1).cuda()
    dz = torch.empty(M, n1, dtype=BF, device="cuda")
    dx1 = torch.empty(M, 128, device="cuda")
    dyo, do = torch.empty(M, 128, dtype=BF, device="cuda"), torch.empty(M, 128, dtype=BF, device="cuda")
    dgb = torch.zeros(32, 2, 128, device="cuda")

    def first():
        _hip.call("mm_conv1d_fwd", dy2, w2d, 1, M, 128, n1, 1, 0, None, None, 0, None, None, 1, None, None, dz, None, p, 92, None,
                  z, ops.ACT["gelu"])

    def second():
        _hip.call("mm_linear_dgrad_ln_bwd_gemm2", dz, w1d, M, n1, x1, stat, gam, dres, dx1, dyo, dgb, p, 91, None, wod, do, 0)

    def chain():
        first()
        second()

    def fused():
        _hip.call("mm_ffn_rows_bwd", dy2, w2d, M, n1, z, ops.ACT["gelu"], p, 92, dz, w1d, x1, stat, gam, dres, 0, dx1, dyo, dgb,
                  p, 91, None, wod, do)
    t1, t2, tc, tf = timeit(first), timeit(second), timeit(chain), timeit(fused)
    rows = M * 128
    mb_f = (2 * rows + 2 * 2 * M * n1 + 3 * 4 * rows + 2 * 2 * rows) / 1e6          # dy2, z + dz, x1 + dres + dx1, dyo + do
    mb_c = mb_f + 2 * M * n1 / 1e6                                                   # + the dz read-back
    print(f"ffnbwd M={M} n1={n1} p={p}: FFN-2 dgrad {t1:6.1f} us + FFN-1 dgrad/norm2/out-proj {t2:6.1f} us; back to back {tc:6.1f} us "
          f"({mb_c / tc:5.2f} TB/s of {mb_c:.1f} MB); fused {tf:6.1f} us ({mb_f / tf:5.2f} TB/s of {mb_f:.1f} MB)")


def main():
    flt = sys.argv[1] if len(sys.argv) > 1 else ""
    if flt == "ffnbwd":
        ffnbwd_case()
        return
    if flt == "attnmap":
        attnmap_case(L=512)
        attnmap_case(L=1024)
        return
    if flt.startswith("gat"):          # gat[:B,N,H,C]
        dims = [int(d) for d in flt.split(":", 1)[1].split(",")] if ":" in flt and flt.split(":", 1)[1] else []
        gat_case(*dims)
        return
    if flt == "xai":
        xai_case()
        return
    if flt == "cls":
        cls_case()
        return
    if flt == "bank":
        bank_case()
        return
    if flt == "neighbours":
        neighbours_case()
        return
    if flt == "retrieval_masked":
        retrieval_masked_case()
        return
    if flt == "key":
        key_case()
        return
    if flt == "ema":
        ema_case()
        return
    if flt == "lagpool":
        lagpool_case()
        return
    if flt == "pgroups":
        param_groups_case()
        return
    if flt == "tabfmri":
        tabfmri_case()
        return
    if flt == "tabtx":
        tabtx_case()
        return
    if flt == "aug":
        aug_case()
        return
    if flt == "taug":
        taug_case()
        return
    if flt == "volaug":
        volaug_case()
        return
    if flt == "timepool":
        timepool_case()
        return
    if flt == "groups":
        groups_case()
        return
    if flt == "sigmoid":
        sigmoid_case()
        return
    if flt == "retr":
        retr_case(16384, 16384, 128, 10, vs_torch=True)
        retr_case(65536, 65536, 128, 10)
        return
    if flt in ("step", "step5"):
        step_case("c5" if flt == "step5" else "c2")
        return
    if flt in ("l1", "pmcl1"):
        l1_case()
        return
    if flt == "sus4":
        wres_sustained_case(32, 32, 32, 24)
        return
    if flt == "sus2":
        wres_sustained_case(32, 16, 16, 16, launches=1200)
        return
    if "floor" in flt:
        floor_case()
    M = 32 * 512
    if "lin" in flt or not flt:
        linear_case(M, 128, 384)
        linear_case(M, 128, 128, out_f32=True, residual=True)
        linear_case(M, 128, 512, act="gelu")
        linear_case(M, 512, 128, out_f32=True, residual=True)
        linear_case(M, 384, 128)
    if "conv1" in flt or not flt:
        conv1d_case(32, 1024, 64, 64, 7)
        conv1d_case(32, 1024, 64, 128, 5)
        conv1d_case(32, 512, 128, 128, 3)
        conv1d_wgrad_case(32, 1024, 64, 64, 7)
        conv1d_wgrad_case(32, 1024, 64, 128, 5)
        conv1d_wgrad_case(32, 512, 128, 128, 3)
        conv1d_wgrad_case(1, M, 128, 512, 1)
    if "split" in flt:
        split_case()
        return
    if "bn" in flt:
        bn_bwd_case(32, 512, 128, 1, True)
        bn_bwd_case(32, 1024, 128, 2, False)
        bn_bwd_case(32, 1024, 64, 1, False)
        return
    if "pmc3d" in flt:
        conv3d_case(32, 16, 32, 64, wgrad=False)
        return
    if "c4b" in flt:                # the two roofline shapes only
        conv3d_dims_case(32, 32, 32, 24, 32, 64)
        conv3d_dims_case(32, 16, 16, 16, 32, 64)
        return
    if "pmc4" in flt:               # BASELINE config #4: layer 2 at 32 x 32 x 24
        conv3d_dims_case(32, 32, 32, 24, 32, 64)
        return
    if "attn" in flt:               # attn[:dh,dh,...]: head dims to time (default 32), e.g. attn:16,32,64
        dims = [int(d) for d in flt.split(":", 1)[1].split(",")] if ":" in flt else [32]
        for dh in dims:
            for p_ in (0.0, 0.1, 0.3):
                attn_case(p=p_, head_dim=dh)
        return
    if "c4" in flt:                 # full-resolution fMRI (64x64x48): layer 2 runs at 32x32x24
        for B in (4, 8, 32):
            conv3d_dims_case(B, 32, 32, 24, 32, 64)
        conv3d_dims_case(32, 16, 16, 16, 32, 64)
        return
    if flt == "pmcs":               # layer 3 forward only (PMC passes of the streaming kernel)
        conv3d_dims_case(32, 8, 8, 8, 64, 128)
        return
    if "stream" in flt:
        # conv3d_stream.hip: layer 3 forward, its data gradient, layer 2's data gradient (C2, then config #4 volumes)
        conv3d_dims_case(32, 8, 8, 8, 64, 128)
        conv3d_dims_case(32, 8, 8, 8, 128, 64, dgrad=True)
        conv3d_dims_case(32, 16, 16, 16, 64, 32, dgrad=True)
        conv3d_dims_case(32, 16, 16, 12, 64, 128)
        conv3d_dims_case(32, 16, 16, 12, 128, 64, dgrad=True)
        conv3d_dims_case(32, 32, 32, 24, 64, 32, dgrad=True)
    if flt == "wgrad3":
        conv3d_case(32, 16, 32, 64, fwd=False)
        conv3d_case(32, 8, 64, 128, fwd=False)
        return
    if "conv3" in flt or not flt:
        conv3d_case(32, 16, 32, 64)
        conv3d_case(32, 8, 64, 128)


if __name__ == "__main__":
    main()
