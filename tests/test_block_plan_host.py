"""A transformer block's launch plan (ops.block_plan) and its backward counterpart (autograd.block_bwd_plan) are pure
functions of shapes, consumers and the A/B knobs: every named form over a table, without a GPU."""
import pytest

from multimodal_eeg_fmri_amd import autograd, ops
from multimodal_eeg_fmri_amd.ops import block_plan

POOL, NEXT = dict(pool_out=True), dict(next_norm=True, next_nq=384)


@pytest.mark.parametrize("D, M, n1, consumer, ln_fused, front, tail", [
    (128, 32, 512, POOL, True, "rows", "rows"),
    (128, 32, 512, NEXT, True, "rows", "rows"),
    (128, 64, 128, POOL, True, "rows", "rows"),
    (128, 32, 512, {}, True, "ln_gemm2_act", "generic"),            # a stand-alone TemporalTransformerBlock: no consumer
    (128, 32, 640, POOL, True, "ln_gemm2_act", "meanpool"),         # the hidden tile of a 640-wide FFN does not fit
    (128, 32, 640, NEXT, True, "ln_gemm2_act", "ln_gemm2"),
    (128, 32, 192, POOL, True, "ln", "meanpool"),                   # FFN width not a multiple of 128
    (128, 32, 192, NEXT, True, "ln", "ln_gemm2"),
    (128, 32, 192, {}, True, "ln", "generic"),
    (128, 48, 512, NEXT, False, "generic", "generic"),              # rows not in groups of 32
    (128, 48, 512, POOL, False, "generic", "meanpool"),
    (64, 32, 256, NEXT, False, "generic", "generic"),
    (256, 32, 1024, NEXT, False, "generic", "generic"),
    (256, 32, 512, POOL, False, "generic", "meanpool"),
])
def test_front_and_tail_forms(D, M, n1, consumer, ln_fused, front, tail):
    plan = block_plan(D, M, n1, **consumer)
    assert (plan.ln_fused, plan.front, plan.tail) == (ln_fused, front, tail)
    assert plan.out_proj_128 == (D in range(113, 129)) and plan.ffn_rows_width == (n1 % 128 == 0 and n1 <= 512)


def test_the_hidden_tensor_index_guard():
    """the first FFN Linear rides along only while M * n1 stays below 2**32"""
    assert block_plan(128, (1 << 23) - 32, 512, **POOL).front == "rows"
    assert block_plan(128, 1 << 23, 512, **POOL).front == "ln"


@pytest.mark.parametrize("n1", [512, 640, 192])                     # from the rows launch and from mm_linear_fwd_ln_gemm2 alike
def test_qkv_fusion(n1):
    assert block_plan(128, 32, n1, next_norm=True, next_nq=384).qkv_fused
    assert not block_plan(128, 32, n1, next_norm=True, next_nq=200).qkv_fused
    assert not block_plan(128, 32, n1, next_norm=True).qkv_fused                # no next block
    assert not block_plan(128, 32, n1, pool_out=True, next_nq=384).qkv_fused    # the rows go to the pool, not to a norm1
    assert not block_plan(128, 32, n1, pool_out=True, next_norm=True, next_nq=384).qkv_fused
    assert not block_plan(128, 48, n1, next_norm=True, next_nq=384).qkv_fused
    assert not block_plan(64, 32, n1, next_norm=True, next_nq=192).qkv_fused
    # M * nq at and just below 2**32 (plain ints: nothing is allocated); n1 = 192 keeps M * n1 out of the picture
    M = (1 << 32) // 384 // 32 * 32
    assert M * 384 < 1 << 32 <= (M + 32) * 384
    assert block_plan(128, M, 192, next_norm=True, next_nq=384).qkv_fused
    assert not block_plan(128, M + 32, 192, next_norm=True, next_nq=384).qkv_fused
    assert (1 << 25) * 128 == 1 << 32
    assert not block_plan(128, 1 << 25, 192, next_norm=True, next_nq=128).qkv_fused
    assert block_plan(128, (1 << 25) - 32, 192, next_norm=True, next_nq=128).qkv_fused
    assert block_plan(128, M, 192, next_norm=True, next_nq=384).tail == "ln_gemm2"
    assert block_plan(128, M + 32, 192, next_norm=True, next_nq=384).tail == "ln"


def test_each_forward_knob_alone(monkeypatch):
    base = block_plan(128, 32, 512, **NEXT)
    assert (base.front, base.tail, base.qkv_fused) == ("rows", "rows", True)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "_NO_FFN1_FUSE", True)
        for consumer, tail in ((NEXT, "ln_gemm2"), (POOL, "meanpool"), ({}, "generic")):
            plan = block_plan(128, 32, 512, **consumer)
            assert (plan.ln_fused, plan.front, plan.tail, plan.qkv_fused) == (True, "ln", tail, consumer is NEXT)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "_NO_FFN_ROWS", True)
        for consumer, tail in ((NEXT, "ln_gemm2"), (POOL, "meanpool"), ({}, "generic")):
            plan = block_plan(128, 32, 512, **consumer)
            assert (plan.ln_fused, plan.front, plan.tail, plan.qkv_fused) == (True, "ln_gemm2_act", tail, consumer is NEXT)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "_NO_QKV_FUSE", True)
        plan = block_plan(128, 32, 512, **NEXT)
        assert (plan.front, plan.tail, plan.qkv_fused) == ("rows", "rows", False)
        plan = block_plan(128, 32, 640, **NEXT)
        assert (plan.front, plan.tail, plan.qkv_fused) == ("ln_gemm2_act", "ln", False)
    assert block_plan(128, 32, 512, **NEXT) == base                 # the knobs are read at call time
    # the shape facts the backward reads do not depend on the forward's knobs
    with monkeypatch.context() as mp:
        mp.setattr(ops, "_NO_FFN1_FUSE", True)
        mp.setattr(ops, "_NO_FFN_ROWS", True)
        plan = block_plan(128, 32, 512, **NEXT)
        assert (plan.ln_fused, plan.out_proj_128, plan.ffn_rows_width) == (True, True, True)


# ------------------------------------------------------------------ backward
def _plan(ln_fused=True, out_proj_128=True, ffn_rows_width=True):
    """a plan built by hand: the backward reads these three fields only"""
    return ops.BlockPlan(ln_fused, "generic", "generic", False, out_proj_128, ffn_rows_width)


@pytest.mark.parametrize("plan, ffn, qkv, qkv_bn, head_rows", [
    (_plan(), "ffn_rows", "ln", "ln_bn_reduce", True),
    (_plan(ffn_rows_width=False), "ln_gemm2", "ln", "ln_bn_reduce", True),
    (_plan(out_proj_128=False), "ln", "ln", "ln_bn_reduce", False),
    (_plan(ln_fused=False), "generic", "generic", "generic", False),
    (_plan(ln_fused=False, out_proj_128=False, ffn_rows_width=False), "generic", "generic", "generic", False),
    (block_plan(128, 32, 512, **POOL), "ffn_rows", "ln", "ln_bn_reduce", True),
    (block_plan(128, 32, 512), "ffn_rows", "ln", "ln_bn_reduce", True),          # the backward needs no consumer
    (block_plan(128, 32, 640, **NEXT), "ln_gemm2", "ln", "ln_bn_reduce", True),
    (block_plan(128, 32, 192, **NEXT), "ln_gemm2", "ln", "ln_bn_reduce", True),
    (block_plan(128, 48, 512, **NEXT), "generic", "generic", "generic", False),
    (block_plan(64, 32, 256, **NEXT), "generic", "generic", "generic", False),
    (block_plan(256, 32, 512, **NEXT), "generic", "generic", "generic", False),
])
def test_backward_forms(plan, ffn, qkv, qkv_bn, head_rows):
    assert autograd.block_bwd_plan(plan) == autograd.BlockBwdPlan(ffn, qkv, head_rows)
    assert autograd.block_bwd_plan(plan, bn_below=True) == autograd.BlockBwdPlan(ffn, qkv_bn, head_rows)


def test_each_backward_knob_alone(monkeypatch):
    full, wide = _plan(), _plan(ffn_rows_width=False)
    with monkeypatch.context() as mp:
        mp.setattr(autograd, "_NO_GEMM2", True)                     # no second GEMM: nothing reads the head's row form either
        assert autograd.block_bwd_plan(full, True) == autograd.BlockBwdPlan("ln", "ln_bn_reduce", False)
        assert autograd.block_bwd_plan(wide) == autograd.BlockBwdPlan("ln", "ln", False)
    with monkeypatch.context() as mp:
        mp.setattr(autograd, "_NO_FFN_ROWS_BWD", True)
        assert autograd.block_bwd_plan(full, True) == autograd.BlockBwdPlan("ln_gemm2", "ln_bn_reduce", True)
        assert autograd.block_bwd_plan(wide) == autograd.BlockBwdPlan("ln_gemm2", "ln", True)
    with monkeypatch.context() as mp:
        mp.setattr(autograd, "_NO_BNRED", True)
        assert autograd.block_bwd_plan(full, True) == autograd.BlockBwdPlan("ffn_rows", "ln", True)
    with monkeypatch.context() as mp:
        mp.setattr(autograd, "_NO_BCAST", True)                     # the voxel head's knob: not a block's business
        assert autograd.block_bwd_plan(full, True) == autograd.BlockBwdPlan("ffn_rows", "ln_bn_reduce", True)
    assert autograd.block_bwd_plan(full, True) == autograd.BlockBwdPlan("ffn_rows", "ln_bn_reduce", True)


def test_ffn_rows_bwd_fused_agrees_with_the_backward_form(monkeypatch):
    plans = [_plan(), _plan(ffn_rows_width=False), _plan(out_proj_128=False), _plan(ln_fused=False),
             block_plan(128, 32, 512, **NEXT), block_plan(128, 32, 640, **NEXT), block_plan(128, 48, 512, **POOL)]

    def check():
        took = [autograd.block_bwd_plan(p).ffn == "ffn_rows" for p in plans]
        for p, t in zip(plans, took):
            assert autograd.ffn_rows_bwd_fused([dict(plan=p)]) == t
        for a, ta in zip(plans, took):
            for b, tb in zip(plans, took):
                assert autograd.ffn_rows_bwd_fused([dict(plan=a), dict(plan=b)]) == (ta and tb)
        return took
    assert check() == [True, False, False, False, True, False, False]
    assert autograd.ffn_rows_bwd_fused([]) is False and autograd.ffn_rows_bwd_fused(None) is False
    for knob in ("_NO_GEMM2", "_NO_FFN_ROWS_BWD"):
        with monkeypatch.context() as mp:
            mp.setattr(autograd, knob, True)
            assert not any(check())
    with monkeypatch.context() as mp:
        mp.setattr(autograd, "_NO_BNRED", True)
        assert check() == [True, False, False, False, True, False, False]
