"""The transformer blocks launch what they launched before their launch plan was factored out (ops.BlockPlan): for every
path a block can take - the one-launch rows form, the forms it falls back to by FFN width and by row count, a stand-alone
block, an eval forward that saves nothing - one forward + backward issues the same entry points in the same order with the
same dropout seeds as the commit before the refactor did.  EXPECTED was recorded from that commit with run_case() below;
outputs and gradients must be finite as well, since names alone would pass on garbage."""
import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
import multimodal_eeg_fmri_amd.enhanced_models_v4 as E

SEED = 20240917
# host-only entry points (slot counts, split-K plans, workspace sizes): they launch nothing and _hip caches most of them per
# process, so whether one is called depends on what ran earlier - they are not part of the launch sequence
HOST_ONLY = ("_slots", "_plan", "_ws_floats")

EXPECTED = {'block_F192': [('mm_layernorm_fwd', ()), ('mm_prep_conv_weight', ()), ('mm_conv1d_fwd', ()), ('mm_attn_fwd', (2703381436,)),
                ('mm_prep_conv_weight', ()), ('mm_prep_conv_weight', ()), ('mm_linear_fwd_ln', (2703421939,)), ('mm_conv1d_fwd', (2703462442,)),
                ('mm_prep_conv_weight', ()), ('mm_conv1d_fwd', (2703502945,)), ('mm_act_bwd', (2703502945,)), ('mm_conv1d_fwd', (2703462442,)),
                ('mm_linear_dgrad_ln_bwd_gemm2', (2703421939,)), ('mm_attn_bwd', (2703381436,)), ('mm_linear_dgrad_ln_bwd', ()),
                ('mm_conv1d_wgrad_many', ()), ('mm_flush_many', ())],
 'block_F512': [('mm_layernorm_fwd', ()), ('mm_prep_conv_weight', ()), ('mm_conv1d_fwd', ()), ('mm_attn_fwd', (2703381436,)),
                ('mm_prep_conv_weight', ()), ('mm_prep_conv_weight', ()), ('mm_prep_conv_weight', ()),
                ('mm_linear_fwd_ln_gemm2_act', (2703421939, 2703462442)), ('mm_conv1d_fwd', (2703502945,)), ('mm_act_bwd', (2703502945,)),
                ('mm_ffn_rows_bwd', (2703462442, 2703421939)), ('mm_attn_bwd', (2703381436,)), ('mm_linear_dgrad_ln_bwd', ()),
                ('mm_conv1d_wgrad_many', ()), ('mm_flush_many', ())],
 'block_F640': [('mm_layernorm_fwd', ()), ('mm_prep_conv_weight', ()), ('mm_conv1d_fwd', ()), ('mm_attn_fwd', (2703381436,)),
                ('mm_prep_conv_weight', ()), ('mm_prep_conv_weight', ()), ('mm_prep_conv_weight', ()),
                ('mm_linear_fwd_ln_gemm2_act', (2703421939, 2703462442)), ('mm_conv1d_fwd', (2703502945,)), ('mm_act_bwd', (2703502945,)),
                ('mm_conv1d_fwd', (2703462442,)), ('mm_linear_dgrad_ln_bwd_gemm2', (2703421939,)), ('mm_attn_bwd', (2703381436,)),
                ('mm_linear_dgrad_ln_bwd', ()), ('mm_conv1d_wgrad_many', ()), ('mm_flush_many', ())],
 'encoder_M32': [('mm_pack_nct_bf16', ()), ('mm_prep_conv_weight', ()), ('mm_conv1d_fwd', ()), ('mm_bn_act_fwd_fin', (2703381436,)),
                 ('mm_prep_conv_weight', ()), ('mm_conv1d_fwd', ()), ('mm_bn_act_fwd_fin', (2703421939,)), ('mm_prep_conv_weight', ()),
                 ('mm_conv1d_fwd', ()), ('mm_bn_act_fwd_ln_fin', (2703462442, 2703502945)), ('mm_prep_conv_weight', ()), ('mm_conv1d_fwd', ()),
                 ('mm_attn_fwd', (2703543448,)), ('mm_prep_conv_weight', ()), ('mm_prep_conv_weight', ()), ('mm_prep_conv_weight', ()),
                 ('mm_prep_conv_weight', ()), ('mm_ffn_rows_fwd', (2703583951, 2703624454, 2703664957)), ('mm_attn_fwd', (2703705460,)),
                 ('mm_prep_conv_weight', ()), ('mm_prep_conv_weight', ()), ('mm_prep_conv_weight', ()),
                 ('mm_ffn_rows_fwd', (2703745963, 2703786466, 2703826969)), ('mm_pooled_head_fwd', (2703867472,)),
                 ('mm_pooled_head_bwd_rows', (2703867472, 2703826969)), ('mm_ffn_rows_bwd', (2703786466, 2703745963)), ('mm_attn_bwd', (2703705460,)),
                 ('mm_linear_dgrad_ln_bwd', (2703664957,)), ('mm_ffn_rows_bwd', (2703624454, 2703583951)), ('mm_attn_bwd', (2703543448,)),
                 ('mm_linear_dgrad_ln_bwd_bn_reduce', (2703462442, 2703502945)), ('mm_bn_act_bwd_apply', (2703462442, 2703502945)),
                 ('mm_conv1d_wgrad', ()), ('mm_conv1d_dgrad_bn_reduce', (2703421939,)), ('mm_bn_act_bwd_apply', (2703421939,)),
                 ('mm_conv1d_wgrad', ()), ('mm_conv1d_dgrad_bn_reduce', (2703381436,)), ('mm_bn_act_bwd_apply', (2703381436,)),
                 ('mm_conv1d_wgrad', ()), ('mm_conv1d_wgrad_many', ()), ('mm_flush_many', ())],
 'encoder_M32_eval': [('mm_pack_nct_bf16', ()), ('mm_prep_conv_weight', ()), ('mm_bn_finalize', ()), ('mm_conv1d_fwd', ()),
                      ('mm_prep_conv_weight', ()), ('mm_bn_finalize', ()), ('mm_conv1d_fwd', ()), ('mm_prep_conv_weight', ()), ('mm_bn_finalize', ()),
                      ('mm_conv1d_fwd', ()), ('mm_layernorm_fwd', ()), ('mm_prep_conv_weight', ()), ('mm_conv1d_fwd', ()), ('mm_attn_fwd', ()),
                      ('mm_prep_conv_weight', ()), ('mm_prep_conv_weight', ()), ('mm_prep_conv_weight', ()), ('mm_prep_conv_weight', ()),
                      ('mm_ffn_rows_fwd', ()), ('mm_attn_fwd', ()), ('mm_prep_conv_weight', ()), ('mm_prep_conv_weight', ()),
                      ('mm_prep_conv_weight', ()), ('mm_ffn_rows_fwd', ()), ('mm_pooled_head_fwd', ())],
 'encoder_M48': [('mm_pack_nct_bf16', ()), ('mm_prep_conv_weight', ()), ('mm_conv1d_fwd', ()), ('mm_bn_act_fwd_fin', (2703381436,)),
                 ('mm_prep_conv_weight', ()), ('mm_conv1d_fwd', ()), ('mm_bn_act_fwd_fin', (2703421939,)), ('mm_prep_conv_weight', ()),
                 ('mm_conv1d_fwd', ()), ('mm_bn_act_fwd_ln_fin', (2703462442, 2703502945)), ('mm_prep_conv_weight', ()), ('mm_conv1d_fwd', ()),
                 ('mm_attn_fwd', (2703543448,)), ('mm_prep_conv_weight', ()), ('mm_conv1d_fwd', (2703583951,)), ('mm_layernorm_fwd', ()),
                 ('mm_prep_conv_weight', ()), ('mm_conv1d_fwd', (2703624454,)), ('mm_prep_conv_weight', ()), ('mm_conv1d_fwd', (2703664957,)),
                 ('mm_layernorm_fwd', ()), ('mm_prep_conv_weight', ()), ('mm_conv1d_fwd', ()), ('mm_attn_fwd', (2703705460,)),
                 ('mm_prep_conv_weight', ()), ('mm_conv1d_fwd', (2703745963,)), ('mm_layernorm_fwd', ()), ('mm_prep_conv_weight', ()),
                 ('mm_conv1d_fwd', (2703786466,)), ('mm_prep_conv_weight', ()), ('mm_conv1d_fwd', (2703826969,)), ('mm_meanpool_fwd', ()),
                 ('mm_pooled_head_fwd', (2703867472,)), ('mm_pooled_head_bwd_rows', (2703867472, 2703826969)), ('mm_conv1d_fwd', (2703786466,)),
                 ('mm_conv1d_fwd', ()), ('mm_layernorm_bwd', (2703745963,)), ('mm_conv1d_fwd', ()), ('mm_attn_bwd', (2703705460,)),
                 ('mm_conv1d_fwd', ()), ('mm_layernorm_bwd', (2703664957,)), ('mm_conv1d_fwd', (2703624454,)), ('mm_conv1d_fwd', ()),
                 ('mm_layernorm_bwd', (2703583951,)), ('mm_conv1d_fwd', ()), ('mm_attn_bwd', (2703543448,)), ('mm_conv1d_fwd', ()),
                 ('mm_layernorm_bwd', ()), ('mm_bn_act_bwd_reduce', (2703462442, 2703502945)), ('mm_bn_act_bwd_apply', (2703462442, 2703502945)),
                 ('mm_conv1d_wgrad', ()), ('mm_conv1d_dgrad_bn_reduce', (2703421939,)), ('mm_bn_act_bwd_apply', (2703421939,)),
                 ('mm_conv1d_wgrad', ()), ('mm_conv1d_dgrad_bn_reduce', (2703381436,)), ('mm_bn_act_bwd_apply', (2703381436,)),
                 ('mm_conv1d_wgrad', ()), ('mm_conv1d_wgrad_many', ()), ('mm_flush_many', ())]}


def _encoder(T, train=True):
    def make():
        m = E.EnhancedERPEncoder(8, 128, 2, 4, dropout=0.2).cuda()
        return (m.train() if train else m.eval()), torch.randn(1, 8, T, device="cuda")
    return make


def _block(F):
    def make():
        m = E.TemporalTransformerBlock(128, 4, dim_feedforward=F).cuda().train()
        return m, torch.randn(1, 32, 128, device="cuda", requires_grad=True)
    return make


CASES = {
    "encoder_M32": _encoder(64),            # M = 32: the smallest shape on the fully fused path
    "encoder_M48": _encoder(96),            # M = 48: the smallest that falls off it
    "block_F512": _block(512),
    "block_F640": _block(640),
    "block_F192": _block(192),
    "encoder_M32_eval": _encoder(64, train=False),
}


def run_case(name, monkeypatch):
    """-> ([(entry point, (its dropout-seed arguments, in order))], every output and gradient finite)"""
    torch.manual_seed(0)
    m, x = CASES[name]()
    calls, drawn = [], set()
    real_call, real_seed = _hip.call, ops._next_seed
    state = dict(ops._seed_state)
    ops.set_dropout_seed(SEED)
    monkeypatch.setattr(_hip, "call", lambda entry, *a: (calls.append((entry, a)), real_call(entry, *a))[1])
    monkeypatch.setattr(ops, "_next_seed", lambda: (lambda s: (drawn.add(s), s)[1])(real_seed()))
    try:
        if m.training:
            out = m(x)
            out.square().sum().backward()
            results = [out] + [p.grad for p in m.parameters()] + ([x.grad] if x.requires_grad else [])
        else:
            with torch.no_grad():
                results = [m(x)]
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(_hip, "call", real_call)
        monkeypatch.setattr(ops, "_next_seed", real_seed)
        ops._seed_state.update(state)
    finite = all(t is not None and bool(torch.isfinite(t).all()) for t in results)
    return [(entry, tuple(v for v in a if type(v) is int and v in drawn)) for entry, a in calls
            if not entry.endswith(HOST_ONLY)], finite


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_a_step_launches_what_it_launched_before_the_plan(name, monkeypatch):
    got, finite = run_case(name, monkeypatch)
    assert finite, name
    assert [e for e, _ in got] == [e for e, _ in EXPECTED[name]], name
    assert got == EXPECTED[name], name
