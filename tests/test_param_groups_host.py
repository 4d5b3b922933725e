"""Parameter groups of the fused AdamW step, host side (CPU): `ref_adamw_groups`, the fp64 restatement of per-segment AdamW
with one global-norm clip that the GPU tests compare with (checked here against torch.optim.AdamW with real parameter
groups + clip_grad_norm_ in fp64, and against `ref_adamw` for one segment); `optim.segment_table`; the component layout,
``no_decay`` and ``freeze`` of a `BridgeTrainer` built on the CPU; the refusals; `FusedAdamW` groups <-> torch.optim.AdamW
state dicts; the header's declarations."""
import math

import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, optim
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer
from multimodal_eeg_fmri_amd.fmri_utils import fMRITabularEncoder
from multimodal_eeg_fmri_amd.optim import FusedAdamW, segment_table
from test_clip_loss_refs_host import ref_adamw


def ref_adamw_groups(p, g, m, v, step, lr, beta1, beta2, eps, max_norm, grad_scale, seg_end, seg_lr_mult, seg_wd):
    """one step of mm_adamw_clip_groups in fp64, `step` = the count BEFORE it -> (p, m, v, sumsq, clip, norm).  The norm and
    the clip coefficient are the WHOLE bucket's; segment s = [seg_end[s-1], seg_end[s]) is updated with the learning rate
    fl32(lr * seg_lr_mult[s]) (the one rounding the kernel makes: lr and the multiplier are fp32 values) and the weight
    decay seg_wd[s]:  p <- p (1 - lr_s wd_s);  m <- b1 m + (1 - b1) g';  v <- b2 v + (1 - b2) g'^2;
    p <- p - lr_s / (1 - b1^t) m / (sqrt(v) / sqrt(1 - b2^t) + eps),  g' = g grad_scale clip,  t = step + 1."""
    p, g, m, v = (x.double().clone() for x in (p, g, m, v))
    sumsq = (g * g).sum().item()
    norm = math.sqrt(sumsq) * grad_scale
    clip = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    gs = g * (grad_scale * clip)
    t = step + 1
    m = beta1 * m + (1.0 - beta1) * gs
    v = beta2 * v + (1.0 - beta2) * gs * gs
    lo = 0
    for end, mult, wd in zip(seg_end, seg_lr_mult, seg_wd):
        lr_s = (torch.tensor(lr, dtype=torch.float32) * torch.tensor(mult, dtype=torch.float32)).item()
        sl = slice(lo, end)
        p[sl] = p[sl] * (1.0 - lr_s * wd)
        p[sl] = p[sl] - lr_s / (1.0 - beta1 ** t) * m[sl] / (v[sl].sqrt() / math.sqrt(1.0 - beta2 ** t) + eps)
        lo = end
    assert lo == p.numel()
    return p, m, v, sumsq, clip, norm


def test_reference_is_torch_adamw_with_param_groups_and_clip_grad_norm():
    """three groups (lr x 1 / wd 0.02, lr x 0.1 / wd 0, lr x 0 / wd 0.3) of two, one and two parameters, 3 steps in fp64,
    clipping active: to 1e-12 (multipliers and rates are fp32 values on both sides, as the kernel sees them)"""
    f32 = lambda x: torch.tensor(float(x), dtype=torch.float32).item()
    gen = torch.Generator().manual_seed(5)
    shapes = [(7,), (3, 5), (11,), (2, 2), (1,)]
    group_of = [0, 0, 1, 2, 2]
    mults, wds = [1.0, f32(0.1), 0.0], [f32(0.02), 0.0, f32(0.3)]
    lr, b1, b2, eps = f32(3e-3), f32(0.9), f32(0.98), f32(1e-8)
    init = [torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes]
    params = [torch.nn.Parameter(x.clone()) for x in init]
    groups = [{"params": [q for q, k in zip(params, group_of) if k == gi], "lr": f32(f32(lr) * mults[gi]),
               "weight_decay": wds[gi]} for gi in range(3)]
    topt = torch.optim.AdamW(groups, lr=lr, betas=(b1, b2), eps=eps)
    ends, seg_m, seg_w = segment_table([(q.numel(), mults[k], wds[k]) for q, k in zip(params, group_of)])
    assert ends == [22, 33, 38] and seg_m == mults and seg_w == wds
    flat = lambda xs: torch.cat([x.detach().reshape(-1) for x in xs])
    p, m, v = flat(init), torch.zeros(38, dtype=torch.float64), torch.zeros(38, dtype=torch.float64)
    for step in range(3):
        gr = [torch.randn(s, generator=gen, dtype=torch.float64) * (1 + step) for s in shapes]
        for q, x in zip(params, gr):
            q.grad = x.clone()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        topt.step()
        p, m, v, sumsq, clip, norm = ref_adamw_groups(p, flat(gr), m, v, step, lr, b1, b2, eps, 1.0, 1.0, ends, seg_m, seg_w)
        assert clip < 1.0
        assert (p - flat(params)).abs().max().item() <= 1e-12
    assert torch.equal(p[33:], flat(init)[33:])                               # the lr x 0 group never moved
    assert (m[33:] != 0).all() and (v[33:] != 0).all()                        # ... its moments did


def test_one_segment_of_multiplier_one_is_ref_adamw():
    gen = torch.Generator().manual_seed(6)
    n = 37
    p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    m, v = torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) * 0.01
    lr = torch.tensor(3e-3, dtype=torch.float32).item()                       # (an fp32 value, as the kernel's state[2] is)
    a = ref_adamw(p, g, m, v, 4, lr, 0.9, 0.999, 1e-8, 0.02, 1.0, 0.5)
    b = ref_adamw_groups(p, g, m, v, 4, lr, 0.9, 0.999, 1e-8, 1.0, 0.5, [n], [1.0], [0.02])
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
    assert a[3:] == b[3:]


# ---------------------------------------------------------------------------------------------------------------------------
def test_segment_table_merges_equal_neighbours_and_keeps_the_ends():
    ends, mults, wds = segment_table([(3, 1.0, 0.01), (5, 1.0, 0.01), (0, 7.0, 0.5), (2, 0.1, 0.01), (4, 0.1, 0.0),
                                      (1, 0.1, 0.0), (6, 1.0, 0.01)])
    assert ends == [8, 10, 15, 21] and mults == [1.0, 0.1, 0.1, 1.0] and wds == [0.01, 0.01, 0.0, 0.01]
    # a tag keeps equal values apart; the tags of the segments come back on request
    ends, mults, wds, tags = segment_table([(3, 1.0, 0.0, "a"), (5, 1.0, 0.0, "a"), (2, 1.0, 0.0, "b")], tags=True)
    assert ends == [8, 10] and tags == ["a", "b"]
    assert segment_table([(4, 1, 0)]) == ([4], [1.0], [0.0])


def test_segment_table_cap():
    alternating = [(1 + i % 3, float(i % 2), 0.0) for i in range(optim.MAX_SEGMENTS)]
    ends, mults, _ = segment_table(alternating)
    assert optim.MAX_SEGMENTS == 1024 and len(ends) == 1024 and ends[-1] == sum(k for k, _, _ in alternating)
    assert all(a < b for a, b in zip(ends, ends[1:]))
    with pytest.raises(ValueError, match="1025 segments"):
        segment_table(alternating + [(1, 0.0, 0.0)])
    segment_table(alternating + [(1, 1.0, 0.0)])                              # merges with the last one: still 1024


@pytest.mark.parametrize("bad", [-0.5, float("nan"), float("inf"), -float("inf"), "fast", None])
def test_segment_table_rejects_a_bad_multiplier(bad):
    with pytest.raises(ValueError, match="lr_scale"):
        segment_table([(3, 1.0, 0.0), (2, bad, 0.0)])
    with pytest.raises(ValueError, match="lr_scale"):
        FusedAdamW([{"params": [torch.nn.Parameter(torch.zeros(3))], "lr_scale": bad}])


def test_segment_table_rejects_a_bad_decay_and_an_empty_bucket():
    for wd in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="weight_decay"):
            segment_table([(3, 1.0, wd)])
    with pytest.raises(ValueError, match="no elements"):
        segment_table([(0, 1.0, 0.0)])


def test_header_declares_the_entry_points_and_keeps_the_abi_version():
    sigs = _hip.parse_header()
    plain = sigs["mm_adamw_clip"]
    assert plain == "ppppp" + "l" + "ffffff" + "i" + "p"                       # its argument list is unchanged
    assert sigs["mm_adamw_clip_groups"] == "ppppp" + "l" + "fffff" + "i" + "p" + "ppp" + "i"
    assert sigs["mm_adamw_clip_groups_ema"] == sigs["mm_adamw_clip_groups"] + "pfi"
    assert _hip.header_abi_version() == 5                                      # entry points were only added
    assert "#define MM_OPT_MAX_SEGMENTS 1024\n" in open(_hip.header_path()).read()


# ---------------------------------------------------------------------------------------------------------------------------
def _trainer(**kw):
    torch.manual_seed(0)
    kw.setdefault("eeg_channels", 8)
    return BridgeTrainer(dropout=0.0, device="cpu", **kw)


def _component_ranges(tr):
    """{component: [(lo, hi), ...]} over the flat bucket, from the parameters themselves"""
    ids = {"eeg_encoder": {id(p) for p in tr.eeg_encoder.parameters()},
           "fmri_encoder": {id(p) for p in tr.fmri_encoder.parameters()}}
    out, off = {}, 0
    for p in tr.bucket.params:
        name = next((c for c, s in ids.items() if id(p) in s), "head")
        out.setdefault(name, []).append((off, off + p.numel()))
        off += p.numel()
    return out, off


@pytest.mark.parametrize("loss", ["infonce", "sigmoid"])
def test_components_tile_the_bucket(loss):
    tr = _trainer(loss=loss, lr_scale={"eeg_encoder": 0.1, "fmri_encoder": 0.0, "head": 2.0})
    ranges, n = _component_ranges(tr)
    assert n == tr.bucket.n and set(ranges) == set(BridgeTrainer.COMPONENTS)
    t = tr._table
    assert t.ends[-1] == tr.bucket.n and all(a < b for a, b in zip(t.ends, t.ends[1:]))
    assert len(tr._seg_component) == t.n_seg
    want = {"eeg_encoder": 0.1, "fmri_encoder": 0.0, "head": 2.0}
    assert tr.lr_scales == want
    lo = 0
    for end, mult, wd, c in zip(t.ends, t.mults, t.wds, tr._seg_component):   # every segment lies inside ONE component
        assert _covered(ranges[c], lo, end), (c, lo, end)
        assert mult == want[c] and wd == tr.weight_decay
        lo = end
    covered = sum(hi - lo for rs in ranges.values() for lo, hi in rs)
    assert covered == tr.bucket.n
    head_ids = {id(tr.head.logit_scale)} | ({id(tr.head.logit_bias)} if loss == "sigmoid" else set())
    head_params = [p for p, c in zip(tr.bucket.params, tr._param_component) if c == "head"]
    assert head_ids <= {id(p) for p in head_params}
    assert tr._grouped and not t.uniform


def _covered(ranges, lo, hi):
    """[lo, hi) is a union of the parameter ranges `ranges` (they are contiguous pieces of one component)"""
    inside = sorted((a, b) for a, b in ranges if lo <= a and b <= hi)
    pos = lo
    for a, b in inside:
        if a != pos:
            return False
        pos = b
    return pos == hi


def test_default_trainer_has_a_uniform_table_and_the_plain_kernel():
    tr = _trainer()
    assert not tr._grouped and tr._table.uniform and tr.lr_scales == {c: 1.0 for c in BridgeTrainer.COMPONENTS}
    assert tr.checkpoint_param_groups() is None and "param_groups" not in tr.checkpoint_state()["bridge_trainer_state"]
    same = _trainer(lr_scale={"eeg_encoder": 1.0, "head": 1})
    assert not same._grouped and same.checkpoint_param_groups() is None
    assert same.bucket.n == tr.bucket.n and same.groups == tr.groups


def test_no_decay_marks_exactly_the_vectors_and_scalars():
    tr = _trainer(no_decay=True, weight_decay=0.05)
    t = tr._table
    per_elem = torch.empty(tr.bucket.n)
    lo = 0
    for end, wd in zip(t.ends, t.wds):
        per_elem[lo:end] = wd
        lo = end
    off, seen = 0, {0: 0, 1: 0}
    for p in tr.bucket.params:
        want = 0.0 if p.ndim <= 1 else 0.05
        assert bool((per_elem[off:off + p.numel()] == torch.tensor(want)).all()), (tuple(p.shape), want)
        seen[int(p.ndim > 1)] += 1
        off += p.numel()
    assert seen[0] > 0 and seen[1] > 0 and tr.head.logit_scale.ndim == 0
    assert tr._grouped and set(t.mults) == {1.0}
    assert not _trainer(no_decay=True, weight_decay=0.0)._grouped             # one decay after all: the plain kernel


@pytest.mark.parametrize("freeze", [("fmri_encoder",), ("eeg_encoder",), ("eeg_encoder", "fmri_encoder"), "fmri_encoder"])
def test_freeze_takes_the_component_out_of_the_bucket(freeze):
    base = _trainer()
    tr = _trainer(freeze=freeze)
    names = (freeze,) if isinstance(freeze, str) else freeze
    gone = sum(p.numel() for c in names for p in getattr(tr, c).parameters())
    assert gone > 0 and tr.bucket.n == base.bucket.n - gone
    for c in BridgeTrainer.COMPONENTS[:2]:
        enc = getattr(tr, c)
        assert all(p.requires_grad == (c not in names) for p in enc.parameters())
    bucket_ids = {id(p) for p in tr.bucket.params}
    assert not any(id(p) in bucket_ids for c in names for p in getattr(tr, c).parameters())
    tr.train()                                                                 # a frozen encoder stays in eval form
    for c in BridgeTrainer.COMPONENTS[:2]:
        assert getattr(tr, c).training == (c not in names)
    assert tr.head.training
    # the layer groups still tile the bucket, and the heads sit in a group whose ready point fires
    assert tr.groups[0][2] == 0 and tr.groups[-1][3] == tr.bucket.n
    assert all(a[3] == b[2] for a, b in zip(tr.groups, tr.groups[1:]))
    if "eeg_encoder" in names:
        assert [(n, r) for n, r, _, _ in tr.groups][0] == ("heads", "main")
    assert len(tr.optimizer_param_map()) == len(tr.bucket.params)
    pg = tr.checkpoint_state()["bridge_trainer_state"]["param_groups"]
    assert pg["freeze"] == [c for c in BridgeTrainer.COMPONENTS if c in names] and pg["no_decay"] is False
    assert pg["seg_end"][-1] == tr.bucket.n and not tr._grouped


def test_freeze_with_the_tabular_encoder():
    torch.manual_seed(0)
    enc = fMRITabularEncoder(activation_dim=12, connectivity_dim=20, hidden_dim=64, dropout=0.0)
    tr = _trainer(fmri_encoder=enc, freeze=("fmri_encoder",))
    assert all(not p.requires_grad for p in enc.parameters()) and not tr.train().fmri_encoder.training
    assert tr.groups[-1][2] == tr.groups[-1][3] == tr.bucket.n


def test_refusals():
    with pytest.raises(ValueError, match="component 'decoder'"):
        _trainer(lr_scale={"decoder": 0.1})
    with pytest.raises(ValueError, match="component 'bridge'"):
        _trainer(freeze=("bridge",))
    with pytest.raises(ValueError, match="freeze=\\('head',\\)"):
        _trainer(freeze=("head",))
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lr_scale"):
            _trainer(lr_scale={"head": bad})
    tr = _trainer()
    with pytest.raises(ValueError, match="component"):
        tr.set_lr_scale("decoder", 1.0)
    with pytest.raises(ValueError, match="lr_scale"):
        tr.set_lr_scale("head", -2.0)
    assert tr.lr_scales["head"] == 1.0


def test_freeze_at_world_size_two_is_refused_before_anything_is_built(monkeypatch):
    from multimodal_eeg_fmri_amd import dp
    monkeypatch.setattr(dp, "world_size", lambda group: 2)
    with pytest.raises(NotImplementedError, match="freeze="):
        BridgeTrainer(eeg_channels=8, device="cpu", group=object(), freeze=("fmri_encoder",))


def test_set_lr_scale_rewrites_the_table_in_place():
    tr = _trainer(lr_scale={"eeg_encoder": 0.5})
    ptrs = (tr._table.end.data_ptr(), tr._table.mult.data_ptr(), tr._table.wd.data_ptr())
    ends = list(tr._table.ends)
    tr.set_lr_scale("fmri_encoder", 0.0)
    tr.set_lr_scale("eeg_encoder", 0.25)
    assert (tr._table.end.data_ptr(), tr._table.mult.data_ptr(), tr._table.wd.data_ptr()) == ptrs and tr._table.ends == ends
    want = [{"eeg_encoder": 0.25, "fmri_encoder": 0.0, "head": 1.0}[c] for c in tr._seg_component]
    assert tr._table.mult.tolist() == want == tr._table.mults
    tr.set_lr(5e-4)                                                            # the base rate: the ratios stay
    assert tr.lr_scales == {"eeg_encoder": 0.25, "fmri_encoder": 0.0, "head": 1.0}
    plain = _trainer()
    plain.set_lr_scale("head", 1.0)
    assert not plain._grouped
    plain.set_lr_scale("head", 3.0)
    assert plain._grouped                                                      # switched once, for good
    plain.set_lr_scale("head", 1.0)
    assert plain._grouped


def test_checkpoint_carries_the_groups_and_refuses_another_freeze_or_no_decay():
    a = _trainer(lr_scale={"eeg_encoder": 0.1}, no_decay=True)
    ck = a.checkpoint_state()
    pg = ck["bridge_trainer_state"]["param_groups"]
    assert pg["components"] == list(BridgeTrainer.COMPONENTS) and pg["multipliers"] == [0.1, 1.0, 1.0]
    assert pg["no_decay"] is True and pg["freeze"] == [] and pg["seg_end"] == a._table.ends and pg["seg_wd"] == a._table.wds
    b = _trainer(no_decay=True)
    b.load_checkpoint_state(ck)
    assert b.lr_scales == a.lr_scales and b._table.mults == a._table.mults and b._table.wds == a._table.wds and b._grouped
    for other in (_trainer(), _trainer(no_decay=True, freeze=("fmri_encoder",)), _trainer(freeze=("eeg_encoder",))):
        before = (other.bucket.p.clone(), dict(other.lr_scales), list(other._table.mults))
        with pytest.raises(ValueError, match="no_decay differs|freeze differs"):
            other.load_checkpoint_state(ck)
        assert torch.equal(other.bucket.p, before[0]) and other.lr_scales == before[1] and other._table.mults == before[2]
    # a default checkpoint into a trainer whose multipliers were changed: they come back to 1
    c = _trainer(lr_scale={"head": 4.0})
    c.load_checkpoint_state(_trainer().checkpoint_state())
    assert c.lr_scales == {k: 1.0 for k in BridgeTrainer.COMPONENTS} and c._table.uniform


# ---------------------------------------------------------------------------------------------------------------------------
def _group_params():
    gen = torch.Generator().manual_seed(3)
    a = [torch.nn.Parameter(torch.randn(4, 3, generator=gen)), torch.nn.Parameter(torch.randn(3, generator=gen))]
    b = [torch.nn.Parameter(torch.randn(5, generator=gen))]
    c = [torch.nn.Parameter(torch.randn(2, 2, generator=gen)), torch.nn.Parameter(torch.randn(6, generator=gen), requires_grad=False)]
    return a, b, c


def test_fused_adamw_groups_layout_and_table():
    a, b, c = _group_params()
    opt = FusedAdamW([{"params": a}, {"params": b, "lr_scale": 0.1, "weight_decay": 0.0}, {"params": c, "lr_scale": 0.1,
                                                                                          "weight_decay": 0.0}],
                     lr=2e-3, weight_decay=0.05)
    assert [g["lr"] for g in opt.param_groups] == [2e-3] * 3
    assert [g["lr_scale"] for g in opt.param_groups] == [1.0, 0.1, 0.1]
    assert [g["weight_decay"] for g in opt.param_groups] == [0.05, 0.0, 0.0] and opt.weight_decay == 0.05
    assert opt.bucket.n == 15 + 5 + 4 and [id(p) for p in opt.bucket.params] == [id(p) for p in a + b + c[:1]]
    assert opt._host_table() == ([15, 24], [1.0, 0.1], [0.05, 0.0])          # groups 2 and 3 merge
    opt.param_groups[1]["lr"] = 1e-3
    with pytest.raises(ValueError, match="shared base learning rate"):
        opt.step()
    with pytest.raises(ValueError, match="more than one parameter group"):
        FusedAdamW([{"params": a}, {"params": a[:1]}])
    with pytest.raises(ValueError, match="betas"):
        FusedAdamW([{"params": a, "betas": (0.5, 0.9)}])
    plain = FusedAdamW(a)                                                     # a plain list behaves as before
    assert len(plain.param_groups) == 1 and plain._host_table() == ([15], [1.0], [0.01])
    assert "lr_scale" not in plain.state_dict()["param_groups"][0]


def test_fused_adamw_groups_state_dict_moves_both_ways_with_torch():
    a, b, c = _group_params()
    spec = [{"params": a}, {"params": b, "lr_scale": 0.1, "weight_decay": 0.0}, {"params": c, "lr_scale": 0.0}]
    fused = FusedAdamW(spec, lr=3e-4, betas=(0.8, 0.95), weight_decay=0.05)
    n = fused.bucket.n
    fused.bucket.m.copy_(torch.arange(float(n)))
    fused.bucket.v.copy_(torch.arange(float(n)) * 2)
    fused.bucket.state[0] = 7.0
    sd = fused.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == [[0, 1], [2], [3, 4]]
    assert [g["lr_scale"] for g in sd["param_groups"]] == [1.0, 0.1, 0.0] and 4 not in sd["state"]
    ref = torch.optim.AdamW([{"params": a}, {"params": b}, {"params": c}], lr=1.0)
    ref.load_state_dict(sd)
    assert [g["weight_decay"] for g in ref.param_groups] == [0.05, 0.0, 0.05] and ref.param_groups[1]["lr"] == 3e-4
    assert torch.equal(ref.state[b[0]]["exp_avg"], torch.arange(15.0, 20.0)) and float(ref.state[a[0]]["step"]) == 7.0
    ref.param_groups[2]["weight_decay"] = 0.3                                  # edited through torch, and back
    a2, b2, c2 = _group_params()
    fused2 = FusedAdamW([{"params": a2}, {"params": b2}, {"params": c2}])
    fused2.load_state_dict(ref.state_dict())
    assert torch.equal(fused2.bucket.m, fused.bucket.m) and torch.equal(fused2.bucket.v, fused.bucket.v)
    assert fused2.bucket.state[0] == 7.0 and fused2.betas == (0.8, 0.95)
    assert [g["lr_scale"] for g in fused2.param_groups] == [1.0, 0.1, 0.0]
    assert [g["weight_decay"] for g in fused2.param_groups] == [0.05, 0.0, 0.3]
    with pytest.raises(ValueError, match="number of parameter groups"):
        FusedAdamW(a2 + b2 + c2).load_state_dict(sd)
