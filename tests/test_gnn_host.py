"""CPU: the host side of the GATv2 connectivity encoder - graph preparation (ops.gat_graph), the state_dict layout of
GATv2Conv / GNNConnectivityEncoder / EnhancedTriModalFusionNet, the no-fallback rule, and the argument validation of
mm_gatv2_fwd / mm_gatv2_bwd (which runs before any launch, so without a GPU)."""
import ctypes

import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
import multimodal_eeg_fmri_amd.enhanced_models_v4 as E


def _edges(g):
    """[(source, target)] in CSR order, from the CSR arrays alone"""
    rp, col = g.rowptr.tolist(), g.col.tolist()
    return [(col[e], i) for i in range(g.num_nodes) for e in range(rp[i], rp[i + 1])]


def _check_views(g):
    N, E = g.num_nodes, g.num_edges
    assert all(t.dtype == torch.int32 for t in (g.rowptr, g.col, g.colptr, g.row, g.perm))
    assert g.rowptr.shape == (N + 1,) and g.colptr.shape == (N + 1,) and g.col.shape == g.row.shape == g.perm.shape == (E,)
    assert g.rowptr[0] == 0 and g.rowptr[-1] == E and g.colptr[0] == 0 and g.colptr[-1] == E
    csr = _edges(g)
    cp, row, perm = g.colptr.tolist(), g.row.tolist(), g.perm.tolist()
    assert sorted(perm) == list(range(E))                                   # every edge once
    for j in range(N):
        mine = perm[cp[j]:cp[j + 1]]
        assert mine == sorted(mine)                                         # CSR order within a source
        for t in range(cp[j], cp[j + 1]):
            assert csr[perm[t]] == (j, row[t])                              # the same edge in both views


def test_listed_self_loops_are_replaced_by_one_per_node_and_duplicates_stay():
    #            src -> dst; (1, 1) and (3, 3) twice are listed self-loops, (2, 0) is listed twice
    ei = torch.tensor([[0, 1, 1, 2, 3, 2, 0, 3],
                       [1, 1, 0, 0, 3, 0, 2, 3]])
    g = ops.gat_graph(ei, 5)
    _check_views(g)
    # targets in order; within a target the listed order, the added self-loop last
    assert _edges(g) == [(1, 0), (2, 0), (2, 0), (0, 0), (0, 1), (1, 1), (0, 2), (2, 2), (3, 3), (4, 4)]
    assert g.num_edges == 10
    loops = [e for e in _edges(g) if e[0] == e[1]]
    assert sorted(loops) == [(n, n) for n in range(5)]


def test_order_is_stable_within_a_target():
    ei = torch.tensor([[5, 2, 4, 0, 3, 1],
                       [6, 6, 6, 6, 6, 6]])
    g = ops.gat_graph(ei, 7)
    _check_views(g)
    rp = g.rowptr.tolist()
    assert g.col.tolist()[rp[6]:rp[7]] == [5, 2, 4, 0, 3, 1, 6]


def test_isolated_node_has_degree_one_and_an_empty_edge_list_works():
    g = ops.gat_graph(torch.tensor([[0], [1]]), 4)
    _check_views(g)
    deg = (g.rowptr[1:] - g.rowptr[:-1]).tolist()
    assert deg == [1, 2, 1, 1]
    g0 = ops.gat_graph(torch.zeros(2, 0, dtype=torch.long), 3)
    _check_views(g0)
    assert _edges(g0) == [(0, 0), (1, 1), (2, 2)]


def test_graph_is_built_once_per_edge_index_tensor():
    ei = torch.tensor([[0, 1], [1, 2]])
    g = ops.gat_graph(ei, 3)
    assert ops.gat_graph(ei, 3) is g
    assert ops.gat_graph(ei, 4) is not g                                     # another node count: another graph
    ei[0, 0] = 2                                                             # changed in place: rebuilt
    assert _edges(ops.gat_graph(ei, 3)) == [(0, 0), (2, 1), (1, 1), (1, 2), (2, 2)]


@pytest.mark.parametrize("bad", [
    torch.tensor([[0, 3], [1, 0]]),                  # source out of range
    torch.tensor([[0, 1], [1, -1]]),                 # negative target
    torch.tensor([0, 1, 2]),                         # not (2, E)
    torch.tensor([[0, 1], [1, 0], [0, 0]]),          # three rows
    torch.tensor([[0.0, 1.0], [1.0, 0.0]]),          # not integers
])
def test_malformed_graph_raises_value_error(bad):
    with pytest.raises(ValueError):
        ops.gat_graph(bad, 3)


# ------------------------------------------------------------------------------------------------------ models
def _gat_keys(prefix, inp, H, C):
    return {prefix + "att": (1, H, C), prefix + "bias": (H * C,),
            prefix + "lin_l.weight": (H * C, inp), prefix + "lin_l.bias": (H * C,),
            prefix + "lin_r.weight": (H * C, inp), prefix + "lin_r.bias": (H * C,)}


def _bn_keys(prefix, n):
    return {prefix + "weight": (n,), prefix + "bias": (n,), prefix + "running_mean": (n,),
            prefix + "running_var": (n,), prefix + "num_batches_tracked": ()}


def _gnn_keys(prefix, nodes, types, hid, heads, layers=2):
    want = {prefix + "node_proj.0.weight": (hid, nodes * types), prefix + "node_proj.0.bias": (hid,),
            prefix + "output_proj.0.weight": (hid, hid), prefix + "output_proj.0.bias": (hid,)}
    want.update(_bn_keys(prefix + "node_proj.1.", hid))
    want.update(_bn_keys(prefix + "output_proj.1.", hid))
    for i in range(layers):
        want.update(_gat_keys(f"{prefix}gat_layers.{i}.", hid, heads, hid // heads))
    return want


def _shapes(m, prefix=""):
    return {k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith(prefix)}


def test_gatv2conv_state_dict_layout_and_initialisation():
    torch.manual_seed(0)
    m = E.GATv2Conv(24, 16, heads=4, dropout=0.1)
    assert _shapes(m) == _gat_keys("", 24, 4, 16)
    for b in (m.bias, m.lin_l.bias, m.lin_r.bias):
        assert torch.count_nonzero(b) == 0
    for t, fan in ((m.lin_l.weight, 64 + 24), (m.lin_r.weight, 64 + 24), (m.att, 4 + 16)):      # glorot: |w| <= sqrt(6 / fan)
        a = (6.0 / fan) ** 0.5
        assert t.abs().max() <= a and t.abs().max() > 0.8 * a
    assert not torch.equal(m.lin_l.weight, m.lin_r.weight)
    for kw in (dict(concat=False), dict(share_weights=True), dict(edge_dim=3)):
        with pytest.raises(NotImplementedError):
            E.GATv2Conv(8, 16, **kw)


def test_gnn_encoder_and_trimodal_state_dict_layout():
    enc = E.GNNConnectivityEncoder(num_nodes=12, num_conn_types=3, hidden_dim=64, num_heads=4)
    assert _shapes(enc) == _gnn_keys("", 12, 3, 64, 4)
    m = E.EnhancedTriModalFusionNet(8, 8, 12, hidden_dim=64)
    assert _shapes(m, "conn_encoder.") == _gnn_keys("conn_encoder.", 12, 3, 64, 4)
    tops = {k.split(".")[0] for k in m.state_dict()}
    assert tops == {"erp_encoder", "pw_encoder", "conn_encoder", "fusion", "cross_attn", "classifier"}
    assert m.edge_index is None and "edge_index" not in m.state_dict()
    mlp = E.EnhancedTriModalFusionNet(8, 8, 12, hidden_dim=64, use_gnn=False)
    want = {"conn_encoder.0.weight": (256, 12 * 12 * 3), "conn_encoder.0.bias": (256,),
            "conn_encoder.4.weight": (64, 256), "conn_encoder.4.bias": (64,)}
    want.update(_bn_keys("conn_encoder.1.", 256))
    want.update(_bn_keys("conn_encoder.5.", 64))
    assert _shapes(mlp, "conn_encoder.") == want
    for net in (m, mlp):
        sd = net.state_dict()
        assert sd["classifier.8.weight"].shape == (2, 32) and sd["cross_attn.in_proj_weight"].shape == (192, 64)
        assert sd["fusion.fusion_logits"].shape == (3,)


def test_load_state_dict_round_trip():
    torch.manual_seed(1)
    a = E.EnhancedTriModalFusionNet(8, 8, 12, hidden_dim=64)
    torch.manual_seed(2)
    b = E.EnhancedTriModalFusionNet(8, 8, 12, hidden_dim=64)
    assert not torch.equal(a.conn_encoder.gat_layers[1].att, b.conn_encoder.gat_layers[1].att)
    res = b.load_state_dict(a.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for (k, u), (_, v) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(u, v), k


def test_get_fusion_weights_reads_the_static_weights():
    m = E.EnhancedTriModalFusionNet(8, 8, 12, hidden_dim=64)
    with torch.no_grad():
        m.fusion.fusion_logits.copy_(torch.tensor([0.0, 1.0, 2.0]))
        m.fusion.temperature.fill_(2.0)
    w = E.get_fusion_weights(m)
    want = torch.softmax(torch.tensor([0.0, 0.5, 1.0], dtype=torch.float64), 0).tolist()
    assert set(w) == {"erp_weight", "pw_weight", "conn_weight", "temperature"} and w["temperature"] == 2.0
    assert [w["erp_weight"], w["pw_weight"], w["conn_weight"]] == pytest.approx(want, abs=1e-6)


def test_cpu_tensors_raise_instead_of_falling_back():
    ei = torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(_hip.HipLibraryError):
        E.GATv2Conv(8, 16, heads=2)(torch.zeros(3, 8), ei)
    with pytest.raises(_hip.HipLibraryError):
        E.GNNConnectivityEncoder(num_nodes=3, hidden_dim=64)(torch.zeros(2, 3, 3, 3), ei)
    with pytest.raises(_hip.HipLibraryError):
        E.EnhancedTriModalFusionNet(8, 8, 3, hidden_dim=64)(torch.zeros(2, 8, 64), torch.zeros(2, 8, 64), torch.zeros(2, 3, 3, 3))
    with pytest.raises(_hip.HipLibraryError):
        ops.gatv2_forward(E.GATv2Conv(8, 16), torch.zeros(1, 3, 8), ops.gat_graph(ei, 3))


# --------------------------------------------------------------------------------- kernel argument validation
def _fwd_args(p, N=8, H=2, C=16, E=8, **over):
    a = dict(xl=p, xr=p, ld=2 * H * C, att=p, bias=p, rowptr=p, col=p, out=p, pre=None, alpha=p, B=2, N=N, H=H, C=C, E=E,
             slope=ctypes.c_float(0.2), act=0, drop_p=ctypes.c_float(0.0), seed=0, epoch=None, stream=None)
    a.update(over)
    return tuple(a.values())


def _bwd_args(p, N=8, H=2, C=16, E=8, **over):
    a = dict(dout=p, pre=None, xl=p, xr=p, ld=2 * H * C, att=p, alpha=p, rowptr=p, col=p, colptr=p, row=p, perm=p,
             dxl=p, dxr=p, datt=p, dbias=p, ds=p, dz=None, part=p, B=2, N=N, H=H, C=C, E=E, slope=ctypes.c_float(0.2), act=0,
             drop_p=ctypes.c_float(0.0), seed=0, epoch=None, stream=None)
    a.update(over)
    return tuple(a.values())


def test_gatv2_entry_points_refuse_invalid_arguments_before_any_launch():
    lib = _hip.load()
    p = ctypes.c_void_p(256)
    cases = [
        ("mm_gatv2_fwd", _fwd_args(p, N=129, E=129), b"N=129"),
        ("mm_gatv2_fwd", _fwd_args(p, N=0), b"N=0"),
        ("mm_gatv2_fwd", _fwd_args(p, C=24), b"C=24"),
        ("mm_gatv2_fwd", _fwd_args(p, H=5, C=64), b"H*C=320"),
        ("mm_gatv2_fwd", _fwd_args(p, E=7), b"E=7"),                       # fewer edges than self-loops
        ("mm_gatv2_fwd", _fwd_args(p, ld=16), b"ld=16"),
        ("mm_gatv2_fwd", _fwd_args(p, xl=None), b"null"),
        ("mm_gatv2_fwd", _fwd_args(p, col=None), b"null"),
        ("mm_gatv2_fwd", _fwd_args(p, alpha=None), b"null"),
        ("mm_gatv2_fwd", _fwd_args(p, drop_p=ctypes.c_float(1.0)), b"drop_p"),
        ("mm_gatv2_bwd", _bwd_args(p, N=129, E=129), b"N=129"),
        ("mm_gatv2_bwd", _bwd_args(p, C=24), b"C=24"),
        ("mm_gatv2_bwd", _bwd_args(p, dout=None), b"null"),
        ("mm_gatv2_bwd", _bwd_args(p, perm=None), b"null"),
        ("mm_gatv2_bwd", _bwd_args(p, dxl=None), b"null"),
        ("mm_gatv2_bwd", _bwd_args(p, act=1), b"pre and dz_ws"),            # GELU epilogue without its saved tensors
    ]
    for name, args, word in cases:
        rc = getattr(lib, name)(*args)
        msg = lib.mm_last_error()
        assert rc == -1 and name[3:].encode() in msg and word in msg, (name, rc, msg)
