"""CPU: the host side of GATv2 with edge features - the state_dict layout of GATv2EdgeConv and of the encoder / tri-modal
net with and without edge features, the GatGraph fields that align listed attribute rows with CSR positions, every
refusal that has to come before a launch (ValueError from the layer, MM_ERR_ARG from the entry points)."""
import ctypes

import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
import multimodal_eeg_fmri_amd.enhanced_models_v4 as E
from test_gnn_host import _gnn_keys, _shapes
from test_gnn_kernels_gpu import _edge_index


# ------------------------------------------------------------------------------------------------------ state dicts
def test_gatv2edgeconv_state_dict_layout_and_initialisation():
    torch.manual_seed(0)
    m = E.GATv2EdgeConv(24, 16, heads=4, edge_dim=3, dropout=0.1)
    want = {"att": (1, 4, 16), "bias": (64,), "lin_l.weight": (64, 24), "lin_l.bias": (64,), "lin_r.weight": (64, 24),
            "lin_r.bias": (64,), "lin_edge.weight": (64, 3)}
    assert _shapes(m) == want                                              # torch_geometric's GATv2Conv(edge_dim=3) keys
    for t, fan in ((m.lin_edge.weight, 64 + 3), (m.lin_l.weight, 64 + 24), (m.att, 4 + 16)):   # glorot: |w| <= sqrt(6 / fan)
        a = (6.0 / fan) ** 0.5
        assert t.abs().max() <= a and t.abs().max() > 0.8 * a
    assert m.fill_value == "mean" and m.edge_dim == 3
    plain = E.GATv2Conv(24, 16, heads=4)
    assert set(_shapes(m)) - set(_shapes(plain)) == {"lin_edge.weight"}
    res = m.load_state_dict({k: torch.zeros(v) for k, v in want.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for bad in (0, 9, -1, 2.0, None, True):
        with pytest.raises(ValueError):
            E.GATv2EdgeConv(8, 16, edge_dim=bad)
    for bad in ("max", None, [1.0]):
        with pytest.raises(ValueError):
            E.GATv2EdgeConv(8, 16, edge_dim=2, fill_value=bad)
    assert E.GATv2EdgeConv(8, 16, edge_dim=2, fill_value=0.5).fill_value == 0.5


def test_defaults_keep_their_key_sets_and_edge_features_add_only_lin_edge():
    base = _gnn_keys("", 12, 3, 64, 4)
    enc = E.GNNConnectivityEncoder(num_nodes=12, num_conn_types=3, hidden_dim=64, num_heads=4)
    assert _shapes(enc) == base and enc.edge_dim is None
    assert all(type(l) is E.GATv2Conv for l in enc.gat_layers)
    edge = E.GNNConnectivityEncoder(num_nodes=12, num_conn_types=3, hidden_dim=64, num_heads=4, edge_dim=3)
    extra = {f"gat_layers.{i}.lin_edge.weight": (64, 3) for i in range(2)}
    assert _shapes(edge) == {**base, **extra}
    assert all(type(l) is E.GATv2EdgeConv for l in edge.gat_layers)
    net = E.EnhancedTriModalFusionNet(8, 8, 12, hidden_dim=64)
    net_e = E.EnhancedTriModalFusionNet(8, 8, 12, hidden_dim=64, gnn_edge_features=True)
    assert _shapes(net, "conn_encoder.") == _gnn_keys("conn_encoder.", 12, 3, 64, 4)
    assert set(_shapes(net_e)) - set(_shapes(net)) == {"conn_encoder." + k for k in extra}
    assert set(_shapes(net)) <= set(_shapes(net_e)) and net_e.conn_encoder.edge_dim == 3
    assert _shapes(net_e)["conn_encoder.gat_layers.1.lin_edge.weight"] == (64, 3)


# ----------------------------------------------------------------------------------------------------- graph fields
def test_graph_fields_align_listed_rows_with_csr_positions():
    ei = _edge_index(2)                    # listed self-loops (3, 3) and (7, 7), edge 5 listed twice, node 11 without incoming edge
    n, El = 19, ei.shape[1]
    g = ops.gat_graph(ei, n)
    Ec = g.num_edges
    assert g.num_listed == El and Ec == El - 2 + n
    assert all(t.dtype == torch.int32 for t in (g.eid, g.indeg, g.pos, g.tgt))
    assert g.eid.shape == (Ec,) and g.indeg.shape == (n,) and g.pos.shape == (El,) and g.tgt.shape == (El,)
    rp, col, eid, pos = g.rowptr.tolist(), g.col.tolist(), g.eid.tolist(), g.pos.tolist()
    listed = ei.t().tolist()
    loops = [k for k, (s, t) in enumerate(listed) if s == t]
    assert len(loops) == 2 and all(pos[k] == -1 for k in loops)                   # dropped with their attributes
    assert sorted(e for e in eid if e >= 0) == [k for k in range(El) if k not in loops]   # every kept edge once
    for i in range(n):
        row = list(range(rp[i], rp[i + 1]))
        assert eid[row[-1]] == -1 and col[row[-1]] == i                             # the appended loop closes the row
        ids = [eid[e] for e in row[:-1]]
        assert ids == sorted(ids) and all(k >= 0 for k in ids)                      # listed order within a target
        for e in row[:-1]:
            assert listed[eid[e]] == [col[e], i] and pos[eid[e]] == e               # the same edge, both directions
        assert g.indeg[i] == len(row) - 1
    assert g.indeg[11] == 0 and g.tgt.tolist() == ei[1].tolist()
    dup = [k for k in range(El) if listed[k] == listed[5]]
    assert len(dup) == 2 and 0 <= pos[dup[0]] < pos[dup[1]]                           # both copies kept, in listed order
    # attention output order: the listed non-loop edges in listed order, then the n self-loops
    kept = [k for k in range(El) if k not in loops]
    assert g.attn_edge_index.dtype == torch.int64 and g.attn_edge_index.shape == (2, Ec)
    assert g.attn_edge_index.t().tolist() == [listed[k] for k in kept] + [[i, i] for i in range(n)]
    assert g.attn_pos.tolist() == [pos[k] for k in kept] + [rp[i + 1] - 1 for i in range(n)]
    g0 = ops.gat_graph(torch.zeros(2, 0, dtype=torch.long), 3)
    assert g0.num_listed == 0 and g0.eid.tolist() == [-1, -1, -1] and g0.indeg.tolist() == [0, 0, 0]


def test_existing_constructor_order_still_builds_a_graph():
    g = ops.gat_graph(torch.tensor([[0, 1], [1, 2]]), 3)
    h = ops.GatGraph(3, g.rowptr, g.col, g.colptr, g.row, g.perm)
    assert h.num_edges == 5 and h.eid is None and h.num_listed is None


# ----------------------------------------------------------------------------------------------------- value errors
def test_edge_layer_refuses_bad_edge_attr_before_any_launch():
    ei = torch.tensor([[0, 1, 2, 2], [1, 2, 0, 2]])                                # 4 listed edges, one a self-loop
    x2, x3 = torch.zeros(3, 8), torch.zeros(2, 3, 8)
    conv = E.GATv2EdgeConv(8, 16, heads=2, edge_dim=3)
    bad = [
        (x3, None),                                    # missing on an edge layer
        (x3, torch.zeros(4, 2)),                       # D = 2 on an edge_dim = 3 layer
        (x3, torch.zeros(4)),                          # (E,) is D = 1
        (x3, torch.zeros(5, 3)),                       # wrong E
        (x3, torch.zeros(3, 3)),                       # E without the listed self-loop: rows align with the LISTED edges
        (x3, torch.zeros(3, 4, 3)),                    # wrong B
        (x2, torch.zeros(2, 4, 3)),                    # 2-D x is a batch of one
        (x3, torch.zeros(2, 4, 3, 1)),                 # four dimensions
        (x3, torch.zeros(4, 3, dtype=torch.long)),     # not floating point
    ]
    for x, ea in bad:
        with pytest.raises(ValueError):
            conv(x, ei, ea)
    for d in (0, 9):
        with pytest.raises(ValueError):
            ops.gat_edge_attr(torch.zeros(4, d), ops.gat_graph(ei, 3), 2, d)
    with pytest.raises(ValueError):
        ops.gat_edge_attr(torch.zeros(2, 4, 9), ops.gat_graph(ei, 3), 2, 9)
    conv.fill_value = "median"
    with pytest.raises(ValueError):
        conv(x3, ei, torch.zeros(4, 3))
    # well-formed CPU input gets as far as the no-fallback rule
    conv.fill_value = "mean"
    for ea in (torch.zeros(4, 3), torch.zeros(2, 4, 3)):
        with pytest.raises(_hip.HipLibraryError):
            conv(x3, ei, ea)
    with pytest.raises(_hip.HipLibraryError):
        E.GATv2EdgeConv(8, 16, heads=2, edge_dim=1)(x3, ei, torch.zeros(4))
    with pytest.raises(NotImplementedError):
        E.GATv2Conv(8, 16, heads=2)(x3, ei, torch.zeros(4, 3))                      # the plain layer keeps refusing


def test_encoder_refuses_bad_edge_inputs_before_any_launch():
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    enc = E.GNNConnectivityEncoder(num_nodes=3, num_conn_types=3, hidden_dim=64, edge_dim=3)
    with pytest.raises(ValueError):
        enc(torch.zeros(2, 3, 9), ei)                                              # own connectivity needs (B, N, N, types)
    with pytest.raises(ValueError):
        E.GNNConnectivityEncoder(num_nodes=3, num_conn_types=3, hidden_dim=64, edge_dim=2)(torch.zeros(2, 3, 3, 3), ei)
    with pytest.raises(ValueError):
        enc(torch.zeros(2, 3, 3, 3), ei, torch.zeros(3, 2))                        # wrong D
    with pytest.raises(ValueError):
        enc(torch.zeros(2, 3, 3, 3), ei, torch.zeros(3, 3, 3))                     # wrong B
    with pytest.raises(ValueError):
        E.GNNConnectivityEncoder(num_nodes=3, hidden_dim=64)(torch.zeros(2, 3, 3, 3), ei, torch.zeros(3, 3))
    with pytest.raises(_hip.HipLibraryError):
        enc(torch.zeros(2, 3, 3, 3), ei)
    with pytest.raises(_hip.HipLibraryError):
        E.EnhancedTriModalFusionNet(8, 8, 3, hidden_dim=64, gnn_edge_features=True)(
            torch.zeros(2, 8, 64), torch.zeros(2, 8, 64), torch.zeros(2, 3, 3, 3))


# --------------------------------------------------------------------------------- kernel argument validation
def _args(table, **over):
    table = dict(table)
    table.update(over)
    return tuple(table.values())


def test_edge_entry_points_refuse_invalid_arguments_before_any_launch():
    lib = _hip.load()
    p, f = ctypes.c_void_p(256), ctypes.c_float
    fwd = dict(xl=p, xr=p, ld=64, att=p, bias=p, we=p, ea=p, batched=0, rowptr=p, col=p, out=p, pre=None, alpha=p, B=2, N=8,
               H=2, C=16, E=8, D=3, slope=f(0.2), act=0, drop_p=f(0.0), seed=0, epoch=None, stream=None)
    bwd = dict(dout=p, pre=None, xl=p, xr=p, ld=64, att=p, we=p, ea=p, batched=0, alpha=p, rowptr=p, col=p, colptr=p, row=p,
               perm=p, dxl=p, dxr=p, datt=p, dbias=p, dwe=p, dea=None, ds=p, dz=None, part=p, wpart=p, epart=None, B=2, N=8,
               H=2, C=16, E=8, D=3, slope=f(0.2), act=0, drop_p=f(0.0), seed=0, epoch=None, stream=None)
    pack = dict(listed=p, eid=p, rowptr=p, indeg=p, csr=p, Bo=1, N=8, El=4, E=12, D=3, fill_mean=1, fill=f(0.0), stream=None)
    pbwd = dict(dcsr=p, pos=p, tgt=p, rowptr=p, indeg=p, dlisted=p, Bo=1, N=8, El=4, E=12, D=3, fill_mean=1, stream=None)
    cases = [
        ("mm_gatv2_edge_fwd", _args(fwd, D=0), b"D=0"),
        ("mm_gatv2_edge_fwd", _args(fwd, D=9), b"D=9"),
        ("mm_gatv2_edge_fwd", _args(fwd, we=None), b"null"),
        ("mm_gatv2_edge_fwd", _args(fwd, ea=None), b"null"),
        ("mm_gatv2_edge_fwd", _args(fwd, N=129, E=129), b"N=129"),
        ("mm_gatv2_edge_fwd", _args(fwd, C=24), b"C=24"),
        ("mm_gatv2_edge_bwd", _args(bwd, D=9), b"D=9"),
        ("mm_gatv2_edge_bwd", _args(bwd, wpart=None), b"null"),
        ("mm_gatv2_edge_bwd", _args(bwd, ea=None), b"null"),
        ("mm_gatv2_edge_bwd", _args(bwd, dea=p), b"epart_ws"),              # d edge_attr without its workspace
        ("mm_gatv2_edge_bwd", _args(bwd, act=1), b"pre and dz_ws"),
        ("mm_gatv2_edge_pack", _args(pack, D=9), b"D=9"),
        ("mm_gatv2_edge_pack", _args(pack, eid=None), b"null"),
        ("mm_gatv2_edge_pack", _args(pack, E=13), b"E=13"),                # more CSR edges than listed + loops
        ("mm_gatv2_edge_pack", _args(pack, E=7), b"E=7"),
        ("mm_gatv2_edge_pack", _args(pack, Bo=0), b"B=0"),
        ("mm_gatv2_edge_pack_bwd", _args(pbwd, D=0), b"D=0"),
        ("mm_gatv2_edge_pack_bwd", _args(pbwd, pos=None), b"null"),
        ("mm_gatv2_edge_pack_bwd", _args(pbwd, N=129, E=133), b"N=129"),
    ]
    for name, args, word in cases:
        rc = getattr(lib, name)(*args)
        msg = lib.mm_last_error()
        assert rc == -1 and name[3:].encode() in msg and word in msg, (name, rc, msg)
