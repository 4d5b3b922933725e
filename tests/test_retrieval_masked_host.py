"""CPU: the host side of retrieval with ignored temporal neighbours - mm_retrieval_masked and its workspace query are
declared and bound, every argument error comes back as an error code (or a ValueError from ops.retrieval /
retrieval_metrics / evaluate_retrieval / fit) before any launch, the workspace query agrees with the layout the header
documents, and radius = 0 makes the calls it always made (`_hip.call` patched and recorded; nothing here launches)."""
import contextlib
import ctypes
import re

import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops
from multimodal_eeg_fmri_amd.bridge_trainer import BridgeTrainer
from multimodal_eeg_fmri_amd.bridge_utils import retrieval_metrics

P = ctypes.c_void_p(256)          # a non-null, 16-byte aligned dummy pointer: never dereferenced on a rejected call


def _masked(Q=P, G=P, qgid=P, ggid=P, radius=1, ranks=P, neg=None, ti=None, ts=None, ws=P, Nq=8, Ng=8, D=16, k=0):
    lib = _hip.load()
    rc = lib.mm_retrieval_masked(Q, G, qgid, ggid, radius, ranks, neg, ti, ts, ws, Nq, Ng, D, k, None)
    return rc, lib.mm_last_error()


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", " ", open(_hip.header_path()).read(), flags=re.S)
    m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in the header"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_masked_entry_points_are_declared_and_bound():
    assert _declaration("mm_retrieval_masked") == [
        "const float* Q", "const float* G", "const int* qgid", "const int* ggid", "int radius", "int* ranks",
        "int* negatives", "int* topk_idx", "float* topk_score", "float* ws", "int Nq", "int Ng", "int D", "int k",
        "hipStream_t stream"]
    assert _declaration("mm_retrieval_masked_ws_floats") == [
        "int Nq", "int Ng", "int D", "int k", "int* floats_host", "hipStream_t stream"]
    sigs = _hip.parse_header()
    assert sigs["mm_retrieval_masked"] == "ppppi" + "ppppp" + "iiii"
    assert sigs["mm_retrieval_masked_ws_floats"] == sigs["mm_retrieval_ws_floats"] == "iiiip"
    lib = _hip.load()
    assert hasattr(lib, "mm_retrieval_masked") and hasattr(lib, "mm_retrieval_masked_ws_floats")
    assert _hip.header_abi_version() == 5 and lib.mm_abi_version() == 5          # entry points were only added


@pytest.mark.parametrize("kw,msg", [
    (dict(Q=None), b"null Q"),
    (dict(G=None), b"null Q, G"),
    (dict(qgid=None), b"qgid"),
    (dict(ggid=None), b"ggid"),
    (dict(ws=None), b"ws"),
    (dict(radius=-1), b"radius=-1 must be >= 0"),
    (dict(ranks=None, k=0), b"nothing to compute"),
    (dict(ranks=None, neg=P, k=0), b"nothing to compute"),
    (dict(k=3, ti=None, ts=P), b"topk_idx"),
    (dict(k=3, ti=P, ts=None), b"topk_score"),
    (dict(ranks=None, k=3, ti=None, ts=None), b"topk_idx"),
    (dict(D=6), b"D must be"),
    (dict(D=0), b"D must be"),
    (dict(D=1028), b"D must be"),
    (dict(Nq=0), b"Nq, Ng"),
    (dict(Ng=0), b"Nq, Ng"),
    (dict(Ng=(1 << 20) + 1), b"Nq, Ng"),
    (dict(Nq=(1 << 20) + 1), b"Nq, Ng"),
    (dict(k=17, ti=P, ts=P, Ng=100), b"k must be"),
    (dict(k=9, ti=P, ts=P, Ng=8), b"k must be"),
    (dict(k=-1, ti=P, ts=P), b"k must be"),
    (dict(Q=ctypes.c_void_p(260)), b"aligned"),
    (dict(G=ctypes.c_void_p(264)), b"aligned"),
])
def test_masked_argument_errors_are_reported_not_crashed(kw, msg):
    rc, err = _masked(**kw)
    assert rc == -1 and msg in err and b"mm_retrieval_masked" in err, err


def _slices(nq, ng):
    """the number of gallery slices as include/mmeeg_hip.h documents it"""
    cdiv = lambda a, b: -(-a // b)
    qb, t = cdiv(nq, 128), cdiv(ng, 128)
    w = max(1, min(t, cdiv(512, qb)))
    return cdiv(t, cdiv(t, w))


@pytest.mark.parametrize("nq,ng,d,k", [(1000, 5000, 128, 10), (2049, 4100, 64, 0), (1, 1, 4, 1), (70000, 300, 64, 16)])
def test_masked_workspace_query_agrees_with_the_documented_layout(nq, ng, d, k):
    lib = _hip.load()
    n, plain = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.mm_retrieval_masked_ws_floats(nq, ng, d, k, ctypes.addressof(n), None) == 0
    s = _slices(nq, ng)
    # s* | maxima / counts [S][Nq] | id-only counts [S][Nq] | list scores [S][Nq][k] | list indices [S][Nq][k]
    assert n.value == nq * (1 + s * (2 + 2 * k))
    assert lib.mm_retrieval_ws_floats(nq, ng, d, k, ctypes.addressof(plain), None) == 0
    assert n.value - plain.value == s * nq                    # mm_retrieval's layout plus the second per-slice count


def test_masked_workspace_query_errors_and_the_largest_shape():
    lib = _hip.load()
    n = ctypes.c_int(-1)
    assert _slices(2049, 4100) == 17 and _slices(37, 1000) == 8 and _slices(130, 257) == 3
    assert lib.mm_retrieval_masked_ws_floats(1000, 5000, 128, 10, None, None) == -1
    assert b"floats_host" in lib.mm_last_error()
    assert lib.mm_retrieval_masked_ws_floats(1000, 5000, 130, 10, ctypes.addressof(n), None) == -1
    assert lib.mm_retrieval_masked_ws_floats(1000, 5000, 128, 17, ctypes.addressof(n), None) == -1
    assert lib.mm_retrieval_masked_ws_floats(1 << 20, 1 << 20, 128, 16, ctypes.addressof(n), None) == 0
    assert 0 < n.value < 2 ** 31


class FakeCuda(torch.Tensor):
    """a CPU tensor that claims to be on the GPU: reaches every check that reads metadata only"""
    @property
    def is_cuda(self):
        return True


def test_ops_retrieval_radius_errors_come_before_any_launch(monkeypatch):
    calls = []
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append(name))
    q, g = torch.zeros(4, 8), torch.zeros(6, 8)
    iq, ig = torch.arange(4), torch.arange(6)
    with pytest.raises(ValueError, match="radius must be >= 0"):
        ops.retrieval(q, g, q_groups=iq, g_groups=ig, radius=-1)
    with pytest.raises(ValueError, match="radius=2 needs group ids"):
        ops.retrieval(q, g, radius=2)
    with pytest.raises(ValueError, match="radius=2 needs group ids"):
        ops.retrieval(q, g, q_groups=iq, radius=2)
    with pytest.raises(ValueError, match="return_negatives=True needs group ids"):
        ops.retrieval(q, g, return_negatives=True)
    with pytest.raises(ValueError, match="exclusive"):
        ops.retrieval(q, g, torch.arange(4), q_groups=iq, g_groups=ig, radius=1)
    with pytest.raises(_hip.HipLibraryError, match="CPU tensor"):
        ops.retrieval(q, g, q_groups=iq, g_groups=ig, radius=1)
    qf, gf = q.as_subclass(FakeCuda), g.as_subclass(FakeCuda)
    with pytest.raises(ValueError, match="k must be"):
        ops.retrieval(qf, gf, k=7, q_groups=iq, g_groups=ig, radius=1)
    with pytest.raises(ValueError, match="nothing to compute"):
        ops.retrieval(qf, gf, ranks=False, q_groups=iq, g_groups=ig, radius=1)
    with pytest.raises(ValueError, match="shape"):
        ops.retrieval(qf, gf, q_groups=ig, g_groups=ig, radius=1)
    with pytest.raises(ValueError, match="integer"):
        ops.retrieval(qf, gf, q_groups=iq.float(), g_groups=ig, radius=1)
    # the grouped form's refusals hold at radius = 0 (tests/test_groups_host.py) and only there
    with pytest.raises(ValueError, match="only ranks"):
        ops.retrieval(q, g, k=2, q_groups=iq, g_groups=ig, radius=0)
    assert calls == []


def test_metrics_trainer_and_fit_refuse_a_radius_without_ids_before_any_launch(monkeypatch):
    calls = []
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append(name))
    z = torch.zeros(4, 8)
    with pytest.raises(ValueError, match="radius=1 needs groups"):
        retrieval_metrics(z, z, radius=1)
    with pytest.raises(ValueError, match="radius must be >= 0"):
        retrieval_metrics(z, z, groups=torch.arange(4), radius=-2)
    torch.manual_seed(0)
    tr = BridgeTrainer(eeg_channels=8, device="cpu", mode="manual")
    monkeypatch.setattr(tr, "embed", lambda *a, **k: pytest.fail("the encoders ran"))
    eeg, fmri = torch.zeros(4, 8, 256), torch.zeros(4, 1, 16, 16, 16)
    with pytest.raises(ValueError, match="radius=2 needs groups="):
        tr.evaluate_retrieval(eeg, fmri, radius=2)
    with pytest.raises(ValueError, match="radius must be >= 0"):
        tr.evaluate_retrieval(eeg, fmri, groups=torch.arange(4), radius=-1)
    with pytest.raises(ValueError):
        tr.evaluate_retrieval(eeg, fmri, groups=torch.zeros(4), radius=2)           # bad ids: before the encoders too
    with pytest.raises(ValueError, match="val_radius=2 needs val"):
        tr.fit([], 2, val=(eeg, fmri), val_radius=2, warmup_epochs=0)
    with pytest.raises(ValueError, match="val_radius=2 needs val"):
        tr.fit([], 2, val_radius=2, warmup_epochs=0)
    with pytest.raises(ValueError, match="val_radius must be >= 0"):
        tr.fit([], 2, val=(eeg, fmri, torch.arange(4)), val_radius=-1, warmup_epochs=0)
    assert calls == []


def _record(monkeypatch):
    """patch `_hip.call` (and the workspace queries, which go through it) and record (name, scalar arguments); the
    tensors of these tests are `FakeCuda`, the outputs are whatever torch.empty holds"""
    calls = []
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append((name, tuple(x for x in a if isinstance(x, int)))))
    monkeypatch.setattr(_hip, "host_int", lambda name, *a: 16)
    monkeypatch.setattr(_hip, "load", lambda: None)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    return calls


def test_radius_zero_makes_the_calls_it_always_made(monkeypatch):
    calls = _record(monkeypatch)
    q, g = torch.zeros(4, 8).as_subclass(FakeCuda), torch.zeros(6, 8).as_subclass(FakeCuda)
    iq, ig = torch.arange(4), torch.arange(6)
    out = ops.retrieval(q, g, k=2, radius=0)
    assert len(out) == 3 and calls == [("mm_retrieval", (4, 6, 8, 2))]
    del calls[:]
    out = ops.retrieval(q, g, q_groups=iq, g_groups=ig, radius=0)
    assert len(out) == 3 and out[1] is None and out[2] is None and calls == [("mm_retrieval_grouped", (4, 6, 8))]
    del calls[:]
    out = ops.retrieval(q, g, q_groups=iq, g_groups=ig)                 # the default is radius = 0
    assert calls == [("mm_retrieval_grouped", (4, 6, 8))]
    del calls[:]
    # radius > 0: the masked entry point, radius in front of the outputs, k and ranks=False allowed
    out = ops.retrieval(q, g, k=2, ranks=False, q_groups=iq, g_groups=ig, radius=3)
    assert calls == [("mm_retrieval_masked", (3, 4, 6, 8, 2))]
    assert len(out) == 3 and out[0] is None and out[1].shape == (4, 2) and out[1].dtype == torch.int64
    del calls[:]
    out = ops.retrieval(q, g, q_groups=iq, g_groups=ig, radius=3, return_negatives=True)
    assert calls == [("mm_retrieval_masked", (3, 4, 6, 8, 0))]
    assert len(out) == 4 and out[3].shape == (4,) and out[3].dtype == torch.int64 and out[0].dtype == torch.int64


def test_retrieval_metrics_radius_zero_is_todays_dict_and_calls(monkeypatch):
    calls = _record(monkeypatch)
    z = torch.zeros(4, 8).as_subclass(FakeCuda)
    ids = torch.tensor([0, 1, 5, 6])
    m = retrieval_metrics(z, z, radius=0)
    assert [c[0] for c in calls] == ["mm_retrieval", "mm_retrieval"]
    assert list(m) == ["eeg_to_fmri", "fmri_to_eeg", "n", "chance"]
    assert list(m["eeg_to_fmri"]) == ["R@1", "R@5", "R@10", "median_rank", "mean_rank", "mrr"]
    del calls[:]
    m = retrieval_metrics(z, z, groups=ids, radius=0)
    assert [c[0] for c in calls] == ["mm_retrieval_grouped", "mm_retrieval_grouped"]
    assert list(m) == ["eeg_to_fmri", "fmri_to_eeg", "n", "chance"]
    del calls[:]
    m = retrieval_metrics(z, z, groups=ids, radius=1)
    assert calls == [("mm_retrieval_masked", (1, 4, 4, 8, 0))] * 2
    assert m["radius"] == 1 and set(m) == {"eeg_to_fmri", "fmri_to_eeg", "n", "chance", "radius"}
    for key in ("eeg_to_fmri", "fmri_to_eeg"):
        assert {"ignored_mean", "chance_R@1"} <= set(m[key])
