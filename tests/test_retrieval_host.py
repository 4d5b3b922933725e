"""CPU: the retrieval entry points validate their arguments before touching a device (each bad call returns -1 with a
message), and ops.retrieval refuses CPU, non-fp32 and non-contiguous tensors."""
import ctypes

import pytest
import torch

from multimodal_eeg_fmri_amd import _hip, ops

P = ctypes.c_void_p(256)          # a non-null, 16-byte aligned dummy pointer: never dereferenced on a rejected call


def _retr(Q=P, G=P, pos=None, ranks=P, ti=None, ts=None, ws=P, Nq=8, Ng=8, D=16, k=0):
    lib = _hip.load()
    rc = lib.mm_retrieval(Q, G, pos, ranks, ti, ts, ws, Nq, Ng, D, k, None)
    return rc, lib.mm_last_error()


def test_retrieval_entry_points_are_declared_and_bound():
    sigs = _hip.parse_header()
    assert sigs["mm_retrieval"] == "pppppppiiii"
    assert sigs["mm_retrieval_ws_floats"] == "iiiip"
    assert ops.retrieval_kmax() >= 16


@pytest.mark.parametrize("kw,msg", [
    (dict(Q=None), b"null Q"),
    (dict(G=None), b"null Q, G"),
    (dict(ws=None), b"ws"),
    (dict(D=6), b"D must be"),
    (dict(D=0), b"D must be"),
    (dict(D=1028), b"D must be"),
    (dict(ranks=None, k=0), b"nothing to compute"),
    (dict(k=17, ti=P, ts=P, Ng=100), b"k must be"),
    (dict(k=3, ti=None, ts=P), b"topk_idx"),
    (dict(Nq=9, Ng=8), b"Nq <= Ng"),
    (dict(Nq=0), b"Nq, Ng"),
    (dict(Ng=(1 << 20) + 1), b"Nq, Ng"),
    (dict(k=9, ti=P, ts=P, Ng=8), b"k must be"),
    (dict(Q=ctypes.c_void_p(260)), b"aligned"),
])
def test_retrieval_argument_errors_are_reported_not_crashed(kw, msg):
    rc, err = _retr(**kw)
    assert rc == -1 and msg in err, err


def test_retrieval_workspace_query():
    lib = _hip.load()
    n = ctypes.c_int(-1)
    assert lib.mm_retrieval_ws_floats(1000, 5000, 128, 10, ctypes.addressof(n), None) == 0
    assert n.value >= 1000 * (1 + 1 + 2 * 10)
    assert lib.mm_retrieval_ws_floats(1000, 5000, 128, 10, None, None) == -1
    assert lib.mm_retrieval_ws_floats(1000, 5000, 130, 10, ctypes.addressof(n), None) == -1
    big = ctypes.c_int(-1)
    assert lib.mm_retrieval_ws_floats(1 << 20, 1 << 20, 128, 16, ctypes.addressof(big), None) == 0
    assert 0 < big.value < 2 ** 31


def test_ops_retrieval_refuses_bad_tensors():
    q = torch.randn(4, 8)
    with pytest.raises(_hip.HipLibraryError, match="CPU tensor"):
        ops.retrieval(q, q)
    meta = torch.empty(4, 8, device="meta")
    with pytest.raises((ValueError, _hip.HipLibraryError)):
        ops.retrieval(meta, meta)


def test_ops_retrieval_checks_dtype_and_layout_before_the_device(monkeypatch):
    """dtype / contiguity checks run on the tensor's metadata: a CPU tensor that only claims to be on the GPU reaches them"""
    class FakeCuda(torch.Tensor):
        @property
        def is_cuda(self):
            return True
    q = torch.randn(4, 8).as_subclass(FakeCuda)
    with pytest.raises(ValueError, match="float32"):
        ops.retrieval(q.double().as_subclass(FakeCuda), q)
    with pytest.raises(ValueError, match="contiguous"):
        ops.retrieval(torch.randn(8, 4).t().as_subclass(FakeCuda), q)
    with pytest.raises(ValueError, match="2-D"):
        ops.retrieval(torch.randn(8).as_subclass(FakeCuda), q)
