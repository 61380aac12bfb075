"""CPU tests of the top-k link-prediction boundary (kge_eval_topk_sweep, kge_topk_rows, evaluate.predict): the
workspace query is host arithmetic, bad arguments are rejected with the documented codes before any launch,
build_exclude keeps the query's own answer, and nothing falls back to the CPU."""
import ctypes

import numpy as np
import pytest
import torch

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import _lib, evaluate

EINVAL, ENOTSUP = -22, -95


def test_workspace_size_is_host_arithmetic():
    lib = _lib.load()
    size = lib.kge_eval_topk_sweep_workspace_size
    assert size(-1, 10) == 0 and size(4, 0) == 0 and size(4, 65) == 0 and size(4, -1) == 0
    prev_b = 0
    for B in (0, 1, 2, 15, 16, 17, 31, 32, 33, 1024, 4096):
        prev_k = 0
        for k in (1, 2, 10, 63, 64):
            s = size(B, k)
            assert s >= 0 and s % 16 == 0
            assert s >= prev_k  # non-decreasing in k
            prev_k = s
            # at least one (score, id) list of k entries per query row and entity slice
            assert s >= B * 8 * k * 8
        assert size(B, 10) >= prev_b  # non-decreasing in B
        prev_b = size(B, 10)


def sweep(lib, fn=0, mode=1, ent=16, rel=16, pos=16, B=2, D=4, xptr=None, xids=None, nx=0, k=10, ids=16, scores=16,
          ws=16, ws_bytes=1 << 24):
    p = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731
    return lib.kge_eval_topk_sweep(fn, mode, p(ent), 10, 4, p(rel), 2, 4, 0, p(pos), B, D, 1.0, 1.0, 0.0, p(xptr),
                                   p(xids), nx, k, p(ids), k, p(scores), k, p(ws), ws_bytes, None)


def test_sweep_rejections_precede_any_launch():
    lib = _lib.load()
    assert sweep(lib, k=0) == EINVAL and b"k" in lib.kge_last_error()
    assert sweep(lib, k=65) == EINVAL and b"k" in lib.kge_last_error()
    assert sweep(lib, k=-1) == EINVAL
    assert sweep(lib, mode=3) == EINVAL and b"mode" in lib.kge_last_error()  # KGE_SINGLE
    assert sweep(lib, mode=7) == EINVAL
    assert sweep(lib, fn=99) == EINVAL and b"score function" in lib.kge_last_error()
    for fn in (1, 2):  # DistMult / ComplEx: the matrix path
        assert sweep(lib, fn=fn) == ENOTSUP and lib.kge_last_error()
    assert sweep(lib, D=2048) == ENOTSUP and lib.kge_last_error()  # 8 groups per lane: no instance
    need = lib.kge_eval_topk_sweep_workspace_size(2, 10)
    assert need > 0
    assert sweep(lib, ws_bytes=need - 1) == EINVAL and b"workspace" in lib.kge_last_error()
    assert sweep(lib, ws=8) == EINVAL and lib.kge_last_error()  # not 16-B aligned
    for null in ("pos", "ids", "scores", "ws", "ent", "rel"):
        assert sweep(lib, **{null: None}) == EINVAL and b"null" in lib.kge_last_error(), null
    assert sweep(lib, nx=3, xptr=None, xids=16) == EINVAL
    assert sweep(lib, nx=3, xptr=16, xids=None) == EINVAL
    assert sweep(lib, B=-1) == EINVAL and sweep(lib, D=0) == EINVAL and sweep(lib, nx=-1) == EINVAL
    # an empty batch is a successful no-op
    assert sweep(lib, B=0) == 0
    assert sweep(lib, B=0, pos=None, ids=None, scores=None, ws=None, ws_bytes=0) == 0


def rows(lib, S=16, M=2, N=5, ld=5, xptr=None, xids=None, nx=0, k=3, ids=16, scores=16):
    p = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731
    return lib.kge_topk_rows(p(S), M, N, ld, p(xptr), p(xids), nx, k, p(ids), k, p(scores), k, None)


def test_rows_rejections_precede_any_launch():
    lib = _lib.load()
    assert rows(lib, k=0) == EINVAL and b"k" in lib.kge_last_error()
    assert rows(lib, k=65) == EINVAL and b"k" in lib.kge_last_error()
    assert rows(lib, M=-1) == EINVAL and rows(lib, N=-1) == EINVAL and rows(lib, nx=-1) == EINVAL
    for null in ("S", "ids", "scores"):
        assert rows(lib, **{null: None}) == EINVAL and b"null" in lib.kge_last_error(), null
    assert rows(lib, nx=2, xptr=16, xids=None) == EINVAL
    assert rows(lib, M=0) == 0
    assert rows(lib, M=0, S=None, ids=None, scores=None) == 0


def test_build_exclude_keeps_the_querys_own_answer():
    known = [(0, 0, 1), (0, 0, 5), (0, 0, 3), (2, 0, 3), (4, 1, 3), (0, 0, 3)]  # one duplicate
    q = np.array([[0, 0, 3], [2, 0, 9], [7, 1, 3], [9, 1, 9]])
    ptr, ids = evaluate.build_exclude(q, "tail-batch", known)
    assert ptr.dtype == np.int64 and ids.dtype == np.int64
    # (0, 0, ?): 1, 3, 5 with the query's own tail 3 kept; (2, 0, ?): 3; (7, 1, ?) and (9, 1, ?): nothing known
    assert ptr.tolist() == [0, 3, 4, 4, 4] and ids.tolist() == [1, 3, 5, 3]
    ptr, ids = evaluate.build_exclude(q, "head-batch", known)
    # (?, 0, 3): 0, 2 with the query's own head 0 kept; (?, 0, 9): none; (?, 1, 3): 4; (?, 1, 9): none
    assert ptr.tolist() == [0, 2, 2, 3, 3] and ids.tolist() == [0, 2, 4]
    # build_filter drops the query's own answer, build_exclude does not
    fptr, fids = evaluate.build_filter(q, "tail-batch", known)
    assert fptr.tolist() == [0, 2, 3, 3, 3] and fids.tolist() == [1, 5, 3]
    ptr, ids = evaluate.build_exclude(np.zeros((0, 3), dtype=np.int64), "tail-batch", known)
    assert ptr.tolist() == [0] and len(ids) == 0


def cpu_model(name="TransE"):
    return kge.KGEModel(name, 10, 3, 8, 6.0, device="cpu", seed=0)


@pytest.mark.parametrize("name", ["TransE", "DistMult"])
def test_predict_has_no_cpu_fallback(name):
    m = cpu_model(name)
    q = np.zeros((2, 3), dtype=np.int64)
    with pytest.raises(kge.KGEHipError, match="no CPU fallback"):
        evaluate.predict(m, q, "tail-batch", k=3)
    with pytest.raises(kge.KGEHipError, match="no CPU fallback"):
        m.predict(q, "head-batch", k=3, known_triples=[(0, 0, 0)])
    with pytest.raises(kge.KGEHipError, match="no CPU fallback"):
        evaluate.topk_rows(torch.zeros(2, 5), 3)
    with pytest.raises(kge.KGEHipError, match="no CPU fallback"):
        evaluate.topk_sweep(m, torch.zeros(2, 3, dtype=torch.int64), "tail-batch", 3)


def test_python_argument_checks():
    m = cpu_model()
    q = np.zeros((2, 3), dtype=np.int64)
    for k in (0, 65, -1):
        with pytest.raises(ValueError, match="k must be"):
            evaluate.predict(m, q, "tail-batch", k=k)
        with pytest.raises(ValueError, match="k must be"):
            evaluate.topk_rows(torch.zeros(2, 5), k)
    with pytest.raises(ValueError, match="mode"):
        evaluate.predict(m, q, "single", k=3)
    pos = torch.zeros(4, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="positive_sample"):
        evaluate.topk_sweep(m, pos.int(), "tail-batch", 3)
    with pytest.raises(ValueError, match="excl_ptr"):
        evaluate.topk_sweep(m, pos, "tail-batch", 3, torch.zeros(5, dtype=torch.int32), None, 0)
    with pytest.raises(ValueError, match="excl_ptr"):
        evaluate.topk_sweep(m, pos, "tail-batch", 3, torch.zeros(4, dtype=torch.int64), None, 0)  # B + 1 entries
    with pytest.raises(ValueError, match="excl_ids"):
        evaluate.topk_sweep(m, pos, "tail-batch", 3, torch.zeros(5, dtype=torch.int64),
                            torch.zeros(3, dtype=torch.int32), 3)
    with pytest.raises(ValueError, match="scores"):
        evaluate.topk_rows(torch.zeros(2, 5, dtype=torch.float64), 3)
    for name in ("build_exclude", "topk_sweep", "topk_rows", "predict"):
        assert name in evaluate.__all__


def test_symbols_are_declared_and_bound():
    lib = _lib.load()
    for name in ("kge_eval_topk_sweep_workspace_size", "kge_eval_topk_sweep", "kge_topk_rows"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.kge_abi_version() == 1
