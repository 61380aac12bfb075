"""CPU tests of kge_eval_rank_sweep's boundary: the workspace query is host arithmetic, bad arguments are rejected
with the documented codes before any launch, and evaluate.rank_sweep has no CPU fallback."""
import ctypes

import pytest
import torch

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import _lib, evaluate


def test_workspace_size_is_host_arithmetic():
    lib = _lib.load()
    size = lib.kge_eval_rank_sweep_workspace_size
    assert size(0, 0) >= 0
    assert size(-1, 0) == 0 and size(4, -1) == 0
    prev_b = 0
    for B in (0, 1, 2, 3, 17, 1024, 4096):
        prev_f = 0
        for nf in (0, 1, 3, 4, 5, 1000, 50000):
            s = size(B, nf)
            assert s >= 0 and s % 16 == 0
            assert s >= prev_f  # non-decreasing in nfilter
            prev_f = s
            # the documented layout: float truth scores [B], int32 counts [B], the filter scores at the next 16 B
            assert s >= (B * 8 + 15) // 16 * 16 + 4 * nf
        assert size(B, 7) >= prev_b  # non-decreasing in B
        prev_b = size(B, 7)


def call(lib, fn=0, mode=1, ent=16, rel=16, pos=16, B=2, D=4, truth=16, fptr=None, fids=None, nf=0, ranks=16, ws=16,
         ws_bytes=1 << 20):
    p = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731
    return lib.kge_eval_rank_sweep(fn, mode, p(ent), 10, 4, p(rel), 2, 4, 0, p(pos), B, D, 1.0, 1.0, 0.0, p(truth),
                                   p(fptr), p(fids), nf, p(ranks), p(ws), ws_bytes, None)


def test_bad_arguments_are_rejected_without_a_launch():
    lib = _lib.load()
    assert call(lib, fn=99) == -22 and b"score function" in lib.kge_last_error()
    assert call(lib, mode=3) == -22 and b"mode" in lib.kge_last_error()  # KGE_SINGLE
    assert call(lib, mode=7) == -22 and b"mode" in lib.kge_last_error()
    for null in ("pos", "truth", "ranks", "ws", "ent", "rel"):
        assert call(lib, **{null: None}) == -22 and b"null" in lib.kge_last_error(), null
    assert call(lib, nf=3, fptr=None, fids=16) == -22 and lib.kge_last_error()
    assert call(lib, nf=3, fptr=16, fids=None) == -22 and lib.kge_last_error()
    need = lib.kge_eval_rank_sweep_workspace_size(2, 5)
    assert call(lib, nf=5, fptr=16, fids=16, ws_bytes=need - 1) == -22 and b"workspace" in lib.kge_last_error()
    assert call(lib, ws=8) == -22 and lib.kge_last_error()  # not 16-B aligned
    assert call(lib, B=-1) == -22 and call(lib, D=0) == -22 and call(lib, nf=-1) == -22
    # DistMult / ComplEx rank through the planes
    for fn in (1, 2):
        assert call(lib, fn=fn) == -95 and b"rank_planes" in lib.kge_last_error()
    # a per-half width the sweep has no instance for
    assert call(lib, D=2048) == -95 and lib.kge_last_error()
    # an empty batch is a successful no-op
    assert call(lib, B=0) == 0
    assert call(lib, B=0, pos=None, truth=None, ranks=None, ws=None, ws_bytes=0) == 0


def cpu_model(name="TransE"):
    if name == "InterHT":
        return kge.TFKGEModel(name, 10, 3, 8, 6.0, True, False, True, device="cpu", seed=0)
    return kge.KGEModel(name, 10, 3, 8, 6.0, device="cpu", seed=0)


@pytest.mark.parametrize("name", ["TransE", "InterHT"])
def test_no_cpu_fallback(name):
    m = cpu_model(name)
    pos = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(kge.KGEHipError, match="no CPU fallback"):
        evaluate.rank_sweep(m, pos, "tail-batch", pos[:, 2].contiguous())


def test_index_tensors_are_checked():
    m = cpu_model()
    pos = torch.zeros(4, 3, dtype=torch.int64)
    truth = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="positive_sample"):
        evaluate.rank_sweep(m, pos.int(), "tail-batch", truth)
    with pytest.raises(ValueError, match="truth"):
        evaluate.rank_sweep(m, pos, "tail-batch", truth.int())
    with pytest.raises(ValueError, match="truth"):
        evaluate.rank_sweep(m, pos, "head-batch", pos[:, 0])  # a strided column
    with pytest.raises(ValueError, match="truth"):
        evaluate.rank_sweep(m, pos, "head-batch", truth[:3])  # one per query row
    fptr = torch.zeros(5, dtype=torch.int64)
    with pytest.raises(ValueError, match="filter_ptr"):
        evaluate.rank_sweep(m, pos, "tail-batch", truth, fptr.int(), None, 0)
    with pytest.raises(ValueError, match="filter_ids"):
        evaluate.rank_sweep(m, pos, "tail-batch", truth, fptr, torch.zeros(3, dtype=torch.int32), 3)
    assert "rank_sweep" in evaluate.__all__


def test_models_without_a_sweep_answer_none():
    """Callers fall back on None: a model whose function the library has no sweep for is not an error."""
    class Other:
        model_name = "TranSparse"
    assert evaluate.rank_sweep(Other(), None, "tail-batch", None) is None
    assert not evaluate._sweep_rank_ok(Other())
