"""CPU tests of kge_eval_rank_candidates' boundary: bad arguments are rejected with the documented codes and a
message before any launch, an empty batch is a no-op, and evaluate.rank_candidates checks its tensors and has no CPU
fallback."""
import ctypes

import pytest
import torch

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import _lib, evaluate

EINVAL, ENOTSUP = -22, -95


def call(lib, fn=0, mode=1, ent=16, nent=10, rel=16, nrel=2, pos=16, M=2, D=4, truth=16, cand=16, cand_ld=5, C=5,
         fptr=None, fids=None, nf=0, ranks=16, ties=16, ts=16, ent_ld=None):
    p = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731
    return lib.kge_eval_rank_candidates(fn, mode, p(ent), nent, D if ent_ld is None else ent_ld, p(rel), nrel, D, 0,
                                        p(pos), M, D, 1.0, 1.0, 0.0, p(truth), p(cand), cand_ld, C, p(fptr), p(fids),
                                        nf, p(ranks), p(ties), p(ts), None)


def test_symbol_and_abi_version():
    lib = _lib.load()
    assert hasattr(lib, "kge_eval_rank_candidates")
    assert lib.kge_abi_version() == 1  # the change is additive


def test_bad_arguments_are_rejected_without_a_launch():
    lib = _lib.load()
    assert call(lib, fn=99) == EINVAL and b"score function" in lib.kge_last_error()
    assert call(lib, fn=-1) == EINVAL and b"score function" in lib.kge_last_error()
    for mode in (3, 7, -1):  # KGE_SINGLE and anything else
        assert call(lib, mode=mode) == EINVAL and b"mode" in lib.kge_last_error()
    for kw in (dict(M=-1), dict(C=-1), dict(D=0), dict(D=-4), dict(nent=-1), dict(nrel=-1), dict(nf=-1),
               dict(cand_ld=-1)):
        assert call(lib, **kw) == EINVAL and b"shape" in lib.kge_last_error(), kw
    for null in ("ent", "rel", "pos", "truth", "ranks"):
        assert call(lib, **{null: None}) == EINVAL and b"null" in lib.kge_last_error(), null
    assert call(lib, cand=None) == EINVAL and b"cand" in lib.kge_last_error()
    assert call(lib, cand_ld=4, C=5) == EINVAL and b"cand_ld" in lib.kge_last_error()
    assert call(lib, cand_ld=1, C=5) == EINVAL and b"cand_ld" in lib.kge_last_error()
    assert call(lib, nf=3, fptr=None, fids=16) == EINVAL and b"filter" in lib.kge_last_error()
    assert call(lib, nf=3, fptr=16, fids=None) == EINVAL and b"filter" in lib.kge_last_error()


def test_width_refused_where_score_indexed_refuses_it():
    """More than 8 x 64 vector groups per half-row: float4 rows past 2 048, float2 rows past 1 024, scalar rows past
    512, for every function (DistMult and ComplEx too: this entry point has no function restriction)."""
    lib = _lib.load()
    for fn in range(6):
        assert call(lib, fn=fn, D=2052) == ENOTSUP and b"register-resident" in lib.kge_last_error()
        assert call(lib, fn=fn, D=1026) == ENOTSUP  # D % 4 != 0: float2 rows
        assert call(lib, fn=fn, D=513) == ENOTSUP   # scalar rows
        assert call(lib, fn=fn, D=1024, ent=20) == ENOTSUP  # a base 4 B off 16: scalar rows
        assert call(lib, fn=fn, D=1024, ent_ld=1025) == ENOTSUP  # an odd row stride: scalar rows


def test_empty_batch_is_a_noop():
    lib = _lib.load()
    assert call(lib, M=0) == 0
    assert call(lib, M=0, ent=None, rel=None, pos=None, truth=None, cand=None, ranks=None, ties=None, ts=None) == 0
    assert call(lib, M=0, C=0, cand=None, cand_ld=0) == 0
    assert lib.kge_last_error() == b""


def cpu_model(name="TransE"):
    if name == "InterHT":
        return kge.TFKGEModel(name, 10, 3, 8, 6.0, True, False, True, device="cpu", seed=0)
    return kge.KGEModel(name, 10, 3, 8, 6.0, device="cpu", seed=0)


@pytest.mark.parametrize("name", ["TransE", "DistMult", "InterHT"])
def test_no_cpu_fallback(name):
    m = cpu_model(name)
    pos = torch.zeros(2, 3, dtype=torch.int64)
    cand = torch.zeros(2, 4, dtype=torch.int64)
    with pytest.raises(kge.KGEHipError, match="no CPU fallback"):
        evaluate.rank_candidates(m, pos, "tail-batch", cand)
    with pytest.raises(kge.KGEHipError, match="no CPU fallback"):
        evaluate.rank_candidates(m, pos, "head-batch", cand[0].contiguous(), want_ties=True)
    with pytest.raises(kge.KGEHipError, match="no CPU fallback"):
        evaluate.test_step_candidates(m, pos.numpy(), cand, None)


def test_index_tensors_are_checked():
    m = cpu_model()
    pos = torch.zeros(4, 3, dtype=torch.int64)
    truth = torch.zeros(4, dtype=torch.int64)
    cand = torch.zeros(4, 6, dtype=torch.int64)
    rc = evaluate.rank_candidates
    with pytest.raises(ValueError, match="positive_sample"):
        rc(m, pos.int(), "tail-batch", cand)
    with pytest.raises(ValueError, match="positive_sample"):
        rc(m, pos[:, :2], "tail-batch", cand)
    with pytest.raises(ValueError, match="mode"):
        rc(m, pos, "single", cand)
    with pytest.raises(ValueError, match="candidates"):
        rc(m, pos, "tail-batch", cand.int())
    with pytest.raises(ValueError, match="candidates"):
        rc(m, pos, "tail-batch", cand[:3])  # one list per query row
    with pytest.raises(ValueError, match="candidates"):
        rc(m, pos, "tail-batch", cand[:, ::2])  # strided within a row
    with pytest.raises(ValueError, match="candidates"):
        rc(m, pos, "tail-batch", cand.t().contiguous().t())  # rows not contiguous
    with pytest.raises(ValueError, match="candidates"):
        rc(m, pos, "tail-batch", cand[0, ::2])  # a strided shared list
    with pytest.raises(ValueError, match="candidates"):
        rc(m, pos, "tail-batch", cand.reshape(2, 2, 6))
    with pytest.raises(ValueError, match="truth"):
        rc(m, pos, "tail-batch", cand, truth.int())
    with pytest.raises(ValueError, match="truth"):
        rc(m, pos, "head-batch", cand, pos[:, 0])  # a strided column
    with pytest.raises(ValueError, match="truth"):
        rc(m, pos, "head-batch", cand, truth[:3])  # one per query row
    fptr = torch.zeros(5, dtype=torch.int64)
    with pytest.raises(ValueError, match="filter_ptr"):
        rc(m, pos, "tail-batch", cand, truth, fptr.int(), None, 0)
    with pytest.raises(ValueError, match="filter_ptr"):
        rc(m, pos, "tail-batch", cand, truth, fptr[:4], None, 0)
    with pytest.raises(ValueError, match="filter_ids"):
        rc(m, pos, "tail-batch", cand, truth, fptr, torch.zeros(3, dtype=torch.int32), 3)
    with pytest.raises(ValueError, match="ties"):
        evaluate.test_step_candidates(m, pos.numpy(), cand, None, ties="median")
    assert "rank_candidates" in evaluate.__all__ and "test_step_candidates" in evaluate.__all__


def test_models_without_a_function_id_answer_none():
    class Other:
        model_name = "TranSparse"
    assert evaluate.rank_candidates(Other(), None, "tail-batch", None) is None
