"""CPU tests of PairRE (KGE_PAIRRE = 7): the fp64 reference's self-checks, the host layer of libkge_hip.so on dummy
pointers (tests/test_abi.py's style: everything here is decided before any device call), the model surface, and the
evaluation case generator's premise."""
import ctypes

import numpy as np
import pytest
import torch

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import _lib
from customknowledgegraphembedding_amd.distributed import ShardedKGE
from tests import pairre_cases as PC
from tests import pairre_ref as P
from tests import sweep_cases as W

FN, COMPLEX = 7, 2
EINVAL, ENOTSUP = -22, -95
d = ctypes.c_void_p(4096)  # a 16-B aligned dummy pointer: never dereferenced


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def test_reference_hand_worked_example():
    """D = 2: h = (3, 4) -> (0.6, 0.8); t = (0, 2) -> (0, 1); r_h = (1, -2), r_t = (0.5, 3):
    |0.6 - 0| + |-1.6 - 3| = 5.2, score = 10 - 5.2."""
    ent = torch.tensor([[3.0, 4.0], [0.0, 2.0]], dtype=torch.float64)
    rel = torch.tensor([[1.0, -2.0, 0.5, 3.0]], dtype=torch.float64)
    pos = torch.tensor([[0, 0, 1]])
    for mode, neg in ((3, None), (1, torch.tensor([[1]])), (0, torch.tensor([[0]]))):
        assert abs(float(P.score(ent, rel, pos, neg, mode, 10.0)[0, 0]) - 4.8) < 1e-12


def test_reference_properties():
    c = PC.case(33, 40, 5, 6, 9, seed=3)
    ent, rel = c.ent.double(), c.rel.double()
    for mode in (0, 1, 3):
        base = P.score(ent, rel, c.pos, c.neg, mode, c.gamma)
        # invariant under positive scaling of any entity row
        scale = torch.linspace(0.1, 7.0, c.E, dtype=torch.float64).unsqueeze(1)
        assert torch.allclose(P.score(ent * scale, rel, c.pos, c.neg, mode, c.gamma), base, rtol=0, atol=1e-12)
        # r_h = r_t = 0 gives gamma
        assert bool((P.score(ent, rel * 0, c.pos, c.neg, mode, c.gamma) == c.gamma).all())
    # a zero row (and an out-of-range id, which reads one) is finite and scores gamma - sum |q0|
    z = ent.clone()
    z[4] = 0
    pos = torch.tensor([[2, 1, 4], [2, 1, c.E], [2, 1, -1]])
    s = P.score(z, rel, pos, None, 3, c.gamma)
    want = c.gamma - (P.normalize(ent[2]) * rel[1, :33]).abs().sum()
    assert bool(torch.isfinite(s).all()) and torch.allclose(s, want.expand(3, 1), rtol=0, atol=1e-12)


def test_reference_entity_gradient_is_orthogonal_to_the_row():
    c = PC.case(24, 30, 4, 5, 7, seed=5)
    for mode in (0, 1):
        _, ge, gr = P.train_grads(c.ent.double(), c.rel.double(), c.pos, c.neg, c.w.double(), mode, c.gamma)
        x = c.ent.double()
        touched = ge.abs().sum(1) > 0
        assert int(touched.sum()) > 10
        dots = (x * ge).sum(1).abs()
        assert bool((dots[touched] <= 1e-10 * x.norm(dim=1)[touched] * ge.norm(dim=1)[touched]).all())
        assert float(gr[:, :24].abs().max()) > 0 and float(gr[:, 24:].abs().max()) > 0


# ------------------------------------------------------------------------------------------------
# the host layer
# ------------------------------------------------------------------------------------------------
def _score(lib, fn, B=2, N=4, D=4, rel_ld=8, rel_off=0):
    return lib.kge_score_indexed(fn, 1, d, 10, 4, d, 2, rel_ld, rel_off, d, d, 4, B, N, D, 1.0, 1.0, 0.0, d, 4, None)


def test_ids_and_limits():
    lib = kge.load()
    assert _lib.FN_IDS["PairRE"] == FN and kge.FN_IDS["PairRE"] == FN
    assert 6 not in _lib.FN_IDS.values()
    assert lib.kge_max_dim(FN) == lib.kge_max_dim(0) > 0  # TransE's limit: the entity row is not split
    assert lib.kge_max_dim(6) == 0
    assert _score(lib, 6) == EINVAL and b"score function" in lib.kge_last_error()
    assert lib.kge_shard_nq(6) == 0
    assert lib.kge_train_step_workspace_size(6, 10, 2, 8, 2, 4, 4) == -1


def test_empty_problems_are_noops_and_narrow_relation_rows_are_rejected():
    lib = kge.load()
    assert _score(lib, FN, B=0) == 0
    assert _score(lib, FN, N=0) == 0
    assert lib.kge_step_forward(FN, 1, d, 10, 4, d, 2, 8, 0, d, d, 4, 0, 4, 4, 1.0, 1.0, 0.0, 1.0, 1, d, 4, d, d, d,
                                None, None) == 0
    assert lib.kge_eval_rank_candidates(FN, 1, d, 10, 4, d, 2, 8, 0, d, 0, 4, 1.0, 1.0, 0.0, d, d, 4, 4, None, None,
                                        0, d, None, None, None) == 0
    # rel_ld < rel_off + 2 D
    for rel_ld, rel_off in ((7, 0), (4, 0), (8, 4), (11, 4)):
        assert _score(lib, FN, rel_ld=rel_ld, rel_off=rel_off) == EINVAL, (rel_ld, rel_off)
        assert b"rel_ld" in lib.kge_last_error()
    for size in (lib.kge_step_backward_adam_workspace_size, lib.kge_train_step_workspace_size,
                 lib.kge_train_step_reg_workspace_size, lib.kge_train_step_lazy_workspace_size):
        assert size(FN, 10, 2, 7, 2, 4, 4) == -1 and size(FN, 10, 2, 8, 2, 4, 4) > 0  # no step for rel_ld < 2 D
    ws = lib.kge_train_step_workspace_size(FN, 10, 2, 8, 2, 4, 4)
    rc = lib.kge_train_step(FN, 1, d, 10, 4, d, 2, 7, 0, d, d, 4, 2, 4, 4, 1.0, 1.0, 1.0, 1, 0, d, d, None, d, d, d,
                            d, d, d, 1e-3, 0.9, 0.999, 1e-7, 1, 1, d, ws, None)
    assert rc == EINVAL and b"rel_ld" in lib.kge_last_error()


def test_sharded_family_refuses_pairre():
    lib = kge.load()
    assert lib.kge_shard_nq(FN) == ENOTSUP and b"PairRE" in lib.kge_last_error()
    assert lib.kge_shard_train_workspace_size(FN, 10, 2, 8, 4, 4, 4) == ENOTSUP
    rc = lib.kge_score_sharded(FN, 1, d, 4, d, 2, 8, 0, d, 10, 4, 0, d, d, 4, 2, 4, 4, 1.0, 1.0, 0.0, d, 4, None)
    assert rc == ENOTSUP and b"PairRE" in lib.kge_last_error()
    rc = lib.kge_shard_score(FN, 1, d, 8, 4, d, d, 2, 8, 0, d, 10, 4, 0, d, 4, 4, 4, 1.0, 1.0, 0.0,
                             d, d, d, d, d, 2, 0, 2, 0, d, None)
    assert rc == ENOTSUP and b"PairRE" in lib.kge_last_error()
    big = 1 << 30
    common = [FN, 1, d, 10, 4, 0, d, d, 4, d, 2, 8, 0, d, d, 4, 4, 4, 4, 2, 2, 0, 1.0, 1.0, 1.0, 1, 0, d]
    assert lib.kge_shard_train_forward(*common, d, d, d, big, None) == ENOTSUP
    assert b"PairRE" in lib.kge_last_error()
    assert lib.kge_shard_train_combine(*common, d, d, d, d, d, d, big, None) == ENOTSUP
    assert lib.kge_shard_train_backward(*common, d, d, d, d, d, d, d, 1e-3, 0.9, 0.999, 1e-7, 1, 1, d, big,
                                        None) == ENOTSUP
    h = ctypes.c_void_p()
    rc = lib.kge_shard_exec_create(ctypes.addressof(h), None, 0, FN, 10, 10, 4, 4, 4, 4, 1, 0, 1, d, big, d, big)
    assert rc == ENOTSUP and b"PairRE" in lib.kge_last_error() and not h.value
    with pytest.raises(NotImplementedError, match="PairRE"):
        ShardedKGE("PairRE", 10, 2, 4, 1.0, double_relation_embedding=True, device="cpu", world=1, rank=0)


def test_eval_query_chain_still_refuses():
    lib = kge.load()
    assert lib.kge_eval_query(FN, 1, d, 10, 4, d, 2, 8, d, 2, 4, d, 4, None) == ENOTSUP
    assert lib.kge_eval_query_planes(FN, 1, d, 10, 4, d, 2, 8, d, 2, 4, d, 2, None) == ENOTSUP
    assert b"DistMult" in lib.kge_last_error()


@pytest.mark.parametrize("D,E,R,B,N", [(24, 97, 5, 4, 16), (1000, 523, 7, 40, 128), (1500, 14541, 237, 512, 256)])
def test_workspace_sizes_are_complexs_at_the_same_widths(D, E, R, B, N):
    """Every *_workspace_size depends on the function only through the entity row width and the width of the
    relation part the backward keeps (rel_w). ComplEx at per-half width D / 2 has entity rows D wide, as PairRE at
    D has, but its rel_w is D and its slot buffers (3 D per slot) are half as wide: so the equality relied on is
    with ComplEx at THE SAME per-half D for the buffers sized by D and rel_w = 2 D, after taking out the one term
    that differs, the slots' entity-gradient rows (ent_w = 2 D for ComplEx, D for PairRE): 2 B rows of D floats,
    256-B aligned as every region is."""
    lib = kge.load()
    rel_ld = 2 * D

    def a256(x):
        return (x + 255) // 256 * 256

    diff = a256(2 * B * 2 * D * 4) - a256(2 * B * D * 4)
    assert lib.kge_step_backward_workspace_size(FN, E, B, N, D) == \
        lib.kge_step_backward_workspace_size(COMPLEX, E, B, N, D) - diff
    for f in (lib.kge_step_backward_adam_workspace_size, lib.kge_train_step_workspace_size,
              lib.kge_train_step_reg_workspace_size, lib.kge_train_step_lazy_workspace_size):
        assert f(FN, E, R, rel_ld, B, N, D) == f(COMPLEX, E, R, rel_ld, B, N, D) - diff > 0
    assert lib.kge_score_bwd_workspace_size(FN, 1, B, N, D) == lib.kge_score_bwd_workspace_size(COMPLEX, 1, B, N, D)
    # sizes that do not depend on the function at all
    assert lib.kge_eval_rank_sweep_workspace_size(B, 100) > 0 and lib.kge_eval_topk_sweep_workspace_size(B, 10) > 0
    assert lib.kge_step_plan_size(FN, E, D, R, rel_ld, 0, B, N, D) == \
        (lib.kge_step_plan_size(0, E, D, R, D, 0, B, N, D) if D <= 1024 else 0)


# ------------------------------------------------------------------------------------------------
# the model surface
# ------------------------------------------------------------------------------------------------
def test_model_dims_and_flags():
    from customknowledgegraphembedding_amd.model import _dims_for

    assert _dims_for("PairRE", 8, 16) == (8, 0)
    for ed, rd in ((8, 8), (8, 24), (16, 16)):
        with pytest.raises(ValueError, match="PairRE"):
            _dims_for("PairRE", ed, rd)
    m = kge.TFKGEModel("PairRE", 11, 3, 8, 6.0, double_relation_embedding=True, device="cpu")
    assert (m.entity_dim, m.relation_dim, m._D, m._rel_off) == (8, 16, 8, 0)
    assert "PairRE" in m.model_func
    with pytest.raises(ValueError, match="PairRE"):  # without -dr the relation row is D wide
        kge.TFKGEModel("PairRE", 11, 3, 8, 6.0, device="cpu")
    # Q5's dead -dr stays dead for every other name
    t = kge.TFKGEModel("TransE", 11, 3, 8, 6.0, double_relation_embedding=True, device="cpu")
    assert t.relation_dim == 8
    u = kge.KGEModel("PairRE", 11, 3, 8, 6.0, double_relation_embedding=True, device="cpu")
    assert (u.entity_dim, u.relation_dim, u._D) == (8, 16, 8)
    with pytest.raises(ValueError, match="double_relation_embedding"):
        kge.KGEModel("PairRE", 11, 3, 8, 6.0, device="cpu")
    with pytest.raises(ValueError, match="double_relation_embedding"):
        kge.KGEModel("PairRE", 11, 3, 8, 6.0, double_entity_embedding=True, double_relation_embedding=True,
                     device="cpu")


# ------------------------------------------------------------------------------------------------
# the evaluation cases
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 33, 264, 1000, 1500])
def test_every_query_row_has_a_truth_no_score_within_the_bar_can_move(D):
    for mode, _ in PC.MODES:
        ref = PC.ref_scores(D, mode)
        truth, count = PC.truths(D, mode)  # asserts an isolated candidate in every row: none is left out
        assert (count > 0).all() and len(truth) == PC.B_EVAL
        ptr, ids = PC.filters(D, mode)
        for filt in ((None, None), (ptr, ids)):
            lo, hi = W.rank_bounds(ref, truth, *filt)
            assert (lo == hi).all(), (D, mode)
            want = PC.expected_ranks(D, mode, filtered=filt[0] is not None).numpy()
            assert (want == lo).all()
        inside = (truth >= 0) & (truth < PC.E_EVAL)
        assert int(inside.sum()) == PC.B_EVAL - 2
        lists, ranks, ties = PC.candidate_lists(D, mode)
        assert lists.shape == (PC.B_EVAL, 100) and (ranks >= 1).all() and (ties == 0).all()
        assert len(np.unique(ranks)) > 5
