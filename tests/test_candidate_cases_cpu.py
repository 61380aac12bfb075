"""CPU tests of tests/candidate_cases.py, the yardstick of test_rank_candidates_gpu.py: the twelve kernel instances
are all hit, every row of every case has exactly one rank an evaluation within the score bar can return, the planted
ties are the fp64 ties, the lists hold their edge rows, and the vectorised reference agrees with a brute-force loop
over the header's text."""
import numpy as np
import pytest

from tests import candidate_cases as CC
from tests import strided as S
from tests import sweep_cases as SC


@pytest.mark.parametrize("name", CC.FNS)
def test_widths_hit_every_instance(name):
    got = [CC.dense_vg(name, d) for d in CC.WIDTHS]
    assert got == list(CC.VG) and len(set(got)) == 12
    assert all(g <= S.K_MAX_G for _, g in got)


def test_layout_names_exist():
    assert set(CC.LAYOUTS) <= set(SC.LAYOUTS)


@pytest.mark.parametrize("name", CC.FNS)
def test_every_row_has_one_possible_rank(name):
    """lo == hi for ALL rows, filtered and unfiltered, at every width and in both modes: no row is left out of the
    exact comparison. The distance functions are protected by the seeded tables as they are; DistMult / ComplEx by
    the scale factor (unscaled they are not: see the module text)."""
    for d in CC.WIDTHS:
        for mode, _ in CC.MODES:
            ref = CC.ref_scores(name, d, mode)
            truth, count = CC.truths(name, d, mode)
            assert sorted(CC.tie_plan(name, d, mode)) == list(CC.TIE_ROWS)
            assert count.min() > 0, (name, d, mode, int(count.min()))
            L, tw = CC.lists(name, d, mode), CC.twins(name, d, mode)
            for filtered in (False, True):
                ptr, ids = CC.filters(name, d, mode) if filtered else (None, None)
                lo, hi = CC.bounds(ref, truth, L, ptr, ids, tw)
                assert np.array_equal(lo, hi), (name, d, mode, filtered, np.nonzero(lo != hi)[0])
                ranks, _, _ = CC.expected(name, d, mode, filtered)
                assert np.array_equal(ranks, lo)


@pytest.mark.parametrize("name", SC.FNS)
def test_distance_tables_are_the_sweeps(name):
    """The distance functions' tables are sweep_cases.case's but for the planted copies, which no query reads."""
    d = 50
    for mode, _ in CC.MODES:
        a, b, plan = CC.case(name, d, mode), SC.case(name, d), CC.tie_plan(name, d, mode)
        copies = np.concatenate([cp for _, cp in plan.values()])
        srcs = [s for s, _ in plan.values()]
        assert len(set(copies.tolist()) | set(srcs)) == (1 + CC.NCOPY) * len(CC.TIE_ROWS)
        same = np.ones(CC.E, dtype=bool)
        same[copies] = False
        assert (a["ent"][same] == b["ent"][same]).all() and (a["rel"] == b["rel"]).all()
        assert (a["pos"] == b["pos"]).all()
        assert not np.isin(a["pos"][:, [0, 2]].numpy(), copies).any()
        for s, cp in plan.values():
            assert (a["ent"][cp] == a["ent"][s]).all()


@pytest.mark.parametrize("name,d", [("InterHT", 33), ("ComplEx", 16)])
def test_ref_scores_are_the_tables_scores(name, d):
    """ref_scores copies columns instead of scoring the tables with the copies: the same matrix."""
    for mode, _ in CC.MODES:
        assert np.array_equal(CC.ref_scores(name, d, mode), CC._fp64_scores(CC.case(name, d, mode), mode))


@pytest.mark.parametrize("name", CC.SCALED)
def test_scale_factor(name):
    """The largest |fp64 score| of a scaled case is about 4, and at the widths where the unscaled tables isolate
    nothing the scaled ones isolate most entities."""
    for d in (16, 1000):
        f = CC.scale_factor(name, d)
        assert f.dtype == np.float32 and f > 1.0
        top = max(np.abs(CC.ref_scores(name, d, mode)).max() for mode, _ in CC.MODES)
        assert 2.0 < top < 8.0, top  # 4 before the planted copies moved a few rows
        _, count = CC.truths(name, d, 1)
        assert count.min() >= CC.E // 2, int(count.min())
    raw = S.make_case(name, 1000, E=CC.E, R=CC.R, B=CC.B, N=1, seed=1000, gamma=CC.GAMMA)
    row = CC._fp64_scores(raw, 1)[0]
    assert SC.isolated(row).sum() == 0


@pytest.mark.parametrize("name", CC.FNS)
def test_planted_ties_are_the_fp64_ties(name):
    for d in (16, 255):
        for mode, _ in CC.MODES:
            for filtered in (False, True):
                _, ties, ts = CC.expected(name, d, mode, filtered)
                planted = CC.planted_ties(name, d, mode, filtered)
                assert np.array_equal(ties, planted), (name, d, mode, filtered)
                assert (planted[list(CC.TIE_ROWS)] >= 1).all()
                if not filtered:
                    assert (planted[list(CC.TIE_ROWS)] >= 3).all()
                assert np.isneginf(ts[[CC.ROW_MINUS1, CC.ROW_E]]).all()
            # the filtered copy takes its entries (two planted, and any drawn) out of the count
            q = CC.ROW_TIE_FILTERED
            gone = int((CC.lists(name, d, mode)[q] == CC.twins(name, d, mode)[q][0]).sum())
            assert gone >= 2
            assert CC.planted_ties(name, d, mode, True)[q] == CC.planted_ties(name, d, mode, False)[q] - gone


def test_list_edge_rows():
    name, d, mode = "TransE", 16, 1
    L, (truth, _) = CC.lists(name, d, mode), CC.truths(name, d, mode)
    E = CC.E
    assert L.shape == (CC.B, CC.C) and L.dtype == np.int64
    pad = (L < 0) | (L >= E)
    r = L[CC.ROW_PAD]
    assert pad[CC.ROW_PAD, 0] and pad[CC.ROW_PAD, -1] and pad[CC.ROW_PAD, 200:234].any() and not pad[CC.ROW_PAD].all()
    assert {-1, E, CC.FAR, -CC.FAR} <= set(r.tolist())
    assert (L[CC.ROW_OWN] == truth[CC.ROW_OWN]).sum() >= 2
    assert pad[CC.ROW_ALLPAD].all()
    same = L[CC.ROW_SAME][~pad[CC.ROW_SAME]]
    assert len(same) == 70 and len(set(same.tolist())) == 1 and same[0] != truth[CC.ROW_SAME]
    assert truth[CC.ROW_MINUS1] == -1 and truth[CC.ROW_E] == E
    plain = [q for q in range(CC.B) if q not in (CC.ROW_PAD, CC.ROW_ALLPAD, CC.ROW_SAME)]
    assert not pad[plain].any()
    assert any(len(set(L[q].tolist())) < CC.C for q in plain)  # draws with repeats
    ptr, ids = CC.filters(name, d, mode)
    n = np.diff(ptr)
    assert n[CC.ROW_EMPTY] == 0 and n[CC.ROW_LONG] > 64 and n[CC.ROW_ALL] == E
    assert truth[CC.ROW_TRUTH] in ids[ptr[CC.ROW_TRUTH]:ptr[CC.ROW_TRUTH + 1]]
    out = ids[ptr[CC.ROW_OUTSIDE]:ptr[CC.ROW_OUTSIDE + 1]]
    assert out[0] == -1 and out[-1] == E
    # what the edge rows must come to
    ranks, ties, _ = CC.expected(name, d, mode, False)
    assert ranks[CC.ROW_ALLPAD] == 1 and ties[CC.ROW_ALLPAD] == 0
    assert ranks[CC.ROW_SAME] in (1, 71)  # a repeated id is counted each time it appears
    assert ranks[CC.ROW_MINUS1] == 1 + CC.C and ranks[CC.ROW_E] == 1 + CC.C  # every entry is above -inf
    franks, fties, _ = CC.expected(name, d, mode, True)
    assert franks[CC.ROW_ALL] == 1 and fties[CC.ROW_ALL] == 0


def brute_force(A, truth, L, ptr, ids):
    """The header's text, entry by entry."""
    M, n_ent = A.shape
    ranks, ties = [], []
    for q in range(M):
        tr = int(truth[q])
        st = A[q, tr] if 0 <= tr < n_ent else float("-inf")
        flt = set() if ptr is None else set(int(x) for x in ids[ptr[q]:ptr[q + 1]])
        above = tie = 0
        for c in (L if L.ndim == 1 else L[q]).tolist():
            if not 0 <= c < n_ent or c == tr or c in flt:
                continue
            above += bool(A[q, c] > st)
            tie += bool(A[q, c] == st)
        ranks.append(1 + above)
        ties.append(tie)
    return np.array(ranks), np.array(ties)


@pytest.mark.parametrize("name,d", [("RotatE", 16), ("ComplEx", 33)])
def test_reference_against_brute_force(name, d):
    for mode, _ in CC.MODES:
        ref, (truth, _), L = CC.ref_scores(name, d, mode), CC.truths(name, d, mode), CC.lists(name, d, mode)
        for ptr, ids in ((None, None), CC.filters(name, d, mode)):
            for lst in (L, L[CC.ROW_PAD], L[:, :0]):  # per-row lists, one shared list, empty lists
                r, t, _ = CC.reference(ref, truth, lst, ptr, ids)
                br, bt = brute_force(ref, truth, lst, ptr, ids)
                assert np.array_equal(r, br) and np.array_equal(t, bt)
    # NaN on either side never counts
    A = np.array([[np.nan, 1.0, 2.0], [0.0, np.nan, 2.0]])
    r, t, _ = CC.reference(A, np.array([0, 0]), np.array([[1, 2, 2], [1, 2, 2]]))
    assert r.tolist() == [1, 3] and t.tolist() == [0, 0]
