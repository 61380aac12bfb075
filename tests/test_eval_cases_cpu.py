"""The references and cases of test_eval_widths_gpu.py (tests/eval_cases.py), held to the oracle and to their own
stated properties without a GPU: split3_ref's terms sum to their input exactly, rank_ref is the oracle's rank, the
tied and duplicated cases hold the edges they claim, and the end-to-end models meet the condition the GPU test
puts on its reference (few queries whose fp64 rank an fp32 evaluation may move)."""
import numpy as np
import pytest
import torch

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import evaluate
from oracle import kge_oracle as O
from tests import eval_cases as C
from tests import strided as S


@pytest.mark.parametrize("cols", [1, 13, 16, 50])
def test_split3_ref_terms_sum_to_the_input(cols):
    x = C.split_values(37, cols, seed=cols)
    assert bool(((x == 0) & torch.signbit(x)).any()) and bool(((x == 0) & ~torch.signbit(x)).any())
    p = C.split3_ref(x)
    kp = C.kpad(cols)
    assert p.shape == (3, kp // 16, 37, 16) and p.dtype == torch.bfloat16
    back = C.planes_sum(p.view(torch.int16))
    assert torch.equal(back[:, :cols], x.double())  # 24 significant bits: exact for every normal input
    assert bool((back[:, cols:] == 0).all())
    assert bool((p.view(torch.int16).permute(0, 2, 1, 3).reshape(3, 37, kp)[:, :, cols:] == 0).all())  # +0 bits
    # each term is the rounding of what the earlier ones left (the header's definition, element by element)
    flat = p.permute(0, 2, 1, 3).reshape(3, 37, kp)[:, :, :cols].float()
    assert torch.equal(flat[0].to(torch.bfloat16).float(), flat[0])
    assert torch.equal((x - flat[0]).to(torch.bfloat16).float(), flat[1])
    assert torch.equal(((x - flat[0]) - flat[1]).to(torch.bfloat16).float(), flat[2])


def test_rank_ref_is_the_oracles_dense_rank():
    """Tie-free fp64 data: rank_ref on O.eval_scores_dense's matrix with evaluate.build_filter's CSR equals
    O.eval_ranks_dense's ranks, and O.eval_ranks' (upstream's argsort) on a small DistMult case."""
    E, R, d = 97, 4, 8
    ent, rel, _ = O.make_tables(E, R, d, d, 9.0, d, seed=5, dtype=torch.float64)
    g = np.random.RandomState(1)
    true = np.stack([g.randint(E, size=300), g.randint(R, size=300), g.randint(E, size=300)], 1).astype(np.int64)
    true[40:90, :2] = true[0, :2]
    test = torch.from_numpy(true[:25])
    for mode, col in (("head-batch", 0), ("tail-batch", 2)):
        Sm = O.eval_scores_dense("DistMult", ent, rel, test, mode)
        ptr, ids = evaluate.build_filter(true[:25], mode, true)
        got = C.rank_ref(Sm, test[:, col], ptr, ids)
        want, lo, hi = O.eval_ranks_dense("DistMult", ent, rel, test, mode, [tuple(x) for x in true.tolist()],
                                          rtol=1e-15)
        assert torch.equal(lo, hi)  # tie-free
        assert torch.equal(got, want)
        assert torch.equal(got, O.eval_ranks("DistMult", ent, rel, test, mode, true.tolist(), 9.0))
        assert torch.equal(C.rank_ref(Sm, test[:, col]), 1 + (Sm > Sm.gather(1, test[:, col:col + 1])).sum(1))


def test_rank_ref_edges():
    """The header's rules on a hand-made row: ties and NaN never count, an out-of-range truth scores -inf, filter
    ids out of range or equal to the truth are ignored."""
    A = np.array([[1.0, 2.0, 2.0, np.nan, np.inf, -np.inf, 3.0]], dtype=np.float32)
    r = lambda t, f=None: int(C.rank_ref(A, [t], None if f is None else [0, len(f)], f)[0])  # noqa: E731
    assert r(1) == 3 and r(2) == 3  # above 2.0: inf and 3.0; the tie does not count
    assert r(3) == 1  # a NaN truth: nothing compares above it
    assert r(4) == 1 and r(5) == 6  # above -inf: every entry but the NaN and itself
    assert r(-1) == 6 and r(7) == 6  # -inf truth: everything but NaN and -inf
    assert r(1, [6, 4]) == 1 and r(1, [1, -1, 7, 2, 3]) == 3 and r(-1, [0, 1, 2, 3, 4, 5, 6]) == 1


@pytest.mark.parametrize("N", [1, 2, 3, 5, 64, 211, 1030])
def test_tied_rank_case_holds_its_edges(N):
    A, truth, fptr, fids = (t.numpy() for t in C.tied_rank_case(N))
    assert A.shape == (C.TIE_ROWS, N) and fptr[0] == 0 and fptr[-1] == len(fids)
    assert truth[1] == -1 and truth[2] == N and np.isnan(A[3, truth[3]])
    assert A[4, truth[4]] == np.inf and A[5, truth[5]] == -np.inf
    row = lambda q: fids[fptr[q]:fptr[q + 1]]  # noqa: E731
    assert len(row(0)) == 0 and truth[6] in row(6) and -1 in row(7) and N in row(7) and len(row(8)) == N
    for q in range(C.TIE_ROWS):
        assert len(np.unique(row(q))) == len(row(q))
    if N >= 64:  # many exact ties with the truth on the plain rows, and NaN / inf entries present
        for q in (0, 6, 7):
            assert int((A[q] == A[q, truth[q]]).sum()) > 2, q
        assert np.isnan(A).any() and np.isposinf(A).any() and np.isneginf(A).any()
        # counting >= instead of > would change the rank of a plain row
        assert int((A[0] >= A[0, truth[0]]).sum()) - 1 != int((A[0] > A[0, truth[0]]).sum())


@pytest.mark.parametrize("name,d", [("DistMult", 12), ("ComplEx", 50)])
def test_duplicate_table_ties_by_construction(name, d):
    c = C.duplicate_table(name, d)
    ent, ids = c["ent"], c["dup_ids"]
    assert len(np.unique(ids)) == 160 and bool(torch.isinf(ent[c["E"] - 3]).all())
    for j in range(40):
        assert all(torch.equal(ent[int(ids[j, 0])], ent[int(i)]) for i in ids[j, 1:])
    for mode, col in ((0, 0), (1, 2)):
        truth, fptr, fids = (t.numpy() for t in c["filt"][mode])
        assert truth[9] == -1 and truth[11] == c["E"] and fptr[-1] == len(fids) and fptr[2] == fptr[3]
        ndup = 0
        for q in range(c["B"]):
            row = fids[fptr[q]:fptr[q + 1]]
            assert len(np.unique(row)) == len(row)
            if 0 <= truth[q] < c["E"]:
                assert truth[q] in ids
                j = int(np.nonzero(ids == truth[q])[0][0])
                ndup += len(np.intersect1d(row, ids[j][ids[j] != truth[q]]))
        assert ndup > c["B"] // 2 and -1 in fids and c["E"] in fids and (c["E"] - 3) in fids


def test_query_vg_restates_the_narrowing():
    """query_vg on CPU stand-ins (strides and 16-B aligned bases as the GPU views have): the widths the issue's
    dimensions are labelled with, the narrowing by ldq and by Q's base, and the refusals past K_MAX_G groups."""
    def vg(D, ent_ld=None, ldq=None, qoff=0):
        ent = torch.zeros(4, ent_ld or D)[:, :D]
        q = S.canary(3, D, ldq or D, "cpu", k=qoff)
        assert ent.data_ptr() % 16 == 0 and q._base.data_ptr() % 16 == 0  # (torch's CPU allocator: 64 B)
        return C.query_vg(D, ent, ent, q)

    for D, want in ((4, (4, 1)), (256, (4, 1)), (260, (4, 2)), (1000, (4, 4)), (2048, (4, 8)), (2, (2, 1)),
                    (130, (2, 2)), (1022, (2, 8)), (1, (1, 1)), (33, (1, 1)), (255, (1, 4)), (449, (1, 8)), (450, (2, 4))):
        assert vg(D) == want, D
    assert vg(256, ldq=260) == (4, 1) and vg(256, ldq=257) == (1, 4) and vg(256, ldq=258) == (1, 4)
    assert vg(256, qoff=1) == (1, 4) and vg(256, qoff=2) == (2, 2) and vg(130, qoff=1) == (1, 4)
    assert vg(1000, ldq=1001)[1] > S.K_MAX_G and vg(1000, ent_ld=1001)[1] > S.K_MAX_G
    assert vg(260, ent_ld=261) == (1, 8) and vg(450, ent_ld=451) == (1, 8) and vg(450, qoff=1) == (1, 8)


@pytest.mark.parametrize("name,d,seed", C.E2E_MODELS)
def test_e2e_reference_meets_its_condition(name, d, seed):
    """The condition test_eval_widths_gpu.py puts on its end-to-end reference, for the reference alone: at most
    E2E_MAX_UNDECIDED of the queries have lo != hi under rtol = 1e-6 (observed on the fp64 oracle: 0 of 120 for
    every model here), the hub pairs give long filter lists, and the tables are the model's own."""
    c = C.e2e_case(name, d, seed)
    share = C.undecided_share(c)
    assert share <= C.E2E_MAX_UNDECIDED, f"{name} d={d} seed={seed}: {share:.4f} of the queries have lo != hi"
    for mode in ("head-batch", "tail-batch"):
        ptr, _ = evaluate.build_filter(c["test"], mode, c["true"])
        assert int(np.diff(ptr).max()) > 100, mode
    de = name == "ComplEx"
    m = kge.KGEModel(name, C.E2E_E, C.E2E_R, d, C.E2E_GAMMA, double_entity_embedding=de,
                     double_relation_embedding=de, device="cpu", seed=seed)
    assert torch.equal(m.entity_embedding.detach(), c["ent"]) and torch.equal(m.relation_embedding.detach(), c["rel"])
    print(f"{name} d={d}: undecided share {share:.4f}")
