"""GPU tests of exact filtered top-k link prediction: evaluate.topk_sweep (kge_eval_topk_sweep), evaluate.topk_rows
(kge_topk_rows) and evaluate.predict. The yardstick is a stable descending torch.sort on the CPU of score_all's
matrix, the row's excluded ids and NaNs dropped first (candidates in ascending id, so ties come out by ascending
id): ids must be equal and scores bitwise equal, no tolerance. The fp64 oracle check uses the project's bar
1e-4 max(1, |ref|)."""
import os

import numpy as np
import pytest
import torch

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import evaluate
from oracle import kge_oracle as O
from tests import sweep_cases as W

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
DEV = "cuda"
FNS = ("TransE", "RotatE", "pRotatE", "InterHT")
MODES = ("head-batch", "tail-batch")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def make_model(name, E, R, d, gamma, seed=5):
    if name in ("InterHT",):
        return kge.TFKGEModel(name, E, R, d, gamma, True, False, True, device=DEV, seed=seed)
    if name == "TranSparse":
        return kge.TFKGEModel(name, E, R, d, gamma, device=DEV, seed=seed)
    de = name in ("RotatE", "ComplEx")
    return kge.KGEModel(name, E, R, d, gamma, double_entity_embedding=de, double_relation_embedding=name == "ComplEx",
                        device=DEV, seed=seed)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV)


def queries(g, E, R, B):
    return np.stack([g.randint(E, size=B), g.randint(R, size=B), g.randint(E, size=B)], 1)


# the yardstick and the bitwise comparison, shared with test_sweep_widths_gpu.py
reference, same = W.topk_reference, W.same_topk


def random_exclude(g, E, B, most=12, extra=()):
    rows = [np.unique(np.concatenate([g.randint(E, size=g.randint(most + 1)), np.asarray(extra, dtype=np.int64)]))
            for _ in range(B)]
    rows[0] = np.zeros(0, dtype=np.int64)  # an empty row
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return ptr, np.concatenate(rows).astype(np.int64)


# per-half widths: float4 rows at 1, 2 and 4 groups per lane; float2 rows at 1 and 4; dword rows at 1 and 4
WIDTHS = (16, 300, 1000, 50, 450, 33, 255)


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("name", FNS)
def test_every_instance(name, d):
    E, R, B = 300, 7, 17
    m = make_model(name, E, R, d, 12.0)
    g = np.random.RandomState(E + d)
    pos = dev(queries(g, E, R, B))
    ptr, ids = random_exclude(g, E, B)
    xp, xi = dev(ptr), dev(ids)
    for mode in MODES:
        S = evaluate.score_all(m, pos, mode)
        Sc = S.cpu()
        for k in (1, 10, 64):
            want = reference(Sc, k, ptr, ids)
            got = evaluate.topk_sweep(m, pos, mode, k, xp, xi)
            assert got is not None
            assert same(got, want), (name, d, mode, k, "sweep")
            assert same(evaluate.topk_rows(S, k, xp, xi), want), (name, d, mode, k, "rows")
        want = reference(Sc, 10)
        assert same(evaluate.topk_sweep(m, pos, mode, 10), want), (name, d, mode, "sweep, no exclusion")
        assert same(evaluate.topk_rows(S, 10), want), (name, d, mode, "rows, no exclusion")


@pytest.mark.parametrize("d", [16, 64])
@pytest.mark.parametrize("name", ["DistMult", "ComplEx", "TranSparse"])
def test_matrix_path(name, d):
    """topk_rows on score_all's matrix for the functions the sweep has no kernel for (TranSparse: head-batch), and
    on a padded matrix into padded outputs: nothing outside [M, k] of the outputs is written."""
    E, R, B, k = 300, 5, 17, 10
    m = make_model(name, E, R, d, 12.0)
    g = np.random.RandomState(d)
    pos = dev(queries(g, E, R, B))
    ptr, ids = random_exclude(g, E, B)
    xp, xi = dev(ptr), dev(ids)
    assert evaluate.topk_sweep(m, pos, "head-batch", k) is None
    for mode in (("head-batch",) if name == "TranSparse" else MODES):
        S = evaluate.score_all(m, pos, mode, planes=evaluate.entity_planes(m))
        want = reference(S, k, ptr, ids)
        assert same(evaluate.topk_rows(S, k, xp, xi), want), (name, d, mode)
        pad = torch.full((B, E + 5), 1e30, device=DEV)  # a canary no column beats
        pad[:, :E] = S
        oi = torch.full((B, k + 3), -7, dtype=torch.int64, device=DEV)
        os_ = torch.full((B, k + 2), -7.0, device=DEV)
        evaluate.topk_rows(pad[:, :E], k, xp, xi, out_ids=oi[:, :k], out_scores=os_[:, :k])
        assert same((oi[:, :k], os_[:, :k]), want), (name, d, mode, "padded")
        assert bool((oi[:, k:] == -7).all()) and bool((os_[:, k:] == -7.0).all())
        assert same(m.predict(pos.cpu().numpy(), mode, k=k), reference(S, k)), (name, d, mode, "predict")


ALL = ("TransE", "DistMult", "ComplEx", "RotatE", "pRotatE", "InterHT", "TranSparse")


@pytest.mark.parametrize("name", ALL)
def test_against_fp64_oracle(name):
    """Every returned score within the bar of the fp64 oracle's score of that id, and every returned id's oracle
    score at least the oracle's k-th best valid score minus twice the bar."""
    E, R, d, B, k, gamma = 200, 5, 64, 8, 10, 12.0
    m = make_model(name, E, R, d, gamma)
    g = np.random.RandomState(11)
    q = queries(g, E, R, B)
    pos = dev(q)
    ptr, ids = random_exclude(g, E, B)
    ent, rel = m.entity_embedding.detach().cpu().double(), m.relation_embedding.detach().cpu().double()
    cand = torch.arange(E).unsqueeze(0).expand(B, E)
    for mode in (("head-batch",) if name == "TranSparse" else MODES):
        if name == "TranSparse":
            ref = O.transparse_score(ent, rel, m.W.detach().cpu().double(), m.mask.cpu().double(), torch.from_numpy(q),
                                     cand, mode, gamma)
        else:
            mod = float(m.modulus.detach().reshape(-1)[0]) if name == "pRotatE" else None
            ref = O.score(name, ent, rel, torch.from_numpy(q), cand, mode, gamma, m._range_f, mod)
        S = evaluate.score_all(m, pos, mode)
        results = [evaluate.topk_rows(S, k, dev(ptr), dev(ids)),
                   evaluate.predict(m, q, mode, k=k, known_triples=None)]
        if name in FNS:
            results.append(evaluate.topk_sweep(m, pos, mode, k, dev(ptr), dev(ids)))
        for ri, (gi, gs) in enumerate(results):
            gi, gs = gi.cpu(), gs.cpu().double()
            excluded = ri != 1
            for b in range(B):
                valid = torch.ones(E, dtype=torch.bool)
                if excluded:
                    valid[torch.from_numpy(ids[ptr[b]:ptr[b + 1]])] = False
                assert bool((gi[b] >= 0).all()) and bool(valid[gi[b]].all()) and len(set(gi[b].tolist())) == k
                r = ref[b][gi[b]]
                bar = 1e-4 * r.abs().clamp_min(1.0)
                assert bool(((gs[b] - r).abs() <= bar).all()), (name, mode, ri, b)
                kth = torch.sort(ref[b][valid], descending=True).values[k - 1]
                assert bool((r >= kth - 2 * 1e-4 * max(1.0, abs(float(kth)))).all()), (name, mode, ri, b)


@pytest.mark.parametrize("E", [1, 5, 8, 9, 64, 65])
@pytest.mark.parametrize("name", ["TransE", "InterHT"])
def test_edges(name, E):
    """Empty entity slices, one row per slice, chunk boundaries, fewer entities than k (padding); one query row, a
    full and a short row group; exclusion lists that are empty, hold every entity, or hold ids outside [0, E);
    query ids out of range (a zero row, as everywhere else)."""
    R, d, k = 3, 20, 10
    m = make_model(name, E, R, d, 9.0)
    g = np.random.RandomState(E)
    for B in (1, 16, 17):
        q = queries(g, E, R, B)
        q[B - 1] = (E + 3, R, -1)  # out-of-range query ids
        pos = dev(q)
        lists = {
            "random": random_exclude(g, E, B, most=min(E, 4)),
            "outside": random_exclude(g, E, B, most=min(E, 4), extra=(-3, E, 10 ** 9)),
            "all": (np.arange(B + 1, dtype=np.int64) * E, np.tile(np.arange(E, dtype=np.int64), B)),
            "empty": (np.zeros(B + 1, dtype=np.int64), np.zeros(0, dtype=np.int64)),
        }
        for mode in MODES:
            S = evaluate.score_all(m, pos, mode)
            Sc = S.cpu()
            for tag, (ptr, ids) in lists.items():
                want = reference(Sc, k, ptr, ids)
                if tag == "all":
                    assert bool((want[0] == -1).all()) and bool(torch.isinf(want[1]).all())
                if tag == "outside":  # the same rows without the ids outside [0, E)
                    assert int((ids < 0).sum()) + int((ids >= E).sum()) >= 3 * (B - 1)
                xp, xi = dev(ptr), (dev(ids) if len(ids) else None)
                assert same(evaluate.topk_sweep(m, pos, mode, k, xp, xi), want), (name, E, B, mode, tag, "sweep")
                assert same(evaluate.topk_rows(S, k, xp, xi), want), (name, E, B, mode, tag, "rows")
            if E < k:
                assert bool((want[0][:, E:] == -1).all())


def test_ties_come_out_by_ascending_id():
    E, R, d, B, k = 120, 3, 24, 5, 10
    m = make_model("TransE", E, R, d, 9.0)
    pos = dev(np.array([[2, 1, 9], [9, 0, 5], [7, 2, 7], [50, 1, 60], [3, 0, 40]]))
    with torch.no_grad():
        # tail-batch query 0 is (2, 1, ?): the entity e_2 + r_1, written to row 7 and its copies 3, 40 and 41, is
        # at distance 0; head-batch query 1 is (?, 0, 5) with e_5 = that row + r_0: the same four rows lead there
        best = (m.entity_embedding[2] + m.relation_embedding[1]).clone()
        for e in (7, 3, 40, 41):
            m.entity_embedding[e] = best
        m.entity_embedding[5] = best + m.relation_embedding[0]
    for mode in MODES:
        S = evaluate.score_all(m, pos, mode)
        want = reference(S, k)
        got = evaluate.topk_sweep(m, pos, mode, k)
        assert same(got, want) and same(evaluate.topk_rows(S, k), want), mode
        # the four equal rows are adjacent in every result, in ascending id
        for b in range(B):
            row = got[0][b].tolist()
            if 3 in row and 41 in row:
                assert row[row.index(3):row.index(3) + 4] == [3, 7, 40, 41], (mode, b, row)
    for mode, b in (("tail-batch", 0), ("head-batch", 1)):
        ids, scores = evaluate.topk_sweep(m, pos, mode, k)
        assert ids[b, :4].tolist() == [3, 7, 40, 41] and len(set(scores[b, :4].tolist())) == 1, (mode, ids[b])
    with torch.no_grad():
        m.entity_embedding[:] = m.entity_embedding[0].clone()
    for mode in MODES:
        ids, scores = evaluate.topk_sweep(m, pos, mode, k)
        assert ids.tolist() == [list(range(k))] * B and bool((scores == scores[:, :1]).all())
        ids, _ = evaluate.topk_rows(evaluate.score_all(m, pos, mode), k)
        assert ids.tolist() == [list(range(k))] * B


def test_interht_nan_rows():
    """Q7: a zero entity row scores NaN under InterHT. Those ids never appear, and a query whose own row is zero
    (every score NaN) returns all padding."""
    E, R, d, B, k = 100, 4, 16, 12, 10
    zeros = (7, 31, 64)
    m = make_model("InterHT", E, R, d, 9.0)
    with torch.no_grad():
        for z in zeros:
            m.entity_embedding[z].zero_()
    g = np.random.RandomState(1)
    others = np.array([e for e in range(E) if e not in zeros])
    q = np.stack([g.choice(others, size=B), g.randint(R, size=B), g.choice(others, size=B)], 1)
    q[2] = (7, 1, 7)  # the query's own row is zero in both modes
    pos = dev(q)
    for mode in MODES:
        S = evaluate.score_all(m, pos, mode)
        assert bool(torch.isnan(S[:, list(zeros)]).all()) and bool(torch.isnan(S[2]).all())
        want = reference(S, k)
        for got in (evaluate.topk_sweep(m, pos, mode, k), evaluate.topk_rows(S, k)):
            assert same(got, want), mode
            assert not any(z in got[0].tolist()[b] for z in zeros for b in range(B))
            assert got[0][2].tolist() == [-1] * k and bool(torch.isinf(got[1][2]).all())
            assert bool((got[0][[0, 1, 3]] >= 0).all())


@pytest.mark.parametrize("name", ["RotatE", "InterHT"])
def test_result_does_not_depend_on_the_decomposition(name):
    """A query alone (B = 1: one short group, the most chunks per slice) gives its row of a batch of 40 and of a
    batch of 300 (more groups, other chunk counts)."""
    E, R, d, k = 1500, 6, 64, 10
    m = make_model(name, E, R, d, 9.0)
    g = np.random.RandomState(4)
    q = queries(g, E, R, 300)
    ptr, ids = random_exclude(g, E, 300)
    for mode in MODES:
        big = evaluate.topk_sweep(m, dev(q), mode, k, dev(ptr), dev(ids))
        big = (big[0].cpu(), big[1].cpu())
        assert same(big, reference(evaluate.score_all(m, dev(q), mode), k, ptr, ids))
        mid = evaluate.topk_sweep(m, dev(q[:40]), mode, k, dev(ptr[:41]), dev(ids[:ptr[40]]))
        assert same(mid, (big[0][:40], big[1][:40])), (name, mode, 40)
        for b in (1, 17, 39):
            one = evaluate.topk_sweep(m, dev(q[b:b + 1]), mode, k, dev(ptr[b:b + 2] - ptr[b]),
                                      dev(ids[ptr[b]:ptr[b + 1]]) if ptr[b + 1] > ptr[b] else None)
            assert same(one, (big[0][b:b + 1], big[1][b:b + 1])), (name, mode, b)


def test_determinism_and_workspace_content():
    E, R, d, B, k = 700, 5, 48, 33, 64
    m = make_model("RotatE", E, R, d, 9.0)
    g = np.random.RandomState(6)
    pos = dev(queries(g, E, R, B))
    ptr, ids = random_exclude(g, E, B)
    xp, xi = dev(ptr), dev(ids)
    for mode in MODES:
        a = evaluate.topk_sweep(m, pos, mode, k, xp, xi)
        b = evaluate.topk_sweep(m, pos, mode, k, xp, xi)
        assert same(b, (a[0].cpu(), a[1].cpu()))
        (ws,) = evaluate._TOPK_WS.values()
        ws.fill_(0xFF)
        c = evaluate.topk_sweep(m, pos, mode, k, xp, xi)
        assert same(c, (a[0].cpu(), a[1].cpu()))
        S = evaluate.score_all(m, pos, mode)
        assert same(evaluate.topk_rows(S, k, xp, xi), (a[0].cpu(), a[1].cpu()))


def test_graph_capture_replays_equal():
    E, R, d, B, k = 900, 5, 64, 24, 10
    m = make_model("InterHT", E, R, d, 9.0)
    g = np.random.RandomState(9)
    pos = dev(queries(g, E, R, B))
    ptr, ids = random_exclude(g, E, B)
    xp, xi, nx = dev(ptr), dev(ids), len(ids)
    S = evaluate.score_all(m, pos, "tail-batch")

    def call():
        a = evaluate.topk_sweep(m, pos, "tail-batch", k, xp, xi, nx)
        b = evaluate.topk_rows(S, k)
        return a, b

    (wa, wb) = call()
    want_a, want_b = (wa[0].cpu(), wa[1].cpu()), (wb[0].cpu(), wb[1].cpu())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()  # warm-up on a side stream before capture, as torch.cuda.graph expects
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ga, gb = call()
    graph.replay()
    torch.cuda.synchronize()
    assert same(ga, want_a) and same(gb, want_b)


def test_full_size_wn18rr_interht():
    """WN18RR InterHT d 1 000 (-de -tr), E 40 943: 32 queries, k = 10, exclusion from the dataset's triples."""
    z = np.load(os.path.join(GOLDEN, "wn18rr_ids.npz"))
    triples, E, R = z["triples"].astype(np.int64), int(z["nentity"]), int(z["nrelation"])
    m = make_model("InterHT", E, R, 1000, 24.0, seed=0)
    q = triples[::len(triples) // 32][:32]
    pos = dev(q)
    for mode in MODES:
        ptr, ids = evaluate.build_exclude(q, mode, triples)
        assert len(ids) >= len(q)  # every query's own answer is listed
        want = reference(evaluate.score_all(m, pos, mode), 10, ptr, ids)
        got = evaluate.topk_sweep(m, pos, mode, 10, dev(ptr), dev(ids), len(ids))
        assert got is not None and same(got, want), mode
        col = 0 if mode == "head-batch" else 2
        assert not any(int(q[b, col]) in got[0][b].tolist() for b in range(len(q)))


@pytest.mark.parametrize("name", ["RotatE", "DistMult"])
def test_predict(name, monkeypatch):
    E, R, d, M, k, bs = 400, 6, 32, 75, 10, 32
    m = make_model(name, E, R, d, 9.0)
    g = np.random.RandomState(3)
    known = queries(g, E, R, 900)
    known[100:300, :2] = known[0, :2]  # a hub (h, r): a long exclusion row
    q = known[:M].copy()
    for mode in MODES:
        ptr, ids = evaluate.build_exclude(q, mode, known)
        want_i, want_s = [], []
        for s in range(0, M, bs):  # the per-batch reference
            S = evaluate.score_all(m, dev(q[s:s + bs]), mode, planes=evaluate.entity_planes(m))
            p = ptr[s:s + bs + 1]
            wi, ws = reference(S, k, p - p[0], ids[p[0]:p[-1]])
            want_i.append(wi)
            want_s.append(ws)
        want = (torch.cat(want_i), torch.cat(want_s))
        got = evaluate.predict(m, q, mode, k=k, known_triples=known, batch_size=bs)
        assert got[0].shape == (M, k) and got[0].dtype == torch.int64 and got[0].device.type == "cuda"
        assert same(got, want), (name, mode)
        col = 0 if mode == "head-batch" else 2
        assert not any(int(q[b, col]) in got[0][b].tolist() for b in range(M))  # the known answer is left out
        # the candidate slot of a query is ignored
        q2 = q.copy()
        q2[:, col] = 0
        assert same(evaluate.predict(m, torch.from_numpy(q2), mode, k=k, known_triples=known, batch_size=bs), want)
        assert same(m.predict(q, mode, k=k, known_triples=known, batch_size=bs), want)
        with monkeypatch.context() as mp:  # the matrix path for every batch
            mp.setattr(evaluate, "topk_sweep", lambda *a, **kw: None)
            fb = evaluate.predict(m, q, mode, k=k, known_triples=known, batch_size=bs)
        assert torch.equal(fb[0], got[0]) and same(fb, want)
        free = evaluate.predict(m, q, mode, k=k, batch_size=M)  # nothing known: one batch, no exclusion
        assert same(free, reference(evaluate.score_all(m, dev(q), mode, planes=evaluate.entity_planes(m)), k))
    with pytest.raises(ValueError, match="k must be"):
        evaluate.predict(m, q, "tail-batch", k=65)
    with pytest.raises(ValueError, match="k must be"):
        m.predict(q, "tail-batch", k=0)
