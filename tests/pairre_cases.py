"""Seeded PairRE cases shared by tests/test_pairre_*: tables, batches and the evaluation cases (fp64 scores of every
entity, truths no score within the bar can move, filter lists with tests/sweep_cases.py's edge rows). A plain
module, as tests/sweep_cases.py is; the references come from tests/pairre_ref.py and are never modified."""
import functools
import types

import numpy as np
import torch

from oracle import kge_oracle as O
from tests import eval_cases as C
from tests import pairre_ref as P
from tests import sweep_cases as W

NAME, FN = "PairRE", 7
GAMMA = 12.0
TOL = 1e-4  # the project's score bar: |fp32 - fp64| <= TOL * max(1, |fp64|)
E_EVAL, R_EVAL, B_EVAL = 523, 7, 40
MODES = ((0, "head-batch"), (1, "tail-batch"))


@functools.lru_cache(maxsize=None)
def case(D, E, R, B, N, seed=0, oor=False):
    """CPU fp32 tables (entity rows D wide from O.make_tables' initialiser, relation rows 2 D wide drawn from
    U(-1, 1) so that the scores of different candidates spread), a [B, 3] positive batch, [B, N] candidates and
    weights in [0.2, 1]. oor: ids -1 and E among the negatives, heads and tails (B >= 4, N >= 4)."""
    ent, rel, rng = O.make_tables(E, R, D, 2 * D, GAMMA, D, seed=seed)
    rel = rel / rng
    g = np.random.RandomState(seed + 1)
    pos = torch.from_numpy(np.stack([g.randint(E, size=B), g.randint(R, size=B), g.randint(E, size=B)], 1))
    neg = torch.from_numpy(g.randint(E, size=(B, N)))
    w = torch.from_numpy(g.uniform(0.2, 1.0, size=(B,))).float()
    if oor:
        neg[0, 1], neg[1, 2], neg[B - 1, N - 1] = -1, E, E
        pos[1, 0], pos[2, 2], pos[3, 0], pos[3, 2] = -1, E, E, -1
    return types.SimpleNamespace(name=NAME, D=D, E=E, R=R, B=B, N=N, ent=ent, rel=rel, rng=rng, pos=pos, neg=neg, w=w,
                                 gamma=GAMMA)


def bar(ref):
    return TOL * np.maximum(1.0, np.abs(ref))


def within_bar(got, ref):
    """Whether every fp32 score is within the bar of its fp64 value (both finite)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool(np.isfinite(got).all() and (np.abs(got - ref) <= bar(ref)).all())


# ------------------------------------------------------------------------------------------------
# evaluation cases (E 523, B 40): the dict layout of strided.make_case, which sweep_cases' raw callers take
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def eval_case(d):
    c = case(d, E_EVAL, R_EVAL, B_EVAL, 1, seed=d)
    return dict(name=NAME, D=d, E=c.E, R=c.R, B=c.B, N=1, ent=c.ent, rel=c.rel, pos=c.pos, neg=c.neg, w=c.w,
                gamma=GAMMA, rng=c.rng, mod=0.0)


@functools.lru_cache(maxsize=None)
def ref_scores(d, mode):
    c = eval_case(d)
    out = P.score_all(c["ent"].double(), c["rel"].double(), c["pos"], mode, GAMMA).numpy()
    assert out.shape == (B_EVAL, E_EVAL) and np.isfinite(out).all()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def truths(d, mode):
    """(truth [B], isolated candidates per row [B]): per query row the isolated candidate (sweep_cases.isolated:
    no other score within twice the sum of the bars) whose fp64 rank is nearest to sweep_cases.targets()[row]. Every
    row must have one: no row is left out. Rows ROW_MINUS1 / ROW_E then get the out-of-range truths -1 / E."""
    ref, want = ref_scores(d, mode), W.targets()
    truth, count = np.empty(B_EVAL, dtype=np.int64), np.empty(B_EVAL, dtype=np.int64)
    for q in range(B_EVAL):
        iso = W.isolated(ref[q])
        count[q] = int(iso.sum())
        assert count[q] > 0, (d, mode, q, "no isolated candidate")
        rank = 1 + (ref[q][None, :] > ref[q][:, None]).sum(axis=1)
        ids = np.nonzero(iso)[0]
        truth[q] = ids[np.argmin(np.abs(rank[ids] - want[q]))]
    truth[W.ROW_MINUS1], truth[W.ROW_E] = -1, E_EVAL
    truth.setflags(write=False)
    return truth, count


@functools.lru_cache(maxsize=None)
def filters(d, mode):
    """sweep_cases.filters' lists for these cases: distinct ascending ids per row, the edge rows included."""
    truth, _ = truths(d, mode)
    g = np.random.RandomState(1000 * d + 70 + mode)
    E = E_EVAL
    rows = [np.unique(g.randint(E, size=g.randint(1, 13))) for _ in range(B_EVAL)]
    rows[W.ROW_EMPTY] = np.zeros(0, dtype=np.int64)
    rows[W.ROW_LONG] = np.sort(g.choice(E, size=90, replace=False))
    rows[W.ROW_TRUTH] = np.union1d(rows[W.ROW_TRUTH], [truth[W.ROW_TRUTH]])
    rows[W.ROW_OUTSIDE] = np.concatenate([[-1], rows[W.ROW_OUTSIDE], [E]])
    rows[W.ROW_ALL] = np.arange(E)
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    ids = np.concatenate(rows).astype(np.int64)
    ptr.setflags(write=False)
    ids.setflags(write=False)
    return ptr, ids


@functools.lru_cache(maxsize=None)
def expected_ranks(d, mode, filtered=True):
    truth, _ = truths(d, mode)
    ptr, ids = filters(d, mode) if filtered else (None, None)
    return C.rank_ref(ref_scores(d, mode), truth, ptr, ids)


@functools.lru_cache(maxsize=None)
def candidate_lists(d, mode, n=100):
    """[B, n] candidate ids per query row for kge_eval_rank_candidates: random entities whose fp64 score is isolated
    from the truth's (more than twice the sum of the bars away, so the count above the truth cannot move and no
    tie can appear), then, overwriting the row's first places, the truth itself, an id of the row's filter list and
    the out-of-range ids -1 and E, none of which is counted. Returns (lists, ranks [B], ties [B]) by the header's
    rule on the fp64 scores: rank = 1 + counted entries above the truth; an out-of-range truth scores -inf."""
    ref, (truth, _), (ptr, ids) = ref_scores(d, mode), truths(d, mode), filters(d, mode)
    g = np.random.RandomState(77 * d + mode)
    E = E_EVAL
    lists = np.empty((B_EVAL, n), dtype=np.int64)
    ranks, ties = np.empty(B_EVAL, dtype=np.int64), np.zeros(B_EVAL, dtype=np.int64)
    b = bar(ref)
    for q in range(B_EVAL):
        tr = int(truth[q])
        if 0 <= tr < E:
            far = np.abs(ref[q] - ref[q, tr]) > 2.0 * (b[q] + b[q, tr])
            far[tr] = False
            ts = ref[q, tr]
        else:
            far, ts = np.ones(E, dtype=bool), -np.inf
        pool = np.nonzero(far)[0]
        assert len(pool) >= 8, (d, mode, q)
        lists[q] = g.choice(pool, size=n, replace=True)
        f = ids[ptr[q]:ptr[q + 1]]
        lists[q, 0], lists[q, 1], lists[q, 2] = (tr if 0 <= tr < E else -1), -1, E
        if len(f):
            lists[q, 3] = f[len(f) // 2]
        counted = np.array([0 <= e < E and e != tr and e not in set(f.tolist()) for e in lists[q]])
        sc = np.where(counted, ref[q, np.clip(lists[q], 0, E - 1)], -np.inf)
        ranks[q] = 1 + int((counted & (sc > ts)).sum())
    lists.setflags(write=False)
    return lists, ranks, ties
