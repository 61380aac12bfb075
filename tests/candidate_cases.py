"""Helpers of the candidate-list rank tests (test_rank_candidates_gpu.py, test_candidate_cases_cpu.py):
kge_eval_rank_candidates against a reference written from include/kge_hip.h and the fp64 oracle, not from the
kernel. The seeded cases reuse tests/sweep_cases.py's shape (E = 523, R = 7, B = 40, gamma 12), score bar, isolation
rule, rank targets and layouts, and tests/strided.py's tables, views and width rule. One per-half width per kernel
instance (V, G) in {4, 2, 1} x {1, 2, 4, 8}, all six score functions.

What differs from the sweep's cases, and why:
  * DistMult / ComplEx tables are scaled by the fp32 factor cbrt(4 / max |fp64 score|) of the unscaled case. Their
    scores are trilinear in the tables and shrink with the width (|s| about 1e-4 at d 1000), while the bar is
    absolute below 1, so unscaled no entity is isolated at d >= 450. Scaled, the largest |score| is 4.
  * Exact ties are planted: the truth's table row of each query row in TIE_ROWS is copied onto NCOPY other entity
    ids, so the copies score bitwise what the truth scores, on any evaluation, and the row's list holds them. A copy
    is by construction not isolated from its source; it is left out of the rank bounds (its difference to the truth
    is exactly 0 on every evaluation) and counted in the expected ties. The truths differ per mode, so the tables of
    a case do too.
  * Every other truth is an entity isolated from ALL others (sweep_cases.isolated), every tie row's truth one
    isolated from all others but its own copies: then above(q) is the only value an evaluation within the score bar
    can return, for every row.
A plain module: nothing here is a fixture or changes how the suite is collected."""
import functools

import numpy as np
import torch

from oracle import kge_oracle as O
from tests import strided as S
from tests import sweep_cases as SC

FNS = tuple(S.FNS)  # TransE, DistMult, ComplEx, RotatE, pRotatE, InterHT
SCALED = ("DistMult", "ComplEx")
E, R, B, GAMMA, TOL = SC.E, SC.R, SC.B, SC.GAMMA, SC.TOL
C = 500
MODES = SC.MODES
# per-half widths, one per (V, G): V4 G1/2/4/8, V2 G1/2/4/8, V1 G1/2/4/8
WIDTHS = (16, 264, 1000, 2000, 50, 130, 450, 902, 33, 99, 255, 511)
VG = tuple((v, g) for v in (4, 2, 1) for g in (1, 2, 4, 8))
LAYOUTS = ("dense", "pad4", "pad2", "pad1", "off1", "off2")
# query rows with a purpose. Truths: ROW_MINUS1 / ROW_E are out of range. Filters (sweep_cases.filters' rows): empty,
# more than 64 ids, holding the truth, holding -1 and E, every entity. Lists: padding at both ends and in the middle,
# the truth's own id twice, nothing but padding, one id 70 times.
ROW_MINUS1, ROW_E = SC.ROW_MINUS1, SC.ROW_E
ROW_EMPTY, ROW_LONG, ROW_TRUTH, ROW_OUTSIDE, ROW_ALL = SC.ROW_EMPTY, SC.ROW_LONG, SC.ROW_TRUTH, SC.ROW_OUTSIDE, SC.ROW_ALL
ROW_PAD, ROW_OWN, ROW_ALLPAD, ROW_SAME = 7, 8, 9, 10
TIE_ROWS = tuple(range(11, 19))
ROW_TIE_FILTERED = TIE_ROWS[0]  # its filter holds one of the truth's copies: that copy's entries are not counted
NCOPY = 2  # copies of each tie row's truth
FAR = 1 << 40  # an id far outside the table


def dense_vg(name, d):
    """(V, G) of dense, 16-B aligned tables (strided.expected_vg on their row widths and relation offset)."""
    em, rm = S.MULT[name]
    return S.expected_vg(d, lds=(em * d, rm * d), offs=(S.rel_off(name, d),))


def _fp64_scores(c, mode):
    ent, rel = c["ent"].double(), c["rel"].double()
    rows = []
    for s in range(0, B, 8):  # a few query rows at a time: the gathered candidates of d = 2000 are large
        pos = c["pos"][s:s + 8]
        cand = torch.arange(E).unsqueeze(0).expand(len(pos), E)
        rows.append(O.score(c["name"], ent, rel, pos, cand, mode, c["gamma"], c["rng"], c["mod"]))
    out = torch.cat(rows).numpy()
    assert out.shape == (B, E) and np.isfinite(out).all()
    return out


@functools.lru_cache(maxsize=None)
def scale_factor(name, d):
    """1 for the distance functions; DistMult / ComplEx: fp32 cbrt(4 / max |fp64 score|) of the unscaled case."""
    if name not in SCALED:
        return np.float32(1.0)
    c = S.make_case(name, d, E=E, R=R, B=B, N=1, seed=d, gamma=GAMMA)
    m = max(float(np.abs(_fp64_scores(c, mode)).max()) for mode, _ in MODES)
    return np.float32(np.cbrt(4.0 / m))


@functools.lru_cache(maxsize=None)
def base(name, d):
    """sweep_cases.case's seeded tables and batch (strided.make_case, seed d), scaled for DistMult / ComplEx; no
    copies yet."""
    c = dict(S.make_case(name, d, E=E, R=R, B=B, N=1, seed=d, gamma=GAMMA))
    f = float(scale_factor(name, d))
    if f != 1.0:
        c["ent"], c["rel"] = c["ent"] * f, c["rel"] * f
    return c


@functools.lru_cache(maxsize=None)
def _base_scores(name, d, mode):
    return _fp64_scores(base(name, d), mode)


def _nearest(row, ids, want):
    """The id among ids whose unfiltered fp64 rank in the score row is nearest want."""
    rank = 1 + (row[None, :] > row[ids, None]).sum(axis=1)
    return int(ids[int(np.argmin(np.abs(rank - want)))])


@functools.lru_cache(maxsize=None)
def tie_plan(name, d, mode):
    """{tie row q: (source id, its NCOPY copies' ids)}. The source is the entity of the base tables that is isolated
    from every other in row q's fp64 scores (sweep_cases.isolated) and nearest the row's target rank, distinct over
    the tie rows. The copies' ids are drawn from the entities that are no query's head or tail (a copy there would
    change a query, so every score of its row) and no source. The distance functions isolate few entities at the
    large widths (pRotatE d 2000: two of 523 in some rows), so the sources are chosen per row, and the tables of a
    case differ per mode."""
    ref0, want = _base_scores(name, d, mode), SC.targets()
    pos = base(name, d)["pos"].numpy()
    src = {}
    for q in TIE_ROWS:
        iso = SC.isolated(ref0[q])
        iso[list(src.values())] = False
        assert iso.any(), (name, d, mode, q, "no isolated source")
        src[q] = _nearest(ref0[q], np.nonzero(iso)[0], want[q])
    free = np.ones(E, dtype=bool)
    free[pos[:, 0]] = free[pos[:, 2]] = False
    free[list(src.values())] = False
    g = np.random.RandomState(7700 + _seed(name, d, mode))
    ids = g.permutation(np.nonzero(free)[0])[:NCOPY * len(TIE_ROWS)].reshape(len(TIE_ROWS), NCOPY)
    return {q: (src[q], ids[i].copy()) for i, q in enumerate(TIE_ROWS)}


@functools.lru_cache(maxsize=None)
def case(name, d, mode):
    """base()'s tables with tie_plan's copies planted: the rows of a source's copies hold the source's row."""
    c = dict(base(name, d))
    ent = c["ent"].clone()
    for s, cp in tie_plan(name, d, mode).values():
        ent[torch.from_numpy(cp)] = ent[s].clone()
    c["ent"] = ent
    return c


@functools.lru_cache(maxsize=None)
def ref_scores(name, d, mode):
    """fp64 scores [B, E] of every entity of case()'s tables as the candidate (O.score on the fp32 tables' values),
    as numpy. A copy's column is its source's column of the base tables' scores: the same operands through the same
    arithmetic, and no query reads a copy's row (test_candidate_cases_cpu.py recomputes one case in full)."""
    out = _base_scores(name, d, mode).copy()
    for s, cp in tie_plan(name, d, mode).values():
        out[:, cp] = out[:, [s]]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def truths(name, d, mode):
    """(truth [B] int64, isolated candidates per row [B]). Rows outside TIE_ROWS: the entity isolated from every
    other (sweep_cases.isolated, on the tables with the copies) whose fp64 rank is nearest sweep_cases.targets()[row].
    TIE_ROWS: tie_plan's source, isolated from every entity but its own copies. ROW_MINUS1 / ROW_E: -1 and E."""
    ref, want, plan = ref_scores(name, d, mode), SC.targets(), tie_plan(name, d, mode)
    truth, count = np.empty(B, dtype=np.int64), np.empty(B, dtype=np.int64)
    for q in range(B):
        row = ref[q]
        iso = SC.isolated(row)
        count[q] = int(iso.sum())
        if q in plan:
            s, cp = plan[q]
            other, b = np.ones(E, dtype=bool), SC.bar(row)
            other[[s, *cp]] = False
            assert (row[cp] == row[s]).all()
            assert (np.abs(row[other] - row[s]) > 2.0 * (b[other] + b[s])).all(), (name, d, mode, q)
            truth[q] = s
        else:
            assert count[q] > 0, (name, d, mode, q, "no isolated candidate")
            truth[q] = _nearest(row, np.nonzero(iso)[0], want[q])
    truth[ROW_MINUS1], truth[ROW_E] = -1, E
    truth.setflags(write=False)
    return truth, count


def _seed(name, d, mode):
    return 1000 * d + 10 * FNS.index(name) + mode


@functools.lru_cache(maxsize=None)
def lists(name, d, mode):
    """[B, C] int64: per row C draws with repeats from [0, E), then the edge rows and the tie rows' copies."""
    truth, _ = truths(name, d, mode)
    plan = tie_plan(name, d, mode)
    g = np.random.RandomState(_seed(name, d, mode) + 1)
    L = g.randint(E, size=(B, C)).astype(np.int64)
    L[ROW_PAD, :3], L[ROW_PAD, -2:] = (-1, E, -1), (E, -1)
    L[ROW_PAD, 200:230:3], L[ROW_PAD, 231], L[ROW_PAD, 232], L[ROW_PAD, 233] = -1, E, FAR, -FAR
    L[ROW_OWN, 17] = L[ROW_OWN, 401] = truth[ROW_OWN]
    L[ROW_ALLPAD] = np.resize(np.array([-1, E, E + 5, FAR, -7, -FAR], dtype=np.int64), C)
    L[ROW_SAME] = -1
    L[ROW_SAME, 100:170] = (truth[ROW_SAME] + 1 + g.randint(E - 1)) % E  # one id, not the truth, 70 times
    for q in TIE_ROWS:
        a, b = plan[q][1]
        L[q, 3 + q], L[q, 64 + q], L[q, C - 1 - q] = a, a, b
    L.setflags(write=False)
    return L


@functools.lru_cache(maxsize=None)
def filters(name, d, mode):
    """(ptr [B + 1], ids): sweep_cases.filters' lists for these truths (distinct ascending ids per row; ROW_EMPTY
    empty, ROW_LONG 90 ids, ROW_TRUTH holds the truth, ROW_OUTSIDE holds -1 and E, ROW_ALL every entity, the rest
    random subsets of up to 12 ids), and ROW_TIE_FILTERED's holds the first copy of its truth."""
    truth, _ = truths(name, d, mode)
    plan = tie_plan(name, d, mode)
    g = np.random.RandomState(_seed(name, d, mode))
    rows = [np.unique(g.randint(E, size=g.randint(1, 13))) for _ in range(B)]
    rows[ROW_EMPTY] = np.zeros(0, dtype=np.int64)
    rows[ROW_LONG] = np.sort(g.choice(E, size=90, replace=False))
    rows[ROW_TRUTH] = np.union1d(rows[ROW_TRUTH], [truth[ROW_TRUTH]])
    rows[ROW_OUTSIDE] = np.concatenate([[-1], rows[ROW_OUTSIDE], [E]])
    rows[ROW_ALL] = np.arange(E)
    for q in TIE_ROWS:  # no copy of a tie row's truth by accident; one on purpose
        rows[q] = np.setdiff1d(rows[q], plan[q][1])
    rows[ROW_TIE_FILTERED] = np.union1d(rows[ROW_TIE_FILTERED], [plan[ROW_TIE_FILTERED][1][0]])
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    ids = np.concatenate(rows).astype(np.int64)
    for q in range(B):
        assert (np.diff(ids[ptr[q]:ptr[q + 1]]) > 0).all()
    ptr.setflags(write=False)
    ids.setflags(write=False)
    return ptr, ids


# ------------------------------------------------------------------------------------------------
# the header's semantics, restated
# ------------------------------------------------------------------------------------------------
def counted(lst, tr, n_ent, flt=None):
    """Which entries of one list are counted: an id in [0, n_ent), not the truth, not in the row's filter."""
    lst = np.asarray(lst, dtype=np.int64)
    keep = (lst >= 0) & (lst < n_ent) & (lst != tr)
    if flt is not None and len(flt):
        keep &= ~np.isin(lst, flt)
    return keep


def reference(scores, truth, L, ptr=None, ids=None):
    """(ranks, ties, truth scores) of include/kge_hip.h's kge_eval_rank_candidates on a score table: scores[q, e] is
    the score of entity e as row q's candidate (any float type; IEEE comparisons), L [M, C] or [C] (shared)."""
    A = np.asarray(scores)
    M, n_ent = A.shape
    L = np.asarray(L, dtype=np.int64)
    ranks, ties = np.empty(M, dtype=np.int64), np.empty(M, dtype=np.int64)
    ts = np.empty(M, dtype=A.dtype)
    with np.errstate(invalid="ignore"):
        for q in range(M):
            tr = int(truth[q])
            ts[q] = A[q, tr] if 0 <= tr < n_ent else -np.inf
            lst = L if L.ndim == 1 else L[q]
            keep = counted(lst, tr, n_ent, None if ptr is None else ids[int(ptr[q]):int(ptr[q + 1])])
            s = A[q, np.where(keep, lst, 0)]
            ranks[q] = 1 + int((keep & (s > ts[q])).sum())
            ties[q] = int((keep & (s == ts[q])).sum())
    return ranks, ties, ts


def bounds(ref, truth, L, ptr=None, ids=None, twins=None):
    """(lo, hi) of above(q) + 1 under a perturbation of every score by its bar (sweep_cases.rank_bounds' rule on the
    list's counted entries). twins[q]: ids whose table row is a copy of the truth's: their score equals the truth's
    on every evaluation, so they can never be above it and are left out."""
    M = len(truth)
    lo, hi = np.empty(M, dtype=np.int64), np.empty(M, dtype=np.int64)
    b = SC.bar(ref)
    for q in range(M):
        tr = int(truth[q])
        lst = L if L.ndim == 1 else L[q]
        keep = counted(lst, tr, ref.shape[1], None if ptr is None else ids[int(ptr[q]):int(ptr[q + 1])])
        if twins is not None and q in twins:
            keep &= ~np.isin(lst, twins[q])
        safe = np.where(keep, lst, 0)
        if 0 <= tr < ref.shape[1]:
            dlt, tol = ref[q, safe] - ref[q, tr], b[q, safe] + b[q, tr]
            lo[q], hi[q] = 1 + int((keep & (dlt > tol)).sum()), 1 + int((keep & (dlt > -tol)).sum())
        else:
            lo[q] = hi[q] = 1 + int(keep.sum())
    return lo, hi


def twins(name, d, mode):
    """{tie row: the ids of its truth's copies}."""
    return {q: cp for q, (_, cp) in tie_plan(name, d, mode).items()}


@functools.lru_cache(maxsize=None)
def expected(name, d, mode, filtered=True):
    """reference() on the fp64 scores: (ranks, ties, truth scores)."""
    truth, _ = truths(name, d, mode)
    ptr, ids = filters(name, d, mode) if filtered else (None, None)
    return reference(ref_scores(name, d, mode), truth, lists(name, d, mode), ptr, ids)


def planted_ties(name, d, mode, filtered=True):
    """The ties the construction plants: per tie row the counted list entries that are copies of its truth."""
    truth, _ = truths(name, d, mode)
    L = lists(name, d, mode)
    ptr, ids = filters(name, d, mode) if filtered else (None, None)
    out = np.zeros(B, dtype=np.int64)
    for q, tw in twins(name, d, mode).items():
        keep = counted(L[q], truth[q], E, None if ptr is None else ids[ptr[q]:ptr[q + 1]])
        out[q] = int((keep & np.isin(L[q], tw)).sum())
    return out


# ------------------------------------------------------------------------------------------------
# raw callers
# ------------------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else t.data_ptr()


def rank_candidates_raw(c, mode, ent, rel, pos, truth, cand, cand_ld, n_cand, fptr, fids, nfilter, ranks, ties, ts):
    """kge_eval_rank_candidates of case c on the table views ent / rel with explicit outputs; the return code."""
    from customknowledgegraphembedding_amd import _lib

    return _lib.load().kge_eval_rank_candidates(
        _lib.FN_IDS[c["name"]], mode, ent.data_ptr(), ent.shape[0], ent.stride(0), rel.data_ptr(), rel.shape[0],
        rel.stride(0), S.rel_off(c["name"], c["D"]), pos.data_ptr(), pos.shape[0], c["D"], c["gamma"], c["rng"],
        c["mod"], truth.data_ptr(), _ptr(cand), cand_ld, n_cand, _ptr(fptr), _ptr(fids), nfilter, ranks.data_ptr(),
        _ptr(ties), _ptr(ts), torch.cuda.current_stream(ent.device).cuda_stream)


def score_indexed_rc(c, mode, ent, rel, pos, neg, out):
    """kge_score_indexed's return code for the same tables (neg [M, N] row-contiguous, out [M, N])."""
    from customknowledgegraphembedding_amd import _lib

    return _lib.load().kge_score_indexed(
        _lib.FN_IDS[c["name"]], mode, ent.data_ptr(), ent.shape[0], ent.stride(0), rel.data_ptr(), rel.shape[0],
        rel.stride(0), S.rel_off(c["name"], c["D"]), pos.data_ptr(), neg.data_ptr(), neg.stride(0), pos.shape[0],
        neg.shape[1], c["D"], c["gamma"], c["rng"], c["mod"], out.data_ptr(), out.stride(0),
        torch.cuda.current_stream(ent.device).cuda_stream)


def composition(c, mode, ent, rel, pos, truth, cand, fptr=None, fids=None):
    """The three-step path the fused call replaces: kge_score_indexed's scores of [truth | candidates] (an [M, C + 1]
    matrix), then the header's counting rule applied on the host to those fp32 scores. cand [M, C] or [C] on the
    device; truth, fptr, fids as device tensors. Returns (ranks, ties, truth scores) as CPU tensors; the truth
    scores are the matrix's column 0 (-inf for an out-of-range truth)."""
    M, n_ent = pos.shape[0], ent.shape[0]
    rows = cand.unsqueeze(0).expand(M, -1) if cand.dim() == 1 else cand
    both = torch.cat([truth.reshape(M, 1), rows], dim=1).contiguous()
    out = torch.empty(both.shape, dtype=torch.float32, device=ent.device)
    rc = score_indexed_rc(c, mode, ent, rel, pos, both, out)
    assert rc == 0, rc
    A, ids, tr = out.cpu().numpy(), both.cpu().numpy(), truth.cpu().numpy()
    ptr = None if fptr is None else fptr.cpu().numpy()
    fl = None if fids is None else fids.cpu().numpy()
    ranks, ties = np.empty(M, dtype=np.int64), np.empty(M, dtype=np.int64)
    ts = A[:, 0].copy()
    with np.errstate(invalid="ignore"):
        for q in range(M):
            if not 0 <= tr[q] < n_ent:
                ts[q] = -np.inf
            keep = counted(ids[q, 1:], tr[q], n_ent, None if ptr is None else fl[int(ptr[q]):int(ptr[q + 1])])
            ranks[q] = 1 + int((keep & (A[q, 1:] > ts[q])).sum())
            ties[q] = int((keep & (A[q, 1:] == ts[q])).sum())
    return torch.from_numpy(ranks), torch.from_numpy(ties), torch.from_numpy(ts)
