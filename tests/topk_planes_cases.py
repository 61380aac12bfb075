"""Cases and the numpy reference of kge_eval_topk_planes (tests/test_topk_planes_cpu.py checks the cases
themselves, tests/test_topk_planes_gpu.py runs them). No GPU, no library."""
from __future__ import annotations

import functools

import numpy as np

TOPK_MAX = 64
TILE = 256  # columns per list of the selecting epilogue
SURPLUS_A, SURPLUS_B = 5, 9  # plane rows past M / N (NaN rows that must never appear)

# (M, N, K, k): every M of {1, 40, 257, 300}, N of {1, 31, 255, 256, 257, 523, 700}, K of {1, 15, 16, 17, 100} and
# k of {1, 10, 64}; k > N (padding); M 300 x N 700 at every k
SHAPES = [(1, 1, 1, 1), (40, 1, 15, 10), (40, 31, 16, 10), (40, 31, 17, 64), (257, 255, 17, 10), (257, 256, 16, 64),
          (40, 257, 100, 1), (300, 523, 15, 10), (1, 700, 1, 64), (300, 700, 100, 1), (300, 700, 100, 10),
          (300, 700, 16, 64)]

# duplicated rows of B: across a 32-column accumulator tile, the two column halves of a block, two blocks, far apart
TIE_PAIRS = [(31, 32), (127, 128), (255, 256), (5, 600)]
TIE_BOUNDARIES = {(31, 32): 32, (127, 128): 128, (255, 256): 256, (5, 600): 512}
TIE_M, TIE_N, TIE_K = 300, 700, 16


def reference(S, k, excl_ptr=None, excl_ids=None):
    """(ids [M, k] int64, scores [M, k] fp32) of the contract: the stable sort of each row by descending score
    (so ties come out by ascending id), NaN scores and the row's excluded ids left out, padded with -1 / -inf."""
    S = np.asarray(S)
    M, N = S.shape
    ids = np.full((M, k), -1, dtype=np.int64)
    sc = np.full((M, k), -np.inf, dtype=np.float32)
    for q in range(M):
        ok = ~np.isnan(S[q])
        if excl_ptr is not None:
            x = np.asarray(excl_ids[excl_ptr[q]:excl_ptr[q + 1]])
            x = x[(x >= 0) & (x < N)]
            ok[x] = False
        cand = np.nonzero(ok)[0]
        order = cand[np.argsort(-S[q, cand].astype(np.float64), kind="stable")][:k]
        ids[q, :len(order)] = order
        sc[q, :len(order)] = S[q, order]
    return ids, sc


def csr(rows):
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    for i, r in enumerate(rows):
        ptr[i + 1] = ptr[i] + len(r)
    ids = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if rows else np.zeros(0, dtype=np.int64)
    return ptr, ids.astype(np.int64)


@functools.lru_cache(maxsize=None)
def shape_case(M, N, K, seed=0):
    g = np.random.RandomState(1000 + seed + M + 7 * N + 13 * K)
    return {"A": g.standard_normal((M, K)).astype(np.float32), "B": g.standard_normal((N, K)).astype(np.float32)}


@functools.lru_cache(maxsize=None)
def tie_case():
    """B's rows at TIE_PAIRS duplicated (and scaled up, so that they reach the lists of many query rows)."""
    c = dict(shape_case(TIE_M, TIE_N, TIE_K, seed=1))
    B = c["B"].copy()
    for a, b in TIE_PAIRS:
        B[a] *= 3.0
        B[b] = B[a]
    c["B"] = B
    c["pairs"] = list(TIE_PAIRS)
    return c


@functools.lru_cache(maxsize=None)
def kth_tie_case(k):
    """Query row 0 is the unit vector of dimension 0 and B[:, 0] a permutation of 1 .. N (exact in the planes), so
    row 0's scores are B[:, 0]; the rows holding its k-th and (k + 1)-th largest value are made equal: `pair`."""
    c = dict(shape_case(TIE_M, TIE_N, TIE_K, seed=2))
    A, B = c["A"].copy(), c["B"].copy()
    g = np.random.RandomState(77 + k)
    B[:, 0] = g.permutation(TIE_N).astype(np.float32) + 1.0
    A[0] = 0.0
    A[0, 0] = 1.0
    order = np.argsort(-B[:, 0], kind="stable")
    a, b = sorted((int(order[k - 1]), int(order[k])))
    B[max(a, b)] = B[min(a, b)]
    c.update(A=A, B=B, pair=(a, b), k=k)
    return c


@functools.lru_cache(maxsize=None)
def equal_case():
    c = dict(shape_case(TIE_M, TIE_N, TIE_K, seed=3))
    c["B"] = np.repeat(c["B"][:1], TIE_N, axis=0).copy()
    return c


NAN_ENTITIES = (3, 256, 699)
NAN_QUERY = 7
POS_INF_ENTITIES = (40, 300)
NEG_INF_ENTITIES = (41, 511)


@functools.lru_cache(maxsize=None)
def special_case():
    """NaN entity rows, a NaN query row, and +-inf scores: A[:, 0] = 2^100 and B[e, 0] = +-2^100 (powers of two: the
    lower planes are zero, so the one product 2^200 overflows to +-inf and nothing else does)."""
    c = dict(shape_case(TIE_M, TIE_N, TIE_K, seed=4))
    A, B = c["A"].copy(), c["B"].copy()
    A[:, 0] = np.float32(2.0 ** 100)
    B[:, 0] = 0.0
    for e in POS_INF_ENTITIES:
        B[e, 0] = np.float32(2.0 ** 100)
    for e in NEG_INF_ENTITIES:
        B[e, 0] = -np.float32(2.0 ** 100)
    for e in NAN_ENTITIES:
        B[e] = np.nan
    A[NAN_QUERY] = np.nan
    c.update(A=A, B=B)
    return c


ALL_ROW, BUT3_ROW, OOR_ROW = 2, 4, 6
BUT3_KEPT = (100, 256, 650)


@functools.lru_cache(maxsize=None)
def exclusion_rows(M, N, seed=0):
    """Per-row exclusion lists (ascending, distinct): random ones, runs across the 256-column tile boundaries, one
    with out-of-range ids (-3, N, N + 7), one that excludes everything, one that excludes all but BUT3_KEPT."""
    g = np.random.RandomState(500 + seed)
    rows = []
    for q in range(M):
        n = int(g.randint(0, 12))
        r = set(g.choice(N, size=min(n, N), replace=False).tolist())
        if q % 3 == 0:
            for b in range(TILE, N, TILE):
                r.update(range(max(0, b - 4), min(N, b + 4)))
        rows.append(sorted(r))
    if M > OOR_ROW and N > max(BUT3_KEPT):
        rows[ALL_ROW] = list(range(N))
        rows[BUT3_ROW] = [e for e in range(N) if e not in BUT3_KEPT]
        rows[OOR_ROW] = [-3] + sorted(set(rows[OOR_ROW]) | {0, N - 1}) + [N, N + 7]
    return tuple(tuple(r) for r in rows)


def lists_bytes(M, N, k):
    """The bytes of the lists a call can write: one list of k 8-byte entries per (row, 256-column tile)."""
    return M * ((N + TILE - 1) // TILE) * k * 8
