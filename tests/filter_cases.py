"""Case data of the device-built evaluation filter (kge_filter_table_build, kge_eval_filter_count / _fill,
evaluate.FilterTable) and a numpy reader of the table blob, shared by test_filter_table_cpu.py and
test_filter_gpu.py. The yardstick is the Python already in the tree: evaluate.build_filter (drop_own) and
evaluate.build_exclude (not), computed once per (case, mode) at the largest query count; a smaller count's CSR is
its prefix (both walk the queries one by one). Every comparison is exact integer equality.

The reader looks a query up on the CPU from the blob's own sections (layout: csrc/kge_filter.h), which makes the
layout a tested contract without a GPU."""
import bisect
import functools

import numpy as np

from customknowledgegraphembedding_amd import evaluate

MODES = ("head-batch", "tail-batch")
TILE = evaluate.FILTER_SCAN_TILE
# 0, 1, around a wave, one below / at / above the scan's tile, past two tiles
M_LIST = (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 9)
M_MAX = max(M_LIST)
LENGTHS = (1, 2, 63, 64, 65, 130, 1100)  # crafted list lengths (0: an absent key); one above 1 024


def small():
    """E = 97 synthetic triples (entities 1 .. 96, relations 1 .. 4) plus crafted rows: head-batch lists (r = 10 + i,
    t = 50) and tail-batch lists (h = 60, r = 20 + i) of LENGTHS[i] candidates 0, 3, 6, ... (ids past E: the table
    has no entity bound), and duplicated triples."""
    g = np.random.RandomState(97)
    syn = np.stack([g.randint(1, 97, size=400), g.randint(1, 5, size=400), g.randint(1, 97, size=400)], 1)
    rows = [syn]
    for i, n in enumerate(LENGTHS):
        c = 3 * np.arange(n)
        rows.append(np.stack([c, np.full(n, 10 + i), np.full(n, 50)], 1))  # heads of (10 + i, 50)
        rows.append(np.stack([np.full(n, 60), np.full(n, 20 + i), c], 1))  # tails of (60, 20 + i)
    rows.append(syn[:40])          # duplicated true triples
    rows.append(rows[13][::2])     # and duplicates inside the longest crafted list
    triples = np.concatenate(rows).astype(np.int64)
    triples = triples[g.permutation(len(triples))]

    big = 10 ** 6
    q = [(0, 0, 0),                # a key below the first key (both modes)
         (big, big, big),          # above the last
         (5, 10, 49), (5, 10, 51), (60, 9, 5), (60, 40, 5),  # first word present, second absent
         (5, 7, 50), (98, 2, 5),   # first word absent (relation 7, head 98), between two keys
         (0, 10, 50), (60, 20, 0)]  # a length-1 list that is only the own answer: empty after the drop
    for i, n in enumerate(LENGTHS):
        last = 3 * (n - 1)
        for own in (0, last, 3 * (n // 2), 1, last + 3):  # own answer first, last, middle, absent (inside, past)
            q.append((own, 10 + i, 50))
            q.append((60, 20 + i, own))
    q = np.array(q, dtype=np.int64)
    q = np.concatenate([q, syn[:60], np.stack([syn[:30, 0], syn[:30, 1], syn[30:60, 2]], 1), q[:12]])  # + duplicates
    return triples, _cycle(q, g)


def wide():
    """Ids 2^31 + k and 2^40 + k, and keys that differ only above bit 32, in either word: a compare that drops
    the high half of a word finds the wrong row."""
    g = np.random.RandomState(40)
    a = [5, 5 + 2 ** 32, 2 ** 31 + 5, 2 ** 40 + 5, 5 + 2 ** 33]       # first words
    b = [7, 7 + 2 ** 32, 2 ** 31 + 7, 2 ** 40 + 7, 7 + 2 ** 36]       # second words
    c = [1, 2 ** 31 + 1, 2 ** 31 + 2, 2 ** 40 + 1, 2 ** 40 + 2, 1 + 2 ** 32, 2 ** 62]  # candidates
    triples = []
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            if (i + 2 * j) % 5 == 4:
                continue  # an absent key between present ones
            for k, z in enumerate(c):
                if (i + j + k) % 3 != 0 or k == i:
                    triples.append((z, x, y))  # head-batch key (r, t) = (x, y), head z
                    triples.append((x, y, z))  # tail-batch key (h, r) = (x, y), tail z
    triples = np.array(triples, dtype=np.int64)
    q = [(z, x, y) for x in a + [6, 2 ** 41] for y in b + [8, 2 ** 35] for z in c[:5] + [3]]
    q += [(x, y, z) for x in a + [6, 2 ** 41] for y in b + [8, 2 ** 35] for z in c[:5] + [3]]
    return triples, _cycle(np.array(q, dtype=np.int64), g)


def _cycle(pool, g):
    """M_MAX queries: the pool in order, then shuffled repeats of it (duplicated queries, long lists at every
    offset within a tile)."""
    parts = [pool]
    while sum(len(p) for p in parts) < M_MAX:
        parts.append(pool[g.permutation(len(pool))])
    return np.ascontiguousarray(np.concatenate(parts)[:M_MAX])


CASES = {"small": small, "wide": wide}


@functools.lru_cache(maxsize=None)
def case(name):
    """(triples [T, 3], queries [M_MAX, 3]) of a case, read-only."""
    triples, queries = CASES[name]()
    triples.setflags(write=False)
    queries.setflags(write=False)
    return triples, queries


@functools.lru_cache(maxsize=None)
def reference(name, mode, drop_own):
    """build_filter's (drop_own) or build_exclude's CSR of the case's M_MAX queries, read-only."""
    triples, queries = case(name)
    ptr, ids = (evaluate.build_filter if drop_own else evaluate.build_exclude)(queries, mode, triples)
    ptr.setflags(write=False)
    ids.setflags(write=False)
    return ptr, ids


def prefix(ref, M):
    """The CSR of the first M queries."""
    ptr, ids = ref
    return ptr[:M + 1], ids[:ptr[M]]


class Blob:
    """The filter table's blob read with numpy (csrc/kge_filter.h's header words)."""
    MAGIC, WORDS, T, KEY_A, KEY_B, PTR, IDS, ROWS, HDR = 0, 1, 2, 3, 5, 7, 9, 11, 16
    MAGIC_VALUE = int.from_bytes(b"KFLTTB1\0", "little")

    def __init__(self, words):
        self.w = w = np.asarray(words, dtype=np.int64)
        self.ntriples = int(w[self.T])
        self.rows, self.keys, self.ptr, self.ids = [], [], [], []
        for mode in (0, 1):
            rows = int(w[self.ROWS + mode])
            ka = w[int(w[self.KEY_A + mode]):][:rows]
            kb = w[int(w[self.KEY_B + mode]):][:rows]
            ptr = w[int(w[self.PTR + mode]):][:rows + 1]
            self.rows.append(rows)
            self.keys.append(list(zip(ka.tolist(), kb.tolist())))  # Python ints: an exact lexicographic order
            self.ptr.append(ptr)
            self.ids.append(w[int(w[self.IDS + mode]):][:int(ptr[rows])])

    def check_layout(self):
        """The sections lie back to back in the order the header documents and fill the words in use; keys and
        lists strictly ascending."""
        w = self.w
        assert int(w[self.MAGIC]) == self.MAGIC_VALUE and int(w[self.WORDS]) == len(w)
        at = self.HDR
        for mode in (0, 1):
            rows = self.rows[mode]
            assert [int(w[k + mode]) for k in (self.KEY_A, self.KEY_B, self.PTR, self.IDS)] == \
                [at, at + rows, at + 2 * rows, at + 3 * rows + 1]
            at += 3 * rows + 1 + int(self.ptr[mode][rows])
            assert all(x < y for x, y in zip(self.keys[mode], self.keys[mode][1:]))
            assert int(self.ptr[mode][0]) == 0 and np.all(np.diff(self.ptr[mode]) >= 1)
            for r in range(rows):
                assert np.all(np.diff(self.ids[mode][self.ptr[mode][r]:self.ptr[mode][r + 1]]) > 0)
        assert at == len(w)

    def lookup(self, query, mode, drop_own):
        h, r, t = (int(v) for v in query)
        m = MODES.index(mode)
        key, own = ((r, t), h) if m == 0 else ((h, r), t)
        i = bisect.bisect_left(self.keys[m], key)
        if i == self.rows[m] or self.keys[m][i] != key:
            return []
        lst = self.ids[m][self.ptr[m][i]:self.ptr[m][i + 1]].tolist()
        return [e for e in lst if not (drop_own and e == own)]

    def csr(self, queries, mode, drop_own):
        lists = [self.lookup(q, mode, drop_own) for q in np.asarray(queries, dtype=np.int64).reshape(-1, 3)]
        ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
        ids = np.array([e for x in lists for e in x], dtype=np.int64)
        return ptr, ids
