"""A numpy / Python restatement of the device negative sampler's contract (include/kge_hip.h,
kge_dsampler_sample): Philox4x32-10, the draw u -> u + j over a row's sorted true-answer list, and the true-answer
table's contents from plain dicts, as upstream's TrainDataset keeps them (true_head / true_tail, count_frequency
with start 4). A plain module shared by test_device_sampler_cpu.py and test_device_sampler_gpu.py: nothing here is a
fixture or changes how the suite is collected."""
import bisect
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85  # Random123's Philox4x32 constants
MASK = 0xFFFFFFFF
HEAD, TAIL = 0, 1


def philox4x32_10(counter, key):
    """Philox4x32-10 of counter (c0, c1, c2, c3) and key (k0, k1): Python integers or equal-shaped uint64 arrays
    holding 32-bit values; returns the four output words."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c3 ^ k1) & MASK, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox_rows(rows, N, mode, seed, step):
    """x [len(rows), N] as Python-int object array: the 64-bit word of every (row, slot); one Philox call serves the
    slots 2p and 2p + 1. Vectorised over numpy uint64 (the 32 x 32-bit products fit 64 bits)."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    P = (N + 1) // 2
    pair = np.arange(P, dtype=np.uint64).reshape(1, -1)
    u64 = np.uint64
    shape = (rows.shape[0], P)
    c0 = np.broadcast_to(pair | u64(int(mode) << 31), shape).copy()
    c1 = np.broadcast_to(rows & u64(MASK), shape).copy()
    c2 = np.full(shape, step & MASK, dtype=np.uint64)
    c3 = np.full(shape, (step >> 32) & MASK, dtype=np.uint64)
    k0, k1 = u64(seed & MASK), u64((seed >> 32) & MASK)
    m = u64(MASK)
    for _ in range(10):
        p0, p1 = u64(M0) * c0, u64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> u64(32)) ^ c1 ^ k0) & m, p1 & m, ((p0 >> u64(32)) ^ c3 ^ k1) & m, p0 & m
        k0, k1 = (k0 + u64(W0)) & m, (k1 + u64(W1)) & m
    x = np.empty((rows.shape[0], 2 * P), dtype=object)
    x[:, 0::2] = (c0 | (c1 << u64(32))).astype(object)
    x[:, 1::2] = (c2 | (c3 << u64(32))).astype(object)
    return x[:, :N]


def kth_valid(u, L):
    """The u-th entity (from 0) of the complement of the sorted distinct list L: u + #{i : L[i] - i <= u}."""
    keys = [v - i for i, v in enumerate(L)]
    return u + bisect.bisect_right(keys, u)


class Table:
    """What the table holds, from dicts: the sorted true-answer list of every triple in both modes, and its
    weight as upstream computes it (fp32)."""

    def __init__(self, triples, nentity):
        self.triples = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
        self.E = int(nentity)
        count, true = {}, ({}, {})
        for h, r, t in self.triples.tolist():
            for k in ((h, r), (t, -r - 1)):
                count[k] = count.get(k, 3) + 1  # count_frequency(start=4)
            true[HEAD].setdefault((r, t), set()).add(h)
            true[TAIL].setdefault((h, r), set()).add(t)
        self.lists = tuple({k: sorted(v) for k, v in d.items()} for d in true)
        self.keys = tuple([(r, t) if mode == HEAD else (h, r) for h, r, t in self.triples.tolist()]
                          for mode in (HEAD, TAIL))
        c = np.array([count[(h, r)] + count[(t, -r - 1)] for h, r, t in self.triples.tolist()], dtype=np.float32)
        self.weight = np.sqrt(np.float32(1.0) / c).astype(np.float32)  # torch.sqrt(1 / torch.Tensor([c]))

    def list_of(self, mode, i):
        return self.lists[mode][self.keys[mode][i]]

    def sample(self, idx, N, mode, seed, step, row0=0):
        """(pos [B, 3], neg [B, N], w [B]) the device sampler must give for the triple indices idx; an index outside
        [0, T) gives (-1, -1, -1), -1 and 0."""
        idx = [int(i) for i in idx]
        B, T = len(idx), len(self.triples)
        pos = np.full((B, 3), -1, dtype=np.int64)
        neg = np.full((B, N), -1, dtype=np.int64)
        w = np.zeros(B, dtype=np.float32)
        x = philox_rows([row0 + b for b in range(B)], N, mode, seed, step)
        for b, i in enumerate(idx):
            if not 0 <= i < T:
                continue
            L = self.list_of(mode, i)
            M = self.E - len(L)
            keys = [v - k for k, v in enumerate(L)]
            pos[b], w[b] = self.triples[i], self.weight[i]
            for n in range(N):
                u = (x[b, n] * M) >> 64
                neg[b, n] = u + bisect.bisect_right(keys, u)
        return pos, neg, w


class Blob:
    """The sections of a built table (csrc/kge_dsampler.h) as numpy views of its int64 words."""

    MAGIC, WORDS, T, E, R, TRIPLES, ROW, PTR, IDS, WEIGHT, ROWS = 0, 1, 2, 3, 4, 5, 6, 7, 9, 11, 12

    def __init__(self, words):
        w = self.w = np.asarray(words, dtype=np.int64)
        T = self.ntriples = int(w[self.T])
        self.triples = w[w[self.TRIPLES]:w[self.TRIPLES] + 3 * T].reshape(T, 3)
        self.row = [w[w[self.ROW] + m * T:w[self.ROW] + (m + 1) * T] for m in (HEAD, TAIL)]
        self.ptr = [w[w[self.PTR + m]:w[self.PTR + m] + w[self.ROWS + m] + 1] for m in (HEAD, TAIL)]
        self.ids = [w[w[self.IDS + m]:w[self.IDS + m] + self.ptr[m][-1]] for m in (HEAD, TAIL)]
        self.weight = w[w[self.WEIGHT]:w[self.WEIGHT] + (T + 1) // 2].view(np.float32)[:T]

    def list_of(self, mode, i):
        r = int(self.row[mode][i])
        return self.ids[mode][int(self.ptr[mode][r]):int(self.ptr[mode][r + 1])].tolist()


def countries():
    z = np.load(os.path.join(GOLDEN, "countries_S1_train_ids.npz"))
    return z["triples"], int(z["nentity"]), int(z["nrelation"])


def synthetic97():
    """E = 97, R = 4: lists of length 1, of length E - 1 (M = 1), one starting at 0, one ending at E - 1, and long
    consecutive runs, in both modes (relation 0 .. 3 shape the tails' lists, the same shapes mirrored shape the
    heads')."""
    E, R, t = 97, 4, []
    t += [(1, 0, 50)]                                    # tail list {50}; head list of (0, 50) = {1}
    t += [(2, 0, k) for k in range(E) if k != 40]        # tail list: all but 40 (M = 1)
    t += [(k, 1, 3) for k in range(E) if k != 96]        # head list of (1, 3): all but 96 (M = 1, ends at E - 2)
    t += [(5, 2, k) for k in range(0, 30)]               # a run from 0
    t += [(5, 3, k) for k in range(60, 97)]              # a run to E - 1
    t += [(k, 2, 7) for k in list(range(0, 20)) + list(range(40, 70)) + [96]]   # head runs, first and last entity
    t += [(9, 3, k) for k in (0, 2, 4, 6, 8, 10, 96)]    # gaps of one
    t += [(9, 3, 4), (1, 0, 50)]                         # duplicates (counted for the weights, once in the lists)
    return np.array(t, dtype=np.int64), E, R
