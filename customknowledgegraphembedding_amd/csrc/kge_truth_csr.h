// kge_truth_csr.h — the sort-and-group loop the host table builders share (kge_dsampler_table.cpp: the device
// sampler's true-answer table; kge_filter_table.cpp: the evaluation filter table). A set of triples becomes one
// mode's CSR of true candidates by one sort: rows in ascending key order, each row's distinct candidates
// ascending. Host only.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace kge_impl {

struct TruthKey {
    int64_t a, b, c;  // group key (a, b), candidate c
    int64_t i;        // the triple
    bool operator<(const TruthKey& o) const {
        if (a != o.a) return a < o.a;
        if (b != o.b) return b < o.b;
        return c < o.c;
    }
};

// head-batch: true_head[(r, t)] holds heads; tail-batch: true_tail[(h, r)] holds tails (mode 0 is head-batch)
inline TruthKey truth_key(const int64_t* triples, int64_t i, int head_batch) {
    const int64_t h = triples[3 * i], r = triples[3 * i + 1], t = triples[3 * i + 2];
    return head_batch ? TruthKey{r, t, h, i} : TruthKey{h, r, t, i};
}

// Sorts keys by (group key, candidate) and writes ptr[rows + 1] / ids (each at most keys.size() (+ 1) words).
// on_row(row, s, e, len) is called once per group, in key order, with the group's span keys[s, e) (duplicates
// included) and its count of distinct candidates; it returns false to stop. Returns the rows, or -1 when stopped.
template <class OnRow>
int64_t truth_csr(std::vector<TruthKey>& keys, int64_t* ptr, int64_t* ids, OnRow on_row) {
    std::sort(keys.begin(), keys.end());
    const size_t T = keys.size();
    int64_t rows = 0, n = 0;
    ptr[0] = 0;
    for (size_t s = 0; s < T;) {
        size_t e = s;
        const int64_t start = n;
        while (e < T && keys[e].a == keys[s].a && keys[e].b == keys[s].b) {
            if (n == start || ids[n - 1] != keys[e].c) ids[n++] = keys[e].c;
            ++e;
        }
        if (!on_row(rows, s, e, n - start)) return -1;
        ptr[++rows] = n;
        s = e;
    }
    return rows;
}

}  // namespace kge_impl
