// kge_filter_table.cpp — host side of the device-built evaluation filter (kge_filter.hip): the true-answer table
// of a set of triples, built once into caller-owned host memory as one relocatable blob (layout: kge_filter.h)
// that the caller uploads. It holds what evaluate.build_filter / build_exclude keep in Python dicts of sets, as
// keyed CSR lists found by sorting (kge_truth_csr.h: the loop the device sampler's table shares): two sorts of
// the triples, no per-triple hash set. Ids are any int64 >= 0 (the rank kernels range-check ids themselves), a
// list may cover every entity, duplicated triples collapse. No GPU involved.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "kge_filter.h"
#include "kge_hip.h"
#include "kge_truth_csr.h"

namespace kge_impl {
int set_error(int code, const char* msg);  // kge_abi.hip
}

extern "C" {

using namespace kge_impl;

int64_t kge_filter_table_size(int64_t ntriples) {
    if (ntriples < 0 || ntriples > (INT64_MAX >> 8)) return 0;
    return ft_max_words(ntriples) * 8;
}

int kge_filter_table_build(const int64_t* triples, int64_t ntriples, void* blob, int64_t blob_bytes) {
    const int64_t T = ntriples;
    if (T < 0 || T > (INT64_MAX >> 8) || (T > 0 && !triples) || !blob)
        return set_error(KGE_EINVAL, "kge_filter_table_build: bad arguments");
    if (blob_bytes < ft_max_words(T) * 8 || ((uintptr_t)blob & 7))
        return set_error(KGE_EINVAL, "kge_filter_table_build: blob smaller than kge_filter_table_size or misaligned");
    for (int64_t i = 0; i < 3 * T; ++i) {
        if (triples[i] < 0)
            return set_error(KGE_EINVAL, ("kge_filter_table_build: triple " + std::to_string(i / 3) +
                                          " has a negative id").c_str());
    }
    int64_t* w = (int64_t*)blob;
    memset(w, 0, kFtHdrWords * 8);
    int64_t at = kFtHdrWords;
    std::vector<TruthKey> keys((size_t)T);
    for (int mode = 0; mode < 2; ++mode) {
        for (int64_t i = 0; i < T; ++i) keys[(size_t)i] = truth_key(triples, i, mode == KGE_HEAD_BATCH);
        // the mode's sections at their bounds (T keys twice, T + 1 starts, T ids), moved up against the real row
        // count afterwards; every move is towards lower addresses, in section order
        int64_t* ka = w + at;
        int64_t* kb = ka + T;
        int64_t* ptr = kb + T;
        int64_t* ids = ptr + T + 1;
        const int64_t rows = truth_csr(keys, ptr, ids, [&](int64_t r, size_t s, size_t, int64_t) {
            ka[r] = keys[s].a;
            kb[r] = keys[s].b;
            return true;
        });
        const int64_t n = ptr[rows];
        memmove(ka + rows, kb, (size_t)rows * 8);
        memmove(ka + 2 * rows, ptr, (size_t)(rows + 1) * 8);
        memmove(ka + 3 * rows + 1, ids, (size_t)n * 8);
        w[FT_ROWS + mode] = rows;
        w[FT_KEY_A + mode] = at;
        w[FT_KEY_B + mode] = at + rows;
        w[FT_PTR + mode] = at + 2 * rows;
        w[FT_IDS + mode] = at + 3 * rows + 1;
        at += 3 * rows + 1 + n;
    }
    w[FT_MAGIC] = kFtMagic;
    w[FT_WORDS] = at;
    w[FT_T] = T;
    return 0;
}

}  // extern "C"
