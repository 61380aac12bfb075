// kge_dsampler_table.cpp — host side of the device negative sampler (kge_dsampler.hip): the true-answer
// table of a set of training triples, built once into caller-owned host memory as one relocatable blob
// (layout: kge_dsampler.h) that the caller uploads. It holds what upstream's TrainDataset keeps in Python
// dicts (codes/dataloader.py: true_head / true_tail, count_frequency), as CSR lists found by sorting:
// two sorts of the triples, no per-triple hash set. 64-bit ids throughout. No GPU involved.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "kge_dsampler.h"
#include "kge_hip.h"
#include "kge_truth_csr.h"

namespace kge_impl {
int set_error(int code, const char* msg);  // kge_abi.hip
}

namespace {

using namespace kge_impl;

using Key = TruthKey;

// One mode's CSR from the triples sorted by (group key, candidate): rows in key order, each row's distinct
// candidates ascending (truth_csr). Fills row[i] per triple, group[i] = triples (duplicates included) sharing i's
// key, ptr / ids; returns the rows, or -1 when a list covers every entity.
int64_t build_mode(std::vector<Key>& keys, int64_t E, int64_t* row, int64_t* group, int64_t* ptr, int64_t* ids) {
    return truth_csr(keys, ptr, ids, [&](int64_t r, size_t s, size_t e, int64_t len) {
        if (len >= E) return false;
        for (size_t k = s; k < e; ++k) {
            row[keys[k].i] = r;
            group[keys[k].i] = (int64_t)(e - s);
        }
        return true;
    });
}

}  // namespace

extern "C" {

int64_t kge_dsampler_table_size(int64_t ntriples) {
    if (ntriples < 0 || ntriples > (INT64_MAX >> 8)) return 0;
    return ds_max_words(ntriples) * 8;
}

int kge_dsampler_table_build(const int64_t* triples, int64_t ntriples, int64_t nentity, int64_t nrelation,
                             void* blob, int64_t blob_bytes) {
    const int64_t T = ntriples, E = nentity, R = nrelation;
    if (T < 0 || T > (INT64_MAX >> 8) || E <= 0 || R < 0 || (T > 0 && !triples) || !blob)
        return set_error(KGE_EINVAL, "kge_dsampler_table_build: bad arguments");
    if (blob_bytes < ds_max_words(T) * 8 || ((uintptr_t)blob & 7))
        return set_error(KGE_EINVAL, "kge_dsampler_table_build: blob smaller than kge_dsampler_table_size or misaligned");
    for (int64_t i = 0; i < T; ++i) {
        const int64_t h = triples[3 * i], r = triples[3 * i + 1], t = triples[3 * i + 2];
        if (h < 0 || h >= E || t < 0 || t >= E || r < 0 || r >= R)
            return set_error(KGE_EINVAL, ("kge_dsampler_table_build: triple " + std::to_string(i) +
                                          " has an id out of range").c_str());
    }
    int64_t* w = (int64_t*)blob;
    memset(w, 0, kDsHdrWords * 8);
    int64_t at = kDsHdrWords;
    w[DS_TRIPLES] = at;
    memcpy(w + at, triples, (size_t)T * 24);
    at += 3 * T;
    w[DS_ROW] = at;
    at += 2 * T;
    std::vector<Key> keys((size_t)T);
    std::vector<int64_t> group[2];
    for (int mode = 0; mode < 2; ++mode) {
        for (int64_t i = 0; i < T; ++i) {
            keys[(size_t)i] = truth_key(triples, i, mode == KGE_HEAD_BATCH);
        }
        group[mode].resize((size_t)T);
        // ptr needs at most T + 1 words and ids at most T: the ids start where ptr's bound ends and are
        // moved up against the real ptr afterwards
        int64_t* ptr = w + at;
        int64_t* ids = ptr + T + 1;
        const int64_t rows = build_mode(keys, E, w + w[DS_ROW] + mode * T, group[mode].data(), ptr, ids);
        if (rows < 0)
            return set_error(KGE_EINVAL, "kge_dsampler_table_build: a true-answer list covers every entity "
                                         "(no negative exists for its rows)");
        memmove(ptr + rows + 1, ids, (size_t)ptr[rows] * 8);
        w[DS_ROWS + mode] = rows;
        w[DS_PTR + mode] = at;
        w[DS_IDS + mode] = at + rows + 1;
        at += rows + 1 + ptr[rows];
    }
    w[DS_WEIGHT] = at;
    float* weight = (float*)(w + at);
    for (int64_t i = 0; i < T; ++i) {
        // count_frequency(triples, start=4): count[(h, r)] = 3 + the triples with this (h, r), count[(t, -r-1)]
        // = 3 + the triples with this (r, t); then kge_sampler_get's arithmetic
        const int64_t c = (3 + group[KGE_TAIL_BATCH][(size_t)i]) + (3 + group[KGE_HEAD_BATCH][(size_t)i]);
        weight[i] = sqrtf(1.0f / (float)c);  // torch.sqrt(1 / torch.Tensor([c])) in fp32
    }
    if (T & 1) weight[T] = 0.0f;
    at += (T + 1) / 2;
    w[DS_MAGIC] = kDsMagic;
    w[DS_WORDS] = at;
    w[DS_T] = T;
    w[DS_E] = E;
    w[DS_R] = R;
    return 0;
}

}  // extern "C"
