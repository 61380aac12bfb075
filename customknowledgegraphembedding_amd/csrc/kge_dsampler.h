// kge_dsampler.h — the true-answer table of the device-side negative sampler: one relocatable blob of int64
// words that kge_dsampler_table.cpp builds in host memory and kge_dsampler.hip reads on the device. Every
// section is addressed by a word offset from the blob's start, so the blob can be copied anywhere whole.
//
//   [0, kDsHdrWords)      header (the words below)
//   triples  [T][3]       the training triples (h, r, t)
//   row      [2][T]       per mode (head-batch, tail-batch), the triple's row in that mode's CSR
//   ptr      per mode     [rows + 1] list starts, in words of that mode's ids section
//   ids      per mode     the lists back to back: the sorted distinct true candidates of a row
//                         (head-batch: every h' with (h', r, t) a triple; tail-batch: every t' with (h, r, t'))
//   weight   [T] float    sqrt(1 / (count(h, r) + count(t, -r-1))), count start 4 (two floats per word)
#pragma once

#include <stdint.h>

namespace kge_impl {

constexpr int64_t kDsMagic = 0x3154424C53474B;  // "KGSLBT1"
enum DsHdr {
    DS_MAGIC = 0,
    DS_WORDS = 1,    // words of the whole blob
    DS_T = 2,        // triples
    DS_E = 3,        // entities
    DS_R = 4,        // relations
    DS_TRIPLES = 5,  // word offsets of the sections
    DS_ROW = 6,      // + mode * T
    DS_PTR = 7,      // + mode: the mode's ptr section
    DS_IDS = 9,      // + mode: the mode's ids section
    DS_WEIGHT = 11,
    DS_ROWS = 12,    // + mode: rows of the mode's CSR
    kDsHdrWords = 16,
};

// an upper bound of the blob's words for T triples (every list and every row count is at most T)
inline int64_t ds_max_words(int64_t T) {
    return kDsHdrWords + 3 * T + 2 * T + 2 * (T + 1) + 2 * T + (T + 1) / 2;
}

}  // namespace kge_impl
