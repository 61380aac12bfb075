// kge_filter.h — the true-answer table of the evaluation filter: one relocatable blob of int64 words that
// kge_filter_table.cpp builds in host memory from a set of triples and kge_filter.hip looks up on the device by
// arbitrary query triples (test triples are not table triples, so each row keeps its key). Every section is
// addressed by a word offset from the blob's start, so the blob can be copied anywhere whole.
//
//   [0, kFtHdrWords)      header (the words below)
//   per mode (head-batch, tail-batch):
//   key_a   [rows]        the distinct row keys, ascending in lexicographic order of (key_a, key_b):
//   key_b   [rows]        head-batch (r, t), tail-batch (h, r)
//   ptr     [rows + 1]    list starts, in words of that mode's ids section
//   ids                   the lists back to back: the sorted distinct true candidates of a row
//                         (head-batch: every h' with (h', r, t) a triple; tail-batch: every t' with (h, r, t'))
#pragma once

#include <stdint.h>

namespace kge_impl {

constexpr int64_t kFtMagic = 0x314254544C464B;  // "KFLTTB1"
enum FtHdr {
    FT_MAGIC = 0,
    FT_WORDS = 1,   // words of the whole blob
    FT_T = 2,       // triples the table was built from (duplicates included)
    FT_KEY_A = 3,   // + mode: word offsets of the mode's sections
    FT_KEY_B = 5,   // + mode
    FT_PTR = 7,     // + mode
    FT_IDS = 9,     // + mode
    FT_ROWS = 11,   // + mode: rows of the mode's CSR
    kFtHdrWords = 16,
};

// an upper bound of the blob's words for T triples (per mode: rows and list words are at most T each)
inline int64_t ft_max_words(int64_t T) { return kFtHdrWords + 2 * (T + T + (T + 1) + T); }

// the scan of kge_eval_filter_count walks the counts in tiles of this many queries (one block, carried in int64)
constexpr int kFtScanTile = 4096;

}  // namespace kge_impl
