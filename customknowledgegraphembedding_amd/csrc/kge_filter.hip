// kge_filter.hip — the evaluation filter built on the device: a set of query triples looked up in the true-answer
// table (kge_filter.h, built on the host by kge_filter_table.cpp) gives the filter CSR (ptr [M + 1], ids) that the
// rank and top-k entry points take: evaluate.build_filter's (drop_own = 1: the query's own answer left out) or
// build_exclude's (drop_own = 0). Three launches, no atomics, no allocation, no host sync inside a call:
//
//   kge_eval_filter_count   filter_count_kernel: a thread per query finds the key's row (binary search over the
//                           mode's ascending keys, 64-bit lexicographic compare; an absent key is an empty list),
//                           takes the list's length and, with drop_own, searches the list for the query's own
//                           candidate and takes one off when it is there. The list's start and the own position go
//                           to the workspace, the count to ptr[q + 1].
//                           filter_scan_kernel: one block turns the counts into starts in place, kFtScanTile at a
//                           time with an int64 carry: ptr[0] = 0, ptr[M] = the total.
//   (the caller reads ptr[M], the one host sync of an evaluation pass, and sizes ids)
//   kge_eval_filter_fill    filter_fill_kernel: a wave per query, lanes striding the list (the lists are skewed:
//                           thousands of heads for a popular (r, t), a handful at the median), copies the list into
//                           ids[ptr[q] .. ptr[q + 1]) without the own entry. Every write is guarded by ids_capacity.
//
// A blob whose magic or word count does not fit blob_bytes gives empty lists; nothing outside the blob is read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "kge_filter.h"
#include "kge_hip.h"

namespace kge_impl {
int set_error(int code, const char* msg);  // kge_abi.hip
}

namespace {

using namespace kge_impl;

constexpr int kFtBlock = 256;
constexpr int kFtScanBlock = 1024;  // x 4 counts per thread = kFtScanTile
static_assert(kFtScanBlock * 4 == kFtScanTile, "the scan block takes one tile per pass");

// workspace: per query the list's start (words of the mode's ids section) and the own entry's position in the
// list (-1: not there, or not dropped)
struct FtSlot {
    int64_t lo, own;
};

__device__ __forceinline__ bool ft_table_ok(const int64_t* __restrict__ w, int64_t blob_words) {
    return w[FT_MAGIC] == kFtMagic && w[FT_WORDS] >= kFtHdrWords && w[FT_WORDS] <= blob_words;
}

__global__ __launch_bounds__(kFtBlock) void filter_count_kernel(const int64_t* __restrict__ w, int64_t blob_words,
                                                                int mode, const int64_t* __restrict__ pos, int64_t M,
                                                                int drop_own, int64_t* __restrict__ ptr,
                                                                FtSlot* __restrict__ slot) {
    const int64_t q = (int64_t)blockIdx.x * kFtBlock + threadIdx.x;
    if (q == 0) ptr[0] = 0;
    if (q >= M) return;
    int64_t lo = 0, len = 0, own = -1;
    if (ft_table_ok(w, blob_words)) {
        // head-batch: key (r, t), candidate h; tail-batch: key (h, r), candidate t
        const int64_t a = pos[3 * q + (mode == KGE_HEAD_BATCH ? 1 : 0)];
        const int64_t b = pos[3 * q + (mode == KGE_HEAD_BATCH ? 2 : 1)];
        const int64_t c = pos[3 * q + (mode == KGE_HEAD_BATCH ? 0 : 2)];
        const int64_t rows = w[FT_ROWS + mode];
        const int64_t* __restrict__ ka = w + w[FT_KEY_A + mode];
        const int64_t* __restrict__ kb = w + w[FT_KEY_B + mode];
        int64_t x = 0, y = rows;  // the first row whose key is not below (a, b)
        while (x < y) {
            const int64_t mid = (x + y) >> 1;
            const int64_t va = ka[mid], vb = kb[mid];
            if (va < a || (va == a && vb < b)) x = mid + 1; else y = mid;
        }
        if (x < rows && ka[x] == a && kb[x] == b) {
            const int64_t* __restrict__ rp = w + w[FT_PTR + mode];
            lo = rp[x];
            len = rp[x + 1] - lo;
            if (drop_own) {
                const int64_t* __restrict__ L = w + w[FT_IDS + mode] + lo;
                int64_t u = 0, v = len;
                while (u < v) {
                    const int64_t mid = (u + v) >> 1;
                    if (L[mid] < c) u = mid + 1; else v = mid;
                }
                if (u < len && L[u] == c) {
                    own = u;
                    --len;
                }
            }
        }
    }
    slot[q].lo = lo;
    slot[q].own = own;
    ptr[q + 1] = len;
}

// in place: cnt[0 .. M) counts -> inclusive sums (cnt = ptr + 1, so ptr becomes the exclusive scan with the total
// at ptr[M]). One block; each pass takes a tile of kFtScanTile counts, four consecutive ones per thread.
__global__ __launch_bounds__(kFtScanBlock) void filter_scan_kernel(int64_t* __restrict__ cnt, int64_t M) {
    constexpr int NW = kFtScanBlock / 64;
    __shared__ int64_t wtot[NW];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    int64_t carry = 0;
    for (int64_t base = 0; base < M; base += kFtScanTile) {
        const int64_t i0 = base + 4 * (int64_t)t;
        int64_t x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = i0 + k < M ? cnt[i0 + k] : 0;
        const int64_t mine = x[0] + x[1] + x[2] + x[3];
        int64_t incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        if (lane == 63) wtot[wv] = incl;
        __syncthreads();
        int64_t before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const int64_t s = wtot[k];
            before += k < wv ? s : 0;
            all += s;
        }
        int64_t run = carry + before + incl - mine;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            run += x[k];
            if (i0 + k < M) cnt[i0 + k] = run;
        }
        carry += all;
        __syncthreads();  // wtot is rewritten by the next tile
    }
}

__global__ __launch_bounds__(kFtBlock) void filter_fill_kernel(const int64_t* __restrict__ w, int64_t blob_words,
                                                               int mode, int64_t M, const int64_t* __restrict__ ptr,
                                                               int64_t* __restrict__ ids, int64_t cap,
                                                               const FtSlot* __restrict__ slot) {
    const int lane = threadIdx.x & 63;
    // the wave's query, provably uniform: its bounds are loaded through the scalar cache
    const int64_t q = (int64_t)blockIdx.x * (kFtBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (q >= M || !ft_table_ok(w, blob_words)) return;
    const int64_t d0 = ptr[q], n = ptr[q + 1] - d0;
    const int64_t lo = slot[q].lo, own = slot[q].own;
    const int64_t rows = w[FT_ROWS + mode];
    const int64_t total = (w + w[FT_PTR + mode])[rows];  // words of the ids section
    // a workspace or ptr that is not this table's count's: nothing outside the section is read
    if (n <= 0 || d0 < 0 || lo < 0 || own >= n + 1 || lo > total - n - (own >= 0 ? 1 : 0)) return;
    const int64_t* __restrict__ L = w + w[FT_IDS + mode] + lo;
    for (int64_t j = lane; j < n; j += 64) {
        const int64_t d = d0 + j;
        if (d < cap) ids[d] = L[j + (own >= 0 && j >= own ? 1 : 0)];
    }
}

int ft_check(const char* fn, const void* blob, int64_t blob_bytes, int mode, const int64_t* pos, int64_t M,
             const int64_t* ptr, const void* workspace, size_t workspace_bytes) {
    const std::string f(fn);
    if (mode != KGE_HEAD_BATCH && mode != KGE_TAIL_BATCH)
        return set_error(KGE_EINVAL, (f + ": mode must be 0 (head-batch) or 1 (tail-batch)").c_str());
    if (M < 0 || M > (INT64_MAX >> 8)) return set_error(KGE_EINVAL, (f + ": M < 0 or too large").c_str());
    if (!blob || !ptr || !workspace || (M > 0 && !pos)) return set_error(KGE_EINVAL, (f + ": null pointer").c_str());
    if (blob_bytes < (int64_t)kFtHdrWords * 8 || ((uintptr_t)blob & 7))
        return set_error(KGE_EINVAL, (f + ": blob shorter than its header or not 8-B aligned").c_str());
    if (workspace_bytes < (size_t)kge_eval_filter_workspace_size(M) || ((uintptr_t)workspace & 15))
        return set_error(KGE_EINVAL,
                         (f + ": workspace smaller than kge_eval_filter_workspace_size or not 16-B aligned").c_str());
    if ((M + kFtBlock / 64 - 1) / (kFtBlock / 64) > INT32_MAX)
        return set_error(KGE_EINVAL, (f + ": grid too large").c_str());
    return 0;
}

int ft_launched(const char* fn) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(KGE_EHIP, (std::string(fn) + ": " + hipGetErrorString(e)).c_str());
    return 0;
}

}  // namespace

extern "C" {

int64_t kge_eval_filter_workspace_size(int64_t M) {
    if (M < 0 || M > (INT64_MAX >> 8)) return 0;
    return (int64_t)sizeof(FtSlot) * (M > 0 ? M : 1);
}

int kge_eval_filter_count(const void* blob, int64_t blob_bytes, int mode, const int64_t* pos, int64_t M, int drop_own,
                          int64_t* ptr, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "kge_eval_filter_count";
    if (const int rc = ft_check(fn, blob, blob_bytes, mode, pos, M, ptr, workspace, workspace_bytes)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    // M = 0: one block whose thread 0 writes ptr[0] = 0
    const unsigned blocks = (unsigned)(((M > 0 ? M : 1) + kFtBlock - 1) / kFtBlock);
    hipLaunchKernelGGL(filter_count_kernel, dim3(blocks), dim3(kFtBlock), 0, st, (const int64_t*)blob, blob_bytes / 8,
                       mode, pos, M, drop_own != 0, ptr, (FtSlot*)workspace);
    if (M > 0) hipLaunchKernelGGL(filter_scan_kernel, dim3(1), dim3(kFtScanBlock), 0, st, ptr + 1, M);
    return ft_launched(fn);
}

int kge_eval_filter_fill(const void* blob, int64_t blob_bytes, int mode, const int64_t* pos, int64_t M, int drop_own,
                         const int64_t* ptr, int64_t* ids, int64_t ids_capacity, const void* workspace,
                         size_t workspace_bytes, void* stream) {
    const char* fn = "kge_eval_filter_fill";
    if (const int rc = ft_check(fn, blob, blob_bytes, mode, pos, M, ptr, workspace, workspace_bytes)) return rc;
    if (ids_capacity < 0 || (ids_capacity > 0 && !ids))
        return set_error(KGE_EINVAL, "kge_eval_filter_fill: ids_capacity < 0, or ids NULL with a capacity");
    (void)drop_own;  // the own positions are in the workspace, as kge_eval_filter_count left them
    if (M == 0 || ids_capacity == 0) return 0;
    const unsigned blocks = (unsigned)((M + kFtBlock / 64 - 1) / (kFtBlock / 64));
    hipLaunchKernelGGL(filter_fill_kernel, dim3(blocks), dim3(kFtBlock), 0, (hipStream_t)stream, (const int64_t*)blob,
                       blob_bytes / 8, mode, M, ptr, ids, ids_capacity, (const FtSlot*)workspace);
    return ft_launched(fn);
}

}  // extern "C"
