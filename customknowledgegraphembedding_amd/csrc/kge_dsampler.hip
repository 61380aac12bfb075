// kge_dsampler.hip — device-side negative sampler of the training batches: for every batch row, N negatives
// drawn uniformly from the entities that are NOT true answers of the row (upstream TrainDataset's
// distribution: i.i.d. uniform draws, the true ones dropped, the first N kept), with the batch's positives and
// subsampling weights gathered in the same launch. One launch, no atomics, no workspace, no host round trip.
//
// The draw of slot n of batch row b (global row = row0 + b), L = the row's sorted distinct true candidates
// (kge_dsampler.h), M = E - |L|:
//   w[0..3] = Philox4x32-10(counter (c0, row, step_lo, step_hi), key (seed_lo, seed_hi)),
//             c0 = (n >> 1) | mode << 31                       (Random123's constants)
//   x = w0 | w1 << 32 (n even) or w2 | w3 << 32 (n odd); u = (x * M) >> 64
//   neg[b, n] = u + j, j = #{i : L[i] - i <= u}: the u-th entity of L's complement. L[i] - i never decreases, so j
//   is an upper bound found by binary search: no rejection loop, no data-dependent trip count.
// A value depends on (seed, step, mode, row, n) and the row's list only: not on B, the grid, or how a batch is
// split over calls or ranks.
//
// Shape: a wave takes 64 slot pairs of ONE batch row (a row of N slots is ceil(N / 128) waves), so the row's
// triple, list bounds and M are wave-uniform and come from scalar loads; each lane makes one Philox call, two
// searches with a common trip count (the list's length is uniform; the two chains of dependent L2 loads
// interleave) and one 16-byte store of its two ids, coalesced along n. The searches are latency, hidden by
// occupancy: the kernel keeps few registers so that a CU holds all the waves it is given.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "kge_dsampler.h"
#include "kge_hip.h"

namespace kge_impl {
int set_error(int code, const char* msg);  // kge_abi.hip
}

namespace {

using namespace kge_impl;

constexpr int kDsBlock = 256;  // 4 waves, each with its own batch row (or 128-slot piece of one)

// the table, the indices and the device step are read-only and never alias an output: they are kernel arguments
// of their own (__restrict__), so that the wave-uniform reads of them go through the scalar cache
struct DsArgs {
    int64_t blob_words;
    int64_t step;
    uint64_t seed;
    int64_t B, N, row0;
    int64_t* pos;
    int64_t* neg;
    int64_t neg_ld;
    float* weight;
    int mode;
    int wpr;  // waves per batch row
    int vec;  // neg rows take 16-byte stores (16-B aligned base, even row stride)
};

__device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                     uint32_t (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

__global__ __launch_bounds__(kDsBlock) void dsampler_kernel(const int64_t* __restrict__ w,
                                                            const int64_t* __restrict__ idx,
                                                            const int64_t* __restrict__ step_ptr, const DsArgs a) {
    const int lane = threadIdx.x & 63;
    // the wave's number, provably uniform: everything derived from it is loaded through the scalar cache
    const int64_t wave = (int64_t)blockIdx.x * (kDsBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t b = wave / a.wpr;
    if (b >= a.B) return;
    const int64_t pair = (wave - b * a.wpr) * 64 + lane;  // slots 2 pair, 2 pair + 1
    const int64_t n0 = 2 * pair;

    // the blob's header, and the batch row's triple: -1 when the blob is not a table that fits the bytes given or
    // idx[b] is no triple of it (nothing past the header is read then)
    const bool table = w[DS_MAGIC] == kDsMagic && w[DS_WORDS] <= a.blob_words;
    const int64_t i = idx[b];
    const bool ok = table && i >= 0 && i < w[DS_T];
    int64_t* nrow = a.neg + b * a.neg_ld;
    if (!ok) {
        if (n0 + 1 < a.N && a.vec) {
            *(longlong2*)(nrow + n0) = make_longlong2(-1, -1);
        } else {
            if (n0 < a.N) nrow[n0] = -1;
            if (n0 + 1 < a.N) nrow[n0 + 1] = -1;
        }
        if (pair < 3) a.pos[3 * b + pair] = -1;
        if (pair == 0) a.weight[b] = 0.0f;
        return;
    }
    if (pair < 3) a.pos[3 * b + pair] = w[w[DS_TRIPLES] + 3 * i + pair];
    if (pair == 0) a.weight[b] = ((const float*)(w + w[DS_WEIGHT]))[i];
    if (n0 >= a.N) return;

    const int64_t row = w[w[DS_ROW] + a.mode * w[DS_T] + i];
    const int64_t* __restrict__ ptr = w + w[DS_PTR + a.mode];
    const int64_t lo = ptr[row], len = ptr[row + 1] - lo;
    const int64_t* __restrict__ L = w + w[DS_IDS + a.mode] + lo;
    const uint64_t M = (uint64_t)(w[DS_E] - len);

    const uint64_t step = (uint64_t)(step_ptr ? *step_ptr : a.step);
    const uint64_t grow = (uint64_t)(a.row0 + b);
    uint32_t r[4];
    philox4x32_10((uint32_t)pair | ((uint32_t)a.mode << 31), (uint32_t)grow, (uint32_t)step, (uint32_t)(step >> 32),
                  (uint32_t)a.seed, (uint32_t)(a.seed >> 32), r);
    const int64_t u0 = (int64_t)__umul64hi((uint64_t)r[0] | ((uint64_t)r[1] << 32), M);
    const int64_t u1 = (int64_t)__umul64hi((uint64_t)r[2] | ((uint64_t)r[3] << 32), M);

    // j = #{i : L[i] - i <= u} for both slots: the answer stays in [base, base + n], n the same for every lane
    int64_t j0 = 0, j1 = 0;
    if (len > 0) {
        int64_t n = len;
        while (n > 1) {
            const int64_t half = n >> 1;
            const int64_t m0 = j0 + half - 1, m1 = j1 + half - 1;
            const int64_t v0 = L[m0], v1 = L[m1];
            j0 = v0 - m0 <= u0 ? j0 + half : j0;
            j1 = v1 - m1 <= u1 ? j1 + half : j1;
            n -= half;
        }
        const int64_t v0 = L[j0], v1 = L[j1];
        j0 += v0 - j0 <= u0 ? 1 : 0;
        j1 += v1 - j1 <= u1 ? 1 : 0;
    }
    if (n0 + 1 < a.N && a.vec) {
        *(longlong2*)(nrow + n0) = make_longlong2(u0 + j0, u1 + j1);
    } else {
        nrow[n0] = u0 + j0;
        if (n0 + 1 < a.N) nrow[n0 + 1] = u1 + j1;
    }
}

}  // namespace

extern "C" int kge_dsampler_sample(const void* blob, int64_t blob_bytes, const int64_t* idx, int64_t B, int64_t N,
                                   int64_t row0, int mode, uint64_t seed, int64_t step, const int64_t* step_ptr,
                                   int64_t* pos, int64_t* neg, int64_t neg_ld, float* weight, void* stream) {
    if (mode != KGE_HEAD_BATCH && mode != KGE_TAIL_BATCH)
        return set_error(KGE_EINVAL, "kge_dsampler_sample: mode must be 0 (head-batch) or 1 (tail-batch)");
    if (B < 0 || N < 0 || N > INT32_MAX || row0 < 0 || row0 > ((int64_t)1 << 32) - B)
        return set_error(KGE_EINVAL, "kge_dsampler_sample: bad shape (B, N >= 0, N < 2^31, row0 + B <= 2^32)");
    if (neg_ld < N) return set_error(KGE_EINVAL, "kge_dsampler_sample: neg_ld < N");
    if (B == 0 || N == 0) return 0;
    if (!blob || !idx || !pos || !neg || !weight) return set_error(KGE_EINVAL, "kge_dsampler_sample: null pointer");
    if (blob_bytes < (int64_t)kDsHdrWords * 8 || ((uintptr_t)blob & 7))
        return set_error(KGE_EINVAL, "kge_dsampler_sample: blob shorter than its header or not 8-B aligned");
    DsArgs a;
    a.blob_words = blob_bytes / 8;
    a.step = step;
    a.seed = seed;
    a.B = B;
    a.N = N;
    a.row0 = row0;
    a.pos = pos;
    a.neg = neg;
    a.neg_ld = neg_ld;
    a.weight = weight;
    a.mode = mode;
    a.wpr = (int)((N + 127) / 128);
    a.vec = ((uintptr_t)neg & 15) == 0 && (neg_ld & 1) == 0;
    const int64_t blocks = (B * a.wpr + kDsBlock / 64 - 1) / (kDsBlock / 64);
    if (blocks > INT32_MAX) return set_error(KGE_EINVAL, "kge_dsampler_sample: grid too large");
    hipLaunchKernelGGL(dsampler_kernel, dim3((unsigned)blocks), dim3(kDsBlock), 0, (hipStream_t)stream,
                       (const int64_t*)blob, idx, step_ptr, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return set_error(KGE_EHIP, (std::string("kge_dsampler_sample: ") + hipGetErrorString(e)).c_str());
    return 0;
}
