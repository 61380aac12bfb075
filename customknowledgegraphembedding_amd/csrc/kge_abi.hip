// kge_abi.hip — the C-ABI of libkge_hip.so (include/kge_hip.h): argument checking, kernel
// selection, the per-row reduction kernels and the extern "C" entry points.
#include <string.h>

#include <algorithm>
#include <cmath>

#include <string>

#include "kge_device.h"
#include "kge_scan.h"

namespace kge_impl {
namespace {

// ---------------------------------------------------------------------------------------------
// Per-row reductions (model.py:145, 168-171, 195-198; upstream train_step). One wave per row.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void neg_reduce_kernel(const float* __restrict__ s, int64_t B, int64_t N,
                                                            int64_t ld, float T, int adversarial,
                                                            float* __restrict__ out) {
    const int64_t b = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    const float res = row_reduce_fast(s + b * ld, N, T, adversarial, lane);
    if (lane == 0) out[b] = res;
}

// kge_step_forward's XCD-sliced form: the row reductions after step_fwd_xcd_kernel (one wave per row)
__global__ __launch_bounds__(kBlock) void neg_rows_kernel(ScoreParams p) {
    const int64_t b = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (b >= p.B) return;
    const int lane = threadIdx.x & 63;
    const float* row = p.out + b * p.out_ld;
    const float r = row_reduce_fast(row, p.N, p.temperature, p.adversarial, lane);
    if (lane == 0) p.out_neg[b] = r;
}

// With `ps` set it also writes the positive branch's d_ps[b] = d_out_pos[b] * sigmoid(-ps[b])
// (logsigmoid backward, model.py:145), saving the separate launch in the train step.
__global__ __launch_bounds__(kBlock) void neg_reduce_bwd_kernel(const float* __restrict__ s, int64_t B, int64_t N,
                                                                int64_t ld, float T, int adversarial, int detach,
                                                                const float* __restrict__ d_out,
                                                                float* __restrict__ d_s, int64_t d_ld,
                                                                const float* __restrict__ ps,
                                                                const float* __restrict__ d_out_pos,
                                                                float* __restrict__ d_ps) {
    const int64_t b = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    if (ps && lane == 0) d_ps[b] = d_out_pos[b] * sigmoidf(-ps[b]);
    neg_row_bwd(s + b * ld, N, T, adversarial, detach, d_out[b], d_s + b * d_ld, lane);
}

__global__ __launch_bounds__(kBlock) void log_sigmoid_kernel(const float* __restrict__ x, int64_t n,
                                                             float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = log_sigmoid(x[i]);
}

// Weighted train-step loss of supervisor.py:19-23 and its gradient, one block, fixed reduction order:
//   loss = (-sum(w * pos) / sum(w) - sum(w * neg) / sum(w)) / 2,   d_out[b] = (-0.5 / sum(w)) * w[b]
constexpr int kLossBlock = 1024;
__global__ __launch_bounds__(kLossBlock) void step_loss_kernel(const float* __restrict__ out_neg,
                                                               const float* __restrict__ out_pos,
                                                               const float* __restrict__ w, int64_t B,
                                                               float* __restrict__ loss, float* __restrict__ d_out,
                                                               float* __restrict__ parts) {
    __shared__ float red[3][kLossBlock];
    const int t = threadIdx.x;
    float sw = 0.f, sp = 0.f, sn = 0.f;
    for (int64_t b = t; b < B; b += kLossBlock) {
        const float wb = w ? w[b] : 1.f;  // no weights (kge_train_step_reg's uni_weight): plain means
        sw += wb;
        sp += wb * out_pos[b];
        sn += wb * out_neg[b];
    }
    red[0][t] = sw;
    red[1][t] = sp;
    red[2][t] = sn;
    __syncthreads();
    for (int o = kLossBlock / 2; o > 0; o >>= 1) {
        if (t < o) {
            red[0][t] += red[0][t + o];
            red[1][t] += red[1][t + o];
            red[2][t] += red[2][t + o];
        }
        __syncthreads();
    }
    const float tw = red[0][0];
    if (t == 0 && loss) *loss = (-red[1][0] / tw + -red[2][0] / tw) / 2.f;
    if (t == 0 && parts) {  // positive_sample_loss, negative_sample_loss
        parts[0] = -red[1][0] / tw;
        parts[1] = -red[2][0] / tw;
    }
    if (d_out) {
        const float c = -0.5f / tw;
        for (int64_t b = t; b < B; b += kLossBlock) d_out[b] = c * (w ? w[b] : 1.f);
    }
}

__global__ void add_scalar_kernel(const float* __restrict__ x, float* __restrict__ acc) { *acc += *x; }

// ---------------------------------------------------------------------------------------------
// Value of the L3 ("N3") regulariser of kge_train_step_reg (model.py:4-44; upstream train_step):
// lambda (sum |entity|^3 + sum |relation|^3) over the tables as they were before the step's update, every
// sum in a fixed order (no float atomics).
//   reg_chunk_kernel: blocks [0, nb_ent) each sum kRegChunk of the per-wave partials phase 2 left of the entity
//     rows it held; the blocks after them each sum |x|^3 over kRegChunk elements of the relation table (the
//     table's width of every row, never the padding), BEFORE bwd_rel_kernel updates it in place.
//   reg_finish_kernel: one block sums the chunk sums in index order, adds the term to the loss (and the loss to
//     the running Sum metric) and writes upstream's log {loss, positive_sample_loss, negative_sample_loss,
//     regularization}.
// ---------------------------------------------------------------------------------------------
constexpr int kRegChunk = 4096;
__device__ __forceinline__ float block_tree_sum(float s, float* red, int t) {
    red[t] = s;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(kBlock) void reg_chunk_kernel(const float* __restrict__ part, int64_t nparts,
                                                           int64_t nb_ent, const float* __restrict__ rel,
                                                           int64_t rel_ld, int64_t rel_dim, int64_t nrel,
                                                           float* __restrict__ out) {
    __shared__ float red[kBlock];
    const int t = threadIdx.x;
    float s = 0.f;
    if ((int64_t)blockIdx.x < nb_ent) {
        const int64_t lo = (int64_t)blockIdx.x * kRegChunk, hi = min(nparts, lo + kRegChunk);
        for (int64_t i = lo + t; i < hi; i += kBlock) s += part[i];
    } else {
        const int64_t lo = ((int64_t)blockIdx.x - nb_ent) * kRegChunk, hi = min(nrel, lo + kRegChunk);
        for (int64_t i = lo + t; i < hi; i += kBlock) {
            const int64_t r = i / rel_dim;
            const float x = fabsf(rel[r * rel_ld + (i - r * rel_dim)]);
            s += x * x * x;
        }
    }
    s = block_tree_sum(s, red, t);
    if (t == 0) out[blockIdx.x] = s;
}

__global__ __launch_bounds__(kBlock) void reg_finish_kernel(const float* __restrict__ chunk, int64_t nchunks,
                                                            float lambda, const float* __restrict__ parts,
                                                            float* __restrict__ loss, float* __restrict__ loss_sum,
                                                            float* __restrict__ log) {
    __shared__ float red[kBlock];
    const int t = threadIdx.x;
    float s = 0.f;
    for (int64_t i = t; i < nchunks; i += kBlock) s += chunk[i];
    s = block_tree_sum(s, red, t);
    if (t != 0) return;
    const float reg = nchunks > 0 ? lambda * s : 0.f;
    const float total = *loss + reg;  // upstream: loss = loss + regularization, before backward() and the log
    *loss = total;
    if (loss_sum) *loss_sum += total;
    if (log) {
        log[0] = total;
        log[1] = parts[0];
        log[2] = parts[1];
        log[3] = reg;
    }
}

__global__ __launch_bounds__(kBlock) void log_sigmoid_bwd_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ d_out, int64_t n,
                                                                 float* __restrict__ d_x) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) d_x[i] = d_out[i] * sigmoidf(-x[i]);
}

// ---------------------------------------------------------------------------------------------
// Dense Adam over a whole table (supervisor.py:26 optimizer.apply_gradients; run.py:111 Keras Adam).
//   keras: m += (g - m)(1 - b1); v += (g^2 - v)(1 - b2); p -= m * alpha / (sqrt(v) + eps),
//          alpha = lr * sqrt(1 - b2^t) / (1 - b1^t)
//   torch: m = lerp(m, g, 1 - b1); v = v * b2 + (1 - b2) g^2;
//          p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// HBM-bound elementwise pass: 16-B loads/stores, grid-stride; optionally zeroes the gradient.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void adam_one(float& p, float& g, float& m, float& v, const AdamArgs& a) {
    adam_update(p, g, m, v, a.b1, a.b2, a.eps, a.alpha, a.step_size, a.bc2_sqrt, a.keras);
    if (a.zero_grad) g = 0.f;
}

// one thread per 2 float4 (8 floats): all eight 16-B loads issued before any math
constexpr int kAdamVec = 2;

// Streamed (touch-once) float4 i of a table: nontemporal loads and stores. On gfx950 nt on both
// sides lifts a 3-read/3-write stream from ~4.9 to ~5.4 TB/s (profiles/r01_stream_probe_nt.txt).
typedef float f4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 nt_ld4(const float* base, int64_t i) {
    const f4v x = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(base) + i);
    return make_float4(x[0], x[1], x[2], x[3]);
}
__device__ __forceinline__ void nt_st4(float* base, int64_t i, const float4& v) {
    const f4v x = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(x, reinterpret_cast<f4v*>(base) + i);
}

__global__ __launch_bounds__(kBlock) void adam_kernel(float* __restrict__ p, float* __restrict__ g,
                                                      float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                      AdamArgs a) {
    const int64_t n4 = n / 4;
    const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kAdamVec;
    float4 P[kAdamVec], G[kAdamVec], M[kAdamVec], Vv[kAdamVec];
#pragma unroll
    for (int u = 0; u < kAdamVec; ++u) {
        const int64_t i = i0 + u;
        if (i < n4) {
            P[u] = nt_ld4(p, i);
            G[u] = nt_ld4(g, i);
            M[u] = nt_ld4(m, i);
            Vv[u] = nt_ld4(v, i);
        }
    }
#pragma unroll
    for (int u = 0; u < kAdamVec; ++u) {
        const int64_t i = i0 + u;
        if (i < n4) {
            adam_one(P[u].x, G[u].x, M[u].x, Vv[u].x, a);
            adam_one(P[u].y, G[u].y, M[u].y, Vv[u].y, a);
            adam_one(P[u].z, G[u].z, M[u].z, Vv[u].z, a);
            adam_one(P[u].w, G[u].w, M[u].w, Vv[u].w, a);
            nt_st4(p, i, P[u]);
            nt_st4(m, i, M[u]);
            nt_st4(v, i, Vv[u]);
            if (a.zero_grad) nt_st4(g, i, G[u]);
        }
    }
    if (blockIdx.x == 0)  // scalar tail (n % 4)
        for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += kBlock) adam_one(p[i], g[i], m[i], v[i], a);
}

// The same update for buffers that are not all 16-byte aligned (e.g. a parameter that is an offset
// view of a larger allocation): dword accesses, grid-stride. Bitwise the same per element.
__global__ __launch_bounds__(kBlock) void adam_scalar_kernel(float* __restrict__ p, float* __restrict__ g,
                                                             float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                             AdamArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
        adam_one(p[i], g[i], m[i], v[i], a);
}

// ---------------------------------------------------------------------------------------------
// Owned-row gather of a row-sharded table: out[i] = table[ids[i*stride] - lo] if this shard owns
// the id, else zeros (so a SUM all-reduce over shards assembles the rows exactly). One wave per row.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void gather_owned_kernel(const float* __restrict__ tab, int64_t rows, int64_t ld,
                                                              int64_t lo, const int64_t* __restrict__ ids,
                                                              int64_t stride, int64_t n, int64_t width,
                                                              float* __restrict__ out, int64_t out_ld, int vec4) {
    const int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (i >= n) return;
    const int lane = threadIdx.x & 63;
    const int64_t id = ids[i * stride] - lo;
    const bool ok = id >= 0 && id < rows;
    const float* src = tab + (ok ? id : 0) * ld;
    float* dst = out + i * out_ld;
    if (vec4) {
        const rsrc_t r = make_rsrc(src, ok ? (uint32_t)(width * 4) : 0u);
        for (int64_t e = (int64_t)lane * 4; e < width; e += 4 * kWave) {
            const vecf<4> v = bload<4>(r, (uint32_t)(e * 4));
            *reinterpret_cast<vecf<4>*>(dst + e) = v;
        }
    } else {
        for (int64_t e = lane; e < width; e += kWave) dst[e] = ok ? src[e] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------
// Gradient events of the deterministic backward, bucketed by entity (counting sort).
//   code in [0, BN)            negative candidate (b = code / N, n = code % N)  key neg[b, n]
//   code in [BN, BN+B)         positive candidate of row b (single mode)        key pos[b, 2]
//   code in [BN+B, BN+2B)      query-entity gradient of the negative call's b   key pos[b, 2|0]
//   code in [BN+2B, BN+3B)     query-entity (h) gradient of the positive call   key pos[b, 0]
// ---------------------------------------------------------------------------------------------
struct EvArgs {
    const int64_t* pos;
    const int64_t* neg;
    int64_t neg_ld, B, N, E;
    int qcol;  // query-entity column of the negative call: 2 (head-batch) or 0
    int total;
};

__device__ __forceinline__ int64_t ev_key(const EvArgs& a, int code) {
    const int64_t BN = a.B * a.N;
    if (code < BN) return a.neg[(code / a.N) * a.neg_ld + code % a.N];
    int64_t b = code - BN;
    if (b < a.B) return a.pos[b * 3 + 2];
    b -= a.B;
    if (b < a.B) return a.pos[b * 3 + a.qcol];
    b -= a.B;
    return a.pos[b * 3 + 0];
}

__global__ __launch_bounds__(kBlock) void ev_count_kernel(EvArgs a, int* __restrict__ count) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.total) return;
    const int64_t k = ev_key(a, i);
    if (k >= 0 && k < a.E) atomicAdd(&count[k], 1);
}

__global__ __launch_bounds__(kBlock) void ev_scatter_kernel(EvArgs a, int* __restrict__ cursor, int* __restrict__ code) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.total) return;
    const int64_t k = ev_key(a, i);
    if (k >= 0 && k < a.E) {
        const int at = atomicAdd(&cursor[k], 1);
        if (at >= 0 && at < a.total) code[at] = i;
    }
}

// Relation gradient: one block per (relation, 64-column chunk). Its four waves split the slots (a
// quarter each), find the slots that use the relation 64 at a time (ballot) and add their rows in
// slot order with 8 rows' loads in flight; the partials are combined in wave order (deterministic).
// With `ra.on` the block then applies Adam to its 64 columns of the relation table in place (the
// dense optimizer of supervisor.py:26: columns no score function reads get a zero gradient).
struct RelAdam {
    float *p, *m, *v;
    AdamArgs a;
    int on;
    float reg3;  // 3 lambda of the L3 regulariser: every column of the table's width gets reg3 x |x| (0: off)
};

constexpr int kRelWaves = 16;  // waves per relation chunk: each scans 1/16 of the slots (fewer dependent rounds)
// LAZY (kge_train_step_lazy; needs ra.on): a block whose relation none of the 2B slots uses leaves its columns and
// their moments as they are. Every wave scans its slots whether or not its chunk holds used columns, and the waves'
// ballots are OR-ed block-wide. A template parameter: the dense instance is the code it was.
template <bool LAZY>
__global__ __launch_bounds__(kRelWaves * kWave) void bwd_rel_kernel(const int64_t* __restrict__ pos, int64_t B, int64_t R,
                                                         const float* __restrict__ qg_rel, int64_t rel_w,
                                                         int64_t rel_off, float* __restrict__ d_rel, int64_t rel_ld,
                                                         int64_t rel_dim, const float* __restrict__ dmod_part,
                                                         float* __restrict__ d_mod, RelAdam ra) {
    __shared__ float red[kRelWaves][kWave];
    __shared__ int hit_s[LAZY ? kRelWaves : 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0 && d_mod && dmod_part) {
        float m = 0.f;
        for (int64_t s = 0; s < 2 * B; ++s) m += dmod_part[s];
        *d_mod = m;
    }
    const int64_t chunks = (rel_dim + kWave - 1) / kWave;
    const int64_t rho = blockIdx.x / chunks;
    if (rho >= R) return;
    const int64_t c = (blockIdx.x - rho * chunks) * kWave + lane;  // column of the full relation row
    const bool used = c >= rel_off && c < rel_off + rel_w;
    const int64_t cu = c - rel_off;
    const int64_t S = 2 * B, per = (S + kRelWaves - 1) / kRelWaves;
    const int64_t s_lo = w * per, s_hi = min(S, s_lo + per);
    float acc = 0.f;
    bool hit = false;
    (void)hit;
    if (LAZY || __ballot(used)) {
        for (int64_t s0 = s_lo; s0 < s_hi; s0 += kWave) {
            const int64_t s = s0 + lane;
            unsigned long long m = __ballot(s < s_hi && pos[(s % B) * 3 + 1] == rho);  // slot s: row s % B
            if constexpr (LAZY) hit = hit || m != 0ull;
            while (m) {
                float v[8];
                int nv = 0;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    v[u] = 0.f;
                    if (m) {
                        const int bit = __builtin_ctzll(m);
                        m &= m - 1;
                        v[u] = used ? qg_rel[(s0 + bit) * rel_w + cu] : 0.f;
                        ++nv;
                    }
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (u < nv) acc += v[u];
            }
        }
    }
    red[w][lane] = acc;
    if constexpr (LAZY) {
        if (lane == 0) hit_s[w] = hit ? 1 : 0;
    }
    __syncthreads();
    if constexpr (LAZY) {
        int any = 0;
#pragma unroll
        for (int ww = 0; ww < kRelWaves; ++ww) any |= hit_s[ww];
        if (!any) return;  // untouched relation: nothing of it is read or written
    }
    if (w != 0 || c >= rel_dim) return;
    float g = 0.f;
#pragma unroll
    for (int ww = 0; ww < kRelWaves; ++ww) g += red[ww][lane];
    g = used ? g : 0.f;  // parts no score function reads get 0
    if (ra.on) {
        const int64_t e = rho * rel_ld + c;
        float p = ra.p[e], m = ra.m[e], v = ra.v[e];
        if (ra.reg3 != 0.f) g += ra.reg3 * (p * fabsf(p));  // the unread parts too: their data gradient is 0
        adam_update(p, g, m, v, ra.a.b1, ra.a.b2, ra.a.eps, ra.a.alpha, ra.a.step_size, ra.a.bc2_sqrt, ra.a.keras);
        ra.p[e] = p;
        ra.m[e] = m;
        ra.v[e] = v;
    } else {
        d_rel[rho * rel_ld + c] = g;
    }
}

// ---------------------------------------------------------------------------------------------
// Combine (between the two collectives; one wave per global batch row b): the merged row state and
// this shard's share of the negative slot's query gradient, scaled by the loss weight:
//   TF (RED 2):     go f_r (A_r - T R B_r) / Z      detached (1): go f_r A_r / Z      mean (0): go A_r / N
// Also the forward's outputs for every row: out_neg = R (the reduced negative branch), the positive's
// raw score and logsigmoid. Every rank computes identical merged values (same inputs, same order).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void shard_combine_kernel(ScoreParams p) {
    const int64_t b = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (b >= p.B) return;
    const int lane = threadIdx.x & 63;
    const RowMerge r = merge_row(p, b);
    const float go = home_loss_weight(p, b, lane);
    const bool mean = !p.adversarial;
    const float R = mean ? r.Ln / (float)p.N : (r.Z > 0.f ? r.Ln / r.Z : 0.f);
    float ca = 0.f, cb = 0.f;
    if (mean) {
        ca = go / (float)p.N;
    } else if (r.Z > 0.f) {
        ca = go * r.f_me / r.Z;
        if (!p.detach) cb = -ca * (p.temperature * R);
    }
    const int64_t w = (int64_t)p.nq * p.D;
    const float* A = p.sh_A + b * w;
    const float* Bv = p.sh_B + b * w;
    float* dq = p.sh_dq + b * w;
    for (int64_t i = lane; i < w; i += kWave) {
        float v = ca * A[i];
        if (cb != 0.f) v += cb * Bv[i];
        dq[i] = v;
    }
    if (lane == 0) {
        float* m = p.sh_merged + b * 4;
        m[0] = r.M;
        m[1] = r.Z;
        m[2] = R;
        m[3] = r.pos;
        p.out_neg[b] = R;
        if (p.out_pos_raw) p.out_pos_raw[b] = r.pos;
        p.out_pos_ls[b] = log_sigmoid(r.pos);
    }
}

// ---------------------------------------------------------------------------------------------
// host helpers
// ---------------------------------------------------------------------------------------------
thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

int ok() {
    g_last_error.clear();
    return 0;
}

int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(KGE_EHIP, std::string(what) + ": " + hipGetErrorString(e));
    return ok();
}

bool aligned(const void* ptr, int bytes) { return ptr == nullptr || ((uintptr_t)ptr % (uintptr_t)bytes) == 0; }

// membership, not a range: id 6 is unassigned
bool valid_fn(int fn) {
    switch (fn) {
        case KGE_TRANSE:
        case KGE_DISTMULT:
        case KGE_COMPLEX:
        case KGE_ROTATE:
        case KGE_INTERHT:
        case KGE_PROTATE:
        case KGE_PAIRRE: return true;
        default: return false;
    }
}

// PairRE reads both relation halves, at rel_off and rel_off + D: a row stride that does not hold them is refused
// (every other function keeps its unchecked strides)
int check_rel_width(int fn, int64_t D, int64_t rel_off, int64_t rel_ld) {
    if (fn == KGE_PAIRRE && (rel_off < 0 || rel_ld < rel_off + 2 * D))
        return fail(KGE_EINVAL, "PairRE relation rows hold two halves: rel_ld >= rel_off + 2 D");
    return 0;
}

// the row-sharded family has no PairRE kernels (kKinds' no_pairre): refused ahead of any device call
int refuse_sharded(int fn, const char* who) {
    if (fn == KGE_PAIRRE) return fail(KGE_ENOTSUP, std::string(who) + ": PairRE has no row-sharded form");
    return 0;
}

// ---------------------------------------------------------------------------------------------
// The problem of a call. Each entry point builds these once from its arguments, in the C-ABI's argument
// order; everything below it takes them by const reference. Host only: never a kernel argument.
// ---------------------------------------------------------------------------------------------
struct Tables {  // the score function, its embedding tables and constants
    int fn;
    const float* ent;
    int64_t nentity, ent_ld;
    const float* rel;
    int64_t nrelation, rel_ld, rel_off;
    int64_t D;
    float gamma, emb_range, modulus;
};
struct Batch {  // the triples scored
    int mode;
    const int64_t* pos;
    const int64_t* neg;
    int64_t neg_ld, B, N;
};
// the loss side of kge_step_backward: the forward's scores, the loss' gradients, where the table gradients go
struct StepGrads {
    float temperature;
    int adversarial, detach;
    const float* neg_scores;
    int64_t ns_ld;
    const float* pos_scores;
    const float* d_out_neg;
    const float* d_out_pos;
    float* d_ent;
    float* d_rel;
    float* d_modulus;
    const float* cand_stats;
};

// widest vector width every operand allows, then the groups-per-lane bucket. The sharded train step's positive
// query rows (qent_pos, q_ld) and query-gradient buffer (sh_dq, rows of nq D floats) are read and written with
// the same width, so they count when set.
int pick_vg(const ScoreParams& p, int& V, int& G) {
    const int cand[3] = {4, 2, 1};
    V = 1;
    for (int v : cand) {
        if (p.D % v == 0 && p.q_ld % v == 0 && p.r_ld % v == 0 && p.r_off % v == 0 && p.c_ld % v == 0 &&
            aligned(p.qent, 4 * v) && aligned(p.rel, 4 * v) && aligned(p.cent, 4 * v) &&
            aligned(p.qent_pos, 4 * v) && aligned(p.sh_dq, 4 * v)) {
            V = v;
            break;
        }
    }
    const int groups = (p.D / V + kWave - 1) / kWave;
    G = 1;
    while (G < groups) G <<= 1;
    if (G > kMaxG)
        return fail(KGE_ENOTSUP, "per-half dim " + std::to_string(p.D) + " exceeds the register-resident limit " +
                                     std::to_string(kMaxG * kWave * V) + " for vector width " + std::to_string(V));
    return 0;
}

// candidates per wave: long runs amortise the per-wave query build; keep >= 8192 waves in flight
int pick_cpw(int64_t B, int64_t N) {
    if (N <= 1) return 1;
    int64_t cpw = 16;
    while (cpw > 4 && B * ((N + cpw - 1) / cpw) < 8192) cpw >>= 1;
    return (int)cpw;
}

int pick_cpw_sharded(int64_t B, int64_t N) {
    if (N <= 1) return 1;
    int64_t cpw = 512;
    while (cpw > 16 && B * ((N + cpw - 1) / cpw) < 8192) cpw >>= 1;
    return (int)cpw;
}

int dispatch(int fn, const ScoreParams& p, int kind, hipStream_t st, int blocks, bool ch, int V, int G) {
    switch (fn) {
        case KGE_TRANSE: return launch_transe(p, kind, st, blocks, ch, V, G);
        case KGE_DISTMULT: return launch_distmult(p, kind, st, blocks, ch, V, G);
        case KGE_COMPLEX: return launch_complex(p, kind, st, blocks, ch, V, G);
        case KGE_ROTATE: return launch_rotate(p, kind, st, blocks, ch, V, G);
        case KGE_INTERHT: return launch_interht(p, kind, st, blocks, ch, V, G);
        case KGE_PROTATE: return launch_protate(p, kind, st, blocks, ch, V, G);
        case KGE_PAIRRE: return launch_pairre(p, kind, st, blocks, ch, V, G);
        default: return KGE_EINVAL;
    }
}

int check_fn_mode(int fn, int mode) {
    if (mode != KGE_HEAD_BATCH && mode != KGE_TAIL_BATCH && mode != KGE_SINGLE)
        return fail(KGE_EINVAL, "mode must be 0 (head-batch), 1 (tail-batch) or 3 (single)");
    if (!valid_fn(fn)) return fail(KGE_EINVAL, "unknown score function id " + std::to_string(fn));
    return 0;
}

int run_score(int fn, int mode, ScoreParams& p, int kind, void* stream) {
    int rc = check_fn_mode(fn, mode);
    if (rc) return rc;
    if (p.B < 0 || p.N < 0 || p.D <= 0) return fail(KGE_EINVAL, "bad shape (B, N, D)");
    // (an empty candidate list still ranks: kge_eval_rank_candidates writes rank 1 for every row)
    if (p.B == 0 || (p.N == 0 && kind != KIND_RANK_CAND)) return ok();
    // a rank of the sharded train step that owns no rows has no shard to point at: nothing reads p.cent then
    const bool no_rows =
        p.c_rows == 0 && (kind == KIND_SHARD_FWD_GRAD || kind == KIND_SHARD_POS || kind == KIND_SHARD_EPILOGUE);
    rc = check_rel_width(fn, p.D, p.r_off, p.r_ld);
    if (rc) return rc;
    if (!p.qent || !p.rel || (!p.cent && !no_rows)) return fail(KGE_EINVAL, "null table pointer");
    int V = 1, G = 1;
    rc = pick_vg(p, V, G);
    if (rc) return rc;
    if (kind == KIND_BWD) {
        // backward: dword-per-lane layout (lane l owns elements l + 64k) so the gradient atomics are
        // 256-B contiguous per wave-instruction; falls back to the forward layout past D = 1024
        int g1 = 1;
        while (g1 * kWave < p.D) g1 <<= 1;
        if (g1 <= kBwdMaxG) {
            V = 1;
            G = g1;
        }
    }
    const KindInfo& k = kKinds[kind];
    int64_t waves = 0;
    switch (k.grid) {
        case GRID_WAVE_PER_ROW:
            if (kind == KIND_FINISH) p.cpw = p.wpr = 1;
            waves = p.B;  // one wave per slot / batch row
            break;
        case GRID_BLOCK_PER_ROW: waves = p.B * kWavesPerBlock; break;
        // (the lazy step's phase 2: one wave / block per entry of the touched rows' list)
        case GRID_WAVE_PER_ENT: waves = p.lz_list ? p.lz_rows : p.c_rows; break;
        case GRID_BLOCK_PER_ENT: waves = (p.lz_list ? p.lz_rows : p.c_rows) * kWavesPerBlock; break;
        case GRID_XCD_SLICES:
            waves = (p.B + kWavesPerBlock - 1) / kWavesPerBlock * kWavesPerBlock * 8;
            if (kind == KIND_STEP_FWD_XCD && p.xcd_phases > 1) waves *= p.xcd_phases;
            break;
        case GRID_TILE_GROUPS: {
            if (p.tile_rows < 1 || p.tile_lds > kTileLdsMax) return fail(KGE_EINVAL, "tile plan missing");
            // one block of tile_waves waves per (group of tile_rows batch rows, entity slice): run_score's
            // block count is waves / kWavesPerBlock; then, for a planned step, one tail block per group of the
            // next batch's plan
            const int64_t groups = (p.B + p.tile_rows - 1) / p.tile_rows;
            p.tile_blocks = (int)(groups * 8);
            waves = (groups * 8 + (p.tile_next.plan ? p.tile_plan_blocks : 0)) * kWavesPerBlock;
            break;
        }
        case GRID_CAND_PER_WAVE:
            // sharded scoring compacts each wave's owned candidates: long runs (up to 512 ids, ~64 owned
            // at 8 shards) keep the per-wave query build amortised; >= 8192 waves still fill the chip
            p.cpw = p.skip_foreign ? pick_cpw_sharded(p.B, p.N) : pick_cpw(p.B, p.N);
            p.wpr = (int)((p.N + p.cpw - 1) / p.cpw);
            waves = p.B * p.wpr;
            break;
        case GRID_STEP_EPILOGUE: {
            // one wave per slot (negative rows' chains, positives, negative rows' score gradients), then the
            // event-scatter blocks (about four codes per thread, at most 256 blocks), then one block for the loss
            const int64_t ev = p.B * p.N + 3 * p.B;
            const int64_t sb = std::min<int64_t>(std::max<int64_t>((ev + 4 * kBlock - 1) / (4 * kBlock), 1), 256);
            waves = (3 * p.B + kWavesPerBlock - 1) / kWavesPerBlock * kWavesPerBlock + (sb + 1) * kWavesPerBlock;
            break;
        }
        case GRID_SHARD_EPILOGUE:
            // one wave per slot (negative rows, then positives), then one block for the loss
            waves = (2 * p.B + kWavesPerBlock - 1) / kWavesPerBlock * kWavesPerBlock + kWavesPerBlock;
            break;
        case GRID_RANK_PAIRS: waves = p.B + p.rk.nf; break;
        case GRID_RANK_SWEEP:
            // run_score's block count is waves / kWavesPerBlock (the blocks themselves have kSweepWaves waves)
            if (p.tile_rows < 1 || p.rk.chunks < 1 || p.tile_lds > kTileLdsMax) return fail(KGE_EINVAL, "sweep plan missing");
            waves = (p.B + p.tile_rows - 1) / p.tile_rows * 8 * p.rk.chunks * kWavesPerBlock;
            break;
        case GRID_TOPK_SWEEP:
            if (p.tile_rows < 1 || p.tk.chunks < 1 || p.tile_lds > kTileLdsMax || p.tk.k < 1 || p.tk.k > kTopkMax || !p.tk.parts)
                return fail(KGE_EINVAL, "sweep plan missing");
            waves = (p.B + p.tile_rows - 1) / p.tile_rows * 8 * p.tk.chunks * kWavesPerBlock;
            break;
        case GRID_RANK_CAND: {
            p.wpr = rank_cand_wpr(p.N);
            const int64_t rows = kWavesPerBlock / p.wpr;  // query rows per block
            waves = (p.B + rows - 1) / rows * kWavesPerBlock;
            break;
        }
    }
    const int64_t blocks = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
    if (blocks > INT32_MAX) return fail(KGE_EINVAL, "problem too large for one launch");
    const bool ch = k.ch && mode == KGE_HEAD_BATCH;
    if (k.no_protate && (G > k.max_g || fn == KGE_PROTATE))
        return fail(KGE_ENOTSUP, "the fused forward + query gradient needs D / V <= 256 and no pRotatE");
    if (G > k.max_g) return fail(KGE_ENOTSUP, "dimension too large");
    if (k.g_whole_waves && G % kWavesPerBlock) return fail(KGE_ENOTSUP, "the streaming backward needs G % 4 == 0");
    // a (kind, function, side, V, G) without an instantiation launches nothing and says so
    rc = kind_has(kind, fn, ch, G) ? dispatch(fn, p, kind, (hipStream_t)stream, (int)blocks, ch, V, G) : KGE_ENOTSUP;
    if (rc) return fail(rc, "no kernel for this (function, width) combination");
    return check_launch(k.what);
}

float phase_div_for(int fn, float emb_range) {
    // torch: tensor / (python float: emb_range.item() / pi) -> the divisor is rounded to fp32
    const double pi = (fn == KGE_PROTATE) ? 3.14159262358979323846 : 3.14159265358979323846;
    return (float)((double)emb_range / pi);
}

void fill_indexed(ScoreParams& p, const Tables& t, const Batch& b) {
    memset(&p, 0, sizeof(p));
    const bool ch = b.mode == KGE_HEAD_BATCH;
    p.qent = t.ent;
    p.q_idx = b.pos ? b.pos + (ch ? 2 : 0) : nullptr;
    p.q_ld = t.ent_ld;
    p.q_stride = 3;
    p.q_rows = t.nentity;
    p.rel = t.rel;
    p.r_idx = b.pos ? b.pos + 1 : nullptr;
    p.r_ld = t.rel_ld;
    p.r_stride = 3;
    p.r_rows = t.nrelation;
    p.r_off = t.rel_off;
    p.cent = t.ent;
    p.c_ld = t.ent_ld;
    p.c_rows = t.nentity;
    if (b.mode == KGE_SINGLE) {
        p.c_idx = b.pos ? b.pos + 2 : nullptr;
        p.c_stride = 3;
    } else {
        p.c_idx = b.neg;
        p.c_stride = b.neg_ld;
    }
    p.B = b.B;
    p.N = b.mode == KGE_SINGLE ? 1 : b.N;
    p.D = (int)t.D;
    p.gamma = t.gamma;
    p.phase_div = phase_div_for(t.fn, t.emb_range);
    p.modulus = t.modulus;
}
// the positive (single-mode) call over the same rows
Batch single_of(const Batch& b) { return {KGE_SINGLE, b.pos, nullptr, 0, b.B, 1}; }

void fill_dense(ScoreParams& p, int fn, int mode, const float* head, int64_t head_ld, const float* rel,
                int64_t rel_ld, int64_t rel_off, const float* tail, int64_t tail_ld, int64_t B, int64_t N, int64_t D,
                float gamma, float emb_range, float modulus) {
    memset(&p, 0, sizeof(p));
    const bool ch = mode == KGE_HEAD_BATCH;
    if (mode == KGE_SINGLE) N = 1;
    p.qent = ch ? tail : head;
    p.q_ld = ch ? tail_ld : head_ld;
    p.q_rows = B;
    p.rel = rel;
    p.r_ld = rel_ld;
    p.r_off = rel_off;
    p.r_rows = B;
    p.cent = ch ? head : tail;
    p.c_ld = ch ? head_ld : tail_ld;
    p.c_dense = N;
    p.c_rows = B * N;
    p.B = B;
    p.N = N;
    p.D = (int)D;
    p.gamma = gamma;
    p.phase_div = phase_div_for(fn, emb_range);
    p.modulus = modulus;
}

bool empty(int64_t B, int64_t N) { return B == 0 || N == 0; }

// phases of kge_step_forward's XCD-sliced order (step_fwd_xcd_kernel): forms->xcd_phases chooses (A/B runs)
int xcd_phases(int64_t nentity, int64_t ent_ld, const kge_forms* forms) {
    const int forced = forms ? forms->xcd_phases : 0;
    if (forced > 0) return std::min(forced, 16);
    // a table larger than the 256 MB Infinity Cache is swept in phases of ~96 MB (C2's 327.5 MB: 4 phases,
    // 139 -> 128.5 us); a table that fits gains nothing and pays the extra id walks (C3's 116 MB at 4
    // phases: 144 -> 162 us)
    const int64_t bytes = nentity * ent_ld * 4, mall = (int64_t)256 << 20, phase = (int64_t)96 << 20;
    if (bytes <= mall) return 1;
    return (int)std::min<int64_t>((bytes + phase - 1) / phase, 8);
}

// kge_step_forward's candidate order: 0 batch-row-major (KIND_STEP_FWD), 1 XCD-sliced ascending ids per wave
// (KIND_STEP_FWD_XCD), 2 row-group x XCD-slice tiles (KIND_STEP_FWD_TILE, when its LDS plan fits).
// forms->step_order chooses (A/B runs and the cross-form tests).
int step_order(int64_t nentity, int64_t N, const kge_forms* forms = nullptr) {
    const int forced = forms ? forms->step_order : -1;
    if (nentity >= (int64_t)8 << 25) return 0;  // sort keys hold (id - slice start) << 6
    if (forced >= 0 && forced <= 2) return forced;
    return N >= 128 ? 2 : 0;
}
bool use_xcd_order(int64_t nentity, int64_t N, const kge_forms* forms = nullptr) {
    return step_order(nentity, N, forms) != 0;
}

// Rows per block of the tile kernel (step_fwd_tile_kernel) and its dynamic LDS: 0 when the plan does not fit
// (then the XCD-sliced form runs). forms->tile_rows caps the row count, tile_waves / tile_q2slots choose.
int tile_plan(int fn, ScoreParams& p, const kge_forms* forms = nullptr) {
    int V = 1, G = 1;
    if (pick_vg(p, V, G)) return 0;
    if (G > kFwdGradMaxG || p.N + 1 > 65536 || p.c_rows <= 0) return 0;
    const int64_t opb = (int64_t)G * kWave * V * 4;  // bytes of one query operand image
    // InterHT: batch rows sorted by relation (B <= kTileSortMaxB), relation thirds in LDS slots
    int64_t P2 = 0;
    if (fn == KGE_INTERHT && p.B <= kTileSortMaxB) {
        P2 = kWave;
        while (P2 < p.B) P2 <<= 1;
    }
    // waves per block (each two candidate rows deep): 12 for candidate rows of 4 KB or more (3 waves per SIMD
    // at <= 168 VGPRs; C2 InterHT 105 -> 95 us and C3 RotatE 124-131 -> 115-120 us against 8 waves, whose
    // 2 waves per SIMD leave the score's VALU exposed; 16 spills), 16 for smaller rows (C4 DistMult: 2 KB rows
    // need the waves for bytes in flight). forms->tile_waves chooses (8, 12, 16).
    const int64_t row_bytes = (int64_t)p.D * 4 * (is_split(fn) ? 2 : 1);
    p.tile_waves = row_bytes >= 4096 ? 12 : 16;
    p.tile_depth = 2;  // (kge_step_planner_set_form chooses 1 for a planned step)
    const int fw = forms ? forms->tile_waves : 0;
    if (fw == 8 || fw == 12 || fw == 16) p.tile_waves = fw;
    const int64_t NT = (int64_t)p.tile_waves * kWave;
    const int64_t qrow = tile_nq(fn) * opb + 8 + 8 + 8 + 4, lrow = (p.N + 1) * 4;  // + rrow, brow, qid, q2slot
    const int64_t fixed = kTileBuckets * 4 + 16;
    // the list region also holds the relation sort's per-wave bucket counts ([ceil(kTileSortMaxB / NT) NWV][64],
    // step_fwd_tile_kernel step 0), sized for the block's actual wave count
    const int64_t sort_ints = P2 ? (kTileSortMaxB + NT - 1) / NT * p.tile_waves * kTileSortRel : 0;
    auto lds = [&](int64_t R, int64_t QS) { return R * qrow + QS * opb + fixed + std::max(R * lrow, sort_ints * 4); };
    int64_t R = kTileRows;
    if (forms && forms->tile_rows > 0) R = std::min<int64_t>(R, forms->tile_rows);
    while (R >= 1 && lds(R, 0) > kTileLdsMax) --R;
    if (R < 1) return 0;
    int64_t QS = 0;
    if (fn == KGE_INTERHT)
        while (QS < R && lds(R, QS + 1) <= kTileLdsMax) ++QS;
    if (forms && forms->tile_q2slots >= 0) QS = std::min<int64_t>(QS, forms->tile_q2slots);
#ifdef KGE_PROFILING_KNOBS
    // profiling-only A/B knobs (a build with -DKGE_PROFILING_KNOBS): KGE_TILE_DRY=<level> runs the setup alone and
    // writes no scores (unplanned: 1 = the rows' ids, 2 = + the query build, 3 = + the bucket counts, 4 = the whole
    // setup; a planned step: 1 = the prologue's first round trip, the plan's header, bounds and rows; 2 and above =
    // the whole prologue, through its one barrier); KGE_TILE_NOSORT keeps the batch-row order
    p.tile_dry = getenv("KGE_TILE_DRY") ? std::max(1, atoi(getenv("KGE_TILE_DRY"))) : 0;
    if (getenv("KGE_TILE_NOSORT")) P2 = 0;
#endif
    p.tile_rows = (int)R;
    p.tile_q2slots = (int)QS;
    p.tile_sort = (int)P2;
    p.tile_lds = (int)lds(R, QS);
    return 1;
}

// The tile parameters of a planned step (kge_step_plan / kge_step_forward_planned): tile_plan's choice for
// 16-B aligned tables of these shapes, so that a plan is made without the tables. Returns the rows per group
// (0: the tile form does not apply).
int planned_tile_params(const Tables& t, int64_t B, int64_t N, ScoreParams& p, const kge_forms* forms = nullptr) {
    if (B <= 0 || N <= 0 || t.D <= 0 || t.nentity <= 0 || t.nentity >= ((int64_t)1 << 31) || B >= ((int64_t)1 << 31))
        return 0;
    Tables a = t;
    a.ent = a.rel = reinterpret_cast<const float*>((uintptr_t)4096);
    fill_indexed(p, a, {KGE_TAIL_BATCH, nullptr, nullptr, 0, B, N});
    return tile_plan(t.fn, p, forms) ? p.tile_rows : 0;
}

// The LDS of a PLANNED instance at R rows per block (p.tile_waves set: tile_plan ran): the query images, the
// relation slots and the small arrays. Its sorted list is the plan's, in global memory, so tile_plan's list region
// (R (N + 1) ints, 16-65 KB) is not part of it, and InterHT's relation slots are counted again for the room that
// leaves (C2 at 16 rows: 3 -> 7; at 17 rows: 5). 0 when R rows do not fit, or are more than the prologue's two
// per wave. The tail blocks' plan_lds_ints are the launch's to add (step_forward_planned).
int planned_tile_layout(int fn, ScoreParams& p, int64_t R) {
    int V = 1, G = 1;
    if (pick_vg(p, V, G)) return 0;
    const int64_t opb = (int64_t)G * kWave * V * 4;
    const int64_t qrow = tile_nq(fn) * opb + 8 + 8 + 8 + 4, fixed = kTileBuckets * 4 + 16;
    auto lds = [&](int64_t r, int64_t qs) { return r * qrow + qs * opb + fixed; };
    if (R < 1 || R > std::min(kTileMaxRows, 2 * p.tile_waves) || lds(R, 0) > kTileLdsMax) return 0;
    int64_t QS = 0;
    if (fn == KGE_INTERHT)
        while (QS < R && lds(R, QS + 1) <= kTileLdsMax) ++QS;
    p.tile_rows = (int)R;
    p.tile_q2slots = (int)QS;
    p.tile_lds = (int)lds(R, QS);
    return 1;
}

// The planner's row rule (kge_step_planner_*): rows per group of a planned step whose launch also makes
// the next plan. The launch's plan blocks follow its 8 ceil(B / R) scoring blocks in the grid, so they start at
// once, beside the sweep, only where the scoring blocks leave CUs free. cap(R): the blocks of the step's instance
// resident at once, at R rows' LDS (0: unknown). Where the library's R0 rows fill the device
// (8 ceil(B / R0) > cap - 8) the answer is the smallest larger R that fits the planned LDS with at least the
// relation slots tile_plan gives R0, whose plan fits plan_bytes (0: any), and that leaves 8 CUs; R0 when there is
// none, or the capacity is unknown. waves: the step's waves per block.
template <class Cap>
int planned_rows_rule(const Tables& t, int64_t B, int64_t N, int waves, int64_t plan_bytes, Cap cap) {
    ScoreParams tp;
    const int R0 = planned_tile_params(t, B, N, tp);
    if (!R0) return 0;
    const int qs0 = tp.tile_q2slots;
    if (waves) tp.tile_waves = waves;
    const int64_t c0 = cap(R0);
    if (c0 <= 0 || 8 * plan_groups(B, R0) <= c0 - 8) return R0;
    for (int R = R0 + 1; R <= kTileMaxRows; ++R) {
        if (!planned_tile_layout(t.fn, tp, R) || tp.tile_q2slots < qs0) continue;
        if (plan_bytes > 0 && plan_words(B, N, R) * 4 > plan_bytes) continue;
        const int64_t c = cap(R);
        if (c > 0 && 8 * plan_groups(B, R) <= c - 8) return R;
    }
    return R0;
}

// The form of a planned step's sweep (kge_step_planner_set_form / _set_board / _set_lead): waves per block,
// candidate rows in flight per wave, and the lead throttle's board, tag and lead (board null: no throttle).
struct SweepForm {
    int waves, depth, lead, tag;
    int rev;  // sweep each block's sorted list in descending entity order (kge_step_planner_set_sweep)
    int* board;
    long long* clk;
};

// The library's sweep form of a planned step per candidate row width, as tile_plan's tile_waves is: what
// measured fastest against 12 x 2 / 16 x 2 without a board (scripts/window_probe.py).
void planned_sweep_defaults(int fn, int64_t D, int& waves, int& depth, int& lead) {
    const int64_t row_bytes = D * 4 * (is_split(fn) ? 2 : 1);
    waves = row_bytes >= 4096 ? 12 : 16;
    depth = 2;
    lead = 0;
    // only what was measured and passed (every round faster than every round of the form above, the median gain
    // more than twice that form's own range); every other function and width keeps the form above. Each was
    // measured at ONE shape (B 512, N 256, d 1000: 8 KB rows): other wide-row InterHT / RotatE shapes inherit it
    // unmeasured
    if (row_bytes >= 4096 && fn == KGE_INTERHT) lead = 12;  // C2 (WN18RR): 85.8 -> 82.6 us, leads 8 .. 16 within 1 us
    if (row_bytes >= 4096 && fn == KGE_ROTATE) depth = 1;   // C3 (FB15k-237): 64.8 -> 59.4 us (12 x 2, lead 8: 61.9)
}

PlanArgs plan_args(const ScoreParams& tp, const Tables& t, const Batch& b, void* plan) {
    PlanArgs a;
    a.pos = b.pos;
    a.neg = b.neg;
    a.neg_ld = b.neg_ld;
    a.B = b.B;
    a.N = b.N;
    a.nent = t.nentity;
    a.nrel = t.nrelation;
    a.mode = b.mode;
    a.R = tp.tile_rows;
    a.sort = tp.tile_sort != 0;
    a.plan = reinterpret_cast<int*>(plan);
    return a;
}

// the row reductions after a sliced or tiled scoring launch (kge_step_forward, kge_step_forward_planned)
int launch_neg_rows(const ScoreParams& p, const char* what, void* stream) {
    const int64_t blocks = (p.B + kWavesPerBlock - 1) / kWavesPerBlock;
    hipLaunchKernelGGL(neg_rows_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, p);
    return check_launch(what);
}

}  // namespace

int set_error(int code, const char* msg) { return fail(code, msg); }
}  // namespace kge_impl

using namespace kge_impl;

// =============================================================================================
// C-ABI
// =============================================================================================
extern "C" {

int kge_abi_version(void) { return KGE_ABI_VERSION; }

const char* kge_last_error(void) { return g_last_error.c_str(); }

int64_t kge_max_dim(int fn) {
    if (!valid_fn(fn)) return 0;
    return (int64_t)kMaxG * kWave * 4;
}

int kge_step_forward_order(int64_t nentity, int64_t N) { return step_order(nentity, N); }

int kge_score_indexed(int fn, int mode, const float* ent, int64_t nentity, int64_t ent_ld, const float* rel,
                      int64_t nrelation, int64_t rel_ld, int64_t rel_off, const int64_t* pos, const int64_t* neg,
                      int64_t neg_ld, int64_t B, int64_t N, int64_t D, float gamma, float emb_range, float modulus,
                      float* scores, int64_t scores_ld, void* stream) {
    return kge_score_indexed_ex(fn, mode, ent, nentity, ent_ld, rel, nrelation, rel_ld, rel_off, pos, neg, neg_ld, B,
                                N, D, gamma, emb_range, modulus, scores, scores_ld, nullptr, stream);
}

int kge_score_indexed_ex(int fn, int mode, const float* ent, int64_t nentity, int64_t ent_ld, const float* rel,
                         int64_t nrelation, int64_t rel_ld, int64_t rel_off, const int64_t* pos, const int64_t* neg,
                         int64_t neg_ld, int64_t B, int64_t N, int64_t D, float gamma, float emb_range, float modulus,
                         float* scores, int64_t scores_ld, const kge_forms* forms, void* stream) {
    int rc = check_fn_mode(fn, mode);
    if (rc) return rc;
    if (B < 0 || N < 0 || D <= 0) return fail(KGE_EINVAL, "bad shape (B, N, D)");
    if (empty(B, mode == KGE_SINGLE ? 1 : N)) return ok();
    if (!pos) return fail(KGE_EINVAL, "pos must not be NULL");
    if (mode != KGE_SINGLE && !neg) return fail(KGE_EINVAL, "neg must not be NULL in head/tail-batch mode");
    if (!scores) return fail(KGE_EINVAL, "scores must not be NULL");
    const Tables t = {fn, ent, nentity, ent_ld, rel, nrelation, rel_ld, rel_off, D, gamma, emb_range, modulus};
    ScoreParams p;
    fill_indexed(p, t, {mode, pos, neg, neg_ld, B, N});
    p.out = scores;
    p.out_ld = scores_ld;
    if (mode != KGE_SINGLE && nentity < ((int64_t)1 << 31) && use_xcd_order(nentity, N, forms)) {
        if (step_order(nentity, N, forms) == 2 && tile_plan(fn, p, forms))
            return run_score(fn, mode, p, KIND_SCORE_TILE, stream);  // row-group x XCD-slice tiles (§3.0)
        return run_score(fn, mode, p, KIND_SCORE_SHARD_XCD, stream);  // XCD-sliced gather order (§3.0)
    }
    return run_score(fn, mode, p, KIND_FWD, stream);
}

int kge_step_finish(int fn, const float* ent, int64_t nentity, int64_t ent_ld, const float* rel, int64_t nrelation,
                    int64_t rel_ld, int64_t rel_off, const int64_t* pos, int64_t B, int64_t D, float gamma,
                    float emb_range, float modulus, const float* neg_scores, int64_t N, int64_t ns_ld,
                    float temperature, int adversarial, float* out_neg, float* pos_scores, float* out_pos,
                    void* stream) {
    int rc = check_fn_mode(fn, KGE_SINGLE);
    if (rc) return rc;
    if (B < 0 || N <= 0 || D <= 0) return fail(KGE_EINVAL, "bad shape (B, N, D)");
    if (B == 0) return ok();
    if (!pos || !neg_scores || !out_neg || !out_pos) return fail(KGE_EINVAL, "null pointer");
    const Tables t = {fn, ent, nentity, ent_ld, rel, nrelation, rel_ld, rel_off, D, gamma, emb_range, modulus};
    ScoreParams f;
    fill_indexed(f, t, {KGE_SINGLE, pos, nullptr, 0, B, 1});
    f.neg_scores = neg_scores;
    f.ns_ld = ns_ld;
    f.n_neg = N;
    f.temperature = temperature;
    f.adversarial = adversarial;
    f.out_neg = out_neg;
    f.out_pos_raw = pos_scores;
    f.out_pos_ls = out_pos;
    return run_score(fn, KGE_SINGLE, f, KIND_FINISH, stream);
}

int kge_step_forward(int fn, int mode, const float* ent, int64_t nentity, int64_t ent_ld, const float* rel,
                     int64_t nrelation, int64_t rel_ld, int64_t rel_off, const int64_t* pos, const int64_t* neg,
                     int64_t neg_ld, int64_t B, int64_t N, int64_t D, float gamma, float emb_range, float modulus,
                     float temperature, int adversarial, float* neg_scores, int64_t ns_ld, float* out_neg,
                     float* pos_scores, float* out_pos, float* cand_stats, void* stream) {
    return kge_step_forward_ex(fn, mode, ent, nentity, ent_ld, rel, nrelation, rel_ld, rel_off, pos, neg, neg_ld, B, N,
                               D, gamma, emb_range, modulus, temperature, adversarial, neg_scores, ns_ld, out_neg,
                               pos_scores, out_pos, cand_stats, nullptr, stream);
}

int kge_step_forward_ex(int fn, int mode, const float* ent, int64_t nentity, int64_t ent_ld, const float* rel,
                        int64_t nrelation, int64_t rel_ld, int64_t rel_off, const int64_t* pos, const int64_t* neg,
                        int64_t neg_ld, int64_t B, int64_t N, int64_t D, float gamma, float emb_range, float modulus,
                        float temperature, int adversarial, float* neg_scores, int64_t ns_ld, float* out_neg,
                        float* pos_scores, float* out_pos, float* cand_stats, const kge_forms* forms, void* stream) {
    int rc = check_fn_mode(fn, mode);
    if (rc) return rc;
    if (mode == KGE_SINGLE) return fail(KGE_EINVAL, "kge_step_forward needs a negative mode (0 or 1)");
    if (B < 0 || N <= 0 || D <= 0) return fail(KGE_EINVAL, "bad shape (B, N, D)");
    if (B == 0) return ok();
    if (!pos || !neg || !neg_scores || !out_neg || !out_pos) return fail(KGE_EINVAL, "null pointer");
    const Tables t = {fn, ent, nentity, ent_ld, rel, nrelation, rel_ld, rel_off, D, gamma, emb_range, modulus};
    ScoreParams p;
    fill_indexed(p, t, {mode, pos, neg, neg_ld, B, N});
    p.out = neg_scores;
    p.out_ld = ns_ld;
    p.cand_stats = reinterpret_cast<float2*>(cand_stats);
    p.pos_base = pos;
    p.temperature = temperature;
    p.adversarial = adversarial;
    p.out_neg = out_neg;
    p.out_pos_raw = pos_scores;
    p.out_pos_ls = out_pos;
    const int order = step_order(nentity, N, forms);
    if (!(cand_stats && fn == KGE_INTERHT) && order != 0) {
        // two launches: the negatives (and the positives) in row-group x XCD-slice tiles or in XCD-sliced
        // ascending-id order, then the rows' self-adversarial reductions
        if (order == 2 && tile_plan(fn, p, forms)) {
            p.tile_pos = 1;
            rc = run_score(fn, mode, p, KIND_STEP_FWD_TILE, stream);
        } else {
            p.xcd_phases = xcd_phases(nentity, ent_ld, forms);
            rc = run_score(fn, mode, p, KIND_STEP_FWD_XCD, stream);
        }
        if (rc) return rc;
        return launch_neg_rows(p, "kge_step_forward row reductions", stream);
    }
    // one launch: negatives + the per-row finish (positive, reduction)
    return run_score(fn, mode, p, (cand_stats && fn == KGE_INTERHT) ? KIND_STEP_FWD_STATS : KIND_STEP_FWD, stream);
}

// kge_step_plan_size / kge_step_plan over the descriptors (the planner calls them every step)
static int64_t step_plan_bytes(const Tables& t, int64_t B, int64_t N) {
    if (!valid_fn(t.fn)) return 0;
    ScoreParams tp;
    const int R = planned_tile_params(t, B, N, tp);
    return R ? plan_words(B, N, R) * 4 : 0;
}

int64_t kge_step_plan_size(int fn, int64_t nentity, int64_t ent_ld, int64_t nrelation, int64_t rel_ld,
                           int64_t rel_off, int64_t B, int64_t N, int64_t D) {
    return step_plan_bytes({fn, nullptr, nentity, ent_ld, nullptr, nrelation, rel_ld, rel_off, D, 0.f, 0.f, 0.f}, B, N);
}

// rows: the rows per group (the planner's row rule or kge_step_planner_set_rows); 0: the library's
static int step_plan(const Tables& t, const Batch& b, void* plan, void* stream, int rows = 0) {
    if (!valid_fn(t.fn)) return fail(KGE_EINVAL, "unknown score function id " + std::to_string(t.fn));
    if (b.mode != KGE_HEAD_BATCH && b.mode != KGE_TAIL_BATCH)
        return fail(KGE_EINVAL, "kge_step_plan needs a negative mode (0 or 1)");
    if (b.B <= 0 || b.N <= 0 || t.D <= 0) return fail(KGE_EINVAL, "bad shape (B, N, D)");
    if (!b.pos || !b.neg || !plan) return fail(KGE_EINVAL, "null pointer");
    if (!aligned(plan, 16)) return fail(KGE_EINVAL, "the plan must be 16-B aligned");
    ScoreParams tp;
    if (!planned_tile_params(t, b.B, b.N, tp))
        return fail(KGE_ENOTSUP, "the tile form does not apply to this shape (kge_step_plan_size is 0)");
    if (rows) tp.tile_rows = rows;
    const PlanArgs a = plan_args(tp, t, b, plan);
    const unsigned groups = (unsigned)plan_groups(b.B, tp.tile_rows);
    if (tp.tile_waves == 16)
        hipLaunchKernelGGL(tile_plan_kernel<16>, dim3(groups), dim3(16 * kWave), plan_lds_ints(16 * kWave) * 4,
                           (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(tile_plan_kernel<12>, dim3(groups), dim3(12 * kWave), plan_lds_ints(12 * kWave) * 4,
                           (hipStream_t)stream, a);
    return check_launch("kge_step_plan");
}

int kge_step_plan(int fn, int mode, int64_t nentity, int64_t ent_ld, int64_t nrelation, int64_t rel_ld,
                  int64_t rel_off, const int64_t* pos, const int64_t* neg, int64_t neg_ld, int64_t B, int64_t N,
                  int64_t D, void* plan, void* stream) {
    return step_plan({fn, nullptr, nentity, ent_ld, nullptr, nrelation, rel_ld, rel_off, D, 0.f, 0.f, 0.f},
                     {mode, pos, neg, neg_ld, B, N}, plan, stream);
}

// the outputs of a step forward
struct StepOut {
    float* neg_scores;
    int64_t ns_ld;
    float *out_neg, *pos_scores, *out_pos;
};

// One planned step: batch b (its ids are the plan's: b.pos and b.neg are not read) scored from `plan`, the plan of
// batch `next` made into next_plan (null: none). sf: the planner's sweep form (null: the library's).
static int step_forward_planned(const Tables& t, const Batch& b, float temperature, int adversarial, const void* plan,
                                const Batch& next, void* next_plan, const StepOut& o, const SweepForm* sf,
                                void* stream, int rows = 0, int* occ = nullptr, int plan_blocks = 0) {
    int rc = check_fn_mode(t.fn, b.mode);
    if (rc) return rc;
    if (b.mode == KGE_SINGLE) return fail(KGE_EINVAL, "kge_step_forward_planned needs a negative mode (0 or 1)");
    if (b.B <= 0 || b.N <= 0 || t.D <= 0) return fail(KGE_EINVAL, "bad shape (B, N, D)");
    if (!t.ent || !t.rel || !plan || !o.neg_scores || !o.out_neg || !o.out_pos) return fail(KGE_EINVAL, "null pointer");
    if (next_plan) {
        if (next.mode != KGE_HEAD_BATCH && next.mode != KGE_TAIL_BATCH)
            return fail(KGE_EINVAL, "the next batch needs a negative mode (0 or 1)");
        if (!next.pos || !next.neg) return fail(KGE_EINVAL, "next_plan needs next_pos and next_neg");
        if (next_plan == plan) return fail(KGE_EINVAL, "next_plan must not be the plan this step reads");
        if (!aligned(next_plan, 16)) return fail(KGE_EINVAL, "the plan must be 16-B aligned");
    }
    if (!aligned(plan, 16)) return fail(KGE_EINVAL, "the plan must be 16-B aligned");
    ScoreParams tp;
    const int R = planned_tile_params(t, b.B, b.N, tp);
    ScoreParams p;
    fill_indexed(p, t, {b.mode, nullptr, nullptr, 0, b.B, b.N});
    // the planner's sweep form: a plan does not depend on it (the same rows per group at every wave count)
    kge_forms fm = {-1, 0, 0, -1, sf ? sf->waves : 0, 0, 0};
    if (!R || !tile_plan(t.fn, p, &fm) || p.tile_rows != R)
        return fail(KGE_ENOTSUP, "the tile form does not apply to these tables (unaligned rows, or "
                                 "kge_step_plan_size is 0): use kge_step_forward");
    // the planned instance's own LDS, at the plan's rows per group (rows; 0: the library's)
    if (!planned_tile_layout(t.fn, p, rows ? rows : R))
        return fail(KGE_ENOTSUP, "this many rows per group do not fit a block of the planned step");
    tp.tile_rows = p.tile_rows;
    p.out = o.neg_scores;
    p.out_ld = o.ns_ld;
    p.pos_base = nullptr;
    p.temperature = temperature;
    p.adversarial = adversarial;
    p.out_neg = o.out_neg;
    p.out_pos_raw = o.pos_scores;
    p.out_pos_ls = o.out_pos;
    p.tile_pos = 1;
    p.tile_plan = reinterpret_cast<const int*>(plan);
    if (sf) {
        p.tile_rev = sf->rev;
        p.tile_depth = sf->depth;
        p.tile_board = sf->board;
        p.tile_tag = sf->tag;
        p.tile_lead = sf->lead;
        p.tile_clk = sf->clk;
    }
    // the next batch's plan: the scoring launch's tail blocks, on the CUs its scoring blocks free up at its end
    // (C2 device time per step, alternating modes: 93.6 us; made beside the row reductions 99.5 us, as a launch
    // of its own 101.6 us, not planned 101.9 us; scripts/plan_probe.py, profiles/r05_plan_ab.txt)
    if (next_plan) {
        p.tile_next = plan_args(tp, t, next, next_plan);
        // one plan block per group, or plan_blocks of them that share the groups (the planner's row rule)
        const int ng = (int)plan_groups(next.B, tp.tile_rows);
        p.tile_plan_blocks = (plan_blocks > 0 && p.tile_waves == kTileSharedWaves) ? std::min(plan_blocks, ng) : ng;
        p.tile_lds = std::max(p.tile_lds, plan_lds_ints(p.tile_waves * kWave) * 4);
    }
    p.tile_occ = occ;
    rc = run_score(t.fn, b.mode, p, KIND_STEP_FWD_TILE, stream);
    if (rc || occ) return rc;
    return launch_neg_rows(p, "kge_step_forward_planned row reductions", stream);
}

int kge_step_forward_planned(int fn, int mode, const float* ent, int64_t nentity, int64_t ent_ld, const float* rel,
                             int64_t nrelation, int64_t rel_ld, int64_t rel_off, int64_t B, int64_t N, int64_t D,
                             float gamma, float emb_range, float modulus, float temperature, int adversarial,
                             const void* plan, const int64_t* next_pos, const int64_t* next_neg, int64_t next_neg_ld,
                             int next_mode, void* next_plan, float* neg_scores, int64_t ns_ld, float* out_neg,
                             float* pos_scores, float* out_pos, void* stream) {
    const Tables t = {fn, ent, nentity, ent_ld, rel, nrelation, rel_ld, rel_off, D, gamma, emb_range, modulus};
    return step_forward_planned(t, {mode, nullptr, nullptr, 0, B, N}, temperature, adversarial, plan,
                                {next_mode, next_pos, next_neg, next_neg_ld, B, N}, next_plan,
                                {neg_scores, ns_ld, out_neg, pos_scores, out_pos}, nullptr, stream);
}

// Whether a planner applies the row rule unless kge_step_planner_set_rows says otherwise: as planned_sweep_defaults,
// only what was measured and passed (profiles/r16_rows_ab.txt; each at ONE shape, B 512, N 256, d 1000).
// C2 (InterHT) +2.0 %, C3 (RotatE) +4.6 %; C4 (DistMult d 500, N 1024: 2 KB rows, 17 x 1 025 items per plan group)
// lost 18 % and keeps the library's rows and one plan block per group, as every other function and width does.
int planner_row_rule(int fn, int64_t D) {
    const int64_t row_bytes = D * 4 * (is_split(fn) ? 2 : 1);
    return row_bytes >= 4096 && (fn == KGE_INTERHT || fn == KGE_ROTATE);
}

// The planned step loop as a handle (kge_step_planner_*): the tables, shapes and the two plan buffers are given
// once; a step then passes only the next batch and the outputs (9 arguments instead of 29: at C2 the device
// step is ~93 us and the host issues one step per step, so its per-call cost is part of the loop's rate).
struct kge_step_planner {
    Tables t = {};
    int64_t B = 0, N = 0;
    float temperature = 1.f;
    int adversarial = 1;
    void* plans[2] = {nullptr, nullptr};
    int cur = -1;  // the buffer holding the next step's plan (-1: none)
    int mode = 0;  // that plan's batch mode
    // kge_step_planner_set_sweep: 1 (default) = the tile sweep's direction alternates step by step, so a step starts
    // on the entity rows the step before touched last, which the Infinity Cache still holds when the table is larger
    // than it (C2's 327.5 MB: 92.8 -> 86.3 us per step, scripts/sweep_probe.py, profiles/r06_sweep_ab.txt)
    int sweep = 1;
    // kge_step_planner_set_form / _set_lead / _set_board: 0, 0, -1 = planned_sweep_defaults' choice
    int waves = 0, depth = 0, lead = -1;
    int* board = nullptr;
    long long* clk = nullptr;  // kge_step_planner_set_clocks (profiling builds)
    int cus = 0;               // the device's CUs: the throttle needs every scoring block resident
    int64_t groups = 0;        // row groups of a batch (8 scoring blocks each)
    // rows per group of the plans and steps to come: 0 until the first plan, which takes the library's, or the row
    // rule's (planned_rows_rule) where planner_row_rule or kge_step_planner_set_rows says so (rule)
    int rows = 0;
    int rule = 0;
    // plan blocks of a step's launch: 0 = one per group, at the launch's end; where the row rule found the scoring
    // grid to leave 8 CUs free, 8 that share the groups and run beside the sweep
    int plan_blocks = 0;
    int64_t plan_bytes = 0;    // each plan buffer's size
    int64_t steps = 0;  // steps issued
    void* stream = nullptr;
};

// what the planner's next step runs (the setters' choices over the library's), and whether its throttle runs
// (groups: the row groups the form is for; -1: the planner's current count)
static SweepForm planner_form(const kge_step_planner* sp, int64_t groups = -1) {
    if (groups < 0) groups = sp->groups;
    SweepForm f = {0, 0, 0, 0, sp->sweep ? (int)(sp->steps & 1) : 0, nullptr, sp->clk};
    planned_sweep_defaults(sp->t.fn, sp->t.D, f.waves, f.depth, f.lead);
    if (sp->waves) f.waves = sp->waves;
    if (sp->depth) f.depth = sp->depth;
    if (f.waves == 8) f.depth = 2;
    if (sp->lead >= 0) f.lead = sp->lead;
    f.tag = (int)(sp->steps % kSweepTagMask) + 1;  // 1 .. kSweepTagMask: a zeroed board holds no entry
    if (sp->board && f.lead > 0 && groups <= kSweepBoardLine && groups * 8 <= sp->cus) f.board = sp->board;
    return f;
}

// The blocks of the planner's next step resident at once at R rows per group: the device's CUs times the blocks per
// CU of the step's instance (the smaller of its head-batch and tail-batch instances) at that layout's LDS, from the
// runtime's occupancy answer. 0: no device, or no answer. Nothing is launched.
static int64_t planner_capacity(const kge_step_planner* sp, int R) {
    if (sp->cus <= 0) return 0;
    // (the throttle's instance is the form's where every block is resident)
    const SweepForm sf = planner_form(sp, plan_groups(sp->B, R));
    int per_cu = INT32_MAX;
    float* const none = reinterpret_cast<float*>(sp->plans[0]);  // stands for every buffer: nothing runs
    const int64_t* const ids = reinterpret_cast<const int64_t*>(sp->plans[0]);
    for (int mode : {KGE_HEAD_BATCH, KGE_TAIL_BATCH}) {
        int occ = 0;
        if (step_forward_planned(sp->t, {mode, nullptr, nullptr, 0, sp->B, sp->N}, sp->temperature, sp->adversarial,
                                 sp->plans[0], {mode, ids, ids, sp->N, sp->B, sp->N}, sp->plans[1],
                                 {none, sp->N, none, none, none}, &sf, sp->stream, R, &occ, 8))
            return 0;
        per_cu = std::min(per_cu, occ);
    }
    return (int64_t)sp->cus * per_cu;
}

// the rows per group of the planner's plans and steps, chosen at the first plan (capacity unknown: the library's)
static int planner_rows(kge_step_planner* sp) {
    if (!sp->rows) {
        sp->rows = planned_rows_rule(sp->t, sp->B, sp->N, planner_form(sp).waves, sp->plan_bytes,
                                     [&](int R) { return sp->rule ? planner_capacity(sp, R) : 0; });
        if (plan_groups(sp->B, sp->rows) > sp->groups) sp->clk = nullptr;  // (a clock record is sized for its groups)
        sp->groups = plan_groups(sp->B, sp->rows);
        const int64_t cap = sp->rule ? planner_capacity(sp, sp->rows) : 0;
        sp->plan_blocks = (cap > 0 && 8 * sp->groups <= cap - 8) ? 8 : 0;
    }
    return sp->rows;
}

int64_t kge_step_planner_plan_size(int fn, int64_t nentity, int64_t ent_ld, int64_t nrelation, int64_t rel_ld,
                                   int64_t rel_off, int64_t B, int64_t N, int64_t D) {
    const Tables t = {fn, nullptr, nentity, ent_ld, nullptr, nrelation, rel_ld, rel_off, D, 0.f, 0.f, 0.f};
    if (!valid_fn(fn)) return 0;
    ScoreParams tp;
    const int R0 = planned_tile_params(t, B, N, tp);
    int64_t words = 0;
    for (int R = R0; R0 && R <= kTileMaxRows; ++R) words = std::max(words, plan_words(B, N, R));
    return words * 4;
}

int kge_step_planned_rows(int fn, int64_t nentity, int64_t ent_ld, int64_t nrelation, int64_t rel_ld, int64_t rel_off,
                          int64_t B, int64_t N, int64_t D, int waves, int64_t capacity, int* out) {
    if (!valid_fn(fn)) return fail(KGE_EINVAL, "unknown score function id " + std::to_string(fn));
    if (!out || (waves != 0 && waves != 8 && waves != 12 && waves != 16))
        return fail(KGE_EINVAL, "kge_step_planned_rows: out[4]; waves 0, 8, 12 or 16");
    const Tables t = {fn, nullptr, nentity, ent_ld, nullptr, nrelation, rel_ld, rel_off, D, 0.f, 0.f, 0.f};
    const int R = planned_rows_rule(t, B, N, waves, 0, [&](int) { return capacity; });
    ScoreParams tp;
    if (!R || !planned_tile_params(t, B, N, tp)) return fail(KGE_ENOTSUP, "the tile form does not apply to this shape");
    if (waves) tp.tile_waves = waves;
    if (!planned_tile_layout(fn, tp, R)) return fail(KGE_ENOTSUP, "the rows do not fit this wave count");
    out[0] = R;
    out[1] = tp.tile_q2slots;
    out[2] = std::max(tp.tile_lds, plan_lds_ints(tp.tile_waves * kWave) * 4);
    out[3] = (int)(8 * plan_groups(B, R));
    return ok();
}

int kge_step_planner_create(kge_step_planner** out, int fn, const float* ent, int64_t nentity, int64_t ent_ld,
                            const float* rel, int64_t nrelation, int64_t rel_ld, int64_t rel_off, int64_t B, int64_t N,
                            int64_t D, float gamma, float emb_range, float modulus, float temperature, int adversarial,
                            void* plan0, void* plan1, int64_t plan_bytes, void* stream) {
    if (!out) return fail(KGE_EINVAL, "kge_step_planner_create: null pointer");
    *out = nullptr;
    const Tables t = {fn, ent, nentity, ent_ld, rel, nrelation, rel_ld, rel_off, D, gamma, emb_range, modulus};
    const int64_t need = step_plan_bytes(t, B, N);
    if (need <= 0) return fail(KGE_ENOTSUP, "kge_step_planner_create: the tile form does not apply to this shape");
    if (!ent || !rel || !plan0 || !plan1 || plan0 == plan1) return fail(KGE_EINVAL, "kge_step_planner_create: bad pointers");
    if (plan_bytes < need || !aligned(plan0, 16) || !aligned(plan1, 16))
        return fail(KGE_EINVAL, "kge_step_planner_create: plan buffers too small or not 16-B aligned");
    kge_step_planner* sp = new kge_step_planner;
    sp->t = t;
    sp->B = B;
    sp->N = N;
    sp->temperature = temperature;
    sp->adversarial = adversarial;
    sp->plans[0] = plan0;
    sp->plans[1] = plan1;
    sp->stream = stream;
    sp->plan_bytes = plan_bytes;
    sp->rule = planner_row_rule(fn, D);
    ScoreParams tp;
    sp->groups = plan_groups(B, planned_tile_params(t, B, N, tp));
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&sp->cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        sp->cus = 0;  // unknown: no throttle
    *out = sp;
    return ok();
}

int kge_step_planner_set_form(kge_step_planner* sp, int waves, int depth) {
    if (!sp) return fail(KGE_EINVAL, "kge_step_planner_set_form: null pointer");
    if ((waves != 0 && waves != 8 && waves != 12 && waves != 16) || depth < 0 || depth > 2 || (waves == 8 && depth == 1))
        return fail(KGE_EINVAL, "kge_step_planner_set_form: waves 0, 8, 12 or 16; depth 0, 1 or 2 (8 waves: not 1)");
    if (waves) {  // the plans are made for the library's rows per group: the chosen block must take the same
        ScoreParams tp, tw;
        kge_forms fm = {-1, 0, 0, -1, waves, 0, 0};
        if (planned_tile_params(sp->t, sp->B, sp->N, tw, &fm) != planned_tile_params(sp->t, sp->B, sp->N, tp))
            return fail(KGE_ENOTSUP, "kge_step_planner_set_form: this wave count changes the rows per group");
    }
    if (waves && sp->rows > 2 * waves)  // (the planned prologue builds at most two rows per wave)
        return fail(KGE_ENOTSUP, "kge_step_planner_set_form: this wave count changes the rows per group");
    sp->waves = waves;
    sp->depth = depth;
    return ok();
}

int kge_step_planner_set_rows(kge_step_planner* sp, int rows) {
    if (!sp) return fail(KGE_EINVAL, "kge_step_planner_set_rows: null pointer");
    const bool chosen = rows > 0 || rows < KGE_PLANNER_ROWS_RULE;  // (a refused call changes nothing)
    if (chosen) {
        ScoreParams tp;
        if (rows < 0 || !planned_tile_params(sp->t, sp->B, sp->N, tp)) return fail(KGE_EINVAL, "kge_step_planner_set_rows: bad rows");
        tp.tile_waves = planner_form(sp).waves;
        if (!planned_tile_layout(sp->t.fn, tp, rows))
            return fail(KGE_ENOTSUP, "kge_step_planner_set_rows: this many rows do not fit a block of this form");
        if (plan_words(sp->B, sp->N, rows) * 4 > sp->plan_bytes)
            return fail(KGE_EINVAL, "kge_step_planner_set_rows: the plan buffers are too small (kge_step_planner_plan_size)");
        if (plan_groups(sp->B, rows) > sp->groups) sp->clk = nullptr;  // (a clock record is sized for its groups)
        sp->groups = plan_groups(sp->B, rows);
    }
    sp->rule = rows == KGE_PLANNER_ROWS_RULE || (rows == 0 && planner_row_rule(sp->t.fn, sp->t.D));
    sp->plan_blocks = 0;
    sp->rows = chosen ? rows : 0;
    return ok();
}

int64_t kge_step_board_size(void) { return (int64_t)kSweepBoardInts * 4; }

int kge_step_planner_set_board(kge_step_planner* sp, void* board, int64_t board_bytes) {
    if (!sp) return fail(KGE_EINVAL, "kge_step_planner_set_board: null pointer");
    if (board && (board_bytes < kge_step_board_size() || !aligned(board, 4)))
        return fail(KGE_EINVAL, "kge_step_planner_set_board: kge_step_board_size bytes, 4-B aligned");
    sp->board = reinterpret_cast<int*>(board);
    return ok();
}

int kge_step_planner_set_lead(kge_step_planner* sp, int lead) {
    if (!sp) return fail(KGE_EINVAL, "kge_step_planner_set_lead: null pointer");
    if (lead < -1 || lead >= kTileBuckets) return fail(KGE_EINVAL, "kge_step_planner_set_lead: -1, 0 or 1..255 buckets");
    sp->lead = lead;
    return ok();
}

int kge_step_planner_get(const kge_step_planner* sp, int what) {
    if (!sp) return -1;
    const SweepForm f = planner_form(sp);
    switch (what) {
        case KGE_PLANNER_WAVES: return f.waves;
        case KGE_PLANNER_DEPTH: return f.depth;
        case KGE_PLANNER_LEAD: return f.lead;
        case KGE_PLANNER_THROTTLE: return f.board != nullptr;
        case KGE_PLANNER_TAG: return f.tag;
        case KGE_PLANNER_ROWS: return sp->rows;
        case KGE_PLANNER_PLAN_BLOCKS:
            return !sp->rows ? 0 : (sp->plan_blocks > 0 && f.waves == kTileSharedWaves) ? (int)std::min<int64_t>(sp->plan_blocks, sp->groups) : (int)sp->groups;
        default: return -1;
    }
}

int kge_step_planner_set_clocks(kge_step_planner* sp, void* clocks, int64_t clocks_bytes) {
#ifdef KGE_PROFILING_KNOBS
    if (!sp) return fail(KGE_EINVAL, "kge_step_planner_set_clocks: null pointer");
    if (clocks && (clocks_bytes < kge_sweep_clk_words(sp->groups) * 8 || !aligned(clocks, 8)))
        return fail(KGE_EINVAL, "kge_step_planner_set_clocks: groups * (8 * 40 + 2) * 8 bytes, 8-B aligned");
    sp->clk = reinterpret_cast<long long*>(clocks);
    return ok();
#else
    (void)sp;
    (void)clocks;
    (void)clocks_bytes;
    return fail(KGE_ENOTSUP, "kge_step_planner_set_clocks: a -DKGE_PROFILING_KNOBS build only");
#endif
}

int kge_step_planner_set_modulus(kge_step_planner* sp, float modulus) {
    if (!sp) return fail(KGE_EINVAL, "kge_step_planner_set_modulus: null pointer");
    sp->t.modulus = modulus;
    return ok();
}

int kge_step_planner_set_sweep(kge_step_planner* sp, int alternate) {
    if (!sp) return fail(KGE_EINVAL, "kge_step_planner_set_sweep: null pointer");
    if (alternate != 0 && alternate != 1) return fail(KGE_EINVAL, "kge_step_planner_set_sweep: 0 or 1");
    sp->sweep = alternate;
    return ok();
}

int kge_step_planner_plan(kge_step_planner* sp, const int64_t* pos, const int64_t* neg, int64_t neg_ld, int mode) {
    if (!sp) return fail(KGE_EINVAL, "kge_step_planner_plan: null pointer");
    const int buf = sp->cur < 0 ? 0 : sp->cur;
    const int rc = step_plan(sp->t, {mode, pos, neg, neg_ld, sp->B, sp->N}, sp->plans[buf], sp->stream, planner_rows(sp));
    if (rc) return rc;
    sp->cur = buf;
    sp->mode = mode;
    return ok();
}

int kge_step_planner_step(kge_step_planner* sp, const int64_t* next_pos, const int64_t* next_neg, int64_t next_neg_ld,
                          int next_mode, float* neg_scores, float* out_neg, float* pos_scores, float* out_pos) {
    if (!sp) return fail(KGE_EINVAL, "kge_step_planner_step: null pointer");
    if (sp->cur < 0) return fail(KGE_EINVAL, "kge_step_planner_step: no batch planned (kge_step_planner_plan first)");
    const bool nxt = next_pos && next_neg;
    const int rows = planner_rows(sp);
    const SweepForm sf = planner_form(sp);
    const int rc = step_forward_planned(sp->t, {sp->mode, nullptr, nullptr, 0, sp->B, sp->N}, sp->temperature,
                                        sp->adversarial, sp->plans[sp->cur],
                                        {next_mode, next_pos, next_neg, next_neg_ld, sp->B, sp->N},
                                        nxt ? sp->plans[1 - sp->cur] : nullptr,
                                        {neg_scores, sp->N, out_neg, pos_scores, out_pos}, &sf, sp->stream, rows,
                                        nullptr, sp->plan_blocks);
    if (rc) return rc;
    ++sp->steps;
    if (nxt) {
        sp->cur = 1 - sp->cur;
        sp->mode = next_mode;
    } else {
        sp->cur = -1;
    }
    return ok();
}

int kge_step_planner_destroy(kge_step_planner* sp) {
    delete sp;
    return ok();
}

int kge_score_sharded(int fn, int mode, const float* qent, int64_t q_ld, const float* rel, int64_t nrelation,
                      int64_t rel_ld, int64_t rel_off, const float* shard, int64_t shard_rows, int64_t shard_ld,
                      int64_t shard_lo, const int64_t* pos, const int64_t* neg, int64_t neg_ld, int64_t B, int64_t N,
                      int64_t D, float gamma, float emb_range, float modulus, float* scores, int64_t scores_ld,
                      void* stream) {
    int rc = check_fn_mode(fn, mode);
    if (rc) return rc;
    rc = refuse_sharded(fn, "kge_score_sharded");
    if (rc) return rc;
    if (B < 0 || N < 0 || D <= 0 || shard_rows < 0) return fail(KGE_EINVAL, "bad shape");
    if (empty(B, mode == KGE_SINGLE ? 1 : N)) return ok();
    if (!pos || (mode != KGE_SINGLE && !neg) || !scores || !qent || !shard)
        return fail(KGE_EINVAL, "null pointer");
    const Tables t = {fn, shard, shard_rows, shard_ld, rel, nrelation, rel_ld, rel_off, D, gamma, emb_range, modulus};
    ScoreParams p;
    fill_indexed(p, t, {mode, pos, neg, neg_ld, B, N});
    // query entity rows come pre-assembled (row b of qent); candidates from the local shard
    p.qent = qent;
    p.q_idx = nullptr;
    p.q_ld = q_ld;
    p.q_rows = B;
    p.c_base = shard_lo;
    p.skip_foreign = 1;
    p.out = scores;
    p.out_ld = scores_ld;
    if (mode != KGE_SINGLE && shard_lo >= 0 && shard_lo + shard_rows < ((int64_t)1 << 31) &&
        use_xcd_order(shard_rows, N))
        return run_score(fn, mode, p, KIND_SCORE_SHARD_XCD, stream);  // XCD-sliced order over the shard
    return run_score(fn, mode, p, KIND_FWD, stream);
}

int kge_shard_score(int fn, int mode, const float* qent, int64_t q_rows, int64_t q_ld, const int64_t* q_idx,
                    const float* rel, int64_t nrelation, int64_t rel_ld, int64_t rel_off, const float* shard,
                    int64_t shard_rows, int64_t shard_ld, int64_t shard_lo, const int64_t* pos, int64_t B, int64_t N,
                    int64_t D, float gamma, float emb_range, float modulus, const int* bucket,
                    const int* bucket_start, const int* pre, const int* cnt, const int* tot, int world, int rank,
                    int64_t home_B, int64_t home0, float* send, void* stream) {
    if (mode != KGE_HEAD_BATCH && mode != KGE_TAIL_BATCH)
        return fail(KGE_EINVAL, "kge_shard_score: mode must be 0 (head-batch) or 1 (tail-batch)");
    int rc = check_fn_mode(fn, mode);
    if (rc) return rc;
    rc = refuse_sharded(fn, "kge_shard_score");
    if (rc) return rc;
    if (B < 0 || N < 0 || D <= 0 || shard_rows <= 0 || q_rows < 0) return fail(KGE_EINVAL, "bad shape");
    if (world < 1 || rank < 0 || rank >= world || home_B <= 0 || B % home_B || home0 < 0 ||
        home0 + B / home_B > world)
        return fail(KGE_EINVAL, "kge_shard_score: rows must be whole homes of home_B rows");
    if (shard_lo < 0 || shard_rows >= ((int64_t)1 << 25))
        return fail(KGE_ENOTSUP, "kge_shard_score: the shard must hold < 2^25 rows");
    if (B == 0) return ok();
    if (!pos || !send || !qent || !q_idx || !shard || !bucket || !bucket_start || !pre || !cnt || !tot)
        return fail(KGE_EINVAL, "null pointer");
    const Tables t = {fn, shard, shard_rows, shard_ld, rel, nrelation, rel_ld, rel_off, D, gamma, emb_range, modulus};
    ScoreParams p;
    fill_indexed(p, t, {mode, pos, nullptr, 0, B, N + 1});
    // query entity rows: row q_idx[b] of the exchanged query block; candidates: the bucket's shard rows
    p.qent = qent;
    p.q_idx = q_idx;
    p.q_stride = 1;
    p.q_ld = q_ld;
    p.q_rows = q_rows;
    p.c_idx = nullptr;
    p.c_base = shard_lo;
    p.skip_foreign = 1;
    p.pos_base = pos;
    p.bk_ent = reinterpret_cast<const int2*>(bucket);
    p.bk_start = bucket_start;
    p.bk_ld = N + 1;
    p.cmp_pre = pre;
    p.cmp_cnt = cnt;
    p.cmp_tot = tot;
    p.cmp_home0 = home0;
    p.home_B = home_B;
    p.world = world;
    p.rank = rank;
    p.out = send;
    p.out_ld = 0;
    return run_score(fn, mode, p, KIND_SHARD_BUCKET, stream);
}

int kge_gather_rows(const float* table, int64_t rows, int64_t ld, int64_t lo, const int64_t* ids, int64_t id_stride,
                    int64_t n, int64_t width, float* out, int64_t out_ld, void* stream) {
    if (n < 0 || width < 0 || rows < 0) return fail(KGE_EINVAL, "bad shape");
    if (n == 0 || width == 0) return ok();
    if (!table || !ids || !out) return fail(KGE_EINVAL, "null pointer");
    const int vec4 = (width % 4 == 0 && ld % 4 == 0 && out_ld % 4 == 0 && aligned(table, 16) && aligned(out, 16));
    const int64_t blocks = (n + kWavesPerBlock - 1) / kWavesPerBlock;
    hipLaunchKernelGGL(gather_owned_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, table, rows,
                       ld, lo, ids, id_stride, n, width, out, out_ld, vec4);
    return check_launch("kge_gather_rows");
}

int kge_eval_query(int fn, int mode, const float* ent, int64_t nentity, int64_t ent_ld, const float* rel,
                   int64_t nrelation, int64_t rel_ld, const int64_t* pos, int64_t B, int64_t D, float* Q, int64_t ldq,
                   void* stream) {
    int rc = check_fn_mode(fn, mode);
    if (rc) return rc;
    if (fn != KGE_DISTMULT && fn != KGE_COMPLEX)
        return fail(KGE_ENOTSUP, "kge_eval_query: only DistMult and ComplEx score as a dense contraction");
    if (mode == KGE_SINGLE) return fail(KGE_EINVAL, "kge_eval_query needs mode 0 or 1");
    if (B < 0 || D <= 0) return fail(KGE_EINVAL, "bad shape");
    if (B == 0) return ok();
    if (!ent || !rel || !pos || !Q) return fail(KGE_EINVAL, "null pointer");
    ScoreParams p;
    fill_indexed(p, {fn, ent, nentity, ent_ld, rel, nrelation, rel_ld, 0, D, 0.f, 1.f, 0.f},
                 {mode, pos, nullptr, 0, B, 1});
    int V = 1, G = 1;
    rc = pick_vg(p, V, G);
    if (rc) return rc;
    if (ldq % V) V = 1;
    while (V > 1 && !aligned(Q, 4 * V)) V >>= 1;
    G = 1;
    while (G * kWave * V < D) G <<= 1;
    if (G > kMaxG) return fail(KGE_ENOTSUP, "dimension too large");
    const int64_t blocks = (B + kWavesPerBlock - 1) / kWavesPerBlock;
    rc = launch_eval_query_any(fn, mode == KGE_HEAD_BATCH, p, (hipStream_t)stream, (int)blocks, V, G, Q, ldq);
    if (rc) return fail(rc, "no eval-query kernel for this width");
    return check_launch("kge_eval_query");
}

int kge_eval_query_planes(int fn, int mode, const float* ent, int64_t nentity, int64_t ent_ld, const float* rel,
                          int64_t nrelation, int64_t rel_ld, const int64_t* pos, int64_t B, int64_t D, void* planes,
                          int64_t plane_rows, void* stream) {
    int rc = check_fn_mode(fn, mode);
    if (rc) return rc;
    if (fn != KGE_DISTMULT && fn != KGE_COMPLEX)
        return fail(KGE_ENOTSUP, "kge_eval_query_planes: only DistMult and ComplEx score as a dense contraction");
    if (mode == KGE_SINGLE) return fail(KGE_EINVAL, "kge_eval_query_planes needs mode 0 or 1");
    if (B < 0 || D <= 0 || plane_rows < B) return fail(KGE_EINVAL, "bad shape");
    if (B == 0) return ok();
    if (!ent || !rel || !pos || !planes) return fail(KGE_EINVAL, "null pointer");
    if (!aligned(planes, 16)) return fail(KGE_EINVAL, "kge_eval_query_planes: planes not 16-B aligned");
    ScoreParams p;
    fill_indexed(p, {fn, ent, nentity, ent_ld, rel, nrelation, rel_ld, 0, D, 0.f, 1.f, 0.f},
                 {mode, pos, nullptr, 0, B, 1});
    int V = 1, G = 1;
    rc = pick_vg(p, V, G);
    if (rc) return rc;
    if (V != 4) return fail(KGE_ENOTSUP, "kge_eval_query_planes needs D % 4 == 0 and 16-B aligned tables");
    G = 1;
    while (G * kWave * V < D) G <<= 1;
    if (G > kMaxG) return fail(KGE_ENOTSUP, "dimension too large");
    const int64_t blocks = (B + kWavesPerBlock - 1) / kWavesPerBlock;
    rc = launch_eval_query_any(fn, mode == KGE_HEAD_BATCH, p, (hipStream_t)stream, (int)blocks, V, G, nullptr, 0,
                               planes, plane_rows);
    if (rc) return fail(rc, "no eval-query kernel for this width");
    return check_launch("kge_eval_query_planes");
}

int kge_gemm_nt(const float* A, int64_t lda, const float* Bm, int64_t ldb, float* C, int64_t ldc, int64_t M,
                int64_t N, int64_t K, void* stream) {
    if (M < 0 || N < 0 || K < 0) return fail(KGE_EINVAL, "bad shape");
    if (M == 0 || N == 0) return ok();
    if (!A || !Bm || !C) return fail(KGE_EINVAL, "null pointer");
    if (M > INT32_MAX || N > INT32_MAX || K > INT32_MAX) return fail(KGE_EINVAL, "shape exceeds int32");
    if (K % 4 || lda % 4 || ldb % 4 || !aligned(A, 16) || !aligned(Bm, 16))
        return fail(KGE_ENOTSUP, "kge_gemm_nt needs K, lda, ldb multiples of 4 and 16-byte aligned A, B");
    launch_gemm_nt(A, Bm, C, (int)M, (int)N, (int)K, lda, ldb, ldc, (hipStream_t)stream);
    return check_launch("kge_gemm_nt");
}

int64_t kge_split_bf16x3_bytes(int64_t rows, int64_t cols) {
    if (rows < 0 || cols <= 0) return 0;
    return 3 * rows * ((cols + 15) / 16 * 16) * 2;
}

int kge_split_bf16x3(const float* X, int64_t rows, int64_t cols, int64_t ld, void* planes, int64_t plane_rows,
                     void* stream) {
    if (rows < 0 || cols <= 0 || ld < cols || plane_rows < rows) return fail(KGE_EINVAL, "kge_split_bf16x3: bad shape");
    if (rows == 0) return ok();
    if (!X || !planes) return fail(KGE_EINVAL, "kge_split_bf16x3: null pointer");
    if (!aligned(planes, 16)) return fail(KGE_EINVAL, "kge_split_bf16x3: planes must be 16-B aligned");
    if (kge_split_bf16x3_bytes(plane_rows, cols) >= ((int64_t)1 << 32) - 16)
        return fail(KGE_ENOTSUP, "kge_split_bf16x3: planes past 4 GB (the GEMM's 32-bit buffer offsets)");
    launch_split3_planes(X, rows, cols, ld, planes, plane_rows, (hipStream_t)stream);
    return check_launch("kge_split_bf16x3");
}

int kge_gemm_nt_bf16x3_planes(const void* A_planes, int64_t a_rows, const void* B_planes, int64_t b_rows, int64_t K,
                              float* C, int64_t ldc, int64_t M, int64_t N, void* stream) {
    return kge_gemm_nt_bf16x3_planes_ex(A_planes, a_rows, B_planes, b_rows, K, C, ldc, M, N, nullptr, stream);
}

// the plane GEMM the library runs (forms->gemm_form 0): 1 = gemm_nt_x3p_kernel 256 x 256, 2 = gemm_nt_x3d_kernel,
// 3 = gemm_nt_x3p_kernel 256 x 192, 4 = gemm_nt_x3l_kernel (LDS-DMA staging, three stages; 546 against 551 us at
// C5's shape, 568 against 572 us for the rank call: profiles/r06_gemm_dma_ab.txt)
constexpr int kPlanesGemmForm = 4;

int kge_gemm_nt_bf16x3_planes_ex(const void* A_planes, int64_t a_rows, const void* B_planes, int64_t b_rows, int64_t K,
                                 float* C, int64_t ldc, int64_t M, int64_t N, const kge_forms* forms, void* stream) {
    const int form = forms && forms->gemm_form >= 1 && forms->gemm_form <= 4 ? forms->gemm_form : kPlanesGemmForm;
    if (M < 0 || N < 0 || K <= 0 || M > a_rows || N > b_rows) return fail(KGE_EINVAL, "bad shape");
    if (M == 0 || N == 0) return ok();
    if (!A_planes || !B_planes || !C) return fail(KGE_EINVAL, "null pointer");
    if (M > INT32_MAX || N > INT32_MAX || !aligned(A_planes, 16) || !aligned(B_planes, 16))
        return fail(KGE_EINVAL, "kge_gemm_nt_bf16x3_planes: int32 shapes and 16-B aligned planes");
    if (kge_split_bf16x3_bytes(a_rows, K) >= ((int64_t)1 << 32) - 16 ||
        kge_split_bf16x3_bytes(b_rows, K) >= ((int64_t)1 << 32) - 16)
        return fail(KGE_ENOTSUP, "kge_gemm_nt_bf16x3_planes: planes past 4 GB");
    launch_gemm_nt_x3p(A_planes, a_rows, B_planes, b_rows, K, C, ldc, (int)M, (int)N, (hipStream_t)stream, form);
    return check_launch("kge_gemm_nt_bf16x3_planes");
}

int kge_gemm_nt_bf16x3(const float* A, int64_t lda, const float* Bm, int64_t ldb, float* C, int64_t ldc, int64_t M,
                      int64_t N, int64_t K, void* stream) {
    return kge_gemm_nt_bf16x3_ex(A, lda, Bm, ldb, C, ldc, M, N, K, nullptr, stream);
}

int kge_gemm_nt_bf16x3_ex(const float* A, int64_t lda, const float* Bm, int64_t ldb, float* C, int64_t ldc, int64_t M,
                          int64_t N, int64_t K, const kge_forms* forms, void* stream) {
    if (M < 0 || N < 0 || K < 0) return fail(KGE_EINVAL, "bad shape");
    if (M == 0 || N == 0) return ok();
    if (!A || !Bm || !C) return fail(KGE_EINVAL, "null pointer");
    if (M > INT32_MAX || N > INT32_MAX || K > INT32_MAX) return fail(KGE_EINVAL, "shape exceeds int32");
    if (K % 4 || lda % 4 || ldb % 4 || !aligned(A, 16) || !aligned(Bm, 16))
        return fail(KGE_ENOTSUP, "kge_gemm_nt_bf16x3 needs K, lda, ldb multiples of 4 and 16-byte aligned A, B");
    launch_gemm_nt_f32x3(A, Bm, C, (int)M, (int)N, (int)K, lda, ldb, ldc, (hipStream_t)stream, forms ? forms->gemm_form : 0);
    return check_launch("kge_gemm_nt_bf16x3");
}

int kge_rank_filtered(const float* scores, int64_t M, int64_t N, int64_t ld, const int64_t* truth,
                      const int64_t* filter_ptr, const int64_t* filter_ids, int64_t* ranks, void* stream) {
    if (M < 0 || N < 0) return fail(KGE_EINVAL, "bad shape");
    if (M == 0) return ok();
    if (!scores || !truth || !ranks || (filter_ptr && !filter_ids)) return fail(KGE_EINVAL, "null pointer");
    if (M > INT32_MAX) return fail(KGE_EINVAL, "too many rows");
    launch_rank(scores, M, N, ld, truth, filter_ptr, filter_ids, ranks, (hipStream_t)stream);
    return check_launch("kge_rank_filtered");
}

int64_t kge_eval_rank_planes_workspace_size(int64_t M, int64_t nfilter) {
    if (M < 0 || nfilter < 0) return 0;
    return eval_rank_ws_bytes(M, nfilter);
}

int kge_eval_rank_planes(const void* A_planes, int64_t a_rows, const void* B_planes, int64_t b_rows, int64_t K,
                         int64_t M, int64_t N, const int64_t* truth, const int64_t* filter_ptr,
                         const int64_t* filter_ids, int64_t nfilter, int64_t* ranks, void* workspace,
                         size_t workspace_bytes, void* stream) {
    return kge_eval_rank_planes_ex(A_planes, a_rows, B_planes, b_rows, K, M, N, truth, filter_ptr, filter_ids, nfilter,
                                   ranks, workspace, workspace_bytes, nullptr, stream);
}

int kge_eval_rank_planes_ex(const void* A_planes, int64_t a_rows, const void* B_planes, int64_t b_rows, int64_t K,
                            int64_t M, int64_t N, const int64_t* truth, const int64_t* filter_ptr,
                            const int64_t* filter_ids, int64_t nfilter, int64_t* ranks, void* workspace,
                            size_t workspace_bytes, const kge_forms* forms, void* stream) {
    return kge_eval_rank_planes_phases(A_planes, a_rows, B_planes, b_rows, K, M, N, truth, filter_ptr, filter_ids,
                                       nfilter, ranks, workspace, workspace_bytes, KGE_RANK_ALL, forms, stream);
}

int kge_eval_rank_planes_phases(const void* A_planes, int64_t a_rows, const void* B_planes, int64_t b_rows, int64_t K,
                                int64_t M, int64_t N, const int64_t* truth, const int64_t* filter_ptr,
                                const int64_t* filter_ids, int64_t nfilter, int64_t* ranks, void* workspace,
                                size_t workspace_bytes, int phases, const kge_forms* forms, void* stream) {
    if (phases <= 0 || phases > KGE_RANK_ALL) return fail(KGE_EINVAL, "kge_eval_rank_planes: phases must be 1..7");
    const int form = forms && (forms->gemm_form == 1 || forms->gemm_form >= 3) && forms->gemm_form <= 4
                         ? forms->gemm_form
                         : (kPlanesGemmForm == 2 ? 1 : kPlanesGemmForm);
    if (M < 0 || N <= 0 || K <= 0 || M > a_rows || N > b_rows || nfilter < 0) return fail(KGE_EINVAL, "bad shape");
    if (M == 0) return ok();
    if (!A_planes || !B_planes || !truth || !ranks || !workspace || (filter_ptr && !filter_ids && nfilter > 0) ||
        (nfilter > 0 && !filter_ptr))
        return fail(KGE_EINVAL, "null pointer");
    if (M > INT32_MAX || N > INT32_MAX || !aligned(A_planes, 16) || !aligned(B_planes, 16) || !aligned(workspace, 16))
        return fail(KGE_EINVAL, "kge_eval_rank_planes: int32 shapes and 16-B aligned planes / workspace");
    if (kge_split_bf16x3_bytes(a_rows, K) >= ((int64_t)1 << 32) - 16 ||
        kge_split_bf16x3_bytes(b_rows, K) >= ((int64_t)1 << 32) - 16)
        return fail(KGE_ENOTSUP, "kge_eval_rank_planes: planes past 4 GB");
    if ((int64_t)workspace_bytes < eval_rank_ws_bytes(M, nfilter))
        return fail(KGE_EINVAL, "kge_eval_rank_planes: workspace too small");
    launch_eval_rank_planes(A_planes, a_rows, B_planes, b_rows, K, (int)M, (int)N, truth, filter_ptr, filter_ids,
                            nfilter, ranks, workspace, (hipStream_t)stream, form, phases);
    return check_launch("kge_eval_rank_planes");
}

int64_t kge_eval_rank_sweep_workspace_size(int64_t B, int64_t nfilter) {
    if (B < 0 || nfilter < 0) return 0;
    return eval_rank_ws_bytes(B, nfilter);
}

int kge_eval_rank_sweep(int fn, int mode, const float* ent, int64_t nentity, int64_t ent_ld, const float* rel,
                        int64_t nrelation, int64_t rel_ld, int64_t rel_off, const int64_t* pos, int64_t B, int64_t D,
                        float gamma, float emb_range, float modulus, const int64_t* truth, const int64_t* filter_ptr,
                        const int64_t* filter_ids, int64_t nfilter, int64_t* ranks, void* workspace,
                        size_t workspace_bytes, void* stream) {
    if (!valid_fn(fn)) return fail(KGE_EINVAL, "unknown score function id " + std::to_string(fn));
    if (mode != KGE_HEAD_BATCH && mode != KGE_TAIL_BATCH)
        return fail(KGE_EINVAL, "kge_eval_rank_sweep: mode must be 0 (head-batch) or 1 (tail-batch)");
    if (B < 0 || D <= 0 || nentity <= 0 || nrelation <= 0 || nfilter < 0) return fail(KGE_EINVAL, "bad shape");
    if (fn == KGE_DISTMULT || fn == KGE_COMPLEX)
        return fail(KGE_ENOTSUP, "kge_eval_rank_sweep: DistMult / ComplEx rank through kge_eval_rank_planes");
    if (B == 0) return ok();
    if (!ent || !rel || !pos || !truth || !ranks || !workspace || (nfilter > 0 && (!filter_ptr || !filter_ids)))
        return fail(KGE_EINVAL, "null pointer");
    if (B > INT32_MAX || nentity > INT32_MAX || B + nfilter > INT32_MAX || !aligned(workspace, 16))
        return fail(KGE_EINVAL, "kge_eval_rank_sweep: int32 shapes and a 16-B aligned workspace");
    if ((int64_t)workspace_bytes < eval_rank_ws_bytes(B, nfilter))
        return fail(KGE_EINVAL, "kge_eval_rank_sweep: workspace too small");
    const Tables t = {fn, ent, nentity, ent_ld, rel, nrelation, rel_ld, rel_off, D, gamma, emb_range, modulus};
    ScoreParams p;
    fill_indexed(p, t, {mode, pos, nullptr, 0, B, nentity});
    int V = 1, G = 1;
    int rc = pick_vg(p, V, G);
    if (rc) return rc;
    if (G > kSweepMaxG) return fail(KGE_ENOTSUP, "kge_eval_rank_sweep: per-half dim past " + std::to_string(kSweepMaxG * kWave * V));
    if (nfilter == 0) filter_ptr = filter_ids = nullptr;
    float* ts = static_cast<float*>(workspace);
    p.rk.truth = truth;
    p.rk.fptr = filter_ptr;
    p.rk.fids = filter_ids;
    p.rk.nf = nfilter;
    p.rk.ts = ts;
    p.rk.cnt = reinterpret_cast<int*>(ts + B);
    p.rk.fs = reinterpret_cast<float*>(static_cast<unsigned char*>(workspace) + ((B * 8 + 15) / 16 * 16));
    // query rows per block: as many operand images as the LDS budget holds, at most kSweepMaxRows
    const int64_t row_lds = (int64_t)shard_nq(fn) * G * kWave * V * 4 + 8;  // + truth score, count
    const int64_t R = std::min<int64_t>(std::min<int64_t>(kSweepMaxRows, B), kSweepLdsMax / row_lds);
    const int64_t groups = (B + R - 1) / R, S = (nentity + 7) / 8;
    // a grid of fewer than kSweepMinBlocks blocks cuts every slice into contiguous chunks (of at least
    // 2 kSweepWaves rows: one pair of rows per wave)
    const int64_t want = (kSweepMinBlocks + groups * 8 - 1) / (groups * 8);
    const int64_t most = std::max<int64_t>(1, S / (2 * kSweepWaves));
    p.tile_rows = (int)R;
    p.tile_lds = (int)(R * row_lds);
    p.rk.chunks = (int)std::max<int64_t>(1, std::min(want, most));
    rc = run_score(fn, mode, p, KIND_RANK_PAIRS, stream);
    if (rc) return rc;
    rc = run_score(fn, mode, p, KIND_RANK_SWEEP, stream);
    if (rc) return rc;
    launch_rank_finish(B, nentity, truth, filter_ptr, filter_ids, workspace, ranks, (hipStream_t)stream);
    return check_launch("kge_eval_rank_sweep");
}

int kge_eval_rank_candidates(int fn, int mode, const float* ent, int64_t nentity, int64_t ent_ld, const float* rel,
                             int64_t nrelation, int64_t rel_ld, int64_t rel_off, const int64_t* pos, int64_t M,
                             int64_t D, float gamma, float emb_range, float modulus, const int64_t* truth,
                             const int64_t* cand, int64_t cand_ld, int64_t C, const int64_t* filter_ptr,
                             const int64_t* filter_ids, int64_t nfilter, int64_t* ranks, int64_t* ties,
                             float* truth_scores, void* stream) {
    if (!valid_fn(fn)) return fail(KGE_EINVAL, "unknown score function id " + std::to_string(fn));
    if (mode != KGE_HEAD_BATCH && mode != KGE_TAIL_BATCH)
        return fail(KGE_EINVAL, "kge_eval_rank_candidates: mode must be 0 (head-batch) or 1 (tail-batch)");
    if (M < 0 || C < 0 || D <= 0 || nentity < 0 || nrelation < 0 || nfilter < 0 || cand_ld < 0)
        return fail(KGE_EINVAL, "kge_eval_rank_candidates: bad shape");
    if (cand_ld > 0 && cand_ld < C)
        return fail(KGE_EINVAL, "kge_eval_rank_candidates: cand_ld must be 0 (one shared list) or >= C");
    if (M == 0) return ok();
    if (!ent || !rel || !pos || !truth || !ranks) return fail(KGE_EINVAL, "kge_eval_rank_candidates: null pointer");
    if (C > 0 && !cand) return fail(KGE_EINVAL, "kge_eval_rank_candidates: cand must not be NULL with C > 0");
    if (nfilter > 0 && (!filter_ptr || !filter_ids))
        return fail(KGE_EINVAL, "kge_eval_rank_candidates: null filter pointer with nfilter > 0");
    const Tables t = {fn, ent, nentity, ent_ld, rel, nrelation, rel_ld, rel_off, D, gamma, emb_range, modulus};
    if (nfilter == 0) filter_ptr = filter_ids = nullptr;
    // a launch takes at most kRows query rows (a block per row at the widest); more rows are further launches
    constexpr int64_t kRows = (int64_t)1 << 30;
    for (int64_t r0 = 0; r0 < M; r0 += kRows) {
        const int64_t n = std::min(kRows, M - r0);
        ScoreParams p;
        fill_indexed(p, t, {mode, pos + 3 * r0, cand ? cand + r0 * cand_ld : nullptr, cand_ld, n, C});
        p.rk.truth = truth + r0;
        p.rk.fptr = filter_ptr ? filter_ptr + r0 : nullptr;  // the starts are offsets into filter_ids: no rebase
        p.rk.fids = filter_ids;
        p.rk.nf = nfilter;
        p.rk.ts = truth_scores ? truth_scores + r0 : nullptr;
        p.rc.ranks = ranks + r0;
        p.rc.ties = ties ? ties + r0 : nullptr;
        const int rc = run_score(fn, mode, p, KIND_RANK_CAND, stream);  // refuses a width as kge_score_indexed does
        if (rc) return rc;
    }
    return ok();
}

int64_t kge_eval_topk_sweep_workspace_size(int64_t B, int64_t k) {
    if (B < 0 || B > INT32_MAX || k < 1 || k > kTopkMax) return 0;
    return (topk_ws_lists(B) * k * 8 + 15) / 16 * 16;
}

int kge_eval_topk_sweep(int fn, int mode, const float* ent, int64_t nentity, int64_t ent_ld, const float* rel,
                        int64_t nrelation, int64_t rel_ld, int64_t rel_off, const int64_t* pos, int64_t B, int64_t D,
                        float gamma, float emb_range, float modulus, const int64_t* excl_ptr, const int64_t* excl_ids,
                        int64_t nexcl, int64_t k, int64_t* out_ids, int64_t ids_ld, float* out_scores,
                        int64_t scores_ld, void* workspace, size_t workspace_bytes, void* stream) {
    if (!valid_fn(fn)) return fail(KGE_EINVAL, "unknown score function id " + std::to_string(fn));
    if (mode != KGE_HEAD_BATCH && mode != KGE_TAIL_BATCH)
        return fail(KGE_EINVAL, "kge_eval_topk_sweep: mode must be 0 (head-batch) or 1 (tail-batch)");
    if (k < 1 || k > kTopkMax) return fail(KGE_EINVAL, "kge_eval_topk_sweep: k must be 1 .. " + std::to_string(kTopkMax));
    if (B < 0 || D <= 0 || nentity <= 0 || nrelation <= 0 || nexcl < 0) return fail(KGE_EINVAL, "bad shape");
    if (fn == KGE_DISTMULT || fn == KGE_COMPLEX)
        return fail(KGE_ENOTSUP, "kge_eval_topk_sweep: DistMult / ComplEx select from the score matrix (kge_topk_rows)");
    if (B == 0) return ok();
    if (!ent || !rel || !pos || !out_ids || !out_scores || !workspace || (nexcl > 0 && (!excl_ptr || !excl_ids)))
        return fail(KGE_EINVAL, "null pointer");
    if (B > INT32_MAX || nentity > INT32_MAX || ids_ld < k || scores_ld < k || !aligned(workspace, 16))
        return fail(KGE_EINVAL, "kge_eval_topk_sweep: int32 shapes, row strides >= k and a 16-B aligned workspace");
    if ((int64_t)workspace_bytes < kge_eval_topk_sweep_workspace_size(B, k))
        return fail(KGE_EINVAL, "kge_eval_topk_sweep: workspace too small");
    const Tables t = {fn, ent, nentity, ent_ld, rel, nrelation, rel_ld, rel_off, D, gamma, emb_range, modulus};
    ScoreParams p;
    fill_indexed(p, t, {mode, pos, nullptr, 0, B, nentity});
    int V = 1, G = 1;
    int rc = pick_vg(p, V, G);
    if (rc) return rc;
    if (G > kSweepMaxG) return fail(KGE_ENOTSUP, "kge_eval_topk_sweep: per-half dim past " + std::to_string(kSweepMaxG * kWave * V));
    if (nexcl == 0) excl_ptr = excl_ids = nullptr;
    // query rows per block: the rows' operand images, every wave's list of k entries per row and the row's exclusion
    // range within one block's LDS, at most kSweepMaxRows
    const int64_t row_lds = (int64_t)shard_nq(fn) * G * kWave * V * 4 + (int64_t)kSweepWaves * k * 8 + 16;
    const int64_t R = std::min<int64_t>(std::min<int64_t>(kSweepMaxRows, B), kTileLdsMax / row_lds);
    if (R < 1) return fail(KGE_ENOTSUP, "kge_eval_topk_sweep: one query row does not fit the LDS");
    const int64_t groups = (B + R - 1) / R, S = (nentity + 7) / 8;
    const int64_t chunks = sweep_chunks(groups, S);
    if (B * 8 * chunks > topk_ws_lists(B)) return fail(KGE_EINVAL, "kge_eval_topk_sweep: workspace bound");
    p.tile_rows = (int)R;
    p.tile_lds = (int)(R * row_lds);
    p.tk.xptr = excl_ptr;
    p.tk.xids = excl_ids;
    p.tk.k = (int)k;
    p.tk.chunks = (int)chunks;
    p.tk.parts = static_cast<int2*>(workspace);
    rc = run_score(fn, mode, p, KIND_TOPK_SWEEP, stream);
    if (rc) return rc;
    launch_topk_merge(workspace, B, 8 * chunks, (int)k, out_ids, ids_ld, out_scores, scores_ld, (hipStream_t)stream);
    return check_launch("kge_eval_topk_sweep");
}

int kge_topk_rows(const float* scores, int64_t M, int64_t N, int64_t ld, const int64_t* excl_ptr,
                  const int64_t* excl_ids, int64_t nexcl, int64_t k, int64_t* out_ids, int64_t ids_ld,
                  float* out_scores, int64_t scores_ld, void* stream) {
    if (k < 1 || k > kTopkMax) return fail(KGE_EINVAL, "kge_topk_rows: k must be 1 .. " + std::to_string(kTopkMax));
    if (M < 0 || N < 0 || nexcl < 0) return fail(KGE_EINVAL, "bad shape");
    if (M == 0) return ok();
    if ((!scores && N > 0) || !out_ids || !out_scores || (nexcl > 0 && (!excl_ptr || !excl_ids)))
        return fail(KGE_EINVAL, "null pointer");
    if (M > INT32_MAX || N > INT32_MAX || ld < N || ids_ld < k || scores_ld < k)
        return fail(KGE_EINVAL, "kge_topk_rows: int32 shapes, ld >= N and output row strides >= k");
    if (nexcl == 0) excl_ptr = excl_ids = nullptr;
    launch_topk_rows(scores, M, N, ld, excl_ptr, excl_ids, (int)k, out_ids, ids_ld, out_scores, scores_ld,
                     (hipStream_t)stream);
    return check_launch("kge_topk_rows");
}

int64_t kge_eval_topk_planes_workspace_size(int64_t M, int64_t N, int64_t k) {
    if (M < 0 || M > INT32_MAX || N <= 0 || N > INT32_MAX || k < 1 || k > kTopkMax) return 0;
    return (M * eval_topk_planes_parts(N) * k * 8 + 15) / 16 * 16;
}

int kge_eval_topk_planes(const void* A_planes, int64_t a_rows, const void* B_planes, int64_t b_rows, int64_t K,
                         int64_t M, int64_t N, const int64_t* excl_ptr, const int64_t* excl_ids, int64_t nexcl,
                         int64_t k, int64_t* out_ids, int64_t ids_ld, float* out_scores, int64_t scores_ld,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (k < 1 || k > kTopkMax) return fail(KGE_EINVAL, "kge_eval_topk_planes: k must be 1 .. " + std::to_string(kTopkMax));
    if (M < 0 || N <= 0 || K <= 0 || M > a_rows || N > b_rows || nexcl < 0) return fail(KGE_EINVAL, "bad shape");
    if (M == 0) return ok();
    if (!A_planes || !B_planes || !out_ids || !out_scores || !workspace || (nexcl > 0 && (!excl_ptr || !excl_ids)))
        return fail(KGE_EINVAL, "null pointer");
    if (M > INT32_MAX || N > INT32_MAX || ids_ld < k || scores_ld < k || !aligned(A_planes, 16) ||
        !aligned(B_planes, 16) || !aligned(workspace, 16))
        return fail(KGE_EINVAL, "kge_eval_topk_planes: int32 shapes, row strides >= k, 16-B aligned planes / workspace");
    if (kge_split_bf16x3_bytes(a_rows, K) >= ((int64_t)1 << 32) - 16 ||
        kge_split_bf16x3_bytes(b_rows, K) >= ((int64_t)1 << 32) - 16)
        return fail(KGE_ENOTSUP, "kge_eval_topk_planes: planes past 4 GB");
    if ((int64_t)workspace_bytes < kge_eval_topk_planes_workspace_size(M, N, k))
        return fail(KGE_EINVAL, "kge_eval_topk_planes: workspace too small");
    if (nexcl == 0) excl_ptr = excl_ids = nullptr;
    launch_eval_topk_planes(A_planes, a_rows, B_planes, b_rows, K, (int)M, (int)N, excl_ptr, excl_ids, (int)k, out_ids,
                            ids_ld, out_scores, scores_ld, workspace, (hipStream_t)stream);
    return check_launch("kge_eval_topk_planes");
}

int kge_score_dense(int fn, int mode, const float* head, int64_t head_ld, const float* rel, int64_t rel_ld,
                    int64_t rel_off, const float* tail, int64_t tail_ld, int64_t B, int64_t N, int64_t D, float gamma,
                    float emb_range, float modulus, float* scores, int64_t scores_ld, void* stream) {
    int rc = check_fn_mode(fn, mode);
    if (rc) return rc;
    if (B < 0 || N < 0 || D <= 0) return fail(KGE_EINVAL, "bad shape (B, N, D)");
    if (empty(B, mode == KGE_SINGLE ? 1 : N)) return ok();
    if (!scores) return fail(KGE_EINVAL, "scores must not be NULL");
    ScoreParams p;
    fill_dense(p, fn, mode, head, head_ld, rel, rel_ld, rel_off, tail, tail_ld, B, N, D, gamma, emb_range, modulus);
    p.out = scores;
    p.out_ld = scores_ld;
    return run_score(fn, mode, p, KIND_FWD, stream);
}

int kge_score_dense_bwd(int fn, int mode, const float* head, int64_t head_ld, const float* rel, int64_t rel_ld,
                        int64_t rel_off, const float* tail, int64_t tail_ld, int64_t B, int64_t N, int64_t D,
                        float gamma, float emb_range, float modulus, const float* d_scores, int64_t d_ld,
                        float* d_head, float* d_rel, float* d_tail, float* d_modulus, void* stream) {
    int rc = check_fn_mode(fn, mode);
    if (rc) return rc;
    if (B < 0 || N < 0 || D <= 0) return fail(KGE_EINVAL, "bad shape (B, N, D)");
    if (empty(B, mode == KGE_SINGLE ? 1 : N)) return ok();
    if (!d_scores || !d_head || !d_rel || !d_tail) return fail(KGE_EINVAL, "null gradient pointer");
    ScoreParams p;
    fill_dense(p, fn, mode, head, head_ld, rel, rel_ld, rel_off, tail, tail_ld, B, N, D, gamma, emb_range, modulus);
    const bool ch = mode == KGE_HEAD_BATCH;
    p.d_scores = d_scores;
    p.d_ld = d_ld;
    p.d_qent = ch ? d_tail : d_head;
    p.d_cent = ch ? d_head : d_tail;
    p.d_rel = d_rel;
    p.d_modulus = d_modulus;
    return run_score(fn, mode, p, KIND_BWD, stream);
}

int kge_neg_reduce(const float* scores, int64_t B, int64_t N, int64_t ld, float temperature, int adversarial,
                   float* out, void* stream) {
    if (B < 0 || N <= 0) return fail(KGE_EINVAL, "bad shape (B, N)");
    if (B == 0) return ok();
    if (!scores || !out) return fail(KGE_EINVAL, "null pointer");
    const int64_t blocks = (B + kWavesPerBlock - 1) / kWavesPerBlock;
    hipLaunchKernelGGL(neg_reduce_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, scores, B, N,
                       ld, temperature, adversarial, out);
    return check_launch("kge_neg_reduce");
}

int kge_neg_reduce_bwd(const float* scores, int64_t B, int64_t N, int64_t ld, float temperature, int adversarial,
                       int detach, const float* d_out, float* d_scores, int64_t d_ld, void* stream) {
    if (B < 0 || N <= 0) return fail(KGE_EINVAL, "bad shape (B, N)");
    if (B == 0) return ok();
    if (!scores || !d_out || !d_scores) return fail(KGE_EINVAL, "null pointer");
    const int64_t blocks = (B + kWavesPerBlock - 1) / kWavesPerBlock;
    hipLaunchKernelGGL(neg_reduce_bwd_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, scores,
                       B, N, ld, temperature, adversarial, detach, d_out, d_scores, d_ld, nullptr, nullptr, nullptr);
    return check_launch("kge_neg_reduce_bwd");
}

int kge_log_sigmoid(const float* x, int64_t n, float* out, void* stream) {
    if (n < 0) return fail(KGE_EINVAL, "bad size");
    if (n == 0) return ok();
    if (!x || !out) return fail(KGE_EINVAL, "null pointer");
    hipLaunchKernelGGL(log_sigmoid_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, x, n, out);
    return check_launch("kge_log_sigmoid");
}

int kge_step_loss(const float* out_neg, const float* out_pos, const float* weight, int64_t B, float* loss,
                  float* d_out, void* stream) {
    if (B <= 0) return fail(KGE_EINVAL, "kge_step_loss needs B > 0");
    if (!out_neg || !out_pos || !weight || (!loss && !d_out)) return fail(KGE_EINVAL, "null pointer");
    hipLaunchKernelGGL(step_loss_kernel, dim3(1), dim3(kLossBlock), 0, (hipStream_t)stream, out_neg, out_pos, weight, B,
                       loss, d_out, (float*)nullptr);
    return check_launch("kge_step_loss");
}

int kge_log_sigmoid_bwd(const float* x, const float* d_out, int64_t n, float* d_x, void* stream) {
    if (n < 0) return fail(KGE_EINVAL, "bad size");
    if (n == 0) return ok();
    if (!x || !d_out || !d_x) return fail(KGE_EINVAL, "null pointer");
    hipLaunchKernelGGL(log_sigmoid_bwd_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, x, d_out, n, d_x);
    return check_launch("kge_log_sigmoid_bwd");
}

int kge_adam_update(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                    float beta2, float eps, int64_t step, int keras, int zero_grad, void* stream) {
    if (n < 0 || step < 1) return fail(KGE_EINVAL, "bad size or step (step is 1-based)");
    if (n == 0) return ok();
    if (!param || !grad || !exp_avg || !exp_avg_sq) return fail(KGE_EINVAL, "null pointer");
    if (!aligned(param, 4) || !aligned(grad, 4) || !aligned(exp_avg, 4) || !aligned(exp_avg_sq, 4))
        return fail(KGE_EINVAL, "adam buffers must be 4-byte aligned fp32");
    const bool vec = aligned(param, 16) && aligned(grad, 16) && aligned(exp_avg, 16) && aligned(exp_avg_sq, 16);
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step);
    const double bc2 = 1.0 - std::pow((double)beta2, (double)step);
    AdamArgs a;
    a.b1 = beta1;
    a.b2 = beta2;
    a.eps = eps;
    a.alpha = (float)((double)lr * std::sqrt(bc2) / bc1);
    a.step_size = (float)((double)lr / bc1);
    a.bc2_sqrt = (float)std::sqrt(bc2);
    a.keras = keras;
    a.zero_grad = zero_grad;
    const int64_t per_block = (int64_t)kBlock * kAdamVec;
    const int64_t want = (n / 4 + per_block - 1) / per_block;
    if (want > INT32_MAX) return fail(KGE_EINVAL, "tensor too large for one launch");
    const int blocks = (int)std::max<int64_t>(1, want);
    if (vec)
        hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, param, grad, exp_avg,
                           exp_avg_sq, n, a);
    else
        hipLaunchKernelGGL(adam_scalar_kernel, dim3((unsigned)std::min<int64_t>(4096, (n + kBlock - 1) / kBlock)),
                           dim3(kBlock), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n, a);
    return check_launch("kge_adam_update");
}

// ---------------------------------------------------------------------------------------------
// Deterministic backward of the fused train step
// ---------------------------------------------------------------------------------------------
struct StepWs {
    float *d_ns, *d_ps, *qbuf, *qg_ent, *qg_rel, *dmod, *dqbuf;
    int *count, *off, *cursor, *code, *tiles;
    int64_t bytes;
};

static int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

static StepWs step_ws_layout(char* base, int64_t E, int64_t B, int64_t N, int64_t D, int64_t ent_w, int64_t rel_w) {
    StepWs w;
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        char* p = base ? base + o : nullptr;
        o += align256(bytes);
        return p;
    };
    w.d_ns = (float*)take(B * N * 4);
    w.d_ps = (float*)take(B * 4);
    w.qbuf = (float*)take(2 * B * 3 * D * 4);
    w.qg_ent = (float*)take(2 * B * ent_w * 4);
    w.qg_rel = (float*)take(2 * B * rel_w * 4);
    w.dmod = (float*)take(2 * B * 4);
    w.dqbuf = (float*)take(B * 3 * D * 4);
    w.count = (int*)take(E * 4);
    w.off = (int*)take((E + 1) * 4);
    w.cursor = (int*)take(E * 4);
    w.code = (int*)take((B * N + 3 * B) * 4);
    w.tiles = (int*)take(((E + 1023) / 1024 + 1) * 4);
    w.bytes = o;
    return w;
}

static int64_t ent_width(int fn, int64_t D) { return is_split(fn) ? 2 * D : D; }
static int64_t rel_width(int fn, int64_t D) { return (fn == KGE_COMPLEX || fn == KGE_PAIRRE) ? 2 * D : D; }
// Columns of a relation row that belong to the table (the rest of rel_ld is the caller's padding, which no
// entry point writes): InterHT rows hold three thirds (model.py:209) of which one is read; every other
// function reads its whole row. Never less than the part read, never more than the row stride.
static int64_t rel_table_width(int fn, int64_t D, int64_t rel_off, int64_t rel_ld) {
    const int64_t w = std::max(fn == KGE_INTERHT ? 3 * D : rel_width(fn, D), rel_off + rel_width(fn, D));
    return std::min(w, rel_ld);
}

int64_t kge_score_bwd_workspace_size(int fn, int mode, int64_t B, int64_t N, int64_t D) {
    (void)fn;
    (void)mode;
    (void)B;
    (void)N;
    (void)D;
    return 0;  // the atomic-scatter backward needs no scratch
}

int kge_score_indexed_bwd(int fn, int mode, const float* ent, int64_t nentity, int64_t ent_ld, const float* rel,
                          int64_t nrelation, int64_t rel_ld, int64_t rel_off, const int64_t* pos, const int64_t* neg,
                          int64_t neg_ld, int64_t B, int64_t N, int64_t D, float gamma, float emb_range, float modulus,
                          const float* d_scores, int64_t d_ld, float* d_ent, float* d_rel, float* d_modulus,
                          void* workspace, void* stream) {
    (void)workspace;
    int rc = check_fn_mode(fn, mode);
    if (rc) return rc;
    if (B < 0 || N < 0 || D <= 0) return fail(KGE_EINVAL, "bad shape (B, N, D)");
    if (empty(B, mode == KGE_SINGLE ? 1 : N)) return ok();
    if (!pos) return fail(KGE_EINVAL, "pos must not be NULL");
    if (mode != KGE_SINGLE && !neg) return fail(KGE_EINVAL, "neg must not be NULL in head/tail-batch mode");
    if (!d_scores || !d_ent || !d_rel) return fail(KGE_EINVAL, "null gradient pointer");
    const Tables t = {fn, ent, nentity, ent_ld, rel, nrelation, rel_ld, rel_off, D, gamma, emb_range, modulus};
    ScoreParams p;
    fill_indexed(p, t, {mode, pos, neg, neg_ld, B, N});
    p.d_scores = d_scores;
    p.d_ld = d_ld;
    p.d_qent = d_ent;
    p.d_cent = d_ent;
    p.d_rel = d_rel;
    p.d_modulus = d_modulus;
    return run_score(fn, mode, p, KIND_BWD, stream);
}

int64_t kge_step_backward_workspace_size(int fn, int64_t nentity, int64_t B, int64_t N, int64_t D) {
    if (!valid_fn(fn) || nentity < 0 || B < 0 || N < 0 || D <= 0) return -1;
    return step_ws_layout(nullptr, nentity, B, N, D, ent_width(fn, D), rel_width(fn, D)).bytes;
}

// Options of the shared backward body. The defaults are kge_step_backward's behaviour.
struct StepOpts {
    bool dq_ready = false;      // phase 1 done by the fused forward: dqbuf holds unscaled query gradients
    bool events_ready = false;  // the entity buckets were built by the caller (e.g. on a side stream)
    bool fused_dscores = false; // the positive score gradient comes out of the neg_reduce_bwd launch
    bool epilogue_done = false; // score gradients and both slots' chains done (KIND_STEP_EPILOGUE)
    float *rel_p = nullptr, *rel_m = nullptr, *rel_v = nullptr;  // Adam on the relation table, fused
    // kge_train_step_reg: the L3 regulariser (lambda; needs the fused Adam) and, with reg_finish, the launch that
    // adds its value to the loss and writes the log, between the entity pass and the relation update
    float reg = 0.f;
    bool reg_finish = false;
    float *reg_part = nullptr, *reg_chunk = nullptr;  // workspace: per-wave partials [4 E], chunk sums
    const float* loss_parts = nullptr;                // [2] positive and negative sample loss
    float *loss = nullptr, *loss_sum = nullptr, *log = nullptr;
    // kge_train_step_lazy (needs the fused Adam on both tables): phase 2 visits only the rows with events, listed
    // in the workspace behind the scan, and the relation update leaves relations no slot uses
    bool lazy = false;
    int *lz_list = nullptr, *lz_count = nullptr, *lz_tiles = nullptr;
};

static EvArgs ev_args(const Batch& b, int64_t E) {
    EvArgs a;
    a.pos = b.pos;
    a.neg = b.neg;
    a.neg_ld = b.neg_ld;
    a.B = b.B;
    a.N = b.N;
    a.E = E;
    a.qcol = b.mode == KGE_HEAD_BATCH ? 2 : 0;
    a.total = (int)(b.B * b.N + 3 * b.B);
    return a;
}

// bucket the gradient events by entity: count, exclusive scan, scatter (counting sort)
static int launch_events(const EvArgs& a, const StepWs& w, hipStream_t st) {
    if (hipMemsetAsync(w.count, 0, (size_t)(a.E * 4), st) != hipSuccess) return check_launch("memset");
    const unsigned eb = (unsigned)((a.total + kBlock - 1) / kBlock);
    if (a.total > 0) hipLaunchKernelGGL(ev_count_kernel, dim3(eb), dim3(kBlock), 0, st, a, w.count);
    if (a.E > 0)
        hipLaunchKernelGGL(scan_block_kernel, dim3(1), dim3(kScanTile), 0, st, w.count, a.E, w.off, w.cursor, 1,
                           a.total);
    if (a.total > 0) hipLaunchKernelGGL(ev_scatter_kernel, dim3(eb), dim3(kBlock), 0, st, a, w.cursor, w.code);
    return check_launch("kge_step_backward events");
}

// the streaming forms of the backward (KIND_BWD_STREAM, KIND_BWD_ENT_STREAM): every wave of the block owns whole
// column groups
static bool stream_form(int G) { return G >= kWavesPerBlock && G % kWavesPerBlock == 0 && G <= kMaxG; }

static void set_adam(ScoreParams& p, const AdamArgs& a, float* m, float* v) {
    p.adam.on = 1;
    p.adam.m = m;
    p.adam.v = v;
    p.adam.b1 = a.b1;
    p.adam.b2 = a.b2;
    p.adam.eps = a.eps;
    p.adam.alpha = a.alpha;
    p.adam.step_size = a.step_size;
    p.adam.bc2_sqrt = a.bc2_sqrt;
    p.adam.keras = a.keras;
}

static int step_backward_impl(const Tables& t, const Batch& b, const StepGrads& g, void* workspace,
                              int64_t workspace_bytes, void* stream, const AdamArgs* adam, float* m_ent, float* v_ent,
                              const StepOpts& o = StepOpts()) {
    const int fn = t.fn, mode = b.mode;
    const int64_t B = b.B, N = b.N;
    int rc = check_fn_mode(fn, mode);
    if (rc) return rc;
    if (mode == KGE_SINGLE) return fail(KGE_EINVAL, "kge_step_backward needs a negative mode (0 or 1)");
    if (B < 0 || N <= 0 || t.D <= 0 || t.nentity < 0 || t.nrelation < 0) return fail(KGE_EINVAL, "bad shape");
    // the sharded train step's backward on a rank without rows (o.epilogue_done, nentity 0) has no table and no
    // moments: phase 2 is skipped below
    const bool no_rows = o.epilogue_done && t.nentity == 0;
    if ((!t.ent && !no_rows) || !t.rel || !b.pos || !b.neg || !g.neg_scores || !g.pos_scores || !g.d_out_neg ||
        !g.d_out_pos || !g.d_rel || (!adam && !g.d_ent) || (adam && !no_rows && (!m_ent || !v_ent)))
        return fail(KGE_EINVAL, "null pointer");
    if (B * N + 3 * B >= (int64_t)INT32_MAX || t.nentity >= (int64_t)INT32_MAX)
        return fail(KGE_EINVAL, "too many gradient events for 32-bit codes");
    rc = check_rel_width(fn, t.D, t.rel_off, t.rel_ld);
    if (rc) return rc;
    const int64_t ent_w = ent_width(fn, t.D), rel_w = rel_width(fn, t.D);
    // relation rows are written over the table's width (the parts no score function reads get a zero
    // gradient), never over the padding of a row stride wider than the table
    const int64_t rel_dim = rel_table_width(fn, t.D, t.rel_off, t.rel_ld);
    StepWs w = step_ws_layout((char*)workspace, t.nentity, B, N, t.D, ent_w, rel_w);
    if (!workspace || workspace_bytes < w.bytes) return fail(KGE_EINVAL, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    if (B == 0 && !adam) {
        // the tables' columns only: the last row of a padded buffer may end at its width
        if ((t.nentity > 0 && hipMemset2DAsync(g.d_ent, (size_t)(t.ent_ld * 4), 0, (size_t)(ent_w * 4),
                                               (size_t)t.nentity, st) != hipSuccess) ||
            (t.nrelation > 0 && rel_dim > 0 &&
             hipMemset2DAsync(g.d_rel, (size_t)(t.rel_ld * 4), 0, (size_t)(rel_dim * 4), (size_t)t.nrelation, st) !=
                 hipSuccess))
            return check_launch("kge_step_backward memset");
        if (g.d_modulus && hipMemsetAsync(g.d_modulus, 0, 4, st) != hipSuccess) return check_launch("memset");
        return ok();
    }
    // 1. loss -> score gradients
    if (o.epilogue_done) {
        rc = 0;
    } else if (o.fused_dscores) {
        const unsigned nb = (unsigned)((B + kWavesPerBlock - 1) / kWavesPerBlock);
        hipLaunchKernelGGL(neg_reduce_bwd_kernel, dim3(nb), dim3(kBlock), 0, st, g.neg_scores, B, N, g.ns_ld,
                           g.temperature, g.adversarial, g.detach, g.d_out_neg, w.d_ns, N, g.pos_scores, g.d_out_pos,
                           w.d_ps);
        rc = check_launch("kge_step_backward score gradients");
    } else {
        rc = kge_neg_reduce_bwd(g.neg_scores, B, N, g.ns_ld, g.temperature, g.adversarial, g.detach, g.d_out_neg,
                                w.d_ns, N, stream);
        if (rc) return rc;
        rc = kge_log_sigmoid_bwd(g.pos_scores, g.d_out_pos, B, w.d_ps, stream);
    }
    if (rc) return rc;
    // 2. phase 1: per-slot query gradients (negative call, then positive call)
    ScoreParams p;
    fill_indexed(p, t, b);
    p.d_scores = w.d_ns;
    p.d_ld = N;
    p.qbuf = w.qbuf;
    p.qg_ent = w.qg_ent;
    p.qg_rel = w.qg_rel;
    p.dmod_part = w.dmod;
    p.ent_w = ent_w;
    p.rel_w = rel_w;
    p.slot0 = 0;
    // streaming form when every wave of the block owns whole column groups (G a multiple of 4) and
    // InterHT's candidate norms are available from the forward; the register-resident form otherwise
    int V1 = 1, G1 = 1;
    rc = pick_vg(p, V1, G1);
    if (rc) return rc;
    if (o.epilogue_done) {
        rc = 0;
    } else if (o.dq_ready) {
        // the fused forward (KIND_STEP_FWD_GRAD) left each row's query gradient, unscaled, in dqbuf
        p.dqbuf = w.dqbuf;
        p.dq_scale = g.d_out_neg;
        rc = run_score(fn, mode, p, KIND_BWD_CHAIN, stream);
    } else if (stream_form(G1) && kind_has(KIND_BWD_STREAM, fn, false, G1) && (fn != KGE_INTERHT || g.cand_stats)) {
        // (PairRE has no streaming phase 1: the register-resident form recomputes its candidate norms)
        p.cand_stats = reinterpret_cast<float2*>(const_cast<float*>(g.cand_stats));
        p.dqbuf = w.dqbuf;
        rc = run_score(fn, mode, p, KIND_BWD_STREAM, stream);
        if (rc) return rc;
        rc = run_score(fn, mode, p, KIND_BWD_CHAIN, stream);
    } else {
        rc = run_score(fn, mode, p, KIND_BWD_ROWS, stream);
    }
    if (rc) return rc;
    ScoreParams pp;
    fill_indexed(pp, t, single_of(b));
    pp.d_scores = w.d_ps;
    pp.d_ld = 1;
    pp.qbuf = w.qbuf;
    pp.qg_ent = w.qg_ent;
    pp.qg_rel = w.qg_rel;
    pp.dmod_part = w.dmod;
    pp.ent_w = ent_w;
    pp.rel_w = rel_w;
    pp.slot0 = B;
    if (!o.epilogue_done) {
        rc = run_score(fn, KGE_SINGLE, pp, KIND_BWD_ROWS, stream);
        if (rc) return rc;
    }
    // 3. bucket the gradient events by entity
    if (!o.events_ready) {
        rc = launch_events(ev_args(b, t.nentity), w, st);
        if (rc) return rc;
    }
    // 4. phase 2: one wave per entity row, events in code order -> every row of d_ent written
    ScoreParams q;
    fill_indexed(q, t, b);
    q.qbuf = w.qbuf;
    q.qg_ent = w.qg_ent;
    q.ev_off = w.off;
    q.ev_code = w.code;
    q.d_ns = w.d_ns;
    q.d_ps = w.d_ps;
    q.Bn = B;
    q.Nn = N;
    q.ent_w = ent_w;
    q.d_out_ent = g.d_ent;
    if (adam) set_adam(q, *adam, m_ent, v_ent);
    const float reg3 = adam ? 3.f * o.reg : 0.f;
    q.reg3 = reg3;
    q.reg_part = o.reg_part;
    if (o.lazy && t.nentity > 0) {
        // the touched rows, ascending, from the global bucket offsets (two launches; kge_scan.h)
        const int ntot = (int)(B * N + 3 * B);
        const int64_t lt = (t.nentity + kTile4k - 1) / kTile4k;
        q.lz_rows = std::min<int64_t>(t.nentity, ntot);
        q.lz_list = o.lz_list;
        q.lz_count = o.lz_count;
        hipLaunchKernelGGL(lazy_count_kernel, dim3((unsigned)lt), dim3(kScanTile), 0, st, w.off, t.nentity, ntot,
                           o.lz_tiles);
        hipLaunchKernelGGL(lazy_list_kernel, dim3((unsigned)lt), dim3(kScanTile), 0, st, w.off, t.nentity, ntot,
                           o.lz_tiles, o.lz_list, (int)q.lz_rows, o.lz_count);
        rc = check_launch("kge_train_step_lazy row list");
        if (rc) return rc;
    }
    if (t.nentity > 0) {
        // streaming form (block per row, waves split the columns) under the same condition as phase 1
        rc = run_score(fn, mode, q, stream_form(G1) ? KIND_BWD_ENT_STREAM : KIND_BWD_ENT, stream);
        if (rc) return rc;
    }
    if (o.reg_finish) {
        // the regulariser's value from the entity pass' partials and the relation table, still unchanged
        int64_t nparts = 0, nb_ent = 0, nb_rel = 0;
        if (reg3 != 0.f) {
            nparts = t.nentity * (stream_form(G1) ? kWavesPerBlock : 1);
            nb_ent = (nparts + kRegChunk - 1) / kRegChunk;
            nb_rel = (t.nrelation * rel_dim + kRegChunk - 1) / kRegChunk;
            if (nb_ent + nb_rel > 0)
                hipLaunchKernelGGL(reg_chunk_kernel, dim3((unsigned)(nb_ent + nb_rel)), dim3(kBlock), 0, st,
                                   o.reg_part, nparts, nb_ent, t.rel, t.rel_ld, rel_dim, t.nrelation * rel_dim,
                                   o.reg_chunk);
        }
        hipLaunchKernelGGL(reg_finish_kernel, dim3(1), dim3(kBlock), 0, st, o.reg_chunk, nb_ent + nb_rel, o.reg,
                           o.loss_parts, o.loss, o.loss_sum, o.log);
    }
    // 5. relation rows (slot order) and the pRotatE modulus
    if (t.nrelation > 0 || g.d_modulus) {
        const int64_t rb = std::max<int64_t>(1, t.nrelation * ((rel_dim + kWave - 1) / kWave));
        RelAdam ra;
        memset(&ra, 0, sizeof(ra));
        if (adam && o.rel_p) {
            ra.p = o.rel_p;
            ra.m = o.rel_m;
            ra.v = o.rel_v;
            ra.a = *adam;
            ra.on = 1;
            ra.reg3 = reg3;
        }
        if (o.lazy && ra.on)
            hipLaunchKernelGGL(bwd_rel_kernel<true>, dim3((unsigned)rb), dim3(kRelWaves * kWave), 0, st, b.pos, B,
                               t.nrelation, w.qg_rel, rel_w, t.rel_off, g.d_rel, t.rel_ld, rel_dim, w.dmod,
                               g.d_modulus, ra);
        else
            hipLaunchKernelGGL(bwd_rel_kernel<false>, dim3((unsigned)rb), dim3(kRelWaves * kWave), 0, st, b.pos, B,
                               t.nrelation, w.qg_rel, rel_w, t.rel_off, g.d_rel, t.rel_ld, rel_dim, w.dmod,
                               g.d_modulus, ra);
    }
    return check_launch("kge_step_backward");
}

int kge_step_backward(int fn, int mode, const float* ent, int64_t nentity, int64_t ent_ld, const float* rel,
                      int64_t nrelation, int64_t rel_ld, int64_t rel_off, const int64_t* pos, const int64_t* neg,
                      int64_t neg_ld, int64_t B, int64_t N, int64_t D, float gamma, float emb_range, float modulus,
                      float temperature, int adversarial, int detach, const float* neg_scores, int64_t ns_ld,
                      const float* pos_scores, const float* d_out_neg, const float* d_out_pos, float* d_ent,
                      float* d_rel, float* d_modulus, const float* cand_stats, void* workspace,
                      int64_t workspace_bytes, void* stream) {
    const Tables t = {fn, ent, nentity, ent_ld, rel, nrelation, rel_ld, rel_off, D, gamma, emb_range, modulus};
    const StepGrads g = {temperature, adversarial, detach, neg_scores, ns_ld,    pos_scores,
                         d_out_neg,   d_out_pos,   d_ent,  d_rel,      d_modulus, cand_stats};
    return step_backward_impl(t, {mode, pos, neg, neg_ld, B, N}, g, workspace, workspace_bytes, stream, nullptr,
                              nullptr, nullptr);
}

// Adam coefficients of step t (1-based), in double on the host
static AdamArgs adam_args(float lr, float beta1, float beta2, float eps, int64_t step, int keras) {
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step);
    const double bc2 = 1.0 - std::pow((double)beta2, (double)step);
    AdamArgs a;
    a.b1 = beta1;
    a.b2 = beta2;
    a.eps = eps;
    a.alpha = (float)((double)lr * std::sqrt(bc2) / bc1);
    a.step_size = (float)((double)lr / bc1);
    a.bc2_sqrt = (float)std::sqrt(bc2);
    a.keras = keras;
    a.zero_grad = 0;
    return a;
}

int64_t kge_step_backward_adam_workspace_size(int fn, int64_t nentity, int64_t nrelation, int64_t rel_ld, int64_t B,
                                              int64_t N, int64_t D) {
    const int64_t base = kge_step_backward_workspace_size(fn, nentity, B, N, D);
    if (base < 0 || nrelation < 0 || rel_ld < 0) return -1;
    if (fn == KGE_PAIRRE && rel_ld < 2 * D) return -1;  // a row stride that cannot hold PairRE's two halves: no step
    return base + align256(nrelation * rel_ld * 4) + 256;
}

int kge_step_backward_adam(int fn, int mode, float* ent, int64_t nentity, int64_t ent_ld, float* rel,
                           int64_t nrelation, int64_t rel_ld, int64_t rel_off, const int64_t* pos, const int64_t* neg,
                           int64_t neg_ld, int64_t B, int64_t N, int64_t D, float gamma, float emb_range,
                           float* modulus_param, float modulus, float temperature, int adversarial, int detach,
                           const float* neg_scores, int64_t ns_ld, const float* pos_scores, const float* d_out_neg,
                           const float* d_out_pos, float* m_ent, float* v_ent, float* m_rel, float* v_rel,
                           float* m_mod, float* v_mod, float lr, float beta1, float beta2, float eps, int64_t step,
                           int keras, const float* cand_stats, void* workspace, int64_t workspace_bytes,
                           void* stream) {
    if (step < 1) return fail(KGE_EINVAL, "step is 1-based");
    if (!m_rel || !v_rel || (modulus_param && (!m_mod || !v_mod))) return fail(KGE_EINVAL, "null optimizer state");
    const int64_t base = kge_step_backward_workspace_size(fn, nentity, B, N, D);
    if (base < 0) return fail(KGE_EINVAL, "bad shape");
    if (!workspace || workspace_bytes < kge_step_backward_adam_workspace_size(fn, nentity, nrelation, rel_ld, B, N, D))
        return fail(KGE_EINVAL, "workspace too small");
    float* d_rel = (float*)((char*)workspace + base);
    float* d_mod = (float*)((char*)workspace + base + align256(nrelation * rel_ld * 4));
    const AdamArgs a = adam_args(lr, beta1, beta2, eps, step, keras);
    StepOpts o;
    o.rel_p = rel;  // Adam on the relation table inside the relation-gradient kernel
    o.rel_m = m_rel;
    o.rel_v = v_rel;
    const Tables t = {fn, ent, nentity, ent_ld, rel, nrelation, rel_ld, rel_off, D, gamma, emb_range, modulus};
    const StepGrads g = {temperature, adversarial, detach,  neg_scores, ns_ld,                           pos_scores,
                         d_out_neg,   d_out_pos,   nullptr, d_rel,      modulus_param ? d_mod : nullptr, cand_stats};
    int rc = step_backward_impl(t, {mode, pos, neg, neg_ld, B, N}, g, workspace, base, stream, &a, m_ent, v_ent, o);
    if (rc) return rc;
    // the pRotatE modulus (one element) goes through the dense optimizer kernel, with the same
    // adam_update as the fused rows
    if (modulus_param) {
        rc = kge_adam_update(modulus_param, d_mod, m_mod, v_mod, 1, lr, beta1, beta2, eps, step, keras, 0, stream);
        if (rc) return rc;
    }
    return ok();
}

// ---------------------------------------------------------------------------------------------
// One whole train step (supervisor.py:15-26 train_step_fn): both model calls with phase 1 of the
// backward fused into the forward, the weighted loss and its gradient, the deterministic backward
// with Adam fused into the entity pass, and Adam on the relation table.
// ---------------------------------------------------------------------------------------------
struct TrainWs {
    float *ns, *ps, *d_out, *stats;
    int64_t bwd_bytes, bytes;
};

static TrainWs train_ws_layout(char* base, int fn, int64_t E, int64_t R, int64_t rel_ld, int64_t B, int64_t N,
                               int64_t D) {
    TrainWs t;
    t.bwd_bytes = kge_step_backward_adam_workspace_size(fn, E, R, rel_ld, B, N, D);
    int64_t o = t.bwd_bytes;
    auto take = [&](int64_t bytes) {
        char* p = base ? base + o : nullptr;
        o += align256(bytes);
        return (float*)p;
    };
    t.ns = take(B * N * 4);
    t.ps = take(B * 4);
    t.d_out = take(B * 4);
    t.stats = take(B * N * 8);
    t.bytes = o;
    return t;
}

int64_t kge_train_step_workspace_size(int fn, int64_t nentity, int64_t nrelation, int64_t rel_ld, int64_t B, int64_t N,
                                      int64_t D) {
    if (kge_step_backward_adam_workspace_size(fn, nentity, nrelation, rel_ld, B, N, D) < 0) return -1;
    return train_ws_layout(nullptr, fn, nentity, nrelation, rel_ld, B, N, D).bytes;
}

// kge_train_step_reg's workspace: kge_train_step's, then the regulariser's per-wave partials (four per entity
// row), the chunk sums of reg_chunk_kernel and the two loss parts
struct RegWs {
    float *part, *chunk, *loss_parts;
    int64_t bytes;
};

static RegWs reg_ws_layout(char* base, int64_t train_bytes, int64_t E, int64_t R, int64_t rel_ld) {
    RegWs r;
    int64_t o = train_bytes;
    auto take = [&](int64_t bytes) {
        char* p = base ? base + o : nullptr;
        o += align256(bytes);
        return (float*)p;
    };
    const int64_t nparts = E * kWavesPerBlock;
    r.part = take(nparts * 4);
    r.chunk = take(((nparts + kRegChunk - 1) / kRegChunk + (R * rel_ld + kRegChunk - 1) / kRegChunk) * 4);
    r.loss_parts = take(2 * 4);
    r.bytes = o;
    return r;
}

int64_t kge_train_step_reg_workspace_size(int fn, int64_t nentity, int64_t nrelation, int64_t rel_ld, int64_t B,
                                          int64_t N, int64_t D) {
    const int64_t base = kge_train_step_workspace_size(fn, nentity, nrelation, rel_ld, B, N, D);
    if (base < 0) return -1;
    return reg_ws_layout(nullptr, base, nentity, nrelation, rel_ld).bytes;
}

// kge_train_step_lazy's workspace: kge_train_step_reg's, then the touched rows' list (min(E, events) ints: a batch
// touches no more rows than it has events), its count and the 4096-entity tiles' counts
struct LazyWs {
    int *list, *count, *tiles;
    int64_t bytes;
};

static LazyWs lazy_ws_layout(char* base, int64_t reg_bytes, int64_t E, int64_t B, int64_t N) {
    LazyWs l;
    int64_t o = reg_bytes;
    auto take = [&](int64_t bytes) {
        char* p = base ? base + o : nullptr;
        o += align256(bytes);
        return (int*)p;
    };
    l.list = take(std::min<int64_t>(E, B * N + 3 * B) * 4);
    l.count = take(4);
    l.tiles = take((E + kTile4k - 1) / kTile4k * 4);
    l.bytes = o;
    return l;
}

int64_t kge_train_step_lazy_workspace_size(int fn, int64_t nentity, int64_t nrelation, int64_t rel_ld, int64_t B,
                                           int64_t N, int64_t D) {
    const int64_t base = kge_train_step_reg_workspace_size(fn, nentity, nrelation, rel_ld, B, N, D);
    if (base < 0) return -1;
    return lazy_ws_layout(nullptr, base, nentity, B, N).bytes;
}

// kge_train_step (reg_entry false: weights required, no regulariser, no log, its own workspace size),
// kge_train_step_reg and kge_train_step_lazy (reg_entry with lambda 0, and `lazy`: Adam on the touched rows only)
// in one body. Every rejection comes before the first launch.
static int train_step_impl(int fn, int mode, float* ent, int64_t nentity, int64_t ent_ld, float* rel,
                           int64_t nrelation, int64_t rel_ld, int64_t rel_off, const int64_t* pos, const int64_t* neg,
                           int64_t neg_ld, int64_t B, int64_t N, int64_t D, float gamma, float emb_range,
                           float temperature, int adversarial, int detach, const float* weight, float* loss,
                           float* loss_sum, float* out_neg, float* out_pos, float* m_ent, float* v_ent, float* m_rel,
                           float* v_rel, float lr, float beta1, float beta2, float eps, int64_t step, int keras,
                           void* workspace, int64_t workspace_bytes, void* stream, bool reg_entry,
                           float regularization, float* log, bool lazy = false) {
    int rc = check_fn_mode(fn, mode);
    if (rc) return rc;
    if (fn == KGE_PROTATE) return fail(KGE_ENOTSUP, "kge_train_step: pRotatE uses kge_step_backward_adam");
    if (mode == KGE_SINGLE) return fail(KGE_EINVAL, "kge_train_step needs a negative mode (0 or 1)");
    if (!(regularization >= 0.f) || std::isinf(regularization))
        return fail(KGE_EINVAL, "kge_train_step_reg: regularization must be finite and >= 0");
    if (B <= 0 || N <= 0 || D <= 0 || nentity < 0 || nrelation < 0) return fail(KGE_EINVAL, "bad shape");
    if (step < 1) return fail(KGE_EINVAL, "step is 1-based");
    if (!ent || !rel || !pos || !neg || (!weight && !reg_entry) || !loss || !out_neg || !out_pos || !m_ent || !v_ent ||
        !m_rel || !v_rel)
        return fail(KGE_EINVAL, "null pointer");
    if (B * N + 3 * B >= (int64_t)INT32_MAX || nentity >= (int64_t)INT32_MAX)
        return fail(KGE_EINVAL, "too many gradient events for 32-bit codes");
    rc = check_rel_width(fn, D, rel_off, rel_ld);
    if (rc) return rc;
    const TrainWs t = train_ws_layout((char*)workspace, fn, nentity, nrelation, rel_ld, B, N, D);
    const RegWs rw = reg_ws_layout((char*)workspace, t.bytes, nentity, nrelation, rel_ld);
    const LazyWs lw = lazy_ws_layout((char*)workspace, rw.bytes, nentity, B, N);
    if (!workspace || workspace_bytes < (lazy ? lw.bytes : reg_entry ? rw.bytes : t.bytes))
        return fail(KGE_EINVAL, "workspace too small");
    // the finishing launch of the regulariser's value and the log; without it (kge_train_step; lambda 0 and no
    // log) the step is launch for launch the plain one
    const bool reg_finish = reg_entry && (regularization != 0.f || log);
    const int64_t base = kge_step_backward_workspace_size(fn, nentity, B, N, D);
    const StepWs w = step_ws_layout((char*)workspace, nentity, B, N, D, ent_width(fn, D), rel_width(fn, D));
    float* d_rel = (float*)((char*)workspace + base);
    hipStream_t st = (hipStream_t)stream;
    StepOpts o;
    o.fused_dscores = true;
    o.events_ready = true;
    o.rel_p = rel;
    o.rel_m = m_rel;
    o.rel_v = v_rel;
    o.reg = reg_entry ? regularization : 0.f;
    o.reg_finish = reg_finish;
    o.reg_part = rw.part;
    o.reg_chunk = rw.chunk;
    o.loss_parts = rw.loss_parts;
    o.loss = loss;
    o.loss_sum = loss_sum;  // with the finishing launch, the Sum metric advances there, by the loss with its term
    o.log = log;
    o.lazy = lazy;
    o.lz_list = lw.list;
    o.lz_count = lw.count;
    o.lz_tiles = lw.tiles;
    float* const parts = reg_finish ? rw.loss_parts : nullptr;
    float* const sum_now = reg_finish ? nullptr : loss_sum;

    // 1. forward of both model calls (supervisor.py:17-18); phase 1 of the backward fused in where its
    //    accumulators fit, and the gradient events counted into their entity buckets
    const Tables tab = {fn, ent, nentity, ent_ld, rel, nrelation, rel_ld, rel_off, D, gamma, emb_range, 0.f};
    const Batch batch = {mode, pos, neg, neg_ld, B, N};
    // the backward's loss side: the forward's scores and the loss kernel's (or the epilogue's) gradients, in the
    // workspace; Adam is fused, so no gradient table but the relation's
    StepGrads g = {temperature, adversarial, detach, t.ns, N, t.ps, t.d_out, t.d_out, nullptr, d_rel, nullptr, nullptr};
    ScoreParams p;
    fill_indexed(p, tab, batch);
    p.out = t.ns;
    p.out_ld = N;
    p.pos_base = pos;
    p.temperature = temperature;
    p.adversarial = adversarial;
    p.detach = detach;
    p.out_neg = out_neg;
    p.out_pos_raw = t.ps;
    p.out_pos_ls = out_pos;
    p.dqbuf = w.dqbuf;
    int V = 1, G = 1;
    rc = pick_vg(p, V, G);
    if (rc) return rc;
    const AdamArgs a = adam_args(lr, beta1, beta2, eps, step, keras);
    if (G > kFwdGradMaxG) {
        // fallback (D > 1024): the step forward, the loss kernel, then the backward with its own phase 1
        o.events_ready = false;
        p.cand_stats = reinterpret_cast<float2*>(t.stats);
        rc = run_score(fn, mode, p, fn == KGE_INTERHT ? KIND_STEP_FWD_STATS : KIND_STEP_FWD, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(step_loss_kernel, dim3(1), dim3(kLossBlock), 0, st, out_neg, out_pos, weight, B, loss,
                           t.d_out, parts);
        if (sum_now) hipLaunchKernelGGL(add_scalar_kernel, dim3(1), dim3(1), 0, st, loss, sum_now);
        rc = check_launch("kge_train_step loss");
        if (rc) return rc;
        g.cand_stats = t.stats;
        return step_backward_impl(tab, batch, g, workspace, base, stream, &a, m_ent, v_ent, o);
    }
    // the per-entity event counters are zeroed here, on every call: the workspace carries no state
    // between calls, so any workspace contents (fresh, shared, or left by an aborted call) are valid. The
    // size is rounded up inside the 256-B aligned region: an unaligned tail costs the runtime a second
    // fill kernel (~3-5 us on the step's critical path)
    if (nentity > 0 && hipMemsetAsync(w.count, 0, (size_t)align256(nentity * 4), st) != hipSuccess)
        return check_launch("kge_train_step memset");
    p.ev_count = w.count;
    rc = run_score(fn, mode, p, KIND_STEP_FWD_GRAD, stream);
    if (rc) return rc;
    // 2. bucket offsets (one launch): every 4096-entity tile scanned at once, the tiles' prefix added by the
    //    epilogue; one block walking all tiles for tables of more than 4M entities
    const int64_t ntiles = (nentity + kTile4k - 1) / kTile4k;
    const bool tiled = nentity > 0 && ntiles <= kEvMaxTiles;
    if (tiled)
        hipLaunchKernelGGL(scan_tiles4k_kernel, dim3((unsigned)ntiles), dim3(kScanTile), 0, st, w.count, nentity, w.off,
                           w.cursor, w.tiles);
    else
        hipLaunchKernelGGL(scan_block_kernel, dim3(1), dim3(kScanTile), 0, st, w.count, nentity, w.off, w.cursor, 0,
                           (int)(B * N + 3 * B));
    rc = check_launch("kge_train_step scan");
    if (rc) return rc;
    // 3. one launch: event scatter, loss weights, score gradients, both slots' query chains, the loss
    ScoreParams e = p;
    e.ev_count = nullptr;
    e.neg_scores = t.ns;
    e.ns_ld = N;
    e.d_ns = w.d_ns;
    e.d_ps = w.d_ps;
    e.qbuf = w.qbuf;
    e.qg_ent = w.qg_ent;
    e.qg_rel = w.qg_rel;
    e.ent_w = ent_width(fn, D);
    e.rel_w = rel_width(fn, D);
    e.weight = weight;
    e.pos_raw = t.ps;
    e.loss = loss;
    e.loss_sum = sum_now;
    e.loss_parts = parts;
    e.ev_cursor = w.cursor;
    e.ev_code_w = w.code;
    if (tiled) {
        e.ev_tile_sum = w.tiles;
        e.ev_off_fix = w.off;
        e.ev_ntiles = (int)ntiles;
    }
    rc = run_score(fn, mode, e, KIND_STEP_EPILOGUE, stream);
    if (rc) return rc;
    // 4. phase 2 with Adam fused into the entity pass, relation gradient with Adam (supervisor.py:25-26)
    o.dq_ready = o.epilogue_done = true;
    return step_backward_impl(tab, batch, g, workspace, base, stream, &a, m_ent, v_ent, o);
}

int kge_train_step(int fn, int mode, float* ent, int64_t nentity, int64_t ent_ld, float* rel, int64_t nrelation,
                   int64_t rel_ld, int64_t rel_off, const int64_t* pos, const int64_t* neg, int64_t neg_ld, int64_t B,
                   int64_t N, int64_t D, float gamma, float emb_range, float temperature, int adversarial, int detach,
                   const float* weight, float* loss, float* loss_sum, float* out_neg, float* out_pos,
                   float* m_ent, float* v_ent, float* m_rel, float* v_rel, float lr, float beta1, float beta2,
                   float eps, int64_t step, int keras, void* workspace, int64_t workspace_bytes, void* stream) {
    return train_step_impl(fn, mode, ent, nentity, ent_ld, rel, nrelation, rel_ld, rel_off, pos, neg, neg_ld, B, N, D,
                           gamma, emb_range, temperature, adversarial, detach, weight, loss, loss_sum, out_neg,
                           out_pos, m_ent, v_ent, m_rel, v_rel, lr, beta1, beta2, eps, step, keras, workspace,
                           workspace_bytes, stream, false, 0.f, nullptr);
}

int kge_train_step_reg(int fn, int mode, float* ent, int64_t nentity, int64_t ent_ld, float* rel, int64_t nrelation,
                       int64_t rel_ld, int64_t rel_off, const int64_t* pos, const int64_t* neg, int64_t neg_ld,
                       int64_t B, int64_t N, int64_t D, float gamma, float emb_range, float temperature,
                       int adversarial, int detach, const float* weight, float* loss, float* loss_sum, float* out_neg,
                       float* out_pos, float* m_ent, float* v_ent, float* m_rel, float* v_rel, float lr, float beta1,
                       float beta2, float eps, int64_t step, int keras, void* workspace, int64_t workspace_bytes,
                       void* stream, float regularization, float* log) {
    return train_step_impl(fn, mode, ent, nentity, ent_ld, rel, nrelation, rel_ld, rel_off, pos, neg, neg_ld, B, N, D,
                           gamma, emb_range, temperature, adversarial, detach, weight, loss, loss_sum, out_neg,
                           out_pos, m_ent, v_ent, m_rel, v_rel, lr, beta1, beta2, eps, step, keras, workspace,
                           workspace_bytes, stream, true, regularization, log);
}

// kge_train_step with a lazy Adam: only the rows a batch touches are read or written (see kge_hip.h)
int kge_train_step_lazy(int fn, int mode, float* ent, int64_t nentity, int64_t ent_ld, float* rel, int64_t nrelation,
                        int64_t rel_ld, int64_t rel_off, const int64_t* pos, const int64_t* neg, int64_t neg_ld,
                        int64_t B, int64_t N, int64_t D, float gamma, float emb_range, float temperature,
                        int adversarial, int detach, const float* weight, float* loss, float* loss_sum, float* out_neg,
                        float* out_pos, float* m_ent, float* v_ent, float* m_rel, float* v_rel, float lr, float beta1,
                        float beta2, float eps, int64_t step, int keras, void* workspace, int64_t workspace_bytes,
                        void* stream, float* log) {
    return train_step_impl(fn, mode, ent, nentity, ent_ld, rel, nrelation, rel_ld, rel_off, pos, neg, neg_ld, B, N, D,
                           gamma, emb_range, temperature, adversarial, detach, weight, loss, loss_sum, out_neg,
                           out_pos, m_ent, v_ent, m_rel, v_rel, lr, beta1, beta2, eps, step, keras, workspace,
                           workspace_bytes, stream, true, 0.f, log, true);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Row-sharded train step (owner-computes; kge_shard.h): supervisor.py:15-26 over the
// W replicas' batches, the entity table row-sharded over the W ranks, in three calls with the
// caller's two collectives between them.
// ---------------------------------------------------------------------------------------------
struct ShardWs {
    StepWs step;
    float *d_rel, *ns, *A, *Bv, *merged;
    int64_t base, bytes;
};

static ShardWs shard_ws_layout(char* ws, int fn, int64_t rows, int64_t R, int64_t rel_ld, int64_t Bg, int64_t N,
                               int64_t D) {
    ShardWs s;
    s.step = step_ws_layout(ws, rows, Bg, N, D, ent_width(fn, D), rel_width(fn, D));
    s.base = s.step.bytes;
    int64_t o = kge_step_backward_adam_workspace_size(fn, rows, R, rel_ld, Bg, N, D);
    s.d_rel = ws ? (float*)(ws + s.base) : nullptr;
    auto take = [&](int64_t bytes) {
        char* q = ws ? ws + o : nullptr;
        o += align256(bytes);
        return (float*)q;
    };
    const int64_t nqd = (int64_t)shard_nq(fn) * D;
    s.ns = take(Bg * N * 4);
    s.A = take(Bg * nqd * 4);
    s.Bv = take(Bg * nqd * 4);
    s.merged = take(Bg * 4 * 4);
    s.bytes = o;
    return s;
}

// what the three calls of the sharded train step share beyond the tables (the shard is t.ent) and the batch
struct ShardArgs {
    int64_t shard_lo;
    const float* qent;
    const float* qent_pos;
    int64_t q_ld, home_B;
    int world, rank;
    float temperature;
    int adversarial, detach;
    const float* weight;
};

static int shard_check(const Tables& t, const Batch& b, const ShardArgs& a, void* ws, int64_t ws_bytes) {
    int rc = check_fn_mode(t.fn, b.mode);
    if (rc) return rc;
    if (t.fn == KGE_PROTATE) return fail(KGE_ENOTSUP, "the sharded train step has no pRotatE modulus gradient");
    rc = refuse_sharded(t.fn, "the sharded train step");
    if (rc) return rc;
    if (b.mode == KGE_SINGLE) return fail(KGE_EINVAL, "the sharded train step needs a negative mode (0 or 1)");
    if (b.B <= 0 || b.N <= 0 || t.D <= 0 || t.nentity < 0 || a.world < 1 || a.rank < 0 || a.rank >= a.world ||
        a.home_B <= 0 || a.home_B * a.world != b.B)
        return fail(KGE_EINVAL, "bad shape: need Bg = world * home_B > 0, N, D > 0, 0 <= rank < world");
    // a rank that owns no rows (shard_rows 0: fewer entities than ranks) has no shard to point at
    if ((!t.ent && t.nentity > 0) || !a.qent || !a.qent_pos || !t.rel || !b.pos || !b.neg || !a.weight)
        return fail(KGE_EINVAL, "null pointer");
    if (b.B * b.N + 3 * b.B >= (int64_t)INT32_MAX || t.nentity >= (int64_t)INT32_MAX)
        return fail(KGE_EINVAL, "too many gradient events for 32-bit codes");
    if (!ws || ws_bytes < shard_ws_layout(nullptr, t.fn, t.nentity, 0, 0, b.B, b.N, t.D).bytes)
        return fail(KGE_EINVAL, "workspace too small");
    return 0;
}

static void shard_params(ScoreParams& p, const Tables& t, const Batch& b, const ShardArgs& a, const ShardWs& w) {
    fill_indexed(p, t, b);
    p.qent = a.qent;  // row b: the negative call's query entity (assembled by the caller)
    p.q_idx = nullptr;
    p.q_ld = a.q_ld;
    p.q_rows = b.B;
    p.qent_pos = a.qent_pos;
    p.c_base = a.shard_lo;
    p.pos_base = b.pos;
    p.temperature = a.temperature;
    p.adversarial = a.adversarial;
    p.detach = a.detach;
    p.weight = a.weight;
    p.home_B = a.home_B;
    p.world = a.world;
    p.rank = a.rank;
    p.nq = shard_nq(t.fn);
    p.out = w.ns;
    p.out_ld = b.N;
    p.neg_scores = w.ns;
    p.ns_ld = b.N;
    p.d_ns = w.step.d_ns;
    p.d_ps = w.step.d_ps;
    p.sh_A = w.A;
    p.sh_B = w.Bv;
    p.sh_merged = w.merged;
}

// The kernel instance of a sharded train call (p: shard_params and the call's dq), checked by all three calls
// before anything is launched or written. The train kinds keep kFwdGradMaxG groups of V floats per lane, so the
// step exists for D / V <= kFwdGradMaxG * 64: 1024 / 512 / 256 floats per half at vector width 4 / 2 / 1.
static int shard_instance(const ScoreParams& p) {
    int V = 1, G = 1;
    const int rc = pick_vg(p, V, G);  // (its own refusal, past kMaxG groups, is restated with this step's limit)
    if (rc || G > kFwdGradMaxG)
        return fail(KGE_ENOTSUP, "the sharded train step needs D / V <= " + std::to_string(kFwdGradMaxG * kWave) +
                                     " per half (D <= 1024 / 512 / 256 where every row stride, offset and base "
                                     "address is a multiple of 16 / 8 / 4 bytes): D = " + std::to_string(p.D) +
                                     " at vector width V = " + std::to_string(V));
    return 0;
}

extern "C" {

int kge_shard_nq(int fn) {
    if (refuse_sharded(fn, "kge_shard_nq")) return KGE_ENOTSUP;
    return valid_fn(fn) ? shard_nq(fn) : 0;
}

int64_t kge_shard_train_workspace_size(int fn, int64_t shard_rows, int64_t nrelation, int64_t rel_ld, int64_t Bg,
                                       int64_t N, int64_t D) {
    if (refuse_sharded(fn, "kge_shard_train_workspace_size")) return KGE_ENOTSUP;
    if (!valid_fn(fn) || shard_rows < 0 || nrelation < 0 || rel_ld < 0 || Bg < 0 || N < 0 || D <= 0) return -1;
    return shard_ws_layout(nullptr, fn, shard_rows, nrelation, rel_ld, Bg, N, D).bytes;
}

int kge_shard_train_forward(int fn, int mode, const float* shard, int64_t shard_rows, int64_t ent_ld, int64_t shard_lo,
                            const float* qent, const float* qent_pos, int64_t q_ld, const float* rel, int64_t nrelation,
                            int64_t rel_ld, int64_t rel_off, const int64_t* pos, const int64_t* neg, int64_t neg_ld,
                            int64_t Bg, int64_t N, int64_t D, int64_t home_B, int world, int rank, float gamma,
                            float emb_range, float temperature, int adversarial, int detach, const float* weight,
                            float* stats, float* dq, void* workspace, int64_t workspace_bytes, void* stream) {
    const Tables t = {fn, shard, shard_rows, ent_ld, rel, nrelation, rel_ld, rel_off, D, gamma, emb_range, 0.f};
    const Batch b = {mode, pos, neg, neg_ld, Bg, N};
    const ShardArgs a = {shard_lo, qent, qent_pos, q_ld, home_B, world, rank, temperature, adversarial, detach, weight};
    int rc = shard_check(t, b, a, workspace, workspace_bytes);
    if (rc) return rc;
    if (!stats || !dq) return fail(KGE_EINVAL, "null pointer");
    const ShardWs w = shard_ws_layout((char*)workspace, fn, shard_rows, nrelation, rel_ld, Bg, N, D);
    if (workspace_bytes < w.bytes) return fail(KGE_EINVAL, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    ScoreParams p;
    shard_params(p, t, b, a, w);
    p.ev_count = w.step.count;
    p.sh_stats = stats;
    p.sh_dq = dq;
    rc = shard_instance(p);
    if (rc) return rc;
    // per-call state only: the local rows' event counters are zeroed here
    if (shard_rows > 0 && hipMemsetAsync(w.step.count, 0, (size_t)align256(shard_rows * 4), st) != hipSuccess)
        return check_launch("kge_shard_train_forward memset");
    rc = run_score(fn, mode, p, KIND_SHARD_FWD_GRAD, stream);
    if (rc) return rc;
    p.ev_count = nullptr;
    return run_score(fn, KGE_TAIL_BATCH, p, KIND_SHARD_POS, stream);  // owned positives (tail formula)
}

int kge_shard_train_combine(int fn, int mode, const float* shard, int64_t shard_rows, int64_t ent_ld, int64_t shard_lo,
                            const float* qent, const float* qent_pos, int64_t q_ld, const float* rel, int64_t nrelation,
                            int64_t rel_ld, int64_t rel_off, const int64_t* pos, const int64_t* neg, int64_t neg_ld,
                            int64_t Bg, int64_t N, int64_t D, int64_t home_B, int world, int rank, float gamma,
                            float emb_range, float temperature, int adversarial, int detach, const float* weight,
                            const float* stats_all, float* dq, float* out_neg, float* out_pos_raw, float* out_pos,
                            void* workspace, int64_t workspace_bytes, void* stream) {
    const Tables t = {fn, shard, shard_rows, ent_ld, rel, nrelation, rel_ld, rel_off, D, gamma, emb_range, 0.f};
    const Batch b = {mode, pos, neg, neg_ld, Bg, N};
    const ShardArgs a = {shard_lo, qent, qent_pos, q_ld, home_B, world, rank, temperature, adversarial, detach, weight};
    int rc = shard_check(t, b, a, workspace, workspace_bytes);
    if (rc) return rc;
    if (!stats_all || !dq || !out_neg || !out_pos) return fail(KGE_EINVAL, "null pointer");
    const ShardWs w = shard_ws_layout((char*)workspace, fn, shard_rows, nrelation, rel_ld, Bg, N, D);
    if (workspace_bytes < w.bytes) return fail(KGE_EINVAL, "workspace too small");
    ScoreParams p;
    shard_params(p, t, b, a, w);
    p.sh_stats_all = stats_all;
    p.sh_dq = dq;
    p.out_neg = out_neg;
    p.out_pos_raw = out_pos_raw;
    p.out_pos_ls = out_pos;
    rc = shard_instance(p);  // the combine itself has one form; a step the other two calls refuse is refused here too
    if (rc) return rc;
    const int64_t blocks = (Bg + kWavesPerBlock - 1) / kWavesPerBlock;
    hipLaunchKernelGGL(shard_combine_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, p);
    return check_launch("kge_shard_train_combine");
}

int kge_shard_train_backward(int fn, int mode, float* shard, int64_t shard_rows, int64_t ent_ld, int64_t shard_lo,
                             const float* qent, const float* qent_pos, int64_t q_ld, float* rel, int64_t nrelation,
                             int64_t rel_ld, int64_t rel_off, const int64_t* pos, const int64_t* neg, int64_t neg_ld,
                             int64_t Bg, int64_t N, int64_t D, int64_t home_B, int world, int rank, float gamma,
                             float emb_range, float temperature, int adversarial, int detach, const float* weight,
                             const float* dq, float* loss, float* loss_sum, float* m_ent, float* v_ent, float* m_rel,
                             float* v_rel, float lr, float beta1, float beta2, float eps, int64_t step, int keras,
                             void* workspace, int64_t workspace_bytes, void* stream) {
    const Tables t = {fn, shard, shard_rows, ent_ld, rel, nrelation, rel_ld, rel_off, D, gamma, emb_range, 0.f};
    const Batch b = {mode, pos, neg, neg_ld, Bg, N};
    const ShardArgs a = {shard_lo, qent, qent_pos, q_ld, home_B, world, rank, temperature, adversarial, detach, weight};
    int rc = shard_check(t, b, a, workspace, workspace_bytes);
    if (rc) return rc;
    if (step < 1) return fail(KGE_EINVAL, "step is 1-based");
    if (!dq || !loss || (shard_rows > 0 && (!m_ent || !v_ent)) || !m_rel || !v_rel)
        return fail(KGE_EINVAL, "null pointer");
    const ShardWs w = shard_ws_layout((char*)workspace, fn, shard_rows, nrelation, rel_ld, Bg, N, D);
    if (workspace_bytes < w.bytes) return fail(KGE_EINVAL, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    ScoreParams e;
    shard_params(e, t, b, a, w);
    e.sh_dq = const_cast<float*>(dq);
    rc = shard_instance(e);
    if (rc) return rc;
    // bucket offsets of the owned rows' events (counted by the forward)
    if (shard_rows > 0)
        hipLaunchKernelGGL(scan_block_kernel, dim3(1), dim3(kScanTile), 0, st, w.step.count, shard_rows, w.step.off,
                           w.step.cursor, 0, (int)(Bg * N + 3 * Bg));
    rc = check_launch("kge_shard_train_backward scan");
    if (rc) return rc;
    e.qbuf = w.step.qbuf;
    e.qg_ent = w.step.qg_ent;
    e.qg_rel = w.step.qg_rel;
    e.ent_w = ent_width(fn, D);
    e.rel_w = rel_width(fn, D);
    e.loss = loss;
    e.loss_sum = loss_sum;
    e.ev_cursor = w.step.cursor;
    e.ev_code_w = w.step.code;
    rc = run_score(fn, mode, e, KIND_SHARD_EPILOGUE, stream);
    if (rc) return rc;
    // phase 2 with Adam fused into the shard's rows, relation gradient with Adam (supervisor.py:25-26)
    const AdamArgs adam = adam_args(lr, beta1, beta2, eps, step, keras);
    StepOpts o;
    o.dq_ready = o.epilogue_done = o.events_ready = true;
    o.rel_p = rel;
    o.rel_m = m_rel;
    o.rel_v = v_rel;
    const StepGrads g = {temperature, adversarial, detach,  w.ns,    N,       w.ns,
                         w.step.d_ps, w.step.d_ps, nullptr, w.d_rel, nullptr, nullptr};
    return step_backward_impl(t, b, g, workspace, w.base, stream, &adam, m_ent, v_ent, o);
}

}  // extern "C"
