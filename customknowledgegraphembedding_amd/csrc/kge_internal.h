// kge_internal.h — host/device shared definitions of libkge_hip.so (not part of the C-ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kge_hip.h"

namespace kge_impl {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kMaxG = 8;  // float4 groups per lane per half-row kept in VGPRs (D <= 2048)
constexpr int kBwdMaxG = 16;  // dword groups per lane of the backward's atomic-friendly layout (D <= 1024)

enum Kind {
    KIND_FWD = 0,
    KIND_BWD = 1,
    KIND_FINISH = 2,
    KIND_BWD_ROWS = 3,
    KIND_BWD_ENT = 4,
    KIND_BWD_STREAM = 5,  // phase 1, column-group streaming (one wave per column group, dq -> dqbuf)
    KIND_BWD_CHAIN = 6,   // phase 1 epilogue of the streaming form (one wave per slot)
    KIND_FWD_STATS = 7,   // forward that also keeps InterHT's candidate norms (train step)
    KIND_STEP_FWD = 8,    // fused train-step forward: block per batch row, negatives + finish in one launch
    KIND_STEP_FWD_STATS = 9,
    KIND_BWD_ENT_STREAM = 10,  // phase 2, column-group streaming (one block per entity row)
    KIND_STEP_FWD_GRAD = 11,   // train-step forward with phase 1 fused (kge_train_step)
    KIND_STEP_EPILOGUE = 12,   // kge_train_step: loss weights, score gradients, chains, loss (one wave per slot)
    KIND_SHARD_FWD_GRAD = 13,  // row-sharded train step: owned candidates' scores + partial softmax state
    KIND_SHARD_POS = 14,       // row-sharded train step: owned positives (score, gradient, query gradient)
    KIND_SHARD_EPILOGUE = 15,  // row-sharded train step: owned score gradients, every slot's chain, loss
    KIND_STEP_FWD_XCD = 16,    // kge_step_forward's negatives, XCD-sliced entity table, ascending ids per wave
    KIND_SCORE_SHARD_XCD = 17, // kge_score_indexed / kge_score_sharded in the same order (no positives)
    KIND_SHARD_BUCKET = 18,    // row-sharded forward: this rank's bucket (kge_shard_plan) scored, compact out
    KIND_STEP_FWD_TILE = 19,   // kge_step_forward's negatives + positives: row-group x XCD-slice tiles, one
                               // entity-sorted sweep per block (queries in LDS)
    KIND_SCORE_TILE = 20,      // kge_score_indexed in the same order (no positives)
    KIND_RANK_PAIRS = 21,      // kge_eval_rank_sweep: the truths' and the filter entries' scores (one wave per pair)
    KIND_RANK_SWEEP = 22,      // kge_eval_rank_sweep: every entity row against a group of query rows, counting
    KIND_TOPK_SWEEP = 23,      // kge_eval_topk_sweep: the same sweep, each wave keeping the best k per query row
    KIND_RANK_CAND = 24,       // kge_eval_rank_candidates: each query row against its own candidate list, counting
    KIND_COUNT
};
constexpr int kFwdGradMaxG = 4;  // the fused forward + query gradient keeps 6 accumulators per element
// rank_sweep_kernel: a wave holds two candidate rows and one query's operands in registers (G = 8 would spill)
constexpr int kSweepMaxG = 4;
// waves per block: 4 per SIMD (every G <= 4 instance stays under 128 VGPRs), so one wave's LDS query reads overlap
// another's VALU work; 8 waves measured 3-5 % slower, InterHT d 1 000 15 % (profiles/r08_rank_sweep_ab.txt)
constexpr int kSweepWaves = 16;
constexpr int kSweepMaxRows = 16;         // query rows per block
constexpr int kSweepLdsMax = 144 * 1024;  // operand images of one block
constexpr int kSweepMinBlocks = 256;      // blocks wanted before an entity slice is cut into chunks (one per CU)
// topk_sweep_kernel / topk_rows_kernel: a list is one entry per lane; an empty slot is (-inf, kTopkEmpty), behind
// every real entry in the lists' order (score descending, ties by ascending id)
constexpr int kTopkMax = KGE_TOPK_MAX;
constexpr int kTopkEmpty = 0x7fffffff;
static_assert(kTopkMax <= kWave, "one list entry per lane");
// chunks per entity slice of a top-k sweep of `groups` row groups over slices of S rows (kge_eval_rank_sweep's
// rule): a grid of fewer than kSweepMinBlocks blocks cuts every slice into contiguous chunks of at least
// 2 kSweepWaves rows (one pair of rows per wave)
inline int64_t sweep_chunks(int64_t groups, int64_t S) {
    const int64_t want = (kSweepMinBlocks + groups * 8 - 1) / (groups * 8);
    const int64_t most = S / (2 * kSweepWaves) > 1 ? S / (2 * kSweepWaves) : 1;
    const int64_t c = want < most ? want : most;
    return c > 1 ? c : 1;
}
// partial lists of the top-k sweep for B query rows: 8 slices x chunks, chunks <= ceil(kSweepMinBlocks / (8 groups))
// and B <= kSweepMaxRows groups', so B x chunks < kSweepMinBlocks / 8 * kSweepMaxRows + B
constexpr int64_t topk_ws_lists(int64_t B) { return 8 * ((int64_t)kSweepMinBlocks / 8 * kSweepMaxRows + B); }

// How run_score sizes a kind's grid (kWavesPerBlock waves per counted block; B = p.B, E = p.c_rows)
enum GridRule {
    GRID_WAVE_PER_ROW,        // B waves
    GRID_BLOCK_PER_ROW,       // B blocks
    GRID_WAVE_PER_ENT,        // E waves
    GRID_BLOCK_PER_ENT,       // E blocks
    GRID_XCD_SLICES,          // 8 slice blocks per 4 batch rows (times p.xcd_phases for KIND_STEP_FWD_XCD)
    GRID_TILE_GROUPS,         // 8 slice blocks per group of p.tile_rows rows, then the next plan's tail blocks
    GRID_CAND_PER_WAVE,       // B * ceil(N / cpw) waves, cpw picked from the shape
    GRID_STEP_EPILOGUE,       // a wave per slot (3 B), the event-scatter blocks, one loss block
    GRID_SHARD_EPILOGUE,      // a wave per slot (2 B), one loss block
    GRID_RANK_PAIRS,          // a wave per pair: B truths, then p.rk.nf filter entries
    GRID_RANK_SWEEP,          // a block per (group of p.tile_rows rows, entity slice, chunk of p.rk.chunks)
    GRID_TOPK_SWEEP,          // the same with p.tk.chunks chunks
    GRID_RANK_CAND,           // p.wpr = rank_cand_wpr(N) waves per row: ceil(B / (kWavesPerBlock / p.wpr)) blocks
};
// rank_cand_kernel: waves per query row, min(4, ceil(C / 64)) rounded up to a power of two (a list of up to 64
// entries takes one wave, so four rows share a block and none of its waves idles)
constexpr int rank_cand_wpr(int64_t C) { return C <= kWave ? 1 : (C <= 2 * kWave ? 2 : kWavesPerBlock); }

// What a kind needs, stated once: run_score checks a launch against its entry and launch_one / launch_shard
// take their `if constexpr` guards from the same entry (kind_has), so the host check and the set of
// instantiations cannot disagree. A new kind is one enum entry, one row here, one case of run_score's grid
// switch if its grid shape is new, and one branch of launch_one.
struct KindInfo {
    GridRule grid;
    bool ch;            // head-batch selects the CH instantiation (false: the kernel has the tail formula only)
    int max_g;          // groups per lane the kernel is instantiated for
    bool g_whole_waves; // G % kWavesPerBlock == 0: every wave of the block owns whole column groups
    bool no_protate;    // the fused forward + query gradient family: no pRotatE modulus gradient
    bool interht_only;  // keeps InterHT's candidate norms
    const char* what;   // check_launch's name for the launch
    bool distance_only = false;  // TransE, RotatE, pRotatE, InterHT, PairRE (DistMult / ComplEx rank through the planes)
    bool no_pairre = false;      // the row-sharded family, and the streaming phase 1 (which takes the candidates'
                                 // norms from the forward's InterHT-only stats): no PairRE instance
};
constexpr KindInfo kKinds[KIND_COUNT] = {
    /* KIND_FWD */             {GRID_CAND_PER_WAVE, true, kMaxG, false, false, false, "kge score launch"},
    /* KIND_BWD */             {GRID_CAND_PER_WAVE, true, kBwdMaxG, false, false, false, "kge score backward launch"},
    /* KIND_FINISH */          {GRID_WAVE_PER_ROW, false, kMaxG, false, false, false, "kge finish launch"},
    /* KIND_BWD_ROWS */        {GRID_BLOCK_PER_ROW, true, kMaxG, false, false, false, "kge score launch"},
    /* KIND_BWD_ENT */         {GRID_WAVE_PER_ENT, true, kMaxG, false, false, false, "kge score launch"},
    /* KIND_BWD_STREAM */      {GRID_BLOCK_PER_ROW, true, kMaxG, true, false, false, "kge score launch", false, true},
    /* KIND_BWD_CHAIN */       {GRID_WAVE_PER_ROW, true, kMaxG, false, false, false, "kge score launch"},
    /* KIND_FWD_STATS */       {GRID_CAND_PER_WAVE, true, kMaxG, false, false, true, "kge score launch"},
    /* KIND_STEP_FWD */        {GRID_BLOCK_PER_ROW, true, kMaxG, false, false, false, "kge score launch"},
    /* KIND_STEP_FWD_STATS */  {GRID_BLOCK_PER_ROW, true, kMaxG, false, false, true, "kge score launch"},
    /* KIND_BWD_ENT_STREAM */  {GRID_BLOCK_PER_ENT, true, kMaxG, true, false, false, "kge score launch"},
    /* KIND_STEP_FWD_GRAD */   {GRID_BLOCK_PER_ROW, true, kFwdGradMaxG, false, true, false, "kge score launch"},
    /* KIND_STEP_EPILOGUE */   {GRID_STEP_EPILOGUE, true, kFwdGradMaxG, false, true, false, "kge score launch"},
    /* KIND_SHARD_FWD_GRAD */  {GRID_BLOCK_PER_ROW, true, kFwdGradMaxG, false, true, false, "kge score launch", false, true},
    /* KIND_SHARD_POS */       {GRID_WAVE_PER_ROW, false, kFwdGradMaxG, false, true, false, "kge score launch", false, true},
    /* KIND_SHARD_EPILOGUE */  {GRID_SHARD_EPILOGUE, true, kFwdGradMaxG, false, true, false, "kge score launch", false, true},
    /* KIND_STEP_FWD_XCD */    {GRID_XCD_SLICES, true, kMaxG, false, false, false, "kge score launch"},
    /* KIND_SCORE_SHARD_XCD */ {GRID_XCD_SLICES, true, kMaxG, false, false, false, "kge score launch"},
    /* KIND_SHARD_BUCKET */    {GRID_XCD_SLICES, true, kMaxG, false, false, false, "kge score launch", false, true},
    /* KIND_STEP_FWD_TILE */   {GRID_TILE_GROUPS, true, kFwdGradMaxG, false, false, false, "kge score launch"},
    /* KIND_SCORE_TILE */      {GRID_TILE_GROUPS, true, kFwdGradMaxG, false, false, false, "kge score launch"},
    /* KIND_RANK_PAIRS */      {GRID_RANK_PAIRS, true, kSweepMaxG, false, false, false, "kge_eval_rank_sweep", true},
    /* KIND_RANK_SWEEP */      {GRID_RANK_SWEEP, true, kSweepMaxG, false, false, false, "kge_eval_rank_sweep", true},
    /* KIND_TOPK_SWEEP */      {GRID_TOPK_SWEEP, true, kSweepMaxG, false, false, false, "kge_eval_topk_sweep", true},
    /* KIND_RANK_CAND */       {GRID_RANK_CAND, true, kMaxG, false, false, false, "kge_eval_rank_candidates"},
};
// whether kind k has a (FN, CH, G) instantiation
constexpr bool kind_has(int k, int fn, bool ch, int G) {
    return G <= kKinds[k].max_g && (!kKinds[k].g_whole_waves || G % kWavesPerBlock == 0) &&
           (!kKinds[k].distance_only || (fn != KGE_DISTMULT && fn != KGE_COMPLEX)) &&
           (!kKinds[k].no_protate || fn != KGE_PROTATE) && (!kKinds[k].interht_only || fn == KGE_INTERHT) &&
           (!kKinds[k].no_pairre || fn != KGE_PAIRRE) && (kKinds[k].ch || !ch);
}
constexpr int kTileBuckets = 256;  // entity buckets of a slice (the block's counting sort)
constexpr int kTileRows = 16;     // rows per block the library takes when they fit (tile_plan)
// the most rows a block of a planned step holds (the planner's row rule, kge_step_planner_set_rows): it sizes the
// row arrays, the one-lane-per-row ballots and the planned prologue's two rows per wave (so also <= 2 x the waves)
constexpr int kTileMaxRows = 20;
constexpr int kTileLdsMax = 160 * 1024;
constexpr int kTileSortRel = 64;     // relation buckets of the tile kernel's row sort (ids >= 62 share one)
constexpr int kTileSortMaxB = 2048;  // batch rows the tile kernel sorts by relation in LDS
// LDS query operands per batch row of the tile kernel (InterHT's third, the relation, is read per candidate;
// PairRE's second is the other side's relation half)
constexpr int tile_nq(int fn) {
    return (fn == KGE_COMPLEX || fn == KGE_ROTATE || fn == KGE_INTERHT || fn == KGE_PAIRRE) ? 2 : 1;
}
// query operands a score function's gradient has (q0 always; q1 for the complex / split forms and PairRE; q2
// InterHT): the operand images of the rank / top-k sweeps and the row-sharded step's gradient width (which has
// no PairRE: kKinds' no_pairre)
constexpr int shard_nq(int fn) {
    return fn == KGE_INTERHT ? 3 : ((fn == KGE_COMPLEX || fn == KGE_ROTATE || fn == KGE_PAIRRE) ? 2 : 1);
}

// ---------------------------------------------------------------------------------------------
// The planned tile sweep's progress board (kge_step_planner_set_board): one 128-B line per entity slice, one
// int per row group. Wave 0 of the scoring block (group g, slice x) publishes at board[x * 32 + g] the entity
// bucket of the item it is taking (mirrored under a descending sweep, so progress always ascends; kSweepDone
// when its sweep has ended) as (tag << kSweepTagShift) | progress, tag = the planner's step sequence number.
// Every wave of the slice's blocks reads the line and naps once before an item that leads another block's
// entry of the same tag by more than `lead` buckets. A performance hint only: no wait depends on the board,
// so any content (garbage, entries of earlier steps, a wrapped tag) costs at most one nap per item per wave.
// The board is used only while every scoring block is resident (blocks <= the device's CUs, so groups <= 32).
// ---------------------------------------------------------------------------------------------
constexpr int kSweepBoardLine = 32;                   // ints per slice line (128 B)
constexpr int kSweepBoardInts = 8 * kSweepBoardLine;  // the whole board
constexpr int kSweepTagShift = 9;                     // progress: 0 .. kTileBuckets - 1, kSweepDone
constexpr int kSweepDone = (1 << kSweepTagShift) - 1;
constexpr int kSweepTagMask = (1 << (31 - kSweepTagShift)) - 1;
constexpr int kSweepNap = 8;  // s_sleep units of 64 clocks: ~0.2 us, about a tenth of a wave's time per item at C2
// The clock record of a planned step (kge_step_planner_set_clocks, profiling builds), int64 words of the 100 MHz
// clock: per scoring block (slice x, row group g: record x * groups + g) kSweepClkMarks words: [0] wave 0's sweep
// start, [1..3] wave 0 past buckets 64 / 128 / 192, [4] wave 0's sweep end, [5] the XCC id, [6] block entry,
// [7] unused, then per wave w at [kSweepClkWave + 2 w] its sweep's end and at [.. + 1] its exit (after the
// head-batch positives; 0 for waves the block does not have). After the 8 * groups scoring records, per plan block
// of the launch's tail two words: entry, thread 0's exit. kge_sweep_clk_words: the whole record.
constexpr int kSweepClkWave = 8;
constexpr int kSweepClkMarks = kSweepClkWave + 2 * 16;
constexpr int64_t kge_sweep_clk_words(int64_t groups) { return groups * 8 * kSweepClkMarks + groups * 2; }

// ---------------------------------------------------------------------------------------------
// The tile scorer's step plan (kge_step_plan / kge_step_forward_planned): everything step_fwd_tile_kernel
// derives from a batch's ids alone, made ahead of the step. int32 words:
//   [0, kPlanHdr)                 header: magic, B, N, mode, rows per group R, nentity, the relation sort flag
//   meta  [groups][R][4]          per row of a group in the block's row order: batch row b (-1 past the batch),
//                                 then its positive (h, r, t) with out-of-range ids as -1
//   soff  [groups][9]             per group, the start of each entity slice's items in its list, then the total
//   list  [groups][R (N + 1)][2]  per group, its items sorted by (slice, entity bucket): (candidate entity id
//                                 or -1 when out of range, row << 16 | column) — column N: the row's positive
// The plan is a snapshot of the batch's ids: the planned step reads no id but the plan's.
// ---------------------------------------------------------------------------------------------
constexpr int kPlanMagic = 0x4B475031;  // "KGP1"
constexpr int kPlanHdr = 16;
__host__ __device__ inline int64_t plan_groups(int64_t B, int R) { return (B + R - 1) / R; }
__host__ __device__ inline int64_t plan_soff(int64_t B, int R) { return kPlanHdr + plan_groups(B, R) * R * 4; }
__host__ __device__ inline int64_t plan_list(int64_t B, int R) { return (plan_soff(B, R) + plan_groups(B, R) * 9 + 3) & ~(int64_t)3; }
__host__ __device__ inline int64_t plan_words(int64_t B, int64_t N, int R) {
    return plan_list(B, R) + plan_groups(B, R) * R * (N + 1) * 2;
}
// one plan to make: the next batch's ids (same B, N) and where its plan goes
struct PlanArgs {
    const int64_t* pos;
    const int64_t* neg;
    int64_t neg_ld;
    int64_t B, N, nent, nrel;
    int mode;  // KGE_HEAD_BATCH / KGE_TAIL_BATCH
    int R;     // batch rows per group
    int sort;  // rows ranked by relation (InterHT, B <= kTileSortMaxB)
    int* plan;
};
// LDS ints of one plan block of NT threads: row list, (slice, bucket) counts, the relation sort's wave counts
__host__ __device__ constexpr int plan_lds_ints(int NT) {
    return kTileMaxRows + 8 * kTileBuckets + (kTileSortMaxB + NT - 1) / NT * (NT / 64) * kTileSortRel;
}

// Parameters of one scoring launch. Rows are addressed as base + row * ld (floats).
//   query entity row of batch row b:  q_idx ? q_idx[b * q_stride] : b
//   relation row of batch row b:      r_idx ? r_idx[b * r_stride] : b      (+ r_off floats)
//   candidate n of batch row b:       c_idx ? c_idx[b * c_stride + n] : b * c_dense + n
struct ScoreParams {
    const float* qent;
    const int64_t* q_idx;
    int64_t q_ld, q_stride, q_rows;
    const float* rel;
    const int64_t* r_idx;
    int64_t r_ld, r_stride, r_rows, r_off;
    const float* cent;
    const int64_t* c_idx;
    int64_t c_ld, c_stride, c_rows, c_dense;
    int64_t c_base;    // candidate ids are global: row = id - c_base (row-sharded tables)
    int skip_foreign;  // sharded scoring: a candidate outside [c_base, c_base + c_rows) scores 0, no work
    // compact output of the row-sharded score exchange (kge_shard_score): only this rank's owned scores are
    // written, row b's at out[cmp_off(b) + k], k = the candidate's rank among the row's owned ones in column
    // order (the positive last). cmp_off(b) = cmp_pre[b] + the owned counts of the launch's earlier homes:
    // the send block of an all-to-all, home-major.
    const int* cmp_pre;   // [B] home-local exclusive prefix of this rank's owned counts
    const int* cmp_cnt;   // [B] this rank's owned candidates of each row (negatives + the positive)
    const int* cmp_tot;   // [W * W] tot[h * W + o]: candidates of home h's rows owned by rank o
    int64_t cmp_home0;    // home of the launch's row 0 (its rows are whole homes of home_B rows)
    const int2* bk_ent;   // [B, bk_ld] kge_shard_plan's bucket: (local row, rank k) per owned candidate
    const int* bk_start;  // [B, 9] the bucket's XCD-slice starts per row
    int64_t bk_ld;
    int xcd_phases;       // step_fwd_xcd_kernel: the table's 8 slices cut again into this many phases (1: none)
    int tile_rows;        // step_fwd_tile_kernel: batch rows per block (their queries staged in LDS)
    int tile_lds;         // step_fwd_tile_kernel: dynamic LDS bytes of one block
    int tile_pos;         // step_fwd_tile_kernel: also score the rows' positives (kge_step_forward)
    int tile_q2slots;     // step_fwd_tile_kernel (InterHT): LDS slots of relation thirds
    int tile_sort;        // step_fwd_tile_kernel: 0, or the power of two >= B of the (relation, row) sort
    int tile_waves;       // step_fwd_tile_kernel: waves per block (8, 12 or 16)
    int tile_depth;       // step_fwd_tile_kernel: candidate rows in flight per wave (1 or 2; 0 = 2)
    int* tile_board;      // step_fwd_tile_kernel: the sweep's progress board (kSweepBoardInts ints), or null
    int tile_tag;         // ... this step's tag of its entries (entries of another tag are ignored)
    int tile_lead;        // ... buckets a wave may lead the slice's slowest published block before it naps
    long long* tile_clk;  // step_fwd_tile_kernel: per-block clock marks (a -DKGE_PROFILING_KNOBS build), or null
    int tile_dry;         // step_fwd_tile_kernel: setup only, no scoring (A/B knob KGE_TILE_DRY)
    int tile_rev;         // step_fwd_tile_kernel: sweep each block's sorted list in descending entity order
    const int* tile_plan; // step_fwd_tile_kernel: this batch's plan (kge_step_forward_planned), or null
    int* tile_occ;        // host only: launch_tile_as launches nothing and answers here how many blocks of the
                          // instance, at tile_lds bytes of LDS, one CU holds (0: the runtime could not tell)
    int tile_blocks;      // step_fwd_tile_kernel: scoring blocks; blocks past them make the next batch's plan
    PlanArgs tile_next;   // ... that plan (tile_next.plan null: none)
    int tile_plan_blocks; // ... how many: one per group of the plan, or (kTileSharedWaves waves) fewer, plan block j
                          // making the plan's groups j, j + tile_plan_blocks, ...
    // kge_eval_rank_sweep (rank_pairs_kernel, rank_sweep_kernel; tile_rows / tile_lds: the sweep's rows per block
    // and dynamic LDS bytes)
    struct {
        const int64_t* truth;  // [B]
        const int64_t* fptr;   // [B + 1] filter CSR, or null
        const int64_t* fids;   // [nf]
        int64_t nf;
        float* ts;             // [B] the truths' scores
        int* cnt;              // [B] entities scoring above the truth
        float* fs;             // [nf] the filter entries' scores
        int chunks;            // contiguous chunks an entity slice is cut into (one block per chunk and row group)
    } rk;
    // kge_eval_topk_sweep (topk_sweep_kernel; tile_rows / tile_lds as for the rank sweep)
    struct {
        const int64_t* xptr;  // [B + 1] exclusion CSR, or null
        const int64_t* xids;
        int k;
        int chunks;           // contiguous chunks an entity slice is cut into
        int2* parts;          // [B][8 chunks][k] (score bits, id): the sorted list of each (row, chunk, slice)
    } tk;
    float* out;
    int64_t out_ld;
    int64_t B, N;
    int D;    // per-half width
    int cpw;  // candidates per wave
    int wpr;  // waves per batch row = ceil(N / cpw)
    float gamma;
    float phase_div;  // emb_range / pi (RotatE) or emb_range / pi' (pRotatE), fp32 as torch does
    float modulus;    // pRotatE
    // backward only
    const float* d_scores;
    int64_t d_ld;
    float* d_qent;  // gradient table for query entity rows (== d_cent for indexed scoring)
    float* d_rel;
    float* d_cent;
    float* d_modulus;
    // finish kernel only (one wave per batch row: positive score + negative-row reduction)
    const float* neg_scores;
    int64_t ns_ld, n_neg;
    float temperature;
    int adversarial;
    int detach;                // self-adversarial weights detached (upstream) or not (TF, Q3)
    const float* dq_scale;     // [B] chain kernel: scale of the fused forward's query gradient
    // kge_train_step epilogue
    const float* weight;       // [B] subsampling weights
    const float* pos_raw;      // [B] raw positive scores
    float* loss;               // [1]
    float* loss_sum;           // [1] running Sum metric (may be null)
    int* ev_count;             // fused forward: per-entity event counts (atomics)
    int* ev_cursor;            // epilogue: bucket cursors (scatter)
    int* ev_code_w;            // epilogue: event codes grouped by entity
    const int* ev_tile_sum;    // epilogue: per-4096-entity tile totals of the counts (tile-local cursors), or null
    int* ev_off_fix;           // epilogue: the tile-local offsets it rewrites to global ones (phase 2 reads them)
    int ev_ntiles;
    float* out_neg;      // [B] reduced negative branch
    float* out_pos_raw;  // [B] raw positive score (may be null)
    float* out_pos_ls;   // [B] logsigmoid(positive score)
    // deterministic two-phase backward (kge_step_backward). A "slot" is one query side: slots
    // [0, Bn) are the negative call's batch rows, [Bn, 2 Bn) the positive (single) call's.
    float* qbuf;          // [slots, 3 D] query operands q0 | q1 | q2 (phase 1 writes, phase 2 reads)
    float* qg_ent;        // [slots, ent_w] gradient of each slot's raw query-entity row
    float* qg_rel;        // [slots, rel_w] gradient of each slot's used relation part
    float* dmod_part;     // [slots] pRotatE modulus gradient partials
    int64_t slot0;        // first slot of a phase-1 launch
    float2* cand_stats;   // [B * N] per-candidate (1/||a||, 1/||b||) of InterHT, written by the forward
    const int64_t* pos_base;  // [B, 3] positive triples (fused step forward)
    float* dqbuf;         // [B, 3 * D] phase-1 query-part gradients (streaming form)
    int64_t ent_w, rel_w; // floats per entity row / per used relation part
    const int* ev_off;    // [E + 1] bucket offsets of the per-entity gradient events (phase 2)
    const int* ev_code;   // event codes, grouped by entity (order inside a bucket: arbitrary)
    const float* d_ns;    // [Bn, N] dL/d(negative score), contiguous
    const float* d_ps;    // [Bn] dL/d(positive score)
    int64_t Bn, Nn;       // negative batch rows and candidates per row
    float* d_out_ent;     // [E, c_ld] entity gradient table, fully overwritten by phase 2
    // row-sharded train step (kge_shard_train_*; kge_shard.h). Batch rows are GLOBAL: [0, B) over all
    // W home ranks, home h owning rows [h * home_B, (h + 1) * home_B).
    const float* qent_pos;      // [B, q_ld] the positive call's query rows (h), assembled by the caller
    float* sh_stats;            // [B, 4] this shard's partial (M, Z, Ln, positive score)
    const float* sh_stats_all;  // [world, B, 4] every shard's partial stats (all-gathered)
    float* sh_dq;               // [2 B, nq D] this shard's share of each slot's query gradient (SUM-reduced)
    float* sh_A;                // [B, nq D] online-softmax query-gradient sums of the owned candidates
    float* sh_B;                // [B, nq D] (TF semantics only: the softmax term)
    float* sh_merged;           // [B, 4] merged (M, Z, R, positive score): identical on every shard
    int64_t home_B;
    int world, rank, nq;
    // fused optimizer in phase 2 (kge_step_backward_adam): row e of the table is updated in place
    struct {
        float* m;   // [E, c_ld] first moment
        float* v;   // [E, c_ld] second moment
        float b1, b2, eps, alpha, step_size, bc2_sqrt;
        int keras, on;
    } adam;
    float* loss_parts;  // [2] epilogue: positive_sample_loss, negative_sample_loss (kge_train_step_reg; may be null)
    // L3 ("N3") regulariser in phase 2 (kge_train_step_reg). reg3 == 0: off, the plain instances run.
    float reg3;       // 3 lambda: every element x of row e gets reg3 x |x| added to its gradient before Adam
    float* reg_part;  // sum |x|^3 of what each wave holds: [E] (bwd_ent_kernel), [E, 4] (bwd_ent_stream_kernel)
    // lazy Adam in phase 2 (kge_train_step_lazy). lz_list null: off, every row is visited (the plain instances run).
    const int* lz_list;   // [lz_rows] the rows with events, ascending (lazy_list_kernel)
    const int* lz_count;  // [1] how many of them the list holds
    int64_t lz_rows;      // the list's size, min(E, events): block (or wave) i of the LAZY instances takes lz_list[i]
    // kge_eval_rank_candidates (rank_cand_kernel; the lists are c_idx / c_stride / N, the truths and the filter CSR
    // rk.truth / rk.fptr / rk.fids, the truths' scores rk.ts, which may be null here)
    struct {
        int64_t* ranks;  // [B] 1 + counted entries above the truth
        int64_t* ties;   // [B] counted entries equal to the truth, or null
    } rc;
};
// the wave count whose planned instances exist with the plan-sharing loop (SHARED: the row rule's shapes run 12 waves)
constexpr int kTileSharedWaves = 12;
inline bool tile_plan_shared(const ScoreParams& p) {
    return p.tile_next.plan && p.tile_plan_blocks < plan_groups(p.tile_next.B, p.tile_next.R);
}

// Adam coefficients of step t (1-based), computed on the host in double
struct AdamArgs {
    float b1, b2, eps, alpha, step_size, bc2_sqrt;
    int keras, zero_grad;
};

// per-score-function launchers (one translation unit each, see kge_fn_*.hip)
int launch_transe(const ScoreParams& p, int kind, hipStream_t st, int blocks, bool ch, int V, int G);
int launch_distmult(const ScoreParams& p, int kind, hipStream_t st, int blocks, bool ch, int V, int G);
int launch_complex(const ScoreParams& p, int kind, hipStream_t st, int blocks, bool ch, int V, int G);
int launch_rotate(const ScoreParams& p, int kind, hipStream_t st, int blocks, bool ch, int V, int G);
int launch_interht(const ScoreParams& p, int kind, hipStream_t st, int blocks, bool ch, int V, int G);
int launch_protate(const ScoreParams& p, int kind, hipStream_t st, int blocks, bool ch, int V, int G);
int launch_pairre(const ScoreParams& p, int kind, hipStream_t st, int blocks, bool ch, int V, int G);

// link-prediction evaluation (kge_eval.hip)
int launch_eval_query_any(int fn, bool ch, const ScoreParams& p, hipStream_t st, int blocks, int V, int G, float* Q,
                          int64_t ldq, void* P = nullptr, int64_t prows = 0);
int launch_gemm_nt(const float* A, const float* B, float* C, int M, int N, int K, int64_t lda, int64_t ldb,
                   int64_t ldc, hipStream_t st);
int launch_gemm_nt_f32x3(const float* A, const float* B, float* C, int M, int N, int K, int64_t lda, int64_t ldb,
                         int64_t ldc, hipStream_t st, int form = 0);
int launch_split3_planes(const float* X, int64_t rows, int64_t cols, int64_t ld, void* planes, int64_t plane_rows,
                         hipStream_t st);
// form 1: both operands staged through LDS per 16-k chunk (gemm_nt_x3p_kernel, 256 x 256 tiles); 2: B straight into
// registers, A staged per 32 k (gemm_nt_x3d_kernel); 3: gemm_nt_x3p_kernel with 256 x 192 tiles; 4: LDS-DMA staging
// in three stages (gemm_nt_x3l_kernel). Bitwise the same C.
int launch_gemm_nt_x3p(const void* Ap, int64_t a_rows, const void* Bp, int64_t b_rows, int64_t K, float* C, int64_t ldc,
                       int M, int N, hipStream_t st, int form);
// kge_eval_rank_planes: workspace bytes (truth scores and counts [M], filter-entry scores [F]) and the launches of
// the phases in `phases` (1 pair scores + count reset, 2 counting GEMM, 4 finish), in that order
int64_t eval_rank_ws_bytes(int64_t M, int64_t F);
int launch_eval_rank_planes(const void* Ap, int64_t a_rows, const void* Bp, int64_t b_rows, int64_t K, int M, int N,
                            const int64_t* truth, const int64_t* fptr, const int64_t* fids, int64_t F, int64_t* ranks,
                            void* ws, hipStream_t st, int form, int phases);
// rank_finish_kernel alone on a workspace of eval_rank_ws_bytes' layout (kge_eval_rank_sweep)
int launch_rank_finish(int64_t M, int64_t N, const int64_t* truth, const int64_t* fptr, const int64_t* fids, void* ws,
                       int64_t* ranks, hipStream_t st);
// kge_eval_topk_planes: the lists per query row (one per 256-column tile of the form-4 plane GEMM, whose selecting
// epilogue stores them at ws[row][tile][k]) and the two launches (the GEMM, topk_merge_kernel)
int64_t eval_topk_planes_parts(int64_t N);
int launch_eval_topk_planes(const void* Ap, int64_t a_rows, const void* Bp, int64_t b_rows, int64_t K, int M, int N,
                            const int64_t* xptr, const int64_t* xids, int k, int64_t* out_ids, int64_t ids_ld,
                            float* out_scores, int64_t scores_ld, void* ws, hipStream_t st);
// kge_eval_topk_sweep's merge of `parts` lists per row (topk_sweep_kernel's workspace), and kge_topk_rows
int launch_topk_merge(const void* parts, int64_t B, int64_t nparts, int k, int64_t* out_ids, int64_t ids_ld,
                      float* out_scores, int64_t scores_ld, hipStream_t st);
int launch_topk_rows(const float* S, int64_t M, int64_t N, int64_t ld, const int64_t* xptr, const int64_t* xids, int k,
                     int64_t* out_ids, int64_t ids_ld, float* out_scores, int64_t scores_ld, hipStream_t st);
int launch_rank(const float* S, int64_t M, int64_t N, int64_t ld, const int64_t* truth, const int64_t* fptr,
                const int64_t* fids, int64_t* ranks, hipStream_t st);

}  // namespace kge_impl
