"""Filtered link-prediction evaluation against all entities: the upstream `KGEModel.test_step`
(KnowledgeGraphEmbedding/codes/model.py, absent from the snapshot; its TestDataset builds, per test
triple and mode, a candidate list over every entity in which the other true triples are replaced by
the positive with bias -1; ranks come from argsort). BASELINE config C5.

The scores of a query batch against all E entities are computed on the GPU:
  * DistMult / ComplEx: S = Q . E^T at fp32 accuracy on the bf16 matrix cores (kge_eval_query +
    kge_gemm_nt_bf16x3: bf16x3 split in registers, six products, fp32 accumulation);
  * every other score function, and a DistMult / ComplEx table without planes whose rows take no float4 loads:
    the fused VALU scorer with candidate ids 0..E-1 (row stride 0).
Ranks are exact integers from kge_rank_filtered: rank = 1 + #(unfiltered e != truth with
s_e > s_truth). Ties count in the positive's favour; upstream's unstable argsort leaves them
arbitrary, which no test here exercises (continuous random scores). test_step ranks DistMult / ComplEx batches
without materialising S (kge_eval_rank_planes: the same ranks), and TransE / RotatE / pRotatE / InterHT batches
through rank_sweep (kge_eval_rank_sweep: each entity row loaded once per group of query rows, prepared once and
compared with every query's truth score on the spot: the same ranks); score_all + rank_filtered remains the
path of TranSparse and of widths the sweep has no kernel for.

predict answers a query instead of ranking a known truth: the k best entities for (h, r, ?) / (?, r, t) with their
scores, known answers left out (exact filtered top-k: topk_sweep / kge_eval_topk_sweep for the distance functions,
score_all + topk_rows / kge_topk_rows otherwise; topk_planes / kge_eval_topk_planes for DistMult / ComplEx without the
score matrix).

The filter lists themselves (the other true answers of each query) are made on the GPU: FilterTable holds the true
triples as a keyed table (kge_filter_table_build, two sorts on the host, uploaded once) and FilterTable.csr looks
any queries up in it (kge_eval_filter_count / kge_eval_filter_fill: build_filter's and build_exclude's CSR exactly);
test_step and predict make the CSR of a whole pass with one call per mode and hand the batches views of it.
build_filter / build_exclude remain as the host path (filter_on="host") and the yardstick.
"""
from __future__ import annotations

from collections import defaultdict

import numpy as np
import torch

from . import ops
from . import _lib
from ._lib import FN_IDS, HEAD_BATCH, TAIL_BATCH, check

MFMA_FNS = ("DistMult", "ComplEx")


def build_filter(queries: np.ndarray, mode: str, all_true_triples) -> tuple[np.ndarray, np.ndarray]:
    """CSR (ptr [M+1], ids) of the entities upstream's filter pushes below the positive:
    head-batch (h, r, t): every h' != h with (h', r, t) true; tail-batch: every t' != t with
    (h, r, t') true. Ids are distinct and sorted within a row."""
    by_rt, by_hr = defaultdict(set), defaultdict(set)
    for h, r, t in all_true_triples:
        by_rt[(int(r), int(t))].add(int(h))
        by_hr[(int(h), int(r))].add(int(t))
    ptr = np.zeros(len(queries) + 1, dtype=np.int64)
    rows = []
    for i, (h, r, t) in enumerate(np.asarray(queries, dtype=np.int64)):
        if mode == "head-batch":
            s = by_rt.get((int(r), int(t)), set()) - {int(h)}
        else:
            s = by_hr.get((int(h), int(r)), set()) - {int(t)}
        ids = np.array(sorted(s), dtype=np.int64)
        rows.append(ids)
        ptr[i + 1] = ptr[i] + len(ids)
    ids = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    return ptr, ids


def split_planes(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """x [rows, K] fp32 as three bf16 planes (kge_split_bf16x3: uint8 storage of [3][rows][K rounded to 16]),
    the operand form of kge_gemm_nt_bf16x3_planes."""
    lib = _lib.load()
    rows, K = x.shape
    nbytes = int(lib.kge_split_bf16x3_bytes(rows, K))
    if out is None or out.numel() < nbytes:
        out = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    check(lib.kge_split_bf16x3(x.data_ptr(), rows, K, x.stride(0), out.data_ptr(), rows,
                               torch.cuda.current_stream(x.device).cuda_stream), "kge_split_bf16x3")
    return out


PLANES_MAX_BYTES = (1 << 32) - 16  # the plane GEMM's 32-bit buffer offsets (kge_split_bf16x3 refuses past it)


def entity_planes(model) -> torch.Tensor | None:
    """The entity table's bf16 planes for one evaluation pass (DistMult / ComplEx), made once and passed to
    every score_all call of the pass: the table does not change while it is evaluated. None for the other
    score functions, and None where the planes do not fit (PLANES_MAX_BYTES, or no device memory for their
    1.5x the table): score_all then splits the operands at staging (kge_gemm_nt_bf16x3), at the same accuracy, or,
    where the table's rows take no float4 loads, scores through the fused scorer."""
    if model.model_name not in MFMA_FNS:
        return None
    ent = model.entity_embedding.detach()
    if int(_lib.load().kge_split_bf16x3_bytes(ent.shape[0], ent.shape[1])) >= PLANES_MAX_BYTES:
        return None
    try:
        return split_planes(ent)
    except torch.OutOfMemoryError:
        return None


_Q_PLANES = {}


def _float4_rows(*tables) -> bool:
    """Whether every row of every table starts on a 16-B boundary: the base 16-B aligned and the row stride a
    multiple of 4 floats (what kge_eval_query_planes and kge_gemm_nt_bf16x3 need of their operands)."""
    return all(t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0 for t in tables)


def score_all(model, positive_sample: torch.Tensor, mode: str, out: torch.Tensor | None = None,
              planes: torch.Tensor | None = None) -> torch.Tensor:
    """[B, E] scores of every entity as the candidate (head-batch or tail-batch). DistMult / ComplEx: pass
    `planes` = entity_planes(model), made once per evaluation pass (without it the call splits the table
    itself: kge_gemm_nt_bf16x3, the operands split at staging; or, where K, the table's row stride or its base
    is off 16 B, scores every entity through the fused scorer, as for the distance models: any table
    kge_score_indexed accepts)."""
    m = ops.mode_id(mode)
    ent, rel = model.entity_embedding.detach(), model.relation_embedding.detach()
    B, E = positive_sample.shape[0], ent.shape[0]
    dev = ent.device
    if out is None:
        out = torch.empty((B, E), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    if model.model_name == "TranSparse":
        # head-batch: every entity as the head (stride-0 candidate rows); tail-batch scores do not
        # depend on the tail (Q9), so the [B, 1] score is broadcast to every candidate
        if m == HEAD_BATCH:
            cand = torch.arange(E, device=dev, dtype=torch.int64).unsqueeze(0).expand(B, E)
            return ops.transparse_score_raw(m, ent, rel, model.W.detach(), model.mask, positive_sample, cand,
                                            model._gamma_f, out=out)
        s = ops.transparse_score_raw(m, ent, rel, model.W.detach(), model.mask, positive_sample, None,
                                     model._gamma_f)
        out.copy_(s.expand(B, E))
        return out
    if model.model_name in MFMA_FNS:
        K = ent.shape[1]
        lib = _lib.load()
        fq = FN_IDS[model.model_name]
        # S = Q . E^T at fp32 accuracy on the bf16 matrix cores (bf16x3 terms, six products): from the pass's
        # entity planes and the batch's query planes (kge_eval_query_planes: the query rows written as planes, one
        # launch), or with the operands split at staging
        if planes is not None and model._D % 4 == 0 and _float4_rows(ent, rel):
            key = (str(dev), st)
            nbytes = int(lib.kge_split_bf16x3_bytes(B, K))
            qp = _Q_PLANES.get(key)
            if qp is None or qp.numel() < nbytes:
                qp = _Q_PLANES[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            check(lib.kge_eval_query_planes(fq, m, ent.data_ptr(), E, ent.stride(0), rel.data_ptr(), rel.shape[0],
                                            rel.stride(0), positive_sample.data_ptr(), B, model._D, qp.data_ptr(), B,
                                            st), "kge_eval_query_planes")
            check(lib.kge_gemm_nt_bf16x3_planes(qp.data_ptr(), B, planes.data_ptr(), E, K, out.data_ptr(),
                                                out.stride(0), B, E, st), "kge_gemm_nt_bf16x3_planes")
            return out
        # the staging-split GEMM reads float4 quads of Q and of the table: K and the table's row stride multiples
        # of 4, 16-B bases (Q is dense and freshly allocated). A table without planes that does not meet that
        # (hidden_dim 50, a padded or offset view) takes the fused scorer below, which allocates nothing the size
        # of the table (planes are usually missing because memory is short)
        if planes is not None or (K % 4 == 0 and _float4_rows(ent)):
            Q = torch.empty((B, K), dtype=torch.float32, device=dev)
            check(lib.kge_eval_query(fq, m, ent.data_ptr(), E, ent.stride(0), rel.data_ptr(),
                                     rel.shape[0], rel.stride(0), positive_sample.data_ptr(), B, model._D,
                                     Q.data_ptr(), Q.stride(0), st), "kge_eval_query")
            if planes is not None:
                key = (str(dev), st)
                qp = _Q_PLANES[key] = split_planes(Q, _Q_PLANES.get(key))
                check(lib.kge_gemm_nt_bf16x3_planes(qp.data_ptr(), B, planes.data_ptr(), E, K, out.data_ptr(),
                                                    out.stride(0), B, E, st), "kge_gemm_nt_bf16x3_planes")
            else:
                check(lib.kge_gemm_nt_bf16x3(Q.data_ptr(), Q.stride(0), ent.data_ptr(), ent.stride(0),
                                             out.data_ptr(), out.stride(0), B, E, K, st), "kge_gemm_nt_bf16x3")
            return out
    cand = torch.arange(E, device=dev, dtype=torch.int64).unsqueeze(0).expand(B, E)  # row stride 0
    modulus = float(model.modulus.detach().reshape(-1)[0]) if model.model_name == "pRotatE" else 0.0
    return ops.score_indexed_raw(FN_IDS[model.model_name], m, ent, rel, model._rel_off, positive_sample, cand,
                                 model._D, model._gamma_f, model._range_f, modulus, out=out)


_RANK_WS = {}


def _planes_rank_ok(model, planes) -> bool:
    """Whether the ranks-from-planes path applies: DistMult / ComplEx with entity planes, float4 rows (D, both
    tables' row strides and bases: kge_eval_query_planes' precondition)."""
    if model.model_name not in MFMA_FNS or planes is None:
        return False
    return model._D % 4 == 0 and _float4_rows(model.entity_embedding, model.relation_embedding)


def rank_planes(model, positive_sample: torch.Tensor, mode: str, planes: torch.Tensor, truth: torch.Tensor,
                filter_ptr: torch.Tensor | None = None, filter_ids: torch.Tensor | None = None,
                nfilter: int | None = None) -> torch.Tensor | None:
    """Filtered ranks of a query batch straight from the entity planes, without the [B, E] score matrix
    (kge_eval_rank_planes: the truth's and the filter entries' scores with the GEMM's own arithmetic, the plane GEMM
    counting per row the entities above the truth, the filter correction): rank_filtered(score_all(...))'s ranks
    exactly. DistMult / ComplEx with planes; None where the query-plane form does not apply (then score_all +
    rank_filtered). filter_ptr must start at 0; nfilter = filter_ptr[-1] (read from the device when not given)."""
    if not _planes_rank_ok(model, planes):
        return None
    ent, rel = model.entity_embedding.detach(), model.relation_embedding.detach()
    lib = _lib.load()
    m = ops.mode_id(mode)
    B, E, K = positive_sample.shape[0], ent.shape[0], ent.shape[1]
    dev = ent.device
    st = torch.cuda.current_stream(dev).cuda_stream
    key = (str(dev), st)
    nbytes = int(lib.kge_split_bf16x3_bytes(B, K))
    qp = _Q_PLANES.get(key)
    if qp is None or qp.numel() < nbytes:
        qp = _Q_PLANES[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(lib.kge_eval_query_planes(FN_IDS[model.model_name], m, ent.data_ptr(), E, ent.stride(0), rel.data_ptr(),
                                    rel.shape[0], rel.stride(0), positive_sample.data_ptr(), B, model._D, qp.data_ptr(),
                                    B, st), "kge_eval_query_planes")
    nf = (int(filter_ptr[-1]) if nfilter is None else int(nfilter)) if filter_ptr is not None else 0
    wsb = int(lib.kge_eval_rank_planes_workspace_size(B, nf))
    ws = _RANK_WS.get(key)
    if ws is None or ws.numel() < wsb:
        ws = _RANK_WS[key] = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    ranks = torch.empty(B, dtype=torch.int64, device=dev)
    check(lib.kge_eval_rank_planes(qp.data_ptr(), B, planes.data_ptr(), E, K, B, E, truth.data_ptr(),
                                   None if filter_ptr is None else filter_ptr.data_ptr(),
                                   None if filter_ids is None else filter_ids.data_ptr(), nf, ranks.data_ptr(),
                                   ws.data_ptr(), ws.numel(), st), "kge_eval_rank_planes")
    return ranks


SWEEP_FNS = ("TransE", "RotatE", "pRotatE", "InterHT", "PairRE")
_SWEEP_WS = {}
_ENOTSUP = -95  # KGE_ENOTSUP (include/kge_hip.h)


def _sweep_rank_ok(model) -> bool:
    """Whether test_step ranks this model through rank_sweep: the distance functions with their tables on a GPU
    (each measured faster than the score-matrix path by DESIGN §3.0's rule, §3.4). rank_sweep itself may still
    answer None (a width it has no kernel for): test_step then falls back to score_all + rank_filtered for that
    batch."""
    return model.model_name in SWEEP_FNS and model.entity_embedding.device.type == "cuda"


def rank_sweep(model, positive_sample: torch.Tensor, mode: str, truth: torch.Tensor,
               filter_ptr: torch.Tensor | None = None, filter_ids: torch.Tensor | None = None,
               nfilter: int | None = None) -> torch.Tensor | None:
    """Filtered ranks of a query batch against every entity for TransE / RotatE / pRotatE / InterHT, without the
    [B, E] score matrix (kge_eval_rank_sweep: the truth's and the filter entries' scores, a sweep that loads each
    entity row once per group of query rows and counts the scores above the truth's, the filter correction):
    rank_filtered(score_all(...))'s ranks exactly. None where the library has no sweep for the model (DistMult /
    ComplEx / TranSparse, a per-half width past 1 024): callers fall back. filter_ptr must start at 0; nfilter =
    filter_ptr[-1] (read from the device when not given). The index tensors must be int64, contiguous and on the
    tables' device (ValueError otherwise)."""
    if model.model_name not in FN_IDS:
        return None
    ent, rel = model.entity_embedding.detach(), model.relation_embedding.detach()
    dev = ent.device
    if positive_sample.dim() != 2 or positive_sample.shape[1] != 3:
        raise ValueError("rank_sweep: positive_sample must be [B, 3]")
    B, E = positive_sample.shape[0], ent.shape[0]
    if filter_ptr is None:
        filter_ids = None
    for name, t, n in (("positive_sample", positive_sample, 3 * B), ("truth", truth, B),
                       ("filter_ptr", filter_ptr, B + 1), ("filter_ids", filter_ids, None)):
        if t is None:
            continue
        if t.dtype != torch.int64 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"rank_sweep: {name} must be a contiguous int64 tensor on {dev}")
        if n is not None and t.numel() != n:
            raise ValueError(f"rank_sweep: {name} has {t.numel()} elements, expected {n}")
    ops._need_gpu(ent, rel)
    lib = _lib.load()
    nf = (int(filter_ptr[-1]) if nfilter is None else int(nfilter)) if filter_ptr is not None else 0
    if nf > 0 and (filter_ids is None or filter_ids.numel() < nf):
        raise ValueError("rank_sweep: filter_ids shorter than nfilter")
    st = torch.cuda.current_stream(dev).cuda_stream
    key = (str(dev), st)
    wsb = int(lib.kge_eval_rank_sweep_workspace_size(B, nf))
    ws = _SWEEP_WS.get(key)
    if ws is None or ws.numel() < wsb:
        ws = _SWEEP_WS[key] = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    ranks = torch.empty(B, dtype=torch.int64, device=dev)
    modulus = float(model.modulus.detach().reshape(-1)[0]) if model.model_name == "pRotatE" else 0.0
    rc = lib.kge_eval_rank_sweep(FN_IDS[model.model_name], ops.mode_id(mode), ent.data_ptr(), E, ent.stride(0),
                                 rel.data_ptr(), rel.shape[0], rel.stride(0), model._rel_off,
                                 positive_sample.data_ptr(), B, model._D, model._gamma_f, model._range_f, modulus,
                                 truth.data_ptr(), None if filter_ptr is None else filter_ptr.data_ptr(),
                                 None if filter_ids is None or nf == 0 else filter_ids.data_ptr(), nf,
                                 ranks.data_ptr(), ws.data_ptr(), ws.numel(), st)
    if rc == _ENOTSUP:
        return None
    check(rc, "kge_eval_rank_sweep")
    return ranks


def rank_candidates(model, positive_sample: torch.Tensor, mode: str, candidates: torch.Tensor,
                    truth: torch.Tensor | None = None, filter_ptr: torch.Tensor | None = None,
                    filter_ids: torch.Tensor | None = None, nfilter: int | None = None, want_ties: bool = False):
    """Ranks of a query batch against a given candidate list per query (kge_eval_rank_candidates: one launch, no
    score matrix, no workspace): the protocol of the large-graph benchmarks (ogbl-wikikg2's 500 negatives per test
    triple and mode) and of validation against sampled candidates. `candidates` is [M, C] (row-contiguous, any row
    stride >= C) or [C] (one list shared by all queries), int64 on the tables' device; an id outside [0, nentity)
    is padding (pad ragged lists with -1). An entry is counted unless it is padding, equals the row's truth or is
    among the row's filter ids (CSR as rank_sweep's: filter_ptr starts at 0, ids ascending within a row, nfilter =
    filter_ptr[-1], read from the device when not given); rank = 1 + #{counted entries scoring above the truth}
    (ties in the positive's favour), ties = #{counted entries scoring exactly the truth's score}. `truth` [M]
    defaults to the positive's head (head-batch) or tail column. Returns ranks [M] int64, or (ranks, ties) with
    want_ties. None for a model without a function id (TranSparse), as rank_sweep. The index tensors must be
    int64, contiguous and on the tables' device (ValueError otherwise). There is no CPU fallback."""
    if model.model_name not in FN_IDS:
        return None
    m = ops.mode_id(mode)
    if m not in (HEAD_BATCH, TAIL_BATCH):
        raise ValueError("rank_candidates: mode must be 'head-batch' or 'tail-batch'")
    ent, rel = model.entity_embedding.detach(), model.relation_embedding.detach()
    dev = ent.device
    if positive_sample.dim() != 2 or positive_sample.shape[1] != 3:
        raise ValueError("rank_candidates: positive_sample must be [M, 3]")
    M, E = positive_sample.shape[0], ent.shape[0]
    if not torch.is_tensor(candidates) or candidates.dim() not in (1, 2):
        raise ValueError("rank_candidates: candidates must be a [M, C] or [C] tensor")
    if candidates.dtype != torch.int64 or candidates.device != dev:
        raise ValueError(f"rank_candidates: candidates must be a contiguous int64 tensor on {dev}")
    if candidates.dim() == 1:
        if not candidates.is_contiguous():
            raise ValueError(f"rank_candidates: candidates must be a contiguous int64 tensor on {dev}")
        C, cand_ld = candidates.shape[0], 0
    else:
        C = candidates.shape[1]
        if candidates.shape[0] != M:
            raise ValueError(f"rank_candidates: candidates has {candidates.shape[0]} rows, expected {M}")
        shared = M > 1 and candidates.stride(0) == 0  # an expanded [C] list
        if (C > 1 and candidates.stride(1) != 1) or (M > 1 and not shared and candidates.stride(0) < C):
            raise ValueError(f"rank_candidates: candidates must be a contiguous int64 tensor on {dev} "
                             "(rows contiguous, row stride >= C)")
        cand_ld = 0 if shared else (max(candidates.stride(0), C) if M > 1 else C)
    if truth is None and positive_sample.dtype == torch.int64:
        truth = positive_sample[:, 0 if m == HEAD_BATCH else 2].contiguous()
    if filter_ptr is None:
        filter_ids = None
    for name, t, n in (("positive_sample", positive_sample, 3 * M), ("truth", truth, M),
                       ("filter_ptr", filter_ptr, M + 1), ("filter_ids", filter_ids, None)):
        if t is None:
            continue
        if t.dtype != torch.int64 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"rank_candidates: {name} must be a contiguous int64 tensor on {dev}")
        if n is not None and t.numel() != n:
            raise ValueError(f"rank_candidates: {name} has {t.numel()} elements, expected {n}")
    ops._need_gpu(ent, rel)
    lib = _lib.load()
    nf = (int(filter_ptr[-1]) if nfilter is None else int(nfilter)) if filter_ptr is not None else 0
    if nf > 0 and (filter_ids is None or filter_ids.numel() < nf):
        raise ValueError("rank_candidates: filter_ids shorter than nfilter")
    ranks = torch.empty(M, dtype=torch.int64, device=dev)
    ties = torch.empty(M, dtype=torch.int64, device=dev) if want_ties else None
    modulus = float(model.modulus.detach().reshape(-1)[0]) if model.model_name == "pRotatE" else 0.0
    check(lib.kge_eval_rank_candidates(FN_IDS[model.model_name], m, ent.data_ptr(), E, ent.stride(0), rel.data_ptr(),
                                       rel.shape[0], rel.stride(0), model._rel_off, positive_sample.data_ptr(), M,
                                       model._D, model._gamma_f, model._range_f, modulus, truth.data_ptr(),
                                       candidates.data_ptr() if C else None, cand_ld, C,
                                       None if nf == 0 else filter_ptr.data_ptr(),
                                       None if nf == 0 else filter_ids.data_ptr(), nf, ranks.data_ptr(),
                                       None if ties is None else ties.data_ptr(), None,
                                       torch.cuda.current_stream(dev).cuda_stream), "kge_eval_rank_candidates")
    return (ranks, ties) if want_ties else ranks


_TIE_RULES = ("optimistic", "pessimistic", "mean")


def _transparse_candidates(model, pos, mode, cand, filtered, ties):
    """TranSparse has no function id: [truth | candidates] scored with model.score, ranked by rank_filtered with the
    truth in column 0. That composition knows no padding, no filter and no tie count, so it refuses them."""
    E = model.entity_embedding.shape[0]
    if filtered or ties != "optimistic" or bool(((cand < 0) | (cand >= E)).any()):
        raise NotImplementedError("test_step_candidates: TranSparse ranks candidate lists through model.score + "
                                  "rank_filtered, which takes only lists without padding (every id in [0, nentity)), "
                                  "no known_triples filter and ties='optimistic'")
    M = pos.shape[0]
    col = 0 if mode == "head-batch" else 2
    rows = cand.unsqueeze(0).expand(M, -1) if cand.dim() == 1 else cand
    both = torch.cat([pos[:, col:col + 1], rows], dim=1).contiguous()
    s = model.score(mode, pos, both).detach()
    if s.shape[1] != both.shape[1]:  # tail-batch scores do not depend on the tail (Q9): one column
        s = s.expand(M, both.shape[1])
    return rank_filtered(s.contiguous(), torch.zeros(M, dtype=torch.int64, device=pos.device))


def test_step_candidates(model, test_triples, head_candidates, tail_candidates, known_triples=None, batch_size=None,
                         ties: str = "optimistic"):
    """Evaluation against given candidate lists (the large-graph protocol: ogbl-wikikg2 ships 500 head and 500 tail
    negatives per test triple): MRR, MR and HITS@{1,3,10} over the head-batch ranks against `head_candidates` and
    the tail-batch ranks against `tail_candidates`, each [M, C] (one list per test triple, ragged lists padded with
    -1) or [C] (one list for all), or None to skip that mode. With `known_triples` (triples, or a FilterTable of
    them) the other true answers of a query are left out of its list (FilterTable.csr(..., drop_own=True), one call
    per mode for the whole pass; the batches take views). `ties`: "optimistic" rank = 1 + above (the project's rule;
    with a shared list of all entities test_step's ranks), "pessimistic" 1 + above + ties, "mean" 1 + above +
    ties / 2 (the OGB evaluator's rule). Batches of `batch_size` (1 024) queries run through rank_candidates; the
    ranks stay on the device and go to the host once. TranSparse: model.score + rank_filtered, only for lists
    without padding, without a filter and with ties="optimistic" (NotImplementedError otherwise)."""
    if ties not in _TIE_RULES:
        raise ValueError(f"test_step_candidates: ties must be one of {_TIE_RULES}")
    bs = int(batch_size or 1024)
    if bs < 1:
        raise ValueError("test_step_candidates: batch_size must be positive")
    ent = model.entity_embedding
    ops._need_gpu(ent, model.relation_embedding)
    dev = ent.device
    triples = np.ascontiguousarray(np.asarray(test_triples, dtype=np.int64).reshape(-1, 3))
    M = len(triples)
    lists = {}
    for mode, c in (("head-batch", head_candidates), ("tail-batch", tail_candidates)):
        if c is None:
            continue
        c = c.to(dev) if torch.is_tensor(c) else torch.from_numpy(np.array(c, dtype=np.int64)).to(dev)
        if c.dtype != torch.int64 or c.dim() not in (1, 2) or (c.dim() == 2 and c.shape[0] != M):
            raise ValueError(f"test_step_candidates: the {mode} candidates must be int64, [M, C] or [C]")
        lists[mode] = c.contiguous()
    above, tied = [], []
    with torch.no_grad():
        if M and lists:
            pos_all = torch.from_numpy(triples).to(dev)
            csr = {}
            if known_triples is not None:
                table = _device_table(known_triples, dev, "device")
                for mode in lists:
                    if table is not None:
                        ptr_dev, ids_dev, ptr_host = table.csr(pos_all, mode, drop_own=True)
                    else:  # triples the table build refuses (a negative id): build_filter's CSR, uploaded once
                        ptr_host, ids = build_filter(triples, mode, known_triples)
                        ptr_dev, ids_dev = torch.from_numpy(ptr_host).to(dev), torch.from_numpy(ids).to(dev)
                    csr[mode] = (_batch_ptrs(ptr_dev, M, bs), ids_dev, ptr_host)
            for mode, cand in lists.items():
                for s in range(0, M, bs):
                    n = min(bs, M - s)
                    pos = pos_all[s:s + n]
                    c = cand if cand.dim() == 1 else cand[s:s + n]
                    fptr = fids = None
                    nf = 0
                    if mode in csr:
                        bptr, ids_dev, ph = csr[mode]
                        nf = int(ph[s + n] - ph[s])
                        if nf:  # views of the pass's CSR (8-B aligned: the kernel loads the ids one by one)
                            fptr, fids = bptr[s // bs, :n + 1], ids_dev[int(ph[s]):int(ph[s + n])]
                    if model.model_name not in FN_IDS:
                        above.append(_transparse_candidates(model, pos, mode, c, known_triples is not None, ties))
                        continue
                    r, t = rank_candidates(model, pos, mode, c, None, fptr, fids, nf, want_ties=True)
                    above.append(r)
                    tied.append(t)
    if not above:
        return metrics_from_ranks(np.zeros(0, dtype=np.int64))
    if tied and ties != "optimistic":
        both = torch.stack([torch.cat(above), torch.cat(tied)]).cpu().numpy()  # the pass's one transfer
        ranks = both[0] + both[1] if ties == "pessimistic" else both[0] + both[1] / 2.0
    else:
        ranks = torch.cat(above).cpu().numpy()
    return metrics_from_ranks(ranks)


TOPK_MAX = 64  # KGE_TOPK_MAX (include/kge_hip.h)
_TOPK_WS = {}


def build_exclude(queries: np.ndarray, mode: str, triples) -> tuple[np.ndarray, np.ndarray]:
    """CSR (ptr [M+1], ids) of the answers `triples` already hold for each query: head-batch (?, r, t): every h'
    with (h', r, t) known; tail-batch (h, r, ?): every t' with (h, r, t') known. build_filter without the removal
    of the query's own answer (the candidate slot of a query triple is ignored). Ids are distinct and sorted
    within a row."""
    by_rt, by_hr = defaultdict(set), defaultdict(set)
    for h, r, t in triples:
        by_rt[(int(r), int(t))].add(int(h))
        by_hr[(int(h), int(r))].add(int(t))
    queries = np.asarray(queries, dtype=np.int64).reshape(-1, 3)
    ptr = np.zeros(len(queries) + 1, dtype=np.int64)
    rows = []
    for i, (h, r, t) in enumerate(queries):
        s = by_rt.get((int(r), int(t)), ()) if mode == "head-batch" else by_hr.get((int(h), int(r)), ())
        rows.append(np.array(sorted(s), dtype=np.int64))
        ptr[i + 1] = ptr[i] + len(rows[-1])
    ids = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    return ptr, ids


_MODE_IDS = {"head-batch": HEAD_BATCH, "tail-batch": TAIL_BATCH}
FILTER_SCAN_TILE = 4096  # kFtScanTile (csrc/kge_filter.h): the queries kge_eval_filter_count's scan takes per pass


class FilterTable:
    """The true answers of a set of triples as a table on the device (kge_filter_table_build: per mode the
    distinct (r, t) / (h, r) keys in ascending order with their sorted distinct heads / tails, found by two sorts;
    layout in csrc/kge_filter.h), from which `csr` makes build_filter's and build_exclude's CSR for any queries on
    the GPU. Built once and uploaded; pass it to test_step / predict in place of the triples to reuse it over
    validation passes. Ids are any int64 >= 0 (a negative id: KGEHipError)."""

    def __init__(self, triples, device=None):
        triples = np.ascontiguousarray(np.asarray(triples, dtype=np.int64).reshape(-1, 3))
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise _lib.KGEHipError(f"FilterTable needs a GPU device, got {self.device} (build_filter / "
                                   "build_exclude make the CSR on the host)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.ntriples = len(triples)
        self.table = torch.from_numpy(build_filter_table(triples)).to(self.device)

    def csr(self, queries, mode: str, drop_own: bool = True):
        """(ptr [M + 1], ids [ptr[M]]) on the device and ptr on the host (a numpy copy: the call's one host sync) for
        the query triples [M, 3] (a contiguous int64 tensor on the table's device, or anything np.asarray takes):
        build_filter(queries, mode, triples) with drop_own, build_exclude(queries, mode, triples) without, exactly.
        Runs on the current stream (kge_eval_filter_count, kge_eval_filter_fill)."""
        if mode not in _MODE_IDS:
            raise ValueError("FilterTable.csr: mode must be 'head-batch' or 'tail-batch'")
        dev = self.device
        if torch.is_tensor(queries):
            if queries.dim() != 2 or queries.shape[1] != 3:
                raise ValueError("FilterTable.csr: queries must be [M, 3]")
            if queries.dtype != torch.int64 or not queries.is_contiguous() or queries.device != dev:
                raise ValueError(f"FilterTable.csr: queries must be a contiguous int64 tensor on {dev}")
            pos = queries
        else:
            q = np.asarray(queries)
            if q.size and (q.ndim != 2 or q.shape[1] != 3):
                raise ValueError("FilterTable.csr: queries must be [M, 3]")
            pos = torch.from_numpy(np.array(q, dtype=np.int64).reshape(-1, 3)).to(dev)  # a copy: q may be read-only
        lib = _lib.load()
        M, m, own = pos.shape[0], _MODE_IDS[mode], 1 if drop_own else 0
        st = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            ws = torch.empty(int(lib.kge_eval_filter_workspace_size(M)), dtype=torch.uint8, device=dev)
            ptr = torch.empty(M + 1, dtype=torch.int64, device=dev)
            blob, nbytes = self.table.data_ptr(), self.table.numel() * 8
            check(lib.kge_eval_filter_count(blob, nbytes, m, pos.data_ptr(), M, own, ptr.data_ptr(), ws.data_ptr(),
                                            ws.numel(), st), "kge_eval_filter_count")
            ptr_host = ptr.cpu().numpy()
            total = int(ptr_host[M])
            ids = torch.empty(total, dtype=torch.int64, device=dev)
            check(lib.kge_eval_filter_fill(blob, nbytes, m, pos.data_ptr(), M, own, ptr.data_ptr(),
                                           ids.data_ptr() if total else None, total, ws.data_ptr(), ws.numel(), st),
                  "kge_eval_filter_fill")
        return ptr, ids, ptr_host


def build_filter_table(triples) -> np.ndarray:
    """The filter table of `triples` [T, 3] as a host int64 array (kge_filter_table_build: layout in
    csrc/kge_filter.h), cut to the words in use."""
    triples = np.ascontiguousarray(np.asarray(triples, dtype=np.int64).reshape(-1, 3))
    lib = _lib.load()
    nbytes = int(lib.kge_filter_table_size(len(triples)))
    blob = np.empty(nbytes // 8, dtype=np.int64)
    check(lib.kge_filter_table_build(triples.ctypes.data, len(triples), blob.ctypes.data, nbytes),
          "kge_filter_table_build")
    return blob[:int(blob[1])].copy()


def _device_table(triples, dev, filter_on):
    """The FilterTable test_step / predict look their filters up in, or None for the host path (filter_on="host",
    tables off the GPU, or triples the table build refuses: a negative id)."""
    if filter_on not in ("device", "host"):
        raise ValueError("filter_on must be 'device' or 'host'")
    if isinstance(triples, FilterTable):
        if filter_on == "host":
            raise ValueError("filter_on='host' needs the triples, not a FilterTable")
        if triples.device != dev:
            raise ValueError(f"the FilterTable is on {triples.device}, the model on {dev}")
        return triples
    if filter_on == "host" or dev.type != "cuda":
        return None
    try:
        return FilterTable(triples, dev)
    except _lib.KGEHipError:
        return None


def _batch_ptrs(ptr_dev: torch.Tensor, M: int, bs: int) -> torch.Tensor:
    """[batches, bs + 1]: row i holds ptr[i bs .. i bs + bs] - ptr[i bs] (the batch's CSR starts rebased to 0; past
    M the last start repeats), one gather for the whole pass."""
    dev = ptr_dev.device
    start = torch.arange(0, max(M, 1), bs, device=dev, dtype=torch.int64).unsqueeze(1)
    idx = (start + torch.arange(bs + 1, device=dev, dtype=torch.int64).unsqueeze(0)).clamp_(max=M)
    return (ptr_dev[idx] - ptr_dev[start]).contiguous()


def _check_k(k, what):
    if int(k) != k or not 1 <= int(k) <= TOPK_MAX:
        raise ValueError(f"{what}: k must be in 1 .. {TOPK_MAX}, got {k}")
    return int(k)


def _check_excl(what, dev, rows, excl_ptr, excl_ids, nexcl):
    """(excl_ptr, excl_ids, nexcl) checked as rank_sweep checks its filter: contiguous int64 tensors on `dev`."""
    if excl_ptr is None:
        return None, None, 0
    for name, t, n in (("excl_ptr", excl_ptr, rows + 1), ("excl_ids", excl_ids, None)):
        if t is None:
            continue
        if t.dtype != torch.int64 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{what}: {name} must be a contiguous int64 tensor on {dev}")
        if n is not None and t.numel() != n:
            raise ValueError(f"{what}: {name} has {t.numel()} elements, expected {n}")
    nx = int(excl_ptr[-1]) if nexcl is None else int(nexcl)
    if nx > 0 and (excl_ids is None or excl_ids.numel() < nx):
        raise ValueError(f"{what}: excl_ids shorter than nexcl")
    if nx == 0:
        return None, None, 0
    return excl_ptr, excl_ids, nx


def topk_sweep(model, positive_sample: torch.Tensor, mode: str, k: int, excl_ptr: torch.Tensor | None = None,
               excl_ids: torch.Tensor | None = None, nexcl: int | None = None):
    """(ids [B, k] int64, scores [B, k]) of the k best entities per query row for TransE / RotatE / pRotatE /
    InterHT, without the [B, E] score matrix (kge_eval_topk_sweep: rank_sweep's sweep, each wave keeping the best k
    per query row, then a merge): score descending, ties by ascending id, without the ids of the row's exclusion
    list (CSR, build_exclude's form; excl_ptr starts at 0, nexcl = excl_ptr[-1], read from the device when not
    given) and without NaN scores; rows with fewer than k valid entities are padded with id -1 and score -inf. The
    scores are bitwise score_all's. None where the library has no sweep for the model (DistMult / ComplEx /
    TranSparse, a per-half width past 1 024): callers fall back to score_all + topk_rows. The index tensors must be
    int64, contiguous and on the tables' device (ValueError otherwise)."""
    k = _check_k(k, "topk_sweep")
    if model.model_name not in FN_IDS:
        return None
    ent, rel = model.entity_embedding.detach(), model.relation_embedding.detach()
    dev = ent.device
    if positive_sample.dim() != 2 or positive_sample.shape[1] != 3:
        raise ValueError("topk_sweep: positive_sample must be [B, 3]")
    B, E = positive_sample.shape[0], ent.shape[0]
    if positive_sample.dtype != torch.int64 or not positive_sample.is_contiguous() or positive_sample.device != dev:
        raise ValueError(f"topk_sweep: positive_sample must be a contiguous int64 tensor on {dev}")
    excl_ptr, excl_ids, nx = _check_excl("topk_sweep", dev, B, excl_ptr, excl_ids, nexcl)
    ops._need_gpu(ent, rel)
    lib = _lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    key = (str(dev), st)
    wsb = int(lib.kge_eval_topk_sweep_workspace_size(B, k))
    ws = _TOPK_WS.get(key)
    if ws is None or ws.numel() < wsb:
        ws = _TOPK_WS[key] = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    ids = torch.empty((B, k), dtype=torch.int64, device=dev)
    scores = torch.empty((B, k), dtype=torch.float32, device=dev)
    modulus = float(model.modulus.detach().reshape(-1)[0]) if model.model_name == "pRotatE" else 0.0
    rc = lib.kge_eval_topk_sweep(FN_IDS[model.model_name], ops.mode_id(mode), ent.data_ptr(), E, ent.stride(0),
                                 rel.data_ptr(), rel.shape[0], rel.stride(0), model._rel_off,
                                 positive_sample.data_ptr(), B, model._D, model._gamma_f, model._range_f, modulus,
                                 None if excl_ptr is None else excl_ptr.data_ptr(),
                                 None if excl_ids is None else excl_ids.data_ptr(), nx, k, ids.data_ptr(), k,
                                 scores.data_ptr(), k, ws.data_ptr(), ws.numel(), st)
    if rc == _ENOTSUP:
        return None
    check(rc, "kge_eval_topk_sweep")
    return ids, scores


def topk_rows(scores: torch.Tensor, k: int, excl_ptr: torch.Tensor | None = None,
              excl_ids: torch.Tensor | None = None, out_ids: torch.Tensor | None = None,
              out_scores: torch.Tensor | None = None):
    """(ids [M, k] int64, scores [M, k]) of the k best columns of each row of a [M, N] fp32 score matrix
    (kge_topk_rows, one block per row), under topk_sweep's contract: the path of score_all's matrix for DistMult /
    ComplEx / TranSparse and for widths the sweep has no kernel for. `out_ids` / `out_scores`: [M, k] views to
    write into (any row stride)."""
    k = _check_k(k, "topk_rows")
    if scores.dim() != 2 or scores.dtype != torch.float32 or (scores.shape[1] > 1 and scores.stride(1) != 1):
        raise ValueError("topk_rows: scores must be a [M, N] float32 matrix with contiguous rows")
    ops._need_gpu(scores)
    M, N = scores.shape
    dev = scores.device
    excl_ptr, excl_ids, nx = _check_excl("topk_rows", dev, M, excl_ptr, excl_ids, None)
    if out_ids is None:
        out_ids = torch.empty((M, k), dtype=torch.int64, device=dev)
    if out_scores is None:
        out_scores = torch.empty((M, k), dtype=torch.float32, device=dev)
    for name, t, dt in (("out_ids", out_ids, torch.int64), ("out_scores", out_scores, torch.float32)):
        if t.shape != (M, k) or t.dtype != dt or t.device != dev or (k > 1 and t.stride(1) != 1):
            raise ValueError(f"topk_rows: {name} must be a [M, k] {dt} tensor with contiguous rows on {dev}")
    check(_lib.load().kge_topk_rows(scores.data_ptr(), M, N, scores.stride(0),
                                    None if excl_ptr is None else excl_ptr.data_ptr(),
                                    None if excl_ids is None else excl_ids.data_ptr(), nx, k, out_ids.data_ptr(),
                                    out_ids.stride(0), out_scores.data_ptr(), out_scores.stride(0),
                                    torch.cuda.current_stream(dev).cuda_stream), "kge_topk_rows")
    return out_ids, out_scores


_TOPK_PLANES_WS = {}


def topk_planes(model, positive_sample: torch.Tensor, mode: str, k: int, planes: torch.Tensor | None,
                excl_ptr: torch.Tensor | None = None, excl_ids: torch.Tensor | None = None,
                nexcl: int | None = None):
    """(ids [B, k] int64, scores [B, k]) of the k best entities per query row for DistMult / ComplEx straight from
    the entity planes, without the [B, E] score matrix (kge_eval_query_planes, then kge_eval_topk_planes: the plane
    GEMM keeping the best k per 256-entity tile, then a merge), under topk_sweep's contract and with its argument
    checks: topk_rows(score_all(..., planes=planes))'s ids and scores exactly. The workspace is k / 128 of the matrix
    it replaces. None exactly where rank_planes answers None (another model, no planes, rows without float4 loads):
    callers fall back to score_all + topk_rows."""
    k = _check_k(k, "topk_planes")
    if not _planes_rank_ok(model, planes):
        return None
    ent, rel = model.entity_embedding.detach(), model.relation_embedding.detach()
    dev = ent.device
    if positive_sample.dim() != 2 or positive_sample.shape[1] != 3:
        raise ValueError("topk_planes: positive_sample must be [B, 3]")
    B, E, K = positive_sample.shape[0], ent.shape[0], ent.shape[1]
    if positive_sample.dtype != torch.int64 or not positive_sample.is_contiguous() or positive_sample.device != dev:
        raise ValueError(f"topk_planes: positive_sample must be a contiguous int64 tensor on {dev}")
    excl_ptr, excl_ids, nx = _check_excl("topk_planes", dev, B, excl_ptr, excl_ids, nexcl)
    ops._need_gpu(ent, rel)
    lib = _lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    key = (str(dev), st)
    nbytes = int(lib.kge_split_bf16x3_bytes(B, K))
    qp = _Q_PLANES.get(key)
    if qp is None or qp.numel() < nbytes:
        qp = _Q_PLANES[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    check(lib.kge_eval_query_planes(FN_IDS[model.model_name], ops.mode_id(mode), ent.data_ptr(), E, ent.stride(0),
                                    rel.data_ptr(), rel.shape[0], rel.stride(0), positive_sample.data_ptr(), B,
                                    model._D, qp.data_ptr(), B, st), "kge_eval_query_planes")
    wsb = int(lib.kge_eval_topk_planes_workspace_size(B, E, k))
    ws = _TOPK_PLANES_WS.get(key)
    if ws is None or ws.numel() < wsb:
        ws = _TOPK_PLANES_WS[key] = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    ids = torch.empty((B, k), dtype=torch.int64, device=dev)
    scores = torch.empty((B, k), dtype=torch.float32, device=dev)
    check(lib.kge_eval_topk_planes(qp.data_ptr(), B, planes.data_ptr(), E, K, B, E,
                                   None if excl_ptr is None else excl_ptr.data_ptr(),
                                   None if excl_ids is None else excl_ids.data_ptr(), nx, k, ids.data_ptr(), k,
                                   scores.data_ptr(), k, ws.data_ptr(), ws.numel(), st), "kge_eval_topk_planes")
    return ids, scores


# The functions predict sends through topk_sweep: those whose sweep measured faster than score_all + topk_rows by
# DESIGN §3.0's rule (§3.4, profiles/r11_topk_ab.txt); the others, and every batch topk_sweep answers None for, take
# the matrix path.
TOPK_SWEEP_FNS = ("TransE", "RotatE", "pRotatE", "InterHT", "PairRE")
# The functions predict sends through topk_planes, up to TOPK_PLANES_MAX_K, by the same rule (§3.4,
# profiles/r15_topk_planes_ab.txt). Empty: the selecting epilogue has not measured faster than score_all +
# topk_rows; topk_planes is there for callers short of the [B, E] matrix's memory.
TOPK_PLANES_FNS = ()
TOPK_PLANES_MAX_K = TOPK_MAX


def predict(model, queries, mode: str, k: int = 10, known_triples=None, batch_size: int | None = None,
            filter_on: str = "device"):
    """Link prediction: for each query triple the k best entities in the candidate slot, (h, r, ?) for tail-batch
    and (?, r, t) for head-batch (the slot's own value is ignored), as (ids [M, k] int64, scores [M, k]) on the
    model's device: score descending, ties by ascending id, padded with -1 / -inf. With `known_triples` (an array
    of triples, or a FilterTable of them to reuse over calls), the answers they already hold for a query are left
    out: the exclusion lists of all queries come from one FilterTable.csr call on the GPU and the batches slice
    them; filter_on="host" (and triples the table refuses: a negative id) makes them with build_exclude instead.
    Batches of `batch_size` (1 024) queries run through topk_sweep where it applies and through score_all +
    topk_rows otherwise (DistMult / ComplEx from the entity planes made once per call). There is no CPU fallback."""
    k = _check_k(k, "predict")
    if mode not in ("head-batch", "tail-batch"):
        raise ValueError("predict: mode must be 'head-batch' or 'tail-batch'")
    ent = model.entity_embedding
    ops._need_gpu(ent, model.relation_embedding)
    dev = ent.device
    q = queries.detach().cpu().numpy() if isinstance(queries, torch.Tensor) else np.asarray(queries)
    q = np.ascontiguousarray(q, dtype=np.int64).reshape(-1, 3)
    M = len(q)
    bs = int(batch_size or 1024)
    if bs < 1:
        raise ValueError("predict: batch_size must be positive")
    ids = torch.empty((M, k), dtype=torch.int64, device=dev)
    scores = torch.empty((M, k), dtype=torch.float32, device=dev)
    ptr = xids = table = q_dev = None
    if known_triples is not None:
        table = _device_table(known_triples, dev, filter_on)
        if table is None:
            ptr, xids = build_exclude(q, mode, known_triples)
        else:
            q_dev = torch.from_numpy(q).to(dev)
            ptr_dev, xids, ptr = table.csr(q_dev, mode, drop_own=False)
            bptr = _batch_ptrs(ptr_dev, M, bs)
    with torch.no_grad():
        planes = entity_planes(model)  # once per call (DistMult / ComplEx)
        sweep = model.model_name in TOPK_SWEEP_FNS
        for s in range(0, M, bs):
            pos = torch.from_numpy(q[s:s + bs]).to(dev) if q_dev is None else q_dev[s:s + bs]
            xp = xi = None
            nx = 0
            if ptr is not None:
                p = ptr[s:s + len(pos) + 1]
                nx = int(p[-1] - p[0])
                if nx and table is None:
                    xp = torch.from_numpy(p - p[0]).to(dev)
                    xi = torch.from_numpy(xids[p[0]:p[-1]]).to(dev)
                elif nx:  # views of the pass's CSR (8-B aligned: every reader loads the ids one by one)
                    xp = bptr[s // bs, :len(pos) + 1]
                    xi = xids[int(p[0]):int(p[-1])]
            got = topk_sweep(model, pos, mode, k, xp, xi, nx) if sweep else None
            if got is None and model.model_name in TOPK_PLANES_FNS and k <= TOPK_PLANES_MAX_K:
                got = topk_planes(model, pos, mode, k, planes, xp, xi, nx)
            if got is None:
                topk_rows(score_all(model, pos, mode, planes=planes), k, xp, xi, ids[s:s + bs], scores[s:s + bs])
            else:
                ids[s:s + bs], scores[s:s + bs] = got
    return ids, scores


class RankPipeline:
    """rank_planes over consecutive query batches on two streams: batch i runs its whole chain (query planes,
    kge_eval_rank_planes_phases' pair scores, counting GEMM and finish) on stream i % 2, with a query-plane buffer and
    a workspace of its own. The counting GEMM holds every CU's VGPRs while its blocks run, so a single stream leaves
    the CUs of its last partial round idle (944 tiles = 3.7 rounds at C5) and runs the small kernels between GEMMs;
    with two streams the next batch's kernels and GEMM blocks fill them. submit() returns the batch's ranks tensor,
    valid on the caller's stream after flush(). Same ranks as rank_planes, batch by batch. DistMult / ComplEx with
    entity planes only (rank_planes' domain). Inputs given as CPU tensors are uploaded on the batch's stream; device
    inputs must already be complete (the streams wait for the caller's stream only in the constructor and in
    wait_caller())."""

    def __init__(self, model, planes: torch.Tensor, max_rows: int, max_filter: int, forms: dict | None = None):
        if model.model_name not in MFMA_FNS or planes is None:
            raise ValueError("RankPipeline: DistMult / ComplEx with entity planes")
        self.m, self.planes = model, planes
        self.ent, self.rel = model.entity_embedding.detach(), model.relation_embedding.detach()
        dev = self.ent.device
        self.lib = _lib.load()
        K = self.ent.shape[1]
        qb = int(self.lib.kge_split_bf16x3_bytes(max_rows, K))
        wb = max(int(self.lib.kge_eval_rank_planes_workspace_size(max_rows, max_filter)), 16)
        self.qp = [torch.empty(qb, dtype=torch.uint8, device=dev) for _ in range(2)]
        self.ws = [torch.empty(wb, dtype=torch.uint8, device=dev) for _ in range(2)]
        self.max_rows, self.max_filter = max_rows, max_filter
        self.main = torch.cuda.current_stream(dev)
        self.streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
        self.forms = forms
        self.i = 0
        self.wait_caller()  # the tables and planes as the caller's stream left them

    def wait_caller(self):
        """Both streams wait for the caller's stream: after the caller rewrote the tables or the planes."""
        for st in self.streams:
            st.wait_stream(self.main)

    def submit(self, positive_sample, mode, truth, filter_ptr=None, filter_ids=None, nfilter=None, events=None):
        """Queue one batch; `events` (optional pair of timing events) are recorded on the batch's stream around its
        counting GEMM."""
        B = positive_sample.shape[0]
        if filter_ptr is not None and nfilter is None:
            nfilter = int(filter_ptr[-1])
        nf = int(nfilter) if filter_ptr is not None else 0
        if B > self.max_rows or nf > self.max_filter:
            raise ValueError("RankPipeline: batch or filter larger than the pipeline was sized for")
        E, K = self.ent.shape
        slot = self.i & 1
        self.i += 1
        st = self.streams[slot]
        dev = self.ent.device
        fp, _keep = ops._forms_ptr(self.forms)
        with torch.cuda.stream(st):
            ranks = torch.empty(B, dtype=torch.int64, device=dev)
            positive_sample, truth, filter_ptr, filter_ids = (
                None if t is None else t.to(dev) for t in (positive_sample, truth, filter_ptr, filter_ids))
            check(self.lib.kge_eval_query_planes(FN_IDS[self.m.model_name], ops.mode_id(mode), self.ent.data_ptr(), E,
                                                 self.ent.stride(0), self.rel.data_ptr(), self.rel.shape[0],
                                                 self.rel.stride(0), positive_sample.data_ptr(), B, self.m._D,
                                                 self.qp[slot].data_ptr(), B, st.cuda_stream), "kge_eval_query_planes")
            args = (self.qp[slot].data_ptr(), B, self.planes.data_ptr(), E, K, B, E, truth.data_ptr(),
                    None if filter_ptr is None else filter_ptr.data_ptr(),
                    None if filter_ids is None else filter_ids.data_ptr(), nf, ranks.data_ptr(),
                    self.ws[slot].data_ptr(), self.ws[slot].numel())
            for ph in (1, 2, 4):  # KGE_RANK_PAIRS, KGE_RANK_COUNT (events around it), KGE_RANK_FINISH
                if ph == 2 and events is not None:
                    events[0].record(st)
                check(self.lib.kge_eval_rank_planes_phases(*args, ph, fp, st.cuda_stream), "kge_eval_rank_planes")
                if ph == 2 and events is not None:
                    events[1].record(st)
            for t in (positive_sample, truth, filter_ptr, filter_ids):
                if t is not None and t.device.type == "cuda":
                    t.record_stream(st)
        ranks.record_stream(self.main)
        return ranks

    def flush(self):
        """The caller's stream waits for both streams (every submitted batch's ranks)."""
        for st in self.streams:
            self.main.wait_stream(st)


def rank_filtered(scores: torch.Tensor, truth: torch.Tensor, filter_ptr: torch.Tensor | None = None,
                  filter_ids: torch.Tensor | None = None) -> torch.Tensor:
    M, N = scores.shape
    ranks = torch.empty(M, dtype=torch.int64, device=scores.device)
    if filter_ids is not None and filter_ids.numel() == 0:  # every row's filter list empty: no filter
        filter_ptr = filter_ids = None
    rc = _lib.load().kge_rank_filtered(scores.data_ptr(), M, N, scores.stride(0), truth.data_ptr(),
                                       None if filter_ptr is None else filter_ptr.data_ptr(),
                                       None if filter_ids is None else filter_ids.data_ptr(), ranks.data_ptr(),
                                       torch.cuda.current_stream(scores.device).cuda_stream)
    check(rc, "kge_rank_filtered")
    return ranks


def metrics_from_ranks(ranks: np.ndarray) -> dict:
    r = np.asarray(ranks, dtype=np.float64)
    return {"MRR": float(np.mean(1.0 / r)), "MR": float(np.mean(r)), "HITS@1": float(np.mean(r <= 1.0)),
            "HITS@3": float(np.mean(r <= 3.0)), "HITS@10": float(np.mean(r <= 10.0))}


def average_precision(y_true, y_score) -> float:
    """Average precision = area under the precision-recall curve, as sklearn's
    average_precision_score (the metric upstream test_step reports as auc_pr for countries):
    sum over distinct score thresholds (descending) of (R_n - R_{n-1}) * P_n."""
    y_true = np.asarray(y_true, dtype=np.float64).reshape(-1)
    y_score = np.asarray(y_score, dtype=np.float64).reshape(-1)
    order = np.argsort(-y_score, kind="mergesort")
    y_true, y_score = y_true[order], y_score[order]
    last = np.r_[np.where(np.diff(y_score) != 0)[0], y_true.size - 1]  # last index of each tie group
    tps = np.cumsum(y_true)[last]
    fps = (last + 1) - tps
    if tps[-1] == 0:
        return 0.0
    precision = tps / (tps + fps)
    recall = tps / tps[-1]
    return float(np.sum(np.diff(np.r_[0.0, recall]) * precision))


def read_regions(data_path, entity2id):
    """Upstream run.py: the countries datasets' candidate regions (data/countries_S*/regions.list)."""
    import os

    with open(os.path.join(data_path, "regions.list")) as fin:
        return [entity2id[line.strip()] for line in fin if line.strip()]


def countries_auc_pr(model, test_triples, regions):
    """Upstream test_step for args.countries: every test (h, r, t) is scored against every candidate
    region (single mode, on the GPU); y_true marks the true region; auc_pr = average precision."""
    dev = model.entity_embedding.device
    sample, y_true = [], []
    for h, r, t in np.asarray(test_triples, dtype=np.int64).reshape(-1, 3).tolist():
        for region in regions:
            y_true.append(1 if region == t else 0)
            sample.append((h, r, region))
    pos = torch.tensor(sample, dtype=torch.int64, device=dev)
    with torch.no_grad():
        y_score = model.score(ops.SINGLE, pos).reshape(-1).cpu().numpy()
    return {"auc_pr": average_precision(np.array(y_true), y_score)}


def test_step(model, test_triples, all_true_triples, args=None, batch_size=None, filter_on="device"):
    """Upstream `KGEModel.test_step(model, test_triples, all_true_triples, args)`: filtered MRR,
    MR and HITS@{1,3,10} over head-batch and tail-batch ranking of every test triple; with
    args.countries, the AUC-PR over args.regions instead. The filter lists come from a FilterTable of
    `all_true_triples` (which may be one already, to reuse it over validation passes): the test triples go to the
    device once, one FilterTable.csr call per mode makes the whole pass's CSR on the GPU and the batches take views
    of it. filter_on="host" (and triples the table refuses: a negative id) builds them with build_filter on the
    host instead: the same ranks."""
    if args is not None and getattr(args, "countries", False):
        return countries_auc_pr(model, test_triples, args.regions)
    bs = batch_size or int(getattr(args, "test_batch_size", 1024) or 1024)
    dev = model.entity_embedding.device
    triples = np.asarray(test_triples, dtype=np.int64).reshape(-1, 3)
    # multi-GPU: replicas. Each rank ranks a strided share of the test triples against its own copy
    # of the table; the integer ranks are all-gathered before the metrics (no collective while scoring)
    import torch.distributed as dist

    world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
    if world > 1:
        triples = triples[dist.get_rank()::world]
    table = _device_table(all_true_triples, dev, filter_on)
    modes = ("head-batch", "tail-batch")
    all_ranks = []
    with torch.no_grad():
        planes = entity_planes(model)  # once per evaluation pass (DistMult / ComplEx)
        sweep = _sweep_rank_ok(model)
        if table is not None and len(triples):
            # everything the batches read is made here, on the caller's stream, before the pipeline (whose streams
            # wait for the caller's in its constructor) exists: the pass's CSRs, the rebased batch starts and the
            # truth columns. The batches' ids are views of csr's tensors, which live until the ranks are on the host
            M = len(triples)
            pos_all = torch.from_numpy(np.array(triples)).to(dev)  # a copy: the caller's array may be read-only
            csr = {m: table.csr(pos_all, m, drop_own=True) for m in modes}
            bptr = {m: _batch_ptrs(csr[m][0], M, bs) for m in modes}
            truth = {m: pos_all[:, 0 if m == "head-batch" else 2].contiguous() for m in modes}
            starts = range(0, M, bs)
            pipe = None
            if _planes_rank_ok(model, planes):
                # ranks straight from the planes (no [B, E] score matrix), batches pipelined over two streams
                maxf = max(int(ph[min(s + bs, M)] - ph[s]) for _, _, ph in csr.values() for s in starts)
                pipe = RankPipeline(model, planes, min(bs, M), maxf)
            for mode in modes:
                _, ids_dev, ph = csr[mode]
                for s in starts:
                    n = min(bs, M - s)
                    pos, tr = pos_all[s:s + n], truth[mode][s:s + n]
                    fptr = bptr[mode][s // bs, :n + 1]
                    # an 8-B aligned view: every reader of the filter ids loads them one by one
                    fids = ids_dev[int(ph[s]):int(ph[s + n])]
                    nf = int(ph[s + n] - ph[s])
                    if pipe is not None:
                        all_ranks.append(pipe.submit(pos, mode, tr, fptr, fids, nf))
                        continue
                    r = rank_sweep(model, pos, mode, tr, fptr, fids, nf) if sweep else None
                    if r is None:
                        r = rank_filtered(score_all(model, pos, mode, planes=planes), tr, fptr, fids)
                    all_ranks.append(r)
            if pipe is not None:
                pipe.flush()
            all_ranks = [r.cpu().numpy() for r in all_ranks]
        elif _planes_rank_ok(model, planes) and len(triples):
            # ranks straight from the planes (no [B, E] score matrix), batches pipelined over two streams
            filt = {m: build_filter(triples, m, all_true_triples) for m in modes}
            starts = range(0, len(triples), bs)
            maxf = max(int(ptr[min(s + bs, len(triples))] - ptr[s]) for ptr, _ in filt.values() for s in starts)
            pipe = RankPipeline(model, planes, min(bs, len(triples)), maxf)
            for mode in modes:
                col = 0 if mode == "head-batch" else 2
                ptr, ids = filt[mode]
                for s in starts:
                    q = triples[s:s + bs]
                    p = ptr[s:s + len(q) + 1]
                    pos = torch.from_numpy(q)
                    all_ranks.append(pipe.submit(pos, mode, pos[:, col].contiguous(), torch.from_numpy(p - p[0]),
                                                 torch.from_numpy(ids[p[0]:p[-1]]), int(p[-1] - p[0])))
            pipe.flush()
            all_ranks = [r.cpu().numpy() for r in all_ranks]
        for mode in (() if all_ranks else modes):
            col = 0 if mode == "head-batch" else 2
            ptr, ids = build_filter(triples, mode, all_true_triples)
            for s in range(0, len(triples), bs):
                q = triples[s:s + bs]
                pos = torch.from_numpy(q).to(dev)
                p = ptr[s:s + len(q) + 1]
                fptr = torch.from_numpy(p - p[0]).to(dev)
                fids = torch.from_numpy(ids[p[0]:p[-1]]).to(dev)
                truth = pos[:, col].contiguous()
                # the distance functions: ranks from one sweep of the table per group of query rows (no [B, E]
                # score matrix); the matrix path where the sweep does not apply
                r = rank_sweep(model, pos, mode, truth, fptr, fids, int(p[-1] - p[0])) if sweep else None
                if r is None:
                    r = rank_filtered(score_all(model, pos, mode, planes=planes), truth, fptr, fids)
                all_ranks.append(r.cpu().numpy())
    ranks = np.concatenate(all_ranks) if all_ranks else np.zeros(0, dtype=np.int64)
    if world > 1:
        gathered = [None] * world
        dist.all_gather_object(gathered, ranks)
        ranks = np.concatenate(gathered)
    return metrics_from_ranks(ranks)


__all__ = ["build_filter", "score_all", "rank_filtered", "rank_planes", "rank_sweep", "RankPipeline", "metrics_from_ranks", "test_step", "entity_planes",
           "split_planes", "HEAD_BATCH", "TAIL_BATCH", "build_exclude", "topk_sweep", "topk_rows", "topk_planes", "predict", "TOPK_MAX",
           "FilterTable", "build_filter_table", "rank_candidates", "test_step_candidates"]
