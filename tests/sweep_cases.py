"""Helpers of the sweep-rank and sweep-top-k width tests (test_sweep_widths_gpu.py, test_sweep_cases_cpu.py):
kge_eval_rank_sweep and kge_eval_topk_sweep on table views of every row stride and base alignment tests/strided.py
names, against references written from include/kge_hip.h and the fp64 oracle, not from the kernels. The seeded
cases (E = 523, B = 40: three row groups with a short last one, two chunks per entity slice), the layouts, the
kernel instance and block decomposition the host code chooses (restated from csrc/kge_abi.hip and kge_internal.h),
fp64 score matrices, truths whose fp64 rank no evaluation within the project's score bar can move, filter /
exclusion lists with the edge rows, the top-k checks against fp64, canary buffers of any element type, and raw
callers of the two entry points. A plain module: nothing here is a fixture or changes how the suite is collected."""
import functools

import numpy as np
import torch

from oracle import kge_oracle as O
from tests import eval_cases as C
from tests import strided as S

FNS = ("TransE", "RotatE", "pRotatE", "InterHT")
WIDTHS = (16, 128, 264, 1000, 50, 33, 255)  # per-half widths D
# float2 rows at two register groups need an even D in 130 .. 256, which WIDTHS does not hold (264 is G = 4 at V = 2,
# 128 is G = 1): 130 is there for the (V, G) = (2, 2) instance alone (dense, rel_pad2, pad2, off2)
EXTRA_WIDTHS = (130,)
ALL_WIDTHS = WIDTHS + EXTRA_WIDTHS
LAYOUTS = ("dense", "pad4", "pad2", "pad1", "ent_pad1", "rel_pad2", "off1", "off2")
MODES = ((0, "head-batch"), (1, "tail-batch"))
KS = (1, 10, 64)
E, R, B, GAMMA = 523, 7, 40, 12.0
ENOTSUP = C.ENOTSUP
TOL = 1e-4  # the project's score bar (tests/test_widths_gpu.py): |fp32 - fp64| <= TOL * max(1, |fp64|)
K_SWEEP_MAX_G, K_SWEEP_MAX_ROWS, K_SWEEP_WAVES, K_SWEEP_MIN_BLOCKS = 4, 16, 16, 256  # csrc/kge_internal.h
K_SWEEP_LDS_MAX, K_TILE_LDS_MAX = 144 * 1024, 160 * 1024
NQ = {"TransE": 1, "RotatE": 2, "pRotatE": 1, "InterHT": 3}  # shard_nq: LDS operand images per query row
ROW_MINUS1, ROW_E = 3, 5  # the query rows whose truth is -1 / E
ROW_EMPTY, ROW_LONG, ROW_TRUTH, ROW_OUTSIDE, ROW_ALL = 0, 1, 2, 4, 6  # the filter / exclusion lists' edge rows


@functools.lru_cache(maxsize=None)
def case(name, d):
    return S.make_case(name, d, E=E, R=R, B=B, N=1, seed=d, gamma=GAMMA)


# ------------------------------------------------------------------------------------------------
# layouts and the instance the host code chooses
# ------------------------------------------------------------------------------------------------
_SPECS = {"dense": (None, None), "pad4": (("pad", 4), ("pad", 4)), "pad2": (("pad", 2), ("pad", 2)),
          "pad1": (("pad", 1), ("pad", 1)), "ent_pad1": (("pad", 1), None), "rel_pad2": (None, ("pad", 2)),
          "off1": (("off", 1), ("off", 1)), "off2": (("off", 2), ("off", 2))}


def _lay(t, spec, device):
    if spec is None:
        v = t.to(device) if device is not None else t.clone()
        assert v.is_contiguous() and v.data_ptr() % 16 == 0
        return v
    return S.padded(t, spec[1], device) if spec[0] == "pad" else S.offset(t, spec[1], device)


def lay(ent, rel, layout, device=None):
    """(entity view, relation view) of a named layout (tests/test_strides_gpu.py's names and meaning): NaN in
    every padding element and around an offset view."""
    es, rs = _SPECS[layout]
    return _lay(ent, es, device), _lay(rel, rs, device)


def layout_promise(layout):
    """What a layout's name promises of (entity, relation): (row padding in floats, base residue in bytes mod 16)."""
    out = []
    for spec in _SPECS[layout]:
        out.append((0, 0) if spec is None else ((spec[1], 0) if spec[0] == "pad" else (0, 4 * spec[1])))
    return tuple(out)


def expected(name, d, ent, rel):
    """(V, G, supported) of kge_eval_rank_sweep / kge_eval_topk_sweep for these table views: pick_vg's choice
    (strided.table_vg), supported up to kSweepMaxG register groups."""
    V, G = S.table_vg(name, d, ent, rel)
    return V, G, G <= K_SWEEP_MAX_G


def block_rule(name, V, G, entry, k=None, nrows=B, nent=E):
    """The decomposition the host chooses (csrc/kge_abi.hip: kge_eval_rank_sweep, kge_eval_topk_sweep; sweep_chunks
    in kge_internal.h): query rows per block R (as many rows' LDS as the budget holds, at most kSweepMaxRows), row
    groups, the rows of the last group, chunks per entity slice and the slice height S."""
    img = NQ[name] * G * S.K_WAVE * V * 4
    if entry == "rank":
        row_lds, budget = img + 8, K_SWEEP_LDS_MAX
    else:
        row_lds, budget = img + K_SWEEP_WAVES * k * 8 + 16, K_TILE_LDS_MAX
    rows = min(K_SWEEP_MAX_ROWS, nrows, budget // row_lds)
    groups = (nrows + rows - 1) // rows
    slice_rows = (nent + 7) // 8
    want = (K_SWEEP_MIN_BLOCKS + groups * 8 - 1) // (groups * 8)
    most = max(1, slice_rows // (2 * K_SWEEP_WAVES))
    return dict(R=rows, groups=groups, last=nrows - (groups - 1) * rows, chunks=max(1, min(want, most)), S=slice_rows)


# ------------------------------------------------------------------------------------------------
# fp64 references
# ------------------------------------------------------------------------------------------------
def bar(ref):
    return TOL * np.maximum(1.0, np.abs(ref))


@functools.lru_cache(maxsize=None)
def ref_scores(name, d, mode):
    """fp64 scores [B, E] of every entity as the candidate (O.score on the fp32 tables' values), as numpy."""
    c = case(name, d)
    ent, rel = c["ent"].double(), c["rel"].double()
    rows = []
    for s in range(0, B, 8):  # a few query rows at a time: the gathered candidates of d = 1000 are large
        pos = c["pos"][s:s + 8]
        cand = torch.arange(E).unsqueeze(0).expand(len(pos), E)
        rows.append(O.score(name, ent, rel, pos, cand, mode, c["gamma"], c["rng"], c["mod"]))
    out = torch.cat(rows).numpy()
    assert out.shape == (B, E) and np.isfinite(out).all()
    out.setflags(write=False)
    return out


def isolated(row):
    """Which candidates of one fp64 score row are isolated: no other candidate's score within
    2 (bar_e + bar_other). Two fp32 scores each within its bar of fp64 keep the fp64 order once the gap exceeds the
    sum of the bars; the factor 2 is slack."""
    b = bar(row)
    gap = np.abs(row[:, None] - row[None, :])
    need = 2.0 * (b[:, None] + b[None, :])
    far = gap > need
    np.fill_diagonal(far, True)
    return far.all(axis=1)


def targets():
    """The fp64 rank each query row's truth aims at: the best, the worst, then quantiles of 1 .. E."""
    t = np.rint(1 + (E - 1) * ((np.arange(B) * 0.381966) % 1.0)).astype(np.int64)
    t[0], t[1] = 1, E
    return t


@functools.lru_cache(maxsize=None)
def truths(name, d, mode):
    """(truth [B] int64, the number of isolated candidates per row [B]): per query row the isolated candidate whose
    fp64 rank is nearest to targets()[row]; rows ROW_MINUS1 and ROW_E get truth -1 and truth E."""
    ref = ref_scores(name, d, mode)
    want = targets()
    truth, count = np.empty(B, dtype=np.int64), np.empty(B, dtype=np.int64)
    for q in range(B):
        iso = isolated(ref[q])
        count[q] = int(iso.sum())
        assert count[q] > 0, (name, d, mode, q, "no isolated candidate")
        rank = 1 + (ref[q][None, :] > ref[q][:, None]).sum(axis=1)  # unfiltered fp64 rank of every candidate
        ids = np.nonzero(iso)[0]
        truth[q] = ids[np.argmin(np.abs(rank[ids] - want[q]))]
    truth[ROW_MINUS1], truth[ROW_E] = -1, E
    truth.setflags(write=False)
    return truth, count


def truth_ranks(name, d, mode):
    """The unfiltered fp64 ranks of the chosen truths (the out-of-range rows left out)."""
    ref, (truth, _) = ref_scores(name, d, mode), truths(name, d, mode)
    return np.array([1 + int((ref[q] > ref[q, truth[q]]).sum()) for q in range(B) if 0 <= truth[q] < E])


@functools.lru_cache(maxsize=None)
def filters(name, d, mode):
    """(ptr [B + 1], ids): per query row a list of distinct ascending ids, the filter of the rank sweep and the
    exclusion list of the top-k sweep alike: row ROW_EMPTY empty, ROW_LONG more than 64 ids, ROW_TRUTH holds the
    row's truth, ROW_OUTSIDE holds -1 and E, ROW_ALL every entity, the rest random subsets of up to 12 ids."""
    truth, _ = truths(name, d, mode)
    g = np.random.RandomState(1000 * d + 10 * FNS.index(name) + mode)
    rows = [np.unique(g.randint(E, size=g.randint(1, 13))) for _ in range(B)]
    rows[ROW_EMPTY] = np.zeros(0, dtype=np.int64)
    rows[ROW_LONG] = np.sort(g.choice(E, size=90, replace=False))
    rows[ROW_TRUTH] = np.union1d(rows[ROW_TRUTH], [truth[ROW_TRUTH]])
    rows[ROW_OUTSIDE] = np.concatenate([[-1], rows[ROW_OUTSIDE], [E]])
    rows[ROW_ALL] = np.arange(E)
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    ids = np.concatenate(rows).astype(np.int64)
    ptr.setflags(write=False)
    ids.setflags(write=False)
    return ptr, ids


def rank_bounds(ref, truth, ptr=None, ids=None):
    """(lo, hi) int64 [B] of include/kge_hip.h's filtered rank under a perturbation of every score by its bar
    (O.eval_ranks_dense's bounds at atol = bar): lo counts the candidates above the truth by more than both bars,
    hi those not below it by more. An out-of-range truth scores -inf: every score is above it."""
    lo, hi = np.empty(len(truth), dtype=np.int64), np.empty(len(truth), dtype=np.int64)
    b = bar(ref)
    for q, tr in enumerate(np.asarray(truth).tolist()):
        keep = np.ones(ref.shape[1], dtype=bool)
        if ptr is not None:
            f = np.asarray(ids[ptr[q]:ptr[q + 1]])
            keep[f[(f >= 0) & (f < ref.shape[1])]] = False
        if 0 <= tr < ref.shape[1]:
            keep[tr] = False
            dlt, tol = ref[q] - ref[q, tr], b[q] + b[q, tr]
            lo[q], hi[q] = 1 + int(((dlt > tol) & keep).sum()), 1 + int(((dlt > -tol) & keep).sum())
        else:
            lo[q] = hi[q] = 1 + int(keep.sum())
    return lo, hi


@functools.lru_cache(maxsize=None)
def expected_ranks(name, d, mode, filtered=True):
    """eval_cases.rank_ref (the header's rank) on the fp64 scores: with an isolated truth the only rank an
    evaluation within the bar can return."""
    truth, _ = truths(name, d, mode)
    ptr, ids = filters(name, d, mode) if filtered else (None, None)
    return C.rank_ref(ref_scores(name, d, mode), truth, ptr, ids)


def check_topk_fp64(ref, got_ids, got_scores, k, ptr=None, ids=None):
    """tests/test_topk_gpu.py::test_against_fp64_oracle's checks of a top-k result against fp64 scores ref [B, E]:
    every returned id is valid (in range, not excluded) and distinct, its score within the bar of its fp64 score,
    and its fp64 score at least the fp64 k-th best valid score minus twice the bar; a row with n < k valid
    entities returns all n and then (-1, -inf) padding."""
    gi, gs = got_ids.cpu().numpy(), got_scores.cpu().double().numpy()
    rows, n_ent = ref.shape
    assert gi.shape == (rows, k) and gs.shape == (rows, k)
    for q in range(rows):
        valid = np.ones(n_ent, dtype=bool)
        if ptr is not None:
            x = np.asarray(ids[ptr[q]:ptr[q + 1]])
            valid[x[(x >= 0) & (x < n_ent)]] = False
        n = min(k, int(valid.sum()))
        assert (gi[q, n:] == -1).all() and np.isneginf(gs[q, n:]).all(), (q, "padding")
        if n == 0:
            continue
        i = gi[q, :n]
        assert (i >= 0).all() and (i < n_ent).all() and valid[i].all() and len(set(i.tolist())) == n, (q, i)
        r = ref[q, i]
        assert (np.abs(gs[q, :n] - r) <= bar(r)).all(), (q, "score off its fp64 value")
        kth = np.sort(ref[q][valid])[::-1][n - 1]
        assert (r >= kth - 2 * TOL * max(1.0, abs(float(kth)))).all(), (q, "an id below the k-th best")
        assert (np.diff(gs[q, :n]) <= 0).all(), (q, "scores not descending")


def topk_reference(Sm, k, ptr=None, ids=None):
    """The k best columns of each row of the CPU matrix Sm by a stable descending sort, excluded ids and NaNs
    dropped first (candidates in ascending id, so ties come out by ascending id): (ids [M, k] int64, scores
    [M, k]), -1 / -inf padding. The yardstick of tests/test_topk_gpu.py, which imports it from here."""
    Sm = Sm.detach().cpu()
    M, N = Sm.shape
    out_i = torch.full((M, k), -1, dtype=torch.int64)
    out_s = torch.full((M, k), float("-inf"), dtype=torch.float32)
    for b in range(M):
        valid = ~torch.isnan(Sm[b])
        if ptr is not None:
            x = torch.as_tensor(np.asarray(ids[int(ptr[b]):int(ptr[b + 1])], dtype=np.int64))
            valid[x[(x >= 0) & (x < N)]] = False
        cand = torch.nonzero(valid).reshape(-1)  # ascending id
        s, order = torch.sort(Sm[b][cand], descending=True, stable=True)
        n = min(k, len(cand))
        out_i[b, :n] = cand[order[:n]]
        out_s[b, :n] = s[:n]
    return out_i, out_s


def same_topk(got, want):
    """ids equal and scores bitwise equal."""
    gi, gs = got[0].cpu(), got[1].cpu()
    return torch.equal(gi, want[0]) and torch.equal(gs.contiguous().view(torch.int32), want[1].contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------
# canary buffers of any element type
# ------------------------------------------------------------------------------------------------
CANARY64 = 0x5CA1AB1E0DDBA11  # int64 pattern of the id / rank buffers: no id, rank or -1


def canary_i64(rows, w, ld, device, k=0):
    """An int64 [rows, w] view with row stride ld starting k elements into a buffer that holds CANARY64 everywhere
    (the view's own elements too); w = None: a 1-D view of `rows` elements."""
    if w is None:
        buf = torch.full((rows + k + 5,), CANARY64, dtype=torch.int64, device=device)
        return buf[k:k + rows]
    assert ld >= w
    buf = torch.full((rows * ld + k + 5,), CANARY64, dtype=torch.int64, device=device)
    return buf[k:k + rows * ld].view(rows, ld)[:, :w]


def canary_bytes(nbytes, device, lead=48, tail=80):
    """(buffer, view): a uint8 view of exactly nbytes bytes, 16-B aligned, `lead` bytes into a buffer of 0xA5."""
    buf = torch.full((lead + nbytes + tail,), 0xA5, dtype=torch.uint8, device=device)
    v = buf[lead:lead + nbytes]
    assert v.data_ptr() % 16 == 0 and lead % 16 == 0
    return buf, v


def outside(v):
    """A copy of every element of v's underlying buffer that is not an element of v (any element type, v 1-D or
    2-D with contiguous rows): equal before and after a call exactly when the call wrote nothing outside v."""
    base = v._base if v._base is not None else v
    flat = base.reshape(-1)
    es = flat.element_size()
    keep = torch.ones(flat.numel(), dtype=torch.bool, device=v.device)
    start = (v.data_ptr() - base.data_ptr()) // es
    rows, w = (v.shape[0], v.shape[1]) if v.dim() == 2 else (1, v.numel())
    ld = v.stride(0) if v.dim() == 2 and rows > 1 else w
    idx = start + torch.arange(rows, device=v.device)[:, None] * ld + torch.arange(w, device=v.device)[None, :]
    keep[idx.reshape(-1)] = False
    out = flat[keep].clone()
    return out.view(torch.int32) if out.dtype == torch.float32 else out


# ------------------------------------------------------------------------------------------------
# raw callers
# ------------------------------------------------------------------------------------------------
def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def rank_sweep_raw(c, mode, ent, rel, pos, truth, fptr, fids, nfilter, ranks, ws, ws_bytes=None):
    """kge_eval_rank_sweep of case c on the table views ent / rel (rel_off from strided.rel_off), explicit outputs
    and workspace (a uint8 view); returns the return code."""
    from customknowledgegraphembedding_amd import _lib

    return _lib.load().kge_eval_rank_sweep(
        _lib.FN_IDS[c["name"]], mode, ent.data_ptr(), ent.shape[0], ent.stride(0), rel.data_ptr(), rel.shape[0],
        rel.stride(0), S.rel_off(c["name"], c["D"]), pos.data_ptr(), pos.shape[0], c["D"], c["gamma"], c["rng"],
        c["mod"], truth.data_ptr(), _ptr(fptr), _ptr(fids), nfilter, ranks.data_ptr(), ws.data_ptr(),
        ws.numel() if ws_bytes is None else ws_bytes, _stream(ent))


def topk_sweep_raw(c, mode, ent, rel, pos, xptr, xids, nexcl, k, out_ids, out_scores, ws, ws_bytes=None):
    """kge_eval_topk_sweep of case c on the table views ent / rel into the [B, k] views out_ids / out_scores (their
    row strides are passed as ids_ld / scores_ld) with an explicit workspace; returns the return code."""
    from customknowledgegraphembedding_amd import _lib

    rows = pos.shape[0]
    return _lib.load().kge_eval_topk_sweep(
        _lib.FN_IDS[c["name"]], mode, ent.data_ptr(), ent.shape[0], ent.stride(0), rel.data_ptr(), rel.shape[0],
        rel.stride(0), S.rel_off(c["name"], c["D"]), pos.data_ptr(), rows, c["D"], c["gamma"], c["rng"], c["mod"],
        _ptr(xptr), _ptr(xids), nexcl, k, out_ids.data_ptr(), out_ids.stride(0) if rows > 1 else k,
        out_scores.data_ptr(), out_scores.stride(0) if rows > 1 else k, ws.data_ptr(),
        ws.numel() if ws_bytes is None else ws_bytes, _stream(ent))


def score_matrix(c, mode, ent, rel, pos):
    """kge_score_indexed_ex's [B, E] matrix of candidates 0 .. E - 1 (row stride 0 ids) on the same table views:
    what the header holds both sweeps to, bitwise."""
    from customknowledgegraphembedding_amd import _lib, ops

    n_ent = ent.shape[0]
    cand = torch.arange(n_ent, device=ent.device, dtype=torch.int64).unsqueeze(0).expand(pos.shape[0], n_ent)
    return ops.score_indexed_raw(_lib.FN_IDS[c["name"]], mode, ent, rel, S.rel_off(c["name"], c["D"]), pos, cand,
                                 c["D"], c["gamma"], c["rng"], c["mod"])
