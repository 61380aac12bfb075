"""kge_eval_rank_sweep and kge_eval_topk_sweep (rank_pairs_kernel, rank_sweep_kernel, topk_sweep_kernel,
topk_merge_kernel) at every vector width, register depth, row stride and base alignment their host code branches
on, on table views with NaN in every padding element, against references that do not share the kernels' arithmetic
(tests/sweep_cases.py): exact ranks from the fp64 oracle on truths no evaluation within the score bar can move, the
top-k checks against fp64, and, as the header's contract, rank_filtered / a stable sort of kge_score_indexed_ex's
matrix on the same views, bitwise. Every output and workspace lies in a buffer of a known bit pattern and nothing
outside it may change; combinations past four register groups are refused with KGE_ENOTSUP and write nothing; the
Python layer (rank_sweep, topk_sweep, test_step, predict) falls back exactly there."""
import functools

import numpy as np
import pytest
import torch

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import _lib as L
from customknowledgegraphembedding_amd import evaluate
from tests import strided as S
from tests import sweep_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
# one case per (function, width, mode): a case pays for its fp64 reference (RotatE d = 1000: seconds per mode)
CASES = [(n, d, m) for n in W.FNS for d in W.ALL_WIDTHS for m, _ in W.MODES]
case_params = pytest.mark.parametrize("name,d,mode", CASES, ids=[f"{n}-{d}-{W.MODES[m][1]}" for n, d, m in CASES])


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.int64)).to(DEV)  # (a copy: the cases' arrays are read-only)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ceil16(n):
    return (n + 15) // 16 * 16


def _last_error():
    return L.load().kge_last_error().decode(errors="replace")


def _refusal_names_the_width(msg, d, V):
    """A refused call's message speaks of the per-half width: pick_vg's names D and its own limit, the sweeps'
    names the widest per-half width their instances hold at this vector width."""
    return "per-half dim" in msg and (str(d) in msg or str(W.K_SWEEP_MAX_G * S.K_WAVE * V) in msg)


@functools.lru_cache(maxsize=None)
def _lists(name, d, mode):
    """The case's truth and filter / exclusion lists on the device."""
    truth, _ = W.truths(name, d, mode)
    ptr, ids = W.filters(name, d, mode)
    return _dev(truth), _dev(ptr), _dev(ids)


def _rank_call(c, mode, ent, rel, pos, truth, fptr, fids, nf):
    """One kge_eval_rank_sweep call into canary buffers: (rc, ranks view, workspace buffer, workspace view, whether
    anything outside the ranks and outside the workspace's declared bytes changed)."""
    wsb = int(L.load().kge_eval_rank_sweep_workspace_size(W.B, nf))
    assert wsb == _ceil16(8 * W.B) + _ceil16(4 * nf)  # the header's layout
    ranks = W.canary_i64(W.B, None, None, DEV, k=7)
    buf, ws = W.canary_bytes(wsb, DEV)
    r_before, lead, tail = W.outside(ranks), buf[:48].clone(), buf[48 + wsb:].clone()
    rc = W.rank_sweep_raw(c, mode, ent, rel, pos, truth, fptr, fids, nf, ranks, ws)
    torch.cuda.synchronize()
    intact = torch.equal(W.outside(ranks), r_before) and torch.equal(buf[:48], lead) and torch.equal(buf[48 + wsb:], tail)
    return rc, ranks, buf, ws, intact


@case_params
def test_rank_sweep_every_layout(name, d, mode):
    """Where the instance exists: rc 0; ranks equal to the fp64 expectation exactly (the truths are isolated) and to
    rank_filtered of kge_score_indexed_ex's matrix on the same views; the workspace's truth scores, counts and
    filter-entry scores bitwise that matrix's, and within the bar of fp64 (-inf for the out-of-range truths);
    nothing written outside ranks [B] and the workspace's declared bytes; the same without a filter; pad4 bitwise
    the dense call. Elsewhere: KGE_ENOTSUP, nothing written, a message that names the width."""
    c = W.case(name, d)
    pos = c["pos"].to(DEV)
    reached, refused, dense = set(), set(), {}
    worst = 0.0
    for layout in W.LAYOUTS:
        ent, rel = W.lay(c["ent"], c["rel"], layout, DEV)
        V, G, ok = W.expected(name, d, ent, rel)
        tag = (layout, mode, V, G)
        truth, fptr, fids = _lists(name, d, mode)
        nf = fids.numel()
        rc, ranks, buf, ws, intact = _rank_call(c, mode, ent, rel, pos, truth, fptr, fids, nf)
        assert intact, (tag, "written outside ranks [B] or the workspace's bytes")
        if not ok:
            assert rc == W.ENOTSUP, (tag, rc, _last_error())
            assert _refusal_names_the_width(_last_error(), d, V), (tag, _last_error())
            assert bool((ranks == W.CANARY64).all()) and bool((buf == 0xA5).all()), (tag, "a refused call wrote")
            refused.add(layout)
            continue
        assert rc == 0, (tag, rc, _last_error())
        reached.add((V, G))
        got = ranks.cpu()
        want = W.expected_ranks(name, d, mode)
        assert torch.equal(got, want), (tag, "fp64", got.tolist(), want.tolist())
        Sm = W.score_matrix(c, mode, ent, rel, pos)
        assert torch.equal(ranks, evaluate.rank_filtered(Sm, truth, fptr, fids)), (tag, "same-view matrix")
        # the workspace: [B] truth scores, [B] counts, then the filter entries' scores at the next 16 B
        Sc, tc = Sm.cpu(), truth.cpu()
        inr = (tc >= 0) & (tc < W.E)
        ts = ws[:4 * W.B].view(torch.float32).cpu()
        rows = torch.arange(W.B)
        assert torch.equal(_bits(ts[inr]), _bits(Sc[rows[inr], tc[inr]])), (tag, "truth scores")
        assert bool(torch.isneginf(ts[~inr]).all()) and int((~inr).sum()) == 2, (tag, "out-of-range truths")
        cnt = ws[4 * W.B:8 * W.B].view(torch.int32).cpu()
        assert torch.equal(cnt.long(), (Sc > ts[:, None]).sum(1)), (tag, "counts")
        fs = ws[_ceil16(8 * W.B):_ceil16(8 * W.B) + 4 * nf].view(torch.float32).cpu()
        fc, pc = fids.cpu(), fptr.cpu()
        frow = torch.repeat_interleave(rows, pc[1:] - pc[:-1])
        fin = (fc >= 0) & (fc < W.E)
        assert int((~fin).sum()) == 2 and nf > W.E
        assert torch.equal(_bits(fs[fin]), _bits(Sc[frow[fin], fc[fin]])), (tag, "filter-entry scores")
        ref = torch.from_numpy(W.ref_scores(name, d, mode).copy())  # (a copy: the cached array is read-only)
        for what, gs, r in (("truth", ts[inr], ref[rows[inr], tc[inr]]), ("filter", fs[fin], ref[frow[fin], fc[fin]])):
            err = ((gs.double() - r).abs() / r.abs().clamp_min(1.0)).max().item()
            worst = max(worst, err)
            assert err <= W.TOL, (tag, what, err)
        # no filter: NULL, NULL, 0
        rc0, ranks0, _, ws0, intact0 = _rank_call(c, mode, ent, rel, pos, truth, None, None, 0)
        assert rc0 == 0 and intact0, (tag, "no filter", rc0)
        assert torch.equal(ranks0.cpu(), W.expected_ranks(name, d, mode, False)), (tag, "no filter, fp64")
        assert torch.equal(ranks0, evaluate.rank_filtered(Sm, truth)), (tag, "no filter, same-view matrix")
        assert torch.equal(ws0[:8 * W.B], ws[:8 * W.B]), (tag, "no filter: truth scores and counts")
        if layout == "dense":
            dense[mode] = (got, ws.cpu().clone())
        if layout == "pad4":  # 16-B base, stride a multiple of 4: the dense instance, bitwise
            assert torch.equal(got, dense[mode][0]) and torch.equal(ws.cpu(), dense[mode][1]), (tag, "pad4 != dense")
    want_refused = {lay for lay in W.LAYOUTS if not W.expected(name, d, *W.lay(c["ent"], c["rel"], lay))[2]}
    assert refused == want_refused
    print(f"rank sweep {name} D={d} {W.MODES[mode][1]}: (V, G) reached {sorted(reached)}, refused layouts {sorted(refused)}, "
          f"largest workspace score error {worst:.2e} of the bar's scale")


_TOPK_REF = {}


def _topk_ref(Sc, k, ptr, ids, filtered):
    """sweep_cases.topk_reference, remembered by the matrix's bits (layouts of one vector width give one matrix)."""
    key = (hash(Sc.numpy().tobytes()), k, filtered)
    if key not in _TOPK_REF:
        _TOPK_REF[key] = W.topk_reference(Sc, k, ptr if filtered else None, ids if filtered else None)
    return _TOPK_REF[key]


def _topk_call(c, mode, ent, rel, pos, xptr, xids, nx, k, padded):
    """One kge_eval_topk_sweep call into canary buffers (padded: ids_ld = k + 3, scores_ld = k + 5 starting one float
    into the buffer; else dense rows): (rc, ids view, scores view, workspace buffer, whether anything outside
    [B, k] of either output or outside the workspace's bytes changed)."""
    wsb = int(L.load().kge_eval_topk_sweep_workspace_size(W.B, k))
    assert wsb == _ceil16(8 * (W.K_SWEEP_MIN_BLOCKS // 8 * W.K_SWEEP_MAX_ROWS + W.B) * k * 8)  # topk_ws_lists
    oi = W.canary_i64(W.B, k, k + 3 if padded else k, DEV)
    osc = S.canary(W.B, k, k + 5 if padded else k, DEV, k=1 if padded else 0)
    buf, ws = W.canary_bytes(wsb, DEV)
    i_before, s_before, lead, tail = W.outside(oi), S.outside_bits(osc), buf[:48].clone(), buf[48 + wsb:].clone()
    rc = W.topk_sweep_raw(c, mode, ent, rel, pos, xptr, xids, nx, k, oi, osc, ws)
    torch.cuda.synchronize()
    intact = (torch.equal(W.outside(oi), i_before) and torch.equal(S.outside_bits(osc), s_before)
              and torch.equal(buf[:48], lead) and torch.equal(buf[48 + wsb:], tail))
    return rc, oi, osc, buf, intact


@case_params
def test_topk_sweep_every_layout(name, d, mode):
    """k = 1, 10, 64 into row-padded outputs (ids_ld = k + 3, scores_ld = k + 5, the scores one float off 16 B) with
    the exclusion lists, and into dense outputs without them: ids and scores equal to the stable-sort reference on
    kge_score_indexed_ex's matrix of the same views (scores bitwise); the fp64 checks (valid distinct ids, scores
    within the bar, nothing below the fp64 k-th best by more than twice the bar); (-1, -inf) rows where the list
    holds every entity; nothing written outside [B, k] or past the workspace; pad4 bitwise dense; refused layouts
    write nothing."""
    c = W.case(name, d)
    pos = c["pos"].to(DEV)
    reached, refused, dense = set(), set(), {}
    for layout in W.LAYOUTS:
        ent, rel = W.lay(c["ent"], c["rel"], layout, DEV)
        V, G, ok = W.expected(name, d, ent, rel)
        _, xptr, xids = _lists(name, d, mode)
        ptr, ids = W.filters(name, d, mode)
        ref = W.ref_scores(name, d, mode)
        Sc = W.score_matrix(c, mode, ent, rel, pos).cpu() if ok else None
        for k in W.KS:
            for padded, filtered in ((True, True), (False, False)):
                tag = (layout, mode, V, G, k, padded)
                args = (xptr, xids, xids.numel()) if filtered else (None, None, 0)
                rc, oi, osc, buf, intact = _topk_call(c, mode, ent, rel, pos, *args, k, padded)
                assert intact, (tag, "written outside [B, k] or the workspace's bytes")
                if not ok:
                    assert rc == W.ENOTSUP, (tag, rc, _last_error())
                    assert _refusal_names_the_width(_last_error(), d, V), (tag, _last_error())
                    assert bool((oi == W.CANARY64).all()) and bool((_bits(osc) == S.CANARY).all()), tag
                    assert bool((buf == 0xA5).all()), (tag, "a refused call wrote its workspace")
                    refused.add(layout)
                    continue
                assert rc == 0, (tag, rc, _last_error())
                reached.add((V, G))
                got = (oi.cpu(), osc.cpu())
                assert W.same_topk(got, _topk_ref(Sc, k, ptr, ids, filtered)), (tag, "same-view matrix")
                W.check_topk_fp64(ref, got[0], got[1], k, ptr if filtered else None, ids if filtered else None)
                if filtered:
                    assert bool((got[0][W.ROW_ALL] == -1).all()) and bool(torch.isneginf(got[1][W.ROW_ALL]).all()), tag
                    assert bool((got[0][W.ROW_LONG] >= 0).all()), tag
                else:
                    assert bool((got[0] >= 0).all()), tag
                if layout == "dense":
                    dense[(mode, k, padded)] = got
                if layout == "pad4":
                    assert W.same_topk(got, dense[(mode, k, padded)]), (tag, "pad4 != dense")
    want_refused = {lay for lay in W.LAYOUTS if not W.expected(name, d, *W.lay(c["ent"], c["rel"], lay))[2]}
    assert refused == want_refused
    print(f"top-k sweep {name} D={d} {W.MODES[mode][1]}: (V, G) reached {sorted(reached)}, refused layouts {sorted(refused)}")


# ------------------------------------------------------------------------------------------------
# through the Python layer
# ------------------------------------------------------------------------------------------------
PY_E, PY_R, PY_GAMMA = 700, 6, 9.0
PY_LAYOUTS = ("dense", "pad2", "pad1", "off1")


def _model(name, hidden, layout):
    """RotatE / InterHT with its tables replaced by views of a named layout, installed as parameters."""
    if name == "InterHT":
        m = kge.TFKGEModel(name, PY_E, PY_R, hidden, PY_GAMMA, True, False, True, device=DEV, seed=7)
    else:
        m = kge.KGEModel(name, PY_E, PY_R, hidden, PY_GAMMA, double_entity_embedding=True, device=DEV, seed=7)
    e0, r0 = m.entity_embedding.detach().cpu(), m.relation_embedding.detach().cpu()
    assert e0.shape == (PY_E, 2 * hidden) and r0.shape == (PY_R, S.MULT[name][1] * hidden)
    ent, rel = W.lay(e0, r0, layout, DEV)
    m.entity_embedding = torch.nn.Parameter(ent)
    m.relation_embedding = torch.nn.Parameter(rel)
    for p, v in ((m.entity_embedding, ent), (m.relation_embedding, rel)):
        assert p.stride() == v.stride() and p.data_ptr() == v.data_ptr()
    assert m._D == hidden and m._rel_off == S.rel_off(name, hidden)
    return m


@pytest.mark.parametrize("layout", PY_LAYOUTS)
@pytest.mark.parametrize("name,hidden", [("RotatE", 132), ("InterHT", 264)])
def test_python_layer_falls_back_where_the_sweep_is_refused(monkeypatch, name, hidden, layout):
    """rank_sweep / topk_sweep answer None exactly where the instance is refused (InterHT per-half 264 at V = 1);
    test_step (300 queries in batches of 128) gives the metrics of the matrix path on the same model, and predict
    the top-k of score_all + topk_rows."""
    m = _model(name, hidden, layout)
    V, G, ok = W.expected(name, hidden, m.entity_embedding, m.relation_embedding)
    want_vg = {("RotatE", "dense"): (4, 1), ("RotatE", "pad2"): (2, 2), ("RotatE", "pad1"): (1, 4),
               ("RotatE", "off1"): (1, 4), ("InterHT", "dense"): (4, 2), ("InterHT", "pad2"): (2, 4),
               ("InterHT", "pad1"): (1, 8), ("InterHT", "off1"): (1, 8)}[(name, layout)]
    assert (V, G) == want_vg and ok == (G <= 4)
    g = np.random.RandomState(3)
    true = np.stack([g.randint(PY_E, size=1500), g.randint(PY_R, size=1500), g.randint(PY_E, size=1500)], 1)
    true[300:500, :2] = true[0, :2]  # hub pairs: long filter and exclusion rows
    true[500:700, 1:] = true[1, 1:]
    q = true[:40]
    pos = _dev(q)
    for mode, col in (("head-batch", 0), ("tail-batch", 2)):
        ptr, ids = evaluate.build_filter(q, mode, true)
        truth = pos[:, col].contiguous()
        r = evaluate.rank_sweep(m, pos, mode, truth, _dev(ptr), _dev(ids))
        assert (r is not None) == ok, (mode, "rank_sweep")
        Sm = evaluate.score_all(m, pos, mode)
        if ok:
            assert torch.equal(r, evaluate.rank_filtered(Sm, truth, _dev(ptr), _dev(ids))), mode
        xp, xi = evaluate.build_exclude(q, mode, true)
        t = evaluate.topk_sweep(m, pos, mode, 10, _dev(xp), _dev(xi))
        assert (t is not None) == ok, (mode, "topk_sweep")
        if ok:
            assert W.same_topk(t, W.topk_reference(Sm, 10, xp, xi)), mode
    calls = []
    real = evaluate.rank_sweep

    def counted(*a, **kw):
        out = real(*a, **kw)
        calls.append(out is not None)
        return out

    monkeypatch.setattr(evaluate, "rank_sweep", counted)
    shipped = evaluate.test_step(m, true[:300], true, batch_size=128)
    assert len(calls) == 6 and all(x == ok for x in calls)
    with monkeypatch.context() as mp:
        mp.setattr(evaluate, "_sweep_rank_ok", lambda model: False)
        calls.clear()
        assert evaluate.test_step(m, true[:300], true, batch_size=128) == shipped
        assert not calls
    pq = true[:75]
    for mode in ("head-batch", "tail-batch"):
        got = evaluate.predict(m, pq, mode, k=10, known_triples=true, batch_size=32)
        xp, xi = evaluate.build_exclude(pq, mode, true)
        want = evaluate.topk_rows(evaluate.score_all(m, _dev(pq), mode), 10, _dev(xp), _dev(xi))
        assert W.same_topk(got, (want[0].cpu(), want[1].cpu())), (mode, "predict")
