"""kge_eval_rank_candidates / evaluate.rank_candidates / evaluate.test_step_candidates on the GPU: integer equality
with the composition the call replaces (kge_score_indexed's scores of [truth | candidates], counted on the host by
the header's rule) and with tests/candidate_cases.py's fp64 reference, at every kernel instance (V, G), list length,
list stride, table layout and edge row the header names."""
import numpy as np
import pytest
import torch

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import evaluate
from tests import candidate_cases as CC
from tests import strided as S
from tests import sweep_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
E = CC.E


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.int64)).to(DEV)  # a copy: the cases' arrays are read-only


def bits(t):
    return t.contiguous().view(torch.int32)


def fused(c, mode, ent, rel, pos, truth, cand, cand_ld, n_cand, fptr=None, fids=None, ties=True, ts=True):
    """(ranks, ties, truth scores) of one call into garbage-filled outputs, as CPU tensors."""
    M = pos.shape[0]
    r = torch.full((M,), SC.CANARY64, dtype=torch.int64, device=DEV)
    t = torch.full((M,), SC.CANARY64, dtype=torch.int64, device=DEV) if ties else None
    s = torch.full((M,), float("nan"), dtype=torch.float32, device=DEV) if ts else None
    nf = 0 if fptr is None else int(fptr[-1])
    rc = CC.rank_candidates_raw(c, mode, ent, rel, pos, truth, cand if n_cand else None, cand_ld, n_cand,
                                fptr if nf else None, fids if nf else None, nf, r, t, s)
    assert rc == 0, (rc, kge._lib.load().kge_last_error())
    return r.cpu(), None if t is None else t.cpu(), None if s is None else s.cpu()


def same(got, want):
    return torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(bits(got[2]), bits(want[2]))


@pytest.mark.parametrize("d", CC.WIDTHS)
@pytest.mark.parametrize("name", CC.FNS)
def test_equals_composition_and_fp64(name, d):
    """Six functions x twelve instances x both modes at M 40, C 500, filtered and unfiltered: ranks and ties equal
    the composition's and the fp64 reference's, the truth scores are bitwise the score matrix's column 0."""
    assert CC.dense_vg(name, d) == CC.VG[CC.WIDTHS.index(d)]
    for mode, _ in CC.MODES:
        c = CC.case(name, d, mode)
        ent, rel, pos = c["ent"].to(DEV), c["rel"].to(DEV), c["pos"].to(DEV)
        truth, _ = CC.truths(name, d, mode)
        tr, L = dev(truth), dev(CC.lists(name, d, mode))
        for filtered in (False, True):
            fptr, fids = (dev(x) for x in CC.filters(name, d, mode)) if filtered else (None, None)
            got = fused(c, mode, ent, rel, pos, tr, L, CC.C, CC.C, fptr, fids)
            want = CC.composition(c, mode, ent, rel, pos, tr, L, fptr, fids)
            assert same(got, want), (name, d, mode, filtered)
            ranks, ties, ts = CC.expected(name, d, mode, filtered)
            assert np.array_equal(got[0].numpy(), ranks), (name, d, mode, filtered)
            assert np.array_equal(got[1].numpy(), ties), (name, d, mode, filtered)
            ok = np.isfinite(ts)
            assert np.array_equal(np.isneginf(got[2].numpy()), ~ok)
            assert (np.abs(got[2].double().numpy()[ok] - ts[ok]) <= SC.bar(ts[ok])).all()
        assert got[1][list(CC.TIE_ROWS)].min() >= 1  # the planted ties are seen


LENGTHS = (0, 1, 63, 64, 65, 128, 129, 256, 257, 1000)  # around the 1 / 2 / 4 waves-per-row thresholds
SHAPE_WIDTHS = (16, 1000, 50, 450, 33, 255)  # two per vector width


def random_problem(g, M, n_cand, ld_kind):
    """Queries' truths (some out of range), lists with padding and repeats, a filter CSR for every other problem."""
    truth = g.randint(-1, E + 1, size=M).astype(np.int64)
    rows = 1 if ld_kind == 0 else M
    ld = 0 if ld_kind == 0 else n_cand + (3 if ld_kind == 2 else 0)
    buf = g.randint(-2, E + 2, size=(rows, max(ld, n_cand))).astype(np.int64)
    flt = [np.unique(g.randint(E, size=g.randint(0, 80))) for _ in range(M)]
    ptr = np.concatenate([[0], np.cumsum([len(f) for f in flt])]).astype(np.int64)
    return truth, buf, ld, ptr, np.concatenate(flt).astype(np.int64)


@pytest.mark.parametrize("d", SHAPE_WIDTHS)
def test_lengths_rows_and_list_strides(d):
    """C over the waves-per-row thresholds x M 1 / 37 (packed rows, a partial last block) x the three list strides
    (shared, dense, padded), against the composition."""
    name = CC.FNS[SHAPE_WIDTHS.index(d)]
    g = np.random.RandomState(d)
    for mode, _ in CC.MODES:
        c = CC.case(name, d, mode)
        ent, rel = c["ent"].to(DEV), c["rel"].to(DEV)
        for i, n_cand in enumerate(LENGTHS):
            for M in (1, 37):
                pos = c["pos"][:M].to(DEV).contiguous()
                for ld_kind in (0, 1, 2):
                    truth, buf, ld, ptr, ids = random_problem(g, M, n_cand, ld_kind)
                    tr, bd = dev(truth), dev(buf)
                    cand = bd[0, :n_cand] if ld_kind == 0 else bd[:, :n_cand]
                    fptr, fids = (dev(ptr), dev(ids)) if (i + M + ld_kind) % 2 else (None, None)
                    got = fused(c, mode, ent, rel, pos, tr, bd, ld, n_cand, fptr, fids)
                    want = CC.composition(c, mode, ent, rel, pos, tr, cand, fptr, fids)
                    assert same(got, want), (name, d, mode, n_cand, M, ld_kind)
                    if n_cand == 0:
                        assert (got[0] == 1).all() and (got[1] == 0).all()


@pytest.mark.parametrize("d", SHAPE_WIDTHS)
@pytest.mark.parametrize("name", CC.FNS)
def test_layouts_and_the_refused_widths(name, d):
    """Padded and offset table views (NaN in every padding element) at C 129, M 37, a padded list: the composition's
    results where kge_score_indexed accepts the view, KGE_ENOTSUP exactly where it refuses it."""
    g = np.random.RandomState(7 * d + CC.FNS.index(name))
    M, n_cand = 37, 129
    seen = set()
    for mode, _ in CC.MODES:
        c = CC.case(name, d, mode)
        pos = c["pos"][:M].to(DEV).contiguous()
        truth, buf, ld, ptr, ids = random_problem(g, M, n_cand, 2)
        tr, bd, fptr, fids = dev(truth), dev(buf), dev(ptr), dev(ids)
        cand = bd[:, :n_cand]
        for layout in CC.LAYOUTS:
            ent, rel = SC.lay(c["ent"], c["rel"], layout, DEV)
            V, G = S.table_vg(name, d, ent, rel)
            seen.add(G <= S.K_MAX_G)
            if G > S.K_MAX_G:
                out = torch.empty((M, n_cand), dtype=torch.float32, device=DEV)
                assert CC.score_indexed_rc(c, mode, ent, rel, pos, cand, out) == SC.ENOTSUP
                r = torch.zeros(M, dtype=torch.int64, device=DEV)
                assert CC.rank_candidates_raw(c, mode, ent, rel, pos, tr, bd, ld, n_cand, fptr, fids, len(ids), r,
                                              None, None) == SC.ENOTSUP
                assert (r == 0).all()
                continue
            got = fused(c, mode, ent, rel, pos, tr, bd, ld, n_cand, fptr, fids)
            want = CC.composition(c, mode, ent, rel, pos, tr, cand, fptr, fids)
            assert same(got, want), (name, d, mode, layout, V, G)
    assert True in seen and (d != 1000 or False in seen)  # d 1000: scalar rows are past the register-resident limit


@pytest.mark.parametrize("name,d", [("InterHT", 264), ("DistMult", 33), ("pRotatE", 450)])
def test_buffers_optional_outputs_and_determinism(name, d):
    mode = 0
    c = CC.case(name, d, mode)
    ent, rel, pos = c["ent"].to(DEV), c["rel"].to(DEV), c["pos"].to(DEV)
    truth, _ = CC.truths(name, d, mode)
    tr, L = dev(truth), dev(CC.lists(name, d, mode))
    fptr, fids = (dev(x) for x in CC.filters(name, d, mode))
    nf, M = len(fids), CC.B
    want = CC.composition(c, mode, ent, rel, pos, tr, L, fptr, fids)
    for k in (1, 3):  # outputs inside canary buffers, 8-B and 4-B aligned only
        r, t = SC.canary_i64(M, None, None, DEV, k), SC.canary_i64(M, None, None, DEV, k)
        s = S.canary(1, M, M, DEV, k=k)[0]
        before = [SC.outside(r), SC.outside(t), SC.outside(s)]
        assert CC.rank_candidates_raw(c, mode, ent, rel, pos, tr, L, CC.C, CC.C, fptr, fids, nf, r, t, s) == 0
        assert same((r.cpu(), t.cpu(), s.cpu()), want)
        for v, b in zip((r, t, s), before):
            assert torch.equal(SC.outside(v), b)
    # ties / truth_scores NULL: the same ranks; nothing depends on what the outputs held
    assert torch.equal(fused(c, mode, ent, rel, pos, tr, L, CC.C, CC.C, fptr, fids, ties=False, ts=False)[0], want[0])
    a = fused(c, mode, ent, rel, pos, tr, L, CC.C, CC.C, fptr, fids)
    b = fused(c, mode, ent, rel, pos, tr, L, CC.C, CC.C, fptr, fids)
    assert same(a, b) and same(a, want)


def test_python_wrapper_matches_the_raw_call():
    name, d, mode = "RotatE", 50, 1
    c = CC.case(name, d, mode)
    model = kge.KGEModel(name, E, CC.R, d, CC.GAMMA, double_entity_embedding=True, device=DEV, seed=0)
    with torch.no_grad():
        model.entity_embedding.copy_(c["ent"].to(DEV))
        model.relation_embedding.copy_(c["rel"].to(DEV))
    assert model._range_f == pytest.approx(c["rng"], rel=1e-6)
    pos = c["pos"].to(DEV)
    truth, _ = CC.truths(name, d, mode)
    tr, L = dev(truth), dev(CC.lists(name, d, mode))
    fptr, fids = (dev(x) for x in CC.filters(name, d, mode))
    ranks, ties, _ = CC.expected(name, d, mode, True)
    r, t = evaluate.rank_candidates(model, pos, "tail-batch", L, tr, fptr, fids, want_ties=True)
    assert np.array_equal(r.cpu().numpy(), ranks) and np.array_equal(t.cpu().numpy(), ties)
    r2 = evaluate.rank_candidates(model, pos, "tail-batch", L, tr, fptr, fids, nfilter=len(fids))
    assert torch.equal(r, r2)
    # one shared list, the default truth (the positive's tail)
    shared = L[CC.ROW_PAD].contiguous()
    r3, t3 = evaluate.rank_candidates(model, pos, "tail-batch", shared, want_ties=True)
    er, et, _ = CC.reference(CC.ref_scores(name, d, mode), c["pos"][:, 2].numpy(), shared.cpu().numpy())
    lo, hi = CC.bounds(CC.ref_scores(name, d, mode), c["pos"][:, 2].numpy(), shared.cpu().numpy())
    r3 = r3.cpu().numpy()
    assert ((lo <= r3) & (r3 <= hi)).all() and np.array_equal(r3[lo == hi], er[lo == hi])
    r4 = evaluate.rank_candidates(model, pos, "tail-batch", shared.unsqueeze(0).expand(CC.B, -1))
    assert np.array_equal(r4.cpu().numpy(), r3)


# ------------------------------------------------------------------------------------------------
# test_step_candidates
# ------------------------------------------------------------------------------------------------
TE, TR, TTRUE, TTEST = 300, 5, 1500, 70


def make_model(name, d=32, seed=5):
    if name == "InterHT":
        return kge.TFKGEModel(name, TE, TR, d, 9.0, True, False, True, device=DEV, seed=seed)
    if name == "TranSparse":
        return kge.TFKGEModel(name, TE, TR, 16, 9.0, device=DEV, seed=seed)
    return kge.KGEModel(name, TE, TR, d, 9.0, double_entity_embedding=name in ("RotatE", "ComplEx"),
                        double_relation_embedding=name == "ComplEx", device=DEV, seed=seed)


def triples(seed=3):
    g = np.random.RandomState(seed)
    true = np.stack([g.randint(TE, size=TTRUE), g.randint(TR, size=TTRUE), g.randint(TE, size=TTRUE)], 1).astype(np.int64)
    true[100:220, 0], true[100:220, 1] = true[0, 0], true[0, 1]  # a hub: long filter lists
    true[300:420, 2], true[300:420, 1] = true[1, 2], true[1, 1]
    return true, true[:TTEST]


@pytest.mark.parametrize("name", ["TransE", "RotatE", "pRotatE", "InterHT"])
def test_step_candidates_with_every_entity_is_test_step(name):
    """A shared list of all entities and the known triples: test_step's metrics exactly (both score every candidate
    with the fused scorer), in batches that do not divide the pass."""
    model = make_model(name)
    true, test = triples()
    every = torch.arange(TE, dtype=torch.int64, device=DEV)
    want = evaluate.test_step(model, test, true, batch_size=32)
    assert evaluate.test_step_candidates(model, test, every, every, known_triples=true, batch_size=32) == want
    table = evaluate.FilterTable(true, DEV)
    assert evaluate.test_step_candidates(model, test, every.cpu().numpy(), every, known_triples=table) == want
    tail_only = evaluate.test_step_candidates(model, test, None, every, known_triples=table)
    assert tail_only != want and set(tail_only) == set(want)


def model_case(model, name):
    return dict(name=name, D=model._D, gamma=model._gamma_f, rng=model._range_f, mod=0.0)


@pytest.mark.parametrize("name", ["DistMult", "ComplEx"])
def test_step_candidates_against_the_composition(name):
    """Per-triple lists with padding, filtered by the known triples: the metrics of the composition's ranks, and the
    three tie rules on planted ties (entity rows copied onto ids the lists hold)."""
    model = make_model(name)
    true, test = triples()
    g = np.random.RandomState(11)
    with torch.no_grad():  # each of the first 20 test triples' head and tail rows copied onto two other ids
        ent = model.entity_embedding
        for i in range(20):
            for col in (0, 2):
                ent[torch.from_numpy(g.randint(TE, size=2)).to(DEV)] = ent[int(test[i, col])].clone()
    lists = {m: g.randint(-1, TE, size=(TTEST, 200)).astype(np.int64) for m in ("head-batch", "tail-batch")}
    ent, rel = model.entity_embedding.detach(), model.relation_embedding.detach()
    pos, c = dev(test), model_case(model, name)
    above, tied = [], []
    for mode, mname in CC.MODES:
        ptr, ids = evaluate.build_filter(test, mname, true)
        tr = pos[:, 0 if mode == 0 else 2].contiguous()
        r, t, _ = CC.composition(c, mode, ent, rel, pos, tr, dev(lists[mname]), dev(ptr), dev(ids))
        above.append(r.numpy())
        tied.append(t.numpy())
    above, tied = np.concatenate(above), np.concatenate(tied)
    assert tied.sum() > 0 and (tied == 0).any()
    args = (model, test, lists["head-batch"], dev(lists["tail-batch"]))
    for rule, ranks in (("optimistic", above), ("pessimistic", above + tied), ("mean", above + tied / 2.0)):
        got = evaluate.test_step_candidates(*args, known_triples=true, batch_size=32, ties=rule)
        assert got == evaluate.metrics_from_ranks(ranks), rule
    assert evaluate.test_step_candidates(*args, known_triples=true) == evaluate.metrics_from_ranks(above)
    head_only = evaluate.test_step_candidates(model, test, lists["head-batch"], None, known_triples=true)
    assert head_only == evaluate.metrics_from_ranks(above[:TTEST])


def test_step_candidates_transparse():
    """No function id: model.score of [truth | candidates] ranked by rank_filtered; padding, a filter and the tie
    counts are refused."""
    model = make_model("TranSparse")
    true, test = triples()
    g = np.random.RandomState(13)
    lists = {m: g.randint(TE, size=(TTEST, 50)).astype(np.int64) for m in ("head-batch", "tail-batch")}
    pos = dev(test)
    ranks = []
    with torch.no_grad():
        for mname, col in (("head-batch", 0), ("tail-batch", 2)):
            both = torch.cat([pos[:, col:col + 1], dev(lists[mname])], 1).contiguous()
            s = model.score(mname, pos, both).detach().cpu().numpy()
            s = np.broadcast_to(s, both.shape)  # tail-batch: one column
            ranks.append(1 + (s[:, 1:] > s[:, :1]).sum(axis=1))
    got = evaluate.test_step_candidates(model, test, lists["head-batch"], lists["tail-batch"], batch_size=32)
    assert got == evaluate.metrics_from_ranks(np.concatenate(ranks))
    padded = lists["head-batch"].copy()
    padded[3, 7] = -1
    for kw in (dict(head_candidates=padded, tail_candidates=None),
               dict(head_candidates=lists["head-batch"], tail_candidates=None, known_triples=true),
               dict(head_candidates=lists["head-batch"], tail_candidates=None, ties="mean"),
               dict(head_candidates=None, tail_candidates=lists["tail-batch"], ties="pessimistic")):
        with pytest.raises(NotImplementedError, match="TranSparse"):
            evaluate.test_step_candidates(model, test, **kw)
    assert evaluate.rank_candidates(model, pos, "head-batch", dev(lists["head-batch"])) is None
