"""PairRE evaluation and model surface on the GPU: kge_eval_rank_sweep / kge_eval_rank_candidates ranks integer-equal
to the fp64 reference's (tests/pairre_cases.py: truths no score within the bar can move), kge_eval_topk_sweep by
tests/sweep_cases.py's top-k check, the score-matrix fall-back past the sweeps' width, and the two model classes."""
import types

import numpy as np
import pytest
import torch

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import _lib as L
from customknowledgegraphembedding_amd import evaluate as EV
from customknowledgegraphembedding_amd.optim import Adam
from tests import pairre_cases as PC
from tests import pairre_ref as P
from tests import sweep_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR = 1e-3


def _model(c, cls=kge.TFKGEModel):
    """A model holding the tables of an evaluation case."""
    m = cls("PairRE", c["E"], c["R"], c["D"], PC.GAMMA, double_relation_embedding=True, device=DEV, seed=0)
    with torch.no_grad():
        m.entity_embedding.copy_(c["ent"])
        m.relation_embedding.copy_(c["rel"])
    return m


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


# ------------------------------------------------------------------------------------------------
# 5. evaluation
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 33, 264, 1000])
def test_rank_sweep_and_rank_candidates(D):
    c, lib = PC.eval_case(D), L.load()
    ent, rel, pos = c["ent"].to(DEV), c["rel"].to(DEV), c["pos"].to(DEV)
    m = _model(c)
    for mode, mname in PC.MODES:
        truth, _ = PC.truths(D, mode)
        ptr, ids = PC.filters(D, mode)
        for filtered in (False, True):
            nf = int(ptr[-1]) if filtered else 0
            ws = torch.empty(lib.kge_eval_rank_sweep_workspace_size(PC.B_EVAL, nf), dtype=torch.uint8, device=DEV)
            ranks = torch.zeros(PC.B_EVAL, dtype=torch.int64, device=DEV)
            rc = W.rank_sweep_raw(c, mode, ent, rel, pos, _dev(truth), _dev(ptr) if filtered else None,
                                  _dev(ids) if filtered else None, nf, ranks, ws)
            assert rc == 0, lib.kge_last_error()
            assert torch.equal(ranks.cpu(), PC.expected_ranks(D, mode, filtered)), (D, mode, filtered)
        got = EV.rank_sweep(m, pos, mname, _dev(truth), _dev(ptr), _dev(ids))
        assert torch.equal(got.cpu(), PC.expected_ranks(D, mode, True)), (D, mode, "evaluate.rank_sweep")
        lists, want_ranks, want_ties = PC.candidate_lists(D, mode)
        r, t = EV.rank_candidates(m, pos, mname, _dev(lists), _dev(truth), _dev(ptr), _dev(ids), want_ties=True)
        assert np.array_equal(r.cpu().numpy(), want_ranks) and np.array_equal(t.cpu().numpy(), want_ties), (D, mode)


@pytest.mark.parametrize("D", [16, 33, 264, 1000])
def test_topk_sweep(D):
    c = PC.eval_case(D)
    m, pos = _model(c), c["pos"].to(DEV)
    for mode, mname in PC.MODES:
        ref = PC.ref_scores(D, mode)
        ptr, ids = PC.filters(D, mode)
        for k in W.KS:
            gi, gs = EV.topk_sweep(m, pos, mname, k)
            W.check_topk_fp64(ref, gi, gs, k)
            gi, gs = EV.topk_sweep(m, pos, mname, k, _dev(ptr), _dev(ids))
            W.check_topk_fp64(ref, gi, gs, k, ptr, ids)


def test_d1500_sweeps_refuse_and_the_fall_back_answers():
    D = 1500
    c, lib = PC.eval_case(D), L.load()
    m, pos = _model(c), c["pos"].to(DEV)
    ent, rel = m.entity_embedding.detach(), m.relation_embedding.detach()
    truth, _ = PC.truths(D, 1)
    ws = torch.empty(lib.kge_eval_rank_sweep_workspace_size(PC.B_EVAL, 0), dtype=torch.uint8, device=DEV)
    ranks = torch.zeros(PC.B_EVAL, dtype=torch.int64, device=DEV)
    assert W.rank_sweep_raw(c, 1, ent, rel, pos, _dev(truth), None, None, 0, ranks, ws) == W.ENOTSUP
    assert EV.rank_sweep(m, pos, "tail-batch", _dev(truth)) is None
    assert EV.topk_sweep(m, pos, "tail-batch", 10) is None
    # evaluate.test_step through score_all + rank_filtered: every metric inside what the fp64 scores allow
    triples = c["pos"].numpy()
    got = EV.test_step(m, triples, triples)
    lo, hi = [], []
    for mode, mname in PC.MODES:
        ptr, ids = EV.build_filter(triples, mname, triples)
        a, b = W.rank_bounds(PC.ref_scores(D, mode), triples[:, 0 if mode == 0 else 2], ptr, ids)
        lo.append(a)
        hi.append(b)
    lo, hi = np.concatenate(lo).astype(np.float64), np.concatenate(hi).astype(np.float64)
    assert lo.mean() - 1e-9 <= got["MR"] <= hi.mean() + 1e-9, (got, lo.mean(), hi.mean())
    assert (1 / hi).mean() - 1e-9 <= got["MRR"] <= (1 / lo).mean() + 1e-9
    for mode, mname in PC.MODES:
        gi, gs = EV.predict(m, triples, mname, k=10)
        W.check_topk_fp64(PC.ref_scores(D, mode), gi, gs, 10)


def test_test_step_candidates_mean_ties():
    D = 33
    c = PC.eval_case(D)
    m = _model(c)
    triples = c["pos"].numpy().copy()
    want = []
    cands = {}
    for mode, mname in PC.MODES:
        truth, _ = PC.truths(D, mode)
        inside = (truth >= 0) & (truth < PC.E_EVAL)
        triples[inside, 0 if mode == 0 else 2] = truth[inside]
    for mode, mname in PC.MODES:
        # the positives of this pass: the in-range truths of BOTH modes are set, so the fp64 scores are recomputed
        ref = P.score_all(c["ent"].double(), c["rel"].double(), torch.from_numpy(triples), mode, PC.GAMMA).numpy()
        col = 0 if mode == 0 else 2
        b = PC.bar(ref)
        g = np.random.RandomState(5 + mode)
        lists = np.empty((PC.B_EVAL, 60), dtype=np.int64)
        for q in range(PC.B_EVAL):
            tr = triples[q, col]
            far = np.abs(ref[q] - ref[q, tr]) > 2.0 * (b[q] + b[q, tr])
            far[tr] = False
            lists[q] = g.choice(np.nonzero(far)[0], size=60, replace=True)
            lists[q, 0], lists[q, 1] = tr, -1  # the truth itself and padding: not counted
            counted = lists[q, 2:]
            want.append(1.0 + float((ref[q, counted] > ref[q, tr]).sum()))
        cands[mname] = torch.from_numpy(lists)
    got = EV.test_step_candidates(m, triples, cands["head-batch"], cands["tail-batch"], ties="mean")
    assert got == EV.metrics_from_ranks(np.array(want))


# ------------------------------------------------------------------------------------------------
# 6. models
# ------------------------------------------------------------------------------------------------
def _args():
    return types.SimpleNamespace(negative_adversarial_sampling=True, adversarial_temperature=0.5, uni_weight=False,
                                 regularization=0.0)


def _batches(E, R, B, N, steps):
    g = np.random.RandomState(9)
    for i in range(steps):
        pos = torch.from_numpy(np.stack([g.randint(E, size=B), g.randint(R, size=B), g.randint(E, size=B)], 1))
        neg = torch.from_numpy(g.randint(E, size=(B, N)))
        w = torch.from_numpy(g.uniform(0.1, 1.0, size=(B,))).float()
        yield pos, neg, w, ("head-batch", "tail-batch")[i % 2]


def test_kgemodel_train_step_twins():
    """train_step (autograd: kge_step_forward + kge_step_backward + Adam), train_step_fused (kge_train_step_reg) and
    the same with Adam(lazy=True) (kge_train_step_lazy) on models holding the same tables. The two dense rules are
    held together over four steps. The lazy rule is held to them after the first step, where it is the same update:
    from zero moments a row the batch did not touch has zero gradient and zero moments under the dense rule too
    (later a dense Adam keeps moving a row on its momentum, a lazy one does not)."""
    E, R, D, B, N, steps = 120, 6, 24, 10, 17, 4
    ms = [kge.KGEModel("PairRE", E, R, D, 9.0, double_relation_embedding=True, device=DEV, seed=4) for _ in range(3)]
    for m in ms:
        with torch.no_grad():
            m.relation_embedding.div_(m._range_f)  # relation rows of U(-1, 1)
    opts = [Adam(ms[0].parameters(), lr=LR), Adam(ms[1].parameters(), lr=LR),
            Adam(ms[2].parameters(), lr=LR, lazy=True)]
    its = [_batches(E, R, B, N, steps) for _ in ms]

    def same_tables(a, b):
        for x, y in zip(a.parameters(), b.parameters()):
            assert float((x.detach() - y.detach()).abs().max()) <= 5e-2 * LR

    def same_log(got, want, t):
        for k in ("loss", "positive_sample_loss", "negative_sample_loss"):
            assert abs(got[k] - want[k]) <= 1e-4 * max(1.0, abs(want[k])), (t, k, got, want)

    for t in range(steps):
        la = kge.KGEModel.train_step(ms[0], opts[0], its[0], _args())
        same_log(kge.KGEModel.train_step_fused(ms[1], opts[1], its[1], _args()), la, t)
        lc = kge.KGEModel.train_step_fused(ms[2], opts[2], its[2], _args())  # every step runs; the first is compared
        if t == 0:
            same_log(lc, la, t)
            same_tables(ms[0], ms[2])
        assert np.isfinite(lc["loss"])
    same_tables(ms[0], ms[1])


@pytest.mark.parametrize("D", [24, 1000])
def test_tfkgemodel_forward(D):
    c = PC.case(D, 97, 5, 6, 20, seed=D + 2)
    m = _model(dict(E=97, R=5, D=D, ent=c.ent, rel=c.rel))
    pos, neg = c.pos.to(DEV), c.neg.to(DEV)
    for mode in (0, 1, 3):
        got = m(((pos, neg), mode)).detach().cpu().numpy()
        n, p, _, _ = P.reduced(c.ent.double(), c.rel.double(), c.pos, c.neg, 1 if mode == 3 else mode, c.gamma, "tf")
        want = (p if mode == 3 else n).numpy().reshape(-1, 1)
        assert got.shape == want.shape and PC.within_bar(got, want), (D, mode)


@pytest.mark.parametrize("D", [24, 1000])
def test_model_func_on_gathered_rows_with_autograd(D):
    c = PC.case(D, 97, 5, 6, 20, seed=D + 4)
    m = _model(dict(E=97, R=5, D=D, ent=c.ent, rel=c.rel))
    f = m.model_func["PairRE"]
    g = torch.Generator().manual_seed(D)
    for mode in (0, 1, 3):
        h1, t1 = c.ent[c.pos[:, 0]].unsqueeze(1), c.ent[c.pos[:, 2]].unsqueeze(1)
        r1, cand = c.rel[c.pos[:, 1]].unsqueeze(1), c.ent[c.neg]
        head, tail = (cand if mode == 0 else h1), (cand if mode == 1 else t1)
        ds = torch.randn(6, 1 if mode == 3 else 20, generator=g)
        ref_in = [t.double().requires_grad_(True) for t in (head, r1, tail)]
        ref = P.score_rows(*ref_in, c.gamma)
        (ref * ds.double()).sum().backward()
        got_in = [t.clone().to(DEV).requires_grad_(True) for t in (head, r1, tail)]
        got = f(got_in[0], got_in[1], got_in[2], mode)
        assert PC.within_bar(got.detach().cpu().numpy(), ref.detach().numpy()), (D, mode)
        (got * ds.to(DEV)).sum().backward()
        for a, b, what in zip(got_in, ref_in, ("head", "relation", "tail")):
            err = float((a.grad.cpu().double() - b.grad).abs().max())
            assert err <= 1e-4 * float(b.grad.abs().max()), (D, mode, what, err)
