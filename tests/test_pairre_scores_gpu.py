"""PairRE forward on the GPU against the fp64 reference (tests/pairre_ref.py): kge_score_indexed and kge_score_dense
at every (vector width, register depth) class and row layout, out-of-range ids as zero rows; and kge_step_forward's
three candidate orders and the planned step, bitwise equal to one another and within the bar of fp64."""
import pytest
import torch

from customknowledgegraphembedding_amd import ops
from customknowledgegraphembedding_amd._lib import KGEHipError
from tests import pairre_cases as PC
from tests import pairre_ref as P
from tests import strided as S
from tests import sweep_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FN = PC.FN
# per-row widths reaching every (V in 4, 2, 1; G) class over the layouts, G > 4 (1500, 2048; 264 and 1000 on narrow
# layouts) included
WIDTHS = (16, 50, 33, 130, 264, 1000, 1500, 2048)
LAYOUTS = ("dense", "pad1", "pad2", "off1", "off2", "rel_pad2")
E, R, B, N = 97, 5, 4, 16


def _ref(c, mode):
    return P.score(c.ent.double(), c.rel.double(), c.pos, c.neg, mode, c.gamma).numpy()


@pytest.mark.parametrize("D", WIDTHS)
def test_score_indexed_every_layout(D):
    c = PC.case(D, E, R, B, N, seed=D, oor=True)
    pos, neg = c.pos.to(DEV), c.neg.to(DEV)
    refs = {mode: _ref(c, mode) for mode in (0, 1, 3)}
    seen = set()
    for layout in LAYOUTS:
        ent, rel = W.lay(c.ent, c.rel, layout, DEV)
        V, G = S.table_vg(PC.NAME, D, ent, rel)
        seen.add((V, min(G, 16)))
        for mode in (0, 1, 3):
            call = lambda: ops.score_indexed_raw(FN, mode, ent, rel, 0, pos, None if mode == 3 else neg, D, c.gamma,
                                                 c.rng)
            if G > S.K_MAX_G:  # past the register-resident limit at this vector width: refused, as every function
                with pytest.raises(KGEHipError, match="exceeds"):
                    call()
                continue
            got = call().cpu().numpy()
            assert PC.within_bar(got, refs[mode]), (D, layout, mode, V, G)
    assert len({v for v, _ in seen}) == (3 if D % 4 == 0 else (2 if D % 2 == 0 else 1))


@pytest.mark.parametrize("D", WIDTHS)
def test_score_dense(D):
    c = PC.case(D, E, R, B, N, seed=D, oor=True)
    ent, rel = c.ent, c.rel
    h1, t1 = P.rows(ent, c.pos[:, 0]).unsqueeze(1), P.rows(ent, c.pos[:, 2]).unsqueeze(1)
    r1 = P.rows(rel, c.pos[:, 1]).unsqueeze(1)
    cand = P.rows(ent, c.neg)
    for mode, head, tail in ((0, cand, t1), (1, h1, cand), (3, h1, t1)):
        got = ops.score_dense_raw(FN, mode, head.to(DEV), r1.to(DEV), tail.to(DEV), 0, D, c.gamma, c.rng)
        assert PC.within_bar(got.cpu().numpy(), _ref(c, mode)), (D, mode)


def test_out_of_range_ids_score_as_the_zero_row():
    D = 50
    c = PC.case(D, E, R, B, N, seed=D, oor=True)
    z = torch.cat([c.ent, torch.zeros(1, D)])  # row E: the zero row
    fix = lambda ids: torch.where((ids < 0) | (ids >= E), torch.full_like(ids, E), ids)
    pos2 = c.pos.clone()
    pos2[:, 0], pos2[:, 2] = fix(c.pos[:, 0]), fix(c.pos[:, 2])
    for mode in (0, 1, 3):
        a = ops.score_indexed_raw(FN, mode, c.ent.to(DEV), c.rel.to(DEV), 0, c.pos.to(DEV),
                                  None if mode == 3 else c.neg.to(DEV), D, c.gamma, c.rng)
        b = ops.score_indexed_raw(FN, mode, z.to(DEV), c.rel.to(DEV), 0, pos2.to(DEV),
                                  None if mode == 3 else fix(c.neg).to(DEV), D, c.gamma, c.rng)
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), mode


# ------------------------------------------------------------------------------------------------
# the forms of the step forward
# ------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("D", [128, 1000])
def test_step_forward_forms_bitwise_and_against_fp64(D):
    Ef, Bf, Nf = 523, 40, 128
    c = PC.case(D, Ef, 7, Bf, Nf, seed=D + 1, oor=True)
    ent, rel, pos, neg = c.ent.to(DEV), c.rel.to(DEV), c.pos.to(DEV), c.neg.to(DEV)
    want = {}
    for mode in (0, 1):
        run = lambda order, rows=None: ops.step_forward_raw(FN, mode, ent, rel, 0, pos, neg, D, c.gamma, c.rng,
                                                            forms=dict(step_order=order, tile_rows=rows))
        row = run("row")
        assert _same(run("xcd"), row), (D, mode, "xcd")
        for rows in (None, 3):
            assert _same(run("tile", rows), row), (D, mode, "tile", rows)
        for order in ("row", "xcd", "tile"):
            s = ops.score_indexed_raw(FN, mode, ent, rel, 0, pos, neg, D, c.gamma, c.rng,
                                      forms=dict(step_order=order))
            assert _same((s,), (row[2],)), (D, mode, "score", order)
        n, p, s, ps = P.reduced(c.ent.double(), c.rel.double(), c.pos, c.neg, mode, c.gamma, "tf")
        out_neg, out_pos, ns, pss = (t.cpu().numpy() for t in row)
        assert PC.within_bar(ns, s.numpy()) and PC.within_bar(pss, ps.numpy()), (D, mode)
        assert PC.within_bar(out_neg, n.numpy()) and PC.within_bar(out_pos, p.numpy()), (D, mode)
        want[mode] = row
    # the planned step over four alternating-direction steps (its sweep alternates by default)
    assert ops.StepPlanner.available(FN, ent, rel, 0, D, Bf, Nf)
    sp = ops.StepPlanner(FN, ent, rel, 0, D, Bf, Nf, c.gamma, c.rng)
    modes = (1, 0, 1, 0)
    sp.plan(pos, neg, modes[0])
    for i, mode in enumerate(modes):
        out = sp.step(nxt=(pos, neg, modes[i + 1]) if i + 1 < len(modes) else None)
        torch.cuda.synchronize()
        assert _same(out, want[mode]), (D, i, mode)
    f = sp.form()
    assert f["rows"] == 16 and f["throttle"] == 0  # the library defaults: 16 rows, no board
