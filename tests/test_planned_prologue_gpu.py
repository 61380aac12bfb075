"""The planned instances of step_fwd_tile_kernel (kge_step_forward_planned, ops.StepPlanner): their prologue takes
the rows, ids and first list entries straight from the plan (two global round trips and one barrier: each wave
reads the plan rows it builds, ranks InterHT's relation runs itself and fills the runs' LDS slots with the
query loads in flight), and the lead throttle is a template flag (an instance without a board holds none of its
instructions). None of this may change a score: every case runs at least three consecutive planner steps (both
sweep directions; the later plans made in the step before's tail blocks), modes mixed, and compares all four
outputs BITWISE (NaN equal to NaN) with ops.step_forward_raw. Reference: supervisor.py:17-18, model.py:114-205."""
import pytest
import torch

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import ops
from customknowledgegraphembedding_amd._lib import FN_IDS

pytestmark = pytest.mark.gpu
DEV = "cuda"
FNS = ["TransE", "DistMult", "ComplEx", "RotatE", "pRotatE", "InterHT"]
MODES4 = [0, 1, 1, 0]


def _model(name, E, R, d, seed=0, gamma=12.0):
    return kge.TFKGEModel(name, E, R, d, gamma, double_entity_embedding=name in ("ComplEx", "RotatE", "InterHT"),
                          double_relation_embedding=name == "ComplEx", triple_relation_embedding=name == "InterHT",
                          device=DEV, seed=seed)


def _mod(m):
    return float(m.modulus.detach().reshape(-1)[0]) if m.model_name == "pRotatE" else 0.0


def _batches(E, R, B, N, n, seed, hi=None):
    g = torch.Generator().manual_seed(seed)
    hi = hi or E
    out = []
    for _ in range(n):
        pos = torch.stack([torch.randint(0, E, (B,), generator=g), torch.randint(0, R, (B,), generator=g),
                           torch.randint(0, hi, (B,), generator=g)], 1)
        neg = torch.randint(0, hi, (B, N), generator=g)
        out.append((pos.to(DEV), neg.to(DEV)))
    return out


def _unplanned(m, mode, pos, neg):
    return ops.step_forward_raw(FN_IDS[m.model_name], mode, m.entity_embedding.detach(),
                                m.relation_embedding.detach(), m._rel_off, pos, neg, m._D, m._gamma_f, m._range_f,
                                modulus=_mod(m))


def _planner(m, B, N):
    return ops.StepPlanner(FN_IDS[m.model_name], m.entity_embedding.detach(), m.relation_embedding.detach(),
                           m._rel_off, m._D, B, N, m._gamma_f, m._range_f, modulus=_mod(m))


def _same(a, b):
    """Bitwise equal, NaN where the other is NaN (a zero query row gives NaN: no epsilon, Q7)."""
    return all(bool(((x == y) | (torch.isnan(x) & torch.isnan(y))).all()) for x, y in zip(a, b))


def _chain(sp, bs, modes):
    """plan(batch 0), then step i with batch i + 1 planned in its tail; every step's outputs (cloned)."""
    sp.plan(bs[0][0], bs[0][1], modes[0])
    outs = []
    for i in range(len(bs)):
        nxt = (bs[i + 1][0], bs[i + 1][1], modes[i + 1]) if i + 1 < len(bs) else None
        outs.append([t.clone() for t in sp.step(nxt=nxt)])
    torch.cuda.synchronize()
    return outs


def _reference(m, bs, modes):
    ref = [[t.clone() for t in _unplanned(m, md, p, n)] for md, (p, n) in zip(modes, bs)]
    torch.cuda.synchronize()
    return ref


def _check(m, bs, modes, what):
    assert len(bs) >= 3
    B, N = bs[0][1].shape
    got = _chain(_planner(m, B, N), bs, modes)
    ref = _reference(m, bs, modes)
    for i in range(len(bs)):
        assert _same(got[i], ref[i]), (what, i)


@pytest.mark.parametrize("d", [96, 50, 33])  # V4, V2, V1
@pytest.mark.parametrize("name", FNS)
def test_every_function_and_vector_width(name, d):
    E, R, B, N = 3001, 7, 37, 200
    _check(_model(name, E, R, d), _batches(E, R, B, N, 4, seed=d), MODES4, (name, d))


@pytest.mark.parametrize("name", ["InterHT", "RotatE"])
def test_wide_rows_flagship_instance(name):
    """d 1000 (8 KB rows: G 4, 12 waves; two rows of a group share a wave, so both of a wave's row slots run)."""
    E, R, d, B, N = 600, 7, 1000, 20, 130
    _check(_model(name, E, R, d, gamma=24.0), _batches(E, R, B, N, 4, seed=2), MODES4, name)


@pytest.mark.parametrize("name", ["InterHT", "DistMult"])
@pytest.mark.parametrize("B,N,hi", [(33, 200, 300), (5, 1, 300), (1, 1, 300), (5, 1, None), (1, 1, None)])
def test_empty_and_short_slice_lists(name, B, N, hi):
    """Every candidate and tail below 300 of 4 000 entities: slices 1-7 hold no item. B 5 / B 1 with N 1: fewer
    items than waves (a wave's first list entries lie past the block's segment) and a single row."""
    E, R, d = 4000, 5, 64
    _check(_model(name, E, R, d, seed=1), _batches(E, R, B, N, 4, seed=B + N, hi=hi), MODES4, (name, B, N, hi))


def test_interht_relation_runs():
    """More runs than LDS slots (R 300 over 40 rows), relation ids -1 and R among the rows, and groups whose rows
    all share one relation."""
    E, R, d, B, N = 2500, 300, 32, 40, 140
    m = _model("InterHT", E, R, d)
    bs = _batches(E, R, B, N, 4, seed=7)
    bs[1][0][3, 1] = -1
    bs[1][0][17, 1] = R
    bs[1][0][18, 1] = R
    bs[2][0][:, 1] = 5           # one relation in every group
    bs[3][0][:20, 1] = 9         # one group of one relation, the others mixed
    bs[3][0][39, 1] = -1
    _check(m, bs, MODES4, "runs")
    # wide rows: few slots (the relation thirds compete with the rows' images for LDS)
    E, R, d, B, N = 600, 40, 1000, 20, 130
    _check(_model("InterHT", E, R, d, gamma=24.0), _batches(E, R, B, N, 3, seed=8), [1, 0, 1], "wide runs")


@pytest.mark.parametrize("name", FNS)
def test_head_batch_positives_with_out_of_range_ids(name):
    """The head-batch positives' own (h, r) query and tail row: tails at -2, E + 3 and E - 1, a head at -2, a
    relation at R + 1, two rows of one group with the same tail; every batch in both modes."""
    E, R, d, B, N = 3001, 7, 96, 37, 200
    m = _model(name, E, R, d, seed=3)
    bs = _batches(E, R, B, N, 2, seed=5)
    for pos, neg in bs:
        neg[0, :5] = torch.tensor([-1, E, E + 7, -100, 0], device=DEV)
        pos[0, 2] = -2
        pos[1, 2] = E + 3
        pos[6, 2] = E - 1
        pos[2, 0] = -2
        pos[3, 1] = R + 1
        pos[4, 1] = pos[5, 1] = 0  # (InterHT ranks its rows by relation: the same group)
        pos[4, 2] = pos[5, 2] = 77
    bs = [bs[0], bs[1], bs[0], bs[1]]
    _check(m, bs, [0, 0, 1, 1], name)


@pytest.mark.parametrize("name", ["InterHT", "DistMult"])
def test_board_and_no_board_instances_agree(name):
    """The same batches through the instances with and without the lead throttle, at three sweep forms: all six
    settings give the unplanned step's outputs."""
    E, R, d, B, N = (600, 7, 1000, 20, 130) if name == "InterHT" else (3001, 7, 64, 37, 200)
    m = _model(name, E, R, d, gamma=24.0)
    bs = _batches(E, R, B, N, 4, seed=11)
    bs[1][1][0, :4] = torch.tensor([-1, E, E + 7, 0], device=DEV)
    bs[1][0][1, 2] = E + 3
    ref = _reference(m, bs, MODES4)
    for waves, depth in ((12, 2), (12, 1), (16, 2)):
        for lead in (0, 12):
            sp = _planner(m, B, N)
            sp.set_form(waves, depth)
            sp.set_lead(lead)
            f = sp.form()
            assert (f["waves"], f["depth"], f["lead"], f["throttle"]) == (waves, depth, lead, 1 if lead else 0), f
            got = _chain(sp, bs, MODES4)
            for i in range(len(bs)):
                assert _same(got[i], ref[i]), (name, waves, depth, lead, i)
