"""Rows per group of a planned step (kge_step_planner_set_rows, the planner's row rule). A planner whose
steps also make the next plan may take more than the library's 16 rows per group, so that the scoring grid leaves
compute units free and 8 plan blocks make the next plan beside the sweep (the default for InterHT and RotatE rows of
4 KB or more, where it measured faster; opt-in elsewhere), and a planned instance sizes its LDS without the unplanned
form's list region (more InterHT relation slots). Neither may change a score: every case compares all four outputs of
consecutive planner steps BITWISE (NaN equal to NaN) with ops.step_forward_raw (reference: supervisor.py:17-18,
model.py:114-205). The row rule itself is checked on the host against hand-computed layouts (no GPU).

Not covered: more relation runs in a group than relation slots at d 24, 33 and 300. A slot costs one image there
(256 B to 1.2 KB), so a planned block always has one per row and the overflow path (the relation third read from the
table per candidate) runs only at d 1000 (1, 5 or 7 slots for up to 19 rows of up to 19 relations); the planner
has no setter that caps the slots."""
import ctypes

import pytest
import torch

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import _lib, ops
from customknowledgegraphembedding_amd._lib import FN_IDS

DEV = "cuda"
MODES4 = [0, 1, 1, 0]


def _model(name, E, R, d, seed=0, gamma=12.0):
    return kge.TFKGEModel(name, E, R, d, gamma, double_entity_embedding=name in ("ComplEx", "RotatE", "InterHT"),
                          double_relation_embedding=name == "ComplEx", triple_relation_embedding=name == "InterHT",
                          device=DEV, seed=seed)


def _batches(E, R, B, N, n, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        pos = torch.stack([torch.randint(0, E, (B,), generator=g), torch.randint(0, R, (B,), generator=g),
                           torch.randint(0, E, (B,), generator=g)], 1)
        neg = torch.randint(0, E, (B, N), generator=g)
        out.append((pos.to(DEV), neg.to(DEV)))
    return out


def _unplanned(m, mode, pos, neg):
    return ops.step_forward_raw(FN_IDS[m.model_name], mode, m.entity_embedding.detach(),
                                m.relation_embedding.detach(), m._rel_off, pos, neg, m._D, m._gamma_f, m._range_f)


def _planner(m, B, N):
    return ops.StepPlanner(FN_IDS[m.model_name], m.entity_embedding.detach(), m.relation_embedding.detach(),
                           m._rel_off, m._D, B, N, m._gamma_f, m._range_f)


def _same(a, b):
    return all(bool(((x == y) | (torch.isnan(x) & torch.isnan(y))).all()) for x, y in zip(a, b))


def _chain(sp, bs, modes):
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


# (function, d, relations, the most rows a block holds): d 1000 is G 4 at 12 waves, where 19 rows of two 4 KB images
# are the last that fit 160 KB (InterHT then has 1 relation slot, 5 at 17 rows, 7 at 16, and a group of 16 or more of
# the 40 relations' rows has more runs than that); the narrow widths (V 4 / V 1 / V 4 G 2) run 16 waves, whose wave 0
# .. 3 then build a second row
CASES = [("InterHT", 1000, 40, 19), ("InterHT", 24, 40, 20), ("InterHT", 33, 40, 20), ("InterHT", 300, 40, 20),
         ("RotatE", 1000, 7, 19), ("DistMult", 500, 7, 20)]


@pytest.mark.gpu
@pytest.mark.parametrize("N", [128, 129])
@pytest.mark.parametrize("name,d,nrel,rmax", CASES)
def test_forced_rows_match_unplanned_step(name, d, nrel, rmax, N):
    """R forced to 16, 17 and the most that fit; B below one group, exactly one group, a multiple of R, and a last
    group of one row; four steps in modes 0 1 1 0 with the sweep's direction alternating (both directions in both
    modes' neighbourhood), then the same with the lead throttle's board instance and an always-ascending sweep."""
    E = 400
    m = _model(name, E, nrel, d, seed=1, gamma=24.0)
    for R in (16, 17, rmax):
        for B in (R - 3, R, 2 * R, 2 * R + 1):
            bs = _batches(E, nrel, B, N, 4, seed=R * 100 + B)
            ref = _reference(m, bs, MODES4)
            for lead, alternate in ((0, 1), (12, 0)):
                sp = _planner(m, B, N)
                sp.set_rows(R)
                sp.set_lead(lead)
                sp.set_sweep(alternate)
                got = _chain(sp, bs, MODES4)
                f = sp.form()
                assert f["rows"] == R and f["throttle"] == (1 if lead else 0), f
                for i in range(4):
                    assert _same(got[i], ref[i]), (name, d, N, R, B, lead, i)


@pytest.mark.gpu
def test_twelve_waves_one_row_in_flight_and_too_many_rows():
    """The 12 x 1 instance (RotatE's default at wide rows) at narrow rows and 20 rows per group; 8 waves build at most
    two rows each: 17 rows are refused there, and a planner at 17 rows refuses 8 waves."""
    E, nrel, d, B, N = 400, 7, 64, 41, 129
    m = _model("RotatE", E, nrel, d, seed=2)
    bs = _batches(E, nrel, B, N, 3, seed=5)
    ref = _reference(m, bs, [1, 0, 1])
    sp = _planner(m, B, N)
    sp.set_form(12, 1)
    sp.set_rows(20)
    got = _chain(sp, bs, [1, 0, 1])
    for i in range(3):
        assert _same(got[i], ref[i]), i
    with pytest.raises(_lib.KGEHipError):
        sp.set_form(8, 2)
    sp8 = _planner(m, B, N)
    sp8.set_form(8, 2)
    with pytest.raises(_lib.KGEHipError):
        sp8.set_rows(17)
    with pytest.raises(_lib.KGEHipError):
        sp8.set_rows(21)
    with pytest.raises(_lib.KGEHipError):
        sp8.set_rows(-2)
    assert sp8.form()["rows"] == 0  # a refused call changes nothing
    sp8.set_rows(16)
    got = _chain(sp8, bs, [1, 0, 1])
    for i in range(3):
        assert _same(got[i], ref[i]), i


@pytest.mark.gpu
def test_default_and_rule_rows_on_this_device():
    """What a planner chooses here by default (set_rows(0)) and when asked for the row rule (set_rows(-1)) is one of
    the counts the rule may choose, the plan buffers hold it, and the steps are the unplanned step's: B 512 at 16
    rows is 256 scoring blocks (a device of 256 CUs is full: 17 rows), B 64 and B 200 are not. Where the grid leaves
    CUs free, 8 plan blocks share the next plan's groups (B 512: 31 groups, four each; B 200: 13, two or one each;
    B 64: 4 groups, 4 blocks), and the steps after the first run on those plans."""
    E, nrel, d, N = 500, 11, 1000, 128
    m = _model("InterHT", E, nrel, d, seed=3, gamma=24.0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # (rows, plan blocks) by the rule with one 12-wave block per CU: B 512 fills 256 CUs at 16 rows, so 17 rows (31
    # groups, 248 blocks) there; a larger device keeps 16; 8 plan blocks wherever 8 CUs stay free
    want512 = (17, 8) if cus == 256 else ((16, 8) if cus >= 264 else None)
    for B, rule, want in ((512, 0, want512), (512, -1, want512), (200, -1, (16, 8)), (64, -1, (16, 4)), (64, 16, (16, 4))):  # (forced rows: one plan block per group, 4)
        bs = _batches(E, nrel, B, N, 3, seed=B)
        sp = _planner(m, B, N)
        sp.set_rows(rule)
        assert sp.form()["rows"] == (rule if rule > 0 else 0) and (rule > 0 or sp.form()["plan_blocks"] == 0)
        got = _chain(sp, bs, [0, 1, 0])
        f = sp.form()
        if want is not None and cus >= 256:  # (a smaller device may hold none of these grids with 8 CUs to spare)
            assert (f["rows"], f["plan_blocks"]) == want, (B, rule, cus, f)
        assert f["rows"] in (16, 17, 18, 19), f
        ref = _reference(m, bs, [0, 1, 0])
        for i in range(3):
            assert _same(got[i], ref[i]), (B, rule, i)


@pytest.mark.gpu
def test_plan_of_other_rows_writes_nan():
    """A plan made at 16 rows per group stepped at 17 (and the reverse): the header check makes every output NaN."""
    E, nrel, d, B, N = 400, 7, 64, 40, 128
    m = _model("DistMult", E, nrel, d, seed=4)
    (pos, neg), = _batches(E, nrel, B, N, 1, seed=9)
    for made, stepped in ((16, 17), (17, 16)):
        sp = _planner(m, B, N)
        sp.set_rows(made)
        sp.plan(pos, neg, 1)
        sp.set_rows(stepped)
        out = sp.step()
        torch.cuda.synchronize()
        for t in out:
            assert bool(torch.isnan(t).all()), (made, stepped)


# ---- the row rule on the host (kge_step_planned_rows: no device call) ---------------------------------------------
# LDS of a planned block: R * (images + 28) + slots * image + 1040 (256 bucket counters + 16), images of
# G * 64 lanes * V floats: d 1000 at V 4 is G 4, 4 096 B, and InterHT / RotatE hold two per row (8 220 B a row);
# DistMult d 500 is G 2, one 2 048 B image (2 076 B a row). The launch takes at least its plan blocks' LDS,
# (20 + 2 048 + ceil(2 048 / threads) * waves * 64) * 4 = 17 488 B at 12 waves, 16 464 B at 8 and 16.
C2 = (FN_IDS["InterHT"], 40943, 2000, 11, 3000, 1000, 512, 256, 1000)
C3 = (FN_IDS["RotatE"], 14541, 2000, 237, 1000, 0, 512, 256, 1000)
C4 = (FN_IDS["DistMult"], 123182, 500, 37, 500, 0, 512, 1024, 500)
RULE = [
    # shape, waves, capacity -> rows, relation slots, LDS bytes, scoring blocks
    # C2: 256 blocks fill 256 CUs; 17 rows: 31 groups, 17 * 8 220 + 1 040 = 140 780, 5 slots of 4 096 -> 161 260
    (C2, 0, 256, (17, 5, 161260, 248)),
    # no device (capacity unknown): the library's 16 rows, with the slots the list region's room gives:
    # 16 * 8 220 + 1 040 = 132 560, 7 slots -> 161 232
    (C2, 0, 0, (16, 7, 161232, 256)),
    # a device with room (304 CUs): 256 <= 296, 16 rows stay
    (C2, 0, 304, (16, 7, 161232, 256)),
    # 8 waves build at most 16 rows: no larger R, 16 stay
    (C2, 8, 256, (16, 7, 161232, 256)),
    # C3: no slots; 17 * 8 220 + 1 040
    (C3, 0, 256, (17, 0, 140780, 248)),
    # C4: 17 * 2 076 + 1 040 = 36 332; two blocks per CU (capacity 512): 16 * 2 076 + 1 040 = 34 256
    (C4, 0, 256, (17, 0, 36332, 248)),
    (C4, 0, 512, (16, 0, 34256, 256)),
    # B 1 024 at d 1000: 19 rows are the most that fit (20 * 8 220 > 160 KiB) and still make 432 blocks: 16 stay
    (C2[:6] + (1024, 256, 1000), 0, 256, (16, 7, 161232, 512)),
    # B 520: 16 rows make 264 blocks, 17 rows 31 groups = 248: taken; B 560: 17 -> 264, 18 -> 256, 19 -> 30 groups =
    # 240 blocks, 19 * 8 220 + 1 040 = 157 220, 1 slot -> 161 316; but the unplanned layout gives 16 rows 3 slots,
    # and a larger R must keep at least those: 19 rows are not taken, 16 stay
    (C2[:6] + (520, 256, 1000), 0, 256, (17, 5, 161260, 248)),
    (C2[:6] + (560, 256, 1000), 0, 256, (16, 7, 161232, 280)),
    # RotatE has no slots to keep: B 560 takes 19 rows, 157 220 B, 240 blocks
    (C3[:6] + (560, 256, 1000), 0, 256, (19, 0, 157220, 240)),
]


@pytest.mark.parametrize("shape,waves,cap,want", RULE)
def test_row_rule_against_hand_computed_layouts(shape, waves, cap, want):
    lib = _lib.load()
    out = (ctypes.c_int * 4)()
    rc = lib.kge_step_planned_rows(*shape, waves, cap, ctypes.cast(out, ctypes.c_void_p))
    assert rc == 0, lib.kge_last_error()
    assert tuple(out) == want
    assert out[2] <= 160 * 1024
    fn, E, ent_ld, nrel, rel_ld, rel_off, B, N, D = shape
    # the existing entry points keep the library's 16 rows, and a planner's buffer holds a plan at any count
    hdr, groups = 16, (B + 15) // 16
    words16 = ((hdr + groups * 16 * 4 + groups * 9 + 3) & ~3) + groups * 16 * (N + 1) * 2
    assert lib.kge_step_plan_size(*shape) == words16 * 4
    g = (B + want[0] - 1) // want[0]
    words = ((hdr + g * want[0] * 4 + g * 9 + 3) & ~3) + g * want[0] * (N + 1) * 2
    assert lib.kge_step_planner_plan_size(*shape) >= max(words, words16) * 4
