"""The planned tile sweep's forms (kge_step_planner_set_form: waves per block x candidate rows in flight per
wave) and its lead throttle (kge_step_planner_set_board / _set_lead: a progress board per entity slice; a wave
naps once before an item that leads another block of its slice by more than `lead` buckets). Neither may change
a score: every candidate is scored on its own by cand_score, whatever the timing and however many rows are in
flight. So every check is BITWISE on all four step outputs against ops.step_forward_raw (NaN matching NaN; no
tolerance), for every (waves, depth) form, the throttle off, at lead 1 (nearly every item naps) and at lead 32,
both modes, chained steps with the sweep alternating (the step before's tags sit on the board), out-of-range
ids, one-slice and one-row shapes, hostile board contents, and a batch whose scoring blocks outnumber the CUs
(the throttle must then report itself off). Reference: supervisor.py:17-18, model.py:114-205."""
import pytest
import torch

from customknowledgegraphembedding_amd import ops
from tests.test_planned_gpu import _batches, _model, _planner, _same, _unplanned

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORMS = [(8, 2), (12, 2), (12, 1), (16, 2), (16, 1)]
LEADS = [0, 1, 32]  # 0: the throttle off
_cache = {}


def _wide():
    """InterHT d=1000 -de -tr (8 KB rows: 12 waves, G = 4 by default), two row groups, four batches with
    out-of-range ids in candidates and positives; the unplanned reference of both mode sequences, made once."""
    if "wide" not in _cache:
        E, R, d, B, N = 200, 5, 1000, 20, 130
        m = _model("InterHT", E, R, d, gamma=24.0)
        bs = _batches(E, R, B, N, 4, seed=11)
        for pos, neg in bs[1:3]:
            neg[0, :5] = torch.tensor([-1, E, E + 7, -100, 0], device=DEV)
            neg[B - 1, N - 1] = E
            pos[1, 2] = E + 3
            pos[2, 0] = -2
            pos[3, 1] = R + 1
        want = {}
        for mode in (0, 1):
            modes = [mode, 1 - mode, mode, mode]
            want[mode] = (modes, [[t.clone() for t in _unplanned(m, md, p, n)] for md, (p, n) in zip(modes, bs)])
        torch.cuda.synchronize()
        _cache["wide"] = (m, bs, want)
    return _cache["wide"]


def _chain(sp, bs, modes, before_step=None):
    """plan(batch 0), then step i with batch i + 1 planned in its tail (the sweep alternating, the default)."""
    sp.plan(bs[0][0], bs[0][1], modes[0])
    outs = []
    for i in range(len(bs)):
        if before_step is not None:
            before_step(sp, i)
        nxt = (bs[i + 1][0], bs[i + 1][1], modes[i + 1]) if i + 1 < len(bs) else None
        outs.append([t.clone() for t in sp.step(nxt=nxt)])
    torch.cuda.synchronize()
    return outs


def _set(sp, waves, depth, lead):
    sp.set_form(waves, depth)
    sp.set_lead(lead)
    f = sp.form()
    assert (f["waves"], f["depth"], f["lead"]) == (waves, depth, lead), f
    return f


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("waves,depth", FORMS)
def test_wide_rows_every_form_and_lead_bitwise(waves, depth, lead, mode):
    m, bs, want = _wide()
    modes, ref = want[mode]
    sp = _planner(m, bs[0][1].shape[0], bs[0][1].shape[1])
    f = _set(sp, waves, depth, lead)
    assert f["throttle"] == (1 if lead else 0)  # 16 scoring blocks: all resident
    got = _chain(sp, bs, modes)
    for i in range(len(bs)):
        assert _same(got[i], ref[i]), (waves, depth, lead, mode, i)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B,N,hi", [(33, 300, 400), (5, 128, 1), (1, 1, 4000)])
def test_narrow_rows_one_slice_and_one_row_bitwise(B, N, hi, mode):
    """DistMult d=64 (256-B rows: 16 waves by default): every candidate in slice 0 with the other slices' blocks
    empty (they publish nothing), duplicates of one id, and a single row with a single candidate."""
    E, R, d = 4000, 5, 64
    m = _model("DistMult", E, R, d, seed=1)
    bs = _batches(E, R, B, N, 3, seed=B + N, hi=hi)
    modes = [mode, 1 - mode, mode]
    ref = [_unplanned(m, md, p, n) for md, (p, n) in zip(modes, bs)]
    for waves, depth in FORMS:
        for lead in LEADS:
            sp = _planner(m, B, N)
            _set(sp, waves, depth, lead)
            got = _chain(sp, bs, modes)
            for i in range(len(bs)):
                assert _same(got[i], ref[i]), (waves, depth, lead, i)


def _fill(kind):
    def before_step(sp, i):
        b = sp.board.view(torch.int32)
        tag = sp.form()["tag"]
        if kind == "zeros":
            b.zero_()
        elif kind == "max":
            b.fill_(0x7FFFFFFF)
        elif kind == "ghost groups":  # this step's tag, bucket 0, for the row groups that do not exist (2 do)
            b.view(8, 32)[:, 2:] = tag << 9
        else:  # "stuck": every group of every slice a laggard of this step at bucket 0
            b.fill_(tag << 9)
    return before_step


@pytest.mark.parametrize("lead", [1, 32])
@pytest.mark.parametrize("kind", ["zeros", "max", "ghost groups", "stuck"])
def test_hostile_board_contents_change_nothing(kind, lead):
    m, bs, want = _wide()
    modes, ref = want[1]
    for waves, depth in ((12, 2), (16, 1)):
        sp = _planner(m, bs[0][1].shape[0], bs[0][1].shape[1])
        assert _set(sp, waves, depth, lead)["throttle"] == 1
        got = _chain(sp, bs, modes, before_step=_fill(kind))
        for i in range(len(bs)):
            assert _same(got[i], ref[i]), (kind, lead, waves, depth, i)


def test_more_scoring_blocks_than_cus_turns_the_throttle_off():
    """B = 640: 40 row groups x 8 slices = 320 scoring blocks, more than the device's CUs, so they are not all
    resident and a leader would nap for blocks that have not started: the planner reports the throttle off (no
    board reaches the kernel) and the outputs are step_forward_raw's."""
    E, R, d, B, N = 3000, 7, 32, 640, 128
    assert B // 16 * 8 > torch.cuda.get_device_properties(0).multi_processor_count
    m = _model("DistMult", E, R, d, seed=4)
    bs = _batches(E, R, B, N, 2, seed=9)
    modes = [1, 0]
    sp = _planner(m, B, N)
    sp.set_lead(8)
    f = sp.form()
    assert f["lead"] == 8 and f["throttle"] == 0, f
    sp.board.view(torch.int32).fill_(f["tag"] << 9)
    got = _chain(sp, bs, modes)
    for i, (p, n) in enumerate(bs):
        assert _same(got[i], _unplanned(m, modes[i], p, n)), i


def test_setters_refuse_what_the_kernel_does_not_have():
    m, bs, _ = _wide()
    sp = _planner(m, bs[0][1].shape[0], bs[0][1].shape[1])
    lib = sp._lib
    assert lib.kge_step_planner_set_form(sp._h, 8, 1) != 0
    assert lib.kge_step_planner_set_form(sp._h, 10, 2) != 0
    assert lib.kge_step_planner_set_form(sp._h, 12, 3) != 0
    assert lib.kge_step_planner_set_lead(sp._h, 256) != 0
    assert lib.kge_step_planner_set_board(sp._h, sp.board.data_ptr(), sp.board.numel() - 4) != 0
    assert lib.kge_step_planner_get(sp._h, 99) == -1
    assert lib.kge_step_board_size() == sp.board.numel() == 1024
    # the library's own choice is a form the kernel has, and the handle-less planned call takes no board
    f = sp.form()
    assert (f["waves"], f["depth"]) in FORMS and 0 <= f["lead"] < 256
    assert isinstance(ops.StepPlanner.form(sp), dict)
