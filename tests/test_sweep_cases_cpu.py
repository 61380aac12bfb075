"""The references and cases of test_sweep_widths_gpu.py (tests/sweep_cases.py), held to the oracle and to their own
stated properties without a GPU: every query row of every case has a truth whose fp64 rank an evaluation within the
project's score bar cannot move, the chosen truths cover the best, the worst and ranks in between, rank_ref on fp64
scores is the oracle's argsort rank, the filter lists hold the edge rows they claim, the widths and layouts reach
every kernel instance and the refused combinations, the restated block rule gives short last groups, several chunks
and fewer than 16 rows per block for InterHT, and the table views have the strides and base residues their names
promise."""
import numpy as np
import pytest
import torch

from customknowledgegraphembedding_amd import evaluate
from oracle import kge_oracle as O
from tests import eval_cases as C
from tests import strided as S
from tests import sweep_cases as W

# Cases whose best or worst candidate is not isolated: the chosen truths' fp64 ranks start above 1 or end below E.
# (name, d, mode) -> (smallest, largest) fp64 rank among the chosen truths. Every other case has (1, E).
RANK_EDGE_EXCEPTIONS = {("pRotatE", 264, 1): (5, W.E), ("InterHT", 1000, 0): (1, 521)}
# Cases whose isolated candidates lie in the tails only: no chosen truth has an fp64 rank in the middle half
# [E / 4, 3 E / 4] (pRotatE's scores crowd together there: |sin| summed over many elements). Their truths still
# cover both tails (ranks up to about 20 and from about 500). Every other case has truths in the middle half.
TAILS_ONLY = {("pRotatE", 1000, 0), ("pRotatE", 1000, 1), ("pRotatE", 255, 1)}


@pytest.mark.parametrize("d", W.ALL_WIDTHS)
@pytest.mark.parametrize("name", W.FNS)
def test_every_row_has_a_decidable_truth(name, d):
    """Zero undecided queries: every row's truth is isolated (truths asserts there is one), so the rank bounds under
    a perturbation of every score by its bar coincide, with and without the filter, and equal rank_ref's rank."""
    fewest = W.E
    for mode, _ in W.MODES:
        ref = W.ref_scores(name, d, mode)
        truth, count = W.truths(name, d, mode)
        fewest = min(fewest, int(count.min()))
        assert truth[W.ROW_MINUS1] == -1 and truth[W.ROW_E] == W.E
        for q in range(W.B):
            if 0 <= truth[q] < W.E:
                assert W.isolated(ref[q])[truth[q]], (mode, q)
        for filtered in (True, False):
            ptr, ids = W.filters(name, d, mode) if filtered else (None, None)
            lo, hi = W.rank_bounds(ref, truth, ptr, ids)
            assert np.array_equal(lo, hi), (mode, filtered, np.nonzero(lo != hi)[0])
            assert np.array_equal(lo, W.expected_ranks(name, d, mode, filtered).numpy()), (mode, filtered)
        ranks = W.truth_ranks(name, d, mode)
        lo_hi = RANK_EDGE_EXCEPTIONS.get((name, d, mode), (1, W.E))
        assert (int(ranks.min()), int(ranks.max())) == lo_hi, (mode, ranks.min(), ranks.max())
        assert int(((ranks > 1) & (ranks < W.E)).sum()) >= 30, mode  # values in between
        assert len(set(ranks.tolist())) >= 25, mode
        middle = int(((ranks >= W.E // 4) & (ranks <= 3 * W.E // 4)).sum())
        assert (middle == 0) == ((name, d, mode) in TAILS_ONLY), (mode, middle)
        # the filter moves ranks: the filtered expectation differs from the unfiltered one somewhere
        assert not torch.equal(W.expected_ranks(name, d, mode, True), W.expected_ranks(name, d, mode, False))
    assert fewest >= 2
    print(f"{name} d={d}: fewest isolated candidates in a row {fewest}")


def test_issue_widths_have_the_isolation_the_issue_states():
    """The minimum over the issue's seven widths is 2, at pRotatE d = 1000 tail-batch; TransE has >= 270 everywhere."""
    assert int(W.truths("pRotatE", 1000, 1)[1].min()) == 2
    assert min(int(W.truths("TransE", d, m)[1].min()) for d in W.WIDTHS for m, _ in W.MODES) >= 270


@pytest.mark.parametrize("name", W.FNS)
def test_rank_ref_on_fp64_scores_is_the_oracles_rank(name):
    """rank_ref on O.score's fp64 matrix with evaluate.build_filter's CSR equals O.eval_ranks (the upstream argsort
    restatement) on one small tie-free case."""
    n_ent, n_rel, d = 61, 3, 8
    em, rm = S.MULT[name]
    ent, rel, rng = O.make_tables(n_ent, n_rel, em * d, rm * d, 9.0, d, seed=3, dtype=torch.float64)
    g = np.random.RandomState(2)
    true = np.stack([g.randint(n_ent, size=200), g.randint(n_rel, size=200), g.randint(n_ent, size=200)], 1)
    true[30:70, :2] = true[0, :2]
    true[70:110, 1:] = true[1, 1:]
    test = torch.from_numpy(true[:12].astype(np.int64))
    cand = torch.arange(n_ent).unsqueeze(0).expand(len(test), n_ent)
    for mode, col in (("head-batch", 0), ("tail-batch", 2)):
        Sm = O.score(name, ent, rel, test, cand, mode, 9.0, rng, 0.5 * rng)
        ptr, ids = evaluate.build_filter(true[:12], mode, true)
        assert int(np.diff(ptr).max()) >= 20
        got = C.rank_ref(Sm, test[:, col], ptr, ids)
        assert torch.equal(got, O.eval_ranks(name, ent, rel, test, mode, true.tolist(), 9.0, rng, 0.5 * rng)), mode


@pytest.mark.parametrize("name", W.FNS)
def test_filter_lists_hold_their_edge_rows(name):
    for d in (16, 1000):
        for mode, _ in W.MODES:
            truth, _ = W.truths(name, d, mode)
            ptr, ids = W.filters(name, d, mode)
            assert ptr[0] == 0 and ptr[-1] == len(ids) and len(ptr) == W.B + 1
            row = lambda q: ids[ptr[q]:ptr[q + 1]]  # noqa: E731
            assert len(row(W.ROW_EMPTY)) == 0 and len(row(W.ROW_LONG)) > 64 and truth[W.ROW_TRUTH] in row(W.ROW_TRUTH)
            assert row(W.ROW_OUTSIDE)[0] == -1 and row(W.ROW_OUTSIDE)[-1] == W.E and len(row(W.ROW_OUTSIDE)) > 2
            assert np.array_equal(row(W.ROW_ALL), np.arange(W.E))
            for q in range(W.B):  # distinct and ascending: the top-k exclusion lists' contract
                assert (np.diff(row(q)) > 0).all(), q
            assert len(row(W.ROW_MINUS1)) > 0 and len(row(W.ROW_E)) > 0  # out-of-range truths keep a filter


def _cpu_views(name, d, layout):
    """Stand-ins for the GPU views (torch's CPU allocator aligns to 64 B): zeros of the tables' shapes."""
    em, rm = S.MULT[name]
    return W.lay(torch.zeros(9, em * d), torch.zeros(3, rm * d), layout)


@pytest.mark.parametrize("name", W.FNS)
def test_widths_and_layouts_reach_every_instance(name):
    reached, refused = set(), set()
    issue_only = set()
    for d in W.ALL_WIDTHS:
        dense = W.expected(name, d, *_cpu_views(name, d, "dense"))
        for layout in W.LAYOUTS:
            V, G, ok = W.expected(name, d, *_cpu_views(name, d, layout))
            if layout == "pad4":
                assert (V, G, ok) == dense, (d, "pad4 keeps the dense instance")
            if ok:
                reached.add((V, G))
                if d in W.WIDTHS:
                    issue_only.add((V, G))
            else:
                refused.add((d, layout))
                assert G > W.K_SWEEP_MAX_G
    nine = {(v, g) for v in (4, 2, 1) for g in (1, 2, 4)}
    assert reached == nine, sorted(nine - reached)
    assert issue_only == nine - {(2, 2)}  # what the extra width 130 is for
    assert {(264, "pad1"), (1000, "pad2"), (1000, "off1")} <= refused and len(refused) >= 3
    # the boundary moves with the layout: 264 is G = 2 at V = 4, G = 4 at V = 2, refused at V = 1
    assert W.expected(name, 264, *_cpu_views(name, 264, "dense")) == (4, 2, True)
    assert W.expected(name, 264, *_cpu_views(name, 264, "pad2")) == (2, 4, True)
    assert W.expected(name, 264, *_cpu_views(name, 264, "off1")) == (1, 8, False)
    assert W.expected(name, 130, *_cpu_views(name, 130, "dense")) == (2, 2, True)


def test_interht_odd_width_is_narrowed_by_rel_off_alone():
    """InterHT's rel_off = D enters the width choice on its own: with D, both strides and both bases allowing
    float4, an offset of 4 k + 2 floats gives float2 and an odd one dwords. At the odd widths of the cases (33, 255)
    InterHT's entity stride 2 D is even and the base aligned: D, the relation stride 3 D and rel_off = D are what
    leave V = 1."""
    assert S.rel_off("InterHT", 50) == 50 and S.rel_off("TransE", 50) == 0
    assert S.expected_vg(64, lds=(128, 192), offs=(64,), ptrs=(0, 0))[0] == 4
    assert S.expected_vg(64, lds=(128, 192), offs=(66,), ptrs=(0, 0))[0] == 2  # the offset alone
    assert S.expected_vg(64, lds=(128, 192), offs=(65,), ptrs=(0, 0))[0] == 1
    for d in (33, 255):  # odd D: V = 1 on dense aligned tables for every function; InterHT's rows 2 D and 3 D
        ent, rel = _cpu_views("InterHT", d, "dense")
        assert ent.stride(0) % 2 == 0 and W.expected("InterHT", d, ent, rel)[0] == 1


def test_block_rule_of_the_cases():
    """B = 40, E = 523: three row groups (16, 16, 8) and two chunks per slice of 66 rows; InterHT at G V = 16 holds
    11 rows per rank-sweep block (four groups, the last of 7) and 7 per top-k block at k = 64."""
    for name in ("TransE", "RotatE", "pRotatE"):
        for V, G in ((4, 1), (4, 4), (2, 4), (1, 4)):
            for entry, k in (("rank", None), ("topk", 1), ("topk", 10)):
                r = W.block_rule(name, V, G, entry, k)
                assert (r["R"], r["groups"], r["last"], r["chunks"], r["S"]) == (16, 3, 8, 2, 66), (name, V, G, entry, k)
    # k = 64: every wave's list of 64 entries per row is 8 KB of the row's LDS (by hand from 160 KB / row bytes)
    for name, V, G, want in (("TransE", 4, 1, (16, 3, 8)), ("TransE", 4, 4, (13, 4, 1)), ("RotatE", 4, 1, (15, 3, 10)),
                             ("RotatE", 2, 4, (13, 4, 1)), ("RotatE", 4, 4, (9, 5, 4)), ("InterHT", 1, 1, (16, 3, 8))):
        r = W.block_rule(name, V, G, "topk", 64)
        assert (r["R"], r["groups"], r["last"]) == want and r["chunks"] == 2, (name, V, G, r)
    r = W.block_rule("InterHT", 4, 4, "rank")
    assert (r["R"], r["groups"], r["last"], r["chunks"]) == (11, 4, 7, 2)
    r = W.block_rule("InterHT", 4, 4, "topk", 64)
    assert (r["R"], r["groups"], r["last"], r["chunks"]) == (7, 6, 5, 2)
    r = W.block_rule("InterHT", 4, 4, "topk", 10)
    assert r["R"] < 16 and r["groups"] > 3 and 0 < r["last"] < r["R"] and r["chunks"] > 1
    r = W.block_rule("InterHT", 4, 1, "rank")
    assert (r["R"], r["groups"], r["last"]) == (16, 3, 8)
    # a chunk is at least one pair of rows per wave: 66 rows give two chunks of 33
    assert (r["S"] + r["chunks"] - 1) // r["chunks"] >= 2 * W.K_SWEEP_WAVES


@pytest.mark.parametrize("layout", W.LAYOUTS)
def test_views_have_the_strides_and_bases_their_names_promise(layout):
    c = W.case("RotatE", 50)
    ent, rel = W.lay(c["ent"], c["rel"], layout)
    for v, t, (pad, res) in zip((ent, rel), (c["ent"], c["rel"]), W.layout_promise(layout)):
        assert v.shape == t.shape and torch.equal(v, t)
        assert v.stride() == (t.shape[1] + pad, 1) and v.data_ptr() % 16 == res
        if pad or res:  # NaN in every element of the buffer that is not the table's
            base = v._base
            assert int(torch.isnan(base).sum()) == base.numel() - t.numel()
    want_v = {"dense": 2, "pad4": 2, "pad2": 2, "pad1": 1, "ent_pad1": 1, "rel_pad2": 2, "off1": 1, "off2": 2}[layout]
    assert W.expected("RotatE", 50, ent, rel)[0] == want_v
    c4 = W.case("TransE", 16)
    want_v4 = {"dense": 4, "pad4": 4, "pad2": 2, "pad1": 1, "ent_pad1": 1, "rel_pad2": 2, "off1": 1, "off2": 2}[layout]
    assert W.expected("TransE", 16, *W.lay(c4["ent"], c4["rel"], layout))[0] == want_v4


def test_canary_helpers_see_a_stray_write():
    v = W.canary_i64(5, 3, 6, "cpu", k=2)
    assert v.stride(0) == 6 and bool((v == W.CANARY64).all())
    before = W.outside(v)
    v[:] = 7
    assert torch.equal(W.outside(v), before)
    v._base[2 + 3] = 0  # the first row's first padding element
    assert not torch.equal(W.outside(v), before)
    r = W.canary_i64(7, None, None, "cpu", k=4)
    before = W.outside(r)
    r[:] = 1
    assert torch.equal(W.outside(r), before) and before.numel() == 9
    buf, ws = W.canary_bytes(100, "cpu")
    assert ws.numel() == 100 and buf.numel() == 228 and bool((buf == 0xA5).all())
    f = S.canary(4, 3, 5, "cpu", k=1)
    assert torch.equal(W.outside(f), S.outside_bits(f))
