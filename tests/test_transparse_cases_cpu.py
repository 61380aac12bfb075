"""The named TranSparse shapes (transparse_cases.py) reach the branches of csrc/kge_transparse.hip that their
names claim, by the Python restatement of its host dispatch: a later change of a constant there (and in the
restatement) cannot silently empty a case. Runs anywhere; the kernels themselves are held to the oracle at
these shapes in test_transparse_shapes_gpu.py."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import strided as S
from tests import transparse_cases as C

SRC = Path(__file__).resolve().parents[1] / "customknowledgegraphembedding_amd" / "csrc"


def test_restated_constants_are_the_sources():
    ts = (SRC / "kge_transparse.hip").read_text()
    scan = (SRC / "kge_scan.h").read_text()

    def const(text, name):
        m = re.search(r"\b" + name + r"\s*=\s*(0x[0-9A-Fa-f]+|\d+)", text)
        assert m, name
        return int(m.group(1), 0)

    assert const(ts, "TBM") == C.TBM and const(ts, "XBR") == C.XBR and const(ts, "XBC") == C.XBC
    assert const(scan, "kScanTile") == C.K_SCAN_TILE
    assert const(ts, "kTsSortMaxRel") == C.K_TS_SORT_MAX_REL and const(ts, "kTsSortMaxB") == C.K_TS_SORT_MAX_B
    assert const(ts, "kTsBigMaxDim") == C.K_TS_BIG_MAX_DIM and const(ts, "kXsMaxDim") == C.K_XS_MAX_DIM
    assert const(ts, "kXsOOB") == C.K_XS_OOB and const(ts, "kXgKChunks") == C.K_XG_K_CHUNKS
    assert const(ts, "kXgSplitWaves") * 32 == C.K_XG_SPLIT_COLS
    assert const(ts, "kTsPlanesMinRowsPerRel") == C.K_PLANES_MIN_ROWS_PER_REL
    assert "(d + 255) / 256" in ts and C.K_DENT_COLS == 256  # ts_dent_kernel's chunks
    assert "(1024 + base - 1) / base" in ts                   # pick_splits' target


@pytest.mark.parametrize("R,d,S_", [(5, 500, 11), (63, 260, 2), (255, 130, 1), (1023, 8, 1), (1024, 8, 1),
                                    (3, 8, 16)])
def test_pick_splits(R, d, S_):
    assert C.pick_splits(R, C.cdiv(d, C.TBM)) == S_
    assert C.dispatch(300, R, d, 8, 8, 0)["splits"] == S_


@pytest.mark.parametrize("cm", C.ids(C.ALL_CASES), ids=C.case_id)
def test_case_reaches_its_branch(cm):
    c, mode = cm
    got = C.case_dispatch(c, mode)
    want = dict(c["want"].get(None, {}), **c["want"].get(mode, {}))
    for k, v in want.items():
        assert got[k] == v, (c["name"], mode, k, got[k], v)
    kind = c["kind"]
    if kind in ("scan", "rel", "pass", "split", "hot", "accum"):
        _, _, _, _, pos, neg, _ = C.inputs(c, mode)
    if kind == "scan":
        rows = C.entity_rows(pos, neg, mode)
        for i in (0, 1023, 1024, c["E"] - 1):
            assert i >= c["E"] or bool((rows == i).any())
        assert got["scan_tiles_E"] == C.cdiv(c["E"], 1024)
    if kind in ("rel", "pass"):
        for i in (0, 63, 64, c["R"] - 1):
            assert i >= c["R"] or c["B"][mode] < 4 or bool((pos[:, 1] == i).any())
    if kind == "split":
        cnt = np.bincount(pos[:, 1].numpy(), minlength=c["R"])
        assert cnt[c["R"] - 1] == 1 and cnt.max() > 1
        if mode != 0:  # K = that one row: fewer rows than parts wherever there is more than one part
            assert got["splits"] == 1 or cnt[c["R"] - 1] < got["splits"]
    if kind == "width":
        assert got["dent_chunks"] >= 2 and (c["d"] > 256)
    if kind == "hot":
        cnt = np.bincount(C.entity_rows(pos, neg, mode).numpy(), minlength=c["E"])
        assert cnt.max() >= c["bucket"][mode] > C.K_WAVE
    if kind == "accum":
        rows = C.entity_rows(pos, neg, mode)
        assert len(torch.unique(rows)) < c["E"] and set(pos[:, 1].tolist()) == {0, 1, 3}
    if kind == "workload":
        assert C.want_premul(c["R"], c["B"][0], c["N"], 0)


def test_the_cases_cover_every_listed_branch():
    bwd = [C.case_dispatch(c, m) for c, m in C.ids(C.BWD_CASES)]
    assert {x["scan_tiles_E"] for x in bwd} >= {1, 2, 3} and {x["scan_tiles_R"] for x in bwd} == {1, 2}
    assert {x["splits"] for x in bwd} >= {1, 2, 11, 16}
    assert {x["dent_chunks"] for x in bwd} >= {1, 2, 3, 4, 5} and not all(x["use_v4"] for x in bwd)
    fwd = [C.case_dispatch(c, m) for c, m in C.ids(C.FWD_CASES)]
    assert {x["passes"] for x in fwd if x["order"] == "sorted"} >= {1, 2, 4, 16}
    assert {x["order"] for x in fwd} == {"sorted", "natural", "grouped"}
    assert {x["fwd"] for x in fwd} >= {"rows_v1", "rows_x3", "x3", "x3s", "x3g"}
    nblk = [x["nblk"] for x in fwd if x["nblk"]]
    assert any(n % 8 for n in nblk if n > 8) and any(n < 8 for n in nblk)
    # the three default routes no smaller shape reaches
    assert C.dispatch(1100, 2, 1028, 3, 130, 0)["fwd"] == "x3" and C.dispatch(1100, 2, 1024, 3, 130, 0)["fwd"] == "x3s"
    assert C.dispatch(1100, 2, 3076, 3, 130, 0)["fwd"] == "rows_x3"
    assert C.dispatch(1100, 2, 1028, 70, 1, 1)["fwd"] == "rows_x3"
    assert C.dispatch(1100, 2, 1024, 70, 1, 1)["fwd"] == "x3g_split"


@pytest.mark.parametrize("d", C.LAYOUT_DIMS)
def test_pad_and_offset_views_turn_float4_rows_off(d):
    ent = torch.zeros(200, d)
    v4 = d % 4 == 0
    for view, want in ((ent, v4), (S.padded(ent, 4), v4), (S.padded(ent, 1), False), (S.offset(ent, 1), False)):
        ld, ptr = C.view_layout(view)
        assert C.dispatch(200, 3, d, 6, 140, 0, ent_ld=ld, ent_ptr=ptr)["use_v4"] is want
    ld, ptr = C.view_layout(S.padded(ent, 4))
    assert ld == d + 4  # float4 rows with ent_ld != d
    buf = S.like_table(S.padded(ent, 1), fill=0.0)
    assert buf.stride(0) == d + 1 and S.outside_bits(buf).numel() == 200


@pytest.mark.parametrize("mode", [0, 1, 3])
def test_oracle_by_relation_is_the_oracle(mode):
    """oracle_by_relation against O.transparse_score on the whole batch (_oracle), fp64: the same sums per
    row up to the order inside a matmul, 1e-12 of the largest value."""
    E, R, d, B, N = 60, 4, 24, 9, 7
    ent, rel, W, mask = C._tables(E, R, d, seed=2)
    pos, neg = C._batch(E, R, B, N, seed=3)
    grad = torch.randn(B, N if mode == 0 else 1, generator=torch.Generator().manual_seed(4))
    s0, g0 = C._oracle(ent, rel, W, mask, pos, neg, mode, 12.0, grad)
    s1, g1 = C.oracle_by_relation(ent, rel, W, mask, pos, neg, mode, 12.0, grad)
    assert s0.shape == s1.shape and np.abs(s0 - s1).max() <= 1e-12 * np.abs(s0).max()
    for a, b in zip(g0, g1):
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * np.abs(a).max()
    assert C.oracle is not C._oracle and C.K_DIRECT_MAX >= B * d * d
