"""GPU tests of evaluate.rank_sweep / kge_eval_rank_sweep: filtered ranks of the distance models (TransE, RotatE,
pRotatE, InterHT) without the [B, E] score matrix. The yardstick is exact integer equality with
rank_filtered(score_all(...)): both paths score with the same per-candidate arithmetic on the same operands, so no
tolerance is involved."""
import os

import numpy as np
import pytest
import torch

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import _lib, evaluate
from oracle import kge_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
DEV = "cuda"
FNS = ("TransE", "RotatE", "pRotatE", "InterHT")
MODES = ("head-batch", "tail-batch")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def make_model(name, E, R, d, gamma, seed=5):
    if name == "InterHT":
        return kge.TFKGEModel(name, E, R, d, gamma, True, False, True, device=DEV, seed=seed)
    return kge.KGEModel(name, E, R, d, gamma, double_entity_embedding=name == "RotatE", device=DEV, seed=seed)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV)


def matrix_ranks(m, pos, mode, truth, fptr=None, fids=None):
    return evaluate.rank_filtered(evaluate.score_all(m, pos, mode), truth, fptr, fids)


@pytest.mark.parametrize("name", FNS)
def test_sweep_ranks_match_oracle(name):
    """The configuration of test_eval_gpu.py::test_filtered_ranks_match_oracle, where the matrix path meets the
    oracle's argsort ranks exactly."""
    E, R, d, gamma = 211, 5, 16, 6.0
    m = make_model(name, E, R, d, gamma, seed=4)
    g = np.random.RandomState(2)
    true = np.stack([g.randint(E, size=400), g.randint(R, size=400), g.randint(E, size=400)], 1)
    test = true[:29]
    ent = m.entity_embedding.detach().cpu().double()
    rel = m.relation_embedding.detach().cpu().double()
    mod = float(m.modulus.detach().reshape(-1)[0]) if name == "pRotatE" else None
    for mode in MODES:
        ptr, ids = evaluate.build_filter(test, mode, true)
        pos = dev(test)
        col = 0 if mode == "head-batch" else 2
        got = evaluate.rank_sweep(m, pos, mode, pos[:, col].contiguous(), dev(ptr), dev(ids))
        assert got is not None
        want = O.eval_ranks(name, ent, rel, torch.from_numpy(test), mode, true, gamma, m._range_f, mod)
        assert torch.equal(got.cpu(), want), (name, mode, got, want)


# per-half widths: float4 rows at 1, 2 and 4 groups per lane; float2 rows at 1 and 4; dword rows at 1 and 4
WIDTHS = (16, 300, 1000, 50, 450, 33, 255)


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("name", FNS)
def test_every_instance_equals_score_matrix_ranks(name, d):
    """E = 523 (no multiple of the 8 slices, of the wave count or of 64), B = 40 (no multiple of a row group),
    hub (h, r) / (r, t) pairs so that some filter rows pass 64 entries; the workspace's pair scores are bitwise
    the matrix's elements."""
    E, R, B = 523, 7, 40
    m = make_model(name, E, R, d, 12.0)
    g = np.random.RandomState(E + d)
    n = B + 400 + 3 * B
    true = np.stack([g.randint(E, size=n), g.randint(R, size=n), g.randint(E, size=n)], 1)
    true[B:B + 200, 0] = true[0, 0]
    true[B:B + 200, 1] = true[0, 1]
    true[B + 200:B + 400, 2] = true[1, 2]
    true[B + 200:B + 400, 1] = true[1, 1]
    q = true[:B]
    pos = dev(q)
    for mode in MODES:
        ptr, ids = evaluate.build_filter(q, mode, true)
        assert int(np.diff(ptr).max()) > 64
        col = 0 if mode == "head-batch" else 2
        truth = pos[:, col].contiguous()
        fptr, fids = dev(ptr), dev(ids)
        S = evaluate.score_all(m, pos, mode)
        want = evaluate.rank_filtered(S, truth, fptr, fids)
        evaluate._SWEEP_WS.clear()
        got = evaluate.rank_sweep(m, pos, mode, truth, fptr, fids)
        assert got is not None
        torch.cuda.synchronize()
        assert torch.equal(got, want), (name, d, mode, got, want)
        # the workspace: [B] truth scores, [B] counts, then the filter entries' scores at the next 16 B
        (ws,) = evaluate._SWEEP_WS.values()
        Sc, tc = S.cpu(), truth.cpu()
        ts = ws[:4 * B].view(torch.float32).cpu()
        assert torch.equal(ts.view(torch.int32), Sc[torch.arange(B), tc].view(torch.int32))
        off = (B * 8 + 15) // 16 * 16
        nf = len(ids)
        fs = ws[off:off + 4 * nf].view(torch.float32).cpu()
        rows = torch.from_numpy(np.repeat(np.arange(B), np.diff(ptr)))
        assert nf > 10
        assert torch.equal(fs.view(torch.int32), Sc[rows, torch.from_numpy(ids)].contiguous().view(torch.int32))


@pytest.mark.parametrize("E", [1, 5, 8, 9, 64, 65])
@pytest.mark.parametrize("name", ["TransE", "InterHT"])
def test_edges(name, E):
    """Empty entity slices, one row per slice, chunk boundaries; one query row and a short row group; truths and
    filter ids just outside [0, E); no filter; a filter_ptr of zeros with no ids; a workspace of any content."""
    R, d = 3, 20
    m = make_model(name, E, R, d, 9.0)
    g = np.random.RandomState(E)
    for B in (1, 17):
        q = np.stack([g.randint(E, size=B), g.randint(R, size=B), g.randint(E, size=B)], 1)
        pos = dev(q)
        # up to 3 distinct ids per row out of [-1, E]: -1 and E among the valid ones
        rows = [g.choice(np.arange(-1, E + 1), size=min(3, E + 2), replace=False) for _ in range(B)]
        rows[0] = np.array([-1, E, 0])[:min(3, E + 2)] if E + 2 >= 3 else rows[0]
        ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
        ids = np.concatenate(rows)
        fptr, fids, zptr = dev(ptr), dev(ids), dev(np.zeros(B + 1))
        for mode in MODES:
            col = 0 if mode == "head-batch" else 2
            for variant in range(3):
                truth = pos[:, col].contiguous().clone()
                if variant == 1:
                    truth[0] = -1
                if variant == 2:
                    truth[B - 1] = E
                S = evaluate.score_all(m, pos, mode)
                want = evaluate.rank_filtered(S, truth, fptr, fids)
                want0 = evaluate.rank_filtered(S, truth)
                tag = (name, E, B, mode, variant)
                got = evaluate.rank_sweep(m, pos, mode, truth, fptr, fids)
                assert got is not None and torch.equal(got, want), (tag, got, want)
                assert torch.equal(evaluate.rank_sweep(m, pos, mode, truth), want0), tag
                assert torch.equal(evaluate.rank_sweep(m, pos, mode, truth, zptr, None, 0), want0), tag
                (ws,) = evaluate._SWEEP_WS.values()
                for fill in (0xFF, 0):
                    ws.fill_(fill)
                    assert torch.equal(evaluate.rank_sweep(m, pos, mode, truth, fptr, fids), want), (tag, fill)
                a = evaluate.rank_sweep(m, pos, mode, truth, fptr, fids)  # back to back on one workspace
                b = evaluate.rank_sweep(m, pos, mode, truth, fptr, fids)
                assert torch.equal(a, want) and torch.equal(b, want), tag


def test_interht_nan_rows():
    """Q7: InterHT divides by the candidate's norms without an epsilon, so a zero entity row scores NaN. A NaN
    never counts as above a truth, and nothing counts as above a NaN truth: as rank_kernel's comparisons."""
    E, R, d, B, z = 100, 4, 16, 12, 7
    m = make_model("InterHT", E, R, d, 9.0)
    with torch.no_grad():
        m.entity_embedding[z].zero_()
    g = np.random.RandomState(1)
    others = np.array([e for e in range(E) if e != z])
    q = np.stack([g.choice(others, size=B), g.randint(R, size=B), g.choice(others, size=B)], 1)
    for as_truth in (False, True):
        for mode in MODES:
            col = 0 if mode == "head-batch" else 2
            qq = q.copy()
            if as_truth:
                qq[2, col] = z
            pos = dev(qq)
            truth = pos[:, col].contiguous()
            ptr, ids = evaluate.build_filter(qq, mode, np.concatenate([qq, q]))
            S = evaluate.score_all(m, pos, mode)
            assert bool(torch.isnan(S[:, z]).all())
            want = evaluate.rank_filtered(S, truth, dev(ptr), dev(ids))
            got = evaluate.rank_sweep(m, pos, mode, truth, dev(ptr), dev(ids))
            assert torch.equal(got, want), (as_truth, mode, got, want)
            if as_truth:
                assert int(got[2]) == 1


def test_full_size_wn18rr_interht():
    """WN18RR InterHT d 1 000 (-de -tr), E 40 943: 96 queries and the filter from the dataset's triples."""
    z = np.load(os.path.join(GOLDEN, "wn18rr_ids.npz"))
    triples, E, R = z["triples"].astype(np.int64), int(z["nentity"]), int(z["nrelation"])
    m = make_model("InterHT", E, R, 1000, 24.0, seed=0)
    q = triples[::len(triples) // 96][:96]
    pos = dev(q)
    for mode in MODES:
        ptr, ids = evaluate.build_filter(q, mode, triples)
        col = 0 if mode == "head-batch" else 2
        truth = pos[:, col].contiguous()
        want = matrix_ranks(m, pos, mode, truth, dev(ptr), dev(ids))
        got = evaluate.rank_sweep(m, pos, mode, truth, dev(ptr), dev(ids), len(ids))
        assert got is not None and torch.equal(got, want), (mode, got, want)


@pytest.mark.parametrize("name", ["InterHT", "RotatE"])
def test_test_step_uses_the_sweep_and_falls_back(name, monkeypatch):
    """test_step's metrics through the sweep (as shipped), with the predicate off (the matrix path), and with a
    rank_sweep that answers None (the per-batch fallback): the same. 300 queries in batches of 128: a short last
    batch."""
    E, R, d = 1200, 6, 64
    m = make_model(name, E, R, d, 9.0)
    g = np.random.RandomState(3)
    true = np.stack([g.randint(E, size=1500), g.randint(R, size=1500), g.randint(E, size=1500)], 1)
    calls = []
    real = evaluate.rank_sweep

    def counted(*a, **k):
        r = real(*a, **k)
        calls.append(r is not None)
        return r

    monkeypatch.setattr(evaluate, "rank_sweep", counted)
    shipped = evaluate.test_step(m, true[:300], true, batch_size=128)
    if evaluate._sweep_rank_ok(m):
        assert len(calls) == 6 and all(calls)
    else:
        assert not calls
    monkeypatch.setattr(evaluate, "_sweep_rank_ok", lambda model: False)
    calls.clear()
    matrix = evaluate.test_step(m, true[:300], true, batch_size=128)
    assert not calls
    assert shipped == matrix
    monkeypatch.setattr(evaluate, "_sweep_rank_ok", lambda model: True)
    monkeypatch.setattr(evaluate, "rank_sweep", lambda *a, **k: None)
    assert evaluate.test_step(m, true[:300], true, batch_size=128) == matrix


def test_widest_rows():
    """D = 2 048 (8 groups per lane): rank_sweep gives exact ranks or None, and test_step the matrix path's
    metrics either way."""
    E, R, d, B = 300, 5, 2048, 20
    m = make_model("TransE", E, R, d, 12.0)
    g = np.random.RandomState(8)
    true = np.stack([g.randint(E, size=200), g.randint(R, size=200), g.randint(E, size=200)], 1)
    q = true[:B]
    pos = dev(q)
    for mode in MODES:
        ptr, ids = evaluate.build_filter(q, mode, true)
        col = 0 if mode == "head-batch" else 2
        truth = pos[:, col].contiguous()
        got = evaluate.rank_sweep(m, pos, mode, truth, dev(ptr), dev(ids))
        if got is not None:
            assert torch.equal(got, matrix_ranks(m, pos, mode, truth, dev(ptr), dev(ids)))
    shipped = evaluate.test_step(m, q, true, batch_size=16)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(evaluate, "_sweep_rank_ok", lambda model: False)
        assert evaluate.test_step(m, q, true, batch_size=16) == shipped
