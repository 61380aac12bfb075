"""GPU tests of test_step and predict over the device-built filter (evaluate.FilterTable): the metrics and the
concatenated ranks of test_step(..., filter_on="device") are those of filter_on="host" (build_filter, the path
before the table existed), exactly, for a sweep model, a planes model (RankPipeline: the CSRs are made on the
caller's stream before the pipeline's streams wait for it) and the matrix path; several rebased batches, one of them
with a total filter of 0; the same with the true triples given as a FilterTable; negative ids take the host path.
predict's ids and scores are equal with the known triples as an array under both filter_on values and as a
FilterTable."""
import numpy as np
import pytest
import torch

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import evaluate
from customknowledgegraphembedding_amd.evaluate import FilterTable

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
DEV = "cuda"
E, R, BS = 101, 6, 16
MODELS = {  # name -> (constructor, hidden_dim, the path test_step takes)
    "TransE": (lambda d: kge.KGEModel("TransE", E, R, d, 9.0, device=DEV, seed=3), 24, "sweep"),
    "DistMult": (lambda d: kge.KGEModel("DistMult", E, R, d, 9.0, device=DEV, seed=3), 32, "planes"),
    "ComplEx": (lambda d: kge.KGEModel("ComplEx", E, R, d, 9.0, double_entity_embedding=True,
                                       double_relation_embedding=True, device=DEV, seed=3), 25, "matrix"),
    "TranSparse": (lambda d: kge.TFKGEModel("TranSparse", E, R, d, 9.0, device=DEV, seed=3), 16, "matrix"),
}


def data():
    """700 true triples over relations 0 .. R - 2 with a hub (r, t) and a hub (h, r) (long lists), and 60 test
    triples: true ones, unseen ones, and in rows 16 .. 31 (the second batch of 16) relation R - 1, which no true
    triple has: that batch's filter is empty in both modes."""
    g = np.random.RandomState(11)
    true = np.stack([g.randint(E, size=700), g.randint(R - 1, size=700), g.randint(E, size=700)], 1).astype(np.int64)
    true[100:160, 1:] = (2, 7)
    true[200:260, :2] = (9, 3)
    true = np.concatenate([true, true[:50]])  # duplicated true triples
    test = np.concatenate([true[90:120], true[195:215],
                           np.stack([g.randint(E, size=10), g.randint(R - 1, size=10), g.randint(E, size=10)], 1)])
    test = test[g.permutation(len(test))]
    test[16:32, 1] = R - 1
    return true, np.ascontiguousarray(test)


def run(m, test, true, monkeypatch, **kw):
    """(metrics, concatenated ranks) of one test_step call."""
    seen = []
    real = evaluate.metrics_from_ranks
    with monkeypatch.context() as mp:
        mp.setattr(evaluate, "metrics_from_ranks", lambda r: seen.append(np.array(r)) or real(r))
        met = evaluate.test_step(m, test, true, batch_size=BS, **kw)
    return met, seen[0]


@pytest.mark.parametrize("name", sorted(MODELS))
def test_test_step_device_filter_is_the_host_one(name, monkeypatch):
    make, d, path = MODELS[name]
    m = make(d)
    true, test = data()
    for mode in ("head-batch", "tail-batch"):
        ptr, _ = evaluate.build_filter(test, mode, true)
        per_batch = [int(ptr[min(s + BS, len(test))] - ptr[s]) for s in range(0, len(test), BS)]
        assert len(per_batch) == 4 and per_batch[1] == 0 and min(per_batch[0], per_batch[2], per_batch[3]) > 0
    planes = evaluate.entity_planes(m)
    assert evaluate._planes_rank_ok(m, planes) == (path == "planes")
    assert evaluate._sweep_rank_ok(m) == (path == "sweep")
    want_met, want_ranks = run(m, test, true, monkeypatch, filter_on="host")
    assert want_ranks.shape == (2 * len(test),) and want_ranks.min() >= 1
    for given, kw in ((true, dict(filter_on="device")), (true, {}), (FilterTable(true, device=DEV), {})):
        calls = []
        with monkeypatch.context() as mp:  # the device path does not walk the triples in Python
            mp.setattr(evaluate, "build_filter", lambda *a, **k: calls.append(a))
            met, ranks = run(m, test, given, mp, **kw)
        assert not calls
        assert np.array_equal(ranks, want_ranks), name
        assert met == want_met
    # a true set with a negative id is no table: the host path, and its metrics
    bad = np.concatenate([true, [[-1, 0, 3]]])
    calls = []
    real = evaluate.build_filter
    with monkeypatch.context() as mp:
        mp.setattr(evaluate, "build_filter", lambda *a, **k: calls.append(a) or real(*a, **k))
        met, ranks = run(m, test, bad, mp)
    assert calls and np.array_equal(ranks, want_ranks) and met == want_met
    with pytest.raises(ValueError):
        evaluate.test_step(m, test, true, batch_size=BS, filter_on="gpu")


def test_a_table_serves_repeated_passes_and_empty_inputs():
    make, d, _ = MODELS["DistMult"]
    m = make(d)
    true, test = data()
    table = FilterTable(true, device=DEV)
    want = evaluate.test_step(m, test, true, batch_size=BS, filter_on="host")
    assert evaluate.test_step(m, test, table, batch_size=BS) == want
    assert evaluate.test_step(m, test, table, batch_size=BS) == want
    assert evaluate.test_step(m, test, table, batch_size=7) == want  # another batching of the same CSR
    none = np.zeros((0, 3), dtype=np.int64)
    assert evaluate.test_step(m, test, none, batch_size=BS) == evaluate.test_step(m, test, none, batch_size=BS,
                                                                                  filter_on="host")


@pytest.mark.parametrize("name", sorted(MODELS))
def test_predict_device_exclusion_is_the_host_one(name):
    make, d, _ = MODELS[name]
    m = make(d)
    true, test = data()
    k = 10
    for mode in ("head-batch", "tail-batch"):
        want = evaluate.predict(m, test, mode, k=k, known_triples=true, batch_size=BS, filter_on="host")
        for known, kw in ((true, dict(filter_on="device")), (true, {}), (FilterTable(true, device=DEV), {})):
            got = evaluate.predict(m, test, mode, k=k, known_triples=known, batch_size=BS, **kw)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (name, mode)
        got = m.predict(torch.from_numpy(test), mode, k=k, known_triples=true, batch_size=BS)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
