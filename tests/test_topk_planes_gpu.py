"""kge_eval_topk_planes on the GPU, through the C-ABI unless noted. Operands are fp32 matrices split by
kge_split_bf16x3 into plane buffers taller than the matrix (NaN rows in the surplus); the yardstick is
kge_gemm_nt_bf16x3_planes' matrix on the same planes, fed to the numpy reference (tests/topk_planes_cases.py) and to
kge_topk_rows: ids equal, scores bitwise equal."""
import functools

import numpy as np
import pytest
import torch

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import _lib as L
from customknowledgegraphembedding_amd import evaluate
from tests import topk_planes_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 0x5A


def _st():
    return torch.cuda.current_stream().cuda_stream


def _planes(x, surplus):
    """x [rows, K] split into planes of rows + surplus rows; the surplus rows are NaN."""
    lib = L.load()
    rows, K = x.shape
    full = torch.full((rows + surplus, K), float("nan"), dtype=torch.float32, device=DEV)
    full[:rows] = torch.from_numpy(x).to(DEV)
    out = torch.empty(int(lib.kge_split_bf16x3_bytes(rows + surplus, K)), dtype=torch.uint8, device=DEV)
    evaluate.check(lib.kge_split_bf16x3(full.data_ptr(), rows + surplus, K, full.stride(0), out.data_ptr(),
                                        rows + surplus, _st()), "kge_split_bf16x3")
    return out


class Operands:
    """The planes of a case and the yardstick matrix (computed once, never changed)."""

    def __init__(self, A, B):
        lib = L.load()
        self.M, self.K = A.shape
        self.N = B.shape[0]
        self.a_rows, self.b_rows = self.M + C.SURPLUS_A, self.N + C.SURPLUS_B
        self.ap, self.bp = _planes(A, C.SURPLUS_A), _planes(B, C.SURPLUS_B)
        self.Sd = torch.empty((self.M, self.N), dtype=torch.float32, device=DEV)
        evaluate.check(lib.kge_gemm_nt_bf16x3_planes(self.ap.data_ptr(), self.a_rows, self.bp.data_ptr(), self.b_rows,
                                                     self.K, self.Sd.data_ptr(), self.N, self.M, self.N, _st()), "gemm")
        self.S = self.Sd.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _ops(kind, *key):
    c = {"shape": C.shape_case, "tie": C.tie_case, "kth": C.kth_tie_case, "equal": C.equal_case,
         "special": C.special_case}[kind](*key)
    return Operands(c["A"], c["B"])


def _excl(rows):
    if rows is None:
        return None, None, 0, None, None
    ptr, ids = C.csr([list(r) for r in rows])
    keep = torch.from_numpy(ptr).to(DEV), torch.from_numpy(ids if len(ids) else np.zeros(1, np.int64)).to(DEV)
    return keep[0], keep[1], int(ptr[-1]), ptr, ids


def _call(o, k, rows=None, ws_fill=0xFF, ids_pad=3, sc_pad=5, null_excl=False, M=None):
    """One call with strided, misaligned outputs inside canary buffers and an exactly-sized workspace inside a
    canary. Returns (ids, scores) as numpy after checking that nothing outside [M, k] and the workspace changed."""
    lib = L.load()
    M = o.M if M is None else M
    xp, xi, nx, _, _ = _excl(rows)
    ild, sld = k + ids_pad, k + sc_pad
    ids_buf = torch.full((o.M * ild + 8,), -7, dtype=torch.int64, device=DEV)
    sc_buf = torch.full((o.M * sld + 8,), 123.5, dtype=torch.float32, device=DEV)
    sc = sc_buf[1:]  # one float off 16 B
    assert sc.data_ptr() % 16 == 4
    wsb = int(lib.kge_eval_topk_planes_workspace_size(o.M, o.N, k))
    wbuf = torch.full((wsb + 64,), CANARY, dtype=torch.uint8, device=DEV)
    ws = wbuf[32:32 + wsb]
    off = (-ws.data_ptr()) % 16
    assert off == 0
    ws.fill_(ws_fill)
    rc = lib.kge_eval_topk_planes(o.ap.data_ptr(), o.a_rows, o.bp.data_ptr(), o.b_rows, o.K, M, o.N,
                                  None if (xp is None or null_excl) else xp.data_ptr(),
                                  None if (xi is None or null_excl) else xi.data_ptr(), 0 if null_excl else nx, k,
                                  ids_buf.data_ptr(), ild, sc.data_ptr(), sld, ws.data_ptr(), wsb, _st())
    evaluate.check(rc, "kge_eval_topk_planes")
    torch.cuda.synchronize()
    w = wbuf.cpu().numpy()
    assert (w[:32] == CANARY).all() and (w[32 + wsb:] == CANARY).all()
    ib = ids_buf.cpu().numpy()
    sb = sc_buf.cpu().numpy()
    iv = ib[:o.M * ild].reshape(o.M, ild)
    sv = sb[1:1 + o.M * sld].reshape(o.M, sld)
    assert (iv[:, k:] == -7).all() and (ib[o.M * ild:] == -7).all() and (iv[M:] == -7).all()
    assert (sv[:, k:] == 123.5).all() and sb[0] == 123.5 and (sb[1 + o.M * sld:] == 123.5).all() and (sv[M:] == 123.5).all()
    return iv[:M, :k].copy(), sv[:M, :k].copy()


def _rows_yardstick(o, k, rows):
    xp, xi, nx, _, _ = _excl(rows)
    return tuple(t.cpu().numpy() for t in evaluate.topk_rows(o.Sd, k, xp, xi))


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def _check(o, k, rows=None, **kw):
    got = _call(o, k, rows, **kw)
    ptr, ids = C.csr([list(r) for r in rows]) if rows is not None else (None, None)
    _same(got, C.reference(o.S, k, ptr, ids))
    _same(got, _rows_yardstick(o, k, rows))
    return got


@pytest.mark.parametrize("M,N,K,k", C.SHAPES)
def test_shapes(M, N, K, k):
    o = _ops("shape", M, N, K)
    assert not np.isnan(o.S).any()
    ids, sc = _check(o, k)
    if k > N:
        assert (ids[:, N:] == -1).all() and np.isneginf(sc[:, N:]).all() and (ids[:, :N] >= 0).all()
    _check(o, k, C.exclusion_rows(M, N))


@pytest.mark.parametrize("k", [1, 10, 64])
def test_tie_pairs(k):
    o = _ops("tie")
    ids, _ = _check(o, k)
    seen = 0
    for a, b in C.TIE_PAIRS:
        assert np.array_equal(o.S[:, a].view(np.uint32), o.S[:, b].view(np.uint32))
        for r in ids.tolist():
            if b in r:
                assert a in r and r.index(a) + 1 == r.index(b)
                seen += 1
    assert k == 1 or seen > 0


@pytest.mark.parametrize("k", [1, 10, 64])
def test_kth_and_next_tie(k):
    c = C.kth_tie_case(k)
    o = _ops("kth", k)
    ids, _ = _check(o, k)
    a, b = c["pair"]
    assert o.S[0, a] == o.S[0, b] and ids[0, k - 1] == a and b not in ids[0]


@pytest.mark.parametrize("k", [1, 10, 64])
def test_all_equal(k):
    o = _ops("equal")
    assert (o.S == o.S[:, :1]).all()
    ids, _ = _check(o, k)
    assert (ids == np.arange(k)).all()


@pytest.mark.parametrize("k", [10, 64])
def test_nan_and_infinities(k):
    o = _ops("special")
    assert np.isposinf(o.S[0, list(C.POS_INF_ENTITIES)]).all() and np.isneginf(o.S[0, list(C.NEG_INF_ENTITIES)]).all()
    assert np.isnan(o.S[:, list(C.NAN_ENTITIES)]).all() and np.isnan(o.S[C.NAN_QUERY]).all()
    ids, sc = _check(o, k)
    assert not np.isin(ids, C.NAN_ENTITIES).any()
    assert (ids[C.NAN_QUERY] == -1).all() and np.isneginf(sc[C.NAN_QUERY]).all()
    assert ids[0, :2].tolist() == list(C.POS_INF_ENTITIES) and np.isposinf(sc[0, :2]).all()
    # -inf scores are valid entries, behind every finite one: with everything else excluded they are what is left
    rows = [[e for e in range(o.N) if e not in C.NEG_INF_ENTITIES + C.POS_INF_ENTITIES[:1]]] * o.M
    ids, sc = _check(o, k, rows)
    assert ids[0, :3].tolist() == [C.POS_INF_ENTITIES[0], *C.NEG_INF_ENTITIES] and (ids[0, 3:] == -1).all()


def test_exclusion_rows():
    M, N, K, k = 300, 700, 100, 10
    o = _ops("shape", M, N, K)
    rows = C.exclusion_rows(M, N)
    ids, sc = _check(o, k, rows)
    assert (ids[C.ALL_ROW] == -1).all() and np.isneginf(sc[C.ALL_ROW]).all()
    assert sorted(ids[C.BUT3_ROW, :3].tolist()) == list(C.BUT3_KEPT) and (ids[C.BUT3_ROW, 3:] == -1).all()
    for q in range(M):
        assert not set(ids[q].tolist()) & set(rows[q])
    # nexcl = 0 with non-NULL pointers, and NULL pointers: no exclusion
    plain = _check(o, k)
    _same(_call(o, k, [()] * M), plain)
    _same(_call(o, k, rows, null_excl=True), plain)


@pytest.mark.parametrize("k", [10, 64])
def test_workspace_content_and_repeat(k):
    o = _ops("shape", 300, 700, 16 if k == 64 else 100)
    rows = C.exclusion_rows(300, 700)
    a = _call(o, k, rows, ws_fill=0xFF)
    _same(_call(o, k, rows, ws_fill=0x00), a)
    _same(_call(o, k, rows, ws_fill=0xFF), a)


def test_zero_rows_write_nothing():
    o = _ops("shape", 40, 31, 16)
    ids, sc = _call(o, 10, M=0)
    assert ids.shape == (0, 10) and sc.shape == (0, 10)  # _call checked that every byte kept its canary


def test_fp64_bar():
    """Scores within 4e-7 * sum|a b| of the fp64 dot product (the GEMM's bar), and the returned set a valid top-k of
    the fp64 scores up to that bar: no left-out entity beats the k-th by more than twice the bar."""
    M, N, K, k = 300, 700, 100, 10
    c = C.shape_case(M, N, K)
    o = _ops("shape", M, N, K)
    rows = C.exclusion_rows(M, N)
    ids, sc = _call(o, k, rows)
    A, B = c["A"].astype(np.float64), c["B"].astype(np.float64)
    S64, bar = A @ B.T, 4e-7 * (np.abs(A) @ np.abs(B).T)
    for q in range(M):
        n = int((ids[q] >= 0).sum())
        got = ids[q, :n]
        assert (np.abs(sc[q, :n].astype(np.float64) - S64[q, got]) <= bar[q, got]).all()
        if n < k:
            assert n == N - len(set(rows[q]) & set(range(N)))
            continue
        out = np.setdiff1d(np.arange(N), np.concatenate([got, np.asarray(rows[q], dtype=np.int64)]))
        kth = got[-1]
        assert (S64[q, out] <= S64[q, kth] + 2 * np.maximum(bar[q, out], bar[q, kth])).all()


def test_graph_capture():
    lib = L.load()
    o = _ops("shape", 300, 700, 100)
    k = 10
    xp, xi, nx, _, _ = _excl(C.exclusion_rows(300, 700))
    want = _call(o, k, C.exclusion_rows(300, 700), ids_pad=0, sc_pad=0)
    ids = torch.zeros((o.M, k), dtype=torch.int64, device=DEV)
    sc = torch.zeros((o.M, k), dtype=torch.float32, device=DEV)
    wsb = int(lib.kge_eval_topk_planes_workspace_size(o.M, o.N, k))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = lib.kge_eval_topk_planes(o.ap.data_ptr(), o.a_rows, o.bp.data_ptr(), o.b_rows, o.K, o.M, o.N,
                                      xp.data_ptr(), xi.data_ptr(), nx, k, ids.data_ptr(), k, sc.data_ptr(), k,
                                      ws.data_ptr(), wsb, _st())
    assert rc == 0
    for _ in range(2):
        ids.zero_()
        sc.zero_()
        ws.fill_(0x33)
        g.replay()
        torch.cuda.synchronize()
        _same((ids.cpu().numpy(), sc.cpu().numpy()), want)


# ---- Python ----
E_R = 7


def _model(name, d, E):
    de = name == "ComplEx"
    return kge.KGEModel(name, E, E_R, d, 12.0, double_entity_embedding=de, double_relation_embedding=de, device=DEV,
                        seed=3)


def _queries(E, n=70, seed=0):
    g = np.random.RandomState(seed)
    q = np.stack([g.randint(E, size=n), g.randint(E_R, size=n), g.randint(E, size=n)], 1).astype(np.int64)
    q[: n // 2, 0], q[: n // 2, 1] = 5, 2  # a hub (h, r): many known tails
    known = np.concatenate([q, np.stack([np.full(40, 5), np.full(40, 2), g.choice(E, 40, replace=False)], 1)])
    return q, known


@pytest.mark.parametrize("name,d", [("DistMult", 32), ("ComplEx", 16)])
@pytest.mark.parametrize("E", [400, 523])
@pytest.mark.parametrize("mode", ["head-batch", "tail-batch"])
def test_python_topk_planes(name, d, E, mode):
    m = _model(name, d, E)
    q, known = _queries(E)
    pos = torch.from_numpy(q).to(DEV)
    ptr, xids = evaluate.build_exclude(q, mode, known)
    xp, xi = torch.from_numpy(ptr).to(DEV), torch.from_numpy(xids).to(DEV)
    planes = evaluate.entity_planes(m)
    for k in (10, 64):
        got = evaluate.topk_planes(m, pos, mode, k, planes, xp, xi)
        want = evaluate.topk_rows(evaluate.score_all(m, pos, mode, planes=planes), k, xp, xi)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))


def test_python_none_where_rank_planes_is():
    from tests import strided as S
    q, _ = _queries(400)
    pos = torch.from_numpy(q).to(DEV)
    m = _model("DistMult", 50, 400)  # D % 4 != 0
    assert evaluate.topk_planes(m, pos, "tail-batch", 10, evaluate.entity_planes(m)) is None
    m = _model("DistMult", 32, 400)
    planes = evaluate.entity_planes(m)
    assert evaluate.topk_planes(m, pos, "tail-batch", 10, None) is None
    assert evaluate.topk_planes(m, pos, "tail-batch", 10, planes) is not None
    m.entity_embedding = torch.nn.Parameter(S.padded(m.entity_embedding.detach(), 1, DEV))
    assert not evaluate._planes_rank_ok(m, planes)
    assert evaluate.topk_planes(m, pos, "tail-batch", 10, planes) is None
    r = kge.KGEModel("RotatE", 400, E_R, 16, 12.0, double_entity_embedding=True, device=DEV, seed=3)
    assert evaluate.topk_planes(r, pos, "tail-batch", 10, planes) is None
    with pytest.raises(ValueError):
        evaluate.topk_planes(m, pos, "tail-batch", 65, planes)


@pytest.mark.parametrize("name,d", [("DistMult", 32), ("ComplEx", 16)])
def test_predict_routing(name, d, monkeypatch):
    m = _model(name, d, 523)
    q, known = _queries(523)
    calls = []
    real = evaluate.score_all
    monkeypatch.setattr(evaluate, "score_all", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    for mode in ("head-batch", "tail-batch"):
        monkeypatch.setattr(evaluate, "TOPK_PLANES_FNS", ("DistMult", "ComplEx"))
        monkeypatch.setattr(evaluate, "TOPK_PLANES_MAX_K", evaluate.TOPK_MAX)
        calls.clear()
        a = evaluate.predict(m, q, mode, k=10, known_triples=known, batch_size=32)
        assert not calls  # no [B, E] matrix
        monkeypatch.setattr(evaluate, "TOPK_PLANES_FNS", ())
        b = evaluate.predict(m, q, mode, k=10, known_triples=known, batch_size=32)
        assert len(calls) == 3
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
