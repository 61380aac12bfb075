"""The DistMult / ComplEx evaluation chain at every vector width, row stride and base alignment its host code
branches on, each kernel against a plain reference (tests/eval_cases.py, the fp64 oracle): kge_eval_query at
V = 4, 2, 1 with its own narrowing for Q; kge_split_bf16x3's scalar path and zero fill; the plane GEMMs with plane
buffers taller than the matrix and K off 4; ranks with exact ties, NaN and out-of-range entries in score rows off
16 B; and evaluate.score_all / test_step / predict on models whose rows take no float4 loads, with and without the
pass's entity planes. Every output lies in a buffer of a known bit pattern and nothing outside it may change."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import _lib as L
from customknowledgegraphembedding_amd import evaluate
from tests import eval_cases as C
from tests import strided as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ((0, "head-batch"), (1, "tail-batch"))


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------
# a. kge_eval_query
# ------------------------------------------------------------------------------------------------
QUERY_DIMS = [(4, 4, 1), (256, 4, 1), (260, 4, 2), (1000, 4, 4), (2048, 4, 8), (2, 2, 1), (130, 2, 2), (1022, 2, 8),
              (1, 1, 1), (33, 1, 1), (255, 1, 4), (449, 1, 8), (450, 2, 4)]  # (D, V, G) on dense tables and a dense Q
# (450 is even: its dense tables run at V = 2, G = 4; it reaches V = 1, G = 8 through the pad-1 and offset layouts
# and through an odd ldq, which the test asserts; 449 is the dense V = 1, G = 8 case)


@functools.lru_cache(maxsize=None)
def _query_case(name, D):
    return C.query_case(name, D)


@pytest.mark.parametrize("name", ["DistMult", "ComplEx"])
@pytest.mark.parametrize("D,V,G", QUERY_DIMS, ids=[f"D{d}-V{v}G{g}" for d, v, g in QUERY_DIMS])
def test_eval_query_matches_oracle(name, D, V, G):
    """kge_eval_query against O.eval_query_dense in fp64, both modes, tables dense / row-padded by 4 and by 1 / one
    float off 16 B, Q dense / ldq = K + 4 / K + 1 / K + 2 / one and two floats off 16 B, in a canary buffer.
    DistMult is one fp32 multiply: bitwise the rounded fp64 product. ComplEx is two products and an add, with or
    without fma contraction: |err| <= 3 * 2^-24 * (|ab| + |cd|) per element. Rows whose head, relation or tail id
    (of those the mode reads) is out of range are zero. Where the layouts leave more than K_MAX_G groups per lane
    the call is refused with KGE_ENOTSUP and writes nothing."""
    lib = L.load()
    c = _query_case(name, D)
    fn, B, K = L.FN_IDS[name], c["B"], c["K"]
    pos = c["pos"].to(DEV)
    reached, refused, worst = set(), 0, 0.0
    for tl in C.TABLE_LAYOUTS:
        ent, rel = C.lay_tables(c["ent"], c["rel"], tl, DEV)
        for ql in C.Q_LAYOUTS:
            for mode, _ in MODES:
                q = C.q_out(B, K, ql, DEV)
                v, g = C.query_vg(D, ent, rel, q)
                if tl in (None, "pad4") and ql in ("dense", "ld+4"):
                    assert (v, g) == (V, G), (tl, ql)  # the width this dimension is here for
                before = S.outside_bits(q)
                rc = lib.kge_eval_query(fn, mode, ent.data_ptr(), c["E"], ent.stride(0), rel.data_ptr(), c["R"],
                                        rel.stride(0), pos.data_ptr(), B, D, q.data_ptr(), q.stride(0), _st())
                torch.cuda.synchronize()
                assert torch.equal(S.outside_bits(q), before), (tl, ql, mode, "written outside [B, K]")
                if g > S.K_MAX_G:
                    assert rc == C.ENOTSUP, (tl, ql, mode, rc)
                    assert bool((_bits(q) == S.CANARY).all()), (tl, ql, mode, "a refused call wrote Q")
                    refused += 1
                    continue
                assert rc == 0, (tl, ql, mode, lib.kge_last_error())
                reached.add((v, g))
                got = q.cpu()
                ref, scale, zero = c["ref"][mode]
                assert bool((got[zero] == 0).all()), (tl, ql, mode, "an out-of-range id must read as a zero row")
                if name == "DistMult":
                    assert torch.equal(_bits(got[~zero]), _bits(ref.float()[~zero])), (tl, ql, mode)
                else:
                    err = (got.double() - ref).abs()
                    bound = 3 * 2.0 ** -24 * scale
                    rel_err = float((err / scale.clamp_min(1e-300)).max())
                    worst = max(worst, rel_err)
                    assert bool((err <= bound).all()), (tl, ql, mode, rel_err / 2.0 ** -24)
    assert (V, G) in reached
    if D == 450:
        assert (1, 8) in reached
    if D in (1000, 1022, 2048):
        assert refused  # narrowing turns this supported D into KGE_ENOTSUP
    print(f"kge_eval_query {name} D={D}: (V, G) reached {sorted(reached)}, refused {refused}, "
          f"largest |err| / (|ab| + |cd|) = {worst / 2.0 ** -24:.3f} * 2^-24")


# ------------------------------------------------------------------------------------------------
# b. kge_split_bf16x3, kge_eval_query_planes
# ------------------------------------------------------------------------------------------------
def _prefilled_planes(plane_rows, cols):
    nb = int(L.load().kge_split_bf16x3_bytes(plane_rows, cols))
    assert nb == 3 * plane_rows * C.kpad(cols) * 2
    return torch.full((nb,), 0xFF, dtype=torch.uint8, device=DEV)


def _split(x, plane_rows):
    """kge_split_bf16x3 of the view x into 0xFF-prefilled planes (every bf16 a NaN) of plane_rows rows."""
    planes = _prefilled_planes(plane_rows, x.shape[1])
    assert L.load().kge_split_bf16x3(x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), planes.data_ptr(), plane_rows,
                                     _st()) == 0, L.load().kge_last_error()
    return planes


def _check_planes(planes, want, rows, plane_rows, cols, what):
    got = C.planes_bits(planes, plane_rows, cols)
    assert torch.equal(got[:, :, :rows], want.view(torch.int16)), (what, "terms")
    assert bool((got[:, :, rows:] == -1).all()), (what, "rows past `rows` must keep their bytes")
    kp = C.kpad(cols)
    flat = got[:, :, :rows].permute(0, 2, 1, 3).reshape(3, rows, kp)
    assert bool((flat[:, :, cols:] == 0).all()), (what, "k in [cols, kp) must be +0")


@pytest.mark.parametrize("cols", [1, 3, 4, 13, 16, 17, 50, 100])
def test_split_bf16x3_matches_reference(cols):
    """kge_split_bf16x3 bitwise against split3_ref: 37 rows, source dense / ld = cols + 1 / ld rounded up to 4 plus
    4 / one float off 16 B (the float4 path needs ld % 4 == 0, a 16-B base and the whole quad inside cols; every
    other quad takes the scalar path with its zero fill), planes of 37 and 42 rows prefilled with 0xFF. The source
    is surrounded by NaN with 16 floats of it after the last row, so a lost `k + i < cols` test reads a NaN or the
    next row, never past the buffer. Inputs are +-2^-60 .. 2^60 and +-0: subnormal terms and values within a bf16
    ulp of the fp32 maximum (whose first term rounds to inf) are not pinned here."""
    rows = 37
    x = C.split_values(rows, cols, seed=cols)
    want = C.split3_ref(x)
    for layout in C.SPLIT_LAYOUTS:
        ld, off = C.split_layout(cols, layout)
        src = C.source(x, ld, off, DEV)
        for plane_rows in (rows, rows + 5):
            planes = _split(src, plane_rows)
            torch.cuda.synchronize()
            _check_planes(planes, want, rows, plane_rows, cols, (layout, plane_rows))


@pytest.mark.parametrize("name", ["DistMult", "ComplEx"])
@pytest.mark.parametrize("D", [4, 36, 1000])
def test_eval_query_planes_matches_reference(name, D):
    """kge_eval_query_planes on row-padded (pad 4) tables into 0xFF-prefilled planes of B + 5 rows, both modes: the
    planes are bitwise split3_ref of the fp32 query rows they sum to, rows past B keep their bytes, k past K is +0,
    and those query rows meet test_eval_query_matches_oracle's bars against O.eval_query_dense in fp64: DistMult
    bitwise the rounded fp64 product (so the planes are split3_ref(O.eval_query_dense(...).float())), ComplEx within
    3 * 2^-24 * (|ab| + |cd|) (its fp32 value depends on fma contraction, so no fp64 rounding names it bitwise)."""
    lib = L.load()
    c = _query_case(name, D)
    fn, B, K = L.FN_IDS[name], c["B"], c["K"]
    pos = c["pos"].to(DEV)
    ent, rel = C.lay_tables(c["ent"], c["rel"], "pad4", DEV)
    for mode, _ in MODES:
        planes = _prefilled_planes(B + 5, K)
        assert lib.kge_eval_query_planes(fn, mode, ent.data_ptr(), c["E"], ent.stride(0), rel.data_ptr(), c["R"],
                                         rel.stride(0), pos.data_ptr(), B, D, planes.data_ptr(), B + 5, _st()) == 0
        torch.cuda.synchronize()
        q = C.planes_fp32(C.planes_bits(planes, B + 5, K)[:, :, :B])[:, :K]  # the fp32 rows the planes sum to
        ref, scale, zero = c["ref"][mode]
        assert bool((q[zero] == 0).all())
        if name == "DistMult":
            assert torch.equal(_bits(q[~zero]), _bits(ref.float()[~zero]))
            want = ref.float().clone()
            want[zero] = q[zero]  # (the sign of a zero row's zeros is the kernel's)
        else:
            assert bool(((q.double() - ref).abs() <= 3 * 2.0 ** -24 * scale).all())
            want = q
        _check_planes(planes, C.split3_ref(want), B, B + 5, K, (name, D, mode))


# ------------------------------------------------------------------------------------------------
# c. the plane GEMMs
# ------------------------------------------------------------------------------------------------
def _plane_gemm(ap, a_rows, bp, b_rows, K, M, N, form):
    out = S.canary(M, N, N + 3, DEV)
    before = S.outside_bits(out)
    f = L.forms(gemm_form=form)
    assert L.load().kge_gemm_nt_bf16x3_planes_ex(ap.data_ptr(), a_rows, bp.data_ptr(), b_rows, K, out.data_ptr(),
                                                 out.stride(0) if M > 1 else N + 3, M, N, ctypes.addressof(f),
                                                 _st()) == 0, L.load().kge_last_error()
    torch.cuda.synchronize()
    assert torch.equal(S.outside_bits(out), before), (form, "written outside [M, N]")
    return out.cpu()


@pytest.mark.parametrize("M,N", [(1, 1), (37, 193), (257, 300), (70, 513)])
@pytest.mark.parametrize("K", [1, 3, 13, 50, 100])
def test_plane_gemm_forms_match_fp64(M, N, K):
    """kge_gemm_nt_bf16x3_planes_ex, forms 0 to 4, on planes kge_split_bf16x3 wrote into 0xFF-prefilled buffers of
    M or M + 5 and N or N + 7 rows (the rows past M and N hold NaN): every form bitwise the same C, per element
    |C - C64| <= 4e-7 * sum_k |a b| (test_eval_gpu.py's bar for kge_gemm_nt_bf16x3), ldc = N + 3 in a canary buffer
    with nothing written outside [M, N]. K = 1, 3, 13, 50 are no multiples of 4: the last 16-k chunk's zero fill is
    what keeps the planes' prefill out of C."""
    g = torch.Generator().manual_seed(M + 5 * N + K)
    A = (torch.randn(M, K, generator=g) * torch.logspace(-2, 2, K))
    Bm = torch.randn(N, K, generator=g)
    a, b = C.source(A, K, 0, DEV), C.source(Bm, K, 0, DEV)
    ref = A.double() @ Bm.double().T
    scale = A.double().abs() @ Bm.double().abs().T
    worst = 0.0
    for a_rows in (M, M + 5):
        ap = _split(a, a_rows)
        for b_rows in (N, N + 7):
            bp = _split(b, b_rows)
            outs = [_plane_gemm(ap, a_rows, bp, b_rows, K, M, N, form) for form in (0, 1, 2, 3, 4)]
            for form, o in enumerate(outs):
                assert torch.equal(_bits(o), _bits(outs[0])), (a_rows, b_rows, form)
            err = (outs[0].double() - ref).abs()
            rel_err = float((err / scale.clamp_min(1e-300)).max())
            worst = max(worst, rel_err)
            assert bool((err <= 4e-7 * scale).all()), (a_rows, b_rows, rel_err)
    print(f"plane GEMM M={M} N={N} K={K}: largest |C - C64| / sum|ab| = {worst:.3e}")


def test_plane_gemm_asymmetric_identity_at_k13():
    """A = I[:, :13] against an asymmetric integer B, K = 13, every form: I . B^T is exact (rows m < 13 of C are
    the columns of B^T, the others zero), so a transposed write, a swapped k half or a k past 13 read from the
    padded chunk shows."""
    K, M, N = 13, 64, 200
    A = torch.eye(M, K)
    Bm = (torch.arange(N * K, dtype=torch.float32).reshape(N, K) % 97)
    ap, bp = _split(C.source(A, K, 0, DEV), M + 5), _split(C.source(Bm, K, 0, DEV), N + 7)
    want = torch.zeros(M, N)
    want[:K] = Bm.T
    for form in (0, 1, 2, 3, 4):
        assert torch.equal(_plane_gemm(ap, M + 5, bp, N + 7, K, M, N, form), want), form


# ------------------------------------------------------------------------------------------------
# d. ranks with ties and edges
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3, 5, 64, 211, 1030])
def test_rank_filtered_ties_and_edges(N):
    """kge_rank_filtered against rank_ref, exact, on score rows quantised to 8 levels (every row ties with its truth
    many times: counting >= anywhere changes the rank) with NaN and +-inf entries; truth -1 and N, NaN, +inf and
    -inf truth scores; filters that are empty, hold the truth, hold -1 and N, hold every entity; rows dense, with
    ld = N + 1 (every alignment of a row's start in turn) and with ld = N + 3 starting 1, 2 and 3 floats off 16 B
    (the scalar head and tail around the 16-B body), the padding holding +inf. Also with no filter at all."""
    A, truth, fptr, fids = C.tied_rank_case(N)
    want = C.rank_ref(A, truth, fptr, fids)
    want0 = C.rank_ref(A, truth)
    t, p, i = truth.to(DEV), fptr.to(DEV), fids.to(DEV)
    for layout in C.RANK_LAYOUTS:
        ld, off = C.rank_layout(N, layout)
        Sv = C.score_rows(A, ld, off, DEV)
        assert Sv.stride(0) == ld and Sv.data_ptr() % 16 == 4 * off
        got = evaluate.rank_filtered(Sv, t, p, i).cpu()
        assert torch.equal(got, want), (layout, got.tolist(), want.tolist())
        assert torch.equal(evaluate.rank_filtered(Sv, t).cpu(), want0), layout


def _query_planes(c, mode, ent, rel, a_rows):
    """The batch's query planes, a_rows rows, 0xFF-prefilled: kge_eval_query_planes where it applies (D % 4 == 0),
    kge_eval_query (narrower rows) + kge_split_bf16x3 otherwise."""
    lib = L.load()
    fn, B, K, D = L.FN_IDS[c["name"]], c["B"], c["K"], c["D"]
    pos = c["pos"].to(DEV)
    if D % 4 == 0:
        planes = _prefilled_planes(a_rows, K)
        assert lib.kge_eval_query_planes(fn, mode, ent.data_ptr(), c["E"], ent.stride(0), rel.data_ptr(), c["R"],
                                         rel.stride(0), pos.data_ptr(), B, D, planes.data_ptr(), a_rows, _st()) == 0
        return planes
    Q = torch.empty(B, K, device=DEV)
    assert lib.kge_eval_query(fn, mode, ent.data_ptr(), c["E"], ent.stride(0), rel.data_ptr(), c["R"], rel.stride(0),
                              pos.data_ptr(), B, D, Q.data_ptr(), K, _st()) == 0
    return _split(Q, a_rows)


@pytest.mark.parametrize("name,d", [("DistMult", 12), ("ComplEx", 50)])
def test_rank_planes_ties_and_edges(name, d):
    """kge_eval_rank_planes_ex (the library's form and forms 1, 3, 4) and the three phases issued singly, against
    rank_ref applied to the matrix kge_gemm_nt_bf16x3_planes writes from the same planes (the pair scores are
    bitwise that matrix's elements), exact. DistMult K = 12, ComplEx K = 100, E = 300: the entity table holds each
    of 40 rows at four scattered ids, so the scores tied with a truth are bitwise equal by construction; the truths
    are among them and the filters hold their duplicates, the truth itself, -1 and E; one entity row is all +inf
    (a NaN score, never counted); truth -1 and E; entity planes of E + 7 rows, query planes of B + 5."""
    lib = L.load()
    c = C.duplicate_table(name, d)
    B, E, K = c["B"], c["E"], c["K"]
    ent, rel = c["ent"].to(DEV), c["rel"].to(DEV)
    bp = _split(ent, E + 7)
    for mode, _ in MODES:
        ap = _query_planes(c, mode, ent, rel, B + 5)
        Sm = torch.empty(B, E, device=DEV)
        assert lib.kge_gemm_nt_bf16x3_planes(ap.data_ptr(), B + 5, bp.data_ptr(), E + 7, K, Sm.data_ptr(), E, B, E,
                                             _st()) == 0
        torch.cuda.synchronize()
        A = Sm.cpu()
        assert bool(torch.isnan(A[:, E - 3]).all())
        truth, fptr, fids = c["filt"][mode]
        ids = c["dup_ids"]
        for q in (0, 1, 5):  # the ties are there: the truth's duplicates score bitwise the truth's score
            j = int(np.nonzero(ids == int(truth[q]))[0][0])
            assert len(set(_bits(A[q, torch.from_numpy(ids[j])]).tolist())) == 1
        want = C.rank_ref(A, truth, fptr, fids)
        want0 = C.rank_ref(A, truth)
        assert not torch.equal(want, want0)
        t, p, i = truth.to(DEV), fptr.to(DEV), fids.to(DEV)
        nf = int(fptr[-1])
        ws = torch.empty(int(lib.kge_eval_rank_planes_workspace_size(B, nf)), dtype=torch.uint8, device=DEV)
        args = (ap.data_ptr(), B + 5, bp.data_ptr(), E + 7, K, B, E, t.data_ptr())
        for form in (0, 1, 3, 4):
            f = L.forms(gemm_form=form)
            r = torch.full((B,), -5, dtype=torch.int64, device=DEV)
            assert lib.kge_eval_rank_planes_ex(*args, p.data_ptr(), i.data_ptr(), nf, r.data_ptr(), ws.data_ptr(),
                                               ws.numel(), ctypes.addressof(f), _st()) == 0
            torch.cuda.synchronize()
            assert torch.equal(r.cpu(), want), (mode, form, r.tolist(), want.tolist())
            r0 = torch.full((B,), -5, dtype=torch.int64, device=DEV)
            assert lib.kge_eval_rank_planes_ex(*args, None, None, 0, r0.data_ptr(), ws.data_ptr(), ws.numel(),
                                               ctypes.addressof(f), _st()) == 0
            torch.cuda.synchronize()
            assert torch.equal(r0.cpu(), want0), (mode, form, "no filter")
        r = torch.full((B,), -5, dtype=torch.int64, device=DEV)
        for ph in (1, 2, 4):
            assert lib.kge_eval_rank_planes_phases(*args, p.data_ptr(), i.data_ptr(), nf, r.data_ptr(), ws.data_ptr(),
                                                   ws.numel(), ph, None, _st()) == 0
        torch.cuda.synchronize()
        assert torch.equal(r.cpu(), want), (mode, "phases")


# ------------------------------------------------------------------------------------------------
# e. end to end
# ------------------------------------------------------------------------------------------------
def _model(c, layout):
    name, d = c["name"], c["d"]
    de = name == "ComplEx"
    m = kge.KGEModel(name, C.E2E_E, C.E2E_R, d, C.E2E_GAMMA, double_entity_embedding=de, double_relation_embedding=de,
                     device=DEV, seed=c["seed"])
    assert torch.equal(m.entity_embedding.detach().cpu(), c["ent"])
    if layout is not None:
        ent, rel = C.lay_tables(c["ent"], c["rel"], layout, DEV)
        m.entity_embedding = torch.nn.Parameter(ent)
        m.relation_embedding = torch.nn.Parameter(rel)
        assert m.entity_embedding.stride() == ent.stride() and m.entity_embedding.data_ptr() == ent.data_ptr()
    return m


def _topk_of(A, k, ptr, ids):
    """The exact filtered top-k of a score matrix (descending score, ties by ascending id, excluded ids left out)."""
    out_i, out_s = [], []
    for q in range(A.shape[0]):
        s = A[q].astype(np.float64).copy()
        s[ids[ptr[q]:ptr[q + 1]]] = -np.inf
        order = np.lexsort((np.arange(len(s)), -s))[:k]
        out_i.append(order)
        out_s.append(A[q][order])
    return np.stack(out_i), np.stack(out_s)


@pytest.mark.parametrize("planes_on", [True, False], ids=["planes", "noplanes"])
@pytest.mark.parametrize("layout", [None, "pad1", "off1"], ids=["own", "pad1", "off1"])
@pytest.mark.parametrize("name,d,seed", C.E2E_MODELS, ids=[f"{n}{d}" for n, d, _ in C.E2E_MODELS])
def test_evaluation_of_awkward_models(monkeypatch, name, d, seed, layout, planes_on):
    """evaluate.score_all + rank_filtered, rank_planes and test_step for DistMult with hidden_dim 50, 6 (and 8,
    whose float4 rows meet an odd stride) and ComplEx with 25, 50: E = 400, 60 test triples of 1 500 true ones with
    two hub pairs; the model's own tables and pad-1 / offset-1 views of them as its parameters; with the pass's
    entity planes and with planes forced off (the path a table past 4 GB of planes, or short device memory,
    takes). Against O.eval_ranks_dense(rtol = 1e-6) on the fp64 tables: lo <= rank <= hi for every query, equal to
    the fp64 rank wherever lo == hi; at most 5 % of the queries may have lo != hi (a condition on the reference
    alone, checked without a GPU by test_eval_cases_cpu.py); test_step's metrics are metrics_from_ranks of these
    ranks. Before the fix the no-planes cases whose K, row stride or base is off 16 B raised `kge_gemm_nt_bf16x3
    needs K, lda, ldb multiples of 4 and 16-byte aligned A, B`, and d = 8 on a pad-1 view raised
    `kge_eval_query_planes needs D % 4 == 0 and 16-B aligned tables` with planes."""
    c = C.e2e_case(name, d, seed)
    assert C.undecided_share(c) <= C.E2E_MAX_UNDECIDED
    m = _model(c, layout)
    if not planes_on:
        monkeypatch.setattr(evaluate, "PLANES_MAX_BYTES", 16)
    planes = evaluate.entity_planes(m)
    assert (planes is not None) == planes_on
    test, true = c["test"], c["true"]
    pos = torch.from_numpy(test).to(DEV)
    all_ranks = []
    for mode, col in (("head-batch", 0), ("tail-batch", 2)):
        ptr, ids = evaluate.build_filter(test, mode, true)
        fptr, fids = torch.from_numpy(ptr).to(DEV), torch.from_numpy(ids).to(DEV)
        truth = pos[:, col].contiguous()
        Sm = evaluate.score_all(m, pos, mode, planes=planes)
        got = evaluate.rank_filtered(Sm, truth, fptr, fids).cpu()
        ranks, lo, hi = c["ref"][mode]
        assert bool(((lo <= got) & (got <= hi)).all()), (mode, got.tolist(), lo.tolist(), hi.tolist())
        sure = lo == hi
        assert torch.equal(got[sure], ranks[sure]), mode
        rp = evaluate.rank_planes(m, pos, mode, planes, truth, fptr, fids)
        if rp is not None:
            assert torch.equal(rp.cpu(), got), (mode, "rank_planes")
        assert (rp is not None) == (planes_on and d % 4 == 0 and layout is None)
        all_ranks.append(got.numpy())
    want = evaluate.metrics_from_ranks(np.concatenate(all_ranks))
    assert evaluate.test_step(m, test, true, batch_size=32) == want


def test_predict_without_planes_at_d50(monkeypatch):
    """evaluate.predict for DistMult d = 50 without entity planes (K = 50 is no multiple of 4): the exact filtered
    top-k of score_all's matrix (descending score, ties by ascending id, the known answers left out), the matrix
    itself held to the fp64 oracle by test_evaluation_of_awkward_models."""
    name, d, seed = C.E2E_MODELS[0]
    c = C.e2e_case(name, d, seed)
    m = _model(c, None)
    monkeypatch.setattr(evaluate, "PLANES_MAX_BYTES", 16)
    assert evaluate.entity_planes(m) is None
    q = c["test"][:20]
    for mode in ("head-batch", "tail-batch"):
        ids, scores = evaluate.predict(m, q, mode, k=5, known_triples=c["true"], batch_size=16)
        A = evaluate.score_all(m, torch.from_numpy(q).to(DEV), mode).cpu().numpy()
        ptr, xids = evaluate.build_exclude(q, mode, c["true"])
        wi, ws = _topk_of(A, 5, ptr, xids)
        assert np.array_equal(ids.cpu().numpy(), wi) and np.array_equal(scores.cpu().numpy(), ws), mode
