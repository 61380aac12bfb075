"""CPU tests of the evaluation filter's host side: the table kge_filter_table_build builds, read with numpy from
its own sections (tests/filter_cases.py), gives evaluate.build_filter's and build_exclude's CSR for every case and
mode, exactly; its size query, its refusals, and the bad-argument codes of the two device calls, which come back
before any launch. The kernels are held to the same CSRs in test_filter_gpu.py."""
import ctypes

import numpy as np
import pytest

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import _lib, evaluate
from customknowledgegraphembedding_amd.evaluate import build_filter_table
from tests import filter_cases as C


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_blob_gives_the_python_csr(name):
    triples, queries = C.case(name)
    blob = C.Blob(build_filter_table(triples))
    blob.check_layout()
    assert blob.ntriples == len(triples)
    for mode in C.MODES:
        for drop_own in (True, False):
            want = C.reference(name, mode, drop_own)
            got = blob.csr(queries, mode, drop_own)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (mode, drop_own)


def test_case_set_holds_what_it_should():
    """The list lengths and query kinds the cases are there for."""
    triples, queries = C.case("small")
    blob = C.Blob(build_filter_table(triples))
    for m in (0, 1):
        lens = set(np.diff(blob.ptr[m]).tolist())
        assert set(C.LENGTHS) <= lens and max(lens) > 1024
    assert len(np.unique(triples, axis=0)) < len(triples)      # duplicated true triples
    assert len(np.unique(queries, axis=0)) < len(queries)      # duplicated queries
    for mode in C.MODES:
        full, dropped = (C.reference("small", mode, d)[0] for d in (False, True))
        n_full, n_drop = np.diff(full), np.diff(dropped)
        assert (n_full == 0).any() and ((n_full == 1) & (n_drop == 0)).any()   # absent key; only the own answer
        assert ((n_full > 0) & (n_full == n_drop)).any()                       # own answer absent from the list
    wide, _ = C.case("wide")
    assert (wide >= 2 ** 31).any() and (wide >= 2 ** 40).any()
    low = {(int(a) & 0xFFFFFFFF, int(b) & 0xFFFFFFFF) for _, a, b in wide}
    assert len(low) < len({(int(a), int(b)) for _, a, b in wide})  # keys that differ only above bit 32


def test_sizes_are_host_arithmetic():
    lib = _lib.load()
    for T in (0, 1, 7, 592213):
        assert lib.kge_filter_table_size(T) == 8 * (16 + 2 * (4 * T + 1))
    assert lib.kge_filter_table_size(-1) == 0
    for M in (1, 2, 59071):
        assert lib.kge_eval_filter_workspace_size(M) == 16 * M
    assert lib.kge_eval_filter_workspace_size(0) == 16 and lib.kge_eval_filter_workspace_size(-1) == 0


def test_refusals_of_the_build():
    lib = _lib.load()
    for bad in ([[0, 0, -1]], [[1, 2, 3], [-5, 0, 1]], [[1, -2 ** 40, 3]]):
        with pytest.raises(kge.KGEHipError, match="negative id"):
            build_filter_table(bad)
    t = np.array([[1, 2, -3]], dtype=np.int64)
    buf = np.zeros(1024, dtype=np.int64)
    assert lib.kge_filter_table_build(t.ctypes.data, 1, buf.ctypes.data, buf.nbytes) == -22
    assert b"negative id" in lib.kge_last_error()
    t = np.zeros((2, 3), dtype=np.int64)
    need = lib.kge_filter_table_size(2)
    assert 0 < need <= buf.nbytes
    assert lib.kge_filter_table_build(t.ctypes.data, 2, buf.ctypes.data, need - 8) == -22  # short
    assert b"smaller" in lib.kge_last_error()
    assert lib.kge_filter_table_build(t.ctypes.data, 2, buf.ctypes.data + 4, need) == -22  # misaligned
    assert lib.kge_filter_table_build(t.ctypes.data, 2, None, need) == -22
    assert lib.kge_filter_table_build(None, 2, buf.ctypes.data, need) == -22
    assert lib.kge_filter_table_build(t.ctypes.data, -1, buf.ctypes.data, need) == -22
    assert lib.kge_filter_table_build(t.ctypes.data, 2, buf.ctypes.data, need) == 0


def test_a_list_covering_every_entity_builds():
    """Unlike the sampler's table: tails of (0, 0) are all three entities."""
    triples = np.array([[0, 0, 0], [0, 0, 1], [0, 0, 2]], dtype=np.int64)
    blob = C.Blob(build_filter_table(triples))
    blob.check_layout()
    assert blob.lookup((0, 0, 1), "tail-batch", False) == [0, 1, 2]
    assert blob.lookup((0, 0, 1), "tail-batch", True) == [0, 2]


def test_no_triples_builds():
    blob = C.Blob(build_filter_table(np.zeros((0, 3), dtype=np.int64)))
    blob.check_layout()
    assert blob.ntriples == 0 and blob.rows == [0, 0] and len(blob.w) == 18
    q = np.array([[1, 2, 3], [0, 0, 0]])
    for mode in C.MODES:
        ptr, ids = blob.csr(q, mode, True)
        want = evaluate.build_filter(q, mode, np.zeros((0, 3), dtype=np.int64))
        assert np.array_equal(ptr, want[0]) and np.array_equal(ids, want[1])


def test_device_calls_reject_bad_arguments_without_a_launch():
    lib = _lib.load()
    d = ctypes.c_void_p(16)
    args = dict(blob=d, nb=1024, mode=1, pos=d, M=4, own=1, ptr=d, ids=d, cap=8, ws=d, wsb=64)

    def count(**kw):
        a = {**args, **kw}
        return lib.kge_eval_filter_count(a["blob"], a["nb"], a["mode"], a["pos"], a["M"], a["own"], a["ptr"],
                                         a["ws"], a["wsb"], None)

    def fill(**kw):
        a = {**args, **kw}
        return lib.kge_eval_filter_fill(a["blob"], a["nb"], a["mode"], a["pos"], a["M"], a["own"], a["ptr"],
                                        a["ids"], a["cap"], a["ws"], a["wsb"], None)

    bad = (dict(mode=3), dict(mode=-1), dict(M=-1), dict(blob=None), dict(pos=None), dict(ptr=None), dict(ws=None),
           dict(wsb=63), dict(ws=ctypes.c_void_p(24)), dict(nb=120), dict(blob=ctypes.c_void_p(20)))
    for kw in bad:
        for call in (count, fill):
            assert call(**kw) == -22, (call.__name__, kw)
            assert lib.kge_last_error()
    assert fill(ids=None) == -22 and fill(cap=-1) == -22
    assert fill(M=0, pos=None) == 0 and fill(cap=0, ids=None) == 0  # nothing to copy: no launch
