"""GPU tests of the device-built evaluation filter: evaluate.FilterTable.csr (kge_eval_filter_count: lookup and
int64 scan; kge_eval_filter_fill) gives evaluate.build_filter's (drop_own) and build_exclude's (not) CSR, exactly,
for every case, mode and query count of tests/filter_cases.py; the same through the C entry points with ptr and ids
inside canary buffers and ids_capacity exactly ptr[M]; nothing at or past a capacity one short is written; the
result does not depend on the stream or on how the queries are given."""
import numpy as np
import pytest
import torch

from customknowledgegraphembedding_amd import _lib, evaluate
from customknowledgegraphembedding_amd.evaluate import FilterTable
from tests import filter_cases as C

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
DEV = "cuda"
CANARY = -0x5A5A5A5A5A5A5A5B
PAD = 64


@pytest.fixture(scope="module")
def tables():
    return {name: FilterTable(C.case(name)[0], device=DEV) for name in C.CASES}


def queries_dev(name, M):
    return torch.from_numpy(C.case(name)[1][:M].copy()).to(DEV)


def equal(got_ptr, got_ids, want):
    return np.array_equal(got_ptr, want[0]) and np.array_equal(got_ids, want[1])


def raw_csr(table, pos, mode, drop_own, short=0):
    """The two C calls with ptr and ids inside canary buffers, ids_capacity = ptr[M] - short: (ptr, the ids buffer
    behind its front pad, whether every canary in front of ptr and ids and behind ptr survived)."""
    lib = _lib.load()
    M = pos.shape[0]
    m = C.MODES.index(mode)
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(int(lib.kge_eval_filter_workspace_size(M)), dtype=torch.uint8, device=DEV)
    pbuf = torch.full((PAD + M + 1 + PAD,), CANARY, dtype=torch.int64, device=DEV)
    ptr = pbuf[PAD:PAD + M + 1]
    blob, nb = table.table.data_ptr(), table.table.numel() * 8
    _lib.check(lib.kge_eval_filter_count(blob, nb, m, pos.data_ptr(), M, int(drop_own), ptr.data_ptr(), ws.data_ptr(),
                                         ws.numel(), st), "kge_eval_filter_count")
    total = int(ptr[M])
    cap = max(total - short, 0)
    ibuf = torch.full((PAD + total + PAD,), CANARY, dtype=torch.int64, device=DEV)
    _lib.check(lib.kge_eval_filter_fill(blob, nb, m, pos.data_ptr(), M, int(drop_own), ptr.data_ptr(),
                                        ibuf[PAD:].data_ptr(), cap, ws.data_ptr(), ws.numel(), st),
               "kge_eval_filter_fill")
    torch.cuda.synchronize()
    clean = bool((pbuf[:PAD] == CANARY).all() and (pbuf[PAD + M + 1:] == CANARY).all()
                 and (ibuf[:PAD] == CANARY).all())
    return ptr.cpu().numpy(), ibuf[PAD:].cpu().numpy(), clean


@pytest.mark.parametrize("drop_own", [True, False])
@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_csr_is_the_python_one(tables, name, mode, drop_own):
    ref = C.reference(name, mode, drop_own)
    for M in C.M_LIST:
        want = C.prefix(ref, M)
        ptr, ids, ptr_host = tables[name].csr(queries_dev(name, M), mode, drop_own)
        assert ptr.dtype == ids.dtype == torch.int64 and ptr.device.type == ids.device.type == "cuda"
        assert ptr.shape == (M + 1,) and ids.shape == (int(want[0][M]),)
        assert isinstance(ptr_host, np.ndarray) and np.array_equal(ptr_host, want[0])
        assert equal(ptr.cpu().numpy(), ids.cpu().numpy(), want), M


@pytest.mark.parametrize("drop_own", [True, False])
@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_c_calls_write_exactly_ptr_and_ids(tables, name, mode, drop_own):
    """Capacity exactly ptr[M]: the CSR, every canary around ptr and ids intact."""
    ref = C.reference(name, mode, drop_own)
    for M in C.M_LIST:
        want = C.prefix(ref, M)
        ptr, buf, clean = raw_csr(tables[name], queries_dev(name, M), mode, drop_own)
        total = int(want[0][M])
        assert clean and equal(ptr, buf[:total], want), M
        assert (buf[total:] == CANARY).all(), M


@pytest.mark.parametrize("mode", C.MODES)
def test_capacity_one_short(tables, mode):
    """ids_capacity = ptr[M] - 1: the word at the capacity keeps its canary, everything before it is the CSR."""
    ref = C.reference("small", mode, True)
    for M in (65, C.TILE + 1):
        want = C.prefix(ref, M)
        total = int(want[0][M])
        assert total > 1
        ptr, buf, clean = raw_csr(tables["small"], queries_dev("small", M), mode, True, short=1)
        assert clean and np.array_equal(ptr, want[0])
        assert np.array_equal(buf[:total - 1], want[1][:total - 1])
        assert (buf[total - 1:] == CANARY).all()


def test_side_stream_and_numpy_queries(tables):
    """The same CSR on a side stream, and with the queries given as numpy, a list or a device tensor."""
    M = 2 * C.TILE + 9
    side = torch.cuda.Stream()
    for mode in C.MODES:
        want = C.prefix(C.reference("small", mode, True), M)
        q = C.case("small")[1][:M]
        qd = queries_dev("small", M)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            ptr, ids, ptr_host = tables["small"].csr(qd, mode, True)
            side.synchronize()
            assert equal(ptr.cpu().numpy(), ids.cpu().numpy(), want) and np.array_equal(ptr_host, want[0])
        for given in (q, q[:70].tolist()):
            n = len(given)
            ptr, ids, _ = tables["small"].csr(given, mode, True)
            assert equal(ptr.cpu().numpy(), ids.cpu().numpy(), C.prefix(want, n))


def test_a_blob_that_does_not_fit_gives_empty_lists(tables):
    """A table cut short of its word count (and one with another magic): every list empty, ptr all zero."""
    full = tables["small"]
    pos = queries_dev("small", 65)
    for words in (full.table[:full.table.numel() - 1].clone(), torch.cat([full.table[:1] + 1, full.table[1:]])):
        cut = FilterTable.__new__(FilterTable)
        cut.device, cut.table = full.device, words.contiguous()
        ptr, ids, ptr_host = cut.csr(pos, "head-batch", False)
        assert not ptr_host.any() and ids.numel() == 0 and not ptr.cpu().numpy().any()


def test_input_checks(tables):
    t = tables["small"]
    q = queries_dev("small", 8)
    for bad in (q.to(torch.int32), q.cpu(), q[:, :2], q.t().contiguous().t()):  # the last: [8, 3], not contiguous
        with pytest.raises(ValueError):
            t.csr(bad, "head-batch")
    with pytest.raises(ValueError):
        t.csr(q, "single")
    with pytest.raises(ValueError):
        t.csr(np.zeros((4, 2), dtype=np.int64), "head-batch")
    with pytest.raises(_lib.KGEHipError):
        FilterTable([[0, 1, 2]], device="cpu")
    with pytest.raises(_lib.KGEHipError, match="negative id"):
        FilterTable([[0, -1, 2]], device=DEV)
    assert evaluate.FilterTable is FilterTable
