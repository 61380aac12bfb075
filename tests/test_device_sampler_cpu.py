"""CPU tests of the device negative sampler's contract and of its host side: the Philox known-answer vectors,
the draw u -> u + j against brute-force complements, the true-answer table kge_dsampler_table_build builds against
a restatement from plain dicts (tests/device_sampler_ref.py) and against TrainDataset's weights (bitwise), its
refusals, and the uniformity of the restated draw. The kernel itself is held to the same restatement, bit for
bit, in test_device_sampler_gpu.py."""
import ctypes
import os

import numpy as np
import pytest

from customknowledgegraphembedding_amd import _lib
from customknowledgegraphembedding_amd.sampler import TrainDataset, build_table
from tests import device_sampler_ref as ref


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for counter, key, want in kat:
        assert ref.philox4x32_10(counter, key) == want


def test_vectorised_philox_is_the_scalar_one():
    """philox_rows (numpy, what the expected ids are made with) against the scalar restatement, word by word:
    counter (n >> 1 | mode << 31, row, step low, step high), key (seed low, seed high), even n the low pair."""
    seed, step = 0x123456789abcdef0, (5 << 32) | 77
    for mode in (0, 1):
        x = ref.philox_rows([0, 3, 2 ** 32 - 1], 5, mode, seed, step)
        for b, row in enumerate([0, 3, 2 ** 32 - 1]):
            for n in range(5):
                w = ref.philox4x32_10(((n >> 1) | (mode << 31), row, 77, 5), (0x9abcdef0, 0x12345678))
                assert x[b, n] == (w[0] | w[1] << 32 if n % 2 == 0 else w[2] | w[3] << 32)


@pytest.mark.parametrize("E", [1, 2, 5, 13, 97])
def test_draw_maps_onto_the_complement(E):
    g = np.random.RandomState(E)
    lists = [[], [0], [E - 1]] + [sorted(g.choice(E, size=g.randint(0, E), replace=False).tolist())
                                  for _ in range(30)]
    for L in lists:
        comp = [e for e in range(E) if e not in set(L)]
        assert [ref.kth_valid(u, L) for u in range(len(comp))] == comp


def _wn18rr_head(n=2000):
    z = np.load(os.path.join(ref.GOLDEN, "wn18rr_ids.npz"))
    return z["triples"][:n].astype(np.int64), int(z["nentity"]), int(z["nrelation"])


@pytest.mark.parametrize("data", ["countries", "wn18rr2000", "synthetic97"])
def test_built_table_against_the_dicts(data):
    triples, E, R = {"countries": ref.countries, "wn18rr2000": _wn18rr_head, "synthetic97": ref.synthetic97}[data]()
    blob = ref.Blob(build_table(triples, E, R))
    want = ref.Table(triples, E)
    T = len(triples)
    assert blob.w[blob.MAGIC] != 0 and blob.w[blob.WORDS] == len(blob.w)
    assert (blob.ntriples, int(blob.w[blob.E]), int(blob.w[blob.R])) == (T, E, R)
    assert np.array_equal(blob.triples, triples)
    for mode in (ref.HEAD, ref.TAIL):
        assert int(blob.w[blob.ROWS + mode]) == len(want.lists[mode])
        assert all(blob.list_of(mode, i) == want.list_of(mode, i) for i in range(T))
        # triples with one key share one row, and no two keys do
        rows = {}
        for i in range(T):
            assert rows.setdefault(want.keys[mode][i], int(blob.row[mode][i])) == int(blob.row[mode][i])
        assert len(set(rows.values())) == len(rows)
    assert np.array_equal(blob.weight.view(np.uint32), want.weight.view(np.uint32))
    _, _, w = TrainDataset(triples, E, R, 1, "tail-batch").sample(np.arange(T))
    assert np.array_equal(blob.weight.view(np.uint32), w.view(np.uint32))  # bitwise kge_sampler_get's


def test_countries_has_long_lists():
    """The fixture's point: the (r, t) lists of regions are long (tens of heads), so the search runs deep."""
    triples, E, _ = ref.countries()
    t = ref.Table(triples, E)
    assert max(len(v) for v in t.lists[ref.HEAD].values()) >= 20


def test_ids_above_2_31():
    E = 2 ** 31 + 5
    triples = np.array([[2 ** 31 + 1, 0, 3], [2 ** 31 + 1, 0, 2 ** 31 + 4], [7, 1, 2 ** 31 - 1],
                        [2 ** 31, 1, 2 ** 31 - 1], [2 ** 31 + 1, 0, 2 ** 31 - 1]], dtype=np.int64)
    blob, want = ref.Blob(build_table(triples, E, 2)), ref.Table(triples, E)
    for mode in (ref.HEAD, ref.TAIL):
        assert all(blob.list_of(mode, i) == want.list_of(mode, i) for i in range(len(triples)))
    assert blob.list_of(ref.TAIL, 0) == [3, 2 ** 31 - 1, 2 ** 31 + 4]


def test_refusals():
    lib = _lib.load()
    with pytest.raises(_lib.KGEHipError, match="out of range"):
        build_table([[0, 0, 5]], 5, 1)
    with pytest.raises(_lib.KGEHipError, match="out of range"):
        build_table([[0, 1, 1]], 5, 1)
    with pytest.raises(_lib.KGEHipError, match="out of range"):
        build_table([[-1, 0, 1]], 5, 1)
    with pytest.raises(_lib.KGEHipError, match="covers every entity"):
        build_table([[0, 0, 0], [0, 0, 1], [0, 0, 2]], 3, 1)  # tails of (0, 0): all three entities
    with pytest.raises(_lib.KGEHipError, match="covers every entity"):
        build_table([[0, 0, 0]], 1, 1)
    t = np.zeros((2, 3), dtype=np.int64)
    buf = np.zeros(1024, dtype=np.int64)
    need = lib.kge_dsampler_table_size(2)
    assert 0 < need <= buf.nbytes and lib.kge_dsampler_table_size(-1) == 0
    assert lib.kge_dsampler_table_build(t.ctypes.data, 2, 4, 1, buf.ctypes.data, need - 8) == -22
    assert b"smaller" in lib.kge_last_error()
    assert lib.kge_dsampler_table_build(t.ctypes.data, 2, 4, 1, None, need) == -22
    assert lib.kge_dsampler_table_build(t.ctypes.data, 2, 4, 1, buf.ctypes.data, need) == 0
    # the sampling entry point rejects ahead of any launch (dummy pointers, as in test_abi.py)
    d = ctypes.c_void_p(16)
    args = dict(blob=d, nb=1024, idx=d, B=4, N=8, row0=0, mode=1, seed=0, step=0, sp=None, pos=d, neg=d, ld=8, w=d)

    def call(**kw):
        a = {**args, **kw}
        return lib.kge_dsampler_sample(a["blob"], a["nb"], a["idx"], a["B"], a["N"], a["row0"], a["mode"], a["seed"],
                                       a["step"], a["sp"], a["pos"], a["neg"], a["ld"], a["w"], None)

    for bad in (dict(mode=3), dict(B=-1), dict(N=-1), dict(ld=7), dict(row0=-1), dict(row0=2 ** 32 - 3),
                dict(pos=None), dict(neg=None), dict(w=None), dict(idx=None), dict(blob=None), dict(nb=8),
                dict(N=2 ** 31, ld=2 ** 31)):
        assert call(**bad) == -22, bad
        assert lib.kge_last_error()
    assert call(B=0, pos=None) == 0 and call(N=0, ld=0, neg=None) == 0  # empty: no launch
    assert call(B=0, ld=7) == -22  # a bad shape is refused even when empty


def test_restated_draw_is_uniform():
    """Head-batch, E = 13, L = {0, 3, 4, 9, 12}: 81 920 draws over the 8 valid entities. Pearson's chi-square must
    stay below 30, the 1e-4 quantile of chi-square with 7 degrees of freedom; the inputs are fixed (the restatement
    gives 11.5)."""
    L, E = [0, 3, 4, 9, 12], 13
    x = ref.philox_rows(range(40), 2048, ref.HEAD, 1234, 7)
    M = E - len(L)
    got = np.array([ref.kth_valid((int(v) * M) >> 64, L) for v in x.reshape(-1)])
    valid = [e for e in range(E) if e not in L]
    assert set(got.tolist()) <= set(valid)
    counts = np.array([(got == e).sum() for e in valid], dtype=np.float64)
    expect = got.size / len(valid)
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    print("chi2", chi2)
    assert chi2 < 30.0
