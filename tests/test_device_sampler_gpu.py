"""GPU tests of the device negative sampler (sampler.DeviceTrainDataset, kge_dsampler_sample). The yardstick is the
numpy / Python restatement of the contract in tests/device_sampler_ref.py (Philox4x32-10, u = (x M) >> 64, the u-th
entity outside the row's true-answer list, the table from plain dicts): ids, positives and weights must be equal
bit for bit, no tolerance. Shapes are the smallest that take every path: N 1 / 2 / 7 / 256 (a lone slot, one
pair, an odd tail, two waves per row), B 1 / 5 / 64 / 300 (less than a block of rows, many blocks)."""
import functools
from collections import Counter

import numpy as np
import pytest
import torch

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd.sampler import BidirectionalOneShotIterator, DeviceTrainDataset
from tests import device_sampler_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
DEV = "cuda"
MODES = ("head-batch", "tail-batch")
NS, BS = (1, 2, 7, 256), (1, 5, 64, 300)


@functools.lru_cache(maxsize=None)
def _data(name):
    triples, E, R = {"countries": ref.countries, "synthetic97": ref.synthetic97}[name]()
    return triples, E, R, ref.Table(triples, E)


def _idx(T, B, seed):
    return np.random.RandomState(seed).randint(T, size=B)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV)


def _same(got, want):
    pos, neg, w = (t.cpu().numpy() for t in got)
    return (np.array_equal(pos, want[0]) and np.array_equal(neg, want[1])
            and np.array_equal(w.view(np.uint32), want[2].view(np.uint32)))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("data", ["countries", "synthetic97"])
def test_bit_equal_to_the_restatement(data, mode):
    """Every (N, B): pos, neg, w equal the restatement's, and no negative is a true answer of its row (checked
    against Python sets, independently of the expected ids)."""
    triples, E, R, table = _data(data)
    m = MODES.index(mode)
    for N in NS:
        ds = DeviceTrainDataset(triples, E, R, N, mode, seed=0xC0FFEE + N, device=DEV)
        for B in BS:
            idx = _idx(len(triples), B, seed=B + N)
            if data == "synthetic97":
                idx[:min(B, 4)] = [0, 1, 97, 200][:min(B, 4)]  # the length-1 list and both M = 1 lists
            step = 1000 * N + B
            got = ds.sample(_dev(idx), step=step)
            assert _same(got, table.sample(idx, N, m, ds.seed, step)), (N, B)
            neg = got[1].cpu().numpy()
            assert neg.min() >= 0 and neg.max() < E
            for b, i in enumerate(idx):
                assert not set(neg[b].tolist()) & set(table.list_of(m, int(i))), (N, B, b)


def test_single_valid_entity_fills_the_row():
    """M = 1: every slot of the row is the one entity outside the list."""
    triples, E, R, table = _data("synthetic97")
    assert table.list_of(ref.TAIL, 1) == [k for k in range(E) if k != 40]
    assert table.list_of(ref.HEAD, 97) == list(range(96))
    _, neg, _ = DeviceTrainDataset(triples, E, R, 7, "tail-batch", device=DEV).sample(_dev([1]))
    assert neg.cpu().tolist() == [[40] * 7]
    _, neg, _ = DeviceTrainDataset(triples, E, R, 256, "head-batch", device=DEV).sample(_dev([97]))
    assert neg.cpu().tolist() == [[96] * 256]


def test_split_seed_and_step():
    """One call of 64 rows equals two calls of 32 with row0 0 and 32; another step or seed changes the ids; the
    same inputs repeat them."""
    triples, E, R, _ = _data("countries")
    ds = DeviceTrainDataset(triples, E, R, 7, "head-batch", seed=11, device=DEV)
    idx = _dev(_idx(len(triples), 64, seed=1))
    whole = ds.sample(idx, step=5)
    a, b = ds.sample(idx[:32].contiguous(), step=5, row0=0), ds.sample(idx[32:].contiguous(), step=5, row0=32)
    for x, lo, hi in zip(whole, a, b):
        assert torch.equal(x, torch.cat([lo, hi]))
    assert torch.equal(ds.sample(idx, step=5)[1], whole[1])
    assert not torch.equal(ds.sample(idx, step=6)[1], whole[1])
    assert not torch.equal(ds.sample(idx, step=5 + 2 ** 32)[1], whole[1])  # the step's high word counts
    other = DeviceTrainDataset(triples, E, R, 7, "head-batch", seed=12, device=DEV)
    assert not torch.equal(other.sample(idx, step=5)[1], whole[1])
    assert not torch.equal(ds.sample(idx, step=5, row0=1)[1], whole[1])
    # the internal counter: 0, 1, ... when no step is given
    fresh = DeviceTrainDataset(triples, E, R, 7, "head-batch", seed=11, device=DEV)
    assert torch.equal(fresh.sample(idx)[1], ds.sample(idx, step=0)[1])
    assert torch.equal(fresh.sample(idx)[1], ds.sample(idx, step=1)[1])


@pytest.mark.parametrize("N", [2, 7])
def test_padded_rows_keep_their_padding(N):
    """neg_ld = N + 3 over a canary pattern: nothing outside [B, N] is written (odd strides take the 8-byte
    stores, N = 2 with an even stride would take the 16-byte one: both strides run)."""
    triples, E, R, table = _data("countries")
    ds = DeviceTrainDataset(triples, E, R, N, "tail-batch", seed=3, device=DEV)
    B, canary = 37, -0x5CA1AB1E
    idx = _idx(len(triples), B, seed=9)
    for pad in (3, 4):
        buf = torch.full((B, N + pad), canary, dtype=torch.int64, device=DEV)
        pos = torch.full((B, 3), canary, dtype=torch.int64, device=DEV)
        w = torch.full((B,), 7.0, device=DEV)
        ds.sample(_dev(idx), step=2, out=(pos, buf[:, :N], w))
        assert _same((pos, buf[:, :N], w), table.sample(idx, N, ref.TAIL, 3, 2)), pad
        assert bool((buf[:, N:] == canary).all()), pad


def test_indices_out_of_range():
    triples, E, R, table = _data("countries")
    T = len(triples)
    for N in (1, 7, 256):
        ds = DeviceTrainDataset(triples, E, R, N, "head-batch", seed=1, device=DEV)
        idx = np.array([3, -1, T, T - 1, 2 ** 40, -2 ** 40, 0])
        got = ds.sample(_dev(idx), step=4)
        assert _same(got, table.sample(idx, N, ref.HEAD, 1, 4))
        assert got[0][1].tolist() == [-1, -1, -1] and float(got[2][2]) == 0.0 and bool((got[1][2] == -1).all())


@pytest.mark.parametrize("E", [2 ** 31 + 5, 2 ** 40 + 5])
def test_entities_above_2_31(E):
    """E = 2^31 + 5 with triples whose ids straddle 2^31: the ids are 64-bit all the way (no embedding table is
    needed). At E = 2^40 + 5 the draws themselves pass 2^32."""
    triples = np.array([[2 ** 31 + 1, 0, 3], [2 ** 31 + 1, 0, 2 ** 31 + 4], [7, 1, 2 ** 31 - 1],
                        [2 ** 31, 1, 2 ** 31 - 1], [2 ** 31 + 1, 0, 2 ** 31 - 1]], dtype=np.int64)
    table = ref.Table(triples, E)
    idx = np.array([0, 1, 2, 3, 4, 2])
    for m, mode in enumerate(MODES):
        ds = DeviceTrainDataset(triples, E, 2, 256, mode, seed=2 ** 63 + 9, device=DEV)
        got = ds.sample(_dev(idx), step=2 ** 40 + 1)
        assert _same(got, table.sample(idx, 256, m, 2 ** 63 + 9, 2 ** 40 + 1))
        neg = got[1].cpu().numpy()
        assert neg.min() >= 0 and neg.max() < E and int(got[0].max()) > 2 ** 31
        assert E < 2 ** 32 or neg.max() >= 2 ** 32
        for b, i in enumerate(idx):
            assert not set(neg[b].tolist()) & set(table.list_of(m, int(i)))


def test_empty_and_bad_arguments():
    triples, E, R, _ = _data("countries")
    ds = DeviceTrainDataset(triples, E, R, 4, "tail-batch", device=DEV)
    pos, neg, w = ds.sample(torch.empty(0, dtype=torch.int64, device=DEV))
    assert pos.shape == (0, 3) and neg.shape == (0, 4) and w.shape == (0,)
    pos, neg, w = DeviceTrainDataset(triples, E, R, 0, "tail-batch", device=DEV).sample(_dev([1, 2]))
    assert pos.shape == (2, 3) and neg.shape == (2, 0) and w.shape == (2,)
    good = _dev([1, 2, 3, 4])
    for bad in (good.to(torch.int32), good.cpu(), good[::2], good.reshape(2, 2), [1, 2]):
        with pytest.raises(ValueError):
            ds.sample(bad)
    with pytest.raises(ValueError):
        ds.sample(good, step=torch.zeros(1, dtype=torch.int64))  # a host step tensor
    with pytest.raises(kge.KGEHipError):
        ds.sample(good, row0=2 ** 32 - 2)


def test_graph_capture_follows_the_device_step():
    """sample with a device step and the caller's add_(1), captured on one stream: three replays give steps s,
    s + 1, s + 2 of the restatement."""
    triples, E, R, table = _data("countries")
    N, B, s = 7, 64, 41
    ds = DeviceTrainDataset(triples, E, R, N, "head-batch", seed=8, device=DEV)
    idx = _idx(len(triples), B, seed=2)
    idx_d, step = _dev(idx), torch.tensor([s], dtype=torch.int64, device=DEV)
    out = (torch.empty((B, 3), dtype=torch.int64, device=DEV), torch.empty((B, N), dtype=torch.int64, device=DEV),
           torch.empty(B, device=DEV))
    ds.sample(idx_d, step=step, out=out)  # warm: the first launch loads the code object
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ds.sample(idx_d, step=step, out=out)
        step.add_(1)
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert _same(out, table.sample(idx, N, ref.HEAD, 8, s + k)), k
    assert int(step) == s + 3


def test_batches_cover_an_epoch_and_split_over_replicas():
    """batches(): an epoch's batches are a permutation of the triples (drop_last), and the two replicas of a
    world of 2 draw the rows of the global batch that one replica of twice the batch size draws."""
    triples, E, R, _ = _data("countries")
    T, B = len(triples), 100

    def gen():
        return torch.Generator(device=DEV).manual_seed(4)

    def take(it, n):
        return [next(it) for _ in range(n)]

    whole = take(DeviceTrainDataset(triples, E, R, 5, 1, seed=2, device=DEV).batches(2 * B, generator=gen()), 5)
    halves = [take(DeviceTrainDataset(triples, E, R, 5, 1, seed=2, device=DEV)
                   .batches(B, generator=gen(), row0=k * B, world=2), 5) for k in (0, 1)]
    seen = []
    for g, (pos, neg, w, mode) in enumerate(whole):
        assert mode.tolist() == [1] * (2 * B) and mode.device.type == "cpu"
        for k in (0, 1):
            for x, y in zip((pos, neg, w), halves[k][g][:3]):
                assert torch.equal(x[k * B:(k + 1) * B], y)
        seen += [tuple(r) for r in pos.cpu().tolist()]
    # one epoch: no triple more often than the file holds it
    assert len(seen) == T - T % (2 * B)
    assert not Counter(seen) - Counter(tuple(r) for r in triples.tolist())


def test_trainer_end_to_end():
    """TransE d = 16 on countries_S1, B 64, N 8, 20 steps: a Trainer fed by the device iterator and one fed the
    device sampler's own batches from host memory give bitwise the same losses (only where the batches come from
    differs), and the loss falls: the mean of the last four steps (two of each mode) is below the first four's."""
    from customknowledgegraphembedding_amd.optim import Adam
    from customknowledgegraphembedding_amd.supervisor import Strategy, Sum, Trainer

    triples, E, R, _ = _data("countries")

    def iterator():
        its = [DeviceTrainDataset(triples, E, R, 8, mode, seed=5, device=DEV)
               .batches(64, generator=torch.Generator(device=DEV).manual_seed(1 + k)) for k, mode in enumerate(MODES)]
        return BidirectionalOneShotIterator(*its)

    def host_fed():
        for pos, neg, w, mode in iterator():
            yield pos.cpu(), neg.cpu(), w.cpu(), mode

    losses = []
    for it in (iterator(), host_fed()):
        m = kge.TFKGEModel("TransE", E, R, 16, 12.0, device=DEV, seed=3)
        tr = Trainer(Strategy(), None, m, Adam(m.parameters(), lr=0.05), Sum())
        assert tr.fused
        losses.append([float(tr.train_step(it)) for _ in range(20)])
    print("losses", losses[0])
    assert losses[0] == losses[1]
    assert np.isfinite(losses[0]).all()
    assert np.mean(losses[0][-4:]) < np.mean(losses[0][:4])
