"""Training-batch negative sampler: drop-in for the upstream KnowledgeGraphEmbedding
`TrainDataset` / `BidirectionalOneShotIterator` (codes/dataloader.py, absent from the snapshot;
the reference's call sites are compress_data/main.py:64-90), running in the C++ sampler of
libkge_hip.so (kge_sampler_*).

Negative ids are bit-exact with upstream's numpy code for the same numpy RNG state: construct with
`seed=s` to reproduce `np.random.seed(s)` followed by the same sequence of __getitem__ calls.
Batches are produced in host memory (numpy) and moved to the device by the caller (pinned copies
overlap with compute on a side stream).

`DeviceTrainDataset` draws the same distribution on the GPU instead (kge_dsampler_sample, a counter-based
Philox stream: not numpy's ids), so that a run from a triple file is not bound by the one host thread.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import HEAD_BATCH, TAIL_BATCH, check

_MODES = {"head-batch": HEAD_BATCH, "tail-batch": TAIL_BATCH, 0: HEAD_BATCH, 1: TAIL_BATCH}


class TrainDataset:
    """upstream TrainDataset(triples, nentity, nrelation, negative_sample_size, mode)."""

    def __init__(self, triples, nentity, nrelation, negative_sample_size, mode, seed=0):
        self.triples = np.ascontiguousarray(np.asarray(triples, dtype=np.int64).reshape(-1, 3))
        self.len = len(self.triples)
        self.nentity = int(nentity)
        self.nrelation = int(nrelation)
        self.negative_sample_size = int(negative_sample_size)
        self.mode = mode if isinstance(mode, str) else {HEAD_BATCH: "head-batch", TAIL_BATCH: "tail-batch"}[mode]
        lib = _lib.load()
        self._h = lib.kge_sampler_create(self.triples.ctypes.data, self.len, self.nentity, self.nrelation,
                                         self.negative_sample_size, _MODES[self.mode])
        if not self._h:
            raise _lib.KGEHipError(lib.kge_last_error().decode())
        self.seed(seed)

    def seed(self, seed: int):
        check(_lib.load().kge_sampler_seed(self._h, ctypes.c_uint32(int(seed) & 0xFFFFFFFF)), "kge_sampler_seed")

    def __len__(self):
        return self.len

    def sample(self, idx):
        """__getitem__ for every index in `idx`, in order -> (pos [B,3] int64, neg [B,N] int64, w [B] f32)."""
        idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).reshape(-1))
        B, N = len(idx), self.negative_sample_size
        pos = np.empty((B, 3), dtype=np.int64)
        neg = np.empty((B, N), dtype=np.int64)
        w = np.empty((B,), dtype=np.float32)
        check(_lib.load().kge_sampler_get(self._h, idx.ctypes.data, B, pos.ctypes.data, neg.ctypes.data,
                                          w.ctypes.data), "kge_sampler_get")
        return pos, neg, w

    def __getitem__(self, idx):
        pos, neg, w = self.sample([idx])
        return (torch.from_numpy(pos[0]), torch.from_numpy(neg[0]), torch.from_numpy(w[:1]), self.mode)

    @staticmethod
    def collate_fn(data):
        positive_sample = torch.stack([_[0] for _ in data], dim=0)
        negative_sample = torch.stack([_[1] for _ in data], dim=0)
        subsample_weight = torch.cat([_[2] for _ in data], dim=0)
        mode = data[0][3]
        return positive_sample, negative_sample, subsample_weight, mode

    def batches(self, batch_size, shuffle=True, rng=None, drop_last=True, prefetch=0):
        """Endless batches (pos, neg, weight, mode) like a DataLoader over this dataset. With
        prefetch > 0 a host thread samples ahead (the C++ sampler releases the GIL), so sampling
        overlaps the GPU step; the batches and their order are unchanged."""
        rng = rng or np.random.RandomState(0)

        def produce():
            while True:
                order = rng.permutation(self.len) if shuffle else np.arange(self.len)
                stop = self.len - (self.len % batch_size if drop_last else 0)
                for s in range(0, stop, batch_size):
                    pos, neg, w = self.sample(order[s:s + batch_size])
                    yield torch.from_numpy(pos), torch.from_numpy(neg), torch.from_numpy(w), self.mode

        if prefetch <= 0:
            yield from produce()
            return
        import queue
        import threading

        q: queue.Queue = queue.Queue(maxsize=prefetch)
        stop = threading.Event()

        def worker():
            try:
                for item in produce():
                    while not stop.is_set():
                        try:
                            q.put(item, timeout=0.1)
                            break
                        except queue.Full:
                            continue
                    if stop.is_set():
                        return
            except BaseException as e:  # noqa: BLE001 (re-raised in the consumer)
                q.put(e)

        threading.Thread(target=worker, daemon=True).start()
        try:
            while True:
                item = q.get()
                if isinstance(item, BaseException):
                    raise item
                yield item
        finally:
            stop.set()

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.load().kge_sampler_destroy(h)
            except Exception:  # noqa: BLE001 (interpreter shutdown)
                pass
            self._h = None


class DeviceTrainDataset:
    """TrainDataset's batches drawn ON the device (kge_dsampler_sample): N negatives per row, uniform over the
    entities that are not true answers of the row, which is upstream's distribution, from a counter-based
    Philox stream keyed by (seed, step, mode, global row, slot). The ids are NOT numpy's stream: use
    TrainDataset to replay an upstream run bit for bit. The true-answer table is built once on the host
    (kge_dsampler_table_build) and uploaded; after that nothing touches the host per step, and `sample` can be
    captured in a graph in front of the train step."""

    def __init__(self, triples, nentity, nrelation, negative_sample_size, mode, seed=0, device=None):
        triples = np.ascontiguousarray(np.asarray(triples, dtype=np.int64).reshape(-1, 3))
        self.len = len(triples)
        self.nentity = int(nentity)
        self.nrelation = int(nrelation)
        self.negative_sample_size = int(negative_sample_size)
        self.mode = mode if isinstance(mode, str) else {HEAD_BATCH: "head-batch", TAIL_BATCH: "tail-batch"}[mode]
        self._mode = _MODES[self.mode]
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.step = 0  # the next sample()'s step when none is given
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise _lib.KGEHipError(f"DeviceTrainDataset needs a GPU device, got {self.device} (there is no CPU "
                                   "fallback; TrainDataset samples on the host)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.table = torch.from_numpy(build_table(triples, self.nentity, self.nrelation)).to(self.device)
        self._modes = {}

    def __len__(self):
        return self.len

    def sample(self, idx, step=None, row0=0, out=None):
        """(pos [B,3] int64, neg [B,N] int64, w [B] f32) on the device for the triple indices `idx` (a contiguous
        int64 tensor on the device). `step`: an int, a one-element int64 device tensor read when the launch runs
        (a captured launch follows the caller's captured increment), or None for the internal counter, which
        then advances by one. `row0`: the global row number of idx[0] (a replica's offset into the global
        batch). `out`: (pos, neg, w) to write into; neg may be a view with a row stride above N."""
        dev = self.device
        if not torch.is_tensor(idx) or idx.dtype != torch.int64 or not idx.is_contiguous() or idx.device != dev \
                or idx.dim() != 1:
            raise ValueError(f"DeviceTrainDataset.sample: idx must be a contiguous 1-d int64 tensor on {dev}")
        B, N = idx.numel(), self.negative_sample_size
        step_ptr = None
        if step is None:
            step, self.step = self.step, self.step + 1
        elif torch.is_tensor(step):
            if step.dtype != torch.int64 or step.device != dev or step.numel() != 1:
                raise ValueError(f"DeviceTrainDataset.sample: a tensor step must be one int64 on {dev}")
            step_ptr, step = step.data_ptr(), 0
        if out is None:
            pos = torch.empty((B, 3), dtype=torch.int64, device=dev)
            neg = torch.empty((B, N), dtype=torch.int64, device=dev)
            w = torch.empty((B,), dtype=torch.float32, device=dev)
        else:
            pos, neg, w = out
            for name, t, dt, shape in (("pos", pos, torch.int64, (B, 3)), ("neg", neg, torch.int64, (B, N)),
                                       ("w", w, torch.float32, (B,))):
                if t.dtype != dt or t.device != dev or tuple(t.shape) != shape:
                    raise ValueError(f"DeviceTrainDataset.sample: out {name} must be {dt} {shape} on {dev}")
            if not pos.is_contiguous() or not w.is_contiguous() or (N > 0 and neg.stride(1) != 1) \
                    or (B > 1 and N > 0 and neg.stride(0) < N):
                raise ValueError("DeviceTrainDataset.sample: out pos and w contiguous, neg rows contiguous")
        neg_ld = neg.stride(0) if B > 1 and N > 0 else N
        check(_lib.load().kge_dsampler_sample(
            self.table.data_ptr(), self.table.numel() * 8, idx.data_ptr(), B, N, int(row0), self._mode, self.seed,
            int(step), step_ptr, pos.data_ptr(), neg.data_ptr(), neg_ld, w.data_ptr(),
            torch.cuda.current_stream(dev).cuda_stream), "kge_dsampler_sample")
        return pos, neg, w

    def batches(self, batch_size, shuffle=True, generator=None, drop_last=True, row0=0, world=1):
        """Endless device batches (pos, neg, weight, mode) in the form Trainer.train_step consumes (mode: a host
        int64 tensor [B] of the mode code, as tfrecord.load_batches yields it). Each epoch's order is
        torch.randperm on the device (`generator`: a device torch.Generator; replicas seed theirs alike). With
        `world` replicas a global batch is world * batch_size consecutive entries of the order, and the replica
        whose rows start at `row0` (rank k: k * batch_size) takes its batch_size of them."""
        dev = self.device
        B, G = int(batch_size), int(batch_size) * int(world)
        if not 0 <= int(row0) <= G - B:
            raise ValueError("DeviceTrainDataset.batches: row0 outside the global batch")
        mode = torch.full((B,), self._mode, dtype=torch.int64)
        while True:
            order = (torch.randperm(self.len, device=dev, generator=generator) if shuffle
                     else torch.arange(self.len, device=dev))
            stop = self.len - self.len % G if drop_last else self.len
            for s in range(0, stop, G):
                idx = order[s + int(row0):min(s + int(row0) + B, stop)]
                pos, neg, w = self.sample(idx, row0=row0)
                yield pos, neg, w, mode[:idx.numel()]


def build_table(triples, nentity, nrelation):
    """The device sampler's true-answer table of `triples` [T, 3] as a host int64 array (kge_dsampler_table_build:
    layout in csrc/kge_dsampler.h), cut to the words in use."""
    triples = np.ascontiguousarray(np.asarray(triples, dtype=np.int64).reshape(-1, 3))
    lib = _lib.load()
    nbytes = int(lib.kge_dsampler_table_size(len(triples)))
    blob = np.empty(nbytes // 8, dtype=np.int64)
    check(lib.kge_dsampler_table_build(triples.ctypes.data, len(triples), int(nentity), int(nrelation),
                                       blob.ctypes.data, nbytes), "kge_dsampler_table_build")
    return blob[:int(blob[1])].copy()


class BidirectionalOneShotIterator:
    """upstream BidirectionalOneShotIterator: alternates head-batch and tail-batch batches."""

    def __init__(self, dataloader_head, dataloader_tail):
        self.iterator_head = iter(dataloader_head)
        self.iterator_tail = iter(dataloader_tail)
        self.step = 0

    def __iter__(self):
        return self

    def __next__(self):
        self.step += 1
        if self.step % 2 == 0:
            return next(self.iterator_head)
        return next(self.iterator_tail)
