#!/usr/bin/env python3
"""What the device negative sampler costs, and what it buys a train loop fed from a triple file (one GPU, one process).

  1. kge_dsampler_sample's device time at C2's batch (B 512, WN18RR's triples) with N 256 and N 1 024, both modes:
     device events around a captured graph of --launches launches replayed --replays times (a graph keeps the host
     out of the window; the figure still holds one kernel boundary per launch), and around the same number of eager
     launches (what a loop that launches it each step sees).
  2. Trainer steps per second at C2 (InterHT d 1 000, fused step) with the batches drawn from the triples
       host:   TrainDataset.batches(prefetch=2), head and tail alternating, pinned, copied by Trainer.train_step;
       device: DeviceTrainDataset.batches, head and tail alternating;
     each with a model and optimizer of its own, in alternating blocks of --steps steps (A B A B ...), each block
     timed by the host clock around work that ends in a device synchronise. The resident figure (the same step on
     one device-resident batch: what kge_train_step alone allows) is taken the same way.

Prints one line per figure; --out also writes them to a file. --kernel-only stops after part 1 (for a run under a
kernel trace)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import customknowledgegraphembedding_amd as kge  # noqa: E402
from customknowledgegraphembedding_amd.optim import Adam  # noqa: E402
from customknowledgegraphembedding_amd.sampler import (BidirectionalOneShotIterator, DeviceTrainDataset,  # noqa: E402
                                                       TrainDataset)
from customknowledgegraphembedding_amd.supervisor import Strategy, Sum, Trainer  # noqa: E402

DEV = "cuda"
MODES = ("head-batch", "tail-batch")


def kernel_times(triples, E, R, B, launches, replays, say):
    idx = torch.randperm(len(triples), device=DEV)[:B].contiguous()
    for N in (256, 1024):
        for mode in MODES:
            ds = DeviceTrainDataset(triples, E, R, N, mode, seed=1, device=DEV)
            out = (torch.empty((B, 3), dtype=torch.int64, device=DEV),
                   torch.empty((B, N), dtype=torch.int64, device=DEV), torch.empty(B, device=DEV))
            step = torch.zeros(1, dtype=torch.int64, device=DEV)
            for _ in range(10):
                ds.sample(idx, step=step, out=out)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(launches):
                    ds.sample(idx, step=step, out=out)
            graph.replay()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(replays):
                graph.replay()
            t1.record()
            torch.cuda.synchronize()
            us_graph = t0.elapsed_time(t1) * 1e3 / (launches * replays)
            t0.record()
            for _ in range(launches * replays):
                ds.sample(idx, step=step, out=out)
            t1.record()
            torch.cuda.synchronize()
            us_eager = t0.elapsed_time(t1) * 1e3 / (launches * replays)
            say(f"kernel B={B} N={N} {mode}: {us_graph:.2f} us per launch in a graph of {launches} "
                f"({B * N / us_graph / 1e3:.2f} G ids/s), {us_eager:.2f} us per eager launch back to back")


def pinned(it):
    for pos, neg, w, mode in it:
        yield pos.pin_memory(), neg.pin_memory(), w.pin_memory(), torch.tensor([0 if mode == MODES[0] else 1])


def train_rates(triples, E, R, B, N, steps, rounds, say):
    def trainer():
        m = kge.TFKGEModel("InterHT", E, R, 1000, 24.0, double_entity_embedding=True, triple_relation_embedding=True,
                           device=DEV, seed=0)
        tr = Trainer(Strategy(), None, m, Adam(m.parameters(), lr=5e-5), Sum())
        assert tr.fused
        return tr

    host = BidirectionalOneShotIterator(*[pinned(TrainDataset(triples, E, R, N, mode, seed=k)
                                                 .batches(B, rng=np.random.RandomState(k), prefetch=2))
                                          for k, mode in enumerate(MODES)])
    device = BidirectionalOneShotIterator(*[DeviceTrainDataset(triples, E, R, N, mode, seed=k, device=DEV)
                                            .batches(B, generator=torch.Generator(device=DEV).manual_seed(k))
                                            for k, mode in enumerate(MODES)])
    two = [next(device), next(device)]

    def resident():
        while True:
            yield from two

    runs = {"host": (trainer(), host), "device": (trainer(), device), "resident": (trainer(), resident())}
    for tr, it in runs.values():
        for _ in range(20):
            tr.train_step(it)
    torch.cuda.synchronize()
    rates = {k: [] for k in runs}
    for r in range(rounds):
        for name, (tr, it) in runs.items():
            t = time.perf_counter()
            for _ in range(steps):
                loss = tr.train_step(it)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            rates[name].append(steps / dt)
            say(f"train C2 InterHT d=1000 B={B} N={N} round {r} {name}: {steps / dt:.1f} steps/s "
                f"({dt / steps * 1e3:.3f} ms per step, loss {float(loss):.4f})")
    med = {k: float(np.median(v)) for k, v in rates.items()}
    say(f"train C2 medians over {rounds} rounds of {steps} steps: host {med['host']:.1f} steps/s "
        f"({1e3 / med['host']:.3f} ms), device {med['device']:.1f} steps/s ({1e3 / med['device']:.3f} ms), "
        f"resident {med['resident']:.1f} steps/s ({1e3 / med['resident']:.3f} ms); device / host = "
        f"{med['device'] / med['host']:.2f}x, device step - resident step = "
        f"{(1e3 / med['device'] - 1e3 / med['resident']) * 1e3:.1f} us")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dsampler_probe.py needs a GPU: nothing is measured without one")
    z = np.load(os.path.join(ROOT, "tests", "golden", "wn18rr_ids.npz"))
    triples, E, R = z["triples"].astype(np.int64), int(z["nentity"]), int(z["nrelation"])
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"{torch.cuda.get_device_name(0)}; {kge.build_id()['build_id']}; WN18RR {len(triples)} triples, E {E}, R {R}")
    t = time.perf_counter()
    DeviceTrainDataset(triples, E, R, 256, "tail-batch", device=DEV)
    say(f"table build + upload of {len(triples)} triples: {(time.perf_counter() - t) * 1e3:.0f} ms")
    kernel_times(triples, E, R, 512, a.launches, a.replays, say)
    if not a.kernel_only:
        train_rates(triples, E, R, 512, 256, a.steps, a.rounds, say)


if __name__ == "__main__":
    main()
