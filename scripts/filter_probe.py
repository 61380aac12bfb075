#!/usr/bin/env python3
"""What building the evaluation filter costs on the host and on the device (one GPU, one process, no input from
outside the tree).

Two shapes, synthetic ids from a fixed RandomState with a Zipf tail column so that the (r, t) lists are skewed:
  fb15k   592 213 true triples, 59 071 queries (the last of them), E 14 951, R 1 345
  wn18rr   93 003 true triples,  3 134 queries,                    E 40 943, R 11
Both arms make the filter CSR of every query in both modes, interleaved A B A B ... in one process: one warm-up
round, then --rounds kept rounds, torch.cuda.synchronize() around each arm, the host clock around that:
  A  evaluate.build_filter, head-batch and tail-batch (the host path: dicts of sets, a Python loop over queries)
  B  evaluate.FilterTable(triples) (the host build by two sorts plus the upload) and .csr for both modes
B's CSR is checked against A's once per shape. Then test_step's whole wall time under filter_on="host" and
"device" for DistMult d 1 000 at the fb15k shape (--step-rounds each, interleaved, after one warm-up of each).

Prints one line per figure; --out also writes them to a file."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import customknowledgegraphembedding_amd as kge  # noqa: E402
from customknowledgegraphembedding_amd import evaluate  # noqa: E402

DEV = "cuda"
MODES = ("head-batch", "tail-batch")
SHAPES = {"fb15k": (592213, 59071, 14951, 1345), "wn18rr": (93003, 3134, 40943, 11)}


def make(T, E, R, seed):
    g = np.random.RandomState(seed)
    tail = (g.zipf(1.3, size=T) - 1) % E  # a few tails hold most triples: long (r, t) lists
    return np.stack([g.randint(E, size=T), g.randint(R, size=T), tail], 1).astype(np.int64)


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def arm_host(queries, triples):
    return [evaluate.build_filter(queries, m, triples) for m in MODES]


def arm_device(queries, triples):
    table = evaluate.FilterTable(triples, device=DEV)
    return [table.csr(queries, m, drop_own=True) for m in MODES]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--shapes", default="fb15k,wn18rr")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("filter_probe.py needs a GPU: nothing is measured without one")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"{torch.cuda.get_device_name(0)}; {kge.build_id()['build_id']}")
    data = {}
    for k, name in enumerate(a.shapes.split(",")):
        T, M, E, R = SHAPES[name]
        triples = make(T, E, R, 17 + k)
        queries = np.ascontiguousarray(triples[-M:])
        data[name] = (triples, queries, E, R)
        times = {"A": [], "B": []}
        for r in range(-1, a.rounds):  # round -1: the warm-up, not kept
            ta, host = clock(lambda: arm_host(queries, triples))
            tb, dev = clock(lambda: arm_device(queries, triples))
            if r < 0:
                for (hp, hi), (dp, di, dh) in zip(host, dev):
                    assert np.array_equal(hp, dh) and np.array_equal(hp, dp.cpu().numpy())
                    assert np.array_equal(hi, di.cpu().numpy())
                say(f"{name}: T {T}, M {M}, E {E}, R {R}; filter ids head-batch {len(host[0][1])}, tail-batch "
                    f"{len(host[1][1])}, longest list {max(int(np.diff(p).max()) for p, _ in host)}; device CSR equals "
                    f"build_filter's; warm-up A {ta * 1e3:.0f} ms, B {tb * 1e3:.1f} ms")
                continue
            times["A"].append(ta)
            times["B"].append(tb)
            say(f"{name} round {r}: A build_filter x2 {ta * 1e3:.0f} ms, B FilterTable + csr x2 {tb * 1e3:.1f} ms")
        A, B = np.array(times["A"]), np.array(times["B"])
        say(f"{name} medians over {a.rounds} rounds: A {np.median(A) * 1e3:.0f} ms, B {np.median(B) * 1e3:.1f} ms, "
            f"A / B = {np.median(A) / np.median(B):.0f}x; every B below every A: {bool(B.max() < A.min())} "
            f"(max B {B.max() * 1e3:.1f} ms, min A {A.min() * 1e3:.0f} ms)")
        # where B's time goes: the host build and upload against the device calls
        table = evaluate.FilterTable(triples, device=DEV)
        qd = torch.from_numpy(queries).to(DEV)
        t_build = min(clock(lambda: evaluate.FilterTable(triples, device=DEV))[0] for _ in range(3))
        t_csr = min(clock(lambda: [table.csr(qd, m) for m in MODES])[0] for _ in range(5))
        say(f"{name} parts of B (best of a few): table build + upload {t_build * 1e3:.1f} ms "
            f"({table.table.numel() * 8 / 1e6:.1f} MB), csr x2 on resident queries {t_csr * 1e3:.2f} ms")
    if a.no_step or "fb15k" not in data:
        return
    triples, queries, E, R = data["fb15k"]
    m = kge.KGEModel("DistMult", E, R, 1000, 12.0, device=DEV, seed=0)
    table = evaluate.FilterTable(triples, device=DEV)
    arms = {"host": lambda: evaluate.test_step(m, queries, triples, filter_on="host"),
            "device": lambda: evaluate.test_step(m, queries, triples, filter_on="device"),
            "device, table reused": lambda: evaluate.test_step(m, queries, table)}
    got = {}
    times = {k: [] for k in arms}
    for r in range(-1, a.step_rounds):
        for k, fn in arms.items():
            t, met = clock(fn)
            got.setdefault(k, met)
            assert met == got["host"], (k, met, got["host"])
            if r >= 0:
                times[k].append(t)
                say(f"test_step DistMult d=1000 fb15k shape round {r} filter {k}: {t * 1e3:.0f} ms")
    say("test_step DistMult d=1000 fb15k shape, 118 142 ranked queries, medians: " +
        ", ".join(f"{k} {np.median(v) * 1e3:.0f} ms" for k, v in times.items()) + f"; same metrics ({got['host']})")


if __name__ == "__main__":
    main()
