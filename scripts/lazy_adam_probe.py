"""The lazy train step against the dense one: kge_train_step_lazy and kge_train_step through the C ABI, one process,
arms interleaved, ROUNDS rounds of STEPS steps of which the first round is dropped; a round's time is an event pair
around its STEPS calls (device time per step). Each arm has its own tables and moments (drawn on the device, same
seed), so each trains its own model; batches are seeded uniform ids with modes alternating.
Per shape one JSON line: the kept rounds' ms per step, the share of rows a batch touches, and DESIGN §3.0's rule (the
lazy step wins only if every kept round of it is below every kept round of the dense step and the median gain is
more than twice the larger of the two ranges).
Then, for the shapes given with --breakdown (default: the E 2.5 M shape and its E 5 M twin), the device time of each
launch of one lazy and one dense step (torch.profiler, averaged over STEPS steps): what still follows the table
(the counters' reset, the bucket scan, the two list kernels) is on record there.
Usage: python scripts/lazy_adam_probe.py [rounds] [steps] [--no-breakdown]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from customknowledgegraphembedding_amd import _lib  # noqa: E402
from customknowledgegraphembedding_amd._lib import FN_IDS  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
ROUNDS = int(argv[0]) if len(argv) > 0 else 6
STEPS = int(argv[1]) if len(argv) > 1 else 20
BREAKDOWN = "--no-breakdown" not in sys.argv
assert ROUNDS >= 3
dev = torch.device("cuda", 0)
# label, model, E, R, per-half width D, entity / relation row widths in D, rel_off in D, gamma, B, N
SHAPES = [("c2_wn18rr_InterHT_d1000", "InterHT", 40943, 11, 1000, 2, 3, 1, 24.0, 512, 256),
          ("c4_yago310_DistMult_d500", "DistMult", 123182, 37, 500, 1, 1, 0, 24.0, 512, 1024),
          ("wikikg2_sized_InterHT_d200", "InterHT", 2500000, 535, 200, 2, 3, 1, 12.0, 512, 256)]
BREAKDOWN_SHAPES = [SHAPES[2], ("5M_InterHT_d200", "InterHT", 5000000, 535, 200, 2, 3, 1, 12.0, 512, 256)]
lib = _lib.load()
st = torch.cuda.current_stream(dev).cuda_stream


def batches(E, R, B, N, n, seed):
    g = np.random.RandomState(seed)
    out = []
    for i in range(n):
        pos = torch.from_numpy(np.stack([g.randint(E, size=B), g.randint(R, size=B), g.randint(E, size=B)], 1))
        neg = torch.from_numpy(g.randint(E, size=(B, N)))
        w = torch.from_numpy(g.uniform(0.1, 1.0, size=(B,))).float()
        out.append((pos.to(dev), neg.to(dev), w.to(dev), i % 2))
    return out


class Arm:
    def __init__(self, shape, lazy):
        _, name, E, R, D, em, rm, ro, gamma, B, N = shape
        self.shape, self.lazy, self.fn = shape, lazy, FN_IDS[name]
        self.rng = (gamma + 2.0) / D
        g = torch.Generator(device=dev).manual_seed(0)
        self.ent = (torch.rand(E, em * D, generator=g, device=dev) * 2 - 1) * self.rng
        self.rel = (torch.rand(R, rm * D, generator=g, device=dev) * 2 - 1) * self.rng
        self.mv = [torch.zeros_like(t) for t in (self.ent, self.ent, self.rel, self.rel)]
        size = lib.kge_train_step_lazy_workspace_size if lazy else lib.kge_train_step_workspace_size
        self.ws = torch.empty(size(self.fn, E, R, rm * D, B, N, D), dtype=torch.uint8, device=dev)
        self.out = torch.empty(2 * B + 5, dtype=torch.float32, device=dev)
        self.t = 0

    def step(self, pos, neg, w, mode):
        _, name, E, R, D, em, rm, ro, gamma, B, N = self.shape
        o, mv = self.out, self.mv
        args = [self.fn, mode, self.ent.data_ptr(), E, em * D, self.rel.data_ptr(), R, rm * D, ro * D, pos.data_ptr(),
                neg.data_ptr(), N, B, N, D, gamma, self.rng, 1.0, 1, 0, w.data_ptr(), o[4:].data_ptr(), None,
                o[5:].data_ptr(), o[5 + B:].data_ptr(), mv[0].data_ptr(), mv[1].data_ptr(), mv[2].data_ptr(),
                mv[3].data_ptr(), 1e-4, 0.9, 0.999, 1e-7, self.t + 1, 1, self.ws.data_ptr(), self.ws.numel(), st]
        rc = lib.kge_train_step_lazy(*args, None) if self.lazy else lib.kge_train_step(*args)
        _lib.check(rc, "kge_train_step_lazy" if self.lazy else "kge_train_step")
        self.t += 1

    def round(self, data):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for b in data:
            self.step(*b)
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / len(data), 4)


def verdict(a, b):
    """DESIGN §3.0 on the kept rounds: every round of b below every round of a, median gain > 2 x the larger range."""
    gain = float(np.median(a) - np.median(b))
    return bool(max(b) < min(a) and gain > 2 * max(max(a) - min(a), max(b) - min(b)))


def touched_share(data, E):
    return float(np.mean([torch.unique(torch.cat([n.reshape(-1), p[:, 0], p[:, 2]])).numel() / E
                          for p, n, _, _ in data]))


print(json.dumps({"build": _lib.build_id(), "device": torch.cuda.get_device_name(0), "rounds": ROUNDS,
                  "kept": ROUNDS - 1, "steps_per_round": STEPS}), flush=True)
for shape in SHAPES:
    label, name, E, R, D, em, rm, ro, gamma, B, N = shape
    data = batches(E, R, B, N, STEPS, 1)
    dense, lazy = Arm(shape, False), Arm(shape, True)
    t = ([], [])
    for _ in range(ROUNDS):
        t[0].append(dense.round(data))
        t[1].append(lazy.round(data))
    a, b = t[0][1:], t[1][1:]
    print(json.dumps({"shape": label, "E": E, "d": D, "B": B, "N": N, "rows_touched_share": touched_share(data, E),
                      "table_GB": round(E * em * D * 4 / 1e9, 3), "dense_ms": a, "lazy_ms": b,
                      "dense_median_ms": float(np.median(a)), "lazy_median_ms": float(np.median(b)),
                      "gain_ms": round(float(np.median(a) - np.median(b)), 4),
                      "dense_range_ms": round(max(a) - min(a), 4), "lazy_range_ms": round(max(b) - min(b), 4),
                      "every_lazy_round_below_every_dense_round": bool(max(b) < min(a)),
                      "rule_passes": verdict(a, b),
                      "loss_dense_lazy": [float(dense.out[4]), float(lazy.out[4])]}), flush=True)
    del dense, lazy, data
    torch.cuda.empty_cache()

if BREAKDOWN:
    from torch.profiler import ProfilerActivity, profile

    for shape in BREAKDOWN_SHAPES:
        label, name, E, R, D, em, rm, ro, gamma, B, N = shape
        data = batches(E, R, B, N, STEPS, 2)
        for lazy in (False, True):
            arm = Arm(shape, lazy)
            arm.round(data)  # warm
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                arm.round(data)
            rows = [(k.key[:90], round(getattr(k, "device_time_total", getattr(k, "cuda_time_total", 0.0))
                                        / len(data), 2), k.count // len(data) if k.count >= len(data) else k.count)
                    for k in prof.key_averages()]
            rows = sorted([r for r in rows if r[1] > 0], key=lambda r: -r[1])
            print(json.dumps({"breakdown": label, "E": E, "arm": "lazy" if lazy else "dense",
                              "us_per_step_by_launch": rows,
                              "us_per_step_sum": round(sum(r[1] for r in rows), 1)}), flush=True)
            del arm
            torch.cuda.empty_cache()
