"""PairRE beside its neighbours: the scoring step (kge_step_forward, the library's form) and the fused train step
(kge_train_step; kge_train_step_lazy for the large table) at B 512, N 256, alternating modes, for
  (a) D 1500, E 14 541, R 237: an FB15k-237-sized table, dense Adam;
  (b) D 200, E 2 500 000, R 535: a wikikg2-sized table, lazy Adam.
Arms per case: PairRE at D; TransE at the same D (the same gathered bytes per candidate); InterHT at the same entity
row bytes (per-half D / 2: strictly more arithmetic per byte). One process, arms interleaved, ROUNDS rounds of CALLS
calls of which the first round is dropped; a round's time is an event pair around its CALLS calls (device time per
call). One JSON line per (case, measure). No ratio is fixed in advance; "pairre_slower_than_interht_every_round"
is the one outcome DESIGN asks to be explained.
Usage: python scripts/pairre_probe.py [rounds] [calls]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from customknowledgegraphembedding_amd import _lib, ops  # noqa: E402
from customknowledgegraphembedding_amd._lib import FN_IDS  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
assert ROUNDS >= 3
dev = torch.device("cuda", 0)
B, N, GAMMA, LR = 512, 256, 12.0, 1e-3
CASES = [("fb15k237_sized_d1500", 14541, 237, 1500, False), ("wikikg2_sized_d200", 2500000, 535, 200, True)]


def arms(D):
    """name -> (per-half width, entity row width, relation row width, rel_off)"""
    return {"PairRE": (D, D, 2 * D, 0), "TransE": (D, D, D, 0), "InterHT": (D // 2, D, 3 * (D // 2), D // 2)}


class Arm:
    def __init__(self, name, E, R, D, lazy):
        self.name, self.E, self.R, self.lazy = name, E, R, lazy
        self.d, ew, rw, self.ro = arms(D)[name]
        self.fn, self.rng = FN_IDS[name], (GAMMA + 2.0) / self.d
        g = torch.Generator(device=dev).manual_seed(0)
        self.ent = (torch.rand(E, ew, generator=g, device=dev) * 2 - 1) * self.rng
        self.rel = torch.rand(R, rw, generator=g, device=dev) * 2 - 1
        self.mv = [torch.zeros_like(t) for t in (self.ent, self.ent, self.rel, self.rel)]
        self.w = torch.rand(B, generator=g, device=dev) + 0.2
        lib = _lib.load()
        size = lib.kge_train_step_lazy_workspace_size if lazy else lib.kge_train_step_workspace_size
        self.ws = torch.empty(size(self.fn, E, R, rw, B, N, self.d), dtype=torch.uint8, device=dev)
        self.out = torch.empty(2 * B + 5, dtype=torch.float32, device=dev)
        self.step_fn = lib.kge_train_step_lazy if lazy else lib.kge_train_step
        self.t = 0

    def score(self, pos, neg, mode):
        return ops.step_forward_raw(self.fn, mode, self.ent, self.rel, self.ro, pos, neg, self.d, GAMMA, self.rng)

    def train(self, pos, neg, mode):
        o = self.out.data_ptr()
        self.t += 1
        args = [self.fn, mode, self.ent.data_ptr(), self.E, self.ent.stride(0), self.rel.data_ptr(), self.R,
                self.rel.stride(0), self.ro, pos.data_ptr(), neg.data_ptr(), neg.stride(0), B, N, self.d, GAMMA,
                self.rng, 1.0, 1, 0, self.w.data_ptr(), o + 16, None, o + 20, o + 20 + 4 * B] + \
               [m.data_ptr() for m in self.mv] + \
               [LR, 0.9, 0.999, 1e-7, self.t, 1, self.ws.data_ptr(), self.ws.numel(),
                torch.cuda.current_stream(dev).cuda_stream] + ([None] if self.lazy else [])
        _lib.check(self.step_fn(*args), "kge_train_step")


def timed(fn, batches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(CALLS):
        pos, neg = batches[i % len(batches)]
        fn(pos, neg, i % 2)
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / CALLS, 4)


print(json.dumps({"build": _lib.build_id(), "device": torch.cuda.get_device_name(0), "rounds": ROUNDS,
                  "kept": ROUNDS - 1, "calls_per_round": CALLS, "B": B, "N": N}), flush=True)
for label, E, R, D, lazy in CASES:
    g = np.random.RandomState(1)
    batches = []
    for _ in range(4):
        pos = np.stack([g.randint(E, size=B), g.randint(R, size=B), g.randint(E, size=B)], 1)
        batches.append((torch.from_numpy(pos).to(dev), torch.from_numpy(g.randint(E, size=(B, N))).to(dev)))
    A = {name: Arm(name, E, R, D, lazy) for name in arms(D)}
    for measure in ("score_step", "train_step_lazy" if lazy else "train_step"):
        t = {name: [] for name in A}
        for _ in range(ROUNDS):
            for name, a in A.items():
                t[name].append(timed(a.score if measure == "score_step" else a.train, batches))
        kept = {name: v[1:] for name, v in t.items()}
        rec = {"case": label, "measure": measure, "E": E, "D": D, "entity_row_bytes": 4 * D,
               "candidate_rows_GB_per_call": round(B * (N + 2) * 4 * D / 1e9, 4)}
        for name, v in kept.items():
            rec[name + "_ms"] = v
            rec[name + "_median_ms"] = float(np.median(v))
        rec["pairre_over_transe"] = round(rec["PairRE_median_ms"] / rec["TransE_median_ms"], 3)
        rec["pairre_over_interht"] = round(rec["PairRE_median_ms"] / rec["InterHT_median_ms"], 3)
        rec["pairre_slower_than_interht_every_round"] = bool(min(kept["PairRE"]) > max(kept["InterHT"]))
        print(json.dumps(rec), flush=True)
    del A
    torch.cuda.empty_cache()
