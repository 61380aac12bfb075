"""Candidate-list ranks, fused against the composition it replaces: evaluate.rank_candidates (kge_eval_rank_candidates,
one launch) and the three-step path (the fused scorer's [M, C + 1] matrix of [truth | candidates], then the count
by torch comparisons on the device), one process, arms interleaved, ROUNDS rounds of CALLS calls of which the first
round is dropped; a round's time is an event pair around its CALLS calls (device time per call). Both arms read
the same tables, queries and lists (seeded uniform ids, no padding: every entry is gathered); the composition's
[truth | candidates] id matrix is made before the clock starts, and its ranks are checked against the fused call's.
Per shape one JSON line: the kept rounds' ms per call, the gathered bytes computed from the shape (M (C + 1)
candidate rows and M query rows of the entity table), the GB/s that makes, and DESIGN §3.0's rule (the fused call
wins only if every kept round of it is below every kept round of the composition and the median gain is more than
twice the larger of the two ranges).
Usage: python scripts/rank_candidates_probe.py [rounds] [calls]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from customknowledgegraphembedding_amd import _lib, evaluate, ops  # noqa: E402
from customknowledgegraphembedding_amd._lib import FN_IDS  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
assert ROUNDS >= 3
dev = torch.device("cuda", 0)
# label, model, E, R, per-half width D, entity / relation row widths in D, rel_off in D, gamma, M, C
SHAPES = [("wikikg2_sized_InterHT_d200", "InterHT", 2500000, 535, 200, 2, 3, 1, 12.0, 4096, 500),
          ("fb15k237_sized_RotatE_d1000", "RotatE", 14541, 237, 1000, 2, 1, 0, 24.0, 4096, 1000),
          ("yago310_sized_DistMult_d500", "DistMult", 123182, 37, 500, 1, 1, 0, 24.0, 4096, 500)]


class Tables:
    """What evaluate.rank_candidates reads of a model, with the tables drawn on the device."""

    def __init__(self, shape):
        _, name, E, R, D, em, rm, ro, gamma, _, _ = shape
        self.model_name, self._D, self._gamma_f, self._rel_off = name, D, gamma, ro * D
        self._range_f = (gamma + 2.0) / D
        g = torch.Generator(device=dev).manual_seed(0)
        self.entity_embedding = (torch.rand(E, em * D, generator=g, device=dev) * 2 - 1) * self._range_f
        self.relation_embedding = (torch.rand(R, rm * D, generator=g, device=dev) * 2 - 1) * self._range_f

    def score(self, mode, pos, neg):
        return ops.score_indexed_raw(FN_IDS[self.model_name], ops.mode_id(mode), self.entity_embedding,
                                     self.relation_embedding, self._rel_off, pos, neg, self._D, self._gamma_f,
                                     self._range_f)


def composition(m, mode, pos, both, truth, E):
    s = m.score(mode, pos, both)
    ids = both[:, 1:]
    counted = (ids >= 0) & (ids < E) & (ids != truth.unsqueeze(1))
    return 1 + ((s[:, 1:] > s[:, :1]) & counted).sum(1)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / CALLS, 4), out


def verdict(a, b):
    """DESIGN §3.0 on the kept rounds: every round of b below every round of a, median gain > 2 x the larger range."""
    gain = float(np.median(a) - np.median(b))
    return bool(max(b) < min(a) and gain > 2 * max(max(a) - min(a), max(b) - min(b)))


print(json.dumps({"build": _lib.build_id(), "device": torch.cuda.get_device_name(0), "rounds": ROUNDS,
                  "kept": ROUNDS - 1, "calls_per_round": CALLS}), flush=True)
for shape in SHAPES:
    label, name, E, R, D, em, rm, ro, gamma, M, C = shape
    m = Tables(shape)
    g = np.random.RandomState(1)
    pos = torch.from_numpy(np.stack([g.randint(E, size=M), g.randint(R, size=M), g.randint(E, size=M)], 1)).to(dev)
    cand = torch.from_numpy(g.randint(E, size=(M, C))).to(dev)
    mode = "tail-batch"
    truth = pos[:, 2].contiguous()
    both = torch.cat([truth.unsqueeze(1), cand], 1).contiguous()
    t = ([], [])
    for _ in range(ROUNDS):
        ta, ra = timed(lambda: composition(m, mode, pos, both, truth, E))
        tb, rb = timed(lambda: evaluate.rank_candidates(m, pos, mode, cand, truth))
        t[0].append(ta)
        t[1].append(tb)
    a, b = t[0][1:], t[1][1:]
    gathered = (M * (C + 1) + M) * em * D * 4
    print(json.dumps({"shape": label, "E": E, "d": D, "M": M, "C": C, "table_GB": round(E * em * D * 4 / 1e9, 3),
                      "gathered_GB": round(gathered / 1e9, 3), "composition_ms": a, "fused_ms": b,
                      "composition_median_ms": float(np.median(a)), "fused_median_ms": float(np.median(b)),
                      "composition_GBps": round(gathered / 1e6 / float(np.median(a)), 1),
                      "fused_GBps": round(gathered / 1e6 / float(np.median(b)), 1),
                      "gain_ms": round(float(np.median(a) - np.median(b)), 4),
                      "composition_range_ms": round(max(a) - min(a), 4), "fused_range_ms": round(max(b) - min(b), 4),
                      "every_fused_round_below_every_composition_round": bool(max(b) < min(a)),
                      "fused_rule_passes": verdict(a, b), "composition_rule_passes": verdict(b, a),
                      "same_ranks": bool(torch.equal(ra, rb))}), flush=True)
    del m, cand, both
    torch.cuda.empty_cache()
