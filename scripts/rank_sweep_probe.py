"""Filtered ranks of the distance models: the score-matrix path against the sweep, one process, arms interleaved.
Arm A is rank_filtered(score_all(...)) (kge_score_indexed over candidates 0..E-1, the [B, E] matrix, rank_kernel);
arm B is rank_sweep (kge_eval_rank_sweep). 1 024 query rows and a filter from the dataset's triples
(tests/golden/*_ids.npz), both modes, event-pair device time per batch and mode, ROUNDS rounds of which the first is
dropped. The two arms' ranks are asserted equal. Per shape one JSON line with the kept rounds' times, queries/s of
both arms, and the default rule of DESIGN §3.0: the sweep is test_step's default for a function only if every kept
round of arm B beats every kept round of arm A and the median gain is more than twice arm B's own range (per mode).
Usage: python scripts/rank_sweep_probe.py [rounds]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import customknowledgegraphembedding_amd as kge  # noqa: E402
from customknowledgegraphembedding_amd import _lib, evaluate  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 8
assert ROUNDS >= 6
BQ = 1024
GOLDEN = os.path.join(ROOT, "tests", "golden")
dev = torch.device("cuda", 0)
# (label, dataset ids, model, per-half width d, gamma)
SHAPES = [("wn18rr_InterHT_d1000", "wn18rr_ids.npz", "InterHT", 1000, 24.0),
          ("fb15k237_RotatE_d1000", "fb15k237_ids.npz", "RotatE", 1000, 9.0),
          ("wn18rr_TransE_d500", "wn18rr_ids.npz", "TransE", 500, 6.0),
          ("wn18rr_pRotatE_d500", "wn18rr_ids.npz", "pRotatE", 500, 6.0)]
NQ = {"TransE": 1, "pRotatE": 1, "RotatE": 2, "InterHT": 3}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, out  # us


def verdict(a, b):
    """DESIGN §3.0 on one mode's kept rounds (us): every B below every A, median gain > 2 x B's range."""
    gain = float(np.median(a) - np.median(b))
    return bool(max(b) < min(a) and gain > 2 * (max(b) - min(b)))


print(json.dumps({"build": _lib.build_id(), "device": torch.cuda.get_device_name(0), "rounds": ROUNDS,
                  "kept": ROUNDS - 1, "queries": BQ}), flush=True)
for label, ids_file, name, d, gamma in SHAPES:
    z = np.load(os.path.join(GOLDEN, ids_file))
    triples, E, R = z["triples"].astype(np.int64), int(z["nentity"]), int(z["nrelation"])
    if name == "InterHT":
        m = kge.TFKGEModel(name, E, R, d, gamma, True, False, True, device=dev, seed=0)
    else:
        m = kge.KGEModel(name, E, R, d, gamma, double_entity_embedding=name == "RotatE", device=dev, seed=0)
    q = triples[::len(triples) // BQ][:BQ]
    pos = torch.from_numpy(q).to(dev)
    arms = {}
    for mode in ("head-batch", "tail-batch"):
        ptr, ids = evaluate.build_filter(q, mode, triples)
        truth = pos[:, 0 if mode == "head-batch" else 2].contiguous()
        fptr, fids = torch.from_numpy(ptr).to(dev), torch.from_numpy(ids).to(dev)
        nf = len(ids)
        arms[mode] = (nf,
                      lambda mode=mode, truth=truth, fptr=fptr, fids=fids:
                      evaluate.rank_filtered(evaluate.score_all(m, pos, mode), truth, fptr, fids),
                      lambda mode=mode, truth=truth, fptr=fptr, fids=fids, nf=nf:
                      evaluate.rank_sweep(m, pos, mode, truth, fptr, fids, nf))
    t = {mode: {"A": [], "B": []} for mode in arms}
    equal = True
    for _ in range(ROUNDS):
        for mode, (nf, arm_a, arm_b) in arms.items():
            ta, ra = timed(arm_a)
            tb, rb = timed(arm_b)
            assert rb is not None, "no sweep kernel for this shape"
            equal = equal and bool(torch.equal(ra, rb))
            t[mode]["A"].append(round(ta, 1))
            t[mode]["B"].append(round(tb, 1))
    assert equal, f"{label}: the two arms' ranks differ"
    # kge_eval_rank_sweep's rows-per-block rule restated (16-B rows: V = 4, G the power of two >= d / 256)
    G = 1
    while G * 256 < d:
        G *= 2
    row_bytes = NQ[name] * G * 64 * 16 + 8
    rows = min(16, BQ, 144 * 1024 // row_bytes)
    rec = {"shape": label, "E": E, "d": d, "gamma": gamma, "ranks_equal": equal, "rows_per_block": rows,
           "sweep_lds_bytes": rows * row_bytes}
    ok = True
    for mode in arms:
        a, b = t[mode]["A"][1:], t[mode]["B"][1:]
        ok = ok and verdict(a, b)
        rec[mode] = {"nfilter": arms[mode][0], "A_matrix_us": a, "B_sweep_us": b,
                     "A_median_us": float(np.median(a)), "B_median_us": float(np.median(b)),
                     "B_range_us": round(max(b) - min(b), 1), "rule_passes": verdict(a, b)}
    ma = sum(rec[mode]["A_median_us"] for mode in arms)
    mb = sum(rec[mode]["B_median_us"] for mode in arms)
    rec["A_matrix_Mqps"] = round(2 * BQ / ma, 4)  # ranked queries per us = M queries/s, both modes
    rec["B_sweep_Mqps"] = round(2 * BQ / mb, 4)
    rec["sweep_is_default"] = ok
    print(json.dumps(rec), flush=True)
    del m, arms
    torch.cuda.empty_cache()
