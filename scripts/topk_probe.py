"""Top-k link prediction of the distance models: three ways to the k best entities per query, one process, arms
interleaved. Arm A is score_all + torch.topk (what a caller without the library's top-k can do; no exclusion, so it
does less); arm B is score_all + topk_rows (kge_topk_rows on the [B, E] matrix); arm C is topk_sweep
(kge_eval_topk_sweep, no matrix). For scale, rank_sweep on the same queries. 1 024 query rows, k = 10, exclusion lists
from the dataset's triples (tests/golden/*_ids.npz), both modes, event-pair device time per batch and mode, ROUNDS
rounds of which the first is dropped. Arms B and C are asserted equal (ids, and scores bitwise). Per shape one JSON
line with the kept rounds' times and the default rule of DESIGN §3.0: predict sends a function through the sweep only
if every kept round of arm C beats every kept round of arm B and the median gain is more than twice the larger of the
two arms' ranges (per mode).
Usage: python scripts/topk_probe.py [rounds]"""
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
BQ, K = 1024, 10
GOLDEN = os.path.join(ROOT, "tests", "golden")
dev = torch.device("cuda", 0)
# (label, dataset ids, model, per-half width d, gamma)
SHAPES = [("wn18rr_InterHT_d1000", "wn18rr_ids.npz", "InterHT", 1000, 24.0),
          ("fb15k237_RotatE_d1000", "fb15k237_ids.npz", "RotatE", 1000, 9.0),
          ("wn18rr_TransE_d500", "wn18rr_ids.npz", "TransE", 500, 6.0),
          ("wn18rr_pRotatE_d500", "wn18rr_ids.npz", "pRotatE", 500, 6.0)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, out  # us


def verdict(b, c):
    """DESIGN §3.0 on one mode's kept rounds (us): every C below every B, median gain > 2 x the larger range."""
    gain = float(np.median(b) - np.median(c))
    return bool(max(c) < min(b) and gain > 2 * max(max(b) - min(b), max(c) - min(c)))


print(json.dumps({"build": _lib.build_id(), "device": torch.cuda.get_device_name(0), "rounds": ROUNDS,
                  "kept": ROUNDS - 1, "queries": BQ, "k": K}), flush=True)
for label, ids_file, name, d, gamma in SHAPES:
    z = np.load(os.path.join(GOLDEN, ids_file))
    triples, E, R = z["triples"].astype(np.int64), int(z["nentity"]), int(z["nrelation"])
    if name == "InterHT":
        m = kge.TFKGEModel(name, E, R, d, gamma, True, False, True, device=dev, seed=0)
    else:
        m = kge.KGEModel(name, E, R, d, gamma, double_entity_embedding=name == "RotatE", device=dev, seed=0)
    q = triples[::len(triples) // BQ][:BQ]
    pos = torch.from_numpy(q).to(dev)
    S = torch.empty((BQ, E), dtype=torch.float32, device=dev)
    arms = {}
    for mode in ("head-batch", "tail-batch"):
        ptr, ids = evaluate.build_exclude(q, mode, triples)
        xp, xi, nx = torch.from_numpy(ptr).to(dev), torch.from_numpy(ids).to(dev), len(ids)
        fptr, fids = evaluate.build_filter(q, mode, triples)
        fp, fi, nf = torch.from_numpy(fptr).to(dev), torch.from_numpy(fids).to(dev), len(fids)
        truth = pos[:, 0 if mode == "head-batch" else 2].contiguous()
        arms[mode] = (nx, {
            "A": lambda mode=mode: torch.topk(evaluate.score_all(m, pos, mode, out=S), K, dim=1),
            "B": lambda mode=mode, xp=xp, xi=xi: evaluate.topk_rows(evaluate.score_all(m, pos, mode, out=S), K, xp, xi),
            "C": lambda mode=mode, xp=xp, xi=xi, nx=nx: evaluate.topk_sweep(m, pos, mode, K, xp, xi, nx),
            "rank": lambda mode=mode, truth=truth, fp=fp, fi=fi, nf=nf:
            evaluate.rank_sweep(m, pos, mode, truth, fp, fi, nf)})
    t = {mode: {a: [] for a in ("A", "B", "C", "rank")} for mode in arms}
    equal = True
    for _ in range(ROUNDS):
        for mode, (nx, fns) in arms.items():
            out = {}
            for a, fn in fns.items():
                us, out[a] = timed(fn)
                t[mode][a].append(round(us, 1))
            assert out["C"] is not None, "no sweep kernel for this shape"
            equal = equal and bool(torch.equal(out["B"][0], out["C"][0])) and bool(
                torch.equal(out["B"][1].view(torch.int32), out["C"][1].view(torch.int32)))
    assert equal, f"{label}: topk_rows and topk_sweep differ"
    rec = {"shape": label, "E": E, "d": d, "gamma": gamma, "k": K, "rows_equal_sweep": equal}
    ok = True
    for mode in arms:
        kept = {a: v[1:] for a, v in t[mode].items()}
        ok = ok and verdict(kept["B"], kept["C"])
        rec[mode] = {"nexcl": arms[mode][0], "A_matrix_torch_topk_us": kept["A"], "B_matrix_topk_rows_us": kept["B"],
                     "C_topk_sweep_us": kept["C"], "rank_sweep_us": kept["rank"],
                     "medians_us": {a: float(np.median(v)) for a, v in kept.items()},
                     "B_range_us": round(max(kept["B"]) - min(kept["B"]), 1),
                     "C_range_us": round(max(kept["C"]) - min(kept["C"]), 1),
                     "rule_passes": verdict(kept["B"], kept["C"])}
    rec["sweep_is_default"] = ok
    print(json.dumps(rec), flush=True)
    del m, arms, S
    torch.cuda.empty_cache()
