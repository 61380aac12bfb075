"""Top-k link prediction of DistMult / ComplEx: four arms, one process, arms interleaved. Arm A is score_all +
torch.topk (no exclusion, so it does less); arm B is score_all + topk_rows (the [B, E] matrix: the path predict takes);
arm C is topk_planes (kge_eval_topk_planes, no matrix); for scale, rank_planes on the same queries. 1 024 and 4 096
query rows, k = 10 and 64, both modes, exclusion lists from the dataset's triples (tests/golden/*_ids.npz),
event-pair device time per call, ROUNDS rounds of which the first is dropped. Arms B and C are asserted equal (ids,
and scores bitwise). The comparison is C against B of the same run, by DESIGN §3.0's rule: a function and k go
through topk_planes only if, in both modes, every kept round of C beats every kept round of B and the median gain is
more than twice the larger of the two arms' ranges. At E = 123 182 the peak device memory of arms B and C
(torch.cuda.max_memory_allocated above the tables and planes) is recorded too.
Usage: python scripts/topk_planes_probe.py [rounds]"""
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
GOLDEN = os.path.join(ROOT, "tests", "golden")
dev = torch.device("cuda", 0)
# (label, dataset ids, model, d, gamma)
SHAPES = [("fb15k_DistMult_d1000", "fb15k_ids.npz", "DistMult", 1000, 24.0),
          ("fb15k_ComplEx_d1000", "fb15k_ids.npz", "ComplEx", 1000, 24.0),
          ("yago3_10_DistMult_d500", "yago3_10_ids.npz", "DistMult", 500, 24.0)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, out  # us


def verdict(b, c):
    gain = float(np.median(b) - np.median(c))
    return bool(max(c) < min(b) and gain > 2 * max(max(b) - min(b), max(c) - min(c)))


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


print(json.dumps({"build": _lib.build_id(), "device": torch.cuda.get_device_name(0), "rounds": ROUNDS,
                  "kept": ROUNDS - 1, "exclusion": "from the dataset's triples"}), flush=True)
for label, ids_file, name, d, gamma in SHAPES:
    z = np.load(os.path.join(GOLDEN, ids_file))
    triples, E, R = z["triples"].astype(np.int64), int(z["nentity"]), int(z["nrelation"])
    de = name == "ComplEx"
    m = kge.KGEModel(name, E, R, d, gamma, double_entity_embedding=de, double_relation_embedding=de, device=dev, seed=0)
    planes = evaluate.entity_planes(m)
    assert planes is not None
    for BQ in (1024, 4096):
        q = triples[::len(triples) // BQ][:BQ]
        pos = torch.from_numpy(q).to(dev)
        excl = {}
        for mode in ("head-batch", "tail-batch"):
            ptr, ids = evaluate.build_exclude(q, mode, triples)
            fptr, fids = evaluate.build_filter(q, mode, triples)
            excl[mode] = (torch.from_numpy(ptr).to(dev), torch.from_numpy(ids).to(dev), len(ids),
                          torch.from_numpy(fptr).to(dev), torch.from_numpy(fids).to(dev), len(fids),
                          pos[:, 0 if mode == "head-batch" else 2].contiguous())
        for K in (10, 64):
            rec = {"shape": label, "E": E, "d": d, "queries": BQ, "k": K}
            ok = True
            S = torch.empty((BQ, E), dtype=torch.float32, device=dev)
            t = {mode: {a: [] for a in ("A", "B", "C", "rank")} for mode in excl}
            for _ in range(ROUNDS):
                for mode, (xp, xi, nx, fp, fi, nf, truth) in excl.items():
                    fns = {"A": lambda: torch.topk(evaluate.score_all(m, pos, mode, out=S, planes=planes), K, dim=1),
                           "B": lambda: evaluate.topk_rows(evaluate.score_all(m, pos, mode, out=S, planes=planes), K,
                                                           xp, xi),
                           "C": lambda: evaluate.topk_planes(m, pos, mode, K, planes, xp, xi, nx),
                           "rank": lambda: evaluate.rank_planes(m, pos, mode, planes, truth, fp, fi, nf)}
                    out = {}
                    for a, fn in fns.items():
                        us, out[a] = timed(fn)
                        t[mode][a].append(round(us, 1))
                    assert torch.equal(out["B"][0], out["C"][0]) and torch.equal(
                        out["B"][1].view(torch.int32), out["C"][1].view(torch.int32)), f"{label}: B and C differ"
            del S
            for mode in excl:
                kept = {a: v[1:] for a, v in t[mode].items()}
                ok = ok and verdict(kept["B"], kept["C"])
                rec[mode] = {"nexcl": excl[mode][2], "A_matrix_torch_topk_us": kept["A"],
                             "B_matrix_topk_rows_us": kept["B"], "C_topk_planes_us": kept["C"],
                             "rank_planes_us": kept["rank"],
                             "medians_us": {a: float(np.median(v)) for a, v in kept.items()},
                             "B_range_us": round(max(kept["B"]) - min(kept["B"]), 1),
                             "C_range_us": round(max(kept["C"]) - min(kept["C"]), 1),
                             "rule_passes": verdict(kept["B"], kept["C"])}
            rec["topk_planes_is_default"] = ok
            if E > 100000:
                xp, xi, nx = excl["tail-batch"][:3]
                evaluate._TOPK_PLANES_WS.clear()
                rec["peak_bytes_B_matrix"] = peak(
                    lambda: evaluate.topk_rows(evaluate.score_all(m, pos, "tail-batch", planes=planes), K, xp, xi))
                rec["peak_bytes_C_topk_planes"] = peak(
                    lambda: evaluate.topk_planes(m, pos, "tail-batch", K, planes, xp, xi, nx))
            print(json.dumps(rec), flush=True)
    del m, planes
    evaluate._TOPK_PLANES_WS.clear()
    evaluate._Q_PLANES.clear()
    torch.cuda.empty_cache()
