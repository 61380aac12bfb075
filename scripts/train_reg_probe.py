"""Upstream's train step with the L3 regulariser: KGEModel.train_step (autograd, torch.norm, dense d_ent, then
optim.Adam) against KGEModel.train_step_fused (one kge_train_step_reg call), both at lambda = 2e-6 with adversarial
sampling (temperature 1) and subsampling weights. One process, arms interleaved, ROUNDS rounds of STEPS steps each of
which the first round is dropped; a round's time is a host clock around STEPS steps that end in a device
synchronise (the log's .item() of either arm synchronises every step anyway). Batches: seeded random ids, modes
alternating. Two twin models per shape (same seed), so both arms start from the same tables.
Per shape one JSON line with the kept rounds' ms per step and DESIGN §3.0's rule: the fused call wins only if every
kept round of it beats every kept round of train_step and the median gain is more than twice its own range.
Then kge_train_step_reg at lambda = 2e-6 against lambda = 0 at C2's shape (InterHT d 1 000, E 40 943, B 512, N 256),
event-pair device time per step: what the regulariser itself costs the entity pass.
Usage: python scripts/train_reg_probe.py [rounds] [steps]"""
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import customknowledgegraphembedding_amd as kge  # noqa: E402
from customknowledgegraphembedding_amd import _lib  # noqa: E402
from customknowledgegraphembedding_amd._lib import FN_IDS  # noqa: E402
from customknowledgegraphembedding_amd.optim import Adam  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
assert ROUNDS >= 4
LAMBDA = 2e-6
dev = torch.device("cuda", 0)
# label, model, E, R, d, gamma, B, N
SHAPES = [("c4_yago310_DistMult_d500", "DistMult", 123182, 37, 500, 24.0, 512, 1024),
          ("fb15k_ComplEx_d1000", "ComplEx", 14951, 1345, 1000, 500.0, 512, 256)]


def batches(E, R, B, N, n, seed):
    g = np.random.RandomState(seed)
    out = []
    for i in range(n):
        pos = torch.from_numpy(np.stack([g.randint(E, size=B), g.randint(R, size=B), g.randint(E, size=B)], 1))
        neg = torch.from_numpy(g.randint(E, size=(B, N)))
        w = torch.from_numpy(g.uniform(0.1, 1.0, size=(B,))).float()
        out.append((pos.to(dev), neg.to(dev), w.to(dev), "head-batch" if i % 2 == 0 else "tail-batch"))
    return out


def verdict(a, b):
    """DESIGN §3.0 on the kept rounds: every round of b below every round of a, median gain > 2 x b's range."""
    gain = float(np.median(a) - np.median(b))
    return bool(max(b) < min(a) and gain > 2 * (max(b) - min(b)))


print(json.dumps({"build": _lib.build_id(), "device": torch.cuda.get_device_name(0), "rounds": ROUNDS,
                  "kept": ROUNDS - 1, "steps_per_round": STEPS, "lambda": LAMBDA}), flush=True)
args = types.SimpleNamespace(negative_adversarial_sampling=True, adversarial_temperature=1.0, uni_weight=False,
                             regularization=LAMBDA)
for label, name, E, R, d, gamma, B, N in SHAPES:
    cx = name == "ComplEx"
    models = [kge.KGEModel(name, E, R, d, gamma, double_entity_embedding=cx, double_relation_embedding=cx,
                           device=dev, seed=0) for _ in range(2)]
    opts = [Adam(m.parameters(), lr=1e-4, semantics="torch") for m in models]
    data = batches(E, R, B, N, STEPS, 1)
    steps = (kge.KGEModel.train_step, kge.KGEModel.train_step_fused)
    t = ([], [])
    logs = [None, None]
    for _ in range(ROUNDS):
        for arm in (0, 1):
            it = iter(data)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                logs[arm] = steps[arm](models[arm], opts[arm], it, args)
            torch.cuda.synchronize()
            t[arm].append(round((time.perf_counter() - t0) / STEPS * 1e3, 4))
    a, b = t[0][1:], t[1][1:]
    drift = max(float((x - y).abs().max()) for x, y in zip(models[0].parameters(), models[1].parameters()))
    print(json.dumps({"shape": label, "E": E, "d": d, "B": B, "N": N,
                      "train_step_ms": a, "train_step_fused_ms": b,
                      "train_step_median_ms": float(np.median(a)), "train_step_fused_median_ms": float(np.median(b)),
                      "fused_range_ms": round(max(b) - min(b), 4), "rule_passes": verdict(a, b),
                      "last_log_train_step": logs[0], "last_log_fused": logs[1],
                      "tables_max_abs_diff_after_all_steps": drift}), flush=True)
    del models, opts, data
    torch.cuda.empty_cache()

# what the regulariser costs the step itself: kge_train_step_reg at C2's shape, lambda 2e-6 against 0
E, R, D, B, N, gamma = 40943, 11, 1000, 512, 256, 24.0
lib = _lib.load()
data = batches(E, R, B, N, STEPS, 2)
arms = {}
for key in ("lambda_0", "lambda_2e-6"):
    m = kge.TFKGEModel("InterHT", E, R, D, gamma, True, False, True, device=dev, seed=0)
    mv = [torch.zeros_like(p) for p in (m.entity_embedding, m.entity_embedding, m.relation_embedding,
                                         m.relation_embedding)]
    arms[key] = (m, mv)
nbytes = lib.kge_train_step_reg_workspace_size(FN_IDS["InterHT"], E, R, 3 * D, B, N, D)
ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
out = torch.empty(2 * B + 5, dtype=torch.float32, device=dev)
st = torch.cuda.current_stream(dev).cuda_stream


def reg_steps(key, lam, t0):
    m, mv = arms[key]
    ent, rel = m.entity_embedding.data, m.relation_embedding.data
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i, (pos, neg, w, mode) in enumerate(data):
        rc = lib.kge_train_step_reg(
            FN_IDS["InterHT"], 0 if mode == "head-batch" else 1, ent.data_ptr(), E, ent.stride(0), rel.data_ptr(), R,
            rel.stride(0), D, pos.data_ptr(), neg.data_ptr(), neg.stride(0), B, N, D, gamma, m._range_f, 1.0, 1, 1,
            w.data_ptr(), out[4:].data_ptr(), None, out[5:].data_ptr(), out[5 + B:].data_ptr(), mv[0].data_ptr(),
            mv[1].data_ptr(), mv[2].data_ptr(), mv[3].data_ptr(), 1e-4, 0.9, 0.999, 1e-8, t0 + i + 1, 0, ws.data_ptr(),
            ws.numel(), st, lam, out.data_ptr())
        _lib.check(rc, "kge_train_step_reg")
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / len(data), 4)


t = {"lambda_0": [], "lambda_2e-6": []}
for r in range(ROUNDS):
    t["lambda_0"].append(reg_steps("lambda_0", 0.0, r * STEPS))
    t["lambda_2e-6"].append(reg_steps("lambda_2e-6", LAMBDA, r * STEPS))
a, b = t["lambda_0"][1:], t["lambda_2e-6"][1:]
print(json.dumps({"shape": "c2_wn18rr_InterHT_d1000", "E": E, "d": D, "B": B, "N": N, "lambda_0_ms": a,
                  "lambda_2e-6_ms": b, "lambda_0_median_ms": float(np.median(a)),
                  "lambda_2e-6_median_ms": float(np.median(b)),
                  "regulariser_cost_ms": round(float(np.median(b) - np.median(a)), 4),
                  "log": out[:4].tolist()}), flush=True)
