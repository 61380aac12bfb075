"""The planned tile sweep's L2 window: (1) `skew`: how far apart the 32 blocks that sweep one entity slice run
(needs a -DKGE_PROFILING_KNOBS library, KGE_HIP_LIB=abtmp/knobs/libkge_hip.so: kge_step_planner_set_clocks); (2)
`forms`: the sweep forms (waves x candidate rows in flight per wave) and the lead throttle against the 12 x 2 /
16 x 2 sweep without a board, selected through the planner's setters in one process; (3) `tune`: leads between 8
and 24 and the board's own cost. Device us per step, events around 300 steps after 50 warmup, rounds
interleaved, same batches as bench.py; outputs compared bitwise.
(4) `timeline` (the same profiling library): where a planned step's launch spends its time outside the sweep.
`timeline=ROWS`: the same at ROWS rows per group (StepPlanner.set_rows; -1: the library's row rule).
Usage: python scripts/window_probe.py skew [wl..] | timeline[=ROWS] [wl..] | forms [wl..] | tune [wl..]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from customknowledgegraphembedding_amd import ops  # noqa: E402
from customknowledgegraphembedding_amd._lib import FN_IDS, check  # noqa: E402

bench.ops = ops  # bench.py binds its module-level `ops` only inside main(); StepRunner needs it (as sweep_probe.py)
dev = torch.device("cuda", 0)
ROUNDS = 6  # round 1 is dropped
# the clock record (csrc/kge_internal.h): per scoring block CLK_MARKS int64 words (the per-wave pairs from CLK_WAVE
# on), then two per plan block
CLK_WAVE = 8
CLK_MARKS = CLK_WAVE + 2 * 16


def set_clocks(p, B):
    """Hands the planner a zeroed clock record; returns (row groups, the record). After the planner's first plan:
    it chooses its rows per group there."""
    rows = p.form()["rows"]
    assert rows > 0, "set_clocks before the planner's first plan: its rows per group are not chosen yet"
    groups = (B + rows - 1) // rows  # the library refuses a buffer smaller than its own count
    clk = torch.zeros(groups * (8 * CLK_MARKS + 2), dtype=torch.int64, device=dev)
    assert p._lib.kge_step_planner_set_clocks(p._h, clk.data_ptr(), clk.numel() * 8 - 8) != 0
    check(p._lib.kge_step_planner_set_clocks(p._h, clk.data_ptr(), clk.numel() * 8), "kge_step_planner_set_clocks")
    return groups, clk


def timed(f, n=300, warm=50):
    for i in range(warm):
        f(i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(warm, warm + n):
        f(i)
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / n * 1e3, 2)


def runner(m, batches, fn, waves, depth, lead):
    r = bench.StepRunner(m, batches, fn, planned=True)
    r.planner.set_form(waves, depth)
    r.planner.set_lead(lead)
    return r


def skew(wl):
    """Per sweep form: the spread (max - min, us) over a slice's blocks of the clock at the sweep's start, at
    entity buckets 64 / 128 / 192 and at its end, median and worst slice, over 6 sampled steps of both
    directions; the blocks' sweep durations; and whether a slice's blocks share one XCC."""
    w = bench.WORKLOADS[wl]
    m, batches = bench.make_inputs(w, 0, dev)
    fn = FN_IDS[w["fn"]]
    for waves, depth, lead in ((12, 2, 0), (12, 1, 0), (16, 1, 0), (12, 2, 16), (16, 2, 0)):
        r = runner(m, batches, fn, waves, depth, lead)
        p = r.planner
        for i in range(40):
            r(i)
        groups, clk = set_clocks(p, w["B"])
        spreads, durs, one_xcc = [], [], True
        for i in range(40, 46):
            clk.zero_()
            r(i)
            torch.cuda.synchronize()
            c = clk[:8 * groups * CLK_MARKS].view(8, groups, CLK_MARKS)[:, :, :6].cpu()
            t = c[:, :, :5].double() / 100.0  # 100 MHz ticks -> us
            seen = (c[:, :, :5] > 0).all(1)
            sp = t.max(1).values - t.min(1).values  # [slice, mark]
            spreads.append(torch.where(seen, sp, torch.full_like(sp, float("nan"))))
            durs.append(t[:, :, 4] - t[:, :, 0])
            one_xcc = one_xcc and all(len(set(c[x, :, 5].tolist())) == 1 for x in range(8))
        s = torch.stack(spreads)  # [step, slice, mark]
        d = torch.stack(durs)
        print(json.dumps({
            "workload": w["name"], "waves": waves, "depth": depth, "lead": lead, "form": p.form(),
            "marks": ["start", "bucket 64", "bucket 128", "bucket 192", "end"],
            "spread_us_median_over_slices": [round(float(s[:, :, k].nanmedian()), 2) for k in range(5)],
            "spread_us_worst_slice": [round(float(torch.nan_to_num(s[:, :, k], nan=0.0).max()), 2) for k in range(5)],
            "per_step_median_spread_us": [[round(float(s[i, :, k].nanmedian()), 2) for k in range(5)] for i in range(6)],
            "block_sweep_us": {"min": round(float(d.min()), 2), "median": round(float(d.median()), 2),
                               "max": round(float(d.max()), 2),
                               "rel_sigma_within_slice": round(float((d.std(2) / d.mean(2)).median()), 4)},
            "slice_blocks_share_one_xcc": one_xcc}), flush=True)


def timeline(wl, rows=None):
    """The planned step's launch as a timeline, in the library's own sweep form: per mark, the median and the worst
    (latest) block, in us after the step's earliest block entry, over six sampled steps of both modes; the plan
    (tail) blocks' earliest and latest entry and exit; the latest exit of any block."""
    w = bench.WORKLOADS[wl]
    m, batches = bench.make_inputs(w, 0, dev)
    r = bench.StepRunner(m, batches, FN_IDS[w["fn"]], planned=True)
    if rows is not None:
        r.planner.set_rows(rows)
    for i in range(40):
        r(i)
    groups, clk = set_clocks(r.planner, w["B"])
    nsc = 8 * groups
    marks = {k: [] for k in ("sweep_start", "wave0_sweep_end", "last_wave_sweep_end", "block_exit")}
    plan_in, plan_out, last = [], [], []
    for i in range(40, 46):
        clk.zero_()
        r(i)
        torch.cuda.synchronize()
        c = clk.cpu().double() / 100.0  # 100 MHz ticks -> us
        blk = c[:nsc * CLK_MARKS].view(nsc, CLK_MARKS)
        per_wave = blk[:, CLK_WAVE:].view(nsc, 16, 2)
        t0 = float(blk[:, 6].min())
        assert t0 > 0, "no clock marks: the library is not a -DKGE_PROFILING_KNOBS build of this source"
        marks["sweep_start"].append(blk[:, 0] - t0)
        marks["wave0_sweep_end"].append(blk[:, 4] - t0)
        marks["last_wave_sweep_end"].append(per_wave[:, :, 0].max(1).values - t0)
        marks["block_exit"].append(per_wave[:, :, 1].max(1).values - t0)
        entry = blk[:, 6] - t0
        pb = c[nsc * CLK_MARKS:nsc * CLK_MARKS + 2 * groups].view(groups, 2)
        pb = pb[pb[:, 0] > 0] - t0  # (the last sampled step plans a batch like every other)
        if len(pb):
            plan_in.append(pb[:, 0])
            plan_out.append(pb[:, 1])
        last.append(max(float(marks["block_exit"][-1].max()), float(pb[:, 1].max()) if len(pb) else 0.0))
        marks.setdefault("block_entry", []).append(entry)

    def mw(v):
        s = torch.stack(v)  # [step, block]
        return {"median": round(float(s.median()), 2), "worst": round(float(s.max()), 2),
                "worst_median_over_steps": round(float(s.max(1).values.median()), 2)}
    out = {"workload": w["name"], "form": r.planner.form(), "us_after_earliest_block_entry": {k: mw(v) for k, v in marks.items()}}
    if plan_in:
        pi, po = torch.cat(plan_in), torch.cat(plan_out)
        out["plan_blocks"] = {"entry_earliest": round(float(pi.min()), 2), "entry_latest": round(float(pi.max()), 2),
                              "exit_earliest": round(float(po.min()), 2), "exit_latest": round(float(po.max()), 2),
                              "entries_of_last_sampled_step": [round(float(v), 1) for v in plan_in[-1].sort().values]}
    out["latest_exit_of_any_block"] = {"median_over_steps": round(statistics.median(last), 2), "max": round(max(last), 2)}
    print(json.dumps(out), flush=True)
    del m, batches
    torch.cuda.empty_cache()


def forms(wl, tune=False):
    w = bench.WORKLOADS[wl]
    m, batches = bench.make_inputs(w, 0, dev)
    fn = FN_IDS[w["fn"]]
    base = runner(m, batches, fn, 0, 2, 0).planner.form()["waves"]  # the parent's form: the row width's waves x 2
    if tune:  # the lead between 8 and 32, and the board's own cost (lead 255: read and written, never a nap)
        variants = [("parent", base, 2, 0), (f"{base}x2 lead 255", base, 2, 255)]
        variants += [(f"{base}x2 lead {ld}", base, 2, ld) for ld in (8, 10, 12, 14, 16, 18, 20, 24)]
    else:
        variants = [("parent", base, 2, 0), ("12x1", 12, 1, 0), ("16x1", 16, 1, 0)]
        variants += [(f"{base}x2 lead {ld}", base, 2, ld) for ld in (4, 8, 16, 32)]
        variants += [("12x1 lead 16", 12, 1, 16), ("16x1 lead 16", 16, 1, 16)]
    res = {k: [] for k, *_ in variants}
    outs = {}
    for rnd in range(ROUNDS):
        for key, waves, depth, lead in variants:
            r = runner(m, batches, fn, waves, depth, lead)
            res[key].append(timed(r))
            if rnd == 0:
                got = [r(1000 + k) for k in range(2)]
                torch.cuda.synchronize()
                outs[key] = [[t.clone() for t in o] for o in got]
    eq = all(torch.equal(torch.nan_to_num(x), torch.nan_to_num(y)) for k in outs
             for a, b in zip(outs["parent"], outs[k]) for x, y in zip(a, b))
    par = res["parent"][1:]
    noise = max(par) - min(par)
    verdict = {}
    for k, v in res.items():
        if k == "parent":
            continue
        gain = statistics.median(par) - statistics.median(v[1:])
        # kept only if every round beats every parent round and the median gain exceeds twice the parent's range
        verdict[k] = {"median_gain_us": round(gain, 2), "passes": bool(max(v[1:]) < min(par) and gain > 2 * noise)}
    print(json.dumps({"workload": w["name"], "rounds_us (round 1 dropped for the verdict)": res,
                      "parent_max_minus_min": round(noise, 2), "verdict": verdict, "bitwise_equal": eq}), flush=True)
    del m, batches
    torch.cuda.empty_cache()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "forms"
    what, _, rows = what.partition("=")
    for wl in (sys.argv[2:] or (["c2", "c3", "c4"] if what in ("forms", "timeline") else ["c2"])):
        if what == "skew":
            skew(wl)
        elif what == "timeline":
            timeline(wl, int(rows) if rows else None)
        else:
            forms(wl, tune=what == "tune")
