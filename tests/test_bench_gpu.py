"""bench.py's plain run on the GPU: `--steps K` times K steps and the line carries the headline keys and none of
the --full sections; `--dump-outputs DIR` writes the LAST timed step's outputs (what StepRunner returned for
step warmup + K - 1: batch (warmup + K - 1) % 8 in mode (warmup + K - 1) % 2), float32, bitwise those of the
unplanned step on the same batch (ops.step_forward_raw; the planned step is bitwise that one,
test_planned_gpu.py)."""
import json

import numpy as np
import pytest
import torch

import bench
from customknowledgegraphembedding_amd import ops
from customknowledgegraphembedding_amd._lib import FN_IDS

pytestmark = pytest.mark.gpu


def test_plain_run_line_and_dumped_outputs(tmp_path, capsys):
    steps, warmup = 3, 2
    out = tmp_path / "dump"
    assert not bench.main(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(out)])
    (line,) = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert line["metric"] == bench.METRIC and line["unit"] == "triples/s" and line["dtype"] == "f32"
    assert line["higher_is_better"] is True and line["steps"] == steps and line["warmup"] == warmup
    w = bench.WORKLOADS["c2"]
    B, N = w["B"], w["N"]
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx((B * N + B) / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert not {"roofline", "train_step", "cpu_baseline", "yago3_10_rowshard", "yago3_10_shard_sim8"} & set(line)
    assert sorted(p.name for p in out.iterdir()) == sorted(n + ".npy" for n in bench.STEP_OUTPUTS)
    got = {n: np.load(out / (n + ".npy")) for n in bench.STEP_OUTPUTS}
    assert all(x.dtype == np.float32 for x in got.values())
    assert got["neg_scores"].shape == (B, N) and all(got[n].shape == (B,) for n in bench.STEP_OUTPUTS if n != "neg_scores")
    # the same step again, from the same seeded inputs
    m, batches = bench.make_inputs(w, 0, torch.device("cuda", 0))
    last = warmup + steps - 1
    pos, neg = batches[last % len(batches)]
    ref = ops.step_forward_raw(FN_IDS[w["fn"]], last % 2, m.entity_embedding.detach(), m.relation_embedding.detach(),
                               m._rel_off, pos, neg, m._D, m._gamma_f, m._range_f)
    for n, r in zip(bench.STEP_OUTPUTS, ref):
        assert np.array_equal(got[n], r.cpu().numpy(), equal_nan=True), n
