"""The host layer of libkge_hip.so answers what it answered before its dispatch was refactored (CPU only).

tests/golden/abi_matrix.json was recorded by tests/golden/make_abi_matrix.py from a build of the commit before
the refactor (its "recorded_from" names it) and is never regenerated from the code under test, with one kind of
exception: a change that alters an answer on purpose re-records the file and reviews the difference entry by entry
(last: the sharded train step's width refusal, one message changed and four cases added, nothing else). It holds
the library's own output for
  (a) the size and order queries over all six functions x D {4 .. 2048} x B {0 .. 512} x N {1 .. 65536} x
      nentity {0, 1000, 2^28};
  (b) kge_step_planner_get of every `what` after each valid and invalid set_form / set_lead / set_board /
      set_sweep on planners made on dummy pointers;
  (c) the return code and kge_last_error text of one call per argument rejection that sits ahead of its entry
      point's first device call (dummy pointers, as in test_abi.py), the ones inside run_score and pick_vg
      included, and of the empty-problem no-ops.
The calls themselves are defined once, in make_abi_matrix.py (answers()); the file holds the answers only. The
current build is asked the same, in the same order, and must answer the same.

fail() sites of kge_abi.hip NOT covered, and why:
  after a launch or a memset of the same call (reaching them with dummy pointers would run a kernel on them):
    every check_launch(...) HIP error; step_backward_impl's pick_vg (after the score-gradient launches) and the
    run_score calls below it; kge_train_step's and the sharded calls' later run_score rejections;
    kge_step_backward_adam's kge_adam_update of the modulus;
  unreachable today, because every caller filters the case earlier (they guard run_score against new callers):
    run_score "bad shape (B, N, D)" (each entry point checks its shape first), "tile plan missing" (run only
    after tile_plan succeeded), "dimension too large" (pick_vg rejects G > 8 first), "the streaming backward
    needs G % 4 == 0" (chosen only when it holds), "no kernel for this (function, width) combination" (no such
    combination passes the checks above it); kge_eval_query's "no eval-query kernel for this width" (V and G are
    bounded before it) and kge_eval_query_planes' "dimension too large" (V is 4 and pick_vg passed);
    kge_step_planner_set_form's "this wave count changes the rows per group" (the rows per group are bounded by
    the list and query images, which do not depend on the wave count, at every shape found);
  kge_step_planner_set_clocks' argument checks (a -DKGE_PROFILING_KNOBS build only: this build answers
    KGE_ENOTSUP, which is covered).
"""
import importlib.util
import json
import os

import pytest

from customknowledgegraphembedding_amd import _lib

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_abi_matrix", os.path.join(GOLDEN_DIR, "make_abi_matrix.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN_DIR, "abi_matrix.json")) as f:
        return M.unpack(json.load(f))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_size_and_order_queries(golden, lib):
    got, want = M.size_answers(lib), golden["sizes"]
    grid = 8 * 4 * 5 * 3
    assert sorted(want["sweep"]) == sorted(s for s, _ in M.sweep_queries(0, 4, 0, 1, 0))
    for sym, per_fn in want["sweep"].items():
        assert len(per_fn) == 6 and all(isinstance(v, int) or len(v) == grid for v in per_fn), sym
        assert got["sweep"][sym] == per_fn, sym
    assert len(want["small"]) == len(M.SMALL_QUERIES)
    bad = [(q, g, w) for q, g, w in zip(M.SMALL_QUERIES, got["small"], want["small"]) if g != w]
    assert not bad, bad[:5]


def test_planner_form_choices(golden, lib):
    got = M.planner_answers(lib)
    assert len(golden["planners"]) == len(M.PLANNERS)
    for shape, (need, steps), (want_need, want_steps) in zip(M.PLANNERS, got, golden["planners"]):
        assert need == want_need and len(want_steps) == 1 + len(M.PLANNER_OPS), shape
        bad = [(op, g, w) for op, g, w in zip([("create", None)] + M.PLANNER_OPS, steps, want_steps) if g != w]
        assert not bad, (shape, bad[:5])


def test_rejections_ahead_of_a_device_call(golden, lib):
    cases, want = M.rejection_cases(), golden["rejections"]
    assert len(cases) == len(want) >= 400 and len({m for rc, m in want if rc}) >= 75
    bad = [(c, g, tuple(w)) for c, w in zip(cases, want) if (g := M.run_case(lib, *c)) != tuple(w)]
    assert not bad, bad[:5]
