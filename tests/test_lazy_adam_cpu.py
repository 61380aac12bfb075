"""The lazy train step without a GPU: the fp64 reference of tests/lazy_adam_ref.py against torch.optim.SparseAdam,
kge_train_step_lazy's host layer (its rejections sit ahead of the first device call, so dummy pointers reach them,
as in test_train_reg_cpu.py; its size query needs no device), and the Python refusals on CPU models."""
import importlib.util
import itertools
import os
import types

import pytest
import torch

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import _lib
from customknowledgegraphembedding_amd.optim import Adam
from customknowledgegraphembedding_amd.supervisor import Sum, Trainer
from tests import lazy_adam_ref as R

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_abi_matrix", os.path.join(GOLDEN_DIR, "make_abi_matrix.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

KGE_EINVAL, KGE_ENOTSUP = -22, -95  # include/kge_hip.h
P, BIG = 4096, 1 << 40  # a dummy non-null pointer (never dereferenced: every case is refused first)


# ------------------------------------------------------------------------------------------------
# 1. the reference is torch.optim.SparseAdam (Keras form, eps 1e-8)
# ------------------------------------------------------------------------------------------------
def test_reference_is_sparse_adam():
    """Four steps in fp64 on a [12, 5] table: repeated rows (SparseAdam sums them, as the dense gradient does), a
    row named with a gradient that is exactly zero (touched: its moments decay and it moves), rows named in one
    step and not the next, rows never named. Bar 1e-15 (the issue's; it measured 5.6e-17)."""
    g0 = torch.Generator().manual_seed(3)
    rows, w, lr = 12, 5, 1e-2
    p0 = torch.randn(rows, w, generator=g0, dtype=torch.float64)
    prm = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SparseAdam([prm], lr=lr, betas=(R.B1, R.B2), eps=1e-8)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    steps = [[1, 1, 4, 7, 11], [4, 7, 7, 7, 0], [2, 4, 9, 9, 1], [11, 0, 4, 4, 7]]
    for t, idx in enumerate(steps, start=1):
        idx = torch.tensor(idx)
        val = torch.randn(len(idx), w, generator=g0, dtype=torch.float64)
        if t == 2:
            val[idx == 7] = 0.0  # row 7: named three times with a gradient of exactly zero (its moments decay)
        prm.grad = torch.sparse_coo_tensor(idx[None, :], val, (rows, w))
        opt.step()
        dense = torch.zeros(rows, w, dtype=torch.float64).index_add_(0, idx, val)
        mask = torch.zeros(rows, dtype=torch.bool)
        mask[idx] = True
        p, m, v = R.adam_rows(p, dense, m, v, t, lr, mask, keras=True, epsilon=1e-8)
    st = opt.state[prm]
    assert float((prm.detach() - p).abs().max()) <= 1e-15
    assert float((st["exp_avg"] - m).abs().max()) <= 1e-15 and float((st["exp_avg_sq"] - v).abs().max()) <= 1e-15
    never = [3, 5, 6, 8, 10]
    assert torch.equal(p[never], p0[never]) and not bool(m[never].any())
    # the dense rule moves the rows the lazy one leaves: the two references differ
    pd, md, vd = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    pl, ml, vl = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    g1 = torch.zeros(rows, w, dtype=torch.float64)
    g1[1] = 1.0
    only1 = torch.zeros(rows, dtype=torch.bool)
    only1[1] = True
    for t, (g, mask) in enumerate([(g1, only1), (torch.zeros_like(g1), ~only1)], start=1):
        pd, md, vd = R.adam_rows(pd, g, md, vd, t, lr, None, keras=True)
        pl, ml, vl = R.adam_rows(pl, g, ml, vl, t, lr, mask, keras=True)
    assert float((pd[1] - pl[1]).abs().max()) > 1e-3 and float(ml[1].abs().max()) > float(md[1].abs().max())


def test_touched_masks_drop_out_of_range_ids():
    pos = torch.tensor([[0, 1, 5], [9, 3, 9]])
    neg = torch.tensor([[-1, 10, 1 << 40], [2, 2, 9]])
    ent, rel = R.touched_masks(pos, neg, 10, 4)
    assert ent.nonzero().reshape(-1).tolist() == [0, 2, 5, 9] and rel.tolist() == [False, True, False, True]


def test_torch_rule_is_torch_adam():
    g0 = torch.Generator().manual_seed(5)
    p0 = torch.randn(7, 3, generator=g0, dtype=torch.float64)
    prm = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([prm], lr=1e-2, betas=(R.B1, R.B2), eps=1e-8)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for t in (1, 2, 3):
        g = torch.randn(7, 3, generator=g0, dtype=torch.float64)
        prm.grad = g.clone()
        opt.step()
        p, m, v = R.adam_rows(p, g, m, v, t, 1e-2, None, keras=False)
    assert float((prm.detach() - p).abs().max()) <= 1e-15


# ------------------------------------------------------------------------------------------------
# 2. the host layer
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _call(lib, fn=1, mode=1, B=2, N=4, D=4, ent=P, w=P, step=1, log=P, wsb=BIG):
    rc = lib.kge_train_step_lazy(fn, mode, ent, 10, 8, P, 2, 12, 0, P, P, 4, B, N, D, 1.0, 1.0, 1.0, 1, 1, w, P, None,
                                 P, P, P, P, P, P, 0.001, 0.9, 0.999, 1e-8, step, 0, P, wsb, None, log)
    return rc, lib.kge_last_error().decode()


def test_rejections_and_their_order(lib):
    """kge_train_step's rejections, in its order; each case also carries the fault of the NEXT check, which must not
    be the one reported."""
    assert _call(lib, fn=9, mode=7)[0] == KGE_EINVAL and "mode" in _call(lib, fn=9, mode=7)[1]
    assert "unknown score function" in _call(lib, fn=9)[1]
    rc, msg = _call(lib, fn=5, mode=3)
    assert rc == KGE_ENOTSUP and "pRotatE" in msg
    assert _call(lib, mode=3, B=0) == (KGE_EINVAL, "kge_train_step needs a negative mode (0 or 1)")
    assert _call(lib, B=0, step=0) == (KGE_EINVAL, "bad shape")
    assert _call(lib, N=0, step=0) == (KGE_EINVAL, "bad shape")
    assert _call(lib, step=0, ent=None) == (KGE_EINVAL, "step is 1-based")
    assert _call(lib, step=-3) == (KGE_EINVAL, "step is 1-based")
    assert _call(lib, ent=None, wsb=16) == (KGE_EINVAL, "null pointer")
    assert _call(lib, B=1 << 20, N=1 << 12, wsb=16)[1] == "too many gradient events for 32-bit codes"
    assert _call(lib, wsb=16) == (KGE_EINVAL, "workspace too small")
    assert _call(lib, D=4096)[0] != 0
    # NULL weights are uni_weight and a NULL log is no log, as in kge_train_step_reg: on to the workspace check
    assert _call(lib, w=None, wsb=16) == (KGE_EINVAL, "workspace too small")
    assert _call(lib, log=None, wsb=16) == (KGE_EINVAL, "workspace too small")


def test_workspace_size_covers_the_plain_step(lib):
    n = 0
    for fn, D, B, N, E in itertools.product(M.FNS, M.DS, M.BS, M.NS, M.ES):
        a = dict(M.sweep_queries(fn, D, B, N, E))["kge_train_step_workspace_size"]
        plain = lib.kge_train_step_workspace_size(*a)
        lazy = lib.kge_train_step_lazy_workspace_size(*a)
        assert (lazy == -1) == (plain == -1) and lazy >= plain, a
        # the list (min(E, events) ints), its count and the tiles' counts come on top of kge_train_step_reg's
        reg = lib.kge_train_step_reg_workspace_size(*a)
        assert plain == -1 or lazy >= reg + 4 * min(E, B * N + 3 * B) + 4, a
        n += 1
    assert n == 6 * 8 * 4 * 5 * 3
    for a in ([7, 10, 3, 8, 2, 4, 8], [0, 10, 3, 8, -2, 4, 8], [0, -1, 3, 8, 2, 4, 8]):
        assert lib.kge_train_step_lazy_workspace_size(*a) == lib.kge_train_step_workspace_size(*a) == -1, a
    plain = lib.kge_train_step_workspace_size(1, 10, 2, 12, 2, 4, 4)
    assert lib.kge_train_step_lazy_workspace_size(1, 10, 2, 12, 2, 4, 4) > plain
    assert _call(lib, wsb=plain) == (KGE_EINVAL, "workspace too small")


def test_signatures_present(lib):
    for sym in ("kge_train_step_lazy", "kge_train_step_lazy_workspace_size"):
        assert sym in _lib.SIGNATURES and getattr(lib, sym) is not None
    args = _lib.SIGNATURES["kge_train_step_lazy"][1]
    plain = _lib.SIGNATURES["kge_train_step"][1]
    assert args[:len(plain)] == plain and len(args) == len(plain) + 1  # kge_train_step's list, then the log
    assert _lib.SIGNATURES["kge_train_step_lazy_workspace_size"] == _lib.SIGNATURES["kge_train_step_workspace_size"]
    assert lib.kge_abi_version() == 1


# ------------------------------------------------------------------------------------------------
# 3. Python: the flag and the refusals, on CPU models (nothing can be launched: every refusal comes first)
# ------------------------------------------------------------------------------------------------
def _batch(E=20, R=3, B=2, N=4):
    pos = torch.tensor([[1, 0, 2], [3, 2, 4]])[:B]
    neg = torch.arange(B * N).reshape(B, N) % E
    return pos, neg, torch.ones(B), "tail-batch"


def _args(reg=0.0):
    return types.SimpleNamespace(negative_adversarial_sampling=True, adversarial_temperature=1.0, uni_weight=False,
                                 regularization=reg)


def test_adam_stores_the_flag_and_step_refuses_a_lazy_group():
    p = torch.nn.Parameter(torch.zeros(4, 2))
    assert Adam([p]).param_groups[0]["lazy"] is False
    opt = Adam([p], lr=1e-3, lazy=True)
    assert opt.param_groups[0]["lazy"] is True and opt.param_groups[0]["semantics"] == "keras"
    p.grad = torch.ones_like(p)
    with pytest.raises(NotImplementedError, match="train_step_fused"):
        opt.step()
    assert not opt.state[p] and bool((p == 0).all())


def test_tf_model_refusals():
    pos, neg, w, _ = _batch()
    m = kge.TFKGEModel("DistMult", 20, 3, 8, 9.0, device="cpu", seed=1)
    opt = Adam(m.parameters(), lr=1e-3, lazy=True)
    with pytest.raises(ValueError, match="one_call"):
        m.train_step_fused(pos, neg, w, 1, opt, one_call=False)
    p = kge.TFKGEModel("pRotatE", 20, 3, 8, 9.0, device="cpu", seed=1)
    popt = Adam(p.parameters(), lr=1e-3, lazy=True)
    with pytest.raises(NotImplementedError, match="pRotatE"):
        p.train_step_fused(pos, neg, w, 1, popt)
    with pytest.raises(NotImplementedError, match="pRotatE"):
        p.train_step_fused(pos, neg, w, 1, popt, one_call=False)
    for model, o in ((m, opt), (p, popt)):
        assert all(not o.state[q] for q in model.parameters())
    assert m.supports_fused_step and p.supports_fused_step  # unchanged by the flag


def test_upstream_model_refusals():
    m = kge.KGEModel("DistMult", 20, 3, 8, 9.0, device="cpu", seed=1)
    opt = Adam(m.parameters(), lr=1e-3, lazy=True)
    it = iter([_batch()])
    with pytest.raises(ValueError, match="regulari"):
        kge.KGEModel.train_step_fused(m, opt, it, _args(reg=2e-6))
    assert next(it, None) is not None  # refused before the batch was drawn
    p = kge.KGEModel("pRotatE", 20, 3, 8, 9.0, device="cpu", seed=1)
    with pytest.raises(NotImplementedError):
        kge.KGEModel.train_step_fused(p, Adam(p.parameters(), lr=1e-3, lazy=True), iter([_batch()]), _args())
    assert all(not opt.state[q] for q in m.parameters())


def test_trainer_refuses_a_lazy_optimizer_on_several_replicas():
    m = kge.TFKGEModel("DistMult", 20, 3, 8, 9.0, device="cpu", seed=1)
    two = types.SimpleNamespace(num_replicas_in_sync=2)
    with pytest.raises(NotImplementedError, match="single-replica"):
        Trainer(two, [], m, Adam(m.parameters(), lr=1e-3, lazy=True), Sum())
    one = types.SimpleNamespace(num_replicas_in_sync=1)
    t = Trainer(one, [], m, Adam(m.parameters(), lr=1e-3, lazy=True), Sum())
    d = Trainer(one, [], m, Adam(m.parameters(), lr=1e-3), Sum())
    assert (t.fused, t.one_call) == (d.fused, d.one_call) == (True, True)  # the choice of path does not change
