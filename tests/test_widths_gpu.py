"""Every (vector width V, register depth G) instance of the backward, train-step and forward kernels against the
fp64 oracle. launch_v / launch_g (csrc/kge_device.h) instantiate each kernel for V in {4, 2, 1} x G in
{1, 2, 4, 8}; pick_vg (csrc/kge_abi.hip) picks V from D, the leading dimensions and the base alignment. The
widths below reach the instances the rest of the suite does not: V4 G2, V2 G1 / G2 / G4 / G8 and every V = 1
instance, which is where bwd_rows_kernel hands over to bwd_stream_kernel + bwd_chain_kernel and bwd_ent_kernel
to bwd_ent_stream_kernel (G a multiple of 4), and where kge_train_step's fused forward (step_fwd_grad_kernel +
step_epilogue_kernel, G <= 4) hands over to its fallback.

Reference: torch.autograd in fp64 on O.tf_train_loss (supervisor.py:17-25) over the same fp32 values, and
O.keras_adam_step (supervisor.py:26). Bars, the project's own for the same quantities: scores and losses
rel_close <= 1e-4 (tests/conftest.py), gradients _grad_close (1e-4 of the reference's largest magnitude,
tests/test_parity_gpu.py), tables after Adam within 5e-2 * lr (tests/test_train_gpu.py). First moments are
linear in the gradients and take the gradient bar."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import ops
from customknowledgegraphembedding_amd._lib import FN_IDS
from customknowledgegraphembedding_amd.optim import Adam
from oracle import kge_oracle as O
from tests import strided as S
from tests.conftest import rel_close
from tests.test_parity_gpu import _grad_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
LR = 1e-3
FNS = S.FNS
# per-half width -> the (V, G) instance dense 16-B aligned tables get
WIDTHS = {33: (1, 1), 101: (1, 2), 255: (1, 4), 511: (1, 8), 50: (2, 1), 250: (2, 2), 450: (2, 4), 1022: (2, 8),
          300: (4, 2)}
SMALL = (40, 5, 6, 24)   # E, R, B, N
HOT = (3, 5, 40, 160)    # ~2 200 events per entity: phase 2's block-wide sort and its ordered extraction


def _dev(c):
    return (c["ent"].to(DEV), c["rel"].to(DEV), c["pos"].to(DEV), c["neg"].to(DEV), c["w"].to(DEV))


def _check_instance(c, ent, rel):
    assert S.table_vg(c["name"], c["D"], ent, rel) == {**WIDTHS, 64: (4, 1)}[c["D"]]


@functools.lru_cache(maxsize=None)
def _ref(name, D, mode, shape=SMALL, useful=False):
    """(case, loss, d_ent, d_rel, d_modulus) of one train step's loss in fp64; computed once per case and shared
    by the tests that compare against it (they only read it)."""
    E, R, B, N = shape
    c = S.make_case(name, D, E, R, B, N, seed=D)
    e = c["ent"].double().requires_grad_(True)
    r = c["rel"].double().requires_grad_(True)
    mod = torch.tensor(c["mod"], dtype=torch.float64, requires_grad=(name == "pRotatE"))
    loss = O.tf_train_loss(name, e, r, c["pos"], c["neg"], c["w"].double(), [mode], c["gamma"], c["rng"], mod,
                           call=O.tf_call_useful if useful else O.tf_call)
    loss.backward()
    return c, loss.item(), e.grad, r.grad, mod.grad


def _modulus_param(c):
    return torch.tensor([[c["mod"]]], device=DEV, requires_grad=True) if c["name"] == "pRotatE" else None


def _split_path(c, mode):
    """kge_step_forward + kge_step_loss + kge_step_backward through autograd -> (loss, d_ent, d_rel, d_mod)."""
    name, D = c["name"], c["D"]
    ent, rel, pos, neg, w = _dev(c)
    _check_instance(c, ent, rel)
    ent.requires_grad_(True)
    rel.requires_grad_(True)
    mod = _modulus_param(c)
    n, p = ops.step_forward(FN_IDS[name], mode, ent, rel, pos, neg, D, c["gamma"], c["rng"],
                            rel_off=S.rel_off(name, D), modulus=mod)
    loss = ops.step_loss(n, p, w)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), ent.grad.clone(), rel.grad.clone(), None if mod is None else mod.grad.clone()


def _atomic_path(c, mode):
    """kge_score_indexed (+ _bwd), kge_neg_reduce (+ _bwd), kge_log_sigmoid (+ _bwd) through autograd."""
    name, D = c["name"], c["D"]
    ent, rel, pos, neg, w = _dev(c)
    ent.requires_grad_(True)
    rel.requires_grad_(True)
    mod = _modulus_param(c)
    kw = dict(rel_off=S.rel_off(name, D), modulus=mod)
    fn = FN_IDS[name]
    n = ops.neg_reduce(ops.score_indexed(fn, mode, ent, rel, pos, neg, D, c["gamma"], c["rng"], **kw)).unsqueeze(1)
    p = ops.log_sigmoid(ops.score_indexed(fn, 3, ent, rel, pos, None, D, c["gamma"], c["rng"], **kw))
    loss = (-(w * p).sum() / w.sum() - (w * n).sum() / w.sum()) / 2
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), ent.grad.clone(), rel.grad.clone(), None if mod is None else mod.grad.clone()


def _check_grads(got, ref, what):
    c, loss, d_ent, d_rel, d_mod = ref
    g_loss, g_ent, g_rel, g_mod = got
    err = rel_close(g_loss.item(), loss)
    print(what, "loss err", err, "d_ent err", float((g_ent.cpu().double() - d_ent).abs().max() / d_ent.abs().max()),
          "d_rel err", float((g_rel.cpu().double() - d_rel).abs().max() / d_rel.abs().max()))
    assert err <= TOL, (what, err)
    assert _grad_close(g_ent.cpu(), d_ent), what
    assert _grad_close(g_rel.cpu(), d_rel), what
    if c["name"] == "pRotatE":
        assert _grad_close(g_mod.cpu().reshape(-1), d_mod.reshape(-1)), what


def _bitwise(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", FNS)
@pytest.mark.parametrize("D", list(WIDTHS))
@pytest.mark.parametrize("mode", [0, 1])
def test_split_path_backward_matches_oracle(name, D, mode):
    """Loss, d_ent, d_rel (and the pRotatE modulus gradient) of kge_step_forward + kge_step_loss +
    kge_step_backward; the deterministic backward is bitwise equal run to run."""
    ref = _ref(name, D, mode)
    got = _split_path(ref[0], mode)
    _check_grads(got, ref, (name, D, mode, "split"))
    assert _bitwise(got, _split_path(ref[0], mode)), (name, D, mode)


@pytest.mark.parametrize("name", FNS)
@pytest.mark.parametrize("D", list(WIDTHS))
@pytest.mark.parametrize("mode", [0, 1])
def test_atomic_path_backward_matches_oracle(name, D, mode):
    """The same gradients from the unfused calls (kge_score_indexed_bwd: atomic scatter in the dword-per-lane
    layout up to D = 1024)."""
    ref = _ref(name, D, mode)
    _check_grads(_atomic_path(ref[0], mode), ref, (name, D, mode, "atomic"))


# ------------------------------------------------------------------------------------------------
# the fused train step: two steps, head-batch then tail-batch
# ------------------------------------------------------------------------------------------------
def _batches(name, D, shape):
    E, R, B, N = shape
    return [S.make_case(name, D, E, R, B, N, seed=D + 1000 * i) for i in range(2)]


def _oracle_step(name, c, mode, ent, rel, mod, useful):
    """Loss and gradients of one train step in fp64 at the given (fp64) parameters."""
    e = ent.clone().requires_grad_(True)
    r = rel.clone().requires_grad_(True)
    m = mod.clone().requires_grad_(name == "pRotatE")
    loss = O.tf_train_loss(name, e, r, c["pos"], c["neg"], c["w"].double(), [mode], c["gamma"], c["rng"], m,
                           call=O.tf_call_useful if useful else O.tf_call)
    loss.backward()
    return loss.item(), e.grad, r.grad, m.grad


@functools.lru_cache(maxsize=None)
def _train_ref(name, D, shape=SMALL, useful=False):
    """Two oracle steps (fp64 loss graph + Keras Adam): the losses, the tables and the modulus after both, and
    the first moments after the first."""
    bs = _batches(name, D, shape)
    p = {"e": bs[0]["ent"].double(), "r": bs[0]["rel"].double(), "m": torch.tensor(bs[0]["mod"], dtype=torch.float64)}
    st, losses, m1 = {}, [], None
    for t, c in enumerate(bs, start=1):
        loss, *grads = _oracle_step(name, c, (t - 1) % 2, p["e"], p["r"], p["m"], useful)
        losses.append(loss)
        for key, gr in zip("erm", grads):
            if gr is None:
                continue
            mm, vv = st.get(key, (torch.zeros_like(p[key]), torch.zeros_like(p[key])))
            p2, mm, vv = O.keras_adam_step(p[key], gr, mm, vv, t, LR)
            st[key] = (mm, vv)
            p[key] = p2.detach()
        if t == 1:
            m1 = (st["e"][0], st["r"][0])
    return dict(losses=losses, ent=p["e"], rel=p["r"], mod=p["m"], m1_ent=m1[0], m1_rel=m1[1])


def _train_hip(name, D, shape):
    """Two TFKGEModel.train_step_fused calls: kge_train_step, or kge_step_forward + kge_step_loss +
    kge_step_backward_adam for pRotatE (which kge_train_step refuses). Returns the losses and, after each step,
    (entity table, relation table, their first moments, modulus)."""
    E, R, B, N = shape
    bs = _batches(name, D, shape)
    m = kge.TFKGEModel(name, E, R, D, bs[0]["gamma"], *S.model_flags(name), device=DEV, seed=D)
    with torch.no_grad():
        m.entity_embedding.copy_(bs[0]["ent"])
        m.relation_embedding.copy_(bs[0]["rel"])
    _check_instance(bs[0], m.entity_embedding, m.relation_embedding)
    assert m._range_f == bs[0]["rng"]
    if name == "pRotatE":
        assert float(m.modulus.detach().reshape(-1)[0]) == bs[0]["mod"]
    opt = Adam(m.parameters(), lr=LR)
    out = []
    for i, c in enumerate(bs):
        out.append(m.train_step_fused(c["pos"].to(DEV), c["neg"].to(DEV), c["w"].to(DEV), i % 2, opt).clone())
        out += [m.entity_embedding.detach().clone(), m.relation_embedding.detach().clone(),
                opt.state[m.entity_embedding]["exp_avg"].clone(), opt.state[m.relation_embedding]["exp_avg"].clone(),
                m.modulus.detach().clone() if name == "pRotatE" else torch.zeros(1, device=DEV)]
    torch.cuda.synchronize()
    return out


def _check_train(got, ref, name, D, shape, useful, what):
    """Losses and final tables against the two oracle steps, at the project's bars. First moments, which are
    linear in the gradients, at the gradient bar: after step 1 against the oracle's (0.1 * gradient); after
    step 2 against the oracle step taken FROM THE STATE THE LIBRARY HAD after step 1 (its fp32 tables and
    moments, in fp64). The second comparison must start there: the tables after step 1 may differ from the
    oracle's by the table bar (5e-2 * lr, Adam's m / sqrt(v) where |g| ~ eps), and a score function's phase
    divides by embedding_range / pi ~ 4e-3 at D = 1022, so that allowed difference alone moves step 2's
    gradient by more than the gradient bar; it says nothing about the kernels."""
    l1, e1, r1, me1, mr1, mod1, l2, e2, r2, me2, mr2, mod2 = got
    losses = np.array([l1.item(), l2.item()])
    err = rel_close(losses, np.array(ref["losses"]))
    e_err = float((e2.cpu().double() - ref["ent"]).abs().max())
    r_err = float((r2.cpu().double() - ref["rel"]).abs().max())
    print(what, "loss err", err, "ent err / lr", e_err / LR, "rel err / lr", r_err / LR)
    assert err <= TOL, (what, err)
    assert e_err <= 5e-2 * LR, (what, e_err)
    assert r_err <= 5e-2 * LR, (what, r_err)
    if name == "pRotatE":
        assert abs(float(mod2.cpu().double().reshape(-1)[0]) - float(ref["mod"])) <= 5e-2 * LR, what
    assert _grad_close(me1.cpu(), ref["m1_ent"]), (what, "m_ent after step 1")
    assert _grad_close(mr1.cpu(), ref["m1_rel"]), (what, "m_rel after step 1")
    c = _batches(name, D, shape)[1]
    mod64 = mod1.cpu().double().reshape(()) if name == "pRotatE" else torch.tensor(c["mod"], dtype=torch.float64)
    _, g_ent, g_rel, _ = _oracle_step(name, c, 1, e1.cpu().double(), r1.cpu().double(), mod64, useful)
    for got_m, m_prev, g, tag in ((me2, me1, g_ent, "m_ent"), (mr2, mr1, g_rel, "m_rel")):
        prev = m_prev.cpu().double()
        _, want, _ = O.keras_adam_step(prev, g, prev, torch.zeros_like(prev), 2, LR)
        print(what, tag, "step 2 err", float((got_m.cpu().double() - want).abs().max() / want.abs().max()))
        assert _grad_close(got_m.cpu(), want), (what, tag + " after step 2")


@pytest.mark.parametrize("name", FNS)
@pytest.mark.parametrize("D", list(WIDTHS))
def test_fused_train_step_matches_oracle(name, D):
    """Losses, both tables and the first moments after a head-batch and a tail-batch step; D = 511 and 1022
    (G = 8) take kge_train_step's fallback with its own phase 1. Bitwise equal run to run."""
    got = _train_hip(name, D, SMALL)
    _check_train(got, _train_ref(name, D), name, D, SMALL, False, (name, D, "train"))
    assert _bitwise(got, _train_hip(name, D, SMALL)), (name, D)


@pytest.mark.parametrize("name", FNS)
@pytest.mark.parametrize("D", [255, 450])
def test_hot_entities_at_narrow_vector_widths(name, D):
    """E = 3, B = 40, N = 160 at V = 1 (D = 255) and V = 2 (D = 450), both G = 4: every entity row collects
    ~2 200 gradient events, so bwd_ent_stream_kernel runs its block-wide sort and, past 2 048 events, its
    ordered extraction, which otherwise run only at V = 4."""
    for mode in (0, 1):
        ref = _ref(name, D, mode, HOT, True)
        _check_grads(_split_path(ref[0], mode), ref, (name, D, mode, "hot split"))
    got = _train_hip(name, D, HOT)
    _check_train(got, _train_ref(name, D, HOT, True), name, D, HOT, True, (name, D, "hot train"))
    assert _bitwise(got, _train_hip(name, D, HOT)), (name, D)


# ------------------------------------------------------------------------------------------------
# forward forms at V = 2 and V = 1
# ------------------------------------------------------------------------------------------------
def _same(a, b):
    """Bitwise equal, NaN where the other is NaN."""
    return all(bool(((x == y) | (torch.isnan(x) & torch.isnan(y))).all()) for x, y in zip(a, b))


@pytest.mark.parametrize("name", FNS)
@pytest.mark.parametrize("D", [33, 50, 255, 450])
@pytest.mark.parametrize("mode", [0, 1])
def test_forward_forms_bitwise_at_narrow_vector_widths(name, D, mode):
    """kge_step_forward_ex in the orders row (step_fwd_kernel), xcd (step_fwd_xcd_kernel) and tile
    (step_fwd_tile_kernel, whose LDS query image is G * 64 * V * 4 bytes; rows cap none and 3) and two chained
    planned steps give bitwise the same four outputs on a ragged batch, and the row form is within the score bar
    of O.score, O.adv_reduce and logsigmoid in fp64."""
    E, R, B, N = 600, 7, 19, 130
    c = S.make_case(name, D, E, R, B, N, seed=D)
    c2 = S.make_case(name, D, E, R, B, N, seed=D + 77)
    ent, rel, pos, neg, _ = _dev(c)
    pos2, neg2 = c2["pos"].to(DEV), c2["neg"].to(DEV)
    _check_instance(c, ent, rel)
    V, G = WIDTHS[D]
    fn, ro = FN_IDS[name], S.rel_off(name, D)

    def run(order, p, n, md, rows=None):
        out = ops.step_forward_raw(fn, md, ent, rel, ro, p, n, D, c["gamma"], c["rng"], modulus=c["mod"],
                                   forms=dict(step_order=order, tile_rows=rows))
        torch.cuda.synchronize()
        return out

    want = run("row", pos, neg, mode)
    assert _same(run("xcd", pos, neg, mode), want)
    for rows in (None, 3):
        assert _same(run("tile", pos, neg, mode, rows), want), rows
    # the planned step exists exactly when the tile form fits
    size = ops.StepPlanner.plan_size(fn, ent, rel, ro, D, B, N)
    assert (size > 0) == S.tile_fits(name, B, N, D, V, G), size
    if size > 0:
        sp = ops.StepPlanner(fn, ent, rel, ro, D, B, N, c["gamma"], c["rng"], modulus=c["mod"])
        sp.plan(pos, neg, mode)
        first = [t.clone() for t in sp.step(nxt=(pos2, neg2, 1 - mode))]
        second = [t.clone() for t in sp.step()]
        torch.cuda.synchronize()
        assert _same(first, want)
        assert _same(second, run("row", pos2, neg2, 1 - mode))
    # the row form against the oracle
    e64, r64 = c["ent"].double(), c["rel"].double()
    ns = O.score(name, e64, r64, c["pos"], c["neg"], mode, c["gamma"], c["rng"], c["mod"])
    ps = O.score(name, e64, r64, c["pos"], c["neg"], 3, c["gamma"], c["rng"], c["mod"])
    out_neg, out_pos, neg_scores, pos_scores = (t.cpu().numpy() for t in want)
    errs = (rel_close(neg_scores, ns.numpy()), rel_close(pos_scores, ps[:, 0].numpy()),
            rel_close(out_neg, O.adv_reduce(ns)[:, 0].numpy()), rel_close(out_pos, F.logsigmoid(ps)[:, 0].numpy()))
    print((name, D, mode), "errs", errs)
    assert max(errs) <= TOL, errs


# ------------------------------------------------------------------------------------------------
# out-of-range ids in the backward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["TransE", "DistMult", "ComplEx", "RotatE"])
@pytest.mark.parametrize("mode", [0, 1])
def test_out_of_range_candidates_get_no_gradient(name, mode):
    """An out-of-range candidate id reads a zero row in the forward (TF's GPU tf.gather) and must scatter no
    gradient in the backward: ev_count_kernel / ev_scatter_kernel and step_fwd_grad_kernel bucket only
    0 <= id < E, score_bwd_kernel guards its atomics. Oracle: the table extended by a zero row, the bad ids
    remapped to it; loss, d_ent[:E] and d_rel on the split path, and loss, tables and first moments of one
    kge_train_step. InterHT is left out: its zero row gives NaN (Q7)."""
    D = 64
    E, R, B, N = SMALL
    c = S.make_case(name, D, E, R, B, N, seed=17)
    bad = c["neg"].clone()
    bad[0, 1], bad[1, 2], bad[2, 5], bad[3, 0], bad[3, 23] = -3, E, 10 ** 9, E, -3
    remap = bad.clone()
    remap[(bad < 0) | (bad >= E)] = E
    ez = torch.cat([c["ent"], torch.zeros(1, c["ent"].shape[1])]).double().requires_grad_(True)
    r = c["rel"].double().requires_grad_(True)
    loss = O.tf_train_loss(name, ez, r, c["pos"], remap, c["w"].double(), [mode], c["gamma"], c["rng"], c["mod"])
    loss.backward()
    d_ent, d_rel = ez.grad[:E], r.grad
    cb = dict(c, neg=bad)
    _check_grads(_split_path(cb, mode), (cb, loss.item(), d_ent, d_rel, None), (name, mode, "oor split"))
    _check_grads(_atomic_path(cb, mode), (cb, loss.item(), d_ent, d_rel, None), (name, mode, "oor atomic"))
    # one kge_train_step: the first moments are (1 - beta1) * gradient
    m = kge.TFKGEModel(name, E, R, D, c["gamma"], *S.model_flags(name), device=DEV, seed=17)
    with torch.no_grad():
        m.entity_embedding.copy_(c["ent"])
        m.relation_embedding.copy_(c["rel"])
    opt = Adam(m.parameters(), lr=LR)
    got_loss = m.train_step_fused(c["pos"].to(DEV), bad.to(DEV), c["w"].to(DEV), mode, opt)
    torch.cuda.synchronize()
    assert rel_close(got_loss.item(), loss.item()) <= TOL
    zero = torch.zeros_like(d_ent)
    ent1, m_ent, _ = O.keras_adam_step(c["ent"].double(), d_ent, zero, zero, 1, LR)
    zero = torch.zeros_like(d_rel)
    rel1, m_rel, _ = O.keras_adam_step(c["rel"].double(), d_rel, zero, zero, 1, LR)
    assert _grad_close(opt.state[m.entity_embedding]["exp_avg"].cpu(), m_ent), name
    assert _grad_close(opt.state[m.relation_embedding]["exp_avg"].cpu(), m_rel), name
    assert float((m.entity_embedding.detach().cpu().double() - ent1).abs().max()) <= 5e-2 * LR
    assert float((m.relation_embedding.detach().cpu().double() - rel1).abs().max()) <= 5e-2 * LR
