"""kge_train_step_reg and KGEModel.train_step_fused: the fused train step with upstream's loss flags (model.py:4-44;
upstream KGEModel.train_step): uni_weight, adversarial sampling with a temperature, and the L3 ("N3") regulariser
applied inside the entity pass.

The reference of every case is oracle.kge_oracle.upstream_train_loss in fp64 with autograd. LAMBDA = 0.05, not a
realistic 2e-6: the bars below are relative to the largest reference value, and at 0.05 the regulariser is between
0.07 and 0.97 of max|grad| on both tables for every (function, width) used here (DistMult and ComplEx at every
width; TransE and RotatE only at d 24 and 33, their data gradient does not shrink with the width), so a 1e-4 max
bar sees a missing regulariser and a missing data term alike. Every gradient case asserts that premise itself
(>= 0.05 max|grad|): a condition of the test, not a tolerance.

Shapes: E 300, R 6, B 10, N 17, gamma 9 with the ids of RandomState(9): 162 of the 300 entity rows and relation 2
carry no gradient event. Widths per kernel class: d 24 (V4 G1), 300 (V4 G2), 33 (V1 G1): bwd_ent_kernel; 450 (V2 G4),
1 000 (V4 G4): bwd_ent_stream_kernel; 1 500 (G8): the stream kernel behind kge_train_step's fallback forward."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import _lib as L
from customknowledgegraphembedding_amd._lib import FN_IDS
from customknowledgegraphembedding_amd.optim import Adam
from oracle import kge_oracle as O
from tests import strided as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LAMBDA, LR, B1, B2, GAMMA = 0.05, 1e-3, 0.9, 0.999, 9.0
E0, R0, B0, N0 = 300, 6, 10, 17
MODES = {0: "head-batch", 1: "tail-batch"}
ONE_MINUS_B1 = float(np.float32(1.0) - np.float32(B1))  # the library's (1.f - b1)
WIDTHS = [("DistMult", d) for d in (24, 300, 33, 450, 1000, 1500)] + \
         [("ComplEx", d) for d in (24, 300, 33, 450, 1000, 1500)] + \
         [("TransE", 24), ("TransE", 33), ("RotatE", 24), ("RotatE", 33)]
FLAGS = [(True, 0.5, False), (True, 0.5, True), (False, 1.0, False), (False, 1.0, True)]  # adv, temperature, uni


@functools.lru_cache(maxsize=None)
def case(name, D, E=E0, B=B0, N=N0, unit=False):
    """CPU fp32 tables and the seed-9 batch (ids, negatives, weights in the order of test_configs_gpu.py). unit:
    rows drawn from U(-1, 1), so InterHT's normalisation stays finite whatever the width."""
    em, rm = S.MULT[name]
    ent, rel, rng = O.make_tables(E, R0, em * D, rm * D, GAMMA, D, seed=4)
    if unit:
        ent, rel = ent / rng, rel / rng
    g = np.random.RandomState(9)
    pos = torch.from_numpy(np.stack([g.randint(E, size=B), g.randint(R0, size=B), g.randint(E, size=B)], 1))
    neg = torch.from_numpy(g.randint(E, size=(B, N)))
    w = torch.from_numpy(g.uniform(0.1, 1.0, size=(B,))).float()
    return types.SimpleNamespace(name=name, D=D, E=E, B=B, N=N, ent=ent, rel=rel, rng=rng, pos=pos, neg=neg, w=w)


def oracle_step(c, ent, rel, mode, lam, adv, temp, uni):
    """(loss, d_ent, d_rel) of upstream's loss at the fp64 tables ent, rel."""
    e, r = ent.clone().requires_grad_(True), rel.clone().requires_grad_(True)
    loss = O.upstream_train_loss(c.name, e, r, c.pos, c.neg, c.w.double(), MODES[mode], GAMMA, c.rng,
                                 adversarial=adv, temperature=temp, uni_weight=uni, regularization=lam)
    loss.backward()
    return loss.item(), e.grad, r.grad


@functools.lru_cache(maxsize=None)
def ref(key, mode, lam, adv, temp, uni):
    """The oracle's first step of case(*key), computed once per flag set and shared (never modified)."""
    c = case(*key)
    return oracle_step(c, c.ent.double(), c.rel.double(), mode, lam, adv, temp, uni)


def reg_value(ent, rel, lam):
    return lam * float((ent.double().abs() ** 3).sum() + (rel.double().abs() ** 3).sum())


def _pad(t, pad):
    return S.padded(t, pad, DEV) if pad else t.clone().to(DEV)


class Step:
    """The device state of one model (tables, Adam moments, running loss sum) and one C-ABI call per step()."""

    def __init__(self, c, pad=0, loss_sum=0.0):
        self.c = c
        self.ent, self.rel = _pad(c.ent, pad), _pad(c.rel, pad)
        self.mv = [_pad(torch.zeros_like(t), pad) for t in (c.ent, c.ent, c.rel, c.rel)]  # m_ent v_ent m_rel v_rel
        self.pos, self.neg, self.w = c.pos.to(DEV), c.neg.to(DEV), c.w.to(DEV)
        self.loss_sum = torch.full((1,), loss_sum, dtype=torch.float32, device=DEV)
        self.t = 0

    def step(self, mode, lam=LAMBDA, adv=True, temp=0.5, uni=False, keras=1, entry="reg", ws_fill=None, w=None,
             expect_rc=0):
        c, lib = self.c, L.load()
        fn, ro = FN_IDS[c.name], S.rel_off(c.name, c.D)
        size = lib.kge_train_step_reg_workspace_size if entry == "reg" else lib.kge_train_step_workspace_size
        nbytes = size(fn, c.E, R0, self.rel.stride(0), c.B, c.N, c.D)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        if ws_fill is not None:
            ws.fill_(ws_fill)
        out = torch.full((2 * c.B + 5,), float("nan"), dtype=torch.float32, device=DEV)  # log | loss | neg | pos
        o = out.data_ptr()
        wt = None if uni else (self.w if w is None else w)
        args = [fn, mode, self.ent.data_ptr(), c.E, self.ent.stride(0), self.rel.data_ptr(), R0, self.rel.stride(0),
                ro, self.pos.data_ptr(), self.neg.data_ptr(), self.neg.stride(0), c.B, c.N, c.D, GAMMA, c.rng, temp,
                int(adv), 1, None if wt is None else wt.data_ptr(), o + 16, self.loss_sum.data_ptr(), o + 20,
                o + 20 + 4 * c.B] + [m.data_ptr() for m in self.mv] + \
               [LR, B1, B2, 1e-7 if keras else 1e-8, self.t + 1, keras, ws.data_ptr(), ws.numel(),
                torch.cuda.current_stream().cuda_stream]
        if entry == "reg":
            rc = lib.kge_train_step_reg(*args, lam, o)
        else:
            rc = lib.kge_train_step(*args)
        torch.cuda.synchronize()
        assert (rc == 0) == (expect_rc == 0), (rc, lib.kge_last_error())
        if rc == 0:
            self.t += 1
        self.out = out.cpu()
        self.log, self.loss = self.out[:4].numpy().copy(), float(self.out[4])
        return self

    def tensors(self):
        return [self.ent, self.rel] + self.mv + [self.out[4:]]


def _grad_from_moment(m):
    return m.cpu().double() / ONE_MINUS_B1


def _check_premise(key, mode, adv, temp, uni):
    _, ge, gr = ref(key, mode, LAMBDA, adv, temp, uni)
    _, ge0, gr0 = ref(key, mode, 0.0, adv, temp, uni)
    for g, g0 in ((ge, ge0), (gr, gr0)):
        assert float((g - g0).abs().max()) >= 0.05 * float(g.abs().max()), (key, mode, "premise")


def _check_grads(s, key, mode, adv, temp, uni):
    _check_premise(key, mode, adv, temp, uni)
    _, ge, gr = ref(key, mode, LAMBDA, adv, temp, uni)
    for got, want, what in ((s.mv[0], ge, "ent"), (s.mv[2], gr, "rel")):
        err = float((_grad_from_moment(got) - want).abs().max())
        assert err <= 1e-4 * float(want.abs().max()), (key, mode, adv, temp, uni, what, err)


# ------------------------------------------------------------------------------------------------
# 1. gradients through the first moment: exp_avg = (1 - beta1) g after one step from zero moments
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,d", WIDTHS)
def test_gradient_with_regulariser(name, d, mode):
    key = (name, d)
    for adv, temp, uni in FLAGS:
        s = Step(case(*key)).step(mode, adv=adv, temp=temp, uni=uni)
        _check_grads(s, key, mode, adv, temp, uni)
    s = Step(case(*key)).step(mode, adv=True, temp=0.5, uni=False, keras=0)  # torch semantics: the same moment
    _check_grads(s, key, mode, True, 0.5, False)


# ------------------------------------------------------------------------------------------------
# 2. rows without a gradient event get exactly the regulariser's gradient, element by element
# ------------------------------------------------------------------------------------------------
def _idle_rows(c):
    used = torch.cat([c.pos[:, 0], c.pos[:, 2], c.neg.reshape(-1)]).unique()
    idle = torch.ones(c.E, dtype=torch.bool)
    idle[used] = False
    rel_idle = torch.ones(R0, dtype=torch.bool)
    rel_idle[c.pos[:, 1].unique()] = False
    return idle, rel_idle


def _check_pure_reg(moment, table, what):
    x = table.double()
    want = 3 * LAMBDA * x * x.abs()
    assert want.numel() > 0 and bool((want != 0).any()), what
    err = (_grad_from_moment(moment) - want).abs()
    assert bool((err <= 1e-5 * want.abs()).all()), (what, float((err / want.abs().clamp_min(1e-300)).max()))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,d", [("DistMult", 24), ("DistMult", 33), ("ComplEx", 300), ("ComplEx", 450),
                                    ("DistMult", 1000), ("ComplEx", 1500), ("RotatE", 24)])
def test_rows_without_events_get_the_regulariser_only(name, d, mode):
    c = case(name, d)
    idle, rel_idle = _idle_rows(c)
    assert int(idle.sum()) == 162 and rel_idle.tolist() == [False, False, True, False, False, False]
    for keras in (1, 0):
        s = Step(c).step(mode, keras=keras)
        _check_pure_reg(s.mv[0][idle.to(DEV)], c.ent[idle], (name, d, "entity"))
        _check_pure_reg(s.mv[2][rel_idle.to(DEV)], c.rel[rel_idle], (name, d, "relation"))


@pytest.mark.parametrize("mode", [0, 1])
def test_interht_unread_relation_thirds_are_regularised(mode):
    """InterHT reads the middle third of a relation row (rel_off = D, rel_dim = 3 D): the outer thirds have no data
    gradient and must still get 3 lambda x |x|. Unit-scale rows keep the model's normalisation finite."""
    D = 64
    c = case("InterHT", D, unit=True)
    idle, _ = _idle_rows(c)
    s = Step(c).step(mode)
    m_rel = s.mv[2].cpu()
    _check_pure_reg(m_rel[:, :D], c.rel[:, :D], "first third")
    _check_pure_reg(m_rel[:, 2 * D:], c.rel[:, 2 * D:], "last third")
    _check_pure_reg(s.mv[0][idle.to(DEV)], c.ent[idle], "entity rows without events")
    assert bool(torch.isfinite(s.ent).all()) and bool(torch.isfinite(s.rel).all())
    # the middle third carries a data gradient on the relations the batch uses
    x = c.rel[:, D:2 * D].double()
    assert float((_grad_from_moment(m_rel[:, D:2 * D]) - 3 * LAMBDA * x * x.abs()).abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------
# 3. the log {loss, positive_sample_loss, negative_sample_loss, regularization}, loss and loss_sum
# ------------------------------------------------------------------------------------------------
def _log_ref(c, key, mode, lam, adv, temp, uni):
    loss = ref(key, mode, lam, adv, temp, uni)[0]
    loss0 = ref(key, mode, 0.0, adv, temp, uni)[0]
    ps = F.logsigmoid(O.score(c.name, c.ent.double(), c.rel.double(), c.pos, c.neg, "single", GAMMA, c.rng))
    ps = ps.reshape(-1)
    wd = c.w.double()
    pos_loss = float(-ps.mean()) if uni else float(-(wd * ps).sum() / wd.sum())
    reg = reg_value(c.ent, c.rel, lam)
    assert abs((loss - loss0) - reg) <= 1e-9 * max(1.0, reg)  # the oracle's own term
    return loss, pos_loss, 2 * loss0 - pos_loss, reg


def _check_log(s, want, start_sum, what):
    loss, pos_loss, neg_loss, reg = want
    got = s.log
    for g, w_ in ((got[0], loss), (got[1], pos_loss), (got[2], neg_loss)):
        assert abs(float(g) - w_) <= 1e-4 * max(1.0, abs(w_)), (what, got, want)
    assert abs(float(got[3]) - reg) <= 1e-4 * reg, (what, got, want)
    assert np.float32(s.loss) == got[0]
    f = np.float32
    composed = f(f(f(got[1] + got[2]) / f(2)) + got[3])
    assert abs(float(got[0]) - float(composed)) <= float(np.spacing(composed)), (what, got)
    advanced = f(f(start_sum) + got[0])
    assert abs(float(s.loss_sum.item()) - float(advanced)) <= float(np.spacing(advanced)), what


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,d", [("DistMult", 24), ("TransE", 33), ("ComplEx", 300), ("ComplEx", 1000),
                                    ("DistMult", 1500)])
def test_log_values(name, d, mode):
    key = (name, d)
    c = case(*key)
    for adv, temp, uni in FLAGS:
        s = Step(c, loss_sum=3.25).step(mode, adv=adv, temp=temp, uni=uni)
        _check_log(s, _log_ref(c, key, mode, LAMBDA, adv, temp, uni), 3.25, (key, mode, adv, temp, uni))
        assert bool(torch.isfinite(s.out).all())


# ------------------------------------------------------------------------------------------------
# 4. tables after three steps
# ------------------------------------------------------------------------------------------------
def _three_steps(c, keras, update):
    s = Step(c)
    ent, rel = c.ent.double(), c.rel.double()
    for t in (1, 2, 3):
        mode = t % 2
        s.step(mode, keras=keras)
        loss, ge, gr = oracle_step(c, ent, rel, mode, LAMBDA, True, 0.5, False)
        assert abs(s.loss - loss) <= 1e-4 * max(1.0, abs(loss)), t
        ent, rel = update(t, ent, rel, ge, gr)
    assert float((s.ent.cpu().double() - ent).abs().max()) <= 5e-2 * LR
    assert float((s.rel.cpu().double() - rel).abs().max()) <= 5e-2 * LR


@pytest.mark.parametrize("name,d", [("DistMult", 300), ("ComplEx", 1000)])
def test_three_steps_keras_adam(name, d):
    c = case(name, d)
    st = {k: (torch.zeros_like(t, dtype=torch.float64),) * 2 for k, t in (("e", c.ent), ("r", c.rel))}

    def update(t, ent, rel, ge, gr):
        ent, me, ve = O.keras_adam_step(ent, ge, *st["e"], t, LR)
        rel, mr, vr = O.keras_adam_step(rel, gr, *st["r"], t, LR)
        st["e"], st["r"] = (me, ve), (mr, vr)
        return ent, rel

    _three_steps(c, 1, update)


def test_three_steps_torch_adam():
    c = case("DistMult", 300)
    pe, pr = c.ent.double().clone().requires_grad_(True), c.rel.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([pe, pr], lr=LR, betas=(B1, B2), eps=1e-8)

    def update(t, ent, rel, ge, gr):
        pe.grad, pr.grad = ge.clone(), gr.clone()
        opt.step()
        return pe.detach().clone(), pr.detach().clone()

    _three_steps(c, 0, update)


# ------------------------------------------------------------------------------------------------
# 5. lambda = 0 is kge_train_step, bitwise; 6. weight = NULL is weight = ones; 7. determinism, workspace
# ------------------------------------------------------------------------------------------------
def _same(a, b, what):
    for x, y in zip(a.tensors(), b.tensors()):
        assert torch.equal(x.cpu(), y.cpu()), what


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,d", [("InterHT", 24), ("InterHT", 1000), ("DistMult", 24), ("DistMult", 1000)])
def test_lambda_zero_is_the_existing_step(name, d, mode):
    c = case(name, d)
    a, b = Step(c, loss_sum=1.5), Step(c, loss_sum=1.5)
    for t in range(2):
        a.step(mode, lam=0.0, adv=True, temp=1.0, entry="reg")
        b.step(mode, adv=True, temp=1.0, entry="plain")
        _same(a, b, (name, d, mode, t))
        assert torch.equal(a.loss_sum, b.loss_sum)
        assert a.log[3] == 0.0 and a.log[0] == np.float32(a.loss) and np.isfinite(a.log).all()


@pytest.mark.parametrize("name,d", [("ComplEx", 24), ("DistMult", 1000), ("ComplEx", 1500)])
def test_null_weight_is_unit_weight(name, d):
    c = case(name, d)
    ones = torch.ones(c.B, dtype=torch.float32, device=DEV)
    a = Step(c).step(1, uni=True)
    b = Step(c).step(1, uni=False, w=ones)
    for x, y in zip(a.tensors()[:-1], b.tensors()[:-1]):
        assert torch.equal(x, y), (name, d)
    np.testing.assert_allclose(a.out.numpy(), b.out.numpy(), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("name,d", [("ComplEx", 24), ("DistMult", 450), ("ComplEx", 1000), ("DistMult", 1500)])
def test_deterministic_and_stateless_workspace(name, d):
    c = case(name, d)
    a, b, g = Step(c, loss_sum=2.0), Step(c, loss_sum=2.0), Step(c, loss_sum=2.0)
    for t in range(2):
        a.step(t % 2, ws_fill=0)
        b.step(t % 2, ws_fill=0)
        g.step(t % 2, ws_fill=0xFF)
        _same(a, b, (name, d, t, "run to run"))
        _same(a, g, (name, d, t, "0xff workspace"))
        assert torch.equal(a.loss_sum, g.loss_sum) and np.array_equal(a.log, g.log)


# ------------------------------------------------------------------------------------------------
# 8. hot rows: E 12 puts ~800 events in each bucket (the block-wide sort of the stream kernel), E 3 ~2 200
#    (past the sort's 2 048: ordered extraction)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,B,N", [(12, 48, 200), (3, 40, 160)])
@pytest.mark.parametrize("name", ["DistMult", "ComplEx"])
def test_hot_rows(name, E, B, N):
    key = (name, 1000, E, B, N)
    for mode in (0, 1):
        s = Step(case(*key)).step(mode)
        _check_grads(s, key, mode, True, 0.5, False)


# ------------------------------------------------------------------------------------------------
# 9. padded tables and moments (NaN in the padding)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [4, 2, 1])
@pytest.mark.parametrize("name,D", [("ComplEx", 64), ("DistMult", 520)])
def test_padded_layouts(name, D, pad):
    key = (name, D)
    c = case(*key)
    for mode in (0, 1):
        s = Step(c, pad=pad, loss_sum=0.5)
        views = [s.ent, s.rel] + s.mv
        before = [S.outside_bits(v) for v in views]
        _, G = S.table_vg(name, D, s.ent, s.rel)
        if G > S.K_MAX_G:  # D 520 on 4-byte rows: refused, nothing written
            inside = [v.clone() for v in views]
            s.step(mode, expect_rc=1)
            assert all(torch.equal(a, b) for a, b in zip(inside, views))
        else:
            s.step(mode)
            _check_grads(s, key, mode, True, 0.5, False)
            _check_log(s, _log_ref(c, key, mode, LAMBDA, True, 0.5, False), 0.5, (key, pad, mode))
            assert all(bool(torch.isfinite(v).all()) for v in views)
        for v, bits in zip(views, before):
            assert torch.equal(S.outside_bits(v), bits), (key, pad, mode)


# ------------------------------------------------------------------------------------------------
# 10. KGEModel.train_step_fused against KGEModel.train_step on a twin model
# ------------------------------------------------------------------------------------------------
def _args(adv, temp, uni, reg):
    return types.SimpleNamespace(negative_adversarial_sampling=adv, adversarial_temperature=temp, uni_weight=uni,
                                 regularization=reg)


def _twin(name, semantics="keras"):
    de, dr = name in ("RotatE", "ComplEx"), name == "ComplEx"
    ms = [kge.KGEModel(name, 120, 6, 24, GAMMA, double_entity_embedding=de, double_relation_embedding=dr, device=DEV,
                       seed=4) for _ in range(2)]
    return ms, [Adam(m.parameters(), lr=LR, semantics=semantics) for m in ms]


def _batches(E, steps):
    g = np.random.RandomState(9)
    for i in range(steps):
        pos = torch.from_numpy(np.stack([g.randint(E, size=B0), g.randint(R0, size=B0), g.randint(E, size=B0)], 1))
        neg = torch.from_numpy(g.randint(E, size=(B0, N0)))
        w = torch.from_numpy(g.uniform(0.1, 1.0, size=(B0,))).float()
        yield pos, neg, w, MODES[i % 2]


@pytest.mark.parametrize("name", ["RotatE", "TransE", "DistMult", "ComplEx"])
@pytest.mark.parametrize("adv,temp,uni,reg", [(False, 1.0, False, 0.0), (True, 0.5, False, 0.0),
                                              (True, 1.0, True, 0.0), (True, 1.0, False, LAMBDA),
                                              (False, 1.0, True, LAMBDA), (True, 2.0, True, LAMBDA)])
def test_model_train_step_fused_matches_train_step(name, adv, temp, uni, reg):
    (a, b), (oa, ob) = _twin(name, "torch" if uni else "keras")
    args = _args(adv, temp, uni, reg)
    ia, ib = _batches(120, 5), _batches(120, 5)
    for t in range(5):
        la = kge.KGEModel.train_step_fused(a, oa, ia, args)
        lb = kge.KGEModel.train_step(b, ob, ib, args)
        assert list(la) == list(lb) and ("regularization" in la) == (reg != 0.0)
        for k in ("loss", "positive_sample_loss", "negative_sample_loss"):
            assert abs(la[k] - lb[k]) <= 1e-4 * max(1.0, abs(lb[k])), (t, k, la, lb)
        if reg:
            assert abs(la["regularization"] - lb["regularization"]) <= 1e-4 * lb["regularization"], (t, la, lb)
    assert oa.state[a.entity_embedding]["step"] == 5 == oa.state[a.relation_embedding]["step"]
    for x, y in zip(a.parameters(), b.parameters()):
        assert float((x.detach() - y.detach()).abs().max()) <= 5e-2 * LR


def test_model_train_step_fused_rejections():
    args = _args(True, 1.0, False, LAMBDA)
    m = kge.KGEModel("pRotatE", 50, 4, 16, GAMMA, device=DEV, seed=1)
    with pytest.raises(NotImplementedError, match="train_step"):
        kge.KGEModel.train_step_fused(m, Adam(m.parameters(), lr=LR), _batches(50, 1), args)
    (a, _), (oa, _) = _twin("DistMult")
    with pytest.raises(TypeError):
        kge.KGEModel.train_step_fused(a, torch.optim.Adam(a.parameters(), lr=LR), _batches(120, 1), args)
    # a moment laid out unlike its parameter is refused before anything is launched or counted
    ent = a.entity_embedding
    before = ent.detach().clone()
    oa.state[ent].update(step=0, exp_avg=S.padded(torch.zeros_like(ent), 4), exp_avg_sq=torch.zeros_like(ent))
    with pytest.raises(ValueError, match="exp_avg"):
        kge.KGEModel.train_step_fused(a, oa, _batches(120, 1), args)
    torch.cuda.synchronize()
    assert torch.equal(ent.detach(), before) and oa.state[ent]["step"] == 0
    # a lambda the library refuses leaves the step counters where they were
    (c, _), (oc, _) = _twin("DistMult")
    with pytest.raises(L.KGEHipError, match="regularization"):
        kge.KGEModel.train_step_fused(c, oc, _batches(120, 1), _args(True, 1.0, False, -1.0))
    assert oc.state[c.entity_embedding]["step"] == 0
