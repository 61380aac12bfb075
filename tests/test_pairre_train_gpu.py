"""PairRE gradients and train steps on the GPU against autograd of the fp64 reference (tests/pairre_ref.py):
kge_score_indexed_bwd, kge_step_backward, kge_train_step / _reg / _lazy and the split form. The bars are the
project's: gradients 1e-4 max|grad| (tests/test_train_reg_gpu.py), loss 1e-4, tables after Adam within 5e-2 lr
(tests/test_train_c2_gpu.py)."""
import numpy as np
import pytest
import torch

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import _lib as L
from customknowledgegraphembedding_amd import ops
from customknowledgegraphembedding_amd.optim import Adam
from tests import lazy_adam_ref as R
from tests import pairre_cases as PC
from tests import pairre_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FN = PC.FN
LR, B1, B2 = 1e-3, 0.9, 0.999
E0, R0, B0, N0 = 97, 6, 10, 17


def _orthogonal(x, g, what):
    """Each touched row's gradient is orthogonal to the row (the score depends on the row's direction only):
    |<x, g>| <= 1e-4 ||x|| ||g||. A missing or doubled normalisation backward fails this."""
    x, g = x.double(), g.double()
    touched = g.abs().sum(1) > 0
    assert int(touched.sum()) > 0
    dots = (x * g).sum(1).abs()
    lim = 1e-4 * x.norm(dim=1) * g.norm(dim=1)
    assert bool((dots[touched] <= lim[touched]).all()), (what, float((dots / lim.clamp_min(1e-300))[touched].max()))


def _close(got, want, what):
    err = float((got.cpu().double() - want).abs().max())
    assert err <= 1e-4 * float(want.abs().max()), (what, err, float(want.abs().max()))


# ------------------------------------------------------------------------------------------------
# 3. backward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [24, 33, 300, 450, 1000, 1500])
def test_score_indexed_bwd(D):
    c = PC.case(D, E0, R0, B0, N0, seed=D)
    ent, rel, pos, neg = c.ent.to(DEV), c.rel.to(DEV), c.pos.to(DEV), c.neg.to(DEV)
    g = torch.Generator().manual_seed(D)
    for mode in (0, 1, 3):
        ds = torch.randn(B0, 1 if mode == 3 else N0, generator=g)
        e, r = c.ent.double().requires_grad_(True), c.rel.double().requires_grad_(True)
        (P.score(e, r, c.pos, c.neg, mode, c.gamma) * ds.double()).sum().backward()
        d_ent, d_rel = torch.zeros_like(ent), torch.zeros_like(rel)
        ops.score_indexed_bwd_raw(FN, mode, ent, rel, 0, pos, None if mode == 3 else neg, D, c.gamma, c.rng, 0.0,
                                  ds.to(DEV), d_ent, d_rel)
        _close(d_ent, e.grad, (D, mode, "ent"))
        _close(d_rel, r.grad, (D, mode, "rel"))
        assert float(d_rel[:, :D].abs().max()) > 0 and float(d_rel[:, D:].abs().max()) > 0, (D, mode)
        _orthogonal(c.ent, d_ent.cpu(), (D, mode))


@pytest.mark.parametrize("D", [24, 33, 300, 450, 1000, 1500])
def test_step_backward(D):
    c = PC.case(D, E0, R0, B0, N0, seed=D + 3)
    pos, neg, w = c.pos.to(DEV), c.neg.to(DEV), c.w.to(DEV)
    for mode in (0, 1):
        for red, adv, detach, T in (("tf", True, False, 1.0), ("detached", True, True, 0.5), ("mean", False, True, 1.0)):
            loss, ge, gr = P.train_grads(c.ent.double(), c.rel.double(), c.pos, c.neg, c.w.double(), mode, c.gamma,
                                         red, T)
            ent, rel = c.ent.to(DEV).requires_grad_(True), c.rel.to(DEV).requires_grad_(True)
            n, p = ops.step_forward(FN, mode, ent, rel, pos, neg, D, c.gamma, c.rng, temperature=T, adversarial=adv,
                                    detach=detach)
            got = (-(w * p).sum() / w.sum() - (w * n).sum() / w.sum()) / 2
            got.backward()
            assert abs(float(got.detach()) - loss) <= 1e-4 * max(1.0, abs(loss)), (D, mode, red)
            _close(ent.grad, ge, (D, mode, red, "ent"))
            _close(rel.grad, gr, (D, mode, red, "rel"))
            assert float(rel.grad[:, :D].abs().max()) > 0 and float(rel.grad[:, D:].abs().max()) > 0
            _orthogonal(c.ent, ent.grad.cpu(), (D, mode, red))


def test_clamped_row_takes_the_linear_forms_derivative():
    """A row with ||x|| <= 1e-12 normalises as x 1e12: its gradient is 1e12 d, with no projection term."""
    D = 24
    c = PC.case(D, E0, R0, B0, N0, seed=1)
    ent = c.ent.clone()
    tiny = int(c.neg[0, 0])
    ent[tiny] = ent[tiny] * (1e-15 / float(ent[tiny].norm()))
    ds = torch.ones(B0, N0)
    e, r = ent.double().requires_grad_(True), c.rel.double().requires_grad_(True)
    P.score(e, r, c.pos, c.neg, 1, c.gamma).sum().backward()
    d_ent, d_rel = torch.zeros(E0, D, device=DEV), torch.zeros(R0, 2 * D, device=DEV)
    ops.score_indexed_bwd_raw(FN, 1, ent.to(DEV), c.rel.to(DEV), 0, c.pos.to(DEV), c.neg.to(DEV), D, c.gamma, c.rng,
                              0.0, ds.to(DEV), d_ent, d_rel)
    want = e.grad[tiny]
    assert float(want.abs().max()) > 1e9
    assert float((d_ent[tiny].cpu().double() - want).abs().max()) <= 1e-4 * float(want.abs().max())


# ------------------------------------------------------------------------------------------------
# 4. train steps
# ------------------------------------------------------------------------------------------------
class Step:
    """The device state of one model (tables, Adam moments) and one C-ABI call per step()."""

    def __init__(self, c):
        self.c = c
        self.ent, self.rel = c.ent.clone().to(DEV), c.rel.clone().to(DEV)
        self.mv = [torch.zeros_like(t) for t in (self.ent, self.ent, self.rel, self.rel)]  # m_ent v_ent m_rel v_rel
        self.w = c.w.to(DEV)
        self.t = 0

    def step(self, pos, neg, mode, entry="plain", lam=0.0, keras=1, ws_fill=None, adv=True, detach=0, temp=1.0):
        c, lib = self.c, L.load()
        size = {"plain": lib.kge_train_step_workspace_size, "reg": lib.kge_train_step_reg_workspace_size,
                "lazy": lib.kge_train_step_lazy_workspace_size}[entry]
        B, N = neg.shape
        ws = torch.empty(size(FN, c.E, c.R, self.rel.stride(0), B, N, c.D), dtype=torch.uint8, device=DEV)
        if ws_fill is not None:
            ws.fill_(ws_fill)
        out = torch.full((2 * B + 5,), float("nan"), dtype=torch.float32, device=DEV)  # log | loss | neg | pos
        o = out.data_ptr()
        pos, neg = pos.to(DEV), neg.to(DEV)
        args = [FN, mode, self.ent.data_ptr(), c.E, self.ent.stride(0), self.rel.data_ptr(), c.R, self.rel.stride(0),
                0, pos.data_ptr(), neg.data_ptr(), neg.stride(0), B, N, c.D, c.gamma, c.rng, temp, int(adv), detach,
                self.w.data_ptr(), o + 16, None, o + 20, o + 20 + 4 * B] + [m.data_ptr() for m in self.mv] + \
               [LR, B1, B2, 1e-7 if keras else 1e-8, self.t + 1, keras, ws.data_ptr(), ws.numel(),
                torch.cuda.current_stream().cuda_stream]
        if entry == "reg":
            rc = lib.kge_train_step_reg(*args, lam, o)
        elif entry == "lazy":
            rc = lib.kge_train_step_lazy(*args, o)
        else:
            rc = lib.kge_train_step(*args)
        torch.cuda.synchronize()
        assert rc == 0, (rc, lib.kge_last_error())
        self.t += 1
        self.out = out.cpu()
        self.log, self.loss = self.out[:4].numpy().copy(), float(self.out[4])
        return self

    def state(self):
        return [self.ent, self.rel] + self.mv


def _batches(E, R, B, N, seed, steps=3):
    g = np.random.RandomState(seed)
    out = []
    for i in range(steps):
        pos = torch.from_numpy(np.stack([g.randint(E, size=B), g.randint(R, size=B), g.randint(E, size=B)], 1))
        out.append((pos, torch.from_numpy(g.randint(E, size=(B, N))), (i + 1) % 2))
    return out


def _bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _three_steps(D, E, B, N, keras, seed):
    c = PC.case(D, E, R0, B, N, seed=seed)
    batches = _batches(E, R0, B, N, seed + 1)
    ent, rel = c.ent.double(), c.rel.double()
    me, ve, mr, vr = (torch.zeros_like(t) for t in (ent, ent, rel, rel))
    s = Step(c)
    for t, (pos, neg, mode) in enumerate(batches, 1):
        loss, ge, gr = P.train_grads(ent, rel, pos, neg, c.w.double(), mode, c.gamma, "tf")
        ent, me, ve = R.adam_rows(ent, ge, me, ve, t, LR, keras=bool(keras))
        rel, mr, vr = R.adam_rows(rel, gr, mr, vr, t, LR, keras=bool(keras))
        s.step(pos, neg, mode, keras=keras)
        assert abs(s.loss - loss) <= 1e-4 * max(1.0, abs(loss)), (D, E, t, s.loss, loss)
    de = float((s.ent.cpu().double() - ent).abs().max()) / LR
    dr = float((s.rel.cpu().double() - rel).abs().max()) / LR
    assert de <= 5e-2 and dr <= 5e-2, (D, E, keras, de, dr)
    return c, batches, s


@pytest.mark.parametrize("D,E,B,N", [(24, 97, 10, 17), (300, 97, 10, 17), (1000, 97, 10, 17),
                                     (1000, 12, 48, 200), (1000, 3, 40, 160)])  # block sort, ordered extraction
def test_three_steps_keras_adam(D, E, B, N):
    c, batches, s = _three_steps(D, E, B, N, 1, seed=D + E)
    # two runs are bitwise equal, as is a run on a 0xff-filled workspace
    for fill in (None, 0xFF):
        s2 = Step(c)
        for pos, neg, mode in batches:
            s2.step(pos, neg, mode, ws_fill=fill)
        assert _bits_equal(s2.state() + [s2.out[4:]], s.state() + [s.out[4:]]), (D, E, fill)


@pytest.mark.parametrize("D", [24, 1000])
def test_three_steps_torch_adam(D):
    _three_steps(D, 97, 10, 17, 0, seed=D + 5)


def test_d1500_fallback_step():
    """D > 1 024: the step forward, the loss kernel and the backward with its own phase 1."""
    _three_steps(1500, 97, 10, 17, 1, seed=9)


@pytest.mark.parametrize("D", [24, 300, 1000])
def test_train_step_reg_and_log(D):
    lam = 0.05
    c = PC.case(D, E0, R0, B0, N0, seed=D + 11)
    pos, neg = c.pos, c.neg
    for mode in (0, 1):
        e, r = c.ent.double().requires_grad_(True), c.rel.double().requires_grad_(True)
        loss, pl, nl = P.train_loss(e, r, pos, neg, c.w.double(), mode, c.gamma, "detached", 0.5, lam)
        loss.backward()
        s = Step(c).step(pos, neg, mode, entry="reg", lam=lam, detach=1, temp=0.5)
        reg = lam * float((c.ent.double().abs() ** 3).sum() + (c.rel.double().abs() ** 3).sum())
        want = np.array([float(loss), float(pl), float(nl), reg])
        assert (np.abs(s.log - want) <= 1e-4 * np.maximum(1.0, np.abs(want))).all(), (D, mode, s.log, want)
        one_minus_b1 = float(np.float32(1.0) - np.float32(B1))
        _close(s.mv[0] / one_minus_b1, e.grad, (D, mode, "ent"))
        _close(s.mv[2] / one_minus_b1, r.grad, (D, mode, "rel"))
        # lambda 0 through the reg entry is the plain step
        a = Step(c).step(pos, neg, mode, entry="reg", lam=0.0)
        b = Step(c).step(pos, neg, mode)
        assert _bits_equal(a.state() + [a.out[4:]], b.state() + [b.out[4:]]), (D, mode)


@pytest.mark.parametrize("D", [24, 300, 1000, 1500])
def test_train_step_lazy(D):
    """Touched rows bitwise the dense step's; every other row and moment untouched."""
    E = 400
    c = PC.case(D, E, R0, B0, N0, seed=D + 21)
    for mode in (0, 1):
        dense, lazy = Step(c), Step(c)
        for s in (dense, lazy):  # a state in which an untouched row's dense update is visible
            for m in s.mv:
                m.fill_(0.25)
        before = [t.clone() for t in lazy.state()]
        dense.step(c.pos, c.neg, mode)
        lazy.step(c.pos, c.neg, mode, entry="lazy")
        te, tr = R.touched_masks(c.pos, c.neg, E, R0)
        assert 0 < int(te.sum()) < E
        te, tr = te.to(DEV), tr.to(DEV)
        for i, (got, full, old) in enumerate(zip(lazy.state(), dense.state(), before)):
            mask = te if got.shape[0] == E else tr
            assert torch.equal(got[mask].view(torch.int32), full[mask].view(torch.int32)), (D, mode, i, "touched")
            assert torch.equal(got[~mask].view(torch.int32), old[~mask].view(torch.int32)), (D, mode, i, "untouched")
        assert lazy.loss == dense.loss


@pytest.mark.parametrize("D", [24, 1000])
def test_split_form_equals_the_one_call_step(D):
    """kge_step_forward + kge_step_loss + kge_step_backward_adam against kge_train_step: to fp32 rounding (the fused
    forward takes its softmax weights from the hardware exp / log units)."""
    batches = _batches(E0, R0, B0, N0, seed=D)
    models = [kge.TFKGEModel("PairRE", E0, R0, D, PC.GAMMA, double_relation_embedding=True, device=DEV, seed=3)
              for _ in range(2)]
    g = torch.Generator().manual_seed(1)
    rel0 = models[0].relation_embedding.detach() / models[0]._range_f  # relation rows of U(-1, 1), as the cases'
    for m in models:
        with torch.no_grad():
            m.relation_embedding.copy_(rel0)
    opts = [Adam([m.entity_embedding, m.relation_embedding], lr=LR) for m in models]
    w = torch.rand(B0, 1, generator=g).add_(0.2).to(DEV)
    for pos, neg, mode in batches:
        la = models[0].train_step_fused(pos.to(DEV), neg.to(DEV), w, mode, opts[0], one_call=True)
        lb = models[1].train_step_fused(pos.to(DEV), neg.to(DEV), w, mode, opts[1], one_call=False)
        assert abs(float(la) - float(lb)) <= 1e-5 * max(1.0, abs(float(lb)))
    for a, b in ((models[0].entity_embedding, models[1].entity_embedding),
                 (models[0].relation_embedding, models[1].relation_embedding)):
        assert float((a - b).abs().max()) <= 5e-2 * LR
