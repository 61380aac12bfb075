"""kge_train_step_lazy and optim.Adam(lazy=True): the fused train step that updates only the rows a batch touches.

1. One step, exact: from non-zero moments at step 7, kge_train_step and kge_train_step_lazy run on twins. Touched rows
   of both tables and of all four moment tensors are bitwise the dense step's, untouched rows are bitwise what they
   were, loss / out_neg / out_pos are the dense step's, and the dense twin moved an untouched row.
2. No state: any workspace contents, a workspace reused at a smaller batch, run to run.
3. Three steps against the fp64 reference of tests/lazy_adam_ref.py (both Adam rules; weight=None through
   KGEModel.train_step_fused).
4. Trainer with a lazy optimizer.

Widths (tests/test_train_reg_gpu.py's): d 24 (V4 G1), 300 (V4 G2), 33 (V1 G1): bwd_ent_kernel; 450 (V2 G4), 1 000
(V4 G4): bwd_ent_stream_kernel; 1 500 (G8): the stream kernel behind the separate-phase-1 fallback."""
import types

import numpy as np
import pytest
import torch

import customknowledgegraphembedding_amd as kge
from customknowledgegraphembedding_amd import _lib as L
from customknowledgegraphembedding_amd._lib import FN_IDS
from customknowledgegraphembedding_amd.optim import Adam
from customknowledgegraphembedding_amd.supervisor import Strategy, Sum, Trainer
from tests import lazy_adam_ref as R
from tests import strided as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR, B1, B2, GAMMA, STEP0 = 1e-3, 0.9, 0.999, 9.0, 7
NAMES = ["InterHT", "TransE", "DistMult", "ComplEx", "RotatE"]
WIDTHS = [24, 300, 33, 450, 1000, 1500]
NREL, ABSENT_REL = 7, (2, 5)
ENT_VIEWS = (0, 2, 3)  # of State.views(): the entity table and its two moments (the others: the relation's)
BIG_E = 4194400  # past 1 024 tiles of 4 096 entities: the single-block scan


# ------------------------------------------------------------------------------------------------
# batches
# ------------------------------------------------------------------------------------------------
def make_batch(E, B, N, seed=9, force=(), exclude=(), oor=False, all_oor=False):
    """pos [B, 3], neg [B, N] (int64, CPU): ids of RandomState(seed) outside `exclude`, relations outside ABSENT_REL,
    the rows of `force` written into the batch (negatives, a positive head, a positive tail in turn). oor: ids -1, E
    and 2^40 among the negatives. all_oor: every id (relations too) out of range."""
    g = np.random.RandomState(seed)
    ok = np.setdiff1d(np.arange(min(E, 1 << 20)), np.asarray(exclude, dtype=np.int64))
    rels = np.setdiff1d(np.arange(NREL), ABSENT_REL)
    pos = np.stack([g.choice(ok, size=B), g.choice(rels, size=B), g.choice(ok, size=B)], 1).astype(np.int64)
    neg = g.choice(ok, size=(B, N)).astype(np.int64)
    for i, e in enumerate(force):
        b = i % B
        if i % 3 == 0:
            neg[b, (5 * i + 1) % N] = e
        elif i % 3 == 1:
            pos[b, 0] = e
        else:
            pos[b, 2] = e
    if oor:
        neg[B - 1, 0], neg[B - 1, 1], neg[B - 1, N - 1] = -1, E, 1 << 40
        neg[0, N // 2] = E
    if all_oor:
        neg[:] = g.choice([-1, E, E + 7, 1 << 40, -(1 << 35)], size=(B, N))
        pos[:, 0], pos[:, 2] = E, -1
        pos[:, 1] = g.choice([-1, NREL, 1 << 33], size=B)
    assert not (set(exclude) & set(neg.reshape(-1).tolist() + pos[:, 0].tolist() + pos[:, 2].tolist()))
    return torch.from_numpy(pos), torch.from_numpy(neg)


# ------------------------------------------------------------------------------------------------
# one model's device state and one C-ABI call per step()
# ------------------------------------------------------------------------------------------------
def _layout(t, layout):
    if layout == "dense":
        return t.clone()
    if layout.startswith("pad"):  # a row stride wider than the row, NaN in the padding
        return S.padded(t, int(layout[3:]), DEV)
    return S.offset(t, int(layout[3:]), DEV)  # "offK": a base K floats off 16 B, NaN around it


class State:
    """Tables and Adam moments of one model on the device, all six laid out alike. Values are drawn on the device
    from a seeded generator: twins built with the same arguments are bitwise equal."""

    def __init__(self, name, D, E, layout="dense", seed=4):
        em, rm = S.MULT[name]
        self.name, self.D, self.E = name, D, E
        self.rng = (GAMMA + 2.0) / D
        g = torch.Generator(device=DEV).manual_seed(seed)
        scale = 1.0 if name == "InterHT" else self.rng  # unit rows keep InterHT's normalisation finite at any width

        def draw(rows, w, lo, hi):
            return torch.rand(rows, w, generator=g, device=DEV) * (hi - lo) + lo

        vals = [draw(E, em * D, -scale, scale), draw(NREL, rm * D, -scale, scale),
                draw(E, em * D, -1e-3, 1e-3), draw(E, em * D, 0.0, 1e-6),      # m_ent, v_ent >= 0
                draw(NREL, rm * D, -1e-3, 1e-3), draw(NREL, rm * D, 0.0, 1e-6)]
        self.ent, self.rel = _layout(vals[0], layout), _layout(vals[1], layout)
        self.mv = []
        for tab, v in ((self.ent, vals[2]), (self.ent, vals[3]), (self.rel, vals[4]), (self.rel, vals[5])):
            m = S.like_table(tab) if layout != "dense" else torch.empty_like(v)
            m.copy_(v)
            self.mv.append(m)
        self.t = STEP0 - 1
        self.loss_sum = torch.full((1,), 1.5, dtype=torch.float32, device=DEV)

    def views(self):
        return [self.ent, self.rel] + self.mv

    def step(self, entry, pos, neg, mode, keras=1, ws=None, ws_fill=None, w=None):
        lib = L.load()
        fn, ro = FN_IDS[self.name], S.rel_off(self.name, self.D)
        B, N = neg.shape
        size = lib.kge_train_step_lazy_workspace_size if entry == "lazy" else lib.kge_train_step_workspace_size
        nbytes = size(fn, self.E, NREL, self.rel.stride(0), B, N, self.D)
        assert nbytes > 0
        if ws is None:
            ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
            if ws_fill is not None:
                ws.fill_(ws_fill)
        assert ws.numel() >= nbytes
        self.ws = ws
        if w is None:
            w = torch.linspace(0.2, 1.0, B, device=DEV)
        out = torch.full((2 * B + 5,), float("nan"), dtype=torch.float32, device=DEV)  # log | loss | neg | pos
        o = out.data_ptr()
        args = [fn, mode, self.ent.data_ptr(), self.E, self.ent.stride(0), self.rel.data_ptr(), NREL,
                self.rel.stride(0), ro, pos.data_ptr(), neg.data_ptr(), neg.stride(0), B, N, self.D, GAMMA, self.rng,
                1.0, 1, 0, w.data_ptr(), o + 16, self.loss_sum.data_ptr(), o + 20, o + 20 + 4 * B] + \
               [m.data_ptr() for m in self.mv] + \
               [LR, B1, B2, 1e-7 if keras else 1e-8, self.t + 1, keras, ws.data_ptr(), ws.numel(),
                torch.cuda.current_stream().cuda_stream]
        rc = lib.kge_train_step_lazy(*args, o) if entry == "lazy" else lib.kge_train_step(*args)
        torch.cuda.synchronize()
        assert rc == 0, (rc, lib.kge_last_error())
        self.t += 1
        self.out = out
        return self


def _eq(a, b):
    """Bit for bit (a NaN equals itself: InterHT gives a row with an out-of-range negative a NaN loss, in the dense
    step as here)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _same_state(a, b, what):
    for x, y in zip(a.views() + [a.out[4:], a.loss_sum], b.views() + [b.out[4:], b.loss_sum]):
        assert _eq(x, y), what


def check_one_step(name, D, E, B, N, mode, layout="dense", keras=1, want_untouched=True, **batch):
    """Test 1's assertions for one case."""
    pos, neg = make_batch(E, B, N, **batch)
    te, tr = R.touched_masks(pos, neg, E, NREL)
    te, tr = te.to(DEV), tr.to(DEV)
    pd, nd = pos.to(DEV), neg.to(DEV)
    dense, lazy = State(name, D, E, layout), State(name, D, E, layout)
    before = [v.clone() for v in dense.views()]
    assert all(torch.equal(x, y) for x, y in zip(before, lazy.views()))  # twins
    outside = [S.outside_bits(v) for v in lazy.views()] if layout != "dense" else None
    dense.step("plain", pd, nd, mode, keras=keras)
    lazy.step("lazy", pd, nd, mode, keras=keras)
    what = (name, D, E, B, N, mode, layout, keras)
    moved = False
    finite = all(bool(torch.isfinite(v).all()) for v in lazy.views()) and bool(torch.isfinite(lazy.out).all())
    assert finite or (name == "InterHT" and batch.get("oor")), what  # (see _eq)
    for i, (got, ref, old) in enumerate(zip(lazy.views(), dense.views(), before)):
        t = te if i in ENT_VIEWS else tr
        assert t.shape[0] == got.shape[0]
        assert _eq(got[t], ref[t]), what + (i, "touched rows are the dense step's")
        assert _eq(got[~t], old[~t]), what + (i, "untouched rows are what they were")
        moved = moved or (bool((~t).any()) and not _eq(ref[~t], old[~t]))
        assert finite or not bool(torch.isfinite(ref).all()), what + (i, "finite")
    # loss, out_neg, out_pos (out[4:]) and the running sum are the dense step's; the log's loss is the loss
    assert _eq(lazy.out[4:], dense.out[4:]) and _eq(lazy.loss_sum, dense.loss_sum), what
    assert _eq(lazy.out[0:1], lazy.out[4:5]) and float(lazy.out[3]) == 0
    if want_untouched:
        assert bool((~te).any()) and moved, what + ("the dense twin moves an untouched row",)
    else:
        assert bool(te.all())  # the whole entity table and its moments are the dense step's
        assert all(_eq(lazy.views()[i], dense.views()[i]) for i in ENT_VIEWS)
    if outside is not None:
        for v, bits in zip(lazy.views(), outside):
            assert torch.equal(S.outside_bits(v), bits), what + ("padding",)
    return lazy, dense, te, tr


# ------------------------------------------------------------------------------------------------
# 1. one step, exact
# ------------------------------------------------------------------------------------------------
E1 = 9000  # three scan tiles; the list (B N + 3 B = 280 entries) is shorter than the table
FORCE1, EXCL1 = (0, 4096, E1 - 1), (4095, 8191, 8192)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("name", NAMES)
def test_one_step_exact(name, d, mode):
    _, _, te, tr = check_one_step(name, d, E1, 8, 32, mode, force=FORCE1, exclude=EXCL1)
    assert te[list(FORCE1)].all() and not te[list(EXCL1)].any()
    assert tr.tolist() == [r not in ABSENT_REL for r in range(NREL)]


SUBSET = [("InterHT", 24), ("TransE", 33), ("DistMult", 300), ("InterHT", 450), ("ComplEx", 1000), ("RotatE", 1500)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,d", SUBSET)
def test_one_step_exact_torch_rule(name, d, mode):
    check_one_step(name, d, E1, 8, 32, mode, keras=0, force=FORCE1, exclude=EXCL1)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,d", SUBSET)
def test_one_step_exact_bound_equals_table(name, d, mode):
    """E 90, B 40, N 72: B N + 3 B = 3 000 >= E, the grid is the table's; few rows are untouched (row 17 is kept
    out so that one always is)."""
    _, _, te, _ = check_one_step(name, d, 90, 40, 72, mode, exclude=(17,))
    assert int((~te).sum()) <= 5


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,d", SUBSET)
def test_one_step_exact_every_row_hot(name, d, mode):
    """E 3, B 40, N 160: ~2 200 events per row (ordered extraction past the 2 048-entry sort); every row is touched
    and the whole tables equal the dense step's. (Every relation but 2 and 5 is used: those stay.)"""
    check_one_step(name, d, 3, 40, 160, mode, want_untouched=False)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("layout", ["pad4", "pad2", "pad1", "off1", "off2"])
@pytest.mark.parametrize("name,d", [("InterHT", 24), ("ComplEx", 64), ("DistMult", 300), ("TransE", 450)])
def test_one_step_exact_padded_views(name, d, layout, mode):
    check_one_step(name, d, E1, 8, 32, mode, layout=layout, force=FORCE1, exclude=EXCL1)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,d", SUBSET)
def test_out_of_range_ids_are_dropped(name, d, mode):
    check_one_step(name, d, E1, 8, 32, mode, force=FORCE1, exclude=EXCL1, oor=True)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,d", SUBSET)
def test_batch_with_every_id_out_of_range(name, d, mode):
    pos, neg = make_batch(E1, 8, 32, all_oor=True)
    pd, nd = pos.to(DEV), neg.to(DEV)
    dense, lazy = State(name, d, E1), State(name, d, E1)
    before = [v.clone() for v in lazy.views()]
    dense.step("plain", pd, nd, mode)
    lazy.step("lazy", pd, nd, mode)
    for got, old in zip(lazy.views(), before):
        assert _eq(got, old), (name, d, mode)
    assert _eq(lazy.out[4:], dense.out[4:]) and _eq(lazy.loss_sum, dense.loss_sum)
    assert not _eq(dense.ent, before[0])  # the dense step moved rows it had no gradient for


@pytest.mark.parametrize("mode", [0, 1])
def test_single_block_scan_path(mode):
    """E 4 194 400 (TransE d 4): more than 1 024 tiles, scan_block_kernel; touched rows at both ends of the table
    and on both sides of the last tile boundaries."""
    ends = (0, 1, 4095, 4096, 4194303, 4194304, BIG_E - 2, BIG_E - 1)
    _, _, te, _ = check_one_step("TransE", 4, BIG_E, 8, 32, mode, force=ends, exclude=(2, BIG_E - 3))
    assert te[list(ends)].all() and int(te.sum()) <= 8 * 32 + 3 * 8


# ------------------------------------------------------------------------------------------------
# 2. no state
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,d,E", [("InterHT", 24, E1), ("DistMult", 450, E1), ("ComplEx", 1500, E1),
                                      ("TransE", 4, BIG_E)])
def test_workspace_carries_no_state(name, d, E):
    big = make_batch(E, 8, 32, force=(0, E - 1))
    small = make_batch(E, 4, 16, seed=11, force=(1, E - 2))
    big, small = [t.to(DEV) for t in big], [t.to(DEV) for t in small]
    ref = State(name, d, E).step("lazy", *big, 1, ws_fill=0)
    again = State(name, d, E).step("lazy", *big, 1, ws_fill=0)
    _same_state(ref, again, (name, d, "run to run"))
    for fill in (0x7F, 0xFF, 0x01):
        s = State(name, d, E).step("lazy", *big, 1, ws_fill=fill)
        _same_state(ref, s, (name, d, hex(fill)))
    # the same workspace at a smaller batch (and the other mode), against a zeroed one
    ref.step("lazy", *small, 0, ws_fill=0)
    again.step("lazy", *small, 0, ws=again.ws)
    _same_state(ref, again, (name, d, "reused workspace"))


# ------------------------------------------------------------------------------------------------
# 3. three steps against the fp64 reference
# ------------------------------------------------------------------------------------------------
E3, R3, B3, N3 = 400, 4, 6, 24


def _batches3():
    g = np.random.RandomState(6)
    out = []
    for i in range(3):
        pos = torch.from_numpy(np.stack([g.randint(E3, size=B3), g.randint(R3, size=B3), g.randint(E3, size=B3)], 1))
        neg = torch.from_numpy(g.randint(E3, size=(B3, N3)))
        w = torch.from_numpy(g.uniform(0.2, 1.0, size=(B3, 1))).float()
        out.append((pos, neg, w, i % 2))
    return out


def _once_touched_rows(batches):
    """Rows touched in step 1 and not in step 2: where a dense Adam moves and a lazy one does not."""
    t1 = R.touched_masks(batches[0][0], batches[0][1], E3, R3)[0]
    t2 = R.touched_masks(batches[1][0], batches[1][1], E3, R3)[0]
    rows = (t1 & ~t2).nonzero().reshape(-1)
    assert rows.numel() >= 20, rows.numel()  # about 87 with these shapes
    return rows


def _check_three_steps(name, ent, rel, rng, gamma, keras, upstream, run_step, final):
    batches = _batches3()
    rows = _once_touched_rows(batches)
    lazy = R.RefStep(name, ent, rel, gamma, rng, LR, keras=keras, lazy=True, upstream=upstream)
    dense = R.RefStep(name, ent, rel, gamma, rng, LR, keras=keras, lazy=False, upstream=upstream)
    bar = 5e-2 * LR
    for pos, neg, w, mode in batches:
        wr = None if upstream else w
        ref_loss = lazy.step(pos, neg, wr, mode)
        dense.step(pos, neg, wr, mode)
        loss = run_step(pos, neg, w, mode)
        np.testing.assert_allclose(loss, ref_loss, rtol=1e-4)
    # the test tells the two optimizers apart: on every row touched in step 1 only they differ by more than the bar
    gap = (dense.ent[rows] - lazy.ent[rows]).abs().max(dim=1).values
    assert float(gap.min()) > bar, float(gap.min())
    got_ent, got_rel = final()
    assert float((got_ent.cpu().double() - lazy.ent).abs().max()) <= bar
    assert float((got_rel.cpu().double() - lazy.rel).abs().max()) <= bar


@pytest.mark.parametrize("semantics", ["keras", "torch"])
@pytest.mark.parametrize("name,d", [("InterHT", 200), ("DistMult", 24)])
def test_three_steps_match_the_reference(name, d, semantics):
    gamma = 12.0
    de, dr, tr = S.model_flags(name)
    m = kge.TFKGEModel(name, E3, R3, d, gamma, double_entity_embedding=de, double_relation_embedding=dr,
                       triple_relation_embedding=tr, device=DEV, seed=13)
    opt = Adam(m.parameters(), lr=LR, semantics=semantics, lazy=True)

    def run_step(pos, neg, w, mode):
        return float(m.train_step_fused(pos.to(DEV), neg.to(DEV), w.to(DEV), mode, opt))

    _check_three_steps(name, m.entity_embedding.detach().cpu(), m.relation_embedding.detach().cpu(), m._range_f, gamma,
                       semantics == "keras", False, run_step,
                       lambda: (m.entity_embedding.detach(), m.relation_embedding.detach()))
    assert opt.state[m.entity_embedding]["step"] == 3 == opt.state[m.relation_embedding]["step"]


def _args(uni=True, reg=0.0):
    return types.SimpleNamespace(negative_adversarial_sampling=True, adversarial_temperature=1.0, uni_weight=uni,
                                 regularization=reg)


@pytest.mark.parametrize("semantics", ["keras", "torch"])
def test_three_steps_null_weight_through_the_upstream_model(semantics):
    """KGEModel.train_step_fused with uni_weight passes weight = NULL to kge_train_step_lazy."""
    gamma = 12.0
    m = kge.KGEModel("DistMult", E3, R3, 24, gamma, device=DEV, seed=13)
    opt = Adam(m.parameters(), lr=LR, semantics=semantics, lazy=True)
    logs = []

    def run_step(pos, neg, w, mode):
        it = iter([(pos, neg, w.reshape(-1), "tail-batch" if mode else "head-batch")])
        logs.append(kge.KGEModel.train_step_fused(m, opt, it, _args()))
        return logs[-1]["loss"]

    _check_three_steps("DistMult", m.entity_embedding.detach().cpu(), m.relation_embedding.detach().cpu(),
                       m._range_f, gamma, semantics == "keras", True, run_step,
                       lambda: (m.entity_embedding.detach(), m.relation_embedding.detach()))
    for log in logs:
        assert set(log) == {"loss", "positive_sample_loss", "negative_sample_loss"}
        assert abs(log["loss"] - (log["positive_sample_loss"] + log["negative_sample_loss"]) / 2) <= 1e-6


# ------------------------------------------------------------------------------------------------
# 4. Trainer with a lazy optimizer
# ------------------------------------------------------------------------------------------------
def test_trainer_with_a_lazy_optimizer():
    name, d, gamma = "InterHT", 64, 12.0
    m = kge.TFKGEModel(name, E3, R3, d, gamma, double_entity_embedding=True, triple_relation_embedding=True,
                       device=DEV, seed=13)
    ent0 = m.entity_embedding.detach().clone()
    batches = [(p, n, w, torch.tensor([mode] * B3)) for p, n, w, mode in _batches3()]
    opt = Adam(m.parameters(), lr=LR, lazy=True)
    trainer = Trainer(Strategy(), batches, m, opt, Sum())
    assert trainer.fused and trainer.one_call
    it = iter(batches)
    l1 = trainer.train_step(it)
    acc = trainer.metrics.accumulator(DEV)
    assert float(acc) == float(l1)  # the Sum metric advanced inside the step
    st = opt.state[m.entity_embedding]
    m1, v1 = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
    l2 = trainer.train_step(it)
    assert float(trainer.metrics.result()) == float(np.float32(float(l1)) + np.float32(float(l2)))
    assert st["step"] == 2 == opt.state[m.relation_embedding]["step"]
    t1 = R.touched_masks(batches[0][0], batches[0][1], E3, R3)[0].to(DEV)
    t2 = R.touched_masks(batches[1][0], batches[1][1], E3, R3)[0].to(DEV)
    never, once = ~t1 & ~t2, t1 & ~t2
    assert int(never.sum()) > 0 and int(once.sum()) >= 20
    assert torch.equal(m.entity_embedding.detach()[never], ent0[never]) and not bool(st["exp_avg"][never].any())
    assert bool(m1[once].any()) and torch.equal(st["exp_avg"][once], m1[once])  # no decay in step 2
    assert torch.equal(st["exp_avg_sq"][once], v1[once])
    # the upstream model's log dict: the keys of a step without the regulariser (its fourth value, the
    # regularisation term, is 0 and by train_step's rule not a key then)
    u = kge.KGEModel("DistMult", E3, R3, 24, gamma, device=DEV, seed=13)
    p, n, w, _ = _batches3()[0]
    log = kge.KGEModel.train_step_fused(u, Adam(u.parameters(), lr=LR, lazy=True),
                                        iter([(p, n, w.reshape(-1), "head-batch")]), _args(uni=False))
    assert set(log) == {"loss", "positive_sample_loss", "negative_sample_loss"}
    assert all(np.isfinite(v) for v in log.values())
