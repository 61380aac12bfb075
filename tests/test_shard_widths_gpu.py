"""The row-sharded train step (kge_shard_train_forward / _combine / _backward, csrc/kge_shard.h) through the raw
C ABI at every (vector width V, register depth G) instance of its kernels and on padded and offset layouts.
The rest of the suite reaches the step only through ShardedKGE, whose tables are dense and whose widths all give
V = 4 with G = 1 or 2, and checks it only by the tables after a few Adam steps, which a gradient wrong by a
constant factor mostly passes (Adam's first steps move every touched element by about lr).

Driver (_Step): W ranks in one thread, no communicator. Every rank gets a row slice [lo, hi) of one full table
view (distributed.shard_bounds) with moments laid out like it, its own copy of the relation table, workspace,
stats, dq and outputs; qent / qent_pos are rows of the full CPU table. forward on every rank; the stats stacked
rank-major; combine on every rank; the dq buffers added in rank order (the SUM all-reduce) and copied back to
every rank; backward on every rank.

Reference: fp64 autograd of the sum over replicas of the replica loss, each on its own home_B rows of the fp32
values of tests/strided.py::make_case: O.tf_train_loss, or S.replica_loss for the other two reductions and
temperatures (held to O.upstream_train_loss and O.tf_train_loss by tests/test_strided_cpu.py; _ref asserts the
plain case against O.tf_train_loss too), then O.keras_adam_step.

Bars (the project's, tests/test_widths_gpu.py): every replica's loss, out_neg, out_pos_raw and out_pos
rel_close <= 1e-4; gradients _grad_close, recovered after step 1 from the first moment as m / (1 - beta1), for
every shard's rows and the relation table; sqrt(v / (1 - beta2)) against |gradient| at the same bar; tables after
the step within 5e-2 * lr; the relation table and its moments bitwise equal on every rank. Every test asserts
the (V, G) instance (S.expected_vg over the shard, the relation table, qent, qent_pos, dq and every stride) before
it compares.

What the bars catch, tried once against two deliberately wrong builds: with shard_epilogue_kernel's loss weight
`go` doubled, every gradient comparison here fails (error 1.0 against 1e-4), while the multi-step table checks of
test_shard_train_gpu.py notice it only through a later step's loss, 1.3e-4 off against their 1e-4; with
shard_pos_kernel indexing its shard row by c_ld rounded down to a multiple of 4 (the row's width under pad 1 and
pad 2) instead of c_ld, the pad 1 / pad 2 layouts fail here and test_shard_train_gpu.py passes."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from customknowledgegraphembedding_amd import _lib as L
from customknowledgegraphembedding_amd._lib import FN_IDS, KGEHipError
from customknowledgegraphembedding_amd.distributed import shard_bounds
from oracle import kge_oracle as O
from tests import strided as S
from tests.conftest import rel_close
from tests.test_parity_gpu import _grad_close
from tests.test_strides_gpu import LAYOUTS, NAMES, _lay

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL, LR, B1, B2, EPS = 1e-4, 1e-3, 0.9, 0.999, 1e-7
ENOTSUP = -95  # KGE_ENOTSUP
FNS = ["TransE", "DistMult", "ComplEx", "RotatE", "InterHT"]
# per-half width -> the (V, G) instance dense 16-B aligned tables get: all nine of the train kinds
WIDTHS = {33: (1, 1), 101: (1, 2), 255: (1, 4), 50: (2, 1), 250: (2, 2), 450: (2, 4), 64: (4, 1), 300: (4, 2),
          1000: (4, 4)}
# E, R, N, W, home_B. SMALL: E % W != 0 (shards of 14, 14 and 13 rows), three ranks (merge_row's order over ranks)
SMALL = (41, 5, 24, 3, 2)
HOT = (3, 5, 160, 2, 20)      # ~2 200 events per entity row, shards of 2 and 1 rows
NO_ROWS = (2, 5, 24, 3, 2)    # fewer entities than ranks: rank 2 owns nothing
ONE = (41, 5, 24, 1, 6)       # one rank: kge_train_step's algebra
RED = {"tf": (1, 0), "detached": (1, 1), "mean": (0, 0)}  # -> (adversarial, detach): shard_fwd_grad_kernel RED 2, 1, 0


@functools.lru_cache(maxsize=None)
def _case(name, D, shape=SMALL):
    E, R, N, W, hB = shape
    return S.make_case(name, D, E, R, W * hB, N, seed=D)


def _ids(c, drop):
    """(pos, neg) as the library gets them and (pos, neg, keep, pos_keep) for the reference: drop "neg" puts ids
    without an owner (-3, E + 5) among the candidates, "both" also into two positives' tails. The reference
    gets a valid id there and the masks that say the place is dropped."""
    pos, neg, E = c["pos"], c["neg"], c["E"]
    if drop is None:
        return (pos, neg), (pos, neg, None, None)
    bad_n, bad_p = neg.clone(), pos.clone()
    bad_n[0, 1], bad_n[1, 2], bad_n[3, 0], bad_n[5, 23], bad_n[5, 22] = -3, E + 5, E + 5, -3, E + 5
    if drop == "both":
        bad_p[1, 2], bad_p[4, 2] = -3, E + 5
    keep, pos_keep = (bad_n >= 0) & (bad_n < E), (bad_p[:, 2] >= 0) & (bad_p[:, 2] < E)
    ok_p = bad_p.clone()
    ok_p[:, 2] = torch.where(pos_keep, bad_p[:, 2], torch.zeros_like(bad_p[:, 2]))
    return (bad_p, bad_n), (ok_p, torch.where(keep, bad_n, torch.zeros_like(bad_n)), keep, pos_keep)


@functools.lru_cache(maxsize=None)
def _ref(name, D, mode, shape=SMALL, red="tf", T=1.0, drop=None):
    """One sharded step in fp64: every replica's loss and row outputs, the summed loss' gradients, and both tables
    after one Keras Adam step. Computed once per case; the tests only read it."""
    E, R, N, W, hB = shape
    c = _case(name, D, shape)
    pos, neg, keep, pos_keep = _ids(c, drop)[1]
    e, r = c["ent"].double().requires_grad_(True), c["rel"].double().requires_grad_(True)
    w = c["w"].double().reshape(-1)
    per, rows = [], []
    for h in range(W):
        sl = slice(h * hB, (h + 1) * hB)
        loss, n, ps = S.replica_loss(name, e, r, pos[sl], neg[sl], w[sl], mode, c["gamma"], c["rng"], red, T,
                                     None if keep is None else keep[sl], None if keep is None else pos_keep[sl])
        per.append(loss)
        rows.append((n.detach(), ps.detach()))
        if red == "tf" and T == 1.0 and drop is None:
            want = O.tf_train_loss(name, e.detach(), r.detach(), pos[sl], neg[sl], w[sl], [mode], c["gamma"], c["rng"])
            assert loss.item() == pytest.approx(want.item(), rel=1e-12)
    sum(per).backward()
    ps = torch.cat([x[1] for x in rows])
    out = dict(losses=np.array([x.item() for x in per]), out_neg=torch.cat([x[0] for x in rows]).numpy(),
               pos_raw=ps.numpy(), out_pos=F.logsigmoid(ps).numpy(), g_ent=e.grad, g_rel=r.grad)
    for key, p, g in (("ent", c["ent"].double(), e.grad), ("rel", c["rel"].double(), r.grad)):
        z = torch.zeros_like(p)
        out[key] = O.keras_adam_step(p, g, z, z, 1, LR, B1, B2, EPS)[0]
    return out


def _bits(v):
    base = v._base if v._base is not None else v
    return base.reshape(-1).view(torch.int32).clone()


class _Step:
    """One sharded train step of W ranks on one device (module docstring). layout: a key of LAYOUTS for the
    full entity table (every shard is a row slice of that view) and each rank's relation table; q_spec: the
    layout of qent / qent_pos ("ent": the entity table's); pad: neg_ld = N + 3 with valid foreign ids in the
    padding; dq_k / qpos_k: dq / qent_pos start that many floats into a 16-B aligned buffer. Moments are laid out
    like their tables; stats, dq, the row outputs and loss are views into canary buffers."""

    def __init__(self, c, mode, shape=SMALL, red="tf", T=1.0, layout=None, q_spec="ent", pad=False, drop=None,
                 dq_k=4, qpos_k=None):
        self.c, self.mode, self.shape = c, mode, shape
        E, R, N, W, hB = shape
        name, D = c["name"], c["D"]
        self.lib = L.load()
        self.fn, self.ro, self.Bg = FN_IDS[name], S.rel_off(name, D), W * hB
        (self.adv, self.detach), self.T = RED[red], T
        es, rs = LAYOUTS[layout] if layout else (None, None)
        q_spec = es if q_spec == "ent" else q_spec
        self.ent = _lay(c["ent"], es)
        self.m_ent, self.v_ent = S.like_table(self.ent, fill=0.0), S.like_table(self.ent, fill=0.0)
        self.bounds = [shard_bounds(E, W, r) for r in range(W)]
        self.rel = [_lay(c["rel"], rs) for _ in range(W)]
        self.m_rel = [S.like_table(t, fill=0.0) for t in self.rel]
        self.v_rel = [S.like_table(t, fill=0.0) for t in self.rel]
        pos, neg = _ids(c, drop)[0]
        self.pos = pos.to(DEV)
        self.neg = S.padded(neg, 3, DEV, hi=E) if pad else neg.to(DEV)
        zrow = torch.cat([c["ent"], torch.zeros(1, c["ent"].shape[1])])  # kge_gather_rows: no owner, zeros

        def rows(col):
            i = pos[:, col]
            return zrow[torch.where((i >= 0) & (i < E), i, torch.full_like(i, E))]

        self.qent = _lay(rows(2 if mode == 0 else 0), q_spec)
        if qpos_k is not None:
            self.qent_pos = S.offset(rows(0), qpos_k, DEV)
        else:
            self.qent_pos = _lay(rows(0), q_spec) if mode == 0 else self.qent  # tail-batch: the same buffer
        assert self.qent_pos.stride(0) == self.qent.stride(0)
        self.w = c["w"].reshape(-1).to(DEV)
        nqd = self.lib.kge_shard_nq(self.fn) * D
        Bg = self.Bg
        self.stats = [S.canary(1, Bg * 4, Bg * 4, DEV, 4) for _ in range(W)]
        self.dq = [S.canary(2 * Bg, nqd, nqd, DEV, dq_k) for _ in range(W)]
        self.outs = [[S.canary(1, Bg, Bg, DEV, 4) for _ in range(3)] for _ in range(W)]  # out_neg, pos_raw, out_pos
        self.loss = [S.canary(1, W, W, DEV, 4) for _ in range(W)]
        self.ws = []
        for r, (lo, hi) in enumerate(self.bounds):
            nbytes = self.lib.kge_shard_train_workspace_size(self.fn, hi - lo, R, self.rel[r].stride(0), Bg, N, D)
            assert nbytes >= 0
            self.ws.append(torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV))
        self.guarded = ([self.ent, self.m_ent, self.v_ent] + self.rel + self.m_rel + self.v_rel + self.stats + self.dq
                        + [o for per in self.outs for o in per] + self.loss)
        self.outside = [S.outside_bits(v) for v in self.guarded]
        self.whole = [_bits(v) for v in self.guarded]

    def vg(self, r=None):
        """The instance pick_vg gives rank r (None: every rank's, which must agree)."""
        if r is None:
            got = {self.vg(q) for q in range(len(self.bounds))}
            assert len(got) == 1, got
            return got.pop()
        lo, hi = self.bounds[r]
        ptrs = [self.rel[r].data_ptr(), self.qent.data_ptr(), self.qent_pos.data_ptr(), self.dq[r].data_ptr()]
        if hi > lo:
            ptrs.append(self.ent[lo:hi].data_ptr())
        return S.expected_vg(self.c["D"], lds=(self.ent.stride(0), self.rel[r].stride(0), self.qent.stride(0)),
                             offs=(self.ro,), ptrs=ptrs)

    @staticmethod
    def _p(t):
        return t.data_ptr() if t.numel() else None  # a rank without rows has nothing to point at

    def _prefix(self, r):
        E, R, N, W, hB = self.shape
        c, (lo, hi), rel = self.c, self.bounds[r], self.rel[r]
        return (self.fn, self.mode, self._p(self.ent[lo:hi]), hi - lo, self.ent.stride(0), lo, self.qent.data_ptr(),
                self.qent_pos.data_ptr(), self.qent.stride(0), rel.data_ptr(), R, rel.stride(0), self.ro,
                self.pos.data_ptr(), self.neg.data_ptr(), self.neg.stride(0), self.Bg, N, c["D"], hB, W, r,
                c["gamma"], c["rng"], self.T, self.adv, self.detach, self.w.data_ptr())

    def _tail(self, r):
        return (self.ws[r].data_ptr(), self.ws[r].numel(), torch.cuda.current_stream().cuda_stream)

    def forward(self, r):
        return self.lib.kge_shard_train_forward(*self._prefix(r), self.stats[r].data_ptr(), self.dq[r].data_ptr(),
                                                *self._tail(r))

    def combine(self, r, stats_all):
        o = self.outs[r]
        return self.lib.kge_shard_train_combine(*self._prefix(r), stats_all.data_ptr(), self.dq[r].data_ptr(),
                                                o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), *self._tail(r))

    def backward(self, r):
        lo, hi = self.bounds[r]
        return self.lib.kge_shard_train_backward(
            *self._prefix(r), self.dq[r].data_ptr(), self.loss[r].data_ptr(), None, self._p(self.m_ent[lo:hi]),
            self._p(self.v_ent[lo:hi]), self.m_rel[r].data_ptr(), self.v_rel[r].data_ptr(), LR, B1, B2, EPS, 1, 1,
            *self._tail(r))

    def run(self):
        W = len(self.bounds)
        for r in range(W):
            L.check(self.forward(r), "kge_shard_train_forward")
        stats_all = torch.cat([s.reshape(-1) for s in self.stats])  # the all-gather: rank-major
        for r in range(W):
            L.check(self.combine(r, stats_all), "kge_shard_train_combine")
        total = self.dq[0].clone()  # the SUM all-reduce, in rank order
        for r in range(1, W):
            total += self.dq[r]
        for d in self.dq:
            d.copy_(total)
        for r in range(W):
            L.check(self.backward(r), "kge_shard_train_backward")
        torch.cuda.synchronize()
        return self

    def refusals(self):
        """[(return code, kge_last_error)] of the three calls on every rank, none of which may have run."""
        out = []
        stats_all = torch.zeros(len(self.bounds) * self.Bg * 4, device=DEV)
        for r in range(len(self.bounds)):
            for call in (self.forward, lambda q: self.combine(q, stats_all), self.backward):
                out.append((call(r), self.lib.kge_last_error().decode()))
        torch.cuda.synchronize()
        return out

    def intact(self):
        for i, (v, b) in enumerate(zip(self.guarded, self.outside)):
            assert torch.equal(S.outside_bits(v), b), f"buffer {i}: an element outside the view was written"

    def untouched(self):
        for i, (v, b) in enumerate(zip(self.guarded, self.whole)):
            assert torch.equal(_bits(v), b), f"buffer {i} was written"

    def results(self):
        """Everything the step wrote, as CPU copies of the views' own elements."""
        cpu = lambda ts: [t.cpu().clone() for t in ts]  # noqa: E731
        return dict(loss=cpu(self.loss), outs=[cpu(o) for o in self.outs], ent=self.ent.cpu().clone(),
                    m_ent=self.m_ent.cpu().clone(), v_ent=self.v_ent.cpu().clone(), rel=cpu(self.rel),
                    m_rel=cpu(self.m_rel), v_rel=cpu(self.v_rel))


def _check(st, ref, what):
    """The module docstring's bars; every figure is printed before it is held to its bar."""
    res = st.results()
    for r in range(len(st.bounds)):
        errs = [rel_close(res["loss"][r].reshape(-1).numpy(), ref["losses"])]
        errs += [rel_close(res["outs"][r][i].reshape(-1).numpy(), ref[k])
                 for i, k in enumerate(("out_neg", "pos_raw", "out_pos"))]
        print(what, "rank", r, "loss / out_neg / pos_raw / out_pos err", errs)
        assert max(errs) <= TOL, (what, r, errs)
        for k in ("rel", "m_rel", "v_rel"):  # the replicas stay equal
            assert torch.equal(res[k][r], res[k][0]), (what, k, r)
    for key, m, v, p in (("ent", res["m_ent"], res["v_ent"], res["ent"]),
                         ("rel", res["m_rel"][0], res["v_rel"][0], res["rel"][0])):
        g_ref = ref["g_" + key]
        g, g2 = m.double() / (1 - B1), (v.double() / (1 - B2)).sqrt()
        scale = float(g_ref.abs().max())
        t_err = float((p.double() - ref[key]).abs().max())
        print(what, key, "grad err", float((g - g_ref).abs().max()) / scale, "sqrt(v) err",
              float((g2 - g_ref.abs()).abs().max()) / scale, "table err / lr", t_err / LR)
        assert _grad_close(g, g_ref), (what, key, "gradient from the first moment")
        assert _grad_close(g2, g_ref.abs()), (what, key, "|gradient| from the second moment")
        assert t_err <= 5e-2 * LR, (what, key, t_err)


def _same(a, b):
    """Two steps' results bitwise."""
    def flat(x):
        if isinstance(x, torch.Tensor):
            return [x]
        return [t for v in (x.values() if isinstance(x, dict) else x) for t in flat(v)]

    fa, fb = flat(a), flat(b)
    return len(fa) == len(fb) and all(torch.equal(x, y) for x, y in zip(fa, fb))


def _refused(st, V):
    """All three calls of every rank answer KGE_ENOTSUP with the real limit, before anything is written."""
    for rc, msg in st.refusals():
        assert rc == ENOTSUP, (rc, msg)
        assert "D / V <= 256" in msg and f"D = {st.c['D']} at vector width V = {V}" in msg, msg
    st.untouched()


# ------------------------------------------------------------------------------------------------
# a. every instance; b. the three reductions
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FNS)
@pytest.mark.parametrize("D", list(WIDTHS))
@pytest.mark.parametrize("mode", [0, 1])
def test_every_instance_matches_oracle(name, D, mode):
    """V in {4, 2, 1} x G in {1, 2, 4} of shard_fwd_grad_kernel (RED 2), shard_pos_kernel and
    shard_epilogue_kernel on dense tables, TF semantics at T = 1."""
    st = _Step(_case(name, D), mode)
    assert st.vg() == WIDTHS[D]
    st.run().intact()
    _check(st, _ref(name, D, mode), (name, D, mode))


def test_protate_is_refused():
    st = _Step(_case("pRotatE", 64), 1)
    for rc, msg in st.refusals():
        assert rc == ENOTSUP and "pRotatE" in msg, (rc, msg)
    st.untouched()


@pytest.mark.parametrize("red", list(RED))
@pytest.mark.parametrize("name", ["DistMult", "RotatE"])
@pytest.mark.parametrize("D", [33, 50, 300])
def test_three_reductions_match_oracle(red, name, D):
    """shard_fwd_grad_kernel's RED 0 / 1 / 2 and the matching branches of shard_combine_kernel and
    shard_epilogue_kernel: mean, self-adversarial with detached weights, self-adversarial with TF semantics, the
    adversarial ones at temperature 0.5."""
    T = 1.0 if red == "mean" else 0.5
    for mode in (0, 1):
        st = _Step(_case(name, D), mode, red=red, T=T)
        assert st.vg() == WIDTHS[D]
        st.run().intact()
        _check(st, _ref(name, D, mode, SMALL, red, T), (red, name, D, mode))


# ------------------------------------------------------------------------------------------------
# c. padded and offset layouts; d. refusals
# ------------------------------------------------------------------------------------------------
# the seven layouts of test_strides_gpu.py and one where only the query rows are padded (q_ld != ent_ld)
SPECS = {**{k: dict(layout=k) for k in LAYOUTS}, "q_pad1": dict(q_spec=("pad", 1))}
WANT_V = {"pad4": 4, "pad2": 2, "pad1": 1, "ent_pad1": 1, "rel_pad2": 2, "off1": 1, "off2": 2, "q_pad1": 1}


@pytest.mark.parametrize("name,D,layout", [(n, d, k) for n in NAMES for d in (64, 520) for k in SPECS])
def test_padded_and_offset_layouts(name, D, layout):
    """Every shard is a row slice of a padded or offset view of the full table (NaN padding), the moments are laid
    out like their tables, neg_ld = N + 3, every output sits in a canary buffer: results within the bars, nothing
    outside a view written; with pad 4 (V stays 4) bitwise the dense call's. Where the layout leaves more than
    256 vectors per half-row (D = 520 at V = 2 or 1) the step is refused."""
    c = _case(name, D)
    for mode in (0, 1):
        st = _Step(c, mode, pad=True, **SPECS[layout])
        V, G = st.vg()
        assert V == WANT_V[layout], (V, G)
        if D == 520 and layout != "pad4":
            assert G > S.K_FWD_GRAD_MAX_G
            _refused(st, V)
            continue
        assert G <= S.K_FWD_GRAD_MAX_G
        st.run().intact()
        _check(st, _ref(name, D, mode), (name, D, layout, mode))
        if layout == "pad4":
            dense = _Step(c, mode)
            assert dense.vg() == (V, G)
            assert _same(st.results(), dense.run().results()), mode


@pytest.mark.parametrize("name", ["TransE", "InterHT"])
@pytest.mark.parametrize("D,vg", [(511, (1, 8)), (1022, (2, 8)), (1500, (4, 8))])
def test_more_than_256_vectors_per_half_row_is_refused(name, D, vg):
    """G = 8 exists for the forward kinds only: forward, combine and backward all answer KGE_ENOTSUP, naming the
    limit D / V <= 256, ahead of the forward's memset and of every launch."""
    st = _Step(_case(name, D), 1)
    assert st.vg() == vg
    _refused(st, vg[0])


# ------------------------------------------------------------------------------------------------
# e. edges
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["DistMult", "RotatE"])
@pytest.mark.parametrize("D", [33, 64])
def test_rank_without_rows(name, D):
    """E = 2 at three ranks: rank 2 owns no rows and passes shard = m_ent = v_ent = NULL, shard_rows = 0. It still
    takes part in every call and applies the same relation update."""
    c = _case(name, D, NO_ROWS)
    for mode in (0, 1):
        st = _Step(c, mode, NO_ROWS)
        assert st.bounds[2] == (2, 2) and st._prefix(2)[2] is None
        assert st.vg() == {33: (1, 1), 64: (4, 1)}[D]
        st.run().intact()
        _check(st, _ref(name, D, mode, NO_ROWS), (name, D, mode, "no rows"))


def test_sharded_model_with_fewer_entities_than_ranks_trains():
    """ShardedKGE(nentity = 2, world = 3): the third rank's shard is empty (data_ptr() 0); the query exchange and
    the three train calls take it, and the step equals the replicated SUM oracle."""
    from tests.test_shard_train_gpu import _batches, _oracle_run, _sharded_run

    name, E, R, d, Bh, N, gamma, lr, W = "RotatE", 2, 5, 33, 4, 24, 9.0, 2e-3, 3
    batches = _batches(E, R, W * Bh, N, 2, seed=9)
    la, ent, rels, ranks = _sharded_run(name, E, R, d, gamma, W, batches, lr)
    assert [sk.shard.shape[0] for sk in ranks] == [1, 1, 0]
    lb, ent_ref, rel_ref = _oracle_run(name, E, R, d, gamma, W, batches, lr)
    np.testing.assert_allclose(np.array(la), np.array(lb), rtol=1e-4, atol=1e-6)
    assert all(torch.equal(r, rels[0]) for r in rels[1:])
    assert float((ent.double() - ent_ref).abs().max()) <= 5e-2 * lr
    assert float((rels[0].double() - rel_ref).abs().max()) <= 5e-2 * lr


@pytest.mark.parametrize("name", FNS)
@pytest.mark.parametrize("D", [33, 64])
def test_hot_rows_match_oracle(name, D):
    """E = 3 at two ranks, Bg = 40, N = 160: every row collects ~2 200 gradient events (phase 2's block-wide sort
    and ordered extraction), every batch row's candidates are spread over both ranks."""
    c = _case(name, D, HOT)
    for mode in (0, 1):
        st = _Step(c, mode, HOT)
        assert st.vg() == {33: (1, 1), 64: (4, 1)}[D]
        st.run().intact()
        _check(st, _ref(name, D, mode, HOT), (name, D, mode, "hot"))


@pytest.mark.parametrize("name", ["DistMult", "InterHT"])
@pytest.mark.parametrize("D", [255, 450])
def test_hot_rows_bitwise_run_to_run(name, D):
    c = _case(name, D, HOT)
    for mode in (0, 1):
        a, b = _Step(c, mode, HOT), _Step(c, mode, HOT)
        assert a.vg() == b.vg() == WIDTHS[D]
        assert _same(a.run().results(), b.run().results()), mode


@pytest.mark.parametrize("red", list(RED))
@pytest.mark.parametrize("name", ["DistMult", "InterHT"])
@pytest.mark.parametrize("D", [33, 64])
def test_ids_without_an_owner_are_dropped(red, name, D):
    """include/kge_hip.h: a candidate id outside [0, E) is left out of its row's softmax; under the mean
    reduction it adds 0 to a sum that is still divided by N; a positive whose tail has no owner scores 0 and
    sends no gradient. Head-batch: five candidates of four rows are -3 or E + 5. Tail-batch: also the tails of
    two positives (in head-batch the tail is the negatives' query entity, whose row the caller supplies)."""
    T = 1.0 if red == "mean" else 0.5
    c = _case(name, D)
    for mode, drop in ((0, "neg"), (1, "both")):
        st = _Step(c, mode, red=red, T=T, drop=drop)
        assert st.vg() == {33: (1, 1), 64: (4, 1)}[D]
        st.run().intact()
        ref = _ref(name, D, mode, SMALL, red, T, drop)
        if drop == "both":
            assert ref["pos_raw"][1] == 0 and ref["pos_raw"][4] == 0
            assert all(float(o[1][0, b]) == 0 for o in st.results()["outs"] for b in (1, 4))
        _check(st, ref, (red, name, D, mode, "dropped"))


@pytest.mark.parametrize("name", ["DistMult", "InterHT"])
@pytest.mark.parametrize("D", [33, 450])
def test_one_rank_equals_train_step(name, D):
    """W = 1 is kge_train_step's algebra on the same inputs: losses to rtol 2e-6, tables within 2e-2 * lr (the
    bars of test_shard_train_gpu.py's world-1 test), at V = 1 and V = 2."""
    E, R, N, W, B = ONE
    c = _case(name, D, ONE)
    lib = L.load()
    for mode in (0, 1):
        st = _Step(c, mode, ONE)
        assert st.vg() == WIDTHS[D]
        res = st.run().results()
        ent, rel = c["ent"].to(DEV), c["rel"].to(DEV)
        assert S.table_vg(name, D, ent, rel) == WIDTHS[D]
        mv = [torch.zeros_like(t) for t in (ent, ent, rel, rel)]
        outs = torch.zeros(2 * B + 1, device=DEV)
        ws = torch.empty(lib.kge_train_step_workspace_size(st.fn, E, R, rel.stride(0), B, N, D), dtype=torch.uint8,
                         device=DEV)
        o = outs.data_ptr()
        L.check(lib.kge_train_step(
            st.fn, mode, ent.data_ptr(), E, ent.stride(0), rel.data_ptr(), R, rel.stride(0), st.ro, st.pos.data_ptr(),
            st.neg.data_ptr(), st.neg.stride(0), B, N, D, c["gamma"], c["rng"], 1.0, 1, 0, st.w.data_ptr(), o, None,
            o + 4, o + 4 * (1 + B), mv[0].data_ptr(), mv[1].data_ptr(), mv[2].data_ptr(), mv[3].data_ptr(), LR, B1, B2,
            EPS, 1, 1, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "kge_train_step")
        torch.cuda.synchronize()
        np.testing.assert_allclose(res["loss"][0].reshape(-1).numpy(), outs[:1].cpu().numpy(), rtol=2e-6, atol=1e-7)
        assert float((res["ent"] - ent.cpu()).abs().max()) <= 2e-2 * LR
        assert float((res["rel"][0] - rel.cpu()).abs().max()) <= 2e-2 * LR


@pytest.mark.parametrize("name", ["ComplEx", "InterHT"])
@pytest.mark.parametrize("which", ["qent_pos", "dq"])
def test_four_byte_aligned_qent_pos_and_dq_narrow_the_vector_width(name, which):
    """shard_pos_kernel and shard_epilogue_kernel read qent_pos and read / write dq with the instance's vector
    width, so pick_vg counts their addresses: with everything else 16-B aligned at D = 64, a qent_pos or a dq
    that starts one float into its buffer gives V = 1 (include/kge_hip.h), not 16-B accesses at 4-B aligned
    addresses. Head-batch for qent_pos (a buffer of its own there); both modes for dq."""
    D = 64
    c = _case(name, D)
    for mode in ((0,) if which == "qent_pos" else (0, 1)):
        st = _Step(c, mode, **({"qpos_k": 1} if which == "qent_pos" else {"dq_k": 1}))
        assert (st.qent_pos if which == "qent_pos" else st.dq[0]).data_ptr() % 16 == 4
        assert st.vg() == (1, 1)
        st.run().intact()
        _check(st, _ref(name, D, mode), (name, which, mode))


def test_null_shard_with_rows_is_still_rejected():
    st = _Step(_case("TransE", 64), 1)
    args = list(st._prefix(0))
    args[2] = None
    rc = st.lib.kge_shard_train_forward(*args, st.stats[0].data_ptr(), st.dq[0].data_ptr(), *st._tail(0))
    with pytest.raises(KGEHipError, match="null pointer"):
        L.check(rc, "kge_shard_train_forward")
    st.untouched()
