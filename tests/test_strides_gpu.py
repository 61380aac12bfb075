"""Padded leading dimensions and offset table bases through the raw C ABI (include/kge_hip.h). Every matrix
argument carries a leading dimension; the rest of the suite passes dense tensors, so a kernel that indexed a row
by its width instead of its ld, or wrote a vector past a row's end, would pass it. Here every table is a view
(tests/strided.py): row-padded by 4, 2 or 1 floats with NaN in the padding (the kernels' vector width stays 4,
becomes 2, becomes 1), each table padded alone, or starting 1 or 2 floats into its buffer; candidate ids have
neg_ld = N + 3 with valid but different ids in the padding; every output has ld = width + 5 over a canary
pattern; gradients and Adam moments are laid out like their table (they share its ld).

Expected: with pad 4 on a 16-B base the same kernel instance runs, so results are bitwise those of the dense
call (the atomic backward: within the gradient bar); every layout is within the oracle bars of
test_widths_gpu.py; nothing outside a view is written: every padding element of every output, gradient,
in-place table and moment keeps its bits. Where the layout leaves V = 1 at D = 520 the library has no
register-resident instance and must refuse the call (KGE_ENOTSUP) without writing anything."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from customknowledgegraphembedding_amd import _lib as L
from customknowledgegraphembedding_amd import ops
from customknowledgegraphembedding_amd._lib import FN_IDS, KGEHipError
from oracle import kge_oracle as O
from tests import strided as S
from tests.conftest import rel_close
from tests.test_parity_gpu import _grad_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
LR = 1e-3
NAMES = ["InterHT", "ComplEx", "TransE"]  # three-, two- and one-part rows
DIMS = [64, 520]
E, R = 300, 5
SHAPE, WIDE = (6, 24), (7, 130)  # (B, N); N = 130 reaches the XCD-sliced and tile forms
# layout -> (entity table, relation table): ("pad", floats per row) | ("off", floats before the base) | dense
LAYOUTS = {"pad4": (("pad", 4), ("pad", 4)), "pad2": (("pad", 2), ("pad", 2)), "pad1": (("pad", 1), ("pad", 1)),
           "ent_pad1": (("pad", 1), None), "rel_pad2": (None, ("pad", 2)),
           "off1": (("off", 1), ("off", 1)), "off2": (("off", 2), ("off", 2))}
case_params = pytest.mark.parametrize("name,D,layout", [(n, d, k) for n in NAMES for d in DIMS for k in LAYOUTS])


def _lay(t, spec):
    if spec is None:
        return t.to(DEV)
    return S.padded(t, spec[1], DEV) if spec[0] == "pad" else S.offset(t, spec[1], DEV)


@functools.lru_cache(maxsize=None)
def _case(name, D, B, N):
    return S.make_case(name, D, E, R, B, N, seed=D + N)


def _tables(c, layout):
    es, rs = LAYOUTS[layout] if layout else (None, None)
    return _lay(c["ent"], es), _lay(c["rel"], rs)


def _supported(c, ent, rel):
    return S.table_vg(c["name"], c["D"], ent, rel)[1] <= S.K_MAX_G


def _refused(f):
    with pytest.raises(KGEHipError, match="register-resident"):
        f()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _neg(c, pad=True):
    return S.padded(c["neg"], 3, DEV, hi=E) if pad else c["neg"].to(DEV)


def _out(rows, w, pad=True):
    return S.canary(rows, w, w + 5 if pad else w, DEV)


def _intact(views, before):
    for i, (v, b) in enumerate(zip(views, before)):
        assert torch.equal(S.outside_bits(v), b), f"buffer {i}: an element outside the view was written"


def _eq(a, b):
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def test_layouts_reach_the_intended_vector_widths():
    """pad 4 keeps V = 4, pad 2 and a 2-float offset give V = 2, pad 1 and a 1-float offset V = 1, also when
    only one of the two tables is padded."""
    want = {"pad4": 4, "pad2": 2, "pad1": 1, "ent_pad1": 1, "rel_pad2": 2, "off1": 1, "off2": 2}
    for name in NAMES:
        c = _case(name, 64, *SHAPE)
        for layout, v in want.items():
            ent, rel = _tables(c, layout)
            assert S.table_vg(name, 64, ent, rel)[0] == v, (name, layout)
    c = _case("TransE", 520, *SHAPE)
    assert not _supported(c, *_tables(c, "pad1")) and _supported(c, *_tables(c, "pad2"))


# ------------------------------------------------------------------------------------------------
# forward: kge_score_indexed_ex, kge_step_forward_ex, kge_step_finish
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fwd_ref(name, D, B, N, mode):
    """(raw scores [B, N | 1], reduced negatives [B]) in fp64."""
    c = _case(name, D, B, N)
    s = O.score(name, c["ent"].double(), c["rel"].double(), c["pos"], c["neg"], mode, c["gamma"], c["rng"], c["mod"])
    return s.numpy(), O.adv_reduce(s)[:, 0].numpy()


@case_params
def test_score_indexed_padded(name, D, layout):
    fn, ro = FN_IDS[name], S.rel_off(name, D)
    for (B, N), orders in ((SHAPE, ("row",)), (WIDE, ("xcd", "tile"))):
        c = _case(name, D, B, N)
        pos = c["pos"].to(DEV)
        ent, rel = _tables(c, layout)
        dent, drel = _tables(c, None)
        for mode in (0, 1, 3):
            n = 1 if mode == 3 else N
            for order in orders:
                out = _out(B, n)
                before = [S.outside_bits(out)]

                def run(e=ent, r=rel, o=out, pad=True):
                    ops.score_indexed_raw(fn, mode, e, r, ro, pos, _neg(c, pad), D, c["gamma"], c["rng"], c["mod"],
                                          out=o, forms=dict(step_order=order))
                    torch.cuda.synchronize()
                    return o

                if not _supported(c, ent, rel):
                    _refused(run)
                    assert bool((out.contiguous().view(torch.int32) == S.CANARY).all())
                    _intact([out], before)
                    continue
                run()
                _intact([out], before)
                err = rel_close(out.cpu().numpy(), _fwd_ref(name, D, B, N, mode)[0])
                assert err <= TOL, (mode, order, err)
                if layout == "pad4":
                    assert _eq(out, run(dent, drel, _out(B, n, False), False)), (mode, order)


@case_params
def test_step_forward_and_finish_padded(name, D, layout):
    """kge_step_forward_ex (the row form with and without InterHT's candidate statistics at N = 24, the
    library's choice, tiles, at N = 130) and kge_step_finish on the padded scores it left."""
    fn, ro = FN_IDS[name], S.rel_off(name, D)
    for (B, N), order in ((SHAPE, "row"), (WIDE, None)):
        c = _case(name, D, B, N)
        pos = c["pos"].to(DEV)
        ent, rel = _tables(c, layout)
        for mode in (0, 1):
            for with_stats in ((False, True) if (name == "InterHT" and order == "row") else (False,)):
                ns = _out(B, N)
                stats = torch.empty(B * N, 2, device=DEV) if with_stats else None
                before = [S.outside_bits(ns)]

                def run(e=ent, r=rel, o=ns, pad=True, st=stats):
                    out = ops.step_forward_raw(fn, mode, e, r, ro, pos, _neg(c, pad), D, c["gamma"], c["rng"],
                                               modulus=c["mod"], neg_scores=o, cand_stats=st,
                                               forms=None if order is None else dict(step_order=order))
                    torch.cuda.synchronize()
                    return out

                def finish(e=ent, r=rel, o=ns):
                    out = ops.step_finish_raw(fn, e, r, ro, pos, D, c["gamma"], c["rng"], o, modulus=c["mod"])
                    torch.cuda.synchronize()
                    return out

                if not _supported(c, ent, rel):
                    _refused(run)
                    _refused(finish)
                    _intact([ns], before)
                    continue
                out_neg, out_pos, _, pos_scores = run()
                _intact([ns], before)
                s_ref, n_ref = _fwd_ref(name, D, B, N, mode)
                p_ref = _fwd_ref(name, D, B, N, 3)[0][:, 0]
                lp_ref = F.logsigmoid(torch.from_numpy(p_ref)).numpy()
                f_neg, f_pos, f_ps = finish()
                _intact([ns], before)
                errs = (rel_close(ns.cpu().numpy(), s_ref), rel_close(out_neg.cpu().numpy(), n_ref),
                        rel_close(pos_scores.cpu().numpy(), p_ref), rel_close(out_pos.cpu().numpy(), lp_ref),
                        rel_close(f_neg.cpu().numpy(), n_ref), rel_close(f_ps.cpu().numpy(), p_ref),
                        rel_close(f_pos.cpu().numpy(), lp_ref))
                assert max(errs) <= TOL, (mode, order, errs)
                if layout == "pad4":
                    dent, drel = _tables(c, None)
                    dns = _out(B, N, False)
                    d = run(dent, drel, dns, False, torch.empty(B * N, 2, device=DEV) if with_stats else None)
                    assert all(_eq(a, b) for a, b in zip((out_neg, out_pos, ns, pos_scores), d)), (mode, order)
                    assert all(_eq(a, b) for a, b in zip((f_neg, f_pos, f_ps), finish(dent, drel, dns))), mode


# ------------------------------------------------------------------------------------------------
# kge_neg_reduce, kge_neg_reduce_bwd
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [24, 130, 1030])
@pytest.mark.parametrize("adversarial,detach", [(1, 0), (1, 1), (0, 0)])
def test_neg_reduce_and_bwd_padded(N, adversarial, detach):
    """scores with ld = N + 3 (NaN padding), d_scores with ld = N + 5; N = 1 030 is past the register-resident
    row reduction."""
    B = 6
    g = torch.Generator().manual_seed(N)
    s = torch.randn(B, N, generator=g) * 3
    go = torch.randn(B, generator=g)
    s64 = s.double().requires_grad_(True)
    if adversarial:
        w = torch.softmax(s64, 1)
        ref = ((w.detach() if detach else w) * F.logsigmoid(-s64)).sum(1)
    else:
        ref = F.logsigmoid(-s64).mean(1)
    (ref * go.double()).sum().backward()
    sp = S.padded(s, 3, DEV)
    got = ops.neg_reduce_raw(sp, 1.0, bool(adversarial))
    assert rel_close(got.cpu().numpy(), ref.detach().numpy()) <= TOL
    assert torch.equal(got, ops.neg_reduce_raw(s.to(DEV), 1.0, bool(adversarial)))
    ds = _out(B, N)
    before = [S.outside_bits(ds)]
    lib = L.load()
    god = go.to(DEV)
    L.check(lib.kge_neg_reduce_bwd(sp.data_ptr(), B, N, sp.stride(0), 1.0, adversarial, detach, god.data_ptr(),
                                   ds.data_ptr(), ds.stride(0), _st()), "kge_neg_reduce_bwd")
    torch.cuda.synchronize()
    _intact([ds], before)
    assert _grad_close(ds.cpu(), s64.grad)


# ------------------------------------------------------------------------------------------------
# kge_score_dense, kge_score_dense_bwd: the model_func plugin on pre-gathered rows
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense_ref(name, D, mode):
    B, N = SHAPE
    c = _case(name, D, B, N)
    h, r, t = (x.clone().requires_grad_(True)
               for x in O.gather_rows(c["ent"].double(), c["rel"].double(), c["pos"], c["neg"], mode))
    go = torch.from_numpy(np.random.RandomState(mode).normal(size=(B, 1 if mode == 3 else N)))
    s = O.model_func(name, h, r, t, mode, c["gamma"], c["rng"], c["mod"])
    (s * go).sum().backward()
    return s.detach().numpy(), go.float(), (h, r, t)


@case_params
def test_score_dense_and_bwd_padded(name, D, layout):
    fn, ro = FN_IDS[name], S.rel_off(name, D)
    B, N = SHAPE
    c = _case(name, D, B, N)
    es, rs = LAYOUTS[layout]
    lib = L.load()
    for mode in (0, 1, 3):
        s_ref, go, (h64, r64, t64) = _dense_ref(name, D, mode)
        n = 1 if mode == 3 else N
        rows = [x.detach().float().reshape(-1, x.shape[-1]) for x in (h64, r64, t64)]  # [B * Nh, w], [B, w], ...
        h, r, t = _lay(rows[0], es), _lay(rows[1], rs), _lay(rows[2], es)
        vg = S.expected_vg(D, lds=(h.stride(0), r.stride(0), t.stride(0)), offs=(ro,),
                           ptrs=(h.data_ptr(), r.data_ptr(), t.data_ptr()))
        out = _out(B, n)
        ds = S.padded(go, 5, DEV)
        grads = [S.like_table(x, fill=0.0) for x in (h, r, t)]  # the entry point accumulates
        before = [S.outside_bits(v) for v in [out] + grads]

        def fwd():
            L.check(lib.kge_score_dense(fn, mode, h.data_ptr(), h.stride(0), r.data_ptr(), r.stride(0), ro,
                                        t.data_ptr(), t.stride(0), B, n, D, c["gamma"], c["rng"], c["mod"],
                                        out.data_ptr(), out.stride(0), _st()), "kge_score_dense")
            torch.cuda.synchronize()

        def bwd():
            L.check(lib.kge_score_dense_bwd(fn, mode, h.data_ptr(), h.stride(0), r.data_ptr(), r.stride(0), ro,
                                            t.data_ptr(), t.stride(0), B, n, D, c["gamma"], c["rng"], c["mod"],
                                            ds.data_ptr(), ds.stride(0), grads[0].data_ptr(), grads[1].data_ptr(),
                                            grads[2].data_ptr(), None, _st()), "kge_score_dense_bwd")
            torch.cuda.synchronize()

        if vg[1] > S.K_MAX_G:
            _refused(fwd)
            _refused(bwd)
            _intact([out] + grads, before)
            continue
        fwd()
        bwd()
        _intact([out] + grads, before)
        assert rel_close(out.cpu().numpy(), s_ref) <= TOL, mode
        for got, ref in zip(grads, (h64, r64, t64)):
            assert _grad_close(got.cpu(), ref.grad.reshape(got.shape)), mode
        if layout == "pad4":
            dense = ops.score_dense_raw(fn, mode, *(x.detach().float().to(DEV) for x in (h64, r64, t64)), ro, D,
                                        c["gamma"], c["rng"], c["mod"])
            assert _eq(out, dense), mode


# ------------------------------------------------------------------------------------------------
# backward: kge_score_indexed_bwd (atomic), kge_step_backward (deterministic)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bwd_ref(name, D, mode):
    B, N = SHAPE
    c = _case(name, D, B, N)
    e = c["ent"].double().requires_grad_(True)
    r = c["rel"].double().requires_grad_(True)
    go = torch.from_numpy(np.random.RandomState(10 + mode).normal(size=(B, 1 if mode == 3 else N)))
    (O.score(name, e, r, c["pos"], c["neg"], mode, c["gamma"], c["rng"], c["mod"]) * go).sum().backward()
    return go.float(), e.grad, r.grad


@case_params
def test_score_indexed_bwd_padded(name, D, layout):
    """The atomic-scatter backward accumulates into d_ent / d_rel laid out like their tables; d_scores has
    ld = N + 5."""
    fn, ro = FN_IDS[name], S.rel_off(name, D)
    B, N = SHAPE
    c = _case(name, D, B, N)
    ent, rel = _tables(c, layout)
    pos, neg = c["pos"].to(DEV), _neg(c)
    lib = L.load()
    for mode in (0, 1, 3):
        go, de_ref, dr_ref = _bwd_ref(name, D, mode)
        n = 1 if mode == 3 else N
        ds = S.padded(go, 5, DEV)
        d_ent, d_rel = S.like_table(ent, fill=0.0), S.like_table(rel, fill=0.0)
        assert d_ent.stride() == ent.stride() and d_rel.stride() == rel.stride()
        before = [S.outside_bits(v) for v in (d_ent, d_rel)]

        def run():
            L.check(lib.kge_score_indexed_bwd(
                fn, mode, ent.data_ptr(), E, ent.stride(0), rel.data_ptr(), R, rel.stride(0), ro, pos.data_ptr(),
                None if mode == 3 else neg.data_ptr(), neg.stride(0), B, n, D, c["gamma"], c["rng"], c["mod"],
                ds.data_ptr(), ds.stride(0), d_ent.data_ptr(), d_rel.data_ptr(), None, None, _st()),
                "kge_score_indexed_bwd")
            torch.cuda.synchronize()

        if not _supported(c, ent, rel):
            _refused(run)
            assert not d_ent.any() and not d_rel.any()
            _intact([d_ent, d_rel], before)
            continue
        run()
        _intact([d_ent, d_rel], before)
        assert _grad_close(d_ent.cpu(), de_ref), mode
        assert _grad_close(d_rel.cpu(), dr_ref), mode


@functools.lru_cache(maxsize=None)
def _step_ref(name, D, mode):
    """One train step's loss and gradients in fp64, and the tables and moments after one Keras Adam step."""
    B, N = SHAPE
    c = _case(name, D, B, N)
    e = c["ent"].double().requires_grad_(True)
    r = c["rel"].double().requires_grad_(True)
    loss = O.tf_train_loss(name, e, r, c["pos"], c["neg"], c["w"].double(), [mode], c["gamma"], c["rng"], c["mod"])
    loss.backward()
    out = {"loss": loss.item(), "d_ent": e.grad, "d_rel": r.grad}
    for key, p, g in (("ent", c["ent"].double(), e.grad), ("rel", c["rel"].double(), r.grad)):
        z = torch.zeros_like(p)
        out[key], out["m_" + key], _ = O.keras_adam_step(p, g, z, z, 1, LR)
    return out


def _step_forward(c, fn, mode, ent, rel, pos, neg, pad=True):
    """The forward half of the split path on padded buffers -> (ns, ps, d_out, stats, loss)."""
    B, N, D = c["B"], c["N"], c["D"]
    ns = _out(B, N, pad)
    stats = torch.empty(B * N, 2, device=DEV) if c["name"] == "InterHT" else None
    out_neg, out_pos, _, ps = ops.step_forward_raw(fn, mode, ent, rel, S.rel_off(c["name"], D), pos, neg, D,
                                                   c["gamma"], c["rng"], modulus=c["mod"], neg_scores=ns,
                                                   cand_stats=stats)
    loss, d_out = ops.step_loss_raw(out_neg, out_pos, c["w"].to(DEV))
    return ns, ps, d_out, stats, loss


@case_params
def test_step_backward_padded(name, D, layout):
    """kge_step_backward overwrites d_ent / d_rel (here canary-filled, laid out like their tables) in their
    tables' columns only; InterHT with the forward's candidate statistics (streaming phase 1 at G = 4) and
    without."""
    fn, ro = FN_IDS[name], S.rel_off(name, D)
    B, N = SHAPE
    c = _case(name, D, B, N)
    pos = c["pos"].to(DEV)
    lib = L.load()

    def run(ent, rel, neg, mode, use_stats, pad=True):
        ns, ps, d_out, stats, loss = _step_forward(c, fn, mode, ent, rel, pos, neg, pad)
        d_ent, d_rel = S.like_table(ent), S.like_table(rel)
        before = [S.outside_bits(v) for v in (d_ent, d_rel)]
        nbytes = lib.kge_step_backward_workspace_size(fn, E, B, N, D)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        L.check(lib.kge_step_backward(
            fn, mode, ent.data_ptr(), E, ent.stride(0), rel.data_ptr(), R, rel.stride(0), ro, pos.data_ptr(),
            neg.data_ptr(), neg.stride(0), B, N, D, c["gamma"], c["rng"], c["mod"], 1.0, 1, 0, ns.data_ptr(),
            ns.stride(0), ps.data_ptr(), d_out.data_ptr(), d_out.data_ptr(), d_ent.data_ptr(), d_rel.data_ptr(), None,
            stats.data_ptr() if (use_stats and stats is not None) else None, ws.data_ptr(), ws.numel(), _st()),
            "kge_step_backward")
        torch.cuda.synchronize()
        _intact([d_ent, d_rel], before)
        return loss, d_ent, d_rel

    ent, rel = _tables(c, layout)
    if not _supported(c, ent, rel):
        _refused(lambda: run(ent, rel, _neg(c), 1, False))
        return
    for mode in (0, 1):
        ref = _step_ref(name, D, mode)
        for use_stats in ((True, False) if name == "InterHT" else (False,)):
            loss, d_ent, d_rel = run(ent, rel, _neg(c), mode, use_stats)
            assert rel_close(loss.item(), ref["loss"]) <= TOL
            assert _grad_close(d_ent.cpu(), ref["d_ent"]), (mode, use_stats)
            assert _grad_close(d_rel.cpu(), ref["d_rel"]), (mode, use_stats)
            if layout == "pad4":
                dent, drel = _tables(c, None)
                _, e2, r2 = run(dent, drel, _neg(c, False), mode, use_stats, False)
                assert torch.equal(d_ent, e2) and torch.equal(d_rel, r2), (mode, use_stats)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("layout", [None, "pad4", "pad1", "off1"])
def test_step_backward_empty_batch_zeroes_the_tables_columns_only(name, layout):
    """B = 0: every row of d_ent / d_rel becomes zero over the table's width (InterHT: all three thirds of a
    relation row), and nothing else is written; the last row of a padded view ends at its width."""
    D, N = 64, 24
    fn, ro = FN_IDS[name], S.rel_off(name, D)
    c = _case(name, D, *SHAPE)
    ent, rel = _tables(c, layout)
    d_ent, d_rel = S.like_table(ent), S.like_table(rel)
    before = [S.outside_bits(v) for v in (d_ent, d_rel)]
    ids = torch.zeros(4, dtype=torch.int64, device=DEV)  # never read: the pointers only must not be NULL
    fl = torch.zeros(4, device=DEV)
    lib = L.load()
    ws = torch.empty(max(lib.kge_step_backward_workspace_size(fn, E, 0, N, D), 1), dtype=torch.uint8, device=DEV)
    L.check(lib.kge_step_backward(
        fn, 1, ent.data_ptr(), E, ent.stride(0), rel.data_ptr(), R, rel.stride(0), ro, ids.data_ptr(), ids.data_ptr(),
        N, 0, N, D, c["gamma"], c["rng"], c["mod"], 1.0, 1, 0, fl.data_ptr(), N, fl.data_ptr(), fl.data_ptr(),
        fl.data_ptr(), d_ent.data_ptr(), d_rel.data_ptr(), None, None, ws.data_ptr(), ws.numel(), _st()),
        "kge_step_backward")
    torch.cuda.synchronize()
    _intact([d_ent, d_rel], before)
    assert d_ent.shape == ent.shape and not d_ent.any() and not d_rel.any()


# ------------------------------------------------------------------------------------------------
# in place: kge_step_backward_adam, kge_train_step
# ------------------------------------------------------------------------------------------------
def _adam_buffers(ent, rel):
    return [S.like_table(t, fill=0.0) for t in (ent, ent, rel, rel)]  # m_ent, v_ent, m_rel, v_rel


def _check_step(got, ref, what):
    loss, ent, rel, m_ent, m_rel = got
    assert rel_close(loss.item(), ref["loss"]) <= TOL, what
    assert float((ent.cpu().double() - ref["ent"]).abs().max()) <= 5e-2 * LR, what
    assert float((rel.cpu().double() - ref["rel"]).abs().max()) <= 5e-2 * LR, what
    assert _grad_close(m_ent.cpu(), ref["m_ent"]), what
    assert _grad_close(m_rel.cpu(), ref["m_rel"]), what


@case_params
def test_step_backward_adam_padded(name, D, layout):
    """The tables (NaN padding) and their moments (canary padding) are updated in place in the tables' columns
    only."""
    fn, ro = FN_IDS[name], S.rel_off(name, D)
    B, N = SHAPE
    c = _case(name, D, B, N)
    pos = c["pos"].to(DEV)
    lib = L.load()

    def run(layout_, mode, pad=True):
        ent, rel = _tables(c, layout_)
        neg = _neg(c, pad)
        ns, ps, d_out, stats, loss = _step_forward(c, fn, mode, ent, rel, pos, neg, pad)
        mv = _adam_buffers(ent, rel)
        before = [S.outside_bits(v) for v in [ent, rel] + mv]
        nbytes = lib.kge_step_backward_adam_workspace_size(fn, E, R, rel.stride(0), B, N, D)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        L.check(lib.kge_step_backward_adam(
            fn, mode, ent.data_ptr(), E, ent.stride(0), rel.data_ptr(), R, rel.stride(0), ro, pos.data_ptr(),
            neg.data_ptr(), neg.stride(0), B, N, D, c["gamma"], c["rng"], None, 0.0, 1.0, 1, 0, ns.data_ptr(),
            ns.stride(0), ps.data_ptr(), d_out.data_ptr(), d_out.data_ptr(), mv[0].data_ptr(), mv[1].data_ptr(),
            mv[2].data_ptr(), mv[3].data_ptr(), None, None, LR, 0.9, 0.999, 1e-7, 1, 1,
            None if stats is None else stats.data_ptr(), ws.data_ptr(), ws.numel(), _st()), "kge_step_backward_adam")
        torch.cuda.synchronize()
        _intact([ent, rel] + mv, before)
        return loss, ent, rel, mv[0], mv[2], mv[1], mv[3]

    if not _supported(c, *_tables(c, layout)):
        _refused(lambda: run(layout, 1))
        return
    for mode in (0, 1):
        got = run(layout, mode)
        _check_step(got[:5], _step_ref(name, D, mode), (name, D, layout, mode))
        if layout == "pad4":
            assert all(torch.equal(a, b) for a, b in zip(got, run(None, mode, False))), mode


@case_params
def test_train_step_padded(name, D, layout):
    """kge_train_step: the fused forward + query gradient and epilogue (G <= 4), or its fallback (D = 520 at
    V = 2: G = 8), on padded tables, ids and moments; loss, out_neg and out_pos are dense [1] / [B] outputs."""
    fn, ro = FN_IDS[name], S.rel_off(name, D)
    B, N = SHAPE
    c = _case(name, D, B, N)
    pos, w = c["pos"].to(DEV), c["w"].reshape(-1).to(DEV)
    lib = L.load()

    def run(layout_, mode, pad=True):
        ent, rel = _tables(c, layout_)
        neg = _neg(c, pad)
        mv = _adam_buffers(ent, rel)
        outs = S.canary(1, 2 * B + 1, 2 * B + 1, DEV)  # loss | out_neg | out_pos
        before = [S.outside_bits(v) for v in [ent, rel, outs] + mv]
        nbytes = lib.kge_train_step_workspace_size(fn, E, R, rel.stride(0), B, N, D)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        o = outs.data_ptr()
        L.check(lib.kge_train_step(
            fn, mode, ent.data_ptr(), E, ent.stride(0), rel.data_ptr(), R, rel.stride(0), ro, pos.data_ptr(),
            neg.data_ptr(), neg.stride(0), B, N, D, c["gamma"], c["rng"], 1.0, 1, 0, w.data_ptr(), o, None, o + 4,
            o + 4 * (1 + B), mv[0].data_ptr(), mv[1].data_ptr(), mv[2].data_ptr(), mv[3].data_ptr(), LR, 0.9, 0.999,
            1e-7, 1, 1, ws.data_ptr(), ws.numel(), _st()), "kge_train_step")
        torch.cuda.synchronize()
        _intact([ent, rel, outs] + mv, before)
        return outs[0, 0].clone(), ent, rel, mv[0], mv[2], mv[1], mv[3], outs[0, 1:].clone()

    if not _supported(c, *_tables(c, layout)):
        _refused(lambda: run(layout, 1))
        return
    for mode in (0, 1):
        got = run(layout, mode)
        _check_step(got[:5], _step_ref(name, D, mode), (name, D, layout, mode))
        n_ref = _fwd_ref(name, D, B, N, mode)[1]
        lp_ref = F.logsigmoid(torch.from_numpy(_fwd_ref(name, D, B, N, 3)[0][:, 0])).numpy()
        assert rel_close(got[7][:B].cpu().numpy(), n_ref) <= TOL and rel_close(got[7][B:].cpu().numpy(), lp_ref) <= TOL
        if layout == "pad4":
            assert all(torch.equal(a, b) for a, b in zip(got, run(None, mode, False))), mode


# ------------------------------------------------------------------------------------------------
# row-sharded pieces: kge_gather_rows, kge_score_sharded
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [64, 130, 33])
@pytest.mark.parametrize("spec", [None, ("pad", 4), ("pad", 1), ("off", 1), ("off", 2)])
@pytest.mark.parametrize("id_stride", [1, 3])
def test_gather_rows_padded(width, spec, id_stride):
    """out[i] = table[ids[i * id_stride] - lo] or zeros when the shard does not own the id, for a padded or
    offset table, out_ld = width + 5 (dword path) and width + 8 (16-B path where the table allows it)."""
    rows, lo, n = 50, 20, 23
    g = torch.Generator().manual_seed(width)
    tab = torch.randn(rows, width, generator=g)
    ids = torch.randint(0, 90, (n, id_stride), generator=g)  # ids outside [lo, lo + rows) are foreign
    ids[0, 0], ids[1, 0], ids[2, 0] = lo, lo + rows - 1, lo + rows
    own = (ids[:, 0] >= lo) & (ids[:, 0] < lo + rows)
    ref = torch.where(own[:, None], tab[(ids[:, 0] - lo).clamp(0, rows - 1)], torch.zeros(1))
    t = _lay(tab, spec)
    idp = ids.to(DEV)  # row stride id_stride: with 3, the two columns after the used one hold other valid ids
    assert idp.stride(0) == id_stride
    lib = L.load()
    for out_ld in (width + 5, width + 8):
        out = S.canary(n, width, out_ld, DEV)
        before = [S.outside_bits(out)]
        L.check(lib.kge_gather_rows(t.data_ptr(), rows, t.stride(0), lo, idp.data_ptr(), idp.stride(0), n, width,
                                    out.data_ptr(), out.stride(0), _st()), "kge_gather_rows")
        torch.cuda.synchronize()
        _intact([out], before)
        assert torch.equal(out.cpu(), ref), (out_ld,)


@case_params
def test_score_sharded_padded(name, D, layout):
    """kge_score_sharded: pre-assembled query rows (q_ld) against a shard of the entity table (shard_ld,
    rows [lo, lo + rows)); candidates the shard does not own score exactly 0."""
    fn, ro = FN_IDS[name], S.rel_off(name, D)
    es, rs = LAYOUTS[layout]
    lo, hi = 100, 220
    lib = L.load()
    for (B, N) in (SHAPE, WIDE):
        c = _case(name, D, B, N)
        pos, neg = c["pos"].to(DEV), _neg(c)
        rel = _lay(c["rel"], rs)
        shard = _lay(c["ent"][lo:hi], es)
        for mode in (0, 1, 3):
            n = 1 if mode == 3 else N
            q = _lay(c["ent"][c["pos"][:, 2 if mode == 0 else 0]], es)
            vg = S.expected_vg(D, lds=(q.stride(0), rel.stride(0), shard.stride(0)), offs=(ro,),
                               ptrs=(q.data_ptr(), rel.data_ptr(), shard.data_ptr()))
            out = _out(B, n)
            before = [S.outside_bits(out)]

            def run():
                L.check(lib.kge_score_sharded(
                    fn, mode, q.data_ptr(), q.stride(0), rel.data_ptr(), R, rel.stride(0), ro, shard.data_ptr(),
                    hi - lo, shard.stride(0), lo, pos.data_ptr(), None if mode == 3 else neg.data_ptr(),
                    neg.stride(0), B, n, D, c["gamma"], c["rng"], c["mod"], out.data_ptr(), out.stride(0), _st()),
                    "kge_score_sharded")
                torch.cuda.synchronize()

            if vg[1] > S.K_MAX_G:
                _refused(run)
                _intact([out], before)
                continue
            run()
            _intact([out], before)
            cand = c["pos"][:, 2:3] if mode == 3 else c["neg"]
            own = ((cand >= lo) & (cand < hi)).numpy()
            ref = np.where(own, _fwd_ref(name, D, B, N, mode)[0], 0.0)
            got = out.cpu().numpy()
            assert rel_close(got, ref) <= TOL, (mode, N)
            assert (got[~own] == 0).all(), (mode, N)


# ------------------------------------------------------------------------------------------------
# through ops: the gradient of a padded-view table
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES + ["pRotatE"])
@pytest.mark.parametrize("pad", [4, 2, 1])
def test_ops_gradients_of_padded_view_tables(name, pad):
    """ops.score_indexed and ops.step_forward accept any row-contiguous table, so a row-padded view; the
    gradient buffers they hand to the library must then have the view's strides (ops.like_strided), or the
    library, which addresses d_ent with ent_ld, writes past their end. The gradients equal the dense tables'
    on the real columns (bitwise for the deterministic step backward at pad 4)."""
    D = 64
    B, N = SHAPE
    c = S.make_case(name, D, E, R, B, N, seed=pad)
    fn, kw = FN_IDS[name], dict(rel_off=S.rel_off(name, D))
    pos, neg, w = c["pos"].to(DEV), c["neg"].to(DEV), c["w"].to(DEV)
    go = torch.randn(B, N, generator=torch.Generator().manual_seed(1)).to(DEV)

    def grads(ent, rel, step):
        ent.requires_grad_(True)
        rel.requires_grad_(True)
        mod = torch.tensor([[c["mod"]]], device=DEV, requires_grad=True) if name == "pRotatE" else None
        for mode in (0, 1):
            if step:
                n, p = ops.step_forward(fn, mode, ent, rel, pos, neg, D, c["gamma"], c["rng"], modulus=mod, **kw)
                ops.step_loss(n, p, w).backward()
            else:
                (ops.score_indexed(fn, mode, ent, rel, pos, neg, D, c["gamma"], c["rng"], modulus=mod, **kw)
                 * go).sum().backward()
        torch.cuda.synchronize()
        return ent.grad, rel.grad

    for step in (True, False):
        de, dr = grads(c["ent"].to(DEV), c["rel"].to(DEV), step)
        pe, pr = grads(S.padded(c["ent"], pad, DEV), S.padded(c["rel"], pad, DEV), step)
        assert pe.shape == de.shape and pr.shape == dr.shape
        if step and pad == 4:
            assert torch.equal(pe, de) and torch.equal(pr, dr)
        assert _grad_close(pe.cpu(), de.cpu().double()), (step, pad)
        assert _grad_close(pr.cpu(), dr.cpu().double()), (step, pad)
