"""CPU tests of the stride handling around the library calls: the gradient-buffer allocation of the
autograd wrappers (ops.like_strided), the Adam-moment stride check of the fused train steps
(model.check_adam_moments), and the helpers of the GPU stride tests (tests/strided.py)."""
import pytest
import torch

from customknowledgegraphembedding_amd import ops
from customknowledgegraphembedding_amd.model import check_adam_moments
from tests import strided as S


def _views():
    t = torch.arange(320, dtype=torch.float32).view(10, 32)
    return {"dense": t, "pad4": S.padded(t, 4), "pad1": S.padded(t, 1), "off1": S.offset(t, 1), "off2": S.offset(t, 2)}


@pytest.mark.parametrize("kind", ["dense", "pad4", "pad1", "off1", "off2"])
@pytest.mark.parametrize("zero", [False, True])
def test_like_strided_keeps_the_tables_strides(kind, zero):
    """The library addresses d_ent / d_rel with the table's leading dimension, so a gradient buffer must
    have the table's strides: torch.zeros_like / empty_like of a [10, 32] view of a [10, 36] buffer have
    strides (32, 1), like_strided (36, 1). An offset view is dense and stays dense."""
    v = _views()[kind]
    g = ops.like_strided(v, zero=zero)
    assert g.shape == v.shape and g.stride() == v.stride()
    assert g.dtype == v.dtype and g.device == v.device
    assert g.data_ptr() != v.data_ptr()
    # the buffer behind it holds every element the strides can reach
    assert g.untyped_storage().nbytes() >= 4 * ((v.shape[0] - 1) * v.stride(0) + v.shape[1])
    if zero:
        assert not g.any()
    if kind.startswith("pad"):
        assert torch.zeros_like(v).stride() != v.stride()  # what the wrappers used before


def test_like_strided_of_3d_rows():
    """The dense plugin's [B, n, w] operands: a row-padded view keeps all three strides."""
    buf = torch.zeros(3, 5, 20)
    v = buf[:, :, :16]
    g = ops.like_strided(v, zero=True)
    assert g.shape == v.shape and g.stride() == (100, 20, 1)


def test_adam_moment_stride_check():
    """m / v are addressed with the parameter's leading dimension: a moment with other strides is refused
    (ValueError), one with the parameter's strides passes, for padded, offset and dense parameters."""
    for kind, p in _views().items():
        good = {"exp_avg": ops.like_strided(p, zero=True), "exp_avg_sq": ops.like_strided(p, zero=True)}
        check_adam_moments(p, good)
        if kind.startswith("pad"):
            for key in ("exp_avg", "exp_avg_sq"):
                bad = dict(good)
                bad[key] = torch.zeros_like(p)  # dense strides next to a padded parameter
                assert bad[key].stride() != p.stride()
                with pytest.raises(ValueError, match="leading dimension"):
                    check_adam_moments(p, bad)
    dense = torch.zeros(10, 32)
    with pytest.raises(ValueError):  # a padded moment next to a dense parameter
        check_adam_moments(dense, {"exp_avg": S.padded(dense, 4), "exp_avg_sq": torch.zeros_like(dense)})
    with pytest.raises(ValueError):  # another shape
        check_adam_moments(dense, {"exp_avg": torch.zeros(10, 16), "exp_avg_sq": torch.zeros_like(dense)})
    with pytest.raises(ValueError):  # another dtype
        check_adam_moments(dense, {"exp_avg": torch.zeros(10, 32, dtype=torch.float64),
                                   "exp_avg_sq": torch.zeros_like(dense)})
    # a [1, 1] parameter (the pRotatE modulus): the strides of size-1 dimensions carry no layout
    one = torch.zeros(1, 1)
    check_adam_moments(one, {"exp_avg": torch.zeros(4, 4)[:1, :1], "exp_avg_sq": torch.zeros(1, 1)})


def test_train_step_refuses_mismatched_moments_before_any_launch():
    """train_step_fused reaches the check before it touches the library: a CPU model is enough to see the
    ValueError (with matching moments the same call goes on and fails for want of a GPU instead)."""
    import customknowledgegraphembedding_amd as kge
    from customknowledgegraphembedding_amd.optim import Adam

    m = kge.TFKGEModel("TransE", 12, 3, 8, 6.0, device="cpu", seed=0)
    opt = Adam(m.parameters(), lr=1e-3)
    ent = m.entity_embedding
    for prm in (m.entity_embedding, m.relation_embedding):
        opt.state[prm]["step"] = 0
        opt.state[prm]["exp_avg"] = torch.zeros_like(prm)
        opt.state[prm]["exp_avg_sq"] = torch.zeros_like(prm)
    opt.state[ent]["exp_avg"] = S.padded(torch.zeros(12, 8), 4)
    pos = torch.tensor([[0, 1, 2], [3, 0, 5]])
    neg = torch.randint(0, 12, (2, 4))
    w = torch.ones(2)
    for one_call in (True, False):
        with pytest.raises(ValueError, match="leading dimension"):
            m.train_step_fused(pos, neg, w, 1, opt, one_call=one_call)
    assert opt.state[ent]["step"] == 0


def test_padded_offset_canary_helpers():
    t = torch.arange(12, dtype=torch.float32).view(3, 4)
    p = S.padded(t, 3)
    assert p.stride() == (7, 1) and torch.equal(p, t) and bool(torch.isnan(p._base[:, 4:]).all())
    ids = torch.tensor([[0, 5, 9], [9, 9, 1]])
    pi = S.padded(ids, 2, hi=10)
    assert pi.stride() == (5, 1) and torch.equal(pi, ids)
    pad = pi._base[:, 3:]
    assert bool(((pad >= 0) & (pad < 10)).all())
    assert bool((pad != ids[:, :2]).all())  # differ from the real ids a wrong stride would confuse them with
    for k in (1, 2, 3):
        o = S.offset(t, k)
        assert torch.equal(o, t) and o.is_contiguous() and o.data_ptr() % 16 == (4 * k) % 16
    c = S.canary(3, 4, 9, "cpu")
    assert c.stride() == (9, 1)
    assert bool((c.contiguous().view(torch.int32) == S.CANARY).all())
    before = S.outside_bits(c)
    assert before.numel() == c._base.numel() - 12 and bool((before == S.CANARY).all())
    c.fill_(1.0)  # writes inside the view leave the outside alone
    assert torch.equal(S.outside_bits(c), before)
    c._base.view(-1)[4] = 0.0  # one padding element
    assert not torch.equal(S.outside_bits(c), before)
    m = S.like_table(p, fill=0.0)
    assert m.stride() == p.stride() and not m.any() and bool((S.outside_bits(m) == S.CANARY).all())
    mo = S.like_table(S.offset(t, 1))
    assert mo.is_contiguous() and mo.data_ptr() % 16 == 4


def test_expected_vg_names_the_issue_instances():
    """The widths of test_widths_gpu.py and the instance each is meant to reach (dense, 16-B aligned tables;
    leading dimensions are multiples of D, so D alone decides)."""
    table = {33: (1, 1), 101: (1, 2), 255: (1, 4), 511: (1, 8), 50: (2, 1), 250: (2, 2), 450: (2, 4), 1022: (2, 8),
             300: (4, 2), 16: (4, 1), 1000: (4, 4), 1500: (4, 8)}
    for D, vg in table.items():
        for em, rm in S.MULT.values():
            assert S.expected_vg(D, lds=(em * D, rm * D), offs=(0, D), ptrs=(4096, 8192)) == vg, D
    # padding and base offsets lower V; V = 1 stops at D = 512 (G = 16 is refused)
    assert S.expected_vg(64, lds=(68, 68), ptrs=(4096,)) == (4, 1)
    assert S.expected_vg(64, lds=(66, 64), ptrs=(4096,)) == (2, 1)
    assert S.expected_vg(64, lds=(64, 65), ptrs=(4096,)) == (1, 1)
    assert S.expected_vg(64, lds=(64,), ptrs=(4096 + 8,)) == (2, 1)
    assert S.expected_vg(64, lds=(64,), ptrs=(4096 + 4,)) == (1, 1)
    assert S.expected_vg(520, lds=(520,), ptrs=(4096,)) == (4, 4)
    assert S.expected_vg(520, lds=(522,), ptrs=(4096,)) == (2, 8)
    assert S.expected_vg(520, lds=(521,), ptrs=(4096,))[1] > S.K_MAX_G
    assert S.expected_vg(512, lds=(513,), ptrs=(4096,)) == (1, 8)


@pytest.mark.parametrize("name", ["TransE", "DistMult", "ComplEx", "RotatE", "InterHT"])
@pytest.mark.parametrize("mode", [0, 1])
def test_replica_loss_is_the_oracles_loss(name, mode):
    """S.replica_loss (the reference of tests/test_shard_widths_gpu.py) equals O.tf_train_loss at T = 1 and
    O.upstream_train_loss in both of its reductions at T = 0.5, values and gradients, in fp64; and a candidate
    that is dropped counts like one that was never in the row (softmax) or like a zero term (mean)."""
    from oracle import kge_oracle as O

    c = S.make_case(name, 12, 17, 3, 5, 9, seed=mode)
    w = c["w"].double()

    def both(f):
        e, r = c["ent"].double().requires_grad_(True), c["rel"].double().requires_grad_(True)
        loss = f(e, r)
        loss.backward()
        return loss.item(), e.grad, r.grad

    def same(a, b):
        assert a[0] == pytest.approx(b[0], rel=1e-12)
        for x, y in zip(a[1:], b[1:]):
            assert float((x - y).abs().max()) <= 1e-12 * max(float(y.abs().max()), 1.0)

    args = (c["pos"], c["neg"], w)
    same(both(lambda e, r: S.replica_loss(name, e, r, *args, mode, c["gamma"], c["rng"])[0]),
         both(lambda e, r: O.tf_train_loss(name, e, r, *args, [mode], c["gamma"], c["rng"])))
    for red, adv in (("detached", True), ("mean", False)):
        same(both(lambda e, r: S.replica_loss(name, e, r, *args, mode, c["gamma"], c["rng"], red, 0.5)[0]),
             both(lambda e, r: O.upstream_train_loss(name, e, r, *args, mode, c["gamma"], c["rng"], adversarial=adv,
                                                     temperature=0.5)))
    # dropping the last two candidates of every row: the softmax forms equal the loss of the shorter rows
    keep = torch.ones(5, 9, dtype=torch.bool)
    keep[:, 7:] = False
    short = (c["pos"], c["neg"][:, :7], w)
    same(both(lambda e, r: S.replica_loss(name, e, r, *args, mode, c["gamma"], c["rng"], "tf", 0.5, keep)[0]),
         both(lambda e, r: S.replica_loss(name, e, r, *short, mode, c["gamma"], c["rng"], "tf", 0.5)[0]))
    full = S.replica_loss(name, c["ent"].double(), c["rel"].double(), *short, mode, c["gamma"], c["rng"], "mean")[1]
    drop = S.replica_loss(name, c["ent"].double(), c["rel"].double(), *args, mode, c["gamma"], c["rng"], "mean",
                          keep=keep)[1]
    assert torch.allclose(drop * 9, full * 7, rtol=1e-12, atol=0)
