"""Helpers of the vector-width and leading-dimension tests (test_widths_gpu.py, test_strides_gpu.py,
test_shard_widths_gpu.py, test_strided_cpu.py): non-dense views of tables, ids and outputs, a Python
restatement of the library's width choice (pick_vg, csrc/kge_abi.hip), small seeded cases shared by those
tests, and the replica loss the row-sharded train step is held to. A plain module: nothing here is a fixture or
changes how the suite is collected."""
import numpy as np
import torch

from oracle import kge_oracle as O

# entity / relation row widths in units of the per-half width D
MULT = {"TransE": (1, 1), "DistMult": (1, 1), "ComplEx": (2, 2), "RotatE": (2, 1), "pRotatE": (1, 1),
        "InterHT": (2, 3)}
FNS = list(MULT)
CANARY = 0x5CA1AB1E  # as fp32: 3.64e17, finite, never a plausible result
K_WAVE, K_MAX_G, K_FWD_GRAD_MAX_G, K_BWD_MAX_G = 64, 8, 4, 16  # csrc/kge_internal.h


def rel_off(name, D):
    """Where the part of a relation row a score function reads starts (InterHT: the middle third)."""
    return D if name == "InterHT" else 0


def model_flags(name):
    """(double_entity, double_relation, triple_relation) of TFKGEModel for a score function."""
    return MULT[name][0] == 2, name == "ComplEx", name == "InterHT"


def make_case(name, D, E, R, B, N, seed=0, gamma=11.0):
    """CPU fp32 tables (O.make_tables), a [B, 3] positive batch, [B, N] candidates, [B, 1] weights in
    [0.2, 1], gamma, the embedding range and the pRotatE modulus of a seeded case."""
    em, rm = MULT[name]
    ent, rel, rng = O.make_tables(E, R, em * D, rm * D, gamma, D, seed=seed)
    g = np.random.RandomState(seed + 1)
    pos = torch.from_numpy(np.stack([g.randint(E, size=B), g.randint(R, size=B), g.randint(E, size=B)], 1))
    neg = torch.from_numpy(g.randint(E, size=(B, N)))
    w = torch.from_numpy(g.uniform(0.2, 1.0, size=(B, 1))).float()
    # the modulus as the fp32 value the library receives (the oracle runs in fp64 on the same fp32 values)
    return dict(name=name, D=D, E=E, R=R, B=B, N=N, ent=ent, rel=rel, pos=pos, neg=neg, w=w, gamma=gamma, rng=rng,
                mod=float(np.float32(0.5 * rng)))


def replica_loss(name, ent, rel, pos, neg, w, mode, gamma, rng, red="tf", T=1.0, keep=None, pos_keep=None):
    """One replica's train loss (supervisor.py:17-23) with the reduction of the negative branch as a parameter,
    for the row-sharded step's three forward instantiations: red "tf" is O.tf_train_loss at temperature T (the
    softmax weights carry gradient), "detached" is O.upstream_train_loss(adversarial=True, temperature=T),
    "mean" is O.upstream_train_loss(adversarial=False) (tests/test_strided_cpu.py holds it to them).
    keep [B, N] bool / pos_keep [B] bool state include/kge_hip.h's rule for ids without an owner: a dropped
    candidate is left out of the row's softmax, or adds 0 to the mean's sum, which is still divided by N; a
    dropped positive scores 0 and carries no gradient. The ids at dropped places must be valid (any row: its
    score is computed and discarded). Returns (loss, reduced negatives [B], positive scores [B])."""
    s = O.score(name, ent, rel, pos, neg, mode, gamma, rng)
    ps = O.score(name, ent, rel, pos, neg, 3, gamma, rng)[:, 0]
    if keep is None:
        keep = torch.ones_like(s, dtype=torch.bool)
    ls = torch.where(keep, torch.nn.functional.logsigmoid(-s), torch.zeros_like(s))
    if red == "mean":
        n = ls.sum(1) / s.shape[1]
    else:
        p = torch.softmax((T * s).masked_fill(~keep, float("-inf")), 1)
        p = torch.where(keep, p, torch.zeros_like(p))  # (a row with nothing kept reduces to 0)
        n = ((p.detach() if red == "detached" else p) * ls).sum(1)
    if pos_keep is not None:
        ps = torch.where(pos_keep, ps, torch.zeros_like(ps))
    w = w.reshape(-1)
    loss = (-(w * torch.nn.functional.logsigmoid(ps)).sum() / w.sum() - (w * n).sum() / w.sum()) / 2
    return loss, n, ps


# ------------------------------------------------------------------------------------------------
# non-dense views
# ------------------------------------------------------------------------------------------------
def padded(t, pad, device=None, hi=None):
    """A [rows, w] view of a fresh [rows, w + pad] buffer holding t. The padding of a float tensor holds
    NaN. The padding of an id tensor holds VALID ids in [0, hi) that differ from the real ids they sit
    next to (an out-of-range id would score a zero row and could hide a wrong row stride)."""
    rows, w = t.shape
    dev = device if device is not None else t.device
    if t.dtype == torch.int64:
        assert hi is not None and hi > pad + 1
        cols = torch.arange(w, w + pad)
        fill = (t[:, cols % w] + 1 + (cols - w)) % hi  # a shift in [1, pad] < hi: never the real id itself
        buf = torch.cat([t, fill], 1).to(dev)
        assert bool(((buf >= 0) & (buf < hi)).all())
    else:
        buf = torch.full((rows, w + pad), float("nan"), dtype=t.dtype, device=dev)
        buf[:, :w] = t.to(dev)
    v = buf[:, :w]
    assert v.stride() == (w + pad, 1) and v._base is buf
    return v


def offset(t, k, device=None):
    """A dense view of t's values that starts k elements into a 16-B aligned buffer (NaN around it)."""
    dev = device if device is not None else t.device
    n = t.numel()
    buf = torch.full((n + k + 4,), float("nan"), dtype=t.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[k:k + n].view(t.shape)
    v.copy_(t.to(dev))
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + k * t.element_size()
    return v


def canary(rows, w, ld, device, k=0):
    """An fp32 [rows, w] output view with row stride ld (k > 0: starting k floats into its buffer), every
    element of the buffer (the view's own columns too) holding the CANARY bit pattern."""
    assert ld >= w
    buf = torch.full((rows * ld + k + 4,), CANARY, dtype=torch.int32, device=device).view(torch.float32)
    v = buf[k:k + rows * ld].view(rows, ld)[:, :w]
    assert v.stride(0) == ld or rows <= 1
    return v


def outside_bits(v):
    """The int32 bit patterns of every element of v's underlying buffer that is NOT an element of v (row
    padding, what precedes an offset view and what follows it), as a copy: equal before and after a call
    exactly when the call wrote nothing outside the view."""
    base = v._base if v._base is not None else v
    flat = base.reshape(-1).view(torch.int32)
    keep = torch.ones(flat.numel(), dtype=torch.bool, device=v.device)
    start = (v.data_ptr() - base.data_ptr()) // 4
    rows, w = (v.shape[0], v.shape[1]) if v.dim() == 2 else (1, v.numel())
    ld = v.stride(0) if v.dim() == 2 and rows > 1 else w
    idx = (start + torch.arange(rows, device=v.device)[:, None] * ld + torch.arange(w, device=v.device)[None, :])
    keep[idx.reshape(-1)] = False
    return flat[keep].clone()


def like_table(t, fill=None):
    """A buffer laid out exactly like the table view t (same strides, same offset into a buffer of the same
    size) whose surroundings hold the CANARY pattern: gradients and Adam moments share their table's leading
    dimension. fill: the value of the view's own elements (None: the canary too)."""
    base = t._base if t._base is not None else t
    buf = torch.full((base.numel(),), CANARY, dtype=torch.int32, device=t.device).view(torch.float32)
    start = (t.data_ptr() - base.data_ptr()) // 4
    v = buf.as_strided(t.shape, t.stride(), start)
    assert v.data_ptr() % 16 == t.data_ptr() % 16
    if fill is not None:
        v.fill_(fill)
    return v


# ------------------------------------------------------------------------------------------------
# the library's choice of kernel instance, restated
# ------------------------------------------------------------------------------------------------
def expected_vg(D, lds=(), offs=(), ptrs=()):
    """pick_vg (csrc/kge_abi.hip): the widest vector width V in {4, 2, 1} that divides D, every leading
    dimension and rel_off and whose byte size divides every table base address (for the sharded train step
    also qent_pos' and dq's); then the register depth G = pow2ceil(ceil(D / V / 64)). G > 8 is refused by the
    library (KGE_ENOTSUP), G > 4 by the fused train kinds."""
    V = 1
    for v in (4, 2, 1):
        if D % v == 0 and all(x % v == 0 for x in lds) and all(x % v == 0 for x in offs) and \
                all(p % (4 * v) == 0 for p in ptrs):
            V = v
            break
    groups = (D // V + K_WAVE - 1) // K_WAVE
    G = 1
    while G < groups:
        G <<= 1
    return V, G


def table_vg(name, D, ent, rel):
    """expected_vg for (views of) the two tables of an indexed call."""
    return expected_vg(D, lds=(ent.stride(0), rel.stride(0)), offs=(rel_off(name, D),),
                       ptrs=(ent.data_ptr(), rel.data_ptr()))


def tile_fits(name, B, N, D, V, G, waves=None):
    """tile_plan (csrc/kge_abi.hip) at one batch row per block: whether the row-group x XCD-slice tile form
    of the step forward exists for this instance (its LDS plan of query images, id lists and sort counters
    fits 160 KB and the instance is within the fused kernels' register depth)."""
    if G > K_FWD_GRAD_MAX_G or N + 1 > 65536:
        return False
    opb = G * K_WAVE * V * 4
    split = name in ("ComplEx", "RotatE", "InterHT")
    row_bytes = D * 4 * (2 if split else 1)
    waves = waves or (12 if row_bytes >= 4096 else 16)
    nq = 2 if split else 1
    qrow, lrow, fixed = nq * opb + 28, (N + 1) * 4, 256 * 4 + 16
    sort_ints = 0
    if name == "InterHT" and B <= 2048:
        nt = waves * K_WAVE
        sort_ints = (2048 + nt - 1) // nt * waves * 64
    return qrow + fixed + max(lrow, sort_ints * 4) <= 160 * 1024
