"""Helpers of the DistMult / ComplEx evaluation tests (test_eval_widths_gpu.py, test_eval_cases_cpu.py): plain
restatements, in numpy / torch-CPU, of the contracts include/kge_hip.h gives for kge_split_bf16x3 (split3_ref)
and kge_rank_filtered / kge_eval_rank_planes (rank_ref), written from the header and not from the kernels; the
narrowing kge_eval_query applies for its output matrix on top of tests/strided.py's expected_vg; source and
output layouts built from tests/strided.py's views; and the seeded cases the two files share (tied score rows,
an entity table with bitwise duplicate rows, the end-to-end models). A plain module: nothing here is a fixture
or changes how the suite is collected."""
import functools

import numpy as np
import torch

from oracle import kge_oracle as O
from tests import strided as S

ENOTSUP = -95  # KGE_ENOTSUP (include/kge_hip.h)


# ------------------------------------------------------------------------------------------------
# kge_split_bf16x3
# ------------------------------------------------------------------------------------------------
def kpad(cols):
    return (cols + 15) // 16 * 16


def split3_ref(x):
    """The three bf16 terms of an fp32 matrix x [rows, cols] in kge_split_bf16x3's plane layout, as a bf16 tensor
    [3, kp / 16, rows, 16] (kp = cols rounded up to 16): x0 = bf16(x), x1 = bf16(fl32(x - x0)),
    x2 = bf16(fl32((x - x0) - x1)), round to nearest even (torch's conversion); k past cols is +0."""
    assert x.dtype == torch.float32 and x.dim() == 2
    rows, cols = x.shape
    kp = kpad(cols)
    x0 = x.to(torch.bfloat16)
    r1 = x - x0.float()
    x1 = r1.to(torch.bfloat16)
    x2 = (r1 - x1.float()).to(torch.bfloat16)
    out = torch.zeros(3, rows, kp, dtype=torch.bfloat16)
    for i, t in enumerate((x0, x1, x2)):
        out[i, :, :cols] = t
    return out.view(3, rows, kp // 16, 16).permute(0, 2, 1, 3).contiguous()


def planes_bits(buf, plane_rows, cols):
    """A uint8 plane buffer (kge_split_bf16x3_bytes(plane_rows, cols) bytes) as int16 bit patterns
    [3, kp / 16, plane_rows, 16], on the CPU."""
    kp = kpad(cols)
    n = 3 * plane_rows * kp * 2
    return buf[:n].cpu().view(torch.int16).view(3, kp // 16, plane_rows, 16)


def planes_sum(bits):
    """The fp64 sum of the three terms of planes_bits' tensor, as a matrix [plane_rows, kp] (exact: the terms of an
    fp32 value span 24 bits)."""
    p = bits.view(torch.bfloat16).double().sum(0)  # [kp / 16, rows, 16]
    return p.permute(1, 0, 2).reshape(p.shape[1], -1)


def planes_fp32(bits):
    """The fp32 matrix [plane_rows, kp] whose split planes_bits' tensor holds: planes_sum, rounded (exactly) to
    fp32, a zero taking the sign of its first term (x0 = bf16(x) keeps the sign of a zero; the later terms of a
    zero are +0)."""
    s = planes_sum(bits)
    x = s.float()
    assert torch.equal(x.double(), s)
    p0 = bits[0].view(torch.bfloat16).float().permute(1, 0, 2).reshape(x.shape)
    return torch.where(x == 0, p0, x)


def split_values(rows, cols, seed):
    """fp32 values for the split: magnitudes log-uniform in 2^-60 .. 2^60 with a random sign (no term of the split
    is subnormal, none overflows), about one in twelve replaced by +0 or -0."""
    g = np.random.RandomState(seed)
    x = np.exp2(g.uniform(-60.0, 60.0, size=(rows, cols))) * g.choice([-1.0, 1.0], size=(rows, cols))
    z = g.randint(24, size=(rows, cols))
    x[z == 0] = 0.0
    x[z == 1] = -0.0
    return torch.from_numpy(x.astype(np.float32))


SLACK = 16  # floats of NaN after a source's last row: a whole 16-k chunk, the furthest a row's quads reach


def source(x, ld, off, device):
    """x [rows, cols] as a view with row stride ld that starts `off` floats into a 16-B aligned buffer of NaN, with
    SLACK floats of NaN after the last row: a read past a row's `cols` gives a wrong value, never a fault."""
    rows, cols = x.shape
    assert ld >= cols
    buf = torch.full((off + rows * ld + SLACK,), float("nan"), dtype=torch.float32, device=device)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + rows * ld].view(rows, ld)[:, :cols]
    v.copy_(x.to(device))
    return v


SPLIT_LAYOUTS = ("dense", "ld+1", "ld4+4", "off1")


def split_layout(cols, layout):
    """(ld, off) of a named source layout of kge_split_bf16x3."""
    return {"dense": (cols, 0), "ld+1": (cols + 1, 0), "ld4+4": ((cols + 3) // 4 * 4 + 4, 0), "off1": (cols, 1)}[layout]


# ------------------------------------------------------------------------------------------------
# kge_eval_query
# ------------------------------------------------------------------------------------------------
TABLE_LAYOUTS = (None, "pad4", "pad1", "off1")
Q_LAYOUTS = ("dense", "ld+4", "ld+1", "off1", "ld+2", "off2")  # the last two: beyond the issue's list


def lay_tables(ent, rel, layout, device):
    if layout is None:
        return ent.to(device), rel.to(device)
    if layout.startswith("pad"):
        return S.padded(ent, int(layout[3:]), device), S.padded(rel, int(layout[3:]), device)
    return S.offset(ent, int(layout[3:]), device), S.offset(rel, int(layout[3:]), device)


def q_out(B, K, layout, device):
    """The [B, K] output view of kge_eval_query in a canary buffer (tests/strided.py: canary)."""
    ld, off = {"dense": (K, 0), "ld+4": (K + 4, 0), "ld+1": (K + 1, 0), "off1": (K, 1), "ld+2": (K + 2, 0),
               "off2": (K, 2)}[layout]
    return S.canary(B, K, ld, device, k=off)


def query_vg(D, ent, rel, q):
    """(V, G) kge_eval_query runs for tables ent, rel and the output view q: pick_vg's choice for the tables
    (strided.expected_vg; past K_MAX_G groups the call is refused there), then the narrowing for Q: V = 1 when
    ldq is no multiple of V, halved until Q's base is V floats aligned; G recomputed for the narrower V."""
    V, G = S.expected_vg(D, lds=(ent.stride(0), rel.stride(0)), ptrs=(ent.data_ptr(), rel.data_ptr()))
    if G > S.K_MAX_G:
        return V, G
    if q.stride(0) % V:
        V = 1
    while V > 1 and q.data_ptr() % (4 * V):
        V >>= 1
    G = 1
    while G * S.K_WAVE * V < D:
        G <<= 1
    return V, G


def query_case(name, D, E=30, R=4, B=9, seed=0):
    """Tables, a [B, 3] batch with out-of-range head, relation and tail ids in rows 1 .. 6, and per mode the fp64
    query rows (O.eval_query_dense on tables with a zero row appended, out-of-range ids pointing at it: an
    out-of-range id reads as a zero row), the ComplEx error scale |ab| + |cd| per element, and the rows that are
    zero because an id the mode reads is out of range."""
    em = 2 if name == "ComplEx" else 1
    ent, rel, _ = O.make_tables(E, R, em * D, em * D, 12.0, min(D, 64), seed=seed + D)
    g = np.random.RandomState(seed + 1)
    pos = np.stack([g.randint(E, size=B), g.randint(R, size=B), g.randint(E, size=B)], 1).astype(np.int64)
    pos[1, 0], pos[2, 1], pos[3, 2], pos[4, 0], pos[5, 1], pos[6, 2] = -1, R, E, E, -1, -1
    safe = pos.copy()
    for c, n in ((0, E), (1, R), (2, E)):
        bad = (pos[:, c] < 0) | (pos[:, c] >= n)
        safe[bad, c] = n
    ent0 = torch.cat([ent, torch.zeros(1, ent.shape[1])]).double()
    rel0 = torch.cat([rel, torch.zeros(1, rel.shape[1])]).double()
    ref = {}
    for mode, mname, cols in ((0, "head-batch", (1, 2)), (1, "tail-batch", (0, 1))):
        q = O.eval_query_dense(name, ent0, rel0, torch.from_numpy(safe), mname)
        # the same formula on |tables| with ComplEx' minus turned into a plus: sum of the products' magnitudes
        scale = eval_query_scale(name, ent0, rel0, torch.from_numpy(safe), mname)
        zero = np.zeros(B, dtype=bool)
        for c in cols:
            zero |= safe[:, c] != pos[:, c]
        ref[mode] = (q, scale, torch.from_numpy(zero))
    return dict(name=name, D=D, E=E, R=R, B=B, K=em * D, ent=ent, rel=rel, pos=torch.from_numpy(pos), ref=ref)


def eval_query_scale(name, ent, rel, pos, mode):
    """Per element of O.eval_query_dense's result, the sum of the magnitudes of the products it adds (DistMult: the
    one product)."""
    h, r, t = ent[pos[:, 0]].abs(), rel[pos[:, 1]].abs(), ent[pos[:, 2]].abs()
    a, b = (r, t) if mode == "head-batch" else (h, r)
    if name == "DistMult":
        return a * b
    re_a, im_a = torch.chunk(a, 2, dim=1)
    re_b, im_b = torch.chunk(b, 2, dim=1)
    return torch.cat([re_a * re_b + im_a * im_b, re_a * im_b + im_a * re_b], dim=1)


# ------------------------------------------------------------------------------------------------
# kge_rank_filtered / kge_eval_rank_planes
# ------------------------------------------------------------------------------------------------
def rank_ref(S_, truth, fptr=None, fids=None):
    """include/kge_hip.h's rank, with IEEE comparisons, as int64 [M]:
    ranks[q] = 1 + #{e != truth[q] : S[q, e] > S[q, truth[q]]} - #{f in filter[q], f != truth[q] : S[q, f] > S[q, truth[q]]}.
    A NaN never counts (on either side of the comparison); a truth outside [0, N) scores -inf; filter ids outside
    [0, N) or equal to the truth are ignored. The filter list of a row holds distinct ids."""
    A = S_.detach().cpu().numpy() if isinstance(S_, torch.Tensor) else np.asarray(S_)
    truth = np.asarray(truth, dtype=np.int64)
    M, N = A.shape
    out = np.empty(M, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for q in range(M):
            tr = int(truth[q])
            ok = 0 <= tr < N
            st = A[q, tr] if ok else -np.inf
            above = A[q] > st
            if ok:
                above[tr] = False
            r = 1 + int(above.sum())
            if fptr is not None:
                for f in np.asarray(fids[int(fptr[q]):int(fptr[q + 1])], dtype=np.int64).tolist():
                    if 0 <= f < N and f != tr and A[q, f] > st:
                        r -= 1
            out[q] = r
    return torch.from_numpy(out)


TIE_ROWS = 14


def tied_rank_case(N, seed=0):
    """Score rows [TIE_ROWS, N] quantised to 8 levels (every row ties with its truth many times over) with NaN and
    +-inf entries, and per row a truth and a filter list (CSR, distinct ids), covering: an empty filter, truth -1,
    truth N, a NaN truth score, a +inf and a -inf truth score, a filter holding the truth, a filter holding -1 and
    N, a filter of every entity, and random subsets."""
    g = np.random.RandomState(seed * 7919 + N)
    M = TIE_ROWS
    A = (g.randint(8, size=(M, N)) / 4.0 - 1.0).astype(np.float32)
    for v in (np.nan, np.inf, -np.inf):
        A[g.rand(M, N) < 0.04] = v
    truth = g.randint(N, size=M).astype(np.int64)
    truth[1], truth[2] = -1, N
    A[3, truth[3]] = np.nan
    A[4, truth[4]] = np.inf
    A[5, truth[5]] = -np.inf
    for q in (0, 6, 7, 8):  # finite truths on the rows whose point is the filter
        A[q, truth[q]] = 0.25
    rows = []
    for q in range(M):
        k = g.randint(0, N + 1)
        rows.append(np.sort(g.choice(N, size=k, replace=False)).astype(np.int64))
    rows[0] = np.zeros(0, dtype=np.int64)
    rows[6] = np.union1d(rows[6], [truth[6]]).astype(np.int64)
    rows[7] = np.concatenate([[-1], rows[7], [N]]).astype(np.int64)
    rows[8] = np.arange(N, dtype=np.int64)
    rows[1] = np.arange(N, dtype=np.int64)[::2]  # an out-of-range truth with a filter: the filter still subtracts
    fptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    fids = np.concatenate(rows).astype(np.int64)
    return torch.from_numpy(A), torch.from_numpy(truth), torch.from_numpy(fptr), torch.from_numpy(fids)


RANK_LAYOUTS = ("dense", "ld+1", "ld+3off1", "ld+3off2", "ld+3off3")


def rank_layout(N, layout):
    return {"dense": (N, 0), "ld+1": (N + 1, 0), "ld+3off1": (N + 3, 1), "ld+3off2": (N + 3, 2),
            "ld+3off3": (N + 3, 3)}[layout]


def score_rows(A, ld, off, device):
    """A [M, N] as a view with row stride ld, `off` floats into a 16-B aligned buffer whose other elements hold
    +inf: a padding element read as a score would count above every finite truth."""
    M, N = A.shape
    buf = torch.full((off + M * ld + 4,), float("inf"), dtype=torch.float32, device=device)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + M * ld].view(M, ld)[:, :N]
    v.copy_(A.to(device))
    return v


def duplicate_table(name, d, E=300, R=5, B=37, seed=0):
    """An entity table in which each of 40 rows stands at four scattered ids (their scores against any query are
    bitwise equal: the same operands through the same arithmetic) and id E - 3 is all +inf (its bf16 terms are
    inf, NaN, NaN: a NaN score); queries whose truths are among the duplicated ids; per mode a filter (CSR, distinct
    ids) holding, row by row, duplicates of the truth, the truth itself, -1 and E, the +inf row, and random ids;
    truth -1 and truth E on two rows."""
    em = 2 if name == "ComplEx" else 1
    ent, rel, _ = O.make_tables(E, R, em * d, em * d, 12.0, d, seed=seed + d)
    g = np.random.RandomState(seed + 3)
    ids = g.permutation(E - 3)[:160].reshape(40, 4)  # row j's four ids
    for j in range(40):
        ent[torch.from_numpy(ids[j, 1:])] = ent[int(ids[j, 0])].clone()
    ent[E - 3] = float("inf")
    pos = np.stack([g.randint(E - 3, size=B), g.randint(R, size=B), g.randint(E - 3, size=B)], 1).astype(np.int64)
    grp = g.randint(40, size=B)
    pos[:, 0] = ids[grp, g.randint(4, size=B)]
    pos[:, 2] = ids[grp[::-1], g.randint(4, size=B)]
    filt = {}
    for mode, col in ((0, 0), (1, 2)):
        truth = pos[:, col].copy()
        rows = []
        for q in range(B):
            j = int(np.nonzero(ids == truth[q])[0][0])
            extra = g.choice(E, size=g.randint(0, 12), replace=False)
            parts = [extra]
            if q % 3 != 2:
                parts.append(ids[j][ids[j] != truth[q]][:1 + q % 3])  # one to three duplicates of the truth
            if q % 4 == 0:
                parts.append([truth[q]])
            if q % 5 == 0:
                parts.append([-1, E])
            if q % 7 == 0:
                parts.append([E - 3])
            rows.append(np.unique(np.concatenate([np.asarray(p, dtype=np.int64) for p in parts])))
        rows[2] = np.zeros(0, dtype=np.int64)
        truth[9], truth[11] = -1, E
        fptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        filt[mode] = (torch.from_numpy(truth), torch.from_numpy(fptr), torch.from_numpy(np.concatenate(rows)))
    return dict(name=name, D=d, K=em * d, E=E, R=R, B=B, ent=ent, rel=rel, pos=torch.from_numpy(pos), filt=filt,
                dup_ids=ids)


# ------------------------------------------------------------------------------------------------
# end to end: evaluate.score_all / rank_planes / test_step / predict
# ------------------------------------------------------------------------------------------------
E2E_E, E2E_R, E2E_TRUE, E2E_TEST, E2E_GAMMA = 400, 5, 1500, 60, 9.0
# (score function, hidden_dim, seed): the issue's four, and DistMult d = 8, whose float4 rows meet a padded stride
E2E_MODELS = (("DistMult", 50, 11), ("DistMult", 6, 12), ("ComplEx", 25, 13), ("ComplEx", 50, 14), ("DistMult", 8, 15))
E2E_MAX_UNDECIDED = 0.05  # share of queries whose fp64 rank the bounds of rtol = 1e-6 leave open


@functools.lru_cache(maxsize=None)
def e2e_case(name, d, seed):
    """The tables KGEModel(name, E2E_E, E2E_R, d, E2E_GAMMA, seed=seed) draws (O.make_tables: the same generator
    sequence), E2E_TRUE true triples with two hub pairs (long filter lists), the first E2E_TEST as the test
    triples, and per mode O.eval_ranks_dense's (ranks, lo, hi) at rtol = 1e-6 on the fp64 tables."""
    em = 2 if name == "ComplEx" else 1
    ent, rel, _ = O.make_tables(E2E_E, E2E_R, em * d, em * d, E2E_GAMMA, d, seed=seed)
    g = np.random.RandomState(seed)
    true = np.stack([g.randint(E2E_E, size=E2E_TRUE), g.randint(E2E_R, size=E2E_TRUE),
                     g.randint(E2E_E, size=E2E_TRUE)], 1).astype(np.int64)
    true[100:300, 0] = true[0, 0]
    true[100:300, 1] = true[0, 1]
    true[300:500, 2] = true[1, 2]
    true[300:500, 1] = true[1, 1]
    test = true[:E2E_TEST]
    ref = {mode: O.eval_ranks_dense(name, ent.double(), rel.double(), torch.from_numpy(test), mode,
                                    [tuple(x) for x in true.tolist()], rtol=1e-6)
           for mode in ("head-batch", "tail-batch")}
    return dict(name=name, d=d, seed=seed, ent=ent, rel=rel, true=true, test=test, ref=ref)


def undecided_share(case):
    """The share of a case's 2 x E2E_TEST queries with lo != hi."""
    n = sum(int((lo != hi).sum()) for _, lo, hi in case["ref"].values())
    return n / (2.0 * len(case["test"]))
