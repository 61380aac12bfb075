"""Helpers of the TranSparse tests (test_transparse_gpu.py, test_transparse_shapes_gpu.py,
test_transparse_cases_cpu.py): seeded tables and batches, the fp64 oracle, a Python restatement of the host
dispatch of csrc/kge_transparse.hip (which kernel, how many tiles, chunks, splits and bucket passes a shape
gets), and the named shapes that test_transparse_shapes_gpu.py runs, each with the branch it is there to reach.
A plain module: nothing here is a fixture or changes how the suite is collected."""
import functools

import numpy as np
import torch

from oracle import kge_oracle as O

GAMMA = 12.0


# ------------------------------------------------------------------------------------------------
# seeded inputs and the oracle
# ------------------------------------------------------------------------------------------------
def _tables(E, R, d, seed=0, gamma=12.0):
    g = torch.Generator().manual_seed(seed)
    rng = (gamma + 2.0) / d
    ent = torch.empty(E, d).uniform_(-rng, rng, generator=g)
    rel = torch.empty(R, d).uniform_(-rng, rng, generator=g)
    W = torch.empty(R, d, d).uniform_(-rng, rng, generator=g)
    mask = (torch.empty(R, d, d).uniform_(1, 100, generator=g) >= 50).float()
    return ent, rel, W, mask


def _batch(E, R, B, N, seed=1):
    g = np.random.RandomState(seed)
    pos = np.stack([g.randint(E, size=B), g.randint(R, size=B), g.randint(E, size=B)], 1).astype(np.int64)
    neg = g.randint(E, size=(B, N)).astype(np.int64)
    return torch.from_numpy(pos), torch.from_numpy(neg)


def _oracle(ent, rel, W, mask, pos, neg, mode, gamma, grad=None):
    t = [x.double().requires_grad_(True) for x in (ent, rel, W)]
    s = O.transparse_score(t[0], t[1], t[2], mask.double(), pos, neg, mode, gamma)
    if grad is None:
        return s.detach().numpy(), None
    (s * grad.double()).sum().backward()
    return s.detach().numpy(), [x.grad.numpy() for x in t]


def oracle_by_relation(ent, rel, W, mask, pos, neg, mode, gamma, grad=None):
    """_oracle without its [B, d, d] copies: O.transparse_score gathers W[pos[:, 1]] and mask[pos[:, 1]] per
    batch row (5 GB in fp64 at B 70, d 3076), so here the batch rows of one relation go through the same
    O.gather_rows and O.transparse with that relation's one matrix, broadcast. The same arithmetic per row;
    test_transparse_cases_cpu.py holds the two to 1e-12 of each other, scores and gradients. Single and
    tail-batch scores never read the candidates (Q9), so only neg's first column is gathered there."""
    want = grad is not None
    t = [x.double().requires_grad_(want) for x in (ent, rel, W)]
    if mode != 0:
        neg = neg[:, :1] if neg is not None else pos[:, 2:3]
    head, relation, _ = O.gather_rows(t[0], t[1], pos, neg, mode)
    parts, rows = [], []
    for r in torch.unique(pos[:, 1]).tolist():
        idx = (pos[:, 1] == r).nonzero()[:, 0]
        parts.append(O.transparse(head[idx], relation[idx], None, mode, gamma, t[2][r], mask[r].double()))
        rows.append(idx)
    s = torch.cat(parts)[torch.argsort(torch.cat(rows))]
    if not want:
        return s.detach().numpy(), None
    (s * grad.double()).sum().backward()
    return s.detach().numpy(), [x.grad.numpy() for x in t]


K_DIRECT_MAX = 1 << 23  # B * d * d elements up to which the oracle is O.transparse_score itself


def oracle(ent, rel, W, mask, pos, neg, mode, gamma, grad=None):
    """The fp64 reference of a case: O.transparse_score on the whole batch (_oracle) while its per-row matrix
    copies stay small, oracle_by_relation beyond."""
    fn = _oracle if pos.shape[0] * ent.shape[1] ** 2 <= K_DIRECT_MAX else oracle_by_relation
    return fn(ent, rel, W, mask, pos, neg, mode, gamma, grad)


# ------------------------------------------------------------------------------------------------
# the host dispatch of csrc/kge_transparse.hip, restated
# ------------------------------------------------------------------------------------------------
TBM = 128                      # rows and columns of a ts_rows_kernel / ts_dw_kernel tile
XBR, XBC = 256, 256            # rows and columns of the 512-thread head-batch kernels
K_SCAN_TILE = 1024             # kge_scan.h
K_WAVE = 64
K_DENT_COLS = 256              # columns per wave of ts_dent_kernel
K_TS_SORT_MAX_REL = 1023
K_TS_SORT_MAX_B = 8192
K_TS_BIG_MAX_DIM = 3072
K_XS_MAX_DIM = 1024
K_XS_OOB = 0xFFFFFFF0
K_XG_SPLIT_COLS, K_XG_K_CHUNKS = 128, 8
K_PLANES_MIN_ROWS_PER_REL = 16
K_PLANES_MAX_BYTES = 256 << 20


def cdiv(a, b):
    return (a + b - 1) // b


def pick_splits(R, T):
    """pick_splits: how many parts a relation's rows are cut into so that dW has about 1024 blocks."""
    base = (R + 1) * T * T
    return min(16, max(1, cdiv(1024, base)))


def score_workspace_bytes(mode, R, B, d):
    """kge_transparse_score_workspace_size."""
    if B <= 0 or d <= 0 or d > K_XS_MAX_DIM:
        return 0
    if mode == 0:
        cols, nk = cdiv(d, XBC) * XBC, cdiv(d, 16)
        planes = R * 3 * nk * cols * 16 * 2
        return planes if (R + 1) * K_PLANES_MIN_ROWS_PER_REL <= B and planes <= K_PLANES_MAX_BYTES else 0
    xs, ks = cdiv(d, K_XG_SPLIT_COLS), cdiv(cdiv(d, 16), K_XG_K_CHUNKS)
    return ks * B * xs * K_XG_SPLIT_COLS * 4 if xs * ks > 1 else 0


def dispatch(E, R, d, B, N, mode, ent_ld=None, ent_ptr=0, form=0, split=True):
    """What kge_transparse_score(_ex) and kge_transparse_score_bwd do with a shape. ent_ld: the entity
    table's row stride in floats (None: d); ent_ptr: its base address (or that modulo 16); W, mask and M
    come from the allocator and are 16-B aligned. form, split: transparse_score_raw's `forms` and `split`.
      splits       pick_splits (S of ts_dw_kernel)
      T            128-wide tiles per side of dW
      dent_chunks  256-column chunks per entity of ts_dent_kernel
      scan_tiles_E, scan_tiles_R   1024-tiles of launch_exclusive_scan over E and over R + 1
      use_v4       float4 rows (else the scalar instances)
      order        head-batch forward: 'sorted' (relation-sorted ranks) or 'natural'; 'grouped' otherwise
      passes       64-bucket passes of ts_sorted_row(_nt) to reach the last bucket (0 when not sorted)
      fwd          'rows_v1' ts_rows_kernel<FWD, 1>, 'rows_x3' ts_rows_kernel<FWD, 4, true>, 'x3'
                   ts_fwd_x3_kernel, 'x3s' / 'x3s_planes' ts_fwd_x3s_kernel, 'x3g' / 'x3g_split'
                   ts_fwd_x3g_kernel
      nblk         blocks of the head-batch forward (the XCD rank map's B * nchunk)"""
    ent_ld = d if ent_ld is None else ent_ld
    grouped = mode != 0
    Nk = 1 if grouped else N
    T = cdiv(d, TBM)
    use_v4 = d % 4 == 0 and ent_ld % 4 == 0 and ent_ptr % 16 == 0
    xs_ok = form in (0, 2) and d <= K_XS_MAX_DIM and E * ent_ld * 4 < K_XS_OOB and d * d * 4 < K_XS_OOB
    ws = score_workspace_bytes(mode, R, B, d) if split else 0
    nchunk = max(1, cdiv(B if grouped else Nk, TBM))
    if not use_v4:
        fwd = "rows_v1"
    elif grouped and xs_ok:
        fwd = "x3g_split" if ws else "x3g"
    elif not grouped and Nk > TBM and d <= K_TS_BIG_MAX_DIM:
        fwd = ("x3s_planes" if ws else "x3s") if xs_ok else "x3"
        nchunk = cdiv(Nk, XBR)
    else:
        fwd = "rows_x3"
    if grouped:
        order = "grouped"
    else:
        order = "sorted" if R <= K_TS_SORT_MAX_REL and B <= K_TS_SORT_MAX_B else "natural"
    return dict(splits=pick_splits(R, T), T=T, dent_chunks=cdiv(d, K_DENT_COLS),
                scan_tiles_E=cdiv(E, K_SCAN_TILE), scan_tiles_R=cdiv(R + 1, K_SCAN_TILE), use_v4=use_v4,
                order=order, passes=cdiv(R + 1, K_WAVE) if order == "sorted" else 0, fwd=fwd,
                nblk=None if grouped else B * nchunk)


def want_premul(R, B, N, mode):
    """ops._want_premul for allocator-aligned W with d % 4 == 0."""
    return R * 4 <= max(1, B * (N if mode == 0 else 1) // 128)


def view_layout(v):
    """(row stride, base address modulo 16) of a table view, as dispatch takes them."""
    return v.stride(0), v.data_ptr() % 16


# ------------------------------------------------------------------------------------------------
# the named cases
# ------------------------------------------------------------------------------------------------
def _case(name, kind, E, R, d, B, N, modes, why, want=None, **extra):
    """B is {mode: B} or one B for every mode. want: {mode or None (every mode): {dispatch key: value}}."""
    Bs = B if isinstance(B, dict) else {m: B for m in modes}
    return dict(name=name, kind=kind, E=E, R=R, d=d, B=Bs, N=N, modes=tuple(modes), why=why, want=want or {},
                **extra)


M013 = (0, 1, 3)
BWD_CASES = (
    # launch_exclusive_scan over the entity counts: one full tile, a second tile of one element, three tiles
    [_case(f"scan_E{E}", "scan", E, 3, 8, 40, 130, M013, "scan tiles over E", {None: dict(scan_tiles_E=t)})
     for E, t in ((1024, 1), (1025, 2), (2500, 3))]
    # the relation CSR's scan (R + 1 counts) and the forward's bucket search that makes `stats`; at R 1024 the
    # second scan tile holds only the empty bucket of out-of-range relations, at R 1025 also relation 1024's rows
    + [_case(f"rel_R{R}", "rel", 300, R, 8, 300, 3, M013, "relation buckets and the scan over R + 1",
             {None: dict(scan_tiles_R=t, splits=s), 0: dict(order=o, passes=p)})
       for R, t, s, o, p in ((64, 1, 16, "sorted", 2), (65, 1, 16, "sorted", 2), (1023, 1, 1, "sorted", 16),
                             (1024, 2, 1, "natural", 0), (1025, 2, 1, "natural", 0))]
    + [_case("split_S1", "split", 400, 255, 130, 300, 1, M013, "ts_dw_kernel adds to d_W itself",
             {None: dict(splits=1, T=2)}),
       _case("split_S2", "split", 400, 63, 260, 70, 5, M013, "two splits, 4-column last tile and dent chunk",
             {None: dict(splits=2, T=3, dent_chunks=2)}),
       _case("split_S11", "split", 1100, 5, 500, 6, 130, M013, "K splits unevenly over 11 parts",
             {None: dict(splits=11, T=4, dent_chunks=2)})]
    + [_case(f"width_d{d}", "width", 1100, 2, d, {0: 5, 1: 150, 3: 150}, 130, M013,
             "ts_dent chunks, the second trip of the j loops", {None: dict(dent_chunks=c, use_v4=v)})
       for d, c, v in ((257, 2, False), (260, 2, True), (500, 2, True), (516, 3, True), (1000, 4, True),
                       (1028, 5, True))]
    + [_case("hot", "hot", 1100, 3, 260, {0: 4, 1: 300, 3: 300}, 300, M013, "an entity bucket above 64 rows",
             {None: dict(dent_chunks=2)}, bucket={0: 800, 1: 150, 3: 150})]
)
WORKLOAD = _case("workload", "workload", 3000, 11, 500, 24, 256, (0,), "the c6 workload, reduced: with M",
                 {0: dict(fwd="x3s", splits=6, dent_chunks=2, scan_tiles_E=3)})
ACCUM = _case("accum", "accum", 2000, 5, 130, {0: 6, 1: 40, 3: 40}, 140, M013,
              "gradients accumulate; absent rows stay bit for bit", {None: dict(dent_chunks=1)})
LAYOUT_DIMS = (64, 130, 260)
LAYOUT_VARIANTS = ("ent_pad4", "ent_pad1", "ent_off1", "rel_pad4", "rel_pad1", "neg_pad", "dscores_pad",
                   "out_pad", "all_v4", "all_v1")


def layout_case(d):
    return _case(f"layout_d{d}", "layout", 200, 3, d, {0: 6, 1: 140}, 140, (0, 1), "strides and alignment")


FWD_CASES = (
    [_case(f"pass_R{R}_N{N}", "pass", 300, R, 8, 300, N, M013, "bucket passes of the sorted-row search",
           {0: dict(order=o, passes=p, fwd=f)})
     for R, o, p in ((63, "sorted", 1), (64, "sorted", 2), (65, "sorted", 2), (237, "sorted", 4),
                     (1023, "sorted", 16), (1024, "natural", 0))
     for N, f in ((5, "rows_x3"), (130, "x3s"))]
    + [_case("pass_B8192", "pass", 300, 3, 8, 8192, 2, (0,), "the last sorted B", {0: dict(order="sorted")}),
       _case("pass_B8193", "pass", 300, 3, 8, 8193, 2, (0,), "natural order past kTsSortMaxB",
             {0: dict(order="natural", fwd="rows_x3")})]
    + [_case(f"pass_scalar_N{N}", "pass", 300, 65, 50, 300, N, M013, "two passes in the scalar kernel",
             {0: dict(passes=2, fwd="rows_v1", nblk=b)}) for N, b in ((5, 300), (130, 600))]
    + [_case(f"pass_few_N{N}", "pass", 300, 65, 8, 5, N, (0,), "fewer blocks than XCDs",
             {0: dict(passes=2, fwd=f, nblk=5)}) for N, f in ((5, "rows_x3"), (130, "x3s"))]
    + [_case(f"wide_d{d}_N{N}", "wide", 1100, 2, d, {0: 3, 1: 70, 3: 70}, N, M013 if N == 130 else (0,),
             "default routes past kXsMaxDim and kTsBigMaxDim", {0: dict(fwd=f), 1: dict(fwd="rows_x3"),
                                                                3: dict(fwd="rows_x3")})
       for d, N, f in ((1028, 100, "rows_x3"), (1028, 130, "x3"), (3072, 100, "rows_x3"), (3072, 130, "x3"),
                       (3076, 100, "rows_x3"), (3076, 130, "rows_x3"))]
)
STEP = _case("step_R237", "step", 300, 237, 260, 70, 256, (0, 1), "the fused step at FB15k-237's relations",
             {0: dict(fwd="x3s", passes=4), 1: dict(fwd="x3g_split")})

ALL_CASES = BWD_CASES + [WORKLOAD, ACCUM] + FWD_CASES + [STEP] + [layout_case(d) for d in LAYOUT_DIMS]


def case_dispatch(c, mode, **kw):
    return dispatch(c["E"], c["R"], c["d"], c["B"][mode], c["N"], mode, **kw)


def ids(cases):
    return [(c, m) for c in cases for m in c["modes"]]


def case_id(cm):
    return f"{cm[0]['name']}-m{cm[1]}"


@functools.lru_cache(maxsize=2)
def tables(E, R, d, seed):
    return _tables(E, R, d, seed=seed)


def inputs(c, mode, seed=30):
    """CPU fp32 tables, pos [B, 3], neg [B, N] and the upstream gradient [B, N] ([B, 1] grouped) of a case,
    with the ids its branch needs forced in. Every id is inside its table."""
    E, R, d, B, N = c["E"], c["R"], c["d"], c["B"][mode], c["N"]
    ent, rel, W, mask = tables(E, R, d, seed)
    pos, neg = _batch(E, R, B, N, seed=seed + 1 + mode)
    kind = c["kind"]
    if kind == "scan":  # both sides of every tile edge carry gradient, from the candidates and from the heads
        edge = torch.tensor([i for i in (0, 1023, 1024, E - 1) if i < E])
        neg[0, :len(edge)] = edge
        pos[:len(edge), 0] = edge
    elif kind in ("rel", "pass"):  # the first and last bucket of each 64-bucket pass
        edge = torch.tensor(sorted({i for i in (0, 63, 64, R - 1) if i < R}))[:B]
        pos[B - len(edge):, 1] = edge
    elif kind == "split":  # relation R - 1 has exactly one batch row
        pos[:, 1][pos[:, 1] == R - 1] = 0
        pos[B // 2, 1] = R - 1
    elif kind == "hot":
        if mode == 0:
            neg[:, 50:250] = 7
        else:
            pos[::2, 0] = 7
    elif kind == "accum":  # relations 2 and 4 stay out of the batch
        pos[:, 1] = torch.tensor([0, 1, 3])[torch.arange(B) % 3]
    g = np.random.RandomState(seed + 7)
    grad = torch.from_numpy(g.randn(B, N if mode == 0 else 1).astype(np.float32))
    assert bool(((pos[:, [0, 2]] >= 0) & (pos[:, [0, 2]] < E)).all()) and bool(((neg >= 0) & (neg < E)).all())
    assert bool(((pos[:, 1] >= 0) & (pos[:, 1] < R)).all())
    return ent, rel, W, mask, pos, neg, grad


def entity_rows(pos, neg, mode):
    """The entity id of every gradient row: the candidates (head-batch) or the heads."""
    return neg.reshape(-1) if mode == 0 else pos[:, 0]
