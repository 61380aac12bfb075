"""Records tests/golden/abi_matrix.json: what libkge_hip.so's host layer answers without a device call
(size and order queries, the planner's form choices, one case per argument rejection). The calls are defined
here, once; the file holds only the library's answers to them, in this module's order (answers()), at the commit
it was recorded from. tests/test_abi_matrix_cpu.py asks the current build the same and compares, so the file is
recorded from the commit BEFORE a host-layer change, never from the code under test:

    KGE_HIP_LIB=<that commit's libkge_hip.so> python tests/golden/make_abi_matrix.py

Every call here is a pure query, a handle setter/getter, a rejection, or an empty no-op: none may reach a
kernel launch (the pointers are dummies). answers() refuses a KGE_EHIP result for that reason.
"""
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from customknowledgegraphembedding_amd import _lib  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "abi_matrix.json")
P, P2, P3 = 4096, 8192, 12288  # dummy 16-B aligned pointers (never dereferenced)
U4, U1 = 4100, 4097            # 4-B aligned only; unaligned
BIG = 1 << 40
KGE_EHIP = -1000

# ---- (a) the size / order sweep ----------------------------------------------------------------
FNS = range(6)
DS = (4, 33, 64, 255, 500, 1000, 1022, 2048)
BS = (0, 1, 16, 512)
NS = (1, 127, 128, 256, 65536)
ES = (0, 1000, 1 << 28)
NREL = 11


def sweep_queries(fn, D, B, N, E):
    """(symbol, args) of every size query at one grid point: entity rows 2 D wide, relation rows 3 D."""
    ent_ld, rel_ld = 2 * D, 3 * D
    return [
        ("kge_score_bwd_workspace_size", [fn, 1, B, N, D]),
        ("kge_step_backward_workspace_size", [fn, E, B, N, D]),
        ("kge_step_backward_adam_workspace_size", [fn, E, NREL, rel_ld, B, N, D]),
        ("kge_train_step_workspace_size", [fn, E, NREL, rel_ld, B, N, D]),
        ("kge_shard_train_workspace_size", [fn, E, NREL, rel_ld, B, N, D]),
        ("kge_step_plan_size", [fn, E, ent_ld, NREL, rel_ld, 0, B, N, D]),
    ]


SMALL_QUERIES = (
    [("kge_max_dim", [fn]) for fn in (-1, 0, 1, 2, 3, 4, 5, 6, 99)]
    + [("kge_shard_nq", [fn]) for fn in (-1, 0, 1, 2, 3, 4, 5, 6, 99)]
    + [("kge_step_board_size", [])]
    + [("kge_step_forward_order", [E, N]) for E in ES + (40943, (8 << 25) - 1, 8 << 25) for N in NS]
    + [  # invalid and odd arguments of the size queries
        ("kge_step_backward_workspace_size", [9, 10, 2, 4, 8]),
        ("kge_step_backward_workspace_size", [0, -1, 2, 4, 8]),
        ("kge_step_backward_workspace_size", [0, 10, 2, 4, 0]),
        ("kge_step_backward_adam_workspace_size", [0, 10, -1, 8, 2, 4, 8]),
        ("kge_step_backward_adam_workspace_size", [0, 10, 3, -8, 2, 4, 8]),
        ("kge_train_step_workspace_size", [7, 10, 3, 8, 2, 4, 8]),
        ("kge_train_step_workspace_size", [0, 10, 3, 8, -2, 4, 8]),
        ("kge_shard_train_workspace_size", [-1, 10, 3, 8, 2, 4, 8]),
        ("kge_shard_train_workspace_size", [0, 10, 3, 8, 2, -4, 8]),
        ("kge_step_plan_size", [6, 1000, 128, 11, 192, 0, 16, 256, 64]),
        ("kge_step_plan_size", [4, 1 << 31, 128, 11, 192, 0, 16, 256, 64]),
        ("kge_step_plan_size", [4, 1000, 128, 11, 192, 0, 1 << 31, 256, 64]),
        ("kge_step_plan_size", [4, 1000, 130, 11, 192, 0, 16, 256, 64]),   # rows not 16-B aligned: V 2
        ("kge_step_plan_size", [4, 1000, 128, 11, 192, 3, 16, 256, 64]),   # odd relation offset: V 1
    ])


def size_answers(lib):
    """{query: per function, the answers over D x B x N x nentity in product order, or the id of an earlier
    function with the same answers (most sizes depend on the function only through its row widths)}."""
    names = [s for s, _ in sweep_queries(0, 4, 0, 1, 0)]
    per = {s: [[] for _ in FNS] for s in names}
    for fn, D, B, N, E in itertools.product(FNS, DS, BS, NS, ES):
        for s, a in sweep_queries(fn, D, B, N, E):
            per[s][fn].append(int(getattr(lib, s)(*a)))
    for lists in per.values():
        for fn in FNS:
            same = [g for g in range(fn) if lists[g] == lists[fn]]
            if same:
                lists[fn] = same[0]  # (an id never equals a list: `same` holds functions that kept theirs)
    return {"sweep": per, "small": [int(getattr(lib, s)(*a)) for s, a in SMALL_QUERIES]}


# ---- (b) the planner's form choices --------------------------------------------------------------
# B = 1024 gives 64 row groups, more than a board line holds: the throttle is off whatever the device's CU
# count, so the recorded answers do not depend on the machine (kge_step_planner_create asks for that count).
PLANNERS = [
    # fn, nentity, ent_ld, nrelation, rel_ld, rel_off, B, N, D
    [4, 40943, 2000, 11, 3000, 0, 1024, 256, 1000],   # InterHT, 8 KB rows
    [3, 14541, 2000, 237, 1000, 0, 1024, 256, 1000],  # RotatE, 8 KB rows
    [1, 123182, 500, 37, 500, 0, 1024, 1024, 500],    # DistMult, 2 KB rows
]
PLANNER_OPS = (
    [("kge_step_planner_set_form", [w, d]) for w in (0, 8, 12, 16, 4, 24, -1) for d in (0, 1, 2, 3, -1)]
    + [("kge_step_planner_set_lead", [v]) for v in (-2, -1, 0, 1, 12, 255, 256)]
    + [("kge_step_planner_set_board", a) for a in ([P, 1024], [P, 1023], [U1, 1024], [U4, 1024], [None, 0], [P, BIG])]
    + [("kge_step_planner_set_lead", [8])]
    + [("kge_step_planner_set_sweep", [v]) for v in (0, 1, 2, -1)]
    + [("kge_step_planner_set_modulus", [0.5]), ("kge_step_planner_set_clocks", [P, BIG]),
       ("kge_step_planner_plan", [None, P, 256, 1]), ("kge_step_planner_plan", [P, P, 256, 3]),
       ("kge_step_planner_step", [P, P, 256, 1, P, P, P, P])]  # no batch planned: rejected
)


def planner_answers(lib):
    """Per planner: its plan size, then per op [return code, kge_last_error, kge_step_planner_get(-1 .. 5)]."""
    out = []
    for fn, E, ent_ld, R, rel_ld, rel_off, B, N, D in PLANNERS:
        need = int(lib.kge_step_plan_size(fn, E, ent_ld, R, rel_ld, rel_off, B, N, D))
        h = ctypes.c_void_p()
        rc = lib.kge_step_planner_create(ctypes.byref(h), fn, P, E, ent_ld, P, R, rel_ld, rel_off, B, N, D, 24.0, 0.01,
                                         0.0, 1.0, 1, P2, P3, need, None)
        assert rc == 0 and h.value, (rc, lib.kge_last_error())
        steps = []
        for op, args in [("create", None)] + PLANNER_OPS:
            rc = int(getattr(lib, op)(h, *args)) if args is not None else 0
            steps.append([rc, lib.kge_last_error().decode()] + [int(lib.kge_step_planner_get(h, w)) for w in range(-1, 6)])
        assert lib.kge_step_planner_destroy(h) == 0
        out.append([need, steps])
    return out


# ---- (c) one case per rejection ahead of the first device call -------------------------------------
def rejection_cases():
    c = []

    def add(sym, *args):
        c.append([sym, list(args)])

    # kge_score_indexed(_ex): fn, mode, ent, E, ent_ld, rel, R, rel_ld, rel_off, pos, neg, neg_ld, B, N, D, gamma,
    # emb_range, modulus, scores, scores_ld, [forms,] stream
    def si(fn=0, mode=1, ent=P, E=10, ent_ld=4, rel=P, R=2, rel_ld=4, rel_off=0, pos=P, neg=P, neg_ld=4, B=2, N=4,
           D=4, scores=P):
        add("kge_score_indexed", fn, mode, ent, E, ent_ld, rel, R, rel_ld, rel_off, pos, neg, neg_ld, B, N, D, 1.0,
            1.0, 0.0, scores, 4, None)
    si(fn=99), si(fn=-1), si(mode=7), si(mode=2), si(B=-1), si(N=-1), si(D=0), si(B=0), si(N=0), si(mode=3, B=0)
    si(pos=None), si(neg=None), si(mode=3, neg=None, pos=None), si(scores=None), si(ent=None), si(rel=None)
    si(fn=1, ent_ld=4096, rel_ld=4096, D=4096)                  # pick_vg: exceeds (V 4)
    si(fn=1, ent=U4, ent_ld=4096, rel_ld=4096, D=1024)          # pick_vg: exceeds (V 1)
    si(fn=1, ent_ld=1026, rel_ld=1026, D=1026)                  # pick_vg: exceeds (V 2)
    si(mode=1, N=1, B=1 << 34)                                  # run_score: too large for one launch
    add("kge_score_indexed_ex", 0, 1, P, 10, 4, P, 2, 4, 0, None, P, 4, 2, 4, 4, 1.0, 1.0, 0.0, P, 4, None, None)

    def fin(fn=4, ent=P, pos=P, B=2, D=4, ns=P, N=4, out_neg=P, out_pos=P):
        add("kge_step_finish", fn, ent, 10, 8, P, 2, 12, 0, pos, B, D, 1.0, 1.0, 0.0, ns, N, 4, 1.0, 1, out_neg, P,
            out_pos, None)
    fin(fn=9), fin(B=-1), fin(N=0), fin(D=0), fin(B=0), fin(pos=None), fin(ns=None), fin(out_neg=None)
    fin(out_pos=None), fin(ent=None), fin(D=4096)

    def sf(sym="kge_step_forward", fn=4, mode=1, pos=P, neg=P, B=2, N=4, D=4, ns=P, out_neg=P, out_pos=P, extra=()):
        add(sym, fn, mode, P, 10, 8, P, 2, 12, 0, pos, neg, 4, B, N, D, 1.0, 1.0, 0.0, 1.0, 1, ns, 4, out_neg, P,
            out_pos, None, *extra, None)
    sf(fn=9), sf(mode=5), sf(mode=3), sf(B=-1), sf(N=0), sf(D=0), sf(B=0), sf(pos=None), sf(neg=None), sf(ns=None)
    sf(out_neg=None), sf(out_pos=None), sf(D=4096), sf(sym="kge_step_forward_ex", mode=3, extra=(None,))

    def plan(fn=4, mode=1, E=1000, pos=P, neg=P, B=16, N=256, D=64, buf=P):
        add("kge_step_plan", fn, mode, E, 128, 11, 192, 0, pos, neg, N, B, N, D, buf, None)
    plan(fn=9), plan(mode=3), plan(mode=7), plan(B=0), plan(N=0), plan(D=0), plan(pos=None), plan(neg=None)
    plan(buf=None), plan(buf=U4), plan(D=4096), plan(N=65536), plan(E=0), plan(E=1 << 31)

    # kge_step_forward_planned: fn, mode, ent, E, ent_ld, rel, R, rel_ld, rel_off, B, N, D, gamma, emb_range,
    # modulus, temperature, adversarial, plan, next_pos, next_neg, next_neg_ld, next_mode, next_plan, neg_scores,
    # ns_ld, out_neg, pos_scores, out_pos, stream
    def sfp(fn=4, mode=1, ent=P, rel=P, ent_ld=128, B=16, N=256, D=64, plan_=P2, npos=P, nneg=P, nmode=0, nplan=P3,
            ns=P, out_neg=P, out_pos=P):
        add("kge_step_forward_planned", fn, mode, ent, 1000, ent_ld, rel, 11, 192, 0, B, N, D, 1.0, 1.0, 0.0, 1.0, 1,
            plan_, npos, nneg, N, nmode, nplan, ns, N, out_neg, P, out_pos, None)
    sfp(fn=9), sfp(mode=7), sfp(mode=3), sfp(B=0), sfp(N=0), sfp(D=0), sfp(ent=None), sfp(rel=None), sfp(plan_=None)
    sfp(ns=None), sfp(out_neg=None), sfp(out_pos=None), sfp(nmode=3), sfp(npos=None), sfp(nneg=None), sfp(nplan=P2)
    sfp(nplan=U4), sfp(plan_=U4), sfp(plan_=U4, nplan=None), sfp(D=4096)
    sfp(N=65536, nplan=None)

    # kge_step_planner_create: out, fn, ent, E, ent_ld, rel, R, rel_ld, rel_off, B, N, D, gamma, emb_range, modulus,
    # temperature, adversarial, plan0, plan1, plan_bytes, stream  (rejections: *out stays NULL)
    def pc(out="byref", fn=4, ent=P, rel=P, D=64, p0=P2, p1=P3, nbytes=BIG):
        add("kge_step_planner_create", out, fn, ent, 1000, 128, rel, 11, 192, 0, 16, 256, D, 1.0, 1.0, 0.0, 1.0, 1, p0,
            p1, nbytes, None)
    pc(out=None), pc(fn=9), pc(D=4096), pc(ent=None), pc(rel=None), pc(p0=None), pc(p1=None), pc(p1=P2), pc(nbytes=16)
    pc(p0=U4), pc(p1=U4)
    for sym, args in (("kge_step_planner_set_form", [0, 0]), ("kge_step_planner_set_board", [P, 1024]),
                      ("kge_step_planner_set_lead", [0]), ("kge_step_planner_set_modulus", [0.0]),
                      ("kge_step_planner_set_sweep", [1]), ("kge_step_planner_plan", [P, P, 4, 1]),
                      ("kge_step_planner_step", [P, P, 4, 1, P, P, P, P]), ("kge_step_planner_get", [0]),
                      ("kge_step_planner_set_clocks", [P, 1024]), ("kge_step_planner_destroy", [])):
        add(sym, None, *args)

    def ss(fn=1, mode=1, qent=P, shard=P, rows=10, pos=P, neg=P, B=2, N=4, D=4, scores=P):
        add("kge_score_sharded", fn, mode, qent, 4, P, 2, 4, 0, shard, rows, 4, 0, pos, neg, 4, B, N, D, 1.0, 1.0, 0.0,
            scores, 4, None)
    ss(fn=9), ss(mode=9), ss(B=-1), ss(N=-1), ss(D=0), ss(rows=-1), ss(B=0), ss(pos=None), ss(neg=None)
    ss(scores=None), ss(qent=None), ss(shard=None), ss(D=4096), ss(mode=3, neg=None, B=0)

    # kge_shard_score: fn, mode, qent, q_rows, q_ld, q_idx, rel, R, rel_ld, rel_off, shard, rows, shard_ld, shard_lo,
    # pos, B, N, D, gamma, emb_range, modulus, bucket, bucket_start, pre, cnt, tot, world, rank, home_B, home0,
    # send, stream
    def shs(fn=1, mode=1, qent=P, q_rows=8, rows=10, lo=0, pos=P, B=4, N=4, D=4, bucket=P, world=2, rank=0, home_B=2,
            home0=0, send=P):
        add("kge_shard_score", fn, mode, qent, q_rows, 4, P, P, 2, 4, 0, P, rows, 4, lo, pos, B, N, D, 1.0, 1.0, 0.0,
            bucket, P, P, P, P, world, rank, home_B, home0, send, None)
    shs(mode=3), shs(mode=9), shs(fn=9), shs(B=-1), shs(N=-1), shs(D=0), shs(rows=0), shs(q_rows=-1), shs(world=0)
    shs(rank=-1), shs(rank=2), shs(home_B=0), shs(B=3), shs(home0=-1), shs(home0=1), shs(lo=-1), shs(rows=1 << 25)
    shs(B=0), shs(pos=None), shs(send=None), shs(qent=None), shs(bucket=None), shs(D=4096)

    add("kge_gather_rows", P, 10, 4, 0, P, 1, -1, 4, P, 4, None)
    add("kge_gather_rows", P, 10, 4, 0, P, 1, 2, -4, P, 4, None)
    add("kge_gather_rows", P, -1, 4, 0, P, 1, 2, 4, P, 4, None)
    add("kge_gather_rows", P, 10, 4, 0, P, 1, 0, 4, P, 4, None)
    add("kge_gather_rows", None, 10, 4, 0, P, 1, 2, 4, P, 4, None)
    add("kge_gather_rows", P, 10, 4, 0, None, 1, 2, 4, P, 4, None)
    add("kge_gather_rows", P, 10, 4, 0, P, 1, 2, 4, None, 4, None)

    # kge_eval_query(_planes): fn, mode, ent, E, ent_ld, rel, R, rel_ld, pos, B, D, Q | planes, ldq | plane_rows
    def eq(sym="kge_eval_query", fn=1, mode=1, ent=P, pos=P, B=2, D=8, ld=8, Q=P, last=8):
        add(sym, fn, mode, ent, 10, ld, P, 2, ld, pos, B, D, Q, last, None)
    for sym in ("kge_eval_query", "kge_eval_query_planes"):
        eq(sym, fn=9), eq(sym, mode=9), eq(sym, fn=0), eq(sym, fn=4), eq(sym, mode=3), eq(sym, B=-1), eq(sym, D=0)
        eq(sym, B=0), eq(sym, ent=None), eq(sym, pos=None), eq(sym, Q=None), eq(sym, D=4096, ld=4096)
    eq(D=2048, ld=2048, last=2047)                         # ldq odd: V 1, 32 groups: dimension too large
    eq(D=2048, ld=2048, Q=U4, last=2048)                   # Q 4-B aligned only: the same
    eq("kge_eval_query_planes", last=1), eq("kge_eval_query_planes", Q=U4), eq("kge_eval_query_planes", D=6, ld=6)
    eq("kge_eval_query_planes", ent=U4)

    for sym in ("kge_gemm_nt", "kge_gemm_nt_bf16x3"):
        def g(A=P, lda=8, Bm=P, ldb=8, C=P, M=4, N=4, K=8, sym=sym):
            add(sym, A, lda, Bm, ldb, C, 8, M, N, K, None)
        g(M=-1), g(N=-1), g(K=-1), g(M=0), g(N=0), g(A=None), g(Bm=None), g(C=None), g(M=1 << 31), g(N=1 << 31)
        g(K=1 << 31), g(K=6), g(lda=6), g(ldb=6), g(A=U4), g(Bm=U4)
    add("kge_gemm_nt_bf16x3_ex", P, 8, P, 8, P, 8, 4, 4, 6, None, None)

    def sp(X=P, rows=4, cols=8, ld=8, planes=P, prow=4):
        add("kge_split_bf16x3", X, rows, cols, ld, planes, prow, None)
    sp(rows=-1), sp(cols=0), sp(ld=4), sp(prow=2), sp(rows=0, prow=0), sp(X=None), sp(planes=None), sp(planes=U4)
    sp(prow=1 << 26, cols=16, ld=16)                              # 3 * 2^26 * 16 * 2 B = 6 GB of planes

    def gp(sym="kge_gemm_nt_bf16x3_planes", A=P, ar=4, Bp=P, br=4, K=16, C=P, M=4, N=4, extra=()):
        add(sym, A, ar, Bp, br, K, C, 8, M, N, *extra, None)
    gp(M=-1), gp(N=-1), gp(K=0), gp(M=5), gp(N=5), gp(M=0), gp(N=0), gp(A=None), gp(Bp=None), gp(C=None), gp(A=U4)
    gp(Bp=U4), gp(ar=1 << 32, M=1 << 31), gp(ar=1 << 26), gp(br=1 << 26)
    gp(sym="kge_gemm_nt_bf16x3_planes_ex", K=0, extra=(None,))

    add("kge_rank_filtered", P, -1, 4, 4, P, None, None, P, None)
    add("kge_rank_filtered", P, 4, -1, 4, P, None, None, P, None)
    add("kge_rank_filtered", P, 0, 4, 4, P, None, None, P, None)
    add("kge_rank_filtered", None, 4, 4, 4, P, None, None, P, None)
    add("kge_rank_filtered", P, 4, 4, 4, None, None, None, P, None)
    add("kge_rank_filtered", P, 4, 4, 4, P, None, None, None, None)
    add("kge_rank_filtered", P, 4, 4, 4, P, P, None, P, None)
    add("kge_rank_filtered", P, 1 << 31, 4, 4, P, None, None, P, None)

    # kge_eval_rank_planes_phases: A, a_rows, B, b_rows, K, M, N, truth, fptr, fids, nfilter, ranks, ws, ws_bytes,
    # phases, forms, stream
    def rp(A=P, ar=4, Bp=P, br=4, K=16, M=4, N=4, truth=P, fptr=P, fids=P, nf=2, ranks=P, ws=P, wsb=BIG, phases=7):
        add("kge_eval_rank_planes_phases", A, ar, Bp, br, K, M, N, truth, fptr, fids, nf, ranks, ws, wsb, phases, None,
            None)
    rp(phases=0), rp(phases=8), rp(M=-1), rp(N=0), rp(K=0), rp(M=5), rp(N=5), rp(nf=-1), rp(M=0), rp(A=None)
    rp(Bp=None), rp(truth=None), rp(ranks=None), rp(ws=None), rp(fids=None), rp(fptr=None), rp(A=U4), rp(Bp=U4)
    rp(ws=U4), rp(ar=1 << 32, M=1 << 31), rp(ar=1 << 26), rp(br=1 << 26), rp(wsb=8)
    add("kge_eval_rank_planes", P, 4, P, 4, 16, 4, 0, P, P, P, 2, P, P, BIG, None)
    add("kge_eval_rank_planes_ex", P, 4, P, 4, 0, 4, 4, P, P, P, 2, P, P, BIG, None, None)

    # kge_score_dense(_bwd): fn, mode, head, head_ld, rel, rel_ld, rel_off, tail, tail_ld, B, N, D, gamma, emb_range,
    # modulus, ...
    def sd(fn=0, mode=1, head=P, B=2, N=4, D=4, scores=P):
        add("kge_score_dense", fn, mode, head, 4, P, 4, 0, P, 4, B, N, D, 1.0, 1.0, 0.0, scores, 4, None)
    sd(fn=9), sd(mode=9), sd(B=-1), sd(N=-1), sd(D=0), sd(B=0), sd(N=0), sd(scores=None), sd(head=None), sd(D=4096)
    sd(N=1, B=1 << 34)

    def sdb(fn=0, mode=1, B=2, N=4, D=4, ds=P, dh=P, dr=P, dt=P):
        add("kge_score_dense_bwd", fn, mode, P, 4, P, 4, 0, P, 4, B, N, D, 1.0, 1.0, 0.0, ds, 4, dh, dr, dt, None, None)
    sdb(fn=9), sdb(mode=9), sdb(B=-1), sdb(D=0), sdb(N=0), sdb(ds=None), sdb(dh=None), sdb(dr=None), sdb(dt=None)
    sdb(D=4096)

    add("kge_neg_reduce", P, -1, 4, 4, 1.0, 1, P, None)
    add("kge_neg_reduce", P, 2, 0, 4, 1.0, 1, P, None)
    add("kge_neg_reduce", P, 0, 4, 4, 1.0, 1, P, None)
    add("kge_neg_reduce", None, 2, 4, 4, 1.0, 1, P, None)
    add("kge_neg_reduce", P, 2, 4, 4, 1.0, 1, None, None)
    add("kge_neg_reduce_bwd", P, -1, 4, 4, 1.0, 1, 0, P, P, 4, None)
    add("kge_neg_reduce_bwd", P, 2, 0, 4, 1.0, 1, 0, P, P, 4, None)
    add("kge_neg_reduce_bwd", P, 0, 4, 4, 1.0, 1, 0, P, P, 4, None)
    add("kge_neg_reduce_bwd", None, 2, 4, 4, 1.0, 1, 0, P, P, 4, None)
    add("kge_neg_reduce_bwd", P, 2, 4, 4, 1.0, 1, 0, None, P, 4, None)
    add("kge_neg_reduce_bwd", P, 2, 4, 4, 1.0, 1, 0, P, None, 4, None)
    add("kge_log_sigmoid", P, -1, P, None), add("kge_log_sigmoid", P, 0, P, None)
    add("kge_log_sigmoid", None, 4, P, None), add("kge_log_sigmoid", P, 4, None, None)
    add("kge_log_sigmoid_bwd", P, P, -1, P, None), add("kge_log_sigmoid_bwd", P, P, 0, P, None)
    add("kge_log_sigmoid_bwd", None, P, 4, P, None), add("kge_log_sigmoid_bwd", P, None, 4, P, None)
    add("kge_log_sigmoid_bwd", P, P, 4, None, None)
    add("kge_step_loss", P, P, P, 0, P, P, None), add("kge_step_loss", None, P, P, 4, P, P, None)
    add("kge_step_loss", P, None, P, 4, P, P, None), add("kge_step_loss", P, P, None, 4, P, P, None)
    add("kge_step_loss", P, P, P, 4, None, None, None)

    def ad(p=P, g=P, m=P, v=P, n=8, step=1):
        add("kge_adam_update", p, g, m, v, n, 0.001, 0.9, 0.999, 1e-8, step, 0, 0, None)
    ad(n=-1), ad(step=0), ad(n=0), ad(p=None), ad(g=None), ad(m=None), ad(v=None), ad(p=U1), ad(g=U1), ad(m=U1)
    ad(v=U1), ad(n=1 << 45)

    def sib(fn=0, mode=1, pos=P, neg=P, B=2, N=4, D=4, ds=P, de=P, dr=P):
        add("kge_score_indexed_bwd", fn, mode, P, 10, 4, P, 2, 4, 0, pos, neg, 4, B, N, D, 1.0, 1.0, 0.0, ds, 4, de, dr,
            None, None, None)
    sib(fn=9), sib(mode=9), sib(B=-1), sib(N=-1), sib(D=0), sib(B=0), sib(pos=None), sib(neg=None), sib(ds=None)
    sib(de=None), sib(dr=None), sib(D=4096)

    # kge_step_backward: fn, mode, ent, E, ent_ld, rel, R, rel_ld, rel_off, pos, neg, neg_ld, B, N, D, gamma, emb_range,
    # modulus, temperature, adversarial, detach, neg_scores, ns_ld, pos_scores, d_out_neg, d_out_pos, d_ent, d_rel,
    # d_modulus, cand_stats, workspace, workspace_bytes, stream
    def sb(fn=4, mode=1, ent=P, E=10, rel=P, R=2, pos=P, neg=P, B=2, N=4, D=4, ns=P, ps=P, don=P, dop=P, de=P, dr=P,
           ws=P, wsb=BIG):
        add("kge_step_backward", fn, mode, ent, E, 8, rel, R, 12, 0, pos, neg, 4, B, N, D, 1.0, 1.0, 0.0, 1.0, 1, 0, ns,
            4, ps, don, dop, de, dr, None, None, ws, wsb, None)
    sb(fn=9), sb(mode=9), sb(mode=3), sb(B=-1), sb(N=0), sb(D=0), sb(E=-1), sb(R=-1), sb(ent=None), sb(rel=None)
    sb(pos=None), sb(neg=None), sb(ns=None), sb(ps=None), sb(don=None), sb(dop=None), sb(de=None), sb(dr=None)
    sb(B=1 << 20, N=1 << 12), sb(E=1 << 31), sb(ws=None), sb(wsb=16)

    # kge_step_backward_adam: ..., D, gamma, emb_range, modulus_param, modulus, temperature, adversarial, detach,
    # neg_scores, ns_ld, pos_scores, d_out_neg, d_out_pos, m_ent, v_ent, m_rel, v_rel, m_mod, v_mod, lr, b1, b2, eps,
    # step, keras, cand_stats, workspace, workspace_bytes, stream
    def sba(fn=4, mode=1, D=4, B=2, modp=None, me=P, mr=P, vr=P, mm=None, step=1, ws=P, wsb=BIG, de=None):
        add("kge_step_backward_adam", fn, mode, P, 10, 8, P, 2, 12, 0, P, P, 4, B, 4, D, 1.0, 1.0, modp, 0.0, 1.0, 1, 0,
            P, 4, P, P, P, me, P, mr, vr, mm, None, 0.001, 0.9, 0.999, 1e-8, step, 0, None, ws, wsb, None)
    sba(step=0), sba(mr=None), sba(vr=None), sba(fn=5, modp=P), sba(fn=9), sba(D=0), sba(B=-1), sba(ws=None)
    sba(wsb=16), sba(mode=3), sba(me=None)

    # kge_train_step: fn, mode, ent, E, ent_ld, rel, R, rel_ld, rel_off, pos, neg, neg_ld, B, N, D, gamma, emb_range,
    # temperature, adversarial, detach, weight, loss, loss_sum, out_neg, out_pos, m_ent, v_ent, m_rel, v_rel, lr, b1,
    # b2, eps, step, keras, workspace, workspace_bytes, stream
    def ts(fn=4, mode=1, ent=P, E=10, R=2, pos=P, B=2, N=4, D=4, w=P, loss=P, out_neg=P, me=P, vr=P, step=1, ws=P,
           wsb=BIG):
        add("kge_train_step", fn, mode, ent, E, 8, P, R, 12, 0, pos, P, 4, B, N, D, 1.0, 1.0, 1.0, 1, 0, w, loss, None,
            out_neg, P, me, P, P, vr, 0.001, 0.9, 0.999, 1e-8, step, 0, ws, wsb, None)
    ts(fn=9), ts(mode=9), ts(fn=5), ts(mode=3), ts(B=0), ts(N=0), ts(D=0), ts(E=-1), ts(R=-1), ts(step=0)
    ts(ent=None), ts(pos=None), ts(w=None), ts(loss=None), ts(out_neg=None), ts(me=None), ts(vr=None)
    ts(B=1 << 20, N=1 << 12), ts(E=1 << 31), ts(ws=None), ts(wsb=16), ts(D=4096)

    # kge_shard_train_{forward,combine,backward}: fn, mode, shard, rows, ent_ld, shard_lo, qent, qent_pos, q_ld, rel,
    # R, rel_ld, rel_off, pos, neg, neg_ld, Bg, N, D, home_B, world, rank, gamma, emb_range, temperature, adversarial,
    # detach, weight, <call's own>, workspace, workspace_bytes, stream
    tails = {
        "kge_shard_train_forward": lambda x: [x, P],                                    # stats, dq
        "kge_shard_train_combine": lambda x: [x, P, P, P, P],                           # stats_all, dq, outs
        "kge_shard_train_backward": lambda x: [x, P, None, P, P, P, P, 0.001, 0.9, 0.999, 1e-8, 1, 0],
    }

    def sh(sym, fn=4, mode=1, shard=P, rows=10, qent=P, pos=P, Bg=4, N=4, D=4, home_B=2, world=2, rank=0, w=P, own=P,
           ws=P, wsb=BIG, tail=None):
        add(sym, fn, mode, shard, rows, 8, 0, qent, P, 8, P, 2, 12, 0, pos, P, 4, Bg, N, D, home_B, world, rank, 1.0,
            1.0, 1.0, 1, 0, w, *(tail or tails[sym](own)), ws, wsb, None)
    for sym in tails:
        sh(sym, fn=9), sh(sym, own=None), sh(sym, ws=None), sh(sym, wsb=16)
    for kw in (dict(mode=9), dict(fn=5), dict(mode=3), dict(Bg=0), dict(N=0), dict(D=0), dict(rows=-1), dict(world=0),
               dict(rank=-1), dict(rank=2), dict(home_B=0), dict(home_B=3), dict(shard=None), dict(qent=None),
               dict(pos=None), dict(w=None), dict(Bg=1 << 20, home_B=1 << 19, N=1 << 12), dict(rows=1 << 31)):
        sh("kge_shard_train_forward", **kw)  # shard_check: shared by the three calls
    # past shard_check's table-free size, below the call's own
    sh("kge_shard_train_forward", wsb="shard-ws-minus-1"), sh("kge_shard_train_combine", wsb="shard-ws-minus-1")
    sh("kge_shard_train_backward", wsb="shard-ws-minus-1")
    sh("kge_shard_train_backward", tail=[P, P, None, P, P, P, P, 0.001, 0.9, 0.999, 1e-8, 0, 0])   # step 0
    sh("kge_shard_train_backward", tail=[P, None, None, P, P, P, P, 0.001, 0.9, 0.999, 1e-8, 1, 0])  # loss NULL
    # the step's width limit (D / V <= 256; here 8 groups of 4 floats per lane), which all three calls check
    # ahead of their first memset or launch
    sh("kge_shard_train_forward", rows=0, D=2048)
    sh("kge_shard_train_combine", rows=0, D=2048), sh("kge_shard_train_backward", rows=0, D=2048)
    sh("kge_shard_train_forward", D=1028), sh("kge_shard_train_forward", qent=U4, D=260)  # V 4, V 1: 5 groups
    return c


def run_case(lib, sym, args):
    """One recorded call: returns (return value, kge_last_error text or None for the size queries)."""
    a = list(args)
    out = None
    if sym == "kge_step_planner_create" and a[0] == "byref":
        out = ctypes.c_void_p()
        a[0] = ctypes.byref(out)
    if "shard-ws-minus-1" in a:
        # fn, rows, R, rel_ld, Bg, N, D of the call
        a[a.index("shard-ws-minus-1")] = int(lib.kge_shard_train_workspace_size(a[0], a[3], a[10], a[11], a[16], a[17],
                                                                                 a[18])) - 1
    rc = getattr(lib, sym)(*a)
    if out is not None:
        assert not out.value, "a rejected create must leave *out NULL"
    return int(rc), lib.kge_last_error().decode()


def rejection_answers(lib):
    out = []
    for sym, args in rejection_cases():
        rc, msg = run_case(lib, sym, args)
        # a rejection, a -1 of kge_step_planner_get, or an empty no-op: never a device call
        assert rc in (0, -1, -22, -95) and rc != KGE_EHIP, ("reached a device call", sym, args, rc, msg)
        out.append([rc, msg])
    return out


def pack(ans):
    """Message texts stored once: every [rc, text, ...] becomes [rc, index into "messages", ...]."""
    msgs = sorted({r[1] for r in ans["rejections"]} | {s[1] for _, steps in ans["planners"] for s in steps})
    at = {m: i for i, m in enumerate(msgs)}
    return {"sizes": ans["sizes"], "messages": msgs,
            "planners": [[need, [[s[0], at[s[1]]] + s[2:] for s in steps]] for need, steps in ans["planners"]],
            "rejections": [[rc, at[m]] for rc, m in ans["rejections"]]}


def unpack(data):
    msgs = data["messages"]
    return {"sizes": data["sizes"],
            "planners": [[need, [[s[0], msgs[s[1]]] + s[2:] for s in steps]] for need, steps in data["planners"]],
            "rejections": [[rc, msgs[i]] for rc, i in data["rejections"]]}


def answers(lib):
    return {"sizes": size_answers(lib), "planners": planner_answers(lib), "rejections": rejection_answers(lib)}


def main():
    lib = _lib.load()
    data = dict(recorded_from=lib.kge_build_id().decode(), **pack(answers(lib)))
    with open(OUT, "w") as f:
        json.dump(data, f, separators=(",", ":"))
        f.write("\n")
    print(f"{OUT}: {len(data['rejections'])} rejection cases, {len(data['messages'])} messages, "
          f"{os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
