"""The launcher reports "nothing launched" (KGE_ENOTSUP, "no kernel for this (function, width) combination")
for a (kind, function, side, V, G) without an instantiation. This test is the other half: for supported
combinations that report never fires. One small shape per entry point, each call returns 0 and overwrites
every element of its canary-filled outputs, so a launch the dispatch table skipped would show as either.

What the kernels compute is the other GPU tests' business (they compare every entry point at every (V, G)
bitwise or against the oracle); here only "it ran and wrote its whole output"."""
import ctypes

import pytest
import torch

from customknowledgegraphembedding_amd import _lib as L
from customknowledgegraphembedding_amd._lib import FN_IDS
from tests import strided as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
E, R, B, N = 512, 7, 8, 128


def _canary(*shape):
    return torch.full(shape, S.CANARY, dtype=torch.int32, device=DEV).view(torch.float32)


def _overwritten(**outs):
    torch.cuda.synchronize()
    for what, t in outs.items():
        left = int((t.view(torch.int32) == S.CANARY).sum())
        assert left == 0, f"{what}: {left} of {t.numel()} elements not written"


def _st():
    return torch.cuda.current_stream().cuda_stream


def _tables(name, D, v1=False):
    """(case, ent, rel) on the device; v1: one float of row padding, so every kernel takes its V = 1 instance."""
    c = S.make_case(name, D, E, R, B, N, seed=D)
    ent, rel = (S.padded(t, 1, DEV) for t in (c["ent"], c["rel"])) if v1 else (c["ent"].to(DEV), c["rel"].to(DEV))
    return c, ent, rel


def _step_forward(lib, c, ent, rel, mode, order=None, stats=None):
    name, D = c["name"], c["D"]
    pos, neg = c["pos"].to(DEV), c["neg"].to(DEV)
    ns, out_neg, ps, out_pos = _canary(B, N), _canary(B), _canary(B), _canary(B)
    forms = L.forms(step_order=order) if order is not None else None
    rc = lib.kge_step_forward_ex(
        FN_IDS[name], mode, ent.data_ptr(), E, ent.stride(0), rel.data_ptr(), R, rel.stride(0), S.rel_off(name, D),
        pos.data_ptr(), neg.data_ptr(), neg.stride(0), B, N, D, c["gamma"], c["rng"], c["mod"], 1.0, 1, ns.data_ptr(),
        N, out_neg.data_ptr(), ps.data_ptr(), out_pos.data_ptr(), None if stats is None else stats.data_ptr(),
        None if forms is None else ctypes.addressof(forms), _st())
    assert rc == 0, (name, D, mode, order, lib.kge_last_error())
    _overwritten(neg_scores=ns, out_neg=out_neg, pos_scores=ps, out_pos=out_pos)
    return ns, ps, out_neg, out_pos


def test_every_supported_dispatch_launches_and_writes_its_outputs():
    lib = L.load()
    # kge_step_forward in its three candidate orders: D = 64 (V 4, G 1) and D = 33 (V 1, G 1), both sides
    for D in (64, 33):
        c, ent, rel = _tables("RotatE", D)
        assert S.table_vg("RotatE", D, ent, rel) == ((4, 1) if D == 64 else (1, 1))
        for order in ("row", "xcd", "tile"):
            for mode in (0, 1):
                _step_forward(lib, c, ent, rel, mode, order)

    # kge_step_backward: D = 256 at V = 1 is G = 4, the streaming phases 1 and 2; D = 33 the register-resident ones
    for D in (256, 33):
        c, ent, rel = _tables("TransE", D, v1=True)
        assert S.table_vg("TransE", D, ent, rel) == ((1, 4) if D == 256 else (1, 1))
        pos, neg = c["pos"].to(DEV), c["neg"].to(DEV)
        for mode in (0, 1):
            ns, ps, _, _ = _step_forward(lib, c, ent, rel, mode)
            d_out = torch.full((B,), -0.5 / B, device=DEV)
            d_ent, d_rel = _canary(E, ent.stride(0))[:, :D], _canary(R, rel.stride(0))[:, :D]
            ws = torch.empty(lib.kge_step_backward_workspace_size(0, E, B, N, D), dtype=torch.uint8, device=DEV)
            rc = lib.kge_step_backward(
                0, mode, ent.data_ptr(), E, ent.stride(0), rel.data_ptr(), R, rel.stride(0), 0, pos.data_ptr(),
                neg.data_ptr(), neg.stride(0), B, N, D, c["gamma"], c["rng"], 0.0, 1.0, 1, 0, ns.data_ptr(), N,
                ps.data_ptr(), d_out.data_ptr(), d_out.data_ptr(), d_ent.data_ptr(), d_rel.data_ptr(), None, None,
                ws.data_ptr(), ws.numel(), _st())
            assert rc == 0, (D, mode, lib.kge_last_error())
            _overwritten(d_ent=d_ent, d_rel=d_rel)

    # kge_train_step at D = 64: the fused forward + query gradient, the epilogue, phase 2 with Adam
    c, ent, rel = _tables("ComplEx", 64)
    pos, neg, w = c["pos"].to(DEV), c["neg"].to(DEV), c["w"].reshape(-1).to(DEV)
    for mode in (0, 1):
        mv = [torch.zeros_like(t) for t in (ent, ent, rel, rel)]
        loss, out_neg, out_pos = _canary(1), _canary(B), _canary(B)
        ws = torch.empty(lib.kge_train_step_workspace_size(2, E, R, rel.stride(0), B, N, 64), dtype=torch.uint8,
                         device=DEV)
        rc = lib.kge_train_step(
            2, mode, ent.data_ptr(), E, ent.stride(0), rel.data_ptr(), R, rel.stride(0), 0, pos.data_ptr(),
            neg.data_ptr(), neg.stride(0), B, N, 64, c["gamma"], c["rng"], 1.0, 1, 0, w.data_ptr(), loss.data_ptr(),
            None, out_neg.data_ptr(), out_pos.data_ptr(), mv[0].data_ptr(), mv[1].data_ptr(), mv[2].data_ptr(),
            mv[3].data_ptr(), 1e-3, 0.9, 0.999, 1e-7, 1, 1, ws.data_ptr(), ws.numel(), _st())
        assert rc == 0, (mode, lib.kge_last_error())
        _overwritten(loss=loss, out_neg=out_neg, out_pos=out_pos)
        assert bool(torch.isfinite(loss).all()) and all(bool(m.any()) for m in mv)  # every moment table was updated

    # InterHT with cand_stats: the one-launch forward that keeps the candidate norms (KIND_STEP_FWD_STATS). The
    # other statistics kind, KIND_FWD_STATS, has no caller in the library, so no entry point reaches it.
    c, ent, rel = _tables("InterHT", 64)
    for mode in (0, 1):
        stats = _canary(B * N, 2)
        _step_forward(lib, c, ent, rel, mode, stats=stats)
        _overwritten(cand_stats=stats)
