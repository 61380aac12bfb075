"""kge_train_step_reg's host layer (CPU only): its argument rejections sit ahead of the first device call, so dummy
pointers reach them (as in test_abi_matrix_cpu.py), and its workspace size query needs no device."""
import importlib.util
import itertools
import math
import os

import pytest

from customknowledgegraphembedding_amd import _lib

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_abi_matrix", os.path.join(GOLDEN_DIR, "make_abi_matrix.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

KGE_EINVAL, KGE_ENOTSUP = -22, -95  # include/kge_hip.h
P, BIG = 4096, 1 << 40  # a dummy non-null pointer (never dereferenced: every case is refused first)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _call(lib, fn=1, mode=1, B=2, N=4, D=4, w=P, step=1, lam=0.05, log=P, wsb=BIG):
    rc = lib.kge_train_step_reg(fn, mode, P, 10, 8, P, 2, 12, 0, P, P, 4, B, N, D, 1.0, 1.0, 1.0, 1, 1, w, P, None, P,
                                P, P, P, P, P, 0.001, 0.9, 0.999, 1e-8, step, 0, P, wsb, None, lam, log)
    return rc, lib.kge_last_error().decode()


@pytest.mark.parametrize("lam", [-1.0, -1e-30, math.nan, math.inf, -math.inf])
def test_bad_lambda_is_einval(lib, lam):
    rc, msg = _call(lib, lam=lam)
    assert rc == KGE_EINVAL and "regularization" in msg


def test_good_lambda_passes_that_check(lib):
    """The same call with a valid lambda gets as far as the next rejection (a 16-byte workspace)."""
    for lam in (0.0, 2e-6, 0.05):
        rc, msg = _call(lib, lam=lam, wsb=16)
        assert rc == KGE_EINVAL and "workspace too small" in msg


def test_protate_is_enotsup(lib):
    rc, msg = _call(lib, fn=5)
    assert rc == KGE_ENOTSUP and "pRotatE" in msg


def test_step_is_one_based(lib):
    for step in (0, -3):
        rc, msg = _call(lib, step=step)
        assert rc == KGE_EINVAL and "1-based" in msg


def test_rejections_of_the_plain_step_hold(lib):
    assert _call(lib, mode=3) == (KGE_EINVAL, "kge_train_step needs a negative mode (0 or 1)")
    assert _call(lib, B=0) == (KGE_EINVAL, "bad shape")
    assert _call(lib, D=4096)[0] != 0
    # NULL weights are uni_weight here (the call goes on to the workspace check) and an error in kge_train_step
    assert _call(lib, w=None, wsb=16) == (KGE_EINVAL, "workspace too small")
    assert _call(lib, log=None, wsb=16) == (KGE_EINVAL, "workspace too small")
    rc = lib.kge_train_step(1, 1, P, 10, 8, P, 2, 12, 0, P, P, 4, 2, 4, 4, 1.0, 1.0, 1.0, 1, 1, None, P, None, P, P, P,
                            P, P, P, 0.001, 0.9, 0.999, 1e-8, 1, 0, P, BIG, None)
    assert (rc, lib.kge_last_error().decode()) == (KGE_EINVAL, "null pointer")


def test_workspace_size_covers_the_plain_steps(lib):
    """On the size matrix of test_abi_matrix_cpu.py: never smaller than kge_train_step's, -1 exactly where that is,
    and a workspace of the plain size is refused by the new entry point."""
    n = above = 0
    for fn, D, B, N, E in itertools.product(M.FNS, M.DS, M.BS, M.NS, M.ES):
        a = dict(M.sweep_queries(fn, D, B, N, E))["kge_train_step_workspace_size"]
        plain = lib.kge_train_step_workspace_size(*a)
        reg = lib.kge_train_step_reg_workspace_size(*a)
        assert (reg == -1) == (plain == -1) and reg >= plain, a
        n += 1
        above += reg > plain or plain == -1
    assert n == 6 * 8 * 4 * 5 * 3 and above == n  # the regulariser's partials and the log's parts always add
    for a in ([7, 10, 3, 8, 2, 4, 8], [0, 10, 3, 8, -2, 4, 8], [0, -1, 3, 8, 2, 4, 8]):
        assert lib.kge_train_step_reg_workspace_size(*a) == lib.kge_train_step_workspace_size(*a) == -1, a
    plain = lib.kge_train_step_workspace_size(1, 10, 2, 12, 2, 4, 4)
    assert _call(lib, wsb=plain) == (KGE_EINVAL, "workspace too small")


def test_signatures_present():
    for sym in ("kge_train_step_reg", "kge_train_step_reg_workspace_size"):
        assert sym in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["kge_train_step_reg"]
    plain = _lib.SIGNATURES["kge_train_step"][1]
    assert args[:len(plain)] == plain and len(args) == len(plain) + 2  # kge_train_step's list, then lambda and log
    assert _lib.SIGNATURES["kge_train_step_reg_workspace_size"] == _lib.SIGNATURES["kge_train_step_workspace_size"]
