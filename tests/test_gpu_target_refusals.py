"""The capability matrix of the data-set targets that run their own kernels ("The target table"; kTargets of csrc/api_common.h),
cell by cell through the public ABI on ONE context: every entry a target lacks returns MIVI_ERR_UNSUPPORTED with the whole message
"<entry>: not supported on the <target name>" before it reads a buffer, and every mivi_<t>_select_rows on another target's context names
the entry that does select that target's rows.  The expected texts are the ones the hand-written guards gave before the table.  Only
refused cells are called (with placeholder buffers); the per-target test files exercise the others."""
import numpy as np
import pytest

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import _lib

pytestmark = pytest.mark.gpu

SEED = 0x38BEF07CF9CC549D
D, M = 11, 4   # d = 11: PPCA with n = 6, D = 2, k = 1; a 3 -> 2 -> 1 network; softmax with p = 5, C = 2; a GLM with p = 3, J = 7

SOFTMAX = "softmax regression target (mivi_set_target_softmax)"
BNN = "Bayesian neural network target (mivi_set_target_bnn)"
HGLM = "hierarchical GLM target (mivi_set_target_hglm)"
PPCA = "probabilistic PCA target (mivi_set_target_ppca)"

X3, Y8 = np.zeros((8, 3), np.float32), np.zeros(8, np.float32)
PROBLEMS = {
    SOFTMAX: lambda: avi.SoftmaxRegProblem(np.zeros((8, 5), np.float32), np.zeros(8, np.uint8), 2),
    BNN: lambda: avi.BNNProblem(X3, Y8, (2,)),
    HGLM: lambda: avi.HierGLMProblem(X3, Y8, np.arange(8) % 7, 7),
    PPCA: lambda: avi.PPCAProblem(np.zeros((6, 2), np.float32, order="F"), 1),
}
SELECT_ROWS = {SOFTMAX: "mivi_softmax_select_rows", BNN: "mivi_bnn_select_rows", HGLM: "mivi_hglm_select_rows", PPCA: "mivi_ppca_select_rows"}

# the entries every target lacks, as the message names them
HESS2 = "mivi_gauss_expected_grad_hess2 (second-order branch: the target has no Hessian kernel; use mivi_gauss_expected_grad_hess)"
MANY = "mivi_optimize_loop_many (the target has no launch-free loop)"
BATCHES = "mivi_optimize_loop_batches"
SCHEDULE = "mivi_logreg_set_batch_schedule"
SEEK = "mivi_logreg_seek_batch"


def _raw(call):
    return lambda ctx, P, buf: call(ctx.lib, ctx.h, P)


def _wrapped(call):
    def run(ctx, P, buf):
        with pytest.raises(avi.MiviError) as e:
            call(ctx, buf)
        return e.value.status
    return run


CALLS = {
    HESS2: _raw(lambda lib, h, P: lib.mivi_gauss_expected_grad_hess2(h, P, 0, 0, P, P, P)),
    MANY: _wrapped(lambda ctx, buf: ctx.optimize_loop_many(buf[:2 * ctx.params_len], 2, 2, 0, 0)),
    BATCHES: _wrapped(lambda ctx, buf: ctx.optimize_loop_batches(buf, 2, 0, 0)),
    SCHEDULE: _wrapped(lambda ctx, buf: ctx.set_batch_schedule(np.zeros((1, 2), np.int64), likeadj=1.0)),
    SEEK: _raw(lambda lib, h, P: lib.mivi_logreg_seek_batch(h, 0)),
}

# The one cell of the select-rows matrix that is not a refusal by name: (context's target, entry) -> (status, whole message)
NO_TARGET = {(SOFTMAX, "mivi_bnn_select_rows"): "no Bayesian neural network target set"}


@pytest.fixture(scope="module")
def ctx():
    c = avi.MiviContext(np.float32, avi.FULLRANK, D, M, 0, SEED)
    yield c
    c.close()


@pytest.mark.parametrize("target", list(PROBLEMS))
def test_refused_cells_give_the_whole_message(ctx, target):
    ctx.set_problem(PROBLEMS[target]())
    buf, idx = ctx.empty(4 * D * D + 64), np.zeros(2, np.int64)
    P, lib, h = ctx._p(buf), ctx.lib, ctx.h
    for entry, call in CALLS.items():
        status, msg = call(ctx, P, buf), lib.mivi_last_error(h).decode()
        print(f"{target} | {entry} -> {status} {msg!r}")
        assert status == _lib.ERR_UNSUPPORTED, (target, entry)
        assert msg == entry + ": not supported on the " + target, (target, entry, msg)
    others = ["mivi_logreg_select_rows"] + [e for t, e in SELECT_ROWS.items() if t != target]
    assert len(others) == 4
    for entry in others:
        status, msg = getattr(lib, entry)(h, idx.ctypes.data, 2, 1.0), lib.mivi_last_error(h).decode()
        print(f"{target} | {entry} -> {status} {msg!r}")
        if (target, entry) in NO_TARGET:
            assert (status, msg) == (_lib.ERR_NO_TARGET, NO_TARGET[(target, entry)]), (target, entry, status, msg)
        else:
            assert status == _lib.ERR_UNSUPPORTED, (target, entry)
            assert msg == f"{entry} (its rows are selected by {SELECT_ROWS[target]}): not supported on the {target}", (target, entry, msg)
