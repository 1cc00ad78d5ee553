"""What the GPU tests of the measure-space algorithms share (tests/test_gpu_sqrt_ngd.py, tests/test_gpu_natgrad.py): the criteria, the dense
and reference-model cases, the yardstick check and the refusal helper."""
import functools

import numpy as np
import pytest

import advancedvi_jl_amd as avi
from advancedvi_jl_amd._lib import MiviError
from oracle import oracle as O
from tests import solve_ref as S
from tests.helpers import SEED, make_family, make_problem

F32_FACTOR = 8.0                 # tests/test_gpu_solve_yardstick.py
VALUE_RTOL = 1e-5                # tests/test_gpu_parity.py (f32 values)
TOL64 = (1e-12, 1e-11)           # tests/test_gpu_parity.py TOL[np.float64]
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])


def flat(H):
    return np.ascontiguousarray(np.asarray(H).reshape(-1, order="F"))


def hold(tag, what, d, got, yard, ref):
    whole, block = S.block_ratios(got, yard, ref, d)
    print(f"[{tag} yardstick] {what} {d}: {whole:.2f}, {block:.2f}")
    assert np.all(np.isfinite(got))
    assert whole <= F32_FACTOR and block <= F32_FACTOR, (what, d, whole, block)


@functools.lru_cache(maxsize=8)
def dense_setup(d, dtype):
    rng = np.random.default_rng(900 + d)
    q, q_o = make_family(rng, d, avi.FULLRANK, dtype)
    prob, tgt = make_problem(rng, "dense", d, dtype)
    params, _ = avi.destructure(q)
    return params, q_o, prob, tgt


def dense_ctx(d, n, dtype, second):
    params, q_o, prob, tgt = dense_setup(d, dtype)
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, n, 0, SEED)
    ctx.set_problem(avi.DenseNormalProblem(prob.mean, prob.L, order=2 if second else 1))
    return ctx, params, q_o, tgt


def reference_model(dtype, order):
    """test/models/normal.jl `normal_meanfield`: d = 5, mu = 5, sigma = 0.3; q0 = N(0, I)"""
    d = 5
    prob = avi.DiagNormalProblem(np.full(d, 5.0, dtype), np.full(d, 0.3, dtype), order=order)
    return d, prob, O.DiagNormalTarget(np.full(d, 5.0), np.full(d, 0.3)), avi.FullRankGaussian(np.zeros(d, dtype), np.eye(d, dtype=dtype))


def trajectory_case(model, dtype, second):
    if model == "reference":
        d, prob, tgt, q0 = reference_model(dtype, 2 if second else 1)
        params, _ = avi.destructure(q0)
        q_o, n, eta = O.MvLocationScale(np.zeros(d), np.eye(d)), 10, 1e-3
        ctx = avi.MiviContext(dtype, avi.FULLRANK, d, n, 0, SEED)
        ctx.set_problem(prob)
    else:
        d, n, eta = 33, 17, 0.02
        ctx, params, q_o, tgt = dense_ctx(d, n, dtype, second)
    return ctx, d, n, eta, params, q_o, tgt


def logreg(order=1):
    rng = np.random.default_rng(77)
    X = rng.normal(size=(8, 3)) / 2.0
    y = (rng.uniform(size=8) < 0.5).astype(np.uint8)
    return avi.LogRegProblem(X, y, "logsigma_normal", 1.0, order=order)


def refused(fn):
    with pytest.raises(MiviError) as e:
        fn()
    return e.value.status
