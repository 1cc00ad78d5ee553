"""What the `_host` entries of the C ABI return (the calls julia/MIVI.jl makes on every step): mivi_estimate_gradient_host,
mivi_estimate_objective_host, mivi_gauss_expected_grad_hess_host / _hess2_host and mivi_estimate_score_gradient_host.

A `_host` entry is its device entry between an upload of the parameters and a download of the results, so the comparison is BITWISE:
the `_host` call on a fresh context against the device entry on another fresh context, same (params, idx, n_samples).  Every case
first asserts that the device entry is itself bitwise equal across two fresh contexts (otherwise the shape would say nothing).  The
second-order Hessian is compared on the diagonal-Gaussian target only: its Hessian is constant, while the sampled targets accumulate
theirs with f64 atomics in an order that differs from run to run (kernels_hess2.hip).

Status behaviour: mivi_estimate_gradient_host reports the sticky device flags like mivi_synchronize (read_status);
mivi_estimate_objective_host reports a non-positive scale only and returns a non-finite value as it is."""
import numpy as np
import pytest

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import MiviError
from advancedvi_jl_amd import _lib
from tests.helpers import SEED, make_family, make_problem

pytestmark = pytest.mark.gpu

MC = avi.MonteCarloEntropy.code
IDX = 5


def setup(d, family, kind, dtype, seed=41):
    rng = np.random.default_rng(seed + d)
    q, _ = make_family(rng, d, family, dtype)
    prob, _ = make_problem(rng, kind, d, dtype)
    params, _ = avi.destructure(q)
    return prob, np.ascontiguousarray(params, dtype=dtype)


def fresh(d, M, family, dtype, prob, entropy=0):
    ctx = avi.MiviContext(dtype, family, d, M, entropy, SEED)
    ctx.set_problem(prob)
    return ctx


def on_fresh(d, M, family, dtype, prob, call, entropy=0):
    ctx = fresh(d, M, family, dtype, prob, entropy)
    try:
        out = call(ctx)
        ctx.synchronize()
        return [None if o is None else (o.cpu().numpy().copy() if hasattr(o, "cpu") else np.asarray(o)) for o in out]
    finally:
        ctx.close()


def assert_host_is_device(d, M, family, dtype, prob, device_call, host_call, entropy=0):
    """device entry twice (repeatable) and the _host entry once, each on a fresh context; every output bitwise equal."""
    dev = on_fresh(d, M, family, dtype, prob, device_call, entropy)
    dev2 = on_fresh(d, M, family, dtype, prob, device_call, entropy)
    host = on_fresh(d, M, family, dtype, prob, host_call, entropy)
    assert len(dev) == len(dev2) == len(host)
    for k, (a, b, h) in enumerate(zip(dev, dev2, host)):
        if h is None:   # (an output the _host call was asked not to return)
            continue
        a, b, h = a.reshape(-1), b.reshape(-1), np.asarray(h).reshape(-1)
        assert a.dtype == h.dtype == np.dtype(dtype), k
        assert np.all(np.isfinite(a)), k
        assert np.array_equal(a, b), ("the device entry is not repeatable at this shape", k)
        assert np.array_equal(a, h), ("the _host entry differs from the device entry", k, float(np.max(np.abs(a - h))))


@pytest.mark.parametrize("family,dtype,d,M,kind", [
    (avi.FULLRANK, np.float32, 64, 64, "diag"),      # second-generation route
    (avi.FULLRANK, np.float32, 64, 64, "dense"),
    (avi.FULLRANK, np.float64, 10, 8, "diag"),       # general route
    (avi.MEANFIELD, np.float32, 33, 16, "diag"),
], ids=["fullrank-f32-64x64-diag", "fullrank-f32-64x64-dense", "fullrank-f64-10x8-diag", "meanfield-f32-33x16-diag"])
def test_estimate_gradient_host(family, dtype, d, M, kind):
    prob, params = setup(d, family, kind, dtype)
    assert_host_is_device(d, M, family, dtype, prob,
                          lambda c: c.estimate_gradient(params, IDX),
                          lambda c: c.estimate_gradient_host(params, IDX))


@pytest.mark.parametrize("n_samples", [64, 16384 + 64], ids=["single-call", "chunk-loop"])
def test_estimate_objective_host(n_samples):
    d, M, family, dtype = 64, 64, avi.FULLRANK, np.float32
    prob, params = setup(d, family, "diag", dtype)
    assert_host_is_device(d, M, family, dtype, prob,
                          lambda c: (c.estimate_objective(params, IDX, n_samples=n_samples, entropy=MC),),
                          lambda c: (c.estimate_objective_host(params, IDX, n_samples=n_samples, entropy=MC),))


@pytest.mark.parametrize("dtype,d,M,second_order", [
    (np.float32, 64, 128, False),
    (np.float64, 10, 8, False),
    (np.float32, 64, 128, True),     # diagonal-Gaussian target: a constant Hessian
], ids=["first-order-f32-64x128", "first-order-f64-10x8", "second-order-f32-64x128"])
def test_gauss_expected_grad_hess_host(dtype, d, M, second_order):
    family = avi.FULLRANK
    prob, params = setup(d, family, "diag", dtype)
    assert_host_is_device(d, M, family, dtype, prob,
                          lambda c: c.gauss_expected_grad_hess(params, IDX, second_order=second_order),
                          lambda c: c.gauss_expected_grad_hess_host(params, IDX, second_order=second_order))


@pytest.mark.parametrize("want_elbo", [True, False], ids=["elbo", "elbo-null"])
@pytest.mark.parametrize("family,dtype,d,M", [(avi.FULLRANK, np.float32, 64, 64), (avi.MEANFIELD, np.float64, 10, 8)],
                         ids=["fullrank-f32-64x64", "meanfield-f64-10x8"])
def test_estimate_score_gradient_host(family, dtype, d, M, want_elbo):
    prob, params = setup(d, family, "diag", dtype)
    assert_host_is_device(d, M, family, dtype, prob,
                          lambda c: c.estimate_score_gradient(params, IDX),
                          lambda c: c.estimate_score_gradient_host(params, IDX, want_elbo=want_elbo))


def bad_scale_case(family):
    """test_gpu_parity.py's trick: one negative scale-diagonal entry at d = 32, M = 16."""
    d, M = 32, 16
    rng = np.random.default_rng(5)
    q, _ = make_family(rng, d, family, np.float32)
    prob, _ = make_problem(rng, "diag", d, np.float32)
    good, _ = avi.destructure(q)
    good = np.ascontiguousarray(good, dtype=np.float32)
    bad = good.copy()
    bad[d + (3 if family == avi.MEANFIELD else 3 * d + 3)] = -0.25
    return d, M, prob, good, bad


@pytest.mark.parametrize("family", [avi.MEANFIELD, avi.FULLRANK], ids=["meanfield", "fullrank"])
def test_estimate_gradient_host_reports_a_nonpositive_scale_once(family):
    d, M, prob, good, bad = bad_scale_case(family)
    ctx = fresh(d, M, family, np.float32, prob)
    with pytest.raises(MiviError, match="scale diagonal") as ei:
        ctx.estimate_gradient_host(bad, 0)
    assert ei.value.status == _lib.ERR_NONPOSITIVE_SCALE
    v, g = ctx.estimate_gradient_host(good, 1)     # the very next call on the same context: the flag was cleared by the read
    assert np.isfinite(v) and np.all(np.isfinite(g))
    ctx.close()


@pytest.mark.parametrize("family", [avi.MEANFIELD, avi.FULLRANK], ids=["meanfield", "fullrank"])
def test_estimate_objective_host_returns_a_nonfinite_value_without_raising(family):
    """Its difference from read_status: MIVI_ERR_NONPOSITIVE_SCALE is the only status it reports -- a non-finite value comes back as
    it is (like the reference's estimate_objective), and its flag is cleared, so the next _host call does not report it either.
    (The negative scale entry itself sets the non-positive-scale flag, which this entry does report: the value that must come back
    without an error is the one of an infinite location at a positive scale.)"""
    d, M, prob, good, bad = bad_scale_case(family)
    ctx = fresh(d, M, family, np.float32, prob)
    with pytest.raises(MiviError, match="scale diagonal") as ei:
        ctx.estimate_objective_host(bad, 0)
    assert ei.value.status == _lib.ERR_NONPOSITIVE_SCALE
    inf_mean = good.copy()
    inf_mean[2] = np.inf
    v = ctx.estimate_objective_host(inf_mean, 1)   # no MIVI_ERR_NONFINITE
    assert not np.isfinite(v)
    v, g = ctx.estimate_gradient_host(good, 2)     # ... and nothing sticky left behind for read_status
    assert np.isfinite(v) and np.all(np.isfinite(g))
    v = ctx.estimate_objective_host(good, 3)
    assert np.isfinite(v)
    ctx.close()
