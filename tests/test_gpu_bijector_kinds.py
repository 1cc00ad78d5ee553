"""GPU tests of the extended Stacked bijector (mivi_set_bijector_stacked_ex: truncated(lb, ub) and ordered blocks, csrc/kernels_bijector.hip)
and of the constrained approximation (mivi_sample_constrained, mivi_logpdf_constrained, avi.TransformedDistribution) against the numpy
restatement tests/bijector_ref.py on the draws the context itself returns.

Tolerances
    f64: TOL64 of tests/test_gpu_scoregrad.py (value rel 1e-12, gradient l2 1e-11 against max(|g|, 1)), against the float64 restatement.
    f32: no number.  The library's distance from the float64 result is at most F32_FACTOR = 8 x the distance of the same restatement
         evaluated in float32 numpy, both maximised over the estimate indices INDICES (the yardstick and factor of test_gpu_scoregrad.py).
Shapes: d in {5, 37, 300} (300 > 256: the column loop and the scan carry across a chunk), M in {1, 10, 33}; layouts: bijector_ref.layout.
The same kernels are held PER ENTRY, at the helpers' default scales and on wider classes, by tests/test_gpu_bijector_yardstick.py."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import _lib
from oracle import oracle as O
from tests import basedist_ref as B
from tests import bijector_ref as BR
from tests import logpdf_ref as LP
from tests import lowrank_ref as LR
from tests import scoregrad_ref as SR
from tests.helpers import SEED, OraclePlugin, make_family, make_problem

pytestmark = pytest.mark.gpu

TOL64 = (1e-12, 1e-11)
F32_FACTOR = 8.0
INDICES = (0, 1, 2, 7, 1000003)
SHAPES = [(5, 1), (37, 10), (300, 33)]
DTYPES = [np.float32, np.float64]
FAMILIES = [avi.MEANFIELD, avi.FULLRANK]
dt_id = lambda t: "f32" if t == np.float32 else "f64"          # noqa: E731
fam_id = lambda f: "meanfield" if f == avi.MEANFIELD else "fullrank"   # noqa: E731


def make_q(rng, d, family, dtype):
    """helpers.make_family with scales in (0.2, 0.6): behind e^eta the default scales (up to 1.5) let ONE draw carry a whole gradient
    component (e^eta g ~ 1e4 next to 1e1), and the float32 distance of a sum that is one term is the luck of a single rounding -- no
    yardstick.  With these every component is a sum of comparable terms."""
    q, _ = make_family(rng, d, family, dtype, mu_scale=0.3)
    scale = (q.scale * dtype(0.4)).astype(dtype)
    return avi.MvLocationScale(q.location, scale), O.MvLocationScale(q.location.astype(np.float64), scale.astype(np.float64))


def build_problem(rng, kind, d, dtype):
    """(problem the context takes WITHOUT the bijector, oracle target)"""
    if kind == "funnelc":
        return avi.FunnelConstrainedProblem(d, 1.5), O.FunnelConstrainedTarget(d, 1.5)
    if kind == "callback":   # the plugin sees CONSTRAINED samples
        _, tgt = make_problem(rng, "diag", d, dtype)
        return OraclePlugin(tgt), tgt
    return make_problem(rng, kind, d, dtype)


def transformed(prob, blocks):
    return avi.TransformedProblem(prob, avi.StackedBijector(blocks))


def hold(what, lib_d, cpu_d, dtype, ref_scale):
    """lib_d / cpu_d: per index, (|value - ref|, |grad - ref|_2) of the library and of the restatement in dtype; ref_scale: per index
    (|value_ref|, max(|grad_ref|, 1))"""
    lib_d, cpu_d, ref_scale = np.array(lib_d), np.array(cpu_d), np.array(ref_scale)
    if dtype == np.float64:
        rel = lib_d / ref_scale
        print(f"[bijector f64] {what}: value {rel[:, 0].max():.3e}, gradient {rel[:, 1].max():.3e}")
        assert np.all(rel[:, 0] <= TOL64[0]), (what, rel[:, 0])
        assert np.all(rel[:, 1] <= TOL64[1]), (what, rel[:, 1])
        return
    lib_m, cpu_m = lib_d.max(axis=0), cpu_d.max(axis=0)
    ratio = [float(a / b) if b > 0 else (0.0 if a == 0 else math.inf) for a, b in zip(lib_m, cpu_m)]
    print(f"[bijector f32] {what}: library (value, gradient) {lib_m.tolist()}  float32 numpy {cpu_m.tolist()}  ratio {ratio}")
    for name, a, b in zip(("value", "gradient"), lib_m, cpu_m):
        assert a <= F32_FACTOR * b, (what, name, a, b)


def dists(got_v, got_g, ref):
    return abs(got_v - ref["value"]), float(np.linalg.norm(np.asarray(got_g, dtype=np.float64) - ref["grad"]))


def scales(ref):
    return abs(ref["value"]), max(float(np.linalg.norm(ref["grad"])), 1.0)


def run_parity(family, dtype, kind, d, M, ent=0, grad_only=False, case=None):
    if case is None:
        rng = np.random.default_rng(977 + d + 7 * M)
        q, _ = make_q(rng, d, family, dtype)
        prob, tgt = build_problem(rng, kind, d, dtype)
        blocks = BR.layout(d)
    else:
        d, blocks, loc, scale, mean, std = BR.cancellation_case(case, dtype)
        q = avi.MeanFieldGaussian(loc, scale) if family == avi.MEANFIELD else avi.FullRankGaussian(loc, np.diag(scale))
        prob, tgt = avi.DiagNormalProblem(mean, std), O.DiagNormalTarget(mean, std)
    params, _ = avi.destructure(q)
    ctx = avi.MiviContext(dtype, family, d, M, ent, SEED)
    ctx.set_problem(transformed(prob, blocks))
    pd = ctx.to_device(params)
    lib_d, cpu_d, sc = [], [], []
    for idx in INDICES:
        _, eps = ctx.sample(pd, idx)
        eps = eps.cpu().numpy().copy()
        v, g = ctx.estimate_gradient(pd, idx)
        ctx.synchronize()
        v, g = float(v.item()), g.cpu().numpy().astype(np.float64)
        assert np.isfinite(v) and np.all(np.isfinite(g))
        ref = BR.estimate_gradient(params.astype(np.float64), d, family, tgt, blocks, eps.astype(np.float64), ent)
        if family == avi.FULLRANK:   # exact zeros above the diagonal
            assert np.all(np.triu(g[d:].reshape(d, d, order="F"), 1) == 0.0)
        lib_d.append(dists(v, g, ref))
        sc.append(scales(ref))
        if dtype == np.float32:
            cpu_d.append(dists(*[BR.estimate_gradient(params, d, family, tgt, blocks, eps, ent, np.float32)[k] for k in ("value", "grad")], ref))
    ctx.close()
    lib_d, cpu_d = np.array(lib_d), np.array(cpu_d)
    if grad_only:
        lib_d[:, 0] = 0.0
    hold(f"{kind if case is None else case} fam={family} d={d} M={M} ent={ent}", lib_d, cpu_d, dtype, sc)


# ---- 1. parity on identical draws --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["diag", "dense", "logreg0", "funnelc", "callback"])
def test_parity_on_identical_draws(kind, shape, family, dtype):
    run_parity(family, dtype, kind, *shape)


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
@pytest.mark.parametrize("ent", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_entropy_estimator_on_the_diag_target(shape, ent, family, dtype):
    run_parity(family, dtype, "diag", *shape, ent=ent)


def _other_route(dtype, make_ctx, params, d, M, blocks, reference, what):
    """one case of a route that is not Gaussian RepGradELBO: reference(tgt_wrapper_dtype, draws, dtype) -> dict(value, grad)"""
    lib_d, cpu_d, sc = [], [], []
    ctx = make_ctx()
    pd = ctx.to_device(params)
    for idx in INDICES:
        _, U = ctx.sample(pd, idx)
        U = U.cpu().numpy().copy()
        v, g = ctx.estimate_gradient(pd, idx)
        ctx.synchronize()
        ref = reference(np.float64, U.astype(np.float64))
        lib_d.append(dists(float(v.item()), g.cpu().numpy(), ref))
        sc.append(scales(ref))
        if dtype == np.float32:
            yard = reference(np.float32, U)
            cpu_d.append(dists(yard["value"], yard["grad"], ref))
    ctx.close()
    hold(what, lib_d, cpu_d, dtype, sc)


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
def test_low_rank_family(dtype):
    d, M, r = 37, 10, 2
    rng = np.random.default_rng(5)
    q = avi.LowRankGaussian(0.3 * rng.normal(size=d).astype(dtype), rng.uniform(0.5, 1.5, size=d).astype(dtype), (0.3 * rng.normal(size=(d, r))).astype(dtype))
    prob, tgt = make_problem(rng, "dense", d, dtype)
    blocks = BR.layout(d)
    params, _ = avi.destructure(q)

    def make_ctx():
        ctx = avi.MiviContext(dtype, avi.LOWRANK, d, M, 0, SEED, rank=r)
        ctx.set_problem(transformed(prob, blocks))
        return ctx

    def reference(dt, eps):
        ref = LR.estimate_gradient(params.astype(np.float64), d, r, BR.BijectorTarget(tgt, blocks), eps.astype(np.float64), 0)
        if dt == np.float64:
            return ref
        Z = ref["Z"].astype(np.float32)   # the float32 yardstick: the transformed target in float32 at the float32 samples, the family by Woodbury
        ell, G = BR.target_eval(tgt, blocks, Z, np.float32)
        return LR.woodbury_eval(params, d, r, G, ell, eps, 0, np.float32)

    _other_route(dtype, make_ctx, params, d, M, blocks, reference, f"lowrank r={r} d={d} M={M}")


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
@pytest.mark.parametrize("dist", [avi.Laplace(), avi.TDist(5.0)], ids=repr)
def test_non_normal_bases(dist, family, dtype):
    d, M, ent = 37, 10, 3
    rng = np.random.default_rng(6)
    q0, _ = make_q(rng, d, family, dtype)
    q = avi.MvLocationScale(q0.location, q0.scale, dist)
    prob, tgt = make_problem(rng, "dense", d, dtype)
    blocks = BR.layout(d)
    params, _ = avi.destructure(q)

    def make_ctx():
        ctx = avi.MiviContext(dtype, family, d, M, ent, SEED)
        ctx.set_base_dist(dist)
        ctx.set_problem(transformed(prob, blocks))
        return ctx

    def reference(dt, U):
        return B.estimate_gradient(params.astype(dt), d, family, BR.BijectorTarget(tgt, blocks, dt), U, ent, B.base_of(dist), dtype=dt)

    _other_route(dtype, make_ctx, params, d, M, blocks, reference, f"{dist!r} fam={family} d={d} M={M}")


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
def test_score_gradient_estimator(family, dtype):
    d, M = 37, 33
    rng = np.random.default_rng(8)
    q, q_o = make_q(rng, d, family, dtype)
    prob, tgt = make_problem(rng, "dense", d, dtype)
    blocks = BR.layout(d)
    params, _ = avi.destructure(q)
    ctx = avi.MiviContext(dtype, family, d, M, 0, SEED)
    ctx.set_problem(transformed(prob, blocks))
    pd = ctx.to_device(params)
    lib_d, cpu_d, sc, lib_e, cpu_e = [], [], [], [], []
    for idx in INDICES:
        _, eps = ctx.sample(pd, idx)
        eps = eps.cpu().numpy().copy()
        v, e, g = ctx.estimate_score_gradient(pd, idx)
        ctx.synchronize()
        ref = SR.closed_form(O.destructure(q_o), d, family, BR.BijectorTarget(tgt, blocks), eps.astype(np.float64))
        lib_d.append(dists(float(v.item()), g.cpu().numpy(), ref))
        lib_e.append(abs(float(e.item()) - float(ref["elbo"])) / abs(float(ref["elbo"])))
        sc.append(scales(ref))
        if dtype == np.float32:
            yard = SR.closed_form(params, d, family, BR.BijectorTarget(tgt, blocks, np.float32), eps, np.float32)
            cpu_d.append(dists(float(yard["value"]), yard["grad"], ref))
            cpu_e.append(abs(float(yard["elbo"]) - float(ref["elbo"])) / abs(float(ref["elbo"])))
    ctx.close()
    hold(f"score gradient fam={family} d={d} M={M}", lib_d, cpu_d, dtype, sc)
    # the separate elbo scalar: a value, held as one (TOL64[0]; f32: the same yardstick)
    print(f"[bijector {dt_id(dtype)}] score gradient elbo fam={family}: library {max(lib_e):.3e}" + (f", float32 numpy {max(cpu_e):.3e}" if cpu_e else ""))
    assert max(lib_e) <= (TOL64[0] if dtype == np.float64 else F32_FACTOR * max(cpu_e))


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
def test_estimate_objective_past_one_chunk(family, dtype):
    """n_samples past the 16384-sample chunk: the value on the concatenated draws, the log-Jacobian in every chunk"""
    d, n_mc, n, idx = 5, 16, 16384 + 37, 2
    rng = np.random.default_rng(9)
    q, q_o = make_q(rng, d, family, dtype)
    prob, tgt = make_problem(rng, "diag", d, dtype)
    blocks = BR.layout(d)
    params, _ = avi.destructure(q)
    sampler = avi.MiviContext(dtype, family, d, n, 0, SEED)
    eps = sampler.sample(params, idx)[1].cpu().numpy()
    sampler.close()
    ctx = avi.MiviContext(dtype, family, d, n_mc, 0, SEED)
    ctx.set_problem(transformed(prob, blocks))
    got = float(ctx.estimate_objective(params, idx, n_samples=n, entropy=2).item())
    ctx.close()
    Z = BR.samples(params.astype(np.float64), d, family, eps.astype(np.float64))
    ell, _ = BR.target_eval(tgt, blocks, Z)
    want = -(np.mean(ell) + np.mean(0.5 * np.sum(eps.astype(np.float64) ** 2, axis=0)) + 0.5 * d * BR.LOG2PI
             + np.sum(np.log(q_o.scale if family == avi.MEANFIELD else np.diag(q_o.scale))))
    if dtype == np.float64:
        print(f"[bijector f64] estimate_objective fam={family} n={n}: {abs(got - want) / abs(want):.3e}")
        assert abs(got - want) <= TOL64[0] * abs(want), (got, want)
    else:
        Z32 = BR.samples(params, d, family, eps, np.float32)
        ell32, _ = BR.target_eval(tgt, blocks, Z32, np.float32)
        yard = -(np.mean(ell32, dtype=np.float32) + np.mean(np.float32(0.5) * np.sum(eps * eps, axis=0, dtype=np.float32), dtype=np.float32)
                 + np.float32(0.5 * d * BR.LOG2PI) + np.sum(np.log(params[d:] if family == avi.MEANFIELD else np.diag(params[d:].reshape(d, d))), dtype=np.float32))
        print(f"[bijector f32] estimate_objective fam={family} n={n}: library {abs(got - want):.3e}, float32 numpy {abs(float(yard) - want):.3e}")
        assert abs(got - want) <= F32_FACTOR * abs(float(yard) - want)


# ---- 2. cancellation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
@pytest.mark.parametrize("which", ["lower", "ordered"])
def test_jacobian_factor_survives_cancellation_in_f32(which, family):
    """lb = 1000 with eta ~ -5, x_b ~ 100 with eta_k ~ -6: the float32 yardstick takes e^eta from eta (within 1e-5 of float64:
    tests/test_bijector_ref_host.py); a backward pass that differences the stored x misses it by orders of magnitude.  Gradient only."""
    run_parity(family, np.float32, None, None, 33, grad_only=True, case=which)


# ---- 3. known answers --------------------------------------------------------------------------------------------------------------------
def _estimate(family, dtype, d, M, prob, bij, params, idx=4, ent=0):
    ctx = avi.MiviContext(dtype, family, d, M, ent, SEED)
    ctx.set_problem(prob)
    if bij is not None:
        ctx.set_bijector(avi.StackedBijector(bij))
    v, g = ctx.estimate_gradient(params, idx)
    ctx.synchronize()
    out = (v.cpu().numpy().copy(), g.cpu().numpy().copy())
    ctx.close()
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
def test_truncated_zero_inf_is_bitwise_the_exp_kind(family, dtype):
    d, M = 300, 33
    rng = np.random.default_rng(12)
    q, _ = make_q(rng, d, family, dtype)
    prob, _ = make_problem(rng, "dense", d, dtype)
    params, _ = avi.destructure(q)
    a = _estimate(family, dtype, d, M, prob, [(0, 3, "exp"), (250, 270, "exp")], params)
    b = _estimate(family, dtype, d, M, prob, [(0, 3, "truncated", (0.0, np.inf)), (250, 270, "truncated", (0.0, np.inf))], params)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
def test_identity_only_bijector_is_bitwise_no_bijector(family, dtype):
    d, M = 37, 10
    rng = np.random.default_rng(13)
    q, _ = make_family(rng, d, family, dtype)
    prob, _ = make_problem(rng, "diag", d, dtype)
    params, _ = avi.destructure(q)
    a = _estimate(family, dtype, d, M, prob, None, params)
    b = _estimate(family, dtype, d, M, prob, [(0, 5, "truncated", (-np.inf, np.inf)), (5, 6, "ordered"), (9, 10, "ordered"), (10, 10, "ordered")], params)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
def test_logit_normal_density(dtype):
    """d = 1, q = N(0.3, 0.8), truncated(0, 1): log N(logit x; 0.3, 0.8) - log(x (1 - x))"""
    x = np.array([0.02, 0.25, 0.5, 0.731, 0.999], dtype=dtype)
    ctx = avi.MiviContext(dtype, avi.MEANFIELD, 1, 1, 0, SEED)
    ctx.set_bijector(avi.StackedBijector([(0, 1, "truncated", (0.0, 1.0))]))
    params = np.array([0.3, 0.8], dtype=dtype)
    got = ctx.logpdf_constrained(params, x[None, :]).cpu().numpy().astype(np.float64)
    got_h = ctx.logpdf_constrained_host(params, x[None, :]).astype(np.float64)
    ctx.close()
    x64 = x.astype(np.float64)
    p64 = params.astype(np.float64)
    logit = np.log(x64) - np.log1p(-x64)
    want = -0.5 * ((logit - p64[0]) / p64[1]) ** 2 - np.log(p64[1]) - 0.5 * BR.LOG2PI - np.log(x64 * (1.0 - x64))
    tol = 1e-12 if dtype == np.float64 else 2e-6   # f32: logit in f64 from the f32 point, rounded once, then (u^2) / 2 with u <= 5: a few ulp of |want| <= 10
    assert np.max(np.abs(got - want)) <= tol * np.max(np.abs(want)), (got, want)
    assert np.array_equal(got, got_h)
    qt = avi.TransformedDistribution(avi.MeanFieldGaussian(params[:1], params[1:]), avi.StackedBijector([(0, 1, "truncated", (0.0, 1.0))]))
    assert np.array_equal(avi.logpdf(qt, x[None, :]).cpu().numpy().astype(np.float64), got)
    assert avi.logpdf(qt, x[:1]) == got[0]


# ---- 4. constrained rand / logpdf ------------------------------------------------------------------------------------------------------------
def _strictly_inside(blocks, X):
    for lo, hi, kind, (lb, ub) in BR.normalise(blocks):
        if kind == "truncated" and not (np.all(X[lo:hi] > lb) and np.all(X[lo:hi] < ub)):
            return False
        if kind == "ordered" and not np.all(np.diff(X[lo:hi], axis=0) > 0):
            return False
    return True


def _family_for(kind, rng, d, dtype):
    """(q, context keyword arguments, base) of the families mivi_sample serves"""
    if kind == "lowrank":
        q = avi.LowRankGaussian(0.3 * rng.normal(size=d).astype(dtype), rng.uniform(0.5, 1.0, size=d).astype(dtype), (0.2 * rng.normal(size=(d, 2))).astype(dtype))
        return q, dict(rank=2)
    fam = avi.FULLRANK if kind in ("fullrank", "tdist") else avi.MEANFIELD
    q, _ = make_q(rng, d, fam, dtype)
    if kind in ("laplace", "tdist"):
        q = avi.MvLocationScale(q.location, q.scale, avi.Laplace() if kind == "laplace" else avi.TDist(5.0))
    return q, {}


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("kind", ["meanfield", "fullrank", "lowrank", "laplace", "tdist"])
@pytest.mark.parametrize("shape", [(37, 10), (300, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sample_and_logpdf_constrained(shape, kind, dtype):
    d, M = shape
    rng = np.random.default_rng(21 + d)
    q, kw = _family_for(kind, rng, d, dtype)
    blocks = BR.layout(d)
    params, _ = avi.destructure(q)
    ctx = avi.MiviContext(dtype, q.family, d, M, 0, SEED, **kw)
    ctx.set_base_dist(getattr(q, "dist", None))
    ctx.set_bijector(avi.StackedBijector(blocks))
    idx = 6
    Z = ctx.sample(params, idx, want_eps=False).clone()
    X, eta = ctx.sample_constrained(params, idx, want_eta=True)
    assert torch.equal(eta, Z)   # the draws of mivi_sample at the same index
    Zh, Xh = Z.cpu().numpy(), X.cpu().numpy()
    x64, ladj64 = BR.forward(blocks, Zh.astype(np.float64))
    assert _strictly_inside(blocks, x64)   # (q's scales keep the float64 restatement strictly inside)
    for lo, hi, bk, (lb, ub) in BR.normalise(blocks):   # inside [lb, ub], strictly increasing
        if bk == "truncated":
            assert np.all(Xh[lo:hi] >= lb) and np.all(Xh[lo:hi] <= ub)
        if bk == "ordered":
            assert np.all(np.diff(Xh[lo:hi].astype(np.float64), axis=0) > 0)
    err = np.linalg.norm(Xh.astype(np.float64) - x64)
    if dtype == np.float64:
        assert err <= 1e-13 * np.linalg.norm(x64)   # (each x is a handful of f64 roundings: at most 20 terms of an ordered block summed in another order)
    else:
        yard = np.linalg.norm(BR.forward(blocks, Zh, np.float32)[0].astype(np.float64) - x64)
        print(f"[bijector f32] sample_constrained {kind} d={d}: library {err:.3e}, float32 numpy {yard:.3e}")
        assert err <= F32_FACTOR * yard
    # logpdf of the transformed distribution at its own draws == logpdf(eta) - ladj (float64, tests/logpdf_ref.py); the float32 yardstick
    # goes the same way round in float32 numpy: x = binv(eta) rounded to float32, eta back from it, log q of that
    base, rank = (B.base_of(q.dist) if kind in ("laplace", "tdist") else None), kw.get("rank", 0)
    want = LP.logpdf_cols(params, d, q.family, Zh.astype(np.float64), base, np.float64, rank)[0] - ladj64
    got = ctx.logpdf_constrained(params, X).cpu().numpy().astype(np.float64)
    err = np.max(np.abs(got - want) / np.abs(want))
    if dtype == np.float64:
        print(f"[bijector f64] logpdf_constrained {kind} d={d}: {err:.3e}")
        assert err <= TOL64[0]
    else:
        eta32, ladj32, inside = BR.inverse(blocks, BR.forward(blocks, Zh, np.float32)[0], np.float32)
        assert inside.all()
        yq = np.asarray(LP.logpdf_cols(params, d, q.family, eta32, base, np.float32, rank)[0], dtype=np.float64) - ladj32.astype(np.float64)
        yard = np.max(np.abs(yq - want) / np.abs(want))
        print(f"[bijector f32] logpdf_constrained {kind} d={d}: library {err:.3e}, float32 numpy {yard:.3e}")
        assert err <= F32_FACTOR * yard
    ctx.close()


@pytest.mark.parametrize("kind", ["meanfield", "fullrank", "lowrank"])
def test_logpdf_constrained_past_one_chunk(kind):
    """n past the 16384-column chunk: the parameter-only stage runs once, every chunk is inverted into the same scratch -- bitwise the
    two pieces scored by calls of their own, out-of-support columns on both sides of the boundary included"""
    d, n = 5, 16384 + 37
    rng = np.random.default_rng(41)
    q, kw = _family_for(kind, rng, d, np.float32)
    blocks = BR.layout(d)
    params, _ = avi.destructure(q)
    ctx = avi.MiviContext(np.float32, q.family, d, 4, 0, SEED, **kw)
    ctx.set_bijector(avi.StackedBijector(blocks))
    eta = (0.5 * rng.normal(size=(d, n))).astype(np.float32)
    X = BR.forward(blocks, eta, np.float32)[0]
    X[0, 100] = X[0, 16384 + 5] = 0.0    # below the lower bound 0.25
    whole = ctx.logpdf_constrained(params, X).cpu().numpy()
    parts = np.concatenate([ctx.logpdf_constrained(params, np.ascontiguousarray(X[:, :16384])).cpu().numpy(),
                            ctx.logpdf_constrained(params, np.ascontiguousarray(X[:, 16384:])).cpu().numpy()])
    ctx.close()
    assert np.array_equal(whole, parts)
    assert whole[100] == -np.inf and whole[16384 + 5] == -np.inf and np.isfinite(np.delete(whole, [100, 16384 + 5])).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
def test_out_of_support_and_nan_columns(family, dtype):
    d, M = 300, 33
    rng = np.random.default_rng(31)
    q, _ = make_q(rng, d, family, dtype)
    blocks = BR.layout(d)
    params, _ = avi.destructure(q)
    ctx = avi.MiviContext(dtype, family, d, M, 0, SEED)
    ctx.set_bijector(avi.StackedBijector(blocks))
    X = ctx.sample_constrained(params, 2).cpu().numpy().copy()
    good = ctx.logpdf_constrained(params, X).cpu().numpy()
    assert np.all(np.isfinite(good))
    bad = X.copy()
    bad[0, 1] = 0.25                      # on the lower bound
    bad[2, 3] = 1.75                      # beyond the upper bound of truncated(-inf, 1.5)
    bad[10, 5] = -1.5                     # beyond the lower bound of truncated(-1, 2)
    bad[4, 7], bad[5, 7] = X[5, 7], X[4, 7]   # a decreasing pair in the ordered block [3, 6)
    bad[260, 9] = bad[259, 9]             # a tie across the ordered block that straddles row 256
    bad[7, 11] = np.nan                   # NaN in an ordered block
    bad[25, 13] = np.nan                  # NaN in an uncovered coordinate
    bad[0, 15], bad[30, 15] = -1.0, np.nan   # outside AND NaN: NaN
    got = ctx.logpdf_constrained(params, bad).cpu().numpy()
    ctx.synchronize()                     # no status flag
    for k in range(M):
        if k in (1, 3, 5, 7, 9):
            assert got[k] == -np.inf, (k, got[k])
        elif k in (11, 13, 15):
            assert np.isnan(got[k]), (k, got[k])
        else:
            assert got[k] == good[k], (k, got[k], good[k])
    assert np.array_equal(ctx.logpdf_constrained_host(params, bad), got, equal_nan=True)
    ctx.close()


@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
def test_estimates_are_unchanged_by_a_constrained_logpdf_call(family):
    d, M = 37, 10
    rng = np.random.default_rng(33)
    q, _ = make_q(rng, d, family, np.float32)
    prob, _ = make_problem(rng, "dense", d, np.float32)
    params, _ = avi.destructure(q)
    outs = []
    for call in (False, True):
        ctx = avi.MiviContext(np.float32, family, d, M, 3, SEED)
        ctx.set_problem(transformed(prob, BR.layout(d)))
        pd = ctx.to_device(params)
        res = []
        for idx in (3, 4, 5):
            v, g = ctx.estimate_gradient(pd, idx)
            res += [v.clone(), g.clone()]
            if call:
                X = ctx.sample_constrained(pd, 100 + idx) if idx == 4 else torch.rand(d, 7, device=ctx.tdevice)
                ctx.logpdf_constrained(pd, X)
        ctx.synchronize()
        outs.append([r.cpu().numpy() for r in res[:2] + res[4:]])
        ctx.close()
    # (estimate 4 is followed by mivi_sample, which by its own contract drops the eps speculation: compared are the estimates around it)
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_transformed_distribution_rand_and_logpdf():
    d, n = 37, 10
    rng = np.random.default_rng(35)
    q, _ = make_q(rng, d, avi.FULLRANK, np.float64)
    bij = avi.StackedBijector(BR.layout(d))
    qt = avi.TransformedDistribution(q, bij)
    r1, r2 = avi.PhiloxRNG(SEED), avi.PhiloxRNG(SEED)
    X = avi.rand(r1, qt, n)
    Z = avi.rand(r2, q, n)
    assert tuple(X.shape) == (d, n) and r1.counter == r2.counter == 1
    x64, ladj = BR.forward(bij_blocks(bij), Z.cpu().numpy())
    assert np.linalg.norm(X.cpu().numpy() - x64) <= 1e-13 * np.linalg.norm(x64)
    lq = avi.logpdf(qt, X).cpu().numpy()
    want = avi.logpdf(q, Z).cpu().numpy() - ladj
    err = np.max(np.abs(lq - want) / np.abs(want))
    print(f"[bijector f64] avi.logpdf(TransformedDistribution) d={d}: {err:.3e}")
    assert err <= TOL64[0]


def bij_blocks(bij):
    return [(lo, hi, k, b) if k == "truncated" else (lo, hi, k) for (lo, hi, k), b in zip(bij.blocks, bij.bounds)]


# ---- 5. saturation -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
def test_two_sided_block_saturates_cleanly_in_f32(family):
    """eta = +-40 in f32: x equals a bound, ladj and the gradient stay finite, no status flag"""
    d, M = 4, 10
    loc = np.array([40.0, -40.0, 40.0, 0.1], dtype=np.float32)
    scale = np.full(d, 1e-3, dtype=np.float32)
    q = avi.MeanFieldGaussian(loc, scale) if family == avi.MEANFIELD else avi.FullRankGaussian(loc, np.diag(scale))
    blocks = [(0, 2, "truncated", (-1.0, 2.0)), (2, 3, "truncated", (3.0, 7.0))]
    params, _ = avi.destructure(q)
    ctx = avi.MiviContext(np.float32, family, d, M, 0, SEED)
    ctx.set_problem(transformed(avi.DiagNormalProblem(np.zeros(d, np.float32), np.ones(d, np.float32)), blocks))
    X = ctx.sample_constrained(params, 1).cpu().numpy()
    assert np.all(X[0] == 2.0) and np.all(X[1] == -1.0) and np.all(X[2] == 7.0)
    v, g = ctx.estimate_gradient(params, 1)
    ctx.synchronize()   # raises on a status flag
    assert np.isfinite(float(v.item())) and np.all(np.isfinite(g.cpu().numpy()))
    _, eps = ctx.sample(params, 1)
    ref = BR.estimate_gradient(params.astype(np.float64), d, family, O.DiagNormalTarget(np.zeros(d), np.ones(d)), blocks, eps.cpu().numpy().astype(np.float64), 0)
    assert abs(float(v.item()) - ref["value"]) <= 1e-5 * abs(ref["value"])   # ladj ~ log(3) - 40 per saturated row: finite and right
    ctx.close()


# ---- 6. loops ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
@pytest.mark.parametrize("rule", ["descent", "adam"])
def test_device_loop_honours_the_new_kinds(family, rule):
    """optimize(device_loop=True) == the host-driven step loop, bitwise, over 9 steps with a truncated + ordered bijector
    (tests/test_gpu_bijector.py test_device_loop_honours_the_bijector); the same call twice is bitwise equal."""
    d, T = 12, 9
    rng = np.random.default_rng(11)
    mu, sig = rng.uniform(0.5, 1.5, size=d).astype(np.float32), rng.uniform(1.5, 2.5, size=d).astype(np.float32)
    base = avi.DiagNormalProblem(mu, sig)
    prob = transformed(base, [(0, 3, "truncated", (0.0, 4.0)), (3, 4, "truncated", (0.5, np.inf)), (4, 9, "ordered")])
    q0 = (avi.MeanFieldGaussian(np.zeros(d, np.float32), np.full(d, 0.3, np.float32)) if family == avi.MEANFIELD
          else avi.FullRankGaussian(np.zeros(d, np.float32), 0.3 * np.eye(d, dtype=np.float32)))
    opt = avi.Descent(1e-3) if rule == "descent" else avi.Adam(1e-2)
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), n_samples=8, optimizer=opt, averager=avi.NoAveraging(), operator=avi.ClipScale())
    res = {}
    for name, pr, dev in (("dev", prob, True), ("dev2", prob, True), ("host", prob, False), ("plain", base, True)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, info, st = avi.optimize(avi.PhiloxRNG(5), alg, T, pr, q0, device_loop=dev)
        res[name] = (st["params"].cpu().numpy().copy(), np.array([i["elbo"] for i in info]))
    assert np.array_equal(res["dev"][0], res["host"][0])
    assert np.array_equal(res["dev"][0], res["dev2"][0]) and np.array_equal(res["dev"][1], res["dev2"][1])
    assert np.allclose(res["dev"][1], res["host"][1], rtol=1e-6)
    assert not np.allclose(res["dev"][0], res["plain"][0], rtol=1e-4)   # the bijector changed the problem


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------------------
def test_ex_entry_argument_errors():
    ctx = avi.MiviContext(np.float32, avi.MEANFIELD, 8, 4, 0, SEED)
    ctx.set_problem(avi.DiagNormalProblem(np.zeros(8, np.float32), np.ones(8, np.float32)))
    lib = ctx.lib

    def call_ex(ranges, kinds, bounds):
        r, k = np.array(ranges, dtype=np.int32).reshape(-1), np.array(kinds, dtype=np.int32)
        b = None if bounds is None else np.array(bounds, dtype=np.float64).reshape(-1)
        st = lib.mivi_set_bijector_stacked_ex(ctx.h, len(kinds), r.ctypes.data, k.ctypes.data, None if b is None else b.ctypes.data)
        return st, lib.mivi_last_error(ctx.h).decode()

    for ranges, kinds, bounds, word in (([(0, 2)], [2], [(float("nan"), 1.0)], "NaN"), ([(0, 2)], [2], [(0.0, float("nan"))], "NaN"),
                                        ([(0, 2)], [2], [(1.0, 1.0)], "lb < ub"), ([(0, 2)], [2], [(2.0, 1.0)], "lb < ub"),
                                        ([(0, 2)], [4], [(0.0, 1.0)], "kind"), ([(0, 2)], [-1], None, "kind"), ([(0, 2)], [2], None, "bounds"),
                                        ([(0, 9)], [3], None, "range"), ([(0, 4), (3, 6)], [3, 2], [(0, 0), (0.0, 1.0)], "overlap")):
        st, msg = call_ex(ranges, kinds, bounds)
        assert st == _lib.ERR_BAD_ARG and word in msg, (ranges, kinds, bounds, st, msg)
    assert call_ex([(0, 2), (2, 5)], [2, 3], [(0.0, 1.0), (0, 0)])[0] == _lib.MIVI_OK
    assert call_ex([(0, 2), (2, 5)], [1, 3], None)[0] == _lib.MIVI_OK   # bounds may be NULL when no block is truncated
    # the old entry keeps its kinds and its message
    r, k = np.array([0, 2], dtype=np.int32), np.array([2], dtype=np.int32)
    assert lib.mivi_set_bijector_stacked(ctx.h, 1, r.ctypes.data, k.ctypes.data) == _lib.ERR_BAD_ARG
    assert lib.mivi_last_error(ctx.h).decode() == "stacked bijector: kind must be 0 (identity) or 1 (exp)"
    with pytest.raises(avi.MiviError):
        ctx.set_bijector(avi.StackedBijector([(0, 9, "ordered")]))
    ctx.close()
