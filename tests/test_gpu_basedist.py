"""GPU tests of the non-normal base distributions of MvLocationScale (mivi_set_base_dist: Laplace(), TDist(nu); docs/src/families.md:59-101):
libmivi through the C ABI against the float64 restatement of tests/basedist_ref.py on the reference streams.

Tolerances.  f64 contexts: TOL64 of tests/measure_space_cases.py (values relative 1e-12, vectors relative l2 1e-11; draws and samples 1e-12).
f32 contexts: the project's f32 yardstick -- the error against the float64 reference is at most F32_FACTOR (= 8) times the error of the
float32 numpy evaluation of the same formulas, floored at 2^-24 |ref| (basedist_ref.ratio), whole and per parameter block.  Every draw is
also held to a per-element absolute bound, F32_FACTOR unit roundoffs times the first-order error scale of its own evaluation
(basedist_ref.draw_scale), so that the heavy-tailed elements cannot mask the bulk."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest
import torch
from scipy import stats

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import _lib
from oracle import oracle as O
from tests import basedist_ref as B
from tests.helpers import SEED, OraclePlugin, make_family, make_problem, rel_err
from tests.measure_space_cases import F32_FACTOR, TOL64

pytestmark = pytest.mark.gpu

ENTROPIES = [avi.ClosedFormEntropy(), avi.ClosedFormEntropyZeroGradient(), avi.MonteCarloEntropy(),
             avi.StickingTheLandingEntropy(), avi.StickingTheLandingEntropyZeroGradient()]
# partial Philox blocks in both layouts (d % 4, d odd), M below and across the solve's 8- and 16-column groups, d across the 16-, 32- and
# 64-row tiles and the dP padding
SHAPES = [(1, 1), (7, 5), (10, 1), (33, 10), (67, 33), (130, 70), (256, 128)]
BASES = [avi.Laplace(), avi.TDist(3.0), avi.TDist(5.5)]
FAMILIES = [avi.MEANFIELD, avi.FULLRANK]
DTYPES = [np.float32, np.float64]
shape_id = lambda s: "x".join(map(str, s))   # noqa: E731
fam_id = lambda f: "mf" if f == avi.MEANFIELD else "fr"   # noqa: E731
dt_id = lambda t: np.dtype(t).name   # noqa: E731
UNIT = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}


def make_q(rng, d, family, dtype, dist):
    q, _ = make_family(rng, d, family, dtype)
    return avi.MvLocationScale(q.location, q.scale, dist)


def make_ctx(d, M, family, dtype, dist, ent=None, prob=None, **kw):
    ctx = avi.MiviContext(dtype, family, d, M, (ent or avi.ClosedFormEntropy()).code, SEED, **kw)
    ctx.set_base_dist(dist)
    if prob is not None:
        ctx.set_problem(prob)
    return ctx


def ref_draws(dist, idx, d, M, dtype, lo=0):
    """(float64 evaluation, evaluation in dtype, per-element error scale) of the stream of a context of this dtype"""
    f64 = dtype == np.float64
    base = B.base_of(dist)
    return (B.draws(base, SEED, idx, d, lo, lo + M, f64=f64), B.draws(base, SEED, idx, d, lo, lo + M, f64=f64, dtype=dtype),
            B.draw_scale(base, SEED, idx, d, lo, lo + M, f64=f64))


def hold(what, got, yard, ref, dtype, tol64):
    """the f64 criterion (relative l2, scale at least 1 for vectors) or the f32 yardstick"""
    if dtype == np.float64:
        err = np.linalg.norm(np.asarray(got, dtype=np.float64) - ref) / max(np.linalg.norm(ref), 1e-300)
        print(f"[basedist f64] {what}: {err:.3e}")
        assert err <= tol64, (what, err)
    else:
        r = B.ratio(got, yard, ref)
        print(f"[basedist f32 ratio] {what}: {r:.2f}")
        assert np.all(np.isfinite(got)) and r <= F32_FACTOR, (what, r)


# ---- draws and samples -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
@pytest.mark.parametrize("dist", BASES, ids=repr)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_draws_and_samples_are_the_reference_stream(shape, dist, family, dtype):
    d, M = shape
    idx = 3
    q = make_q(np.random.default_rng(100 + d + M), d, family, dtype, dist)
    params, _ = avi.destructure(q)
    ctx = make_ctx(d, M, family, dtype, dist)
    Z, eps = ctx.sample(params, idx)
    Z, eps = Z.cpu().numpy().astype(np.float64), eps.cpu().numpy().astype(np.float64)
    ctx.close()
    assert eps.shape == (d, M) and Z.shape == (d, M)
    U64, Ud, scale = ref_draws(dist, idx, d, M, dtype)
    what = f"{shape} {dist!r} {fam_id(family)}"
    hold(what + " eps", eps, Ud, U64, dtype, TOL64[0])
    elem = np.abs(eps - U64) / np.maximum(scale, 1e-300)
    print(f"[basedist draws] {what}: worst element {elem.max() / UNIT[dtype]:.2f} unit roundoffs of its scale")
    per_unit = F32_FACTOR * UNIT[dtype] if dtype == np.float32 else TOL64[0]
    assert np.all(np.abs(eps - U64) <= per_unit * scale + 1e-300), what
    m, S = B.split(params.astype(np.float64), d, family)
    Z64 = (S[:, None] * U64 if family == avi.MEANFIELD else S @ U64) + m[:, None]
    md, Sd = B.split(params, d, family)
    Zd = (Sd[:, None] * Ud if family == avi.MEANFIELD else Sd @ Ud) + md[:, None]
    hold(what + " Z", Z, Zd, Z64, dtype, TOL64[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("dist", BASES + [avi.TDist(1.0)], ids=repr)
def test_device_draws_have_the_law(dist, dtype):
    """one call at d = 64, M = 2048: the Kolmogorov-Smirnov condition of tests/test_basedist_ref_host.py"""
    d, M = 64, 2048
    ctx = make_ctx(d, M, avi.MEANFIELD, dtype, dist)
    _, eps = ctx.sample(np.concatenate([np.zeros(d), np.ones(d)]).astype(dtype), 11)
    eps = eps.cpu().numpy().astype(np.float64)
    ctx.close()
    sp = stats.laplace if dist.code == 1 else stats.t(dist.nu)
    p = stats.kstest(eps.ravel(), sp.cdf).pvalue
    print(f"[basedist ks device] {dist!r} {dt_id(dtype)}: p = {p:.4f}")
    assert np.all(np.isfinite(eps)) and p > 1e-3


def test_rand_is_the_sample_entry():
    d, n = 10, 7
    for dist in (avi.Laplace(), avi.TDist(3.0)):
        q = make_q(np.random.default_rng(4), d, avi.FULLRANK, np.float64, dist)
        rng = avi.PhiloxRNG(SEED)
        idx = rng.counter
        Z = avi.rand(rng, q, n)
        assert tuple(Z.shape) == (d, n) and rng.counter == idx + 1
        ctx = make_ctx(d, n, avi.FULLRANK, np.float64, dist)
        assert torch.equal(Z, ctx.sample(avi.destructure(q)[0], idx, want_eps=False))
        ctx.close()


# ---- parity ----------------------------------------------------------------------------------------------------------------------------
_REF = {}


def reference(key, params, d, family, tgt, dist, idx, M, kind, dtype):
    """(float64 reference, restatement in dtype): computed once per case, shared and never modified"""
    if key not in _REF:
        U64, Ud, _ = ref_draws(dist, idx, d, M, dtype)
        base = B.base_of(dist)
        ref = B.estimate_gradient(params.astype(np.float64), d, family, tgt, U64, kind, base)
        yard = ref if dtype == np.float64 else B.estimate_gradient(params, d, family, tgt, Ud, kind, base, dtype=dtype)
        _REF[key] = (ref, yard)
    return _REF[key]


def run_case(d, M, family, dtype, dist, kind, ents=ENTROPIES, plugin=False, bijector=False, idx=5):
    rng = np.random.default_rng(4321 + d + 7 * M)
    q = make_q(rng, d, family, dtype, dist)
    prob, tgt = make_problem(rng, kind, d, dtype)
    if plugin:
        prob = OraclePlugin(tgt)
    if bijector:   # Stacked([exp on the first three coordinates, identity on the rest]) around the target
        blocks = [(0, 3, "exp"), (3, d, "identity")]
        prob, tgt = avi.TransformedProblem(prob, avi.StackedBijector(blocks)), O.StackedBijectorTarget(tgt, blocks)
    params, _ = avi.destructure(q)
    for ent in ents:
        ctx = make_ctx(d, M, family, dtype, dist, ent, prob)
        assert ctx.params_len == params.size
        value, grad = ctx.estimate_gradient_host(params, idx)
        ctx.close()
        value, grad = float(value), np.asarray(grad, dtype=np.float64)
        key = (d, M, family, np.dtype(dtype).name, repr(dist), kind, plugin, bijector, ent.code, idx)
        ref, yard = reference(key, params, d, family, tgt, dist, idx, M, ent.code, dtype)
        what = f"{key}"
        assert np.isfinite(value) and np.all(np.isfinite(grad)), what
        if dtype == np.float64:
            v_err, g_err = abs(value - ref["value"]), np.linalg.norm(grad - ref["grad"])
            print(f"[basedist f64] {what}: value {v_err / abs(ref['value']):.3e}, grad {g_err / max(np.linalg.norm(ref['grad']), 1.0):.3e}")
            assert v_err <= TOL64[0] * abs(ref["value"]), (what, value, ref["value"])
            assert g_err <= TOL64[1] * max(np.linalg.norm(ref["grad"]), 1.0), what
        else:
            rv = B.ratio([value], [yard["value"]], [ref["value"]])
            rg = B.ratio(grad, yard["grad"], ref["grad"])
            rl = B.ratio(grad[:d], yard["grad"][:d], ref["grad"][:d])
            rs = B.ratio(grad[d:], yard["grad"][d:], ref["grad"][d:])
            print(f"[basedist f32 ratio] {what}: value {rv:.2f}, grad {rg:.2f}, location {rl:.2f}, scale {rs:.2f}")
            assert rv <= F32_FACTOR and rg <= F32_FACTOR and rl <= F32_FACTOR and rs <= F32_FACTOR, (what, rv, rg, rl, rs)
        if family == avi.FULLRANK:   # the strict upper triangle of dC is exactly zero
            assert not np.any(np.triu(grad[d:].reshape(d, d, order="F"), 1))


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
@pytest.mark.parametrize("dist", BASES, ids=repr)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_diag_target_all_estimators_all_shapes(shape, dist, family, dtype):
    run_case(*shape, family, dtype, dist, "diag")


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
@pytest.mark.parametrize("dist", BASES, ids=repr)
@pytest.mark.parametrize("kind,plugin,bijector", [("dense", False, False), ("dense", True, False), ("funnel", False, False), ("dense", False, True)],
                         ids=["dense", "plugin", "funnel", "stacked"])
def test_targets_all_estimators(kind, plugin, bijector, dist, family, dtype):
    run_case(67, 33, family, dtype, dist, kind, plugin=plugin, bijector=bijector)


# ---- estimate_objective ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
@pytest.mark.parametrize("dist", BASES, ids=repr)
def test_estimate_objective_any_n_samples_every_entropy(dist, family, dtype):
    """any n_samples -- below n_mc, a non-multiple of it, across the 16384-sample chunk -- is the value on the concatenated draws"""
    d, n_mc, idx = 10, 16, 2
    rng = np.random.default_rng(8)
    q = make_q(rng, d, family, dtype, dist)
    prob, tgt = make_problem(rng, "diag", d, dtype)
    params, _ = avi.destructure(q)
    base = B.base_of(dist)
    ctx = make_ctx(d, n_mc, family, dtype, dist, prob=prob)
    for n in (5, 40, 16384 + 37):
        U64, Ud, _ = ref_draws(dist, idx, d, n, dtype)
        for closed in (True, False):
            kind = B.CLOSED_FORM if closed else B.MONTE_CARLO
            want = B.estimate_gradient(params.astype(np.float64), d, family, tgt, U64, kind, base)["value"]
            yard = want if dtype == np.float64 else B.estimate_gradient(params, d, family, tgt, Ud, kind, base, dtype=dtype)["value"]
            for ent in [e for e in ENTROPIES if (e.code < 2) == closed]:   # the estimators share their VALUE within the two groups
                got = float(ctx.estimate_objective(params, idx, n_samples=n, entropy=ent.code).item())
                hold(f"objective n={n} {ent!r} {dist!r}", [got], [yard], np.array([want]), dtype, TOL64[0])
                if n == 40:
                    got_h = float(ctx.estimate_objective_host(params, idx, n_samples=n, entropy=ent.code))
                    hold(f"objective_host n={n} {ent!r}", [got_h], [yard], np.array([want]), dtype, TOL64[0])
    ctx.close()


# ---- known answer ----------------------------------------------------------------------------------------------------------------------
class LogQPlugin:
    """A plugin target whose log density is log q itself (location_scale.jl:59-63), in float64 on the host at the columns the device sends."""

    def __init__(self, params, d, family, base):
        self.m, self.S = B.split(np.asarray(params, dtype=np.float64), d, family)
        self.mf, self.base, self.d = family == avi.MEANFIELD, base, d
        self.logdet = float(np.sum(np.log(self.S if self.mf else np.diag(self.S))))
        self.seen = []

    def dimension(self):
        return self.d

    def logdensity_and_gradient_batch(self, Z):
        R = np.asarray(Z, dtype=np.float64) - self.m[:, None]
        Us = R / self.S[:, None] if self.mf else np.linalg.solve(self.S, R)
        ell = np.sum(B.logphi(self.base, Us), axis=0) - self.logdet
        P = B.psi(self.base, Us)
        self.seen.append(ell.copy())
        return ell, (P / self.S[:, None] if self.mf else np.linalg.solve(self.S.T, P))


@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
@pytest.mark.parametrize("dist", BASES, ids=repr)
def test_objective_of_q_against_itself_is_zero(dist, family):
    """pi = q: the Monte-Carlo objective is zero to rounding, the closed-form one within 4 standard errors at 10^5 samples -- pins lgamma,
    H(phi) and the signs."""
    d, n = 5, 10 ** 5
    q = make_q(np.random.default_rng(31), d, family, np.float64, dist)
    params, _ = avi.destructure(q)
    plug = LogQPlugin(params, d, family, B.base_of(dist))
    ctx = make_ctx(d, 4096, family, np.float64, dist, prob=plug)
    v_mc = float(ctx.estimate_objective(params, 1, n_samples=n, entropy=avi.MonteCarloEntropy.code).item())
    ell = np.concatenate(plug.seen)
    assert ell.size == n
    print(f"[basedist known answer] {dist!r} {fam_id(family)}: MC {v_mc:.3e} of mean |log q| {np.mean(np.abs(ell)):.3f}")
    assert abs(v_mc) <= TOL64[0] * np.mean(np.abs(ell))
    v_cf = float(ctx.estimate_objective(params, 1, n_samples=n, entropy=avi.ClosedFormEntropy.code).item())
    se = np.std(ell) / math.sqrt(n)
    print(f"[basedist known answer] closed form {v_cf:.3e}, standard error {se:.3e}")
    assert abs(v_cf) <= 4.0 * se
    # and the gradient of KL(q || q) estimated with sticking the landing is exactly zero sample by sample: W = G + C^-T (-psi) = 0
    stl = make_ctx(d, 64, family, np.float64, dist, avi.StickingTheLandingEntropy(), plug)
    _, g = stl.estimate_gradient_host(params, 2)
    assert np.linalg.norm(g) <= 1e-11 * math.sqrt(g.size)
    stl.close()
    ctx.close()


# ---- batched entries -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
@pytest.mark.parametrize("shape", [(33, 10), (64, 64), (128, 128)], ids=shape_id)   # ragged; the LDS / lane-batched route's; the batch engine's
def test_batched_entries_equal_single_calls_bitwise(shape, family, dtype):
    d, M = shape
    n = 3
    rng = np.random.default_rng(5)
    for dist, ent in ((avi.Laplace(), avi.StickingTheLandingEntropy()), (avi.TDist(3.0), avi.ClosedFormEntropy())):
        q = make_q(rng, d, family, dtype, dist)
        prob, _ = make_problem(rng, "diag", d, dtype)
        params, _ = avi.destructure(q)
        ctx = make_ctx(d, M, family, dtype, dist, ent, prob)
        p = ctx.to_device(params)
        singles = [ctx.estimate_gradient(p, 7 + i) for i in range(n)]
        singles = [(v.clone(), g.clone()) for v, g in singles]
        values, grads = ctx.estimate_gradient_each(p, 7, n)
        v_last, g_last = ctx.empty(1), ctx.empty(ctx.params_len)
        ctx.estimate_gradient_n(p, 7, n, v_last, g_last)
        ctx.synchronize()
        for i, (v, g) in enumerate(singles):
            assert torch.equal(values[i:i + 1], v) and torch.equal(grads[i], g)
        assert torch.equal(v_last, singles[-1][0]) and torch.equal(g_last, singles[-1][1])
        assert not torch.equal(singles[0][1], singles[1][1])
        ctx.close()


# ---- optimisation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
@pytest.mark.parametrize("opt", [avi.Descent(1e-3), avi.Adam(0.01), avi.COCOB(), avi.DoG(), avi.DoWG()], ids=lambda o: type(o).__name__)
@pytest.mark.parametrize("averager", [avi.NoAveraging(), avi.PolynomialAveraging()], ids=lambda a: type(a).__name__)
def test_device_loop_equals_host_loop(averager, opt, family):
    """mivi_optimize_loop (the graph of launches: the only route of a non-normal base) against the host-driven `step` loop, bitwise:
    d = 10, one sample per step, 20 steps"""
    d, T = 10, 20
    prob, _ = make_problem(np.random.default_rng(21), "dense", d)
    prox_ok = isinstance(opt, (avi.Descent, avi.DoG))   # (DoWG is a DoG)
    for dtype in DTYPES:
        pr = avi.DenseNormalProblem(prob.mean.astype(dtype), prob.L.astype(dtype))
        for dist, ent, op in ((avi.Laplace(), avi.ClosedFormEntropy(), "clip"), (avi.TDist(3.0), avi.StickingTheLandingEntropy(), "clip"),
                              (avi.TDist(5.5), None, "prox")):
            if op == "prox" and not prox_ok:
                continue
            q0 = avi.MvLocationScale(np.zeros(d, dtype), np.ones(d, dtype) if family == avi.MEANFIELD else np.eye(d, dtype=dtype), dist)
            if op == "prox":
                alg = avi.KLMinRepGradProxDescent(avi.AutoMIVI(), optimizer=opt, n_samples=1, averager=averager)
            else:
                alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), entropy=ent, optimizer=opt, n_samples=1, averager=averager, operator=avi.ClipScale())
            q_dev, info_dev, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, T, pr, q0)
            q_host, info_host, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, T, pr, q0, device_loop=False)
            assert q_dev.dist == dist and q_host.dist == dist
            a, b = avi.destructure(q_dev)[0], avi.destructure(q_host)[0]
            what = (type(opt).__name__, type(averager).__name__, fam_id(family), dt_id(dtype), repr(dist), op)
            assert np.all(np.isfinite(a)) and not np.array_equal(a, avi.destructure(q0)[0]), what
            assert np.array_equal(a, b), (what, rel_err(a, b))
            assert [i["elbo"] for i in info_dev] == [i["elbo"] for i in info_host], what


def test_fullrank_tdist_fit_to_the_funnel_raises_the_elbo():
    """The textbook use of a heavy-tailed family: FullRank TDist(3) on Neal's funnel, 300 Adam steps raise the ELBO estimate.
    (The funnel's first coordinate is a log scale, and E exp(-2 eta_1) is infinite under any Student-t: the estimates are dominated by
    their tail draws -- 2.1e13 before and 7.5e3 after on the fixed streams used here -- so only the direction is asserted.)"""
    d = 10
    prob = avi.FunnelProblem(d, 1.5)
    q0 = avi.MvLocationScale(np.zeros(d), np.eye(d), avi.TDist(3.0))
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), optimizer=avi.Adam(0.01), n_samples=8, averager=avi.NoAveraging(), operator=avi.ClipScale())
    before = avi.estimate_objective(avi.PhiloxRNG(SEED), alg, q0, prob, n_samples=4096)
    q, info, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 300, prob, q0)
    assert isinstance(q, avi.MvLocationScale) and q.dist == avi.TDist(3.0) and len(info) == 300
    after = avi.estimate_objective(avi.PhiloxRNG(SEED), alg, q, prob, n_samples=4096)
    print(f"[basedist funnel] negative ELBO {before:.3f} -> {after:.3f}")
    assert np.isfinite(after) and after < before, (before, after)


# ---- guards ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 64), (10, 4), (128, 128)], ids=shape_id)   # the LDS route's shape; a small one; the batch engine's
@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
def test_normal_base_changes_nothing_bitwise(family, shape):
    d, M = shape
    dtype = np.float32
    rng = np.random.default_rng(9)
    q, _ = make_family(rng, d, family, dtype)
    prob, _ = make_problem(rng, "diag", d, dtype)
    params, _ = avi.destructure(q)
    outs = []
    for mode in ("never", "normal", "laplace-then-normal"):
        for ent in (avi.ClosedFormEntropy(), avi.StickingTheLandingEntropy()):
            ctx = avi.MiviContext(dtype, family, d, M, ent.code, SEED)
            ctx.set_problem(prob)
            if mode == "laplace-then-normal":
                ctx.set_base_dist(avi.Laplace())
                ctx.estimate_gradient(params, 0)
            if mode != "never":
                ctx.set_base_dist(avi.Normal())
            p = ctx.to_device(params)
            v1, g1 = ctx.estimate_gradient(p, 4)
            v2, g2 = ctx.estimate_gradient(p, 5)      # (the call the eps speculation serves)
            vals, grads = ctx.estimate_gradient_each(p, 4, 8)
            vn, gn = ctx.empty(1), ctx.empty(ctx.params_len)
            ctx.estimate_gradient_n(p, 4, 8, vn, gn)
            vo = ctx.estimate_objective(p, 4, n_samples=8 * M, entropy=ent.code)
            ctx.synchronize()
            outs.append([t.clone() for t in (v1, g1, v2, g2, vals, grads, vn, gn, vo)])
            ctx.close()
    for k in (2, 3, 4, 5):
        for a, b in zip(outs[k % 2], outs[k]):
            assert torch.equal(a, b), (k, fam_id(family), shape)


def test_unsupported_entries_refuse_the_base():
    """Every entry outside the surface returns MIVI_ERR_UNSUPPORTED (6) with a message naming the entry and the base, before reading a buffer."""
    d, M = 8, 4
    for family in FAMILIES:
        for dist, name in ((avi.Laplace(), "Laplace"), (avi.TDist(3.0), "TDist")):
            ctx = make_ctx(d, M, family, np.float32, dist, prob=avi.DiagNormalProblem(np.zeros(d, np.float32), np.ones(d, np.float32)))
            lib, h = ctx.lib, ctx.h
            buf = ctx.empty(4 * (d * d + d * M) + 64)
            host = np.zeros(4 * (d * d + d * M) + 64, dtype=np.float32)
            P, Hp = ctx._p(buf), host.ctypes.data
            dbl = (C.c_double * 8)()
            calls = {
                "mivi_estimate_score_gradient": lambda: lib.mivi_estimate_score_gradient(h, P, 0, P, P, P),
                "mivi_estimate_score_gradient_host": lambda: lib.mivi_estimate_score_gradient_host(h, Hp, 0, Hp, Hp, Hp),
                "mivi_gauss_expected_grad_hess": lambda: lib.mivi_gauss_expected_grad_hess(h, P, 0, 0, P, P, P),
                "mivi_gauss_expected_grad_hess_host": lambda: lib.mivi_gauss_expected_grad_hess_host(h, Hp, 0, 0, Hp, Hp, Hp),
                "mivi_gauss_expected_grad_hess2": lambda: lib.mivi_gauss_expected_grad_hess2(h, P, 0, 0, P, P, P),
                "mivi_gauss_expected_grad_hess2_host": lambda: lib.mivi_gauss_expected_grad_hess2_host(h, Hp, 0, 0, Hp, Hp, Hp),
                "mivi_sqrt_ngd_update": lambda: lib.mivi_sqrt_ngd_update(h, P, P, P, 0.1, P),
                "mivi_sqrt_ngd_update_host": lambda: lib.mivi_sqrt_ngd_update_host(h, Hp, Hp, Hp, 0.1, Hp),
                "mivi_sqrt_ngd_steps": lambda: lib.mivi_sqrt_ngd_steps(h, P, 0, 1, 0, 0, 0.1, P),
                "mivi_natgrad_init": lambda: lib.mivi_natgrad_init(h, P, P),
                "mivi_natgrad_update": lambda: lib.mivi_natgrad_update(h, P, P, P, P, 0.1, 1, P),
                "mivi_natgrad_update_host": lambda: lib.mivi_natgrad_update_host(h, Hp, Hp, Hp, Hp, 0.1, 1, Hp),
                "mivi_natgrad_steps": lambda: lib.mivi_natgrad_steps(h, P, P, 0, 1, 0, 0, 0.1, 1, P),
                "mivi_bam_init": lambda: lib.mivi_bam_init(h, P, P),
                "mivi_bam_moments": lambda: lib.mivi_bam_moments(h, P, 0, 4, P, P, P, P, P),
                "mivi_bam_moments_host": lambda: lib.mivi_bam_moments_host(h, Hp, 0, 4, Hp, Hp, Hp, Hp, Hp),
                "mivi_estimate_fisher": lambda: lib.mivi_estimate_fisher(h, P, 0, 4, P),
                "mivi_estimate_fisher_host": lambda: lib.mivi_estimate_fisher_host(h, Hp, 0, 4, Hp),
                "mivi_bam_update": lambda: lib.mivi_bam_update(h, P, P, P, P, 4, 1.0, P),
                "mivi_bam_update_host": lambda: lib.mivi_bam_update_host(h, Hp, Hp, Hp, Hp, 4, 1.0, Hp),
                "mivi_bam_steps": lambda: lib.mivi_bam_steps(h, P, P, 0, 1, 1, 4, P, P),
                "mivi_wass_init": lambda: lib.mivi_wass_init(h, P, P),
                "mivi_wass_update": lambda: lib.mivi_wass_update(h, P, P, P, P, 0.1, P),
                "mivi_wass_update_host": lambda: lib.mivi_wass_update_host(h, Hp, Hp, Hp, Hp, 0.1, Hp),
                "mivi_wass_steps": lambda: lib.mivi_wass_steps(h, P, P, 0, 1, 0, 0, 0.1, P),
                "mivi_estimate_partials": lambda: lib.mivi_estimate_partials(h, P, 0, P),
                "mivi_finalize": lambda: lib.mivi_finalize(h, P, P, P, P),
                "mivi_finalize_slice": lambda: lib.mivi_finalize_slice(h, P, P, 0, 1, P),
                "mivi_unpack_final": lambda: lib.mivi_unpack_final(h, P, P, P),
                "mivi_estimate_gradient_dist": lambda: lib.mivi_estimate_gradient_dist(h, P, 0, P, P),
                "mivi_estimate_gradient_dist_n": lambda: lib.mivi_estimate_gradient_dist_n(h, P, 0, 2, P, P),
                "mivi_comm_init": lambda: lib.mivi_comm_init(h, Hp, 0, 1),
                "mivi_comm_enable_p2p": lambda: lib.mivi_comm_enable_p2p(h),
                "mivi_p2p_export": lambda: lib.mivi_p2p_export(h, 0, 1, Hp),
                "mivi_p2p_attach": lambda: lib.mivi_p2p_attach(h, Hp),
                "mivi_p2p_selfcheck": lambda: lib.mivi_p2p_selfcheck(h, P, 0, dbl),
                "mivi_p2p_exchange": lambda: lib.mivi_p2p_exchange(h, P, P, P, P, 7),
                "mivi_p2p_partials_direct": lambda: lib.mivi_p2p_partials_direct(h, P, 0),
                "mivi_profile_dist": lambda: lib.mivi_profile_dist(h, P, 1, dbl),
                "mivi_profile_batch": lambda: lib.mivi_profile_batch(h, P, 1, 1, dbl),
                "mivi_profile_kernel": lambda: lib.mivi_profile_kernel(h, 0, P, 1, dbl),
            }
            for entry, call in calls.items():
                assert call() == _lib.ERR_UNSUPPORTED, (entry, fam_id(family))
                msg = lib.mivi_last_error(h).decode()
                assert name in msg and entry.replace("_host", "") in msg, (entry, msg)
            # what stays supported: the proximal operator and the update entries read no draws
            assert lib.mivi_prox_scale_entropy(h, P, 0.0, None, 0) == 0 and lib.mivi_clip_scale(h, P, 1e-5) == 0
            ctx.close()


def test_lowrank_and_sharded_contexts_refuse_a_non_normal_base():
    low = avi.MiviContext(np.float32, avi.LOWRANK, 8, 4, 0, SEED, rank=2)
    shard = avi.MiviContext(np.float32, avi.MEANFIELD, 8, 4, 0, SEED, m_offset=4, m_total=8)
    shard0 = avi.MiviContext(np.float32, avi.FULLRANK, 8, 4, 0, SEED, m_total=8)
    for ctx in (low, shard, shard0):
        for dist in (avi.Laplace(), avi.TDist(3.0)):
            with pytest.raises(avi.MiviError) as e:
                ctx.set_base_dist(dist)
            assert e.value.status == _lib.ERR_UNSUPPORTED
        ctx.set_base_dist(avi.Normal())   # the normal base is a no-op everywhere
        ctx.close()
    whole = avi.MiviContext(np.float32, avi.MEANFIELD, 8, 4, 0, SEED, m_total=4)   # m_total = n_mc: not sharded
    whole.set_base_dist(avi.Laplace())
    whole.close()
    q = avi.MvLocationScaleLowRank(np.zeros(4), np.ones(4), np.zeros((4, 2)))
    assert not hasattr(q, "dist")


def test_bad_arguments_are_status_1():
    ctx = avi.MiviContext(np.float64, avi.MEANFIELD, 4, 2, 0, SEED)
    lib, h = ctx.lib, ctx.h
    for nu in (0.0, -1.0, math.inf, math.nan):
        assert lib.mivi_set_base_dist(h, _lib.BASE_TDIST, nu) == _lib.ERR_BAD_ARG, nu
    assert lib.mivi_set_base_dist(h, 3, 1.0) == _lib.ERR_BAD_ARG and lib.mivi_set_base_dist(h, -1, 1.0) == _lib.ERR_BAD_ARG
    assert lib.mivi_set_base_dist(None, 1, 0.0) == _lib.ERR_BAD_ARG
    assert lib.mivi_set_base_dist(h, _lib.BASE_LAPLACE, math.nan) == 0   # nu is read for TDist only
    assert lib.mivi_set_base_dist(h, _lib.BASE_TDIST, 0.25) == 0        # any positive real
    ctx.close()


@pytest.mark.parametrize("family", FAMILIES, ids=fam_id)
def test_nonpositive_scale_diagonal_is_status_3(family):
    d = 6
    q = make_q(np.random.default_rng(2), d, family, np.float64, avi.TDist(3.0))
    params, _ = avi.destructure(q)
    params[d + 2 if family == avi.MEANFIELD else d + 2 * d + 2] = -0.1
    for ent in (avi.ClosedFormEntropy(), avi.StickingTheLandingEntropy()):
        ctx = make_ctx(d, 4, family, np.float64, q.dist, ent, avi.DiagNormalProblem(np.zeros(d), np.ones(d)))
        ctx.estimate_gradient(params, 0)
        with pytest.raises(avi.MiviError) as e:
            ctx.synchronize()
        assert e.value.status == _lib.ERR_NONPOSITIVE_SCALE
        with pytest.raises(avi.MiviError) as e:
            ctx.estimate_gradient_host(params, 0)
        assert e.value.status == _lib.ERR_NONPOSITIVE_SCALE
        with pytest.raises(avi.MiviError) as e:
            ctx.estimate_objective_host(params, 0, n_samples=9)
        assert e.value.status == _lib.ERR_NONPOSITIVE_SCALE
        ctx.close()


def test_the_python_objectives_pass_the_base():
    """estimate_objective / init / the subsampled objective hand q.dist to the context: pi = q gives zero with the right base only."""
    d = 4
    q = make_q(np.random.default_rng(3), d, avi.FULLRANK, np.float64, avi.Laplace())
    params, _ = avi.destructure(q)
    plug = LogQPlugin(params, d, avi.FULLRANK, B.LAPLACE)
    v = avi.estimate_objective(avi.PhiloxRNG(SEED), avi.RepGradELBO(64, entropy=avi.MonteCarloEntropy()), q, plug)
    assert abs(v) <= 1e-12 * np.mean(np.abs(np.concatenate(plug.seen)))
    v_wrong = avi.estimate_objective(avi.PhiloxRNG(SEED), avi.RepGradELBO(64, entropy=avi.MonteCarloEntropy()),
                                     avi.MvLocationScale(q.location, q.scale), plug)
    assert abs(v_wrong) > 1e-3
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = avi.init(avi.PhiloxRNG(SEED), avi.RepGradELBO(8), avi.AutoMIVI(), q, avi.DiagNormalProblem(np.zeros(d), np.ones(d)), params, None)
    lib, h = st.obj_ad_prep.lib, st.obj_ad_prep.h
    buf = st.obj_ad_prep.empty(64)
    P = st.obj_ad_prep._p(buf)
    assert lib.mivi_estimate_partials(h, P, 0, P) == _lib.ERR_UNSUPPORTED and "Laplace" in lib.mivi_last_error(h).decode()
    st.obj_ad_prep.close()
