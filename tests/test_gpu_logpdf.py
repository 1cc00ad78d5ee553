"""mivi_logpdf -- Distributions.logpdf(q, z) at the caller's points, every family and base -- against tests/logpdf_ref.py.

Points of a case are the context's own z = C u + mu (ctx.sample), so the standardised values are O(1) and the solve's error shows; a
second set adds 3 N(0, 1) to them, so that the standardised values of an ill-conditioned C are large.

f32 criterion of the full-rank solve (tests/test_gpu_solve_yardstick.py's): ref64 = logpdf_ref.logpdf_cols in float64 on the f32-stored
parameters and points, yard32 the same in float32 (LAPACK substitution, float32 sums).  The standardised points by
solve_ref.block_ratios, whole and worst 64-row block, and log q as an n-vector by logpdf_ref.logq_ratio: each at most F32_FACTOR = 8.
tests/test_logpdf_ref_host.py shows the factor admissible (<= 4.0 for a float32 emulation of the documented algorithm) and with teeth.
Everything else: f32 values to VALUE_RTOL = 1e-5 of max(|ref64|, d) (log q is a sum of d O(1) terms), f64 to 1e-11 relative l2
(tests/test_gpu_parity.py TOL[np.float64]).

Worst ratios measured on the MI355X (std whole, std worst block, log q), per route of k_lp_fwd16 (csrc/kernels_logpdf.hip):
    X in LDS (d <= 1056)        1.45, 1.45, 1.55   (spd4 64 x 32, the perturbed set)
    X in the f64 scratch        0.27, 0.46, 0.53   (default 2400 x 32)
    own draws (std against eps) 0.61, 0.74         (default / ar999 256 x 64)
The bases' worst value: TDist(0.7), full-rank f32, 256 x 64 -- a column with one standardised value of 5.7e5 -- 7.3e-6 of max(|log q|, d)
against the 1e-5 allowed (LAPACK's float32 substitution on the same points: 4.3e-5).
What the log q assertion of the yardstick can detect is what tests/test_logpdf_ref_host.py shows: at ar999 1024 x 32 on the unperturbed
points a 16-bit inverse moves log q by 6.9 only, so there `lq <= 8` alone would not catch that defect -- the two ratios of the
standardised points of the same case (9.4 whole, 83 per block with 16-bit inverses) do."""
import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import _lib
from oracle import oracle as O
from tests import basedist_ref as B
from tests import logpdf_ref as L
from tests import lowrank_ref as LR
from tests import solve_ref as S
from tests.helpers import SEED, make_family, make_problem

pytestmark = pytest.mark.gpu

F32_FACTOR = 8.0                 # tests/test_gpu_solve_yardstick.py
VALUE_RTOL = 1e-5                # tests/test_gpu_parity.py (f32)
TOL64 = 1e-11                    # tests/test_gpu_parity.py TOL[np.float64]
NAMES = {avi.MEANFIELD: "meanfield", avi.FULLRANK: "fullrank", avi.LOWRANK: "lowrank"}


def _np(t):
    return t.cpu().numpy().copy()


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / max(np.linalg.norm(b), np.finfo(np.float64).tiny))


def _lowrank(rng, d, r, dtype):
    return avi.LowRankGaussian(rng.normal(size=d).astype(dtype), rng.uniform(0.5, 1.5, size=d).astype(dtype), (0.7 * rng.normal(size=(d, r))).astype(dtype))


def _family(rng, family, d, dtype, r=0):
    return _lowrank(rng, d, r, dtype) if family == avi.LOWRANK else make_family(rng, d, family, dtype)[0]


def _context(q, n, dtype, ent=0):
    ctx = avi.MiviContext(dtype, q.family, len(q), n, ent, SEED, rank=getattr(q, "rank", 0))
    ctx.set_base_dist(getattr(q, "dist", None))
    return ctx


def _point_sets(ctx, p, idx, rng):
    """the context's own points (and draws) of estimate idx, and the perturbed set"""
    Z, eps = ctx.sample(p, idx)
    Z, eps = _np(Z), _np(eps)
    return [Z, (Z.astype(np.float64) + 3.0 * rng.normal(size=Z.shape)).astype(Z.dtype)], eps


def _logpdf(ctx, p, Z, want_std):
    out = ctx.logpdf(p, Z, std=True if want_std else None)
    ctx.synchronize()
    return (_np(out[0]).astype(np.float64), _np(out[1]).astype(np.float64)) if want_std else (_np(out).astype(np.float64), None)


def _hold_values(got, ref, d, dtype, what):
    """the tolerances of the non-yardstick cases on log q: f32 per value, f64 in relative l2"""
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    if dtype == np.float32:
        bad = np.abs(got - ref) > VALUE_RTOL * np.maximum(np.abs(ref), d)
        assert not bad.any(), (what, int(bad.sum()), float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), d))))
    else:
        assert _rel(got, ref) <= TOL64, (what, _rel(got, ref))


def _hold_std(got, params, d, family, Z, base, dtype, what):
    """the standardised points: f32 by the yardstick criterion, f64 in relative l2"""
    _, ref = L.logpdf_cols(params, d, family, Z, base, np.float64)
    if dtype == np.float32:
        _, yard = L.logpdf_cols(params, d, family, Z, base, np.float32)
        whole, block = S.block_ratios(got, yard, ref, d)
        assert whole <= F32_FACTOR and block <= F32_FACTOR, (what, whole, block)
    else:
        assert _rel(got, ref) <= TOL64, (what, _rel(got, ref))


def _check(ctx, p, params, family, Z, base, dtype, what, rank=0):
    d = ctx.d
    want_std = family != avi.LOWRANK
    got, std = _logpdf(ctx, p, Z, want_std)
    ref, _ = L.logpdf_cols(params, d, family, Z, base, np.float64, rank=rank)
    _hold_values(got, ref, d, dtype, what)
    if want_std:
        _hold_std(std, params, d, family, Z, base, dtype, what)


# ---- 1. the f32 yardstick of the full-rank forward solve -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d,n", L.YARDSTICK_CASES, ids=[f"{k}-{d}x{n}" for k, d, n in L.YARDSTICK_CASES])
def test_f32_yardstick_fullrank(kind, d, n):
    """every (kind, d, n) of logpdf_ref.YARDSTICK_CASES, both point sets; the worst ratios are in the file's docstring"""
    C, mu, params = L.yardstick_setup(kind, d)
    ctx = avi.MiviContext(np.float32, avi.FULLRANK, d, n, 0, SEED)
    p = ctx.to_device(params)
    sets, _ = _point_sets(ctx, p, 3, np.random.default_rng(d + n))
    for which, Z in enumerate(sets):
        got, std = _logpdf(ctx, p, Z, True)
        (lq_ref, U_ref), (lq_yard, U_yard) = (L.logpdf_cols(params, d, L.FULLRANK, Z, None, t) for t in (np.float64, np.float32))
        whole, block = S.block_ratios(std, U_yard, U_ref, d)
        lq = L.logq_ratio(got, lq_yard, lq_ref)
        print(f"[logpdf yardstick] {'lds' if d <= 1056 else 'scratch'} {kind} {d} {n} set {which}: {whole:.2f}, {block:.2f}, logq {lq:.2f}")
        assert np.all(np.isfinite(got)) and np.all(np.isfinite(std))
        assert whole <= F32_FACTOR and block <= F32_FACTOR and lq <= F32_FACTOR, (kind, d, n, which, whole, block, lq)
    ctx.close()


# ---- 2. small and ragged shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 5, 33, 65, 130])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("family", [avi.MEANFIELD, avi.FULLRANK, avi.LOWRANK], ids=lambda f: NAMES[f])
def test_small_and_ragged_shapes(family, dtype, d):
    rng = np.random.default_rng(100 * family + d)
    for r in ((1, 4, 64) if family == avi.LOWRANK else (0,)):   # (r > d included: mivi_create admits every 1 <= r <= 64)
        q = _family(rng, family, d, dtype, r)
        params, _ = avi.destructure(q)
        for n in (1, 7, 65):
            ctx = _context(q, n, dtype)
            p = ctx.to_device(params)
            sets, _ = _point_sets(ctx, p, 1, rng)
            for which, Z in enumerate(sets):
                _check(ctx, p, params, family, Z, None, dtype, (NAMES[family], d, r, n, which), rank=r)
            ctx.close()


# ---- 3. f64, full-rank -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d,n", [(k, d, n) for k in ("default", "ar999", "graded") for d, n in ((200, 33), (1024, 32))] + [("default", 2500, 8)],
                         ids=lambda v: str(v))
def test_f64_fullrank(kind, d, n):
    """(2500, 8) is past the size at which 16 columns of X fit LDS (and past what the C^T solves admit): X lives in the call's scratch.
    With and without std the values are the same bits."""
    C, mu, params = L.yardstick_setup(kind, d, np.float64)
    ctx = avi.MiviContext(np.float64, avi.FULLRANK, d, n, 0, SEED)
    p = ctx.to_device(params)
    sets, _ = _point_sets(ctx, p, 2, np.random.default_rng(d))
    for which, Z in enumerate(sets):
        got, std = _logpdf(ctx, p, Z, True)
        ref, U = L.logpdf_cols(params, d, L.FULLRANK, Z, None, np.float64)
        assert _rel(got, ref) <= TOL64 and _rel(std, U) <= TOL64, (kind, d, n, which, _rel(got, ref), _rel(std, U))
        alone, _ = _logpdf(ctx, p, Z, False)
        assert np.array_equal(alone, got)
    ctx.close()


# ---- 4. bases ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n", [(33, 65), (256, 64)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("family", [avi.MEANFIELD, avi.FULLRANK], ids=lambda f: NAMES[f])
@pytest.mark.parametrize("dist", [avi.Laplace(), avi.TDist(3.0), avi.TDist(0.7)], ids=["laplace", "t3", "t0.7"])
def test_bases(dist, family, dtype, d, n):
    rng = np.random.default_rng(d + family)
    q0 = make_family(rng, d, family, dtype)[0]
    q = avi.MvLocationScale(q0.location, q0.scale, dist)
    params, _ = avi.destructure(q)
    ctx = _context(q, n, dtype)
    p = ctx.to_device(params)
    sets, _ = _point_sets(ctx, p, 4, rng)
    for which, Z in enumerate(sets):
        _check(ctx, p, params, family, Z, B.base_of(dist), dtype, (repr(dist), NAMES[family], d, n, which))
    ctx.close()


# ---- 5. the chunk walk ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("family", [avi.MEANFIELD, avi.LOWRANK], ids=lambda f: NAMES[f])
def test_chunk_walk(family, dtype):
    d, n, r = 8, 16384 + 5, 4
    rng = np.random.default_rng(7)
    q = _family(rng, family, d, dtype, r)
    params, _ = avi.destructure(q)
    ctx = _context(q, n, dtype)
    p = ctx.to_device(params)
    Z, _ = ctx.sample(p, 1)
    _check(ctx, p, params, family, _np(Z), None, dtype, (NAMES[family], "chunks"), rank=r)
    ctx.close()


# ---- 6. consistency with the estimators ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["default", "ar999"])
def test_std_is_the_contexts_own_draws(kind):
    """At z = C eps + mu of ctx.sample the standardised points are eps, to the yardstick of case 1 with eps as the reference."""
    d, n = 256, 64
    C, mu, params = L.yardstick_setup(kind, d)
    ctx = avi.MiviContext(np.float32, avi.FULLRANK, d, n, 0, SEED)
    p = ctx.to_device(params)
    Z, eps = ctx.sample(p, 5)
    Z, eps = _np(Z), _np(eps).astype(np.float64)
    _, std = _logpdf(ctx, p, Z, True)
    ctx.close()
    _, yard = L.logpdf_cols(params, d, L.FULLRANK, Z, None, np.float32)
    whole, block = S.block_ratios(std, yard, eps, d)
    print(f"[logpdf own draws] {kind}: {whole:.2f}, {block:.2f}")
    assert whole <= F32_FACTOR and block <= F32_FACTOR, (kind, whole, block)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("family", [avi.MEANFIELD, avi.FULLRANK, avi.LOWRANK], ids=lambda f: NAMES[f])
def test_mean_neg_logq_is_the_monte_carlo_entropy(family, dtype):
    d, n, r = 48, 40, 3
    rng = np.random.default_rng(21 + family)
    q = _family(rng, family, d, dtype, r)
    params, _ = avi.destructure(q)
    ctx = _context(q, n, dtype)
    p = ctx.to_device(params)
    Z, _ = ctx.sample(p, 9)
    Z = _np(Z)
    got, _ = _logpdf(ctx, p, Z, False)
    ctx.close()
    p64, Z64 = params.astype(np.float64), Z.astype(np.float64)
    if family == avi.LOWRANK:
        qt = LR.split(torch.tensor(p64), d, r)
        ref = float(LR.estimate_entropy(LR.MONTE_CARLO, torch.tensor(Z64), qt, qt))
    else:
        scale = p64[d:] if family == avi.MEANFIELD else np.tril(p64[d:].reshape(d, d, order="F"))
        q_o = O.MvLocationScale(p64[:d], scale)
        ref = O.estimate_entropy(O.ENT_MONTE_CARLO, Z64, q_o, q_o)
    assert abs(float(np.mean(-got)) - ref) <= (VALUE_RTOL if dtype == np.float32 else TOL64) * abs(ref)


# ---- 7. the call leaves the context as it found it ----------------------------------------------------------------------------------------
def _state_case(which, dtype=np.float32):
    rng = np.random.default_rng(31)
    if which == "fullrank-stl":
        d, M, ent = 256, 64, avi.StickingTheLandingEntropy.code
        q = make_family(rng, d, avi.FULLRANK, dtype)[0]
    elif which == "lowrank":
        d, M, ent = 64, 32, avi.MonteCarloEntropy.code
        q = _lowrank(rng, d, 4, dtype)
    else:   # full-rank, a shape the batch engine does not take: mivi_estimate_gradient_n records and replays a hipGraph from 6 estimates on
        d, M, ent = 96, 48, avi.ClosedFormEntropy.code
        q = make_family(rng, d, avi.FULLRANK, dtype)[0]
    prob, _ = make_problem(rng, "diag", d, dtype)
    return q, d, M, ent, prob


@pytest.mark.parametrize("which", ["fullrank-stl", "lowrank"])
def test_estimates_around_a_logpdf_are_bitwise_unchanged(which):
    q, d, M, ent, prob = _state_case(which)
    params, _ = avi.destructure(q)
    Zpts = np.random.default_rng(1).normal(size=(d, 40)).astype(np.float32)
    results = []
    for interleave in (True, False):
        ctx = _context(q, M, np.float32, ent)
        ctx.set_problem(prob)
        p = ctx.to_device(params)
        v0, g0 = ctx.estimate_gradient(p, 7)
        if interleave:
            ctx.logpdf(p, Zpts, std=True if which != "lowrank" else None)
        v1, g1 = ctx.estimate_gradient(p, 8)
        ctx.synchronize()
        results.append([_np(t) for t in (v0, g0, v1, g1)])
        ctx.close()
    for a, b in zip(*results):
        assert np.array_equal(a, b)


def test_graph_batched_estimates_around_a_logpdf_are_bitwise_unchanged():
    """mivi_estimate_gradient_n with count = 8 >= the smallest captured batch (6) on a shape neither the batch engine nor the lane-batched
    routes take: the first call records ONE hipGraph for (count, params, value, grad), the next two replay it.  A logpdf after each call
    (the first one allocates its scratch) neither drops the graph -- the recording count stays 1 -- nor changes a replay's result."""
    q, d, M, ent, prob = _state_case("graph")
    params, _ = avi.destructure(q)
    Zpts = np.random.default_rng(2).normal(size=(d, 33)).astype(np.float32)
    count, results = 8, []
    for interleave in (True, False):
        ctx = _context(q, M, np.float32, ent)
        ctx.set_problem(prob)
        p = ctx.to_device(params)
        assert not ctx.batch_takes_engine(p)
        v, g = ctx.empty(1), ctx.empty(ctx.params_len)   # (the same buffers every call: they are part of the graph's key)
        out = []
        for idx0 in (0, 0, count):   # recorded; replayed at the same index; replayed further on
            ctx.estimate_gradient_n(p, idx0, count, v, g)
            out += [v.clone(), g.clone()]
            if interleave:
                lq, _ = ctx.logpdf(p, Zpts, std=True)
        ctx.synchronize()
        assert ctx.graph_recordings() == 1
        results.append([_np(t) for t in out])
        if interleave:
            ref, _ = L.logpdf_cols(params, d, L.FULLRANK, Zpts, None, np.float64)
            _hold_values(_np(lq).astype(np.float64), ref, d, np.float32, "between replays")
        ctx.close()
    for a, b in zip(*results):
        assert np.array_equal(a, b)
    assert np.array_equal(results[0][0], results[0][2]) and np.array_equal(results[0][1], results[0][3])   # the replay at the same index
    assert not np.array_equal(results[0][1], results[0][5])                                                  # ... and other draws further on


# ---- 8. interface ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", [avi.MEANFIELD, avi.FULLRANK, avi.LOWRANK], ids=lambda f: NAMES[f])
def test_no_target_needed_and_a_bijector_changes_nothing(family):
    d, n, r = 12, 9, 2
    rng = np.random.default_rng(3)
    q = _family(rng, family, d, np.float32, r)
    params, _ = avi.destructure(q)
    Z = rng.normal(size=(d, n)).astype(np.float32)
    ctx = _context(q, 4, np.float32)          # (n is independent of n_mc; no target is ever set)
    p = ctx.to_device(params)
    plain, _ = _logpdf(ctx, p, Z, False)
    ctx.set_bijector(avi.StackedBijector([(0, 3, "exp"), (3, d, "identity")]))
    wrapped, _ = _logpdf(ctx, p, Z, False)
    host = ctx.logpdf_host(params, Z)
    ctx.close()
    assert np.array_equal(plain, wrapped) and np.array_equal(plain, host.astype(np.float64))
    ref, _ = L.logpdf_cols(params, d, family, Z, None, np.float64, rank=r)
    _hold_values(plain, ref, d, np.float32, NAMES[family])


def test_refusals():
    d, r = 6, 2
    rng = np.random.default_rng(4)
    q = _lowrank(rng, d, r, np.float32)
    params, _ = avi.destructure(q)
    ctx = _context(q, 4, np.float32)
    p, Z = ctx.to_device(params), ctx.to_device(np.zeros(d * 3, np.float32))
    out, std = ctx.empty(3), ctx.empty(d * 3)
    with pytest.raises(avi.MiviError) as e:
        ctx.logpdf(p, Z, std=std)
    assert e.value.status == _lib.ERR_UNSUPPORTED and "low-rank" in str(e.value)
    with pytest.raises(avi.MiviError) as e:
        ctx.logpdf_host(params, np.zeros((d, 3), np.float32), want_std=True)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    lib, h, P = ctx.lib, ctx.h, ctx._p
    assert lib.mivi_logpdf(h, P(p), P(Z), 0, P(out), None) == _lib.ERR_BAD_ARG
    assert lib.mivi_logpdf(h, P(p), P(Z), -1, P(out), None) == _lib.ERR_BAD_ARG
    assert lib.mivi_logpdf(h, None, P(Z), 3, P(out), None) == _lib.ERR_BAD_ARG
    assert lib.mivi_logpdf(h, P(p), None, 3, P(out), None) == _lib.ERR_BAD_ARG
    assert lib.mivi_logpdf(h, P(p), P(Z), 3, None, None) == _lib.ERR_BAD_ARG
    assert lib.mivi_logpdf_host(h, params.ctypes.data, None, 3, None, None) == _lib.ERR_BAD_ARG
    ctx.logpdf(p, Z)   # (the context is still usable)
    ctx.synchronize()
    ctx.close()


@pytest.mark.parametrize("family", [avi.MEANFIELD, avi.FULLRANK, avi.LOWRANK], ids=lambda f: NAMES[f])
def test_nonpositive_scale_and_nan_points(family):
    d, n, r = 40, 20, 3
    rng = np.random.default_rng(6)
    q = _family(rng, family, d, np.float32, r)
    params, _ = avi.destructure(q)
    Z = rng.normal(size=(d, n)).astype(np.float32)
    ctx = _context(q, 4, np.float32)
    # a NaN in one column: that log q alone is NaN, nothing is flagged
    Zn = Z.copy()
    Zn[17, 5] = np.nan
    got, _ = _logpdf(ctx, ctx.to_device(params), Zn, False)     # (synchronize inside: status OK)
    clean = ctx.logpdf_host(params, Z)
    assert np.isnan(got[5]) and np.all(np.isfinite(np.delete(got, 5)))
    assert np.array_equal(np.delete(got, 5), np.delete(clean.astype(np.float64), 5))
    # a negative scale diagonal: the sticky flag, reported by the _host form
    bad = params.copy()
    bad[d + 2 if family != avi.FULLRANK else d + 2 * d + 2] = -0.5
    with pytest.raises(avi.MiviError) as e:
        ctx.logpdf_host(bad, Z)
    assert e.value.status == _lib.ERR_NONPOSITIVE_SCALE
    assert np.array_equal(ctx.logpdf_host(params, Z), clean)    # (the flag was cleared; the context goes on)
    ctx.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_avi_logpdf(dtype):
    d, n = 10, 6
    rng = np.random.default_rng(8)
    mf, fr = (make_family(rng, d, f, dtype)[0] for f in (avi.MEANFIELD, avi.FULLRANK))
    qs = [fr, mf, _lowrank(rng, d, 3, dtype), avi.MvLocationScale(fr.location, fr.scale, avi.TDist(3.0))]
    Z = (2.0 * rng.normal(size=(d, n))).astype(dtype)
    for q in qs:
        params, _ = avi.destructure(q)
        base = B.base_of(q.dist) if getattr(q, "dist", avi.Normal()) != avi.Normal() else None
        ref, _ = L.logpdf_cols(params, d, q.family, Z, base, np.float64, rank=getattr(q, "rank", 0))
        one = avi.logpdf(q, Z[:, 2])
        assert isinstance(one, float)
        many = avi.logpdf(q, Z)
        assert isinstance(many, torch.Tensor) and many.is_cuda and tuple(many.shape) == (n,) and many.dtype == (torch.float32 if dtype == np.float32 else torch.float64)
        assert np.dtype(dtype) == q.eltype
        dev = avi.logpdf(q, torch.as_tensor(Z).cuda())
        assert torch.equal(dev, many)
        _hold_values(_np(many).astype(np.float64), ref, d, dtype, repr(type(q)))
        assert abs(one - ref[2]) <= (VALUE_RTOL if dtype == np.float32 else TOL64) * max(abs(ref[2]), d)
    # the reference's own check (test/families/location_scale.jl:38-42): logpdf(q, z) ~ logpdf(MvNormal(mu, C C'), z), rtol 1e-2
    from scipy.stats import multivariate_normal
    C64 = fr.scale.astype(np.float64)
    mvn = multivariate_normal(mean=fr.location.astype(np.float64), cov=C64 @ C64.T)
    for k in range(n):
        assert np.isclose(avi.logpdf(fr, Z[:, k]), mvn.logpdf(Z[:, k].astype(np.float64)), rtol=1e-2)
