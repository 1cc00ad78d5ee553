"""GPU tests of the low-rank Gaussian family (MIVI_LOWRANK; src/families/location_scale_low_rank.jl): libmivi through the C ABI against
the float64 autograd restatement of the reference's own expressions (tests/lowrank_ref.py) on the same Philox stream.

Tolerances.  Samples and draws: those of tests/test_gpu_parity.py (1e-6 f32, 1e-14 f64, relative l2).  Closed-form estimators: TOL of
that file (value relative, gradient relative l2: f32 1e-5 / 2e-5, f64 1e-12 / 1e-11).  Monte-Carlo / sticking-the-landing estimators (log q
and Sigma^-1 (z - m) by Woodbury): the rule of tests/test_gpu_product_yardstick.py -- the error against the float64 reference is at most
8 x the error of the numpy Woodbury evaluation in the context's dtype on the same inputs, floored at TOL.

For GRADIENTS the test to read is tests/test_gpu_lowrank_yardstick.py: per entry and per 64-row block, on classes that span decades, at
shapes past one row block, one slice and one factor-column block (this file stops at d = 256, M = 128, and its whole-gradient bound
admits a lost block on small D: tests/test_lowrank_ref_host.py).  What only this file covers: the entries' contracts (sample / rand,
estimate_objective at any n_samples, the plugin route, _n / _each bitwise against single calls), the refusals and status bits, the
device loop's equality with the host-driven loop for every rule and averager, and ClipScale on the scale diagonal."""
import ctypes as C

import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import _lib
from oracle import oracle as O
from tests import lowrank_ref as R
from tests.helpers import SEED, OraclePlugin, make_problem, rel_err

pytestmark = pytest.mark.gpu

TOL = {np.float32: (1e-5, 2e-5), np.float64: (1e-12, 1e-11)}
ENTROPIES = [avi.ClosedFormEntropy(), avi.ClosedFormEntropyZeroGradient(), avi.MonteCarloEntropy(),
             avi.StickingTheLandingEntropy(), avi.StickingTheLandingEntropyZeroGradient()]
# d not a multiple of 4, tile edges in d (64 / 256 rows), r (16 columns of U per VJP workgroup, 4 per s tile) and M (8 / 4 columns), r = 1,
# r = the maximum, M = 1
SHAPES = [(10, 1, 1), (10, 2, 7), (30, 3, 10), (67, 5, 33), (130, 64, 70), (256, 16, 128)]
DTYPES = [np.float32, np.float64]


def make_lowrank(rng, d, r, dtype, zero_factors=False):
    mu = rng.normal(size=d).astype(dtype)
    D = rng.uniform(0.5, 1.5, size=d).astype(dtype)
    U = (np.zeros((d, r)) if zero_factors else 0.7 * rng.normal(size=(d, r))).astype(dtype)
    return avi.LowRankGaussian(mu, D, U)


def make_ctx(d, r, M, ent, dtype, prob=None):
    ctx = avi.MiviContext(dtype, avi.LOWRANK, d, M, ent.code, SEED, rank=r)
    if prob is not None:
        ctx.set_problem(prob)
    return ctx


_REF = {}


def reference(key, params, d, r, tgt, eps, kind, dtype):
    """(float64 autograd reference, numpy Woodbury yardstick in dtype): computed once per case, shared and never modified."""
    if key not in _REF:
        ref = R.estimate_gradient(params.astype(np.float64), d, r, tgt, eps, kind)
        cols = [tgt.logdensity_and_gradient(ref["Z"][:, k].copy()) for k in range(eps.shape[1])]
        ell, G = np.array([c[0] for c in cols]), np.stack([c[1] for c in cols], axis=1)
        _REF[key] = (ref, R.woodbury_eval(params, d, r, G, ell, eps, kind, dtype))
    return _REF[key]


def run_case(d, r, M, kind, ent, dtype, idx=3, plugin=False, bijector=False, zero_factors=False):
    rng = np.random.default_rng(4321 + d + 7 * M + 13 * r)
    q = make_lowrank(rng, d, r, dtype, zero_factors)
    prob, tgt = make_problem(rng, kind, d, dtype)
    if plugin:
        prob = OraclePlugin(tgt)
    if bijector:   # Stacked([exp on the first three coordinates, identity on the rest]) around the target
        blocks = [(0, 3, "exp"), (3, d, "identity")]
        prob, tgt = avi.TransformedProblem(prob, avi.StackedBijector(blocks)), O.StackedBijectorTarget(tgt, blocks)
    params, _ = avi.destructure(q)
    ctx = make_ctx(d, r, M, ent, dtype, prob)
    assert ctx.params_len == 2 * d + d * r and ctx.partials_len == 0
    Z, eps = ctx.sample(params, idx)
    assert eps.shape == (d + r, M)
    eps = eps.cpu().numpy().astype(np.float64)
    Z = Z.cpu().numpy().astype(np.float64)
    value, grad = ctx.estimate_gradient(params, idx)
    ctx.synchronize()
    value, grad = float(value.item()), grad.cpu().numpy().astype(np.float64)
    ctx.close()
    key = (d, r, M, kind, ent.code, np.dtype(dtype).name, plugin, bijector, zero_factors)
    ref, yard = reference(key, params, d, r, tgt, eps, ent.code, dtype)
    stol = 1e-6 if dtype == np.float32 else 1e-14
    assert rel_err(eps, O.philox_normal(SEED, idx, d + r, 0, M, f64=dtype == np.float64)) < stol
    assert rel_err(Z, ref["Z"]) < stol
    vt, gt = TOL[dtype]
    gscale = max(np.linalg.norm(ref["grad"]), 1.0)
    v_err, g_err = abs(value - ref["value"]), np.linalg.norm(grad - ref["grad"])
    v_bound, g_bound = vt * abs(ref["value"]), gt * gscale
    if ent.code >= 2:   # Woodbury estimators: the float32 (float64) numpy evaluation is the yardstick
        v_bound = max(v_bound, 8 * abs(yard["value"] - ref["value"]))
        g_bound = max(g_bound, 8 * np.linalg.norm(yard["grad"] - ref["grad"]))
    print(f"[lowrank] {key}: value err {v_err:.3e} (bound {v_bound:.3e}), grad err {g_err:.3e} (bound {g_bound:.3e})")
    assert v_err <= v_bound, (value, ref["value"])
    assert g_err <= g_bound, g_err / gscale
    return value, grad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ent", ENTROPIES, ids=lambda e: type(e).__name__)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_diag_target_all_estimators_all_shapes(shape, ent, dtype):
    run_case(*shape, "diag", ent, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ent", ENTROPIES, ids=lambda e: type(e).__name__)
@pytest.mark.parametrize("kind,plugin", [("dense", False), ("dense", True), ("funnel", False)], ids=["dense", "plugin", "funnel"])
def test_targets_all_estimators(kind, plugin, ent, dtype):
    run_case(67, 5, 33, kind, ent, dtype, plugin=plugin)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_target_on_tile_shapes(dtype):
    run_case(256, 16, 128, "dense", avi.StickingTheLandingEntropy(), dtype)
    run_case(130, 64, 70, "dense", avi.MonteCarloEntropy(), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ent", [avi.ClosedFormEntropy(), avi.StickingTheLandingEntropy()], ids=lambda e: type(e).__name__)
def test_stacked_bijector(ent, dtype):
    run_case(30, 3, 10, "dense", ent, dtype, bijector=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ent", ENTROPIES, ids=lambda e: type(e).__name__)
def test_zero_factors_the_docs_initial_point(ent, dtype):
    """LowRankGaussian(mu, D, zeros(d, 3)): A = I, the factors' gradient is the only way out of U = 0."""
    run_case(30, 3, 10, "dense", ent, dtype, zero_factors=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_estimate_objective_any_n_samples_every_entropy(dtype):
    d, r, n_mc, idx = 10, 2, 16, 2
    rng = np.random.default_rng(8)
    q = make_lowrank(rng, d, r, dtype)
    prob, tgt = make_problem(rng, "dense", d, dtype)
    params, _ = avi.destructure(q)
    ctx = make_ctx(d, r, n_mc, avi.ClosedFormEntropy(), dtype, prob)
    vt = 1e-5 if dtype == np.float32 else 1e-11   # (tests/test_gpu_parity.py: TOL for f32, test_estimate_objective_matches_oracle's for f64)
    for n in (5, 40, 16384 + 37):
        # sample m of the call is column m of the estimate's stream whatever n_mc the context has: the draws of a context with n_mc = n
        sampler = make_ctx(d, r, n, avi.ClosedFormEntropy(), dtype)
        eps = sampler.sample(params, idx)[1].cpu().numpy().astype(np.float64)
        sampler.close()
        for ent in ENTROPIES:
            got = float(ctx.estimate_objective(params, idx, n_samples=n, entropy=ent.code).item())
            want = R.estimate_objective(params.astype(np.float64), d, r, tgt, eps, ent.code)
            assert abs(got - want) <= vt * abs(want), (n, ent.code, got, want)
            if n == 40:
                assert abs(float(ctx.estimate_objective_host(params, idx, n_samples=n, entropy=ent.code)) - want) <= vt * abs(want)
    ctx.close()


def test_rand_is_the_sample_entry():
    """rand(rng, q, n) (location_scale_low_rank.jl:79-86) draws the columns mivi_sample does for the rng's next index."""
    d, r, n = 10, 2, 7
    q = make_lowrank(np.random.default_rng(4), d, r, np.float64)
    rng = avi.PhiloxRNG(SEED)
    idx = rng.counter
    Z = avi.rand(rng, q, n)
    assert tuple(Z.shape) == (d, n) and rng.counter == idx + 1
    ctx = make_ctx(d, r, n, avi.ClosedFormEntropy(), np.float64)
    assert torch.equal(Z, ctx.sample(avi.destructure(q)[0], idx, want_eps=False))
    ctx.close()


def test_estimate_objective_at_optimum_is_zero():
    """estimate_objective(q = pi, 10^5 samples) ~ 0 (atol 1e-2, as tests/test_gpu_parity.py): a diagonal-plus-low-rank target written as a
    dense Gaussian."""
    d, r = 8, 2
    rng = np.random.default_rng(11)
    q = make_lowrank(rng, d, r, np.float64)
    L = np.linalg.cholesky(q.cov())
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), operator=avi.ClipScale())
    v = avi.estimate_objective(avi.PhiloxRNG(SEED), alg, q, avi.DenseNormalProblem(q.location, L), n_samples=10 ** 5)
    assert abs(v) < 1e-2


@pytest.mark.parametrize("dtype", DTYPES)
def test_batched_entries_equal_single_calls_bitwise(dtype):
    d, r, M, n = 30, 3, 10, 3
    rng = np.random.default_rng(5)
    q = make_lowrank(rng, d, r, dtype)
    prob, _ = make_problem(rng, "dense", d, dtype)
    params, _ = avi.destructure(q)
    ctx = make_ctx(d, r, M, avi.StickingTheLandingEntropy(), dtype, prob)
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
    ctx.close()


def _problem_30(dtype):
    d, r = 30, 3
    rng = np.random.default_rng(21)
    prob, _ = make_problem(rng, "dense", d, dtype)
    q0 = avi.LowRankGaussian(np.zeros(d, dtype=dtype), np.ones(d, dtype=dtype), np.zeros((d, r), dtype=dtype))   # docs/src/families.md
    return prob, q0


def test_optimize_docs_problem_elbo_increases():
    """docs/src/families.md:103-236 scaled down: KLMinRepGradDescent(Adam(0.01), ClipScale()) on LowRankGaussian(mu, ones(d), zeros(d, 3))."""
    dtype = np.float32
    prob, q0 = _problem_30(dtype)
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), optimizer=avi.Adam(0.01), n_samples=8, averager=avi.NoAveraging(), operator=avi.ClipScale())
    before = avi.estimate_objective(avi.PhiloxRNG(SEED), alg, q0, prob, n_samples=4096)
    q, info, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 300, prob, q0)
    assert isinstance(q, avi.MvLocationScaleLowRank) and q.rank == 3 and len(info) == 300
    after = avi.estimate_objective(avi.PhiloxRNG(SEED), alg, q, prob, n_samples=4096)
    assert after < before - 1.0, (before, after)   # the negative ELBO falls
    assert np.mean([i["elbo"] for i in info[-20:]]) > np.mean([i["elbo"] for i in info[:20]])
    assert np.linalg.norm(q.scale_factors) > 0.0   # the factors left U = 0
    q_host, info_host, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 300, prob, q0, device_loop=False)
    assert np.array_equal(avi.destructure(q)[0], avi.destructure(q_host)[0])   # the device loop IS the host-driven loop (Adam: bitwise)
    assert [i["elbo"] for i in info] == [i["elbo"] for i in info_host]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("opt", [avi.Descent(1e-3), avi.Adam(0.01), avi.COCOB(), avi.DoG(), avi.DoWG()], ids=lambda o: type(o).__name__)
@pytest.mark.parametrize("averager", [avi.NoAveraging(), avi.PolynomialAveraging()], ids=lambda a: type(a).__name__)
def test_device_loop_equals_host_loop(averager, opt, dtype):
    prob, q0 = _problem_30(dtype)
    for ent, op in ((avi.ClosedFormEntropy(), avi.ClipScale()), (avi.StickingTheLandingEntropy(), avi.IdentityOperator())):
        alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), entropy=ent, optimizer=opt, n_samples=6, averager=averager, operator=op)
        with pytest.warns(UserWarning) if isinstance(op, avi.IdentityOperator) else _nullcontext():
            q_dev, info_dev, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 25, prob, q0)
        with pytest.warns(UserWarning) if isinstance(op, avi.IdentityOperator) else _nullcontext():
            q_host, info_host, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 25, prob, q0, device_loop=False)
        a, b = avi.destructure(q_dev)[0], avi.destructure(q_host)[0]
        if isinstance(opt, avi.DoG):   # DoG / DoWG: the two norms are summed in another order on the device
            assert rel_err(a, b) < (1e-5 if dtype == np.float32 else 1e-12)
        else:
            assert np.array_equal(a, b)
            assert [i["elbo"] for i in info_dev] == [i["elbo"] for i in info_host]


class _nullcontext:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


@pytest.mark.parametrize("dtype", DTYPES)
def test_clip_scale_clamps_only_the_scale_diagonal(dtype):
    d, r = 9, 2
    ctx = make_ctx(d, r, 4, avi.ClosedFormEntropy(), dtype)
    rng = np.random.default_rng(1)
    params = rng.normal(size=2 * d + d * r).astype(dtype) * 1e-3   # entries of every block below epsilon, some negative
    p = ctx.to_device(params).clone()
    avi.ClipScale(0.05).apply(ctx, p)
    got = p.cpu().numpy()
    want = params.copy()
    want[d:2 * d] = np.maximum(want[d:2 * d], dtype(0.05))
    assert np.array_equal(got, want)
    ctx.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _create(family, d, n_mc, rank, m_offset=0, m_total=0):
    lib = _lib.load()
    cfg = _lib.MiviConfig(_lib.F32, family, d, n_mc, 0, 0, C.c_uint64(1), m_offset, m_total, None, 0, rank)
    h = C.c_void_p()
    st = lib.mivi_create(C.byref(cfg), C.byref(h))
    if st == 0:
        lib.mivi_destroy(h)
    return st


def test_create_rejects_bad_rank_and_sharded_contexts():
    assert _create(avi.LOWRANK, 8, 4, 0) == _lib.ERR_BAD_ARG
    assert _create(avi.LOWRANK, 8, 4, 65) == _lib.ERR_BAD_ARG
    assert _create(avi.LOWRANK, 8, 4, 1) == 0 and _create(avi.LOWRANK, 8, 4, 64) == 0
    assert _create(avi.LOWRANK, 8, 4, 2, m_offset=4) == _lib.ERR_UNSUPPORTED
    assert _create(avi.LOWRANK, 8, 4, 2, m_total=8) == _lib.ERR_UNSUPPORTED
    assert _create(avi.LOWRANK, 8, 4, 2, m_total=4) == 0
    assert _create(avi.MEANFIELD, 8, 4, 77) == 0 and _create(avi.FULLRANK, 8, 4, -3) == 0   # rank is read for family 2 only


def test_nonpositive_scale_diagonal_is_status_3():
    d, r = 6, 2
    q = make_lowrank(np.random.default_rng(2), d, r, np.float64)
    params, _ = avi.destructure(q)
    params[d + 2] = -0.1
    ctx = make_ctx(d, r, 4, avi.ClosedFormEntropy(), np.float64, avi.DiagNormalProblem(np.zeros(d), np.ones(d)))
    ctx.estimate_gradient(params, 0)
    with pytest.raises(avi.MiviError) as e:
        ctx.synchronize()
    assert e.value.status == _lib.ERR_NONPOSITIVE_SCALE
    with pytest.raises(avi.MiviError) as e:
        ctx.estimate_gradient_host(params, 0)
    assert e.value.status == _lib.ERR_NONPOSITIVE_SCALE
    ctx.close()


def test_unsupported_entries_refuse_the_family():
    """Every entry outside the family's surface returns MIVI_ERR_UNSUPPORTED (6) with a message naming the family, before reading a buffer."""
    d, r, M = 8, 2, 4
    ctx = make_ctx(d, r, M, avi.ClosedFormEntropy(), np.float32, avi.DiagNormalProblem(np.zeros(d, np.float32), np.ones(d, np.float32)))
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
        "mivi_prox_scale_entropy": lambda: lib.mivi_prox_scale_entropy(h, P, 0.1, None, 0),
    }
    for name, call in calls.items():
        assert call() == _lib.ERR_UNSUPPORTED, name
        msg = lib.mivi_last_error(h).decode()
        assert "low-rank" in msg and name.replace("_host", "") in msg, (name, msg)
    # op = 2 (ProximalLocationScaleEntropy) in the device loop; the Python operator and the other algorithms say so themselves
    with pytest.raises(avi.MiviError) as e:
        ctx.optimize_loop(buf, 2, 0, 0, rule=0, op=2, eta=0.1)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(TypeError, match="low-rank"):
        avi.ProximalLocationScaleEntropy().apply(ctx, buf, avi.Descent(0.1))
    ctx.close()
    q = make_lowrank(np.random.default_rng(0), d, r, np.float32)
    prob = avi.DiagNormalProblem(np.zeros(d, np.float32), np.ones(d, np.float32))
    with pytest.raises(TypeError, match="low-rank"):
        avi.optimize(avi.PhiloxRNG(SEED), avi.KLMinScoreGradDescent(avi.AutoMIVI(), n_samples=4, operator=avi.ClipScale()), 2, prob, q)
    with pytest.raises(TypeError, match="low-rank"):
        avi.optimize(avi.PhiloxRNG(SEED), avi.KLMinRepGradProxDescent(avi.AutoMIVI(), optimizer=avi.Descent(0.1)), 2, prob, q)
    for alg in (avi.KLMinSqrtNaturalGradDescent, avi.KLMinNaturalGradDescent, avi.KLMinWassFwdBwd):
        with pytest.raises(TypeError, match="FullRankGaussian"):
            avi.optimize(avi.PhiloxRNG(SEED), alg(0.1), 2, prob, q)
