"""GPU tests of the score-gradient ELBO estimator (mivi_estimate_score_gradient, ScoreGradELBO, KLMinScoreGradDescent = BBVI):
parity with the numpy restatement (tests/scoregrad_ref.py) on identical draws, known answers, determinism, order-0 targets without
AD, error conventions, the reference's algorithm tests (test/algorithms/klminscoregraddescent.jl:9-97) restated, and that no existing
entry changes.

Tolerances
    f64: those tests/test_gpu_parity.py applies (value rel 1e-12, gradient rel-l2 1e-11 against max(|g|, 1)) -- the full-rank path is
         the sticking-the-landing solve and the VJP checked there.
    f32: no number.  The yardstick is the same restatement evaluated in float32 numpy on the same draws: for every case the library's
         distance to the float64 result is at most 8 x the largest distance the float32 evaluation shows over the case's five
         estimate indices (8: a different summation order over the d terms per sample)."""
import numpy as np
import pytest

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import MiviError
from oracle import oracle as O
from tests import scoregrad_ref as R
from tests.helpers import SEED, BenchDist, OraclePlugin, ReadmeLogReg, make_family, make_problem, readme_bijector, rel_err

pytestmark = pytest.mark.gpu

TOL64 = (1e-12, 1e-11)     # tests/test_gpu_parity.py TOL[np.float64]
F32_FACTOR = 8.0
INDICES = (0, 1, 2, 7, 1000003)
FUNNEL_BLOCKS = lambda d: [(0, 1, "exp"), (1, d, "identity")]   # noqa: E731


class ValueOnlyPlugin:
    """A LogDensityProblems plugin of order 0: `logdensity` and `dimension`, nothing else."""

    def __init__(self, tgt):
        self.tgt = tgt
        self.calls = 0

    def dimension(self):
        return self.tgt.dimension()

    def logdensity(self, z):
        self.calls += 1
        return self.tgt.logdensity(np.asarray(z, dtype=np.float64))


def build_problem(rng, kind, d, dtype):
    """(problem for the context, oracle target, values_only)"""
    if kind == "funnelc":   # the constrained funnel under a Stacked bijector: log pi gains logabsdetjac
        prob = avi.TransformedProblem(avi.FunnelConstrainedProblem(d, 1.5), avi.StackedBijector(FUNNEL_BLOCKS(d)))
        return prob, O.StackedBijectorTarget(O.FunnelConstrainedTarget(d, 1.5), FUNNEL_BLOCKS(d)), False
    if kind == "plugin":    # gradient callback: only the values are used
        _, tgt = make_problem(rng, "logreg1", d, dtype)
        return OraclePlugin(tgt), tgt, False
    if kind == "vplugin":   # value-only callback
        _, tgt = make_problem(rng, "dense", d, dtype)
        return ValueOnlyPlugin(tgt), tgt, True
    if kind == "readme":    # the reference README's model: order 0, constrained scale, under its Stacked bijector (README.md:42-119)
        n, p = 32, d - 1
        model = ReadmeLogReg(rng.normal(size=(n, p)) / np.sqrt(d), rng.uniform(size=n) < 0.5)
        blocks = readme_bijector(p).blocks
        return avi.TransformedProblem(model, readme_bijector(p)), O.StackedBijectorTarget(model, blocks), True
    prob, tgt = make_problem(rng, kind, d, dtype)
    return prob, tgt, False


def _dist(a, b):
    """(|value|, |elbo|, gradient relative l2) distances of result dict a from the float64 result b"""
    gn = np.linalg.norm(b["grad"])
    return (abs(float(a["value"]) - float(b["value"])), abs(float(a["elbo"]) - float(b["elbo"])),
            float(np.linalg.norm(np.asarray(a["grad"], dtype=np.float64) - b["grad"]) / (gn if gn > 0 else 1.0)))


def run_parity(family, dtype, kind, d, M):
    rng = np.random.default_rng(4321 + d + 7 * M)
    q, q_o = make_family(rng, d, family, dtype)
    prob, tgt, values_only = build_problem(rng, kind, d, dtype)
    params, _ = avi.destructure(q)
    p64 = O.destructure(q_o)
    ctx = avi.MiviContext(dtype, family, d, M, avi.ClosedFormEntropy.code, SEED)
    ctx.set_problem(prob, values_only=values_only)
    pd = ctx.to_device(params)
    lib_d, cpu_d = [], []
    for idx in INDICES:
        _, eps = ctx.sample(pd, idx)
        eps = eps.cpu().numpy().copy()
        v, e, g = ctx.estimate_score_gradient(pd, idx)
        ctx.synchronize()
        got = dict(value=float(v.item()), elbo=float(e.item()), grad=g.cpu().numpy().astype(np.float64))
        assert v.dtype == ctx.tdtype and e.dtype == ctx.tdtype and g.dtype == ctx.tdtype
        ref = R.closed_form(p64, d, family, tgt, eps.astype(np.float64))
        if family == avi.FULLRANK:   # exact zeros above the diagonal
            assert np.all(np.triu(got["grad"][d:].reshape(d, d, order="F"), 1) == 0.0)
        if M == 1:
            assert got["value"] == 0.0 and np.all(got["grad"] == 0.0)
        if dtype == np.float64:
            vt, gt = TOL64
            print(f"[scoregrad f64] {kind} fam={family} d={d} M={M} idx={idx}: {_dist(got, ref)}")
            assert abs(got["value"] - ref["value"]) <= vt * abs(ref["value"]), (got["value"], ref["value"])
            assert abs(got["elbo"] - ref["elbo"]) <= vt * abs(ref["elbo"]), (got["elbo"], ref["elbo"])
            assert np.linalg.norm(got["grad"] - ref["grad"]) <= gt * max(np.linalg.norm(ref["grad"]), 1.0), rel_err(got["grad"], ref["grad"])
        else:
            lib_d.append(_dist(got, ref))
            cpu_d.append(_dist(R.closed_form(params, d, family, tgt, eps, np.float32), ref))
    ctx.close()
    if dtype == np.float32:
        lib_m, cpu_m = np.max(np.array(lib_d), axis=0), np.max(np.array(cpu_d), axis=0)
        ratio = [float(a / b) if b > 0 else (0.0 if a == 0 else np.inf) for a, b in zip(lib_m, cpu_m)]
        print(f"[scoregrad f32] {kind} fam={family} d={d} M={M}: library (value, elbo, grad) {lib_m.tolist()}  float32 numpy {cpu_m.tolist()}  ratio {ratio}")
        for what, a, b in zip(("value", "elbo", "gradient"), lib_m, cpu_m):
            assert a <= F32_FACTOR * b, (what, a, b)


SHAPES = {
    "diag": [(5, 1), (5, 2), (37, 10), (64, 100), (256, 256), (1000, 100), (1024, 10), (1024, 256)],   # (256 | 1024, M % 32 == 0): launch_stl2 in f32
    "dense": [(37, 10), (64, 100), (256, 256)],
    "logreg0": [(37, 10), (64, 100)],
    "logreg1": [(37, 10), (64, 256)],
    "funnel": [(5, 2), (37, 100)],
    "funnelc": [(37, 10), (64, 256)],
    "plugin": [(37, 10)],
    "vplugin": [(5, 10), (64, 100)],
    "readme": [(11, 16)],
}
PARITY = [(k, d, M) for k, shapes in SHAPES.items() for d, M in shapes]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("family", [avi.MEANFIELD, avi.FULLRANK], ids=["meanfield", "fullrank"])
@pytest.mark.parametrize("kind,d,M", PARITY, ids=[f"{k}-{d}x{M}" for k, d, M in PARITY])
def test_parity_on_identical_draws(kind, d, M, family, dtype):
    run_parity(family, dtype, kind, d, M)


def _q_equal_pi(family, d, dtype=np.float64):
    mu = np.full(d, 5.0)
    if family == avi.MEANFIELD:
        return avi.MeanFieldGaussian(mu.astype(dtype), np.full(d, 0.3, dtype)), avi.DiagNormalProblem(mu, np.full(d, 0.3))
    L = 0.3 * np.eye(d) + 0.05 * np.tril(np.ones((d, d)), -1) / np.sqrt(d)
    return avi.FullRankGaussian(mu.astype(dtype), L.astype(dtype)), avi.DenseNormalProblem(mu, L)


@pytest.mark.parametrize("family", [avi.MEANFIELD, avi.FULLRANK], ids=["meanfield", "fullrank"])
@pytest.mark.parametrize("d", [5, 64])
def test_known_answer_at_q_equal_to_the_target(family, d):
    """f is constant at q = pi: zero variance, zero gradient (the reference's zero-gradient tolerance, test/algorithms/klminrepgraddescent.jl:66-87)."""
    q, prob = _q_equal_pi(family, d)
    params, _ = avi.destructure(q)
    for M in (2, 10):
        ctx = avi.MiviContext(np.float64, family, d, M, 0, SEED)
        ctx.set_problem(prob)
        v, e, g = ctx.estimate_score_gradient(params, 0)
        ctx.synchronize()
        print(f"[scoregrad q=pi] fam={family} d={d} M={M}: |value| {abs(float(v.item())):.3e} |grad|inf {float(g.abs().max().item()):.3e} elbo {float(e.item()):.3e}")
        assert float(g.abs().max().item()) <= 1e-5
        assert abs(float(v.item())) <= 1e-10
        ctx.close()


@pytest.mark.parametrize("family,d,M,dtype", [(avi.MEANFIELD, 1000, 100, np.float32), (avi.FULLRANK, 256, 64, np.float32),
                                              (avi.FULLRANK, 70, 19, np.float64), (avi.MEANFIELD, 37, 10, np.float64)])
def test_same_call_twice_is_bitwise_equal(family, d, M, dtype):
    rng = np.random.default_rng(3)
    q, _ = make_family(rng, d, family, dtype)
    prob, _ = make_problem(rng, "dense" if d <= 256 else "diag", d, dtype)
    params, _ = avi.destructure(q)
    outs = []
    ctx = avi.MiviContext(dtype, family, d, M, 0, SEED)
    ctx.set_problem(prob)
    for k in range(3):
        if k == 2:   # ... and on a fresh context
            ctx.close()
            ctx = avi.MiviContext(dtype, family, d, M, 0, SEED)
            ctx.set_problem(prob)
        v, e, g = ctx.estimate_score_gradient(params, 5)
        ctx.synchronize()
        outs.append((v.cpu().numpy().copy(), e.cpu().numpy().copy(), g.cpu().numpy().copy()))
    ctx.close()
    for o in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(outs[0], o))


def _bbvi_setup(dtype=np.float64, n_samples=10, optimizer=None, operator=None):
    d = 5
    prob = avi.DiagNormalProblem(np.full(d, 5.0), np.full(d, 0.3))
    q0 = avi.MeanFieldGaussian(np.zeros(d, dtype), np.ones(d, dtype))
    alg = avi.KLMinScoreGradDescent(avi.AutoMIVI(), optimizer=optimizer or avi.Descent(1e-3), n_samples=n_samples,
                                    operator=operator or avi.ClipScale())
    return alg, prob, q0


def test_optimize_is_deterministic_for_a_copied_rng():
    """klminscoregraddescent.jl:40-57: two runs from copies of one rng give bitwise equal outputs."""
    alg, prob, q0 = _bbvi_setup()
    rng = avi.PhiloxRNG(SEED)
    outs = []
    for _ in range(2):
        q, info, _ = avi.optimize(rng.copy(), alg, 10, prob, q0)
        outs.append((np.asarray(q.location).copy(), np.asarray(q.scale).copy(), [i["elbo"] for i in info]))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]


def test_order0_problem_runs_without_ad():
    """A problem with only `logdensity` through KLMinScoreGradDescent(AutoMIVI(target_ad=None)): the value-only callback, no AD,
    no @info; KLMinRepGradDescent with that adtype still raises its TypeError."""
    d = 6
    prob = ValueOnlyPlugin(O.DiagNormalTarget(np.full(d, 1.0), np.full(d, 0.5)))
    q0 = avi.MeanFieldGaussian(np.zeros(d), np.ones(d))
    ad = avi.AutoMIVI(target_ad=None)
    alg = avi.KLMinScoreGradDescent(ad, optimizer=avi.Descent(1e-3), n_samples=8, operator=avi.ClipScale())
    q, info, state = avi.optimize(avi.PhiloxRNG(SEED), alg, 3, prob, q0)
    assert len(info) == 3 and all(np.isfinite(i["elbo"]) for i in info)
    assert prob.calls == 3 * 8
    bench = BenchDist(d)   # has logdensity_and_gradient but declares order 0: never asked for a gradient
    avi.optimize(avi.PhiloxRNG(SEED), alg, 2, bench, q0)
    assert bench.grad_calls == 0
    with pytest.raises(TypeError, match="LogDensityOrder"):
        avi.optimize(avi.PhiloxRNG(SEED), avi.KLMinRepGradDescent(ad, operator=avi.ClipScale()), 1, prob, q0)


def test_error_conventions():
    d, M = 8, 4
    q = avi.MeanFieldGaussian(np.zeros(d), np.ones(d))
    params, _ = avi.destructure(q)
    tgt = O.DiagNormalTarget(np.zeros(d), np.ones(d))
    # a sharded context
    for kw in (dict(m_offset=4, m_total=8), dict(m_total=8)):
        ctx = avi.MiviContext(np.float64, avi.MEANFIELD, d, M, 0, SEED, **kw)
        ctx.set_problem(avi.DiagNormalProblem(np.zeros(d), np.ones(d)))
        with pytest.raises(MiviError) as ei:
            ctx.estimate_score_gradient(params, 0)
        assert ei.value.status == 6 and "sharded" in str(ei.value)
        ctx.close()
    # a full-rank d beyond the LDS-resident triangular solve (the limit of the sticking-the-landing route)
    dbig = 2624
    ctx = avi.MiviContext(np.float64, avi.FULLRANK, dbig, 2, 0, SEED)
    ctx.set_problem(avi.DiagNormalProblem(np.zeros(dbig), np.ones(dbig)))
    pbig = ctx.to_device(np.concatenate([np.zeros(dbig), np.eye(dbig).reshape(-1)]))
    with pytest.raises(MiviError) as ei:
        ctx.estimate_score_gradient(pbig, 0)
    assert ei.value.status == 6 and "too large" in str(ei.value)
    ctx.close()
    del pbig
    # every entry that needs the target's gradient refuses a value-only target; the value entries accept it
    ctx = avi.MiviContext(np.float64, avi.MEANFIELD, d, M, 0, SEED)
    ctx.set_problem(ValueOnlyPlugin(tgt), values_only=True)
    with pytest.raises(MiviError) as ei:
        ctx.estimate_gradient(params, 0)
    assert ei.value.status == 6
    with pytest.raises(MiviError) as ei:
        ctx.estimate_partials(params, 0)
    assert ei.value.status == 6
    assert np.isfinite(float(ctx.estimate_objective(params, 0, n_samples=M, entropy=2).item()))
    v, e, g = ctx.estimate_score_gradient(params, 0)
    ctx.synchronize()
    assert np.isfinite(float(v.item()))
    ctx.close()
    # mivi_set_target_callback keeps rejecting a NULL gradient function
    import ctypes as C
    from advancedvi_jl_amd import _lib
    ctx = avi.MiviContext(np.float64, avi.MEANFIELD, d, M, 0, SEED)
    st = ctx.lib.mivi_set_target_callback(ctx.h, C.cast(None, _lib.LOGDENSITY_AND_GRADIENT_FN), C.cast(None, _lib.LOGDENSITY_FN), None)
    assert st == _lib.ERR_BAD_ARG
    ctx.close()

    class NaNTarget:
        def dimension(self):
            return d

        def logdensity(self, z):
            return float("nan")

    alg = avi.KLMinScoreGradDescent(avi.AutoMIVI(), optimizer=avi.Descent(1e-3), n_samples=4, operator=avi.ClipScale())
    with pytest.raises(RuntimeError, match="diverged"):
        avi.optimize(avi.PhiloxRNG(1), alg, 3, NaNTarget(), q)
    # a non-positive scale diagonal: the sticky flag, as mivi_estimate_gradient
    bad = params.copy()
    bad[d + 3] = -0.25
    ctx = avi.MiviContext(np.float64, avi.MEANFIELD, d, M, 0, SEED)
    ctx.set_problem(avi.DiagNormalProblem(np.zeros(d), np.ones(d)))
    ctx.estimate_score_gradient(bad, 0)
    with pytest.raises(Exception, match="scale diagonal"):
        ctx.synchronize()
    ctx.synchronize()
    ctx.close()


# ---- the reference's algorithm tests, restated (test/algorithms/klminscoregraddescent.jl:9-97) ----------------------------------------
@pytest.mark.parametrize("n_samples", [1, 10])
def test_one_step_with_n_samples(n_samples):
    alg, prob, q0 = _bbvi_setup(n_samples=n_samples)
    q, info, state = avi.optimize(avi.PhiloxRNG(SEED), alg, 1, prob, q0)
    assert len(info) == 1 and np.isfinite(info[0]["elbo"]) and state["iteration"] == 1


def test_callback_sees_iterations_one_to_T():
    alg, prob, q0 = _bbvi_setup()
    seen = []
    T = 7
    _, info, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, T, prob, q0, callback=lambda **kw: seen.append(kw["iteration"]) or {"test_value": kw["iteration"]})
    assert seen == list(range(1, T + 1))
    assert [i["test_value"] for i in info] == list(range(1, T + 1)) and [i["iteration"] for i in info] == list(range(1, T + 1))


def test_estimate_objective_of_the_algorithm():
    alg, prob, _ = _bbvi_setup()
    q = avi.MeanFieldGaussian(np.full(5, 5.0), np.full(5, 0.3))   # q = pi
    rng = avi.PhiloxRNG(SEED)
    for n in (None, 1, 3):
        assert np.isfinite(avi.estimate_objective(rng, alg, q, prob, n_samples=n))
    assert np.isfinite(avi.estimate_objective(alg, q, prob))                      # default-rng forms
    assert np.isfinite(avi.estimate_objective(avi.ScoreGradELBO(4), q, prob))
    v = avi.estimate_objective(rng, alg, q, prob, n_samples=10 ** 5)
    print(f"[scoregrad objective q=pi] {v:.3e}")
    assert abs(v) <= 0.2   # the absolute bound of test_objective_at_q_equal_to_the_target_is_about_zero for this quantity
    # ... and it is the value route with the Monte-Carlo entropy on the same draws
    r1, r2 = avi.PhiloxRNG(SEED, 3), avi.PhiloxRNG(SEED, 3)
    q2 = avi.MeanFieldGaussian(np.zeros(5), np.ones(5))
    assert avi.estimate_objective(r1, avi.ScoreGradELBO(16), q2, prob) == avi.estimate_objective(r2, avi.RepGradELBO(16, entropy=avi.MonteCarloEntropy()), q2, prob)


def test_identity_operator_warning():
    d = 5
    prob = avi.DiagNormalProblem(np.full(d, 5.0), np.full(d, 0.3))
    q0 = avi.MeanFieldGaussian(np.zeros(d), np.ones(d))
    alg = avi.KLMinScoreGradDescent(avi.AutoMIVI(), optimizer=avi.Descent(1e-3), n_samples=4)
    with pytest.warns(UserWarning, match="IdentityOperator"):
        avi.optimize(avi.PhiloxRNG(SEED), alg, 1, prob, q0)
    with pytest.warns(UserWarning, match="IdentityOperator"):   # default-rng form of optimize
        avi.optimize(alg, 1, prob, q0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dtypes_of_the_output_and_of_the_elbo(dtype):
    import torch
    alg, prob, q0 = _bbvi_setup(dtype=dtype)
    rng = avi.PhiloxRNG(SEED)
    state = avi.init(rng, alg, q0, prob)
    ctx = state["obj_st"].obj_ad_prep
    assert isinstance(state["obj_st"], avi.ScoreGradELBOState)
    out, _, info = avi.estimate_gradient_(rng, alg.objective, alg.adtype, state["grad_buf"], state["obj_st"], state["params"], state["restructure"])
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    assert out.value_t.dtype == tdt and out.gradient_t.dtype == tdt and info["elbo"].dtype == tdt
    # out.value is the VarGrad objective, info["elbo"] the separate scalar: the same numbers as the context entry
    v, e, g = ctx.estimate_score_gradient(state["params"], 0)
    assert float(v.item()) == out.value() and float(e.item()) == float(info["elbo"]) and np.array_equal(g.cpu().numpy(), out.gradient().cpu().numpy())
    assert out.value() >= 0.0 and float(info["elbo"]) < 0.0
    q, _, _ = avi.optimize(rng, alg, 2, prob, q0)
    assert np.asarray(q.location).dtype == dtype
    new_state, _, info = avi.step(rng, alg, state, None)
    # `step` keeps the objective's own elbo for this algorithm (for RepGradELBO it is -value; here value is a variance)
    assert isinstance(info["elbo"], float) and info["elbo"] < 0.0 and info["elbo"] != -new_state["grad_buf"].value()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_convergence(dtype):
    """klminscoregraddescent.jl:9-38: d = 5, target N(5 1, 0.3^2 I), q0 = N(0, I) mean-field, Descent(1e-3), 100 samples, T = 1000,
    ClipScale: the distance to the optimum at least halves."""
    alg, prob, q0 = _bbvi_setup(dtype=dtype, n_samples=100)
    opt = np.concatenate([np.full(5, 5.0), np.full(5, 0.3)])
    p0, _ = avi.destructure(q0)
    q, info, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 1000, prob, q0)
    p, _ = avi.destructure(q)
    d0, d1 = np.linalg.norm(p0 - opt), np.linalg.norm(np.asarray(p, dtype=np.float64) - opt)
    print(f"[scoregrad convergence {np.dtype(dtype).name}] |dlambda| {d1:.3e} / {d0:.3e} = {d1 / d0:.3e}")
    assert d1 <= d0 / 2


@pytest.mark.parametrize("family,d,M", [(avi.MEANFIELD, 40, 24), (avi.FULLRANK, 256, 64), (avi.FULLRANK, 70, 19)])
def test_existing_entries_are_unchanged_by_a_score_call(family, d, M):
    """mivi_estimate_gradient (sticking-the-landing: the solve and the VJP the score route borrows) is bitwise what it was, before and
    after score calls on the same context -- no scratch, packed operand or speculative draw of the score route is picked up."""
    rng = np.random.default_rng(77)
    q, _ = make_family(rng, d, family, np.float32)
    prob, _ = make_problem(rng, "diag", d, np.float32)
    params, _ = avi.destructure(q)
    ent = avi.StickingTheLandingEntropy.code
    ctx = avi.MiviContext(np.float32, family, d, M, ent, SEED)
    ctx.set_problem(prob)
    pd = ctx.to_device(params)

    def est(idx):
        v, g = ctx.estimate_gradient(pd, idx)
        ctx.synchronize()
        return v.cpu().numpy().copy(), g.cpu().numpy().copy()

    before = [est(i) for i in (5, 6, 9)]
    ctx.estimate_score_gradient(pd, 6)
    after = [est(5)]
    ctx.estimate_score_gradient(pd, 5)     # the index a speculative draw would have been made for
    after.append(est(6))
    ctx.estimate_score_gradient(pd, 123)
    after.append(est(9))
    for (v0, g0), (v1, g1) in zip(before, after):
        assert np.array_equal(v0, v1) and np.array_equal(g0, g1)
    ctx.close()
