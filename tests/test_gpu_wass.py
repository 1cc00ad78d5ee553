"""KLMinWassFwdBwd on the device (src/algorithms/klminwassfwdbwd.jl): the update kernels of csrc/kernels_wass.hip against the numpy restatement
tests/wass_ref.py, mivi_wass_steps against the single calls, trajectories against the restatement driven by the device's own draws, the
algorithm's surface (mirroring test/algorithms/klminwassfwdbwd.jl), the refusals and the failure path.

Sizes: d in {3, 10, 44, 45, 64, 65, 130} (one to three 64-row panels, sizes that are no multiple of the tile), eta in {1e-3, 0.1, 1}, H
symmetric negative definite (`second`), non-symmetric (`stein`) and with an eigenvalue of -1/eta (`singular`: M = I + eta H' singular).

Criteria.  The device builds the square root by the coupled Newton-Schulz iteration; the reference of every update check is the LITERAL
expression (an eigendecomposition), which is not code under test.  f64: relative l2 1e-12 on m', 1e-11 on C', Sigma' and the entropy
(TOL64).  f32: both numbers of tests/solve_ref.block_ratios(got, yard, ref64, d) at most F32_FACTOR = 8, yard the literal expression in
float32, ref64 the same in float64, both on the f32-stored inputs; the entropy relative 1e-5.  `singular`: the square root has a branch
point where A's eigenvalue vanishes, and any two ways to evaluate the expression differ there by the square root of rounding: the tolerance
of a fixture is ten times the distance between the two CPU forms on it, floored at TOL64 (the rule of tests/test_gpu_bam.py).
Trajectories: the same rule on the two forms' trajectories.

Measured on the MI355X (relative l2 unless said otherwise):
    init                                  f64 bitwise symmetric, within TOL64 of Hermitian(C C'); f32 yardstick ratios at most 0.49
    update, second / stein, f64           m' 7.0e-17, C' 3.7e-13, Sigma' 1.6e-13, entropy 2.6e-14 (all but m' at second, d = 65, eta = 1)
    update, second / stein, f32           yardstick ratios 0.80 (whole: m', d = 3), 0.86 (worst 64-row block: m', d = 65); entropy 5.0e-8
    update, singular, f64                 within ten times the CPU forms' distance everywhere, no flag: C' 3.7e-16 .. 9.2e-8 (tolerance
                                          1.6e-6 there), Sigma' 5.0e-16 .. 3.6e-9 (3.6e-8); the CPU form takes 12 to 63 rounds on them
    C' C'' against Sigma'                 f64 at most 2.9e-16, f32 at most 4.9e-8 (bound 1.5e-7 at d = 3)
    10-step f64 trajectories              reference model 4.1e-15 / 2.2e-16 (Stein / Hessians), dense d = 33: 2.8e-15; elbo 1.6e-15
    convergence, T = 1000                 1.3e-5 (Stein), 9.4e-7 (Hessians) of the initial squared distance; subsampling, batch size 1:
                                          0.0034, the restatement on the same batches and draws 0.0034 (m 1.2e-16, C 7.2e-16 from it)"""
import functools

import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import subsampling as SUB
from oracle import oracle as O
from tests import natgrad_ref as NR
from tests import wass_ref as R
from tests.helpers import SEED, make_family, make_problem, rel_err
from tests.measure_space_cases import DTYPES, TOL64, VALUE_RTOL
from tests.measure_space_cases import dense_ctx as _dense_ctx, flat as _flat, logreg as _logreg, reference_model as _reference_model
from tests.measure_space_cases import hold, refused as _refused, trajectory_case as _trajectory_case

pytestmark = pytest.mark.gpu
_hold = functools.partial(hold, "wass")

DS = (3, 10, 44, 45, 64, 65, 130)
ETAS = (1e-3, 0.1, 1.0)
BRANCHES = pytest.mark.parametrize("second", [False, True], ids=["stein", "order2"])


def _mat(v, d):
    return np.asarray(v).reshape(d, -1, order="F")


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _ctx(dtype, d, n=4):
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, n, 0, SEED)
    ctx.set_problem(avi.DiagNormalProblem(np.zeros(d, dtype), np.ones(d, dtype)))
    return ctx


# ---- init and update -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(dtype, kind, d, eta):
    """(params, Sigma0 flat from mivi_wass_init, g, H) in dtype."""
    m, C, g, H = R.fixture(kind, d, eta, dtype)
    params, _ = avi.destructure(avi.FullRankGaussian(m, C))
    ctx = _ctx(dtype, d)
    pd = ctx.to_device(params).clone()
    st0 = ctx.wass_init(pd).cpu().numpy().copy()
    ctx.synchronize()
    assert np.array_equal(pd.cpu().numpy(), params)                          # init only reads the parameters
    ctx.close()
    return params, st0, g, H


@DTYPES
@pytest.mark.parametrize("d", DS)
def test_init_is_the_covariance(d, dtype):
    params, st0, _, _ = _case(dtype, "second", d, 0.1)
    C = np.tril(_mat(params[d:], d))
    S = _mat(st0, d)
    assert S.dtype == dtype and np.array_equal(S, S.T)
    if dtype == np.float64:
        assert rel_err(S, R.hermitian(C @ C.T)) <= TOL64[1]
    else:
        _hold("init Sigma", d, S, R.hermitian(C @ C.T), R.hermitian(_f64(C) @ _f64(C).T))


def _device_update(dtype, kind, d, eta):
    """(m', C', Sigma', entropy) of mivi_wass_update; g and H come back bit-identical."""
    params, st0, g, H = _case(dtype, kind, d, eta)
    ctx = _ctx(dtype, d)
    pd, sd, gd, Hd = ctx.to_device(params).clone(), ctx.to_device(st0).clone(), ctx.to_device(g), ctx.to_device(_flat(H))
    ent = ctx.wass_update(pd, sd, gd, Hd, eta)
    ctx.synchronize()                                                        # (raises on a sticky flag)
    assert np.array_equal(gd.cpu().numpy(), g) and np.array_equal(Hd.cpu().numpy(), _flat(H))
    got, st, ent = pd.cpu().numpy(), sd.cpu().numpy(), ent.cpu().numpy()[0]
    ctx.close()
    assert got.dtype == dtype and st.dtype == dtype and np.all(np.isfinite(got)) and np.all(np.isfinite(st))
    C = _mat(got[d:], d)
    assert np.all(np.triu(C, 1) == 0.0) and np.all(np.diag(C) > 0.0)         # exact zeros above the diagonal
    return got[:d], C, _mat(st, d), ent


def _reference(dtype, kind, d, eta, update=R.update_literal, yard=False):
    """The update on the dtype-stored inputs in float64; yard: the literal expression in float32."""
    params, st0, g, H = _case(dtype, kind, d, eta)
    args = (_f64(params[:d]), _f64(_mat(st0, d)), _f64(g), _f64(H), eta)
    return R.update_literal(*args, np.float32) if yard else update(*args)


@DTYPES
@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("kind", ["second", "stein"])
def test_update_matches_the_literal_expression(kind, d, eta, dtype):
    m, C, S, ent = _device_update(dtype, kind, d, eta)
    m_ref, C_ref, S_ref = _reference(dtype, kind, d, eta)
    ent_ref = float(R.entropy(C_ref))
    if dtype == np.float64:
        errs = (rel_err(m, m_ref), rel_err(C, C_ref), rel_err(S, S_ref), abs(ent - ent_ref) / max(abs(ent_ref), 1.0))
        print(f"[wass f64] {kind} {d} eta {eta}: m {errs[0]:.1e} C {errs[1]:.1e} Sigma {errs[2]:.1e} entropy {errs[3]:.1e}")
        assert errs[0] <= TOL64[0] and max(errs[1:]) <= TOL64[1]
    else:
        m_y, C_y, S_y = _reference(dtype, kind, d, eta, yard=True)
        _hold(f"{kind} eta {eta} m", d, m, m_y, m_ref)
        _hold(f"{kind} eta {eta} C", d, C, C_y, C_ref)
        _hold(f"{kind} eta {eta} Sigma", d, S, S_y, S_ref)
        print(f"[wass f32] {kind} {d} eta {eta}: entropy {abs(float(ent) - ent_ref) / max(abs(ent_ref), 1.0):.1e}")
        assert abs(float(ent) - ent_ref) <= VALUE_RTOL * max(abs(ent_ref), 1.0)


@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("d", [10, 65])
def test_update_with_a_singular_m(d, eta):
    """M = I + eta H' singular: finite, no sticky flag (the synchronize of _device_update would raise), a positive diagonal, and within ten
    times the two CPU forms' distance on this fixture, floored at TOL64."""
    m, C, S, _ = _device_update(np.float64, "singular", d, eta)
    m_ref, C_ref, S_ref = _reference(np.float64, "singular", d, eta)
    m_it, C_it, S_it, rounds = _reference(np.float64, "singular", d, eta, update=R.update_iterated)
    disc = (rel_err(m_it, m_ref), rel_err(C_it, C_ref), rel_err(S_it, S_ref))
    errs = (rel_err(m, m_ref), rel_err(C, C_ref), rel_err(S, S_ref))
    tols = tuple(max(10.0 * x, t) for x, t in zip(disc, (TOL64[0], TOL64[1], TOL64[1])))
    print(f"[wass singular] {d} eta {eta} ({rounds} rounds on the CPU): m {errs[0]:.1e} C {errs[1]:.1e} ({tols[1]:.1e}) Sigma {errs[2]:.1e} ({tols[2]:.1e})")
    assert all(e <= t for e, t in zip(errs, tols))


@DTYPES
@pytest.mark.parametrize("d", DS)
def test_state_and_repeatability(d, dtype):
    """The state's triangles are bitwise mirrored, C' C'' reproduces it, a second run gives the same bits and the _host form equals the
    device form."""
    eta = 0.1
    params, st0, g, H = _case(dtype, "stein", d, eta)
    ctx = _ctx(dtype, d)
    runs = []
    for _ in range(2):
        pd, sd = ctx.to_device(params).clone(), ctx.to_device(st0).clone()
        ent = ctx.wass_update(pd, sd, ctx.to_device(g), ctx.to_device(_flat(H)), eta)
        ctx.synchronize()
        runs.append((pd.cpu().numpy(), sd.cpu().numpy(), ent.cpu().numpy()[0]))
    ph, sh, eh = ctx.wass_update_host(params, st0, g, H, eta)
    ctx.close()
    (p1, s1, e1), (p2, s2, e2) = runs
    assert np.array_equal(p1, p2) and np.array_equal(s1, s2) and e1 == e2
    assert np.array_equal(p1, ph) and np.array_equal(s1, sh) and e1 == eh
    S, C = _mat(s1, d), _f64(_mat(p1[d:], d))
    assert np.array_equal(S, S.T)
    err = rel_err(C @ C.T, _f64(S))
    print(f"[wass state] {d} {np.dtype(dtype).name}: C' C'' against Sigma' {err:.1e}")
    # f32: C' and Sigma' are each rounded once to float32 from float64.  |d(C C'')|_F <= 2 |C|_F |dC|_F <= eps |C|_F^2 = eps tr(Sigma') <=
    # eps sqrt(d) |Sigma'|_F, plus eps / 2 for Sigma' itself
    assert err <= (TOL64[1] if dtype == np.float64 else (np.sqrt(d) + 1.0) * np.finfo(np.float32).eps)


# ---- steps --------------------------------------------------------------------------------------------------------------------------------------------
@DTYPES
@BRANCHES
@pytest.mark.parametrize("d,n", [(5, 10), (65, 64)])
def test_steps_are_the_single_calls_bitwise(d, n, second, dtype):
    ctx, params, _, _ = _dense_ctx(d, n, dtype, second)
    eta, idx = 0.02, 11
    p1 = ctx.to_device(params).clone()
    s1 = ctx.wass_init(p1)
    s0 = s1.clone()
    elbo1 = []
    for t in range(3):
        logpi, g, H = ctx.gauss_expected_grad_hess(p1, idx + t, n, second_order=second)
        elbo1.append((logpi + ctx.wass_update(p1, s1, g, H, eta)).clone())
    p3, s3 = ctx.to_device(params).clone(), s0.clone()
    e3 = ctx.wass_steps(p3, s3, idx, 3, eta, n_samples=n, second_order=second)
    again, s_again = ctx.to_device(params).clone(), s0.clone()
    e_again = ctx.wass_steps(again, s_again, idx, 3, eta, n_samples=n, second_order=second)
    ctx.synchronize()
    assert torch.equal(p1, p3) and torch.equal(s1, s3) and torch.equal(torch.cat(elbo1), e3)        # count = 3 is three {estimator, update}
    assert torch.equal(p3, again) and torch.equal(s3, s_again) and torch.equal(e3, e_again)            # and two runs agree bit for bit
    assert not torch.equal(p3, ctx.to_device(params)) and bool(torch.isfinite(e3).all())
    ctx.close()


@BRANCHES
@pytest.mark.parametrize("model", ["reference", "dense"])
def test_trajectory_f64(model, second):
    ctx, d, n, eta, params, q_o, tgt = _trajectory_case(model, np.float64, second)
    T, idx0 = 10, 5
    p = ctx.to_device(params).clone()
    st = ctx.wass_init(p)
    draws = [ctx.sample(p, idx0 + t)[1].cpu().numpy().copy() for t in range(T)]   # eps is a function of (seed, index) alone
    elbo = ctx.wass_steps(p, st, idx0, T, eta, n_samples=n, second_order=second)
    ctx.synchronize()
    elbo = elbo.cpu().numpy()
    q_a, S_a, elbo_a = R.steps(q_o, tgt, draws, eta, second, update=R.update_literal)
    q_b, S_b, _ = R.steps(q_o, tgt, draws, eta, second, update=R.update_iterated)
    disc = max(rel_err(O.destructure(q_b), O.destructure(q_a)), rel_err(S_b, S_a))
    tol = max(10.0 * disc, TOL64[1])
    errs = (rel_err(p.cpu().numpy(), O.destructure(q_a)), rel_err(_mat(st.cpu().numpy(), d), S_a),
            float(np.max(np.abs(elbo - np.array(elbo_a)) / np.abs(elbo_a))))
    print(f"[wass trajectory] {model} second={second}: params {errs[0]:.1e} Sigma {errs[1]:.1e} elbo {errs[2]:.1e} (tolerance {tol:.1e})")
    assert max(errs) <= tol
    ctx.close()


# ---- the algorithm's surface (test/algorithms/klminwassfwdbwd.jl) -----------------------------------------------------------------------------------
def _alg(**kw):
    return avi.KLMinWassFwdBwd(stepsize=kw.pop("stepsize", 1e-3), n_samples=10, **kw)


def test_callback_iterations():
    _, prob, _, q0 = _reference_model(np.float64, 2)
    seen = []

    def callback(rng, iteration, q, info):
        seen.append((iteration, q.location.copy(), info["elbo"]))
        return {"iteration_check": iteration, "elbo": "shadowed"}

    q, info, _ = avi.optimize(_alg(), 10, prob, q0, callback=callback)
    assert [i["iteration_check"] for i in info] == list(range(1, 11)) == [s[0] for s in seen]
    assert all(isinstance(i["elbo"], float) and np.isfinite(i["elbo"]) for i in info)   # merge(info', info): the step's own entries win
    assert not np.array_equal(seen[0][1], q0.location) and np.array_equal(seen[-1][1], q.location)   # q: the NEW iterate (:118)


def test_estimate_objective_at_the_target():
    d, prob, _, _ = _reference_model(np.float64, 2)
    q_true = avi.FullRankGaussian(np.full(d, 5.0), 0.3 * np.eye(d))
    assert np.isfinite(avi.estimate_objective(_alg(), q_true, prob))
    assert abs(avi.estimate_objective(avi.PhiloxRNG(SEED), _alg(), q_true, prob, n_samples=10 ** 5)) <= 1e-2


@pytest.mark.parametrize("order", [1, 2])
def test_determinism_and_routes(order):
    _, prob, _, q0 = _reference_model(np.float64, order)
    alg = _alg()
    q1, info1, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 20, prob, q0)
    q2, info2, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 20, prob, q0)
    assert np.array_equal(q1.location, q2.location) and np.array_equal(q1.scale, q2.scale)
    q3, info3, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 20, prob, q0, device_loop=False)             # the host-driven `step` loop
    assert np.array_equal(q1.location, q3.location) and np.array_equal(q1.scale, q3.scale)
    assert [i["elbo"] for i in info1] == [i["elbo"] for i in info3] == [i["elbo"] for i in info2]
    assert [i["iteration"] for i in info1] == list(range(1, 21))
    rng = avi.PhiloxRNG(SEED)                                                                            # warm start: 12 + 8 = 20
    _, _, st12 = avi.optimize(rng, alg, 12, prob, q0)
    p12, s12 = st12["params"].clone(), st12["wass"].clone()
    q4, info4, st = avi.optimize(rng, alg, 8, prob, q0, state=st12)
    assert torch.equal(st12["params"], p12) and torch.equal(st12["wass"], s12) and st12["iteration"] == 12   # the caller's state is left as it was
    assert st["iteration"] == 20 and [i["iteration"] for i in info4] == list(range(1, 9))
    assert np.array_equal(q1.location, q4.location) and np.array_equal(q1.scale, q4.scale)
    rng = avi.PhiloxRNG(SEED)                                                                            # ... on either route
    _, _, st12 = avi.optimize(rng, alg, 12, prob, q0, device_loop=False)
    q5, _, _ = avi.optimize(rng, alg, 8, prob, q0, state=st12, device_loop=False)
    assert np.array_equal(q1.location, q5.location) and np.array_equal(q1.scale, q5.scale)


def test_low_capability_raises():
    class Order0:
        def dimension(self):
            return 5

        def logdensity(self, z):
            return -0.5 * float(np.sum((np.asarray(z) - 5.0) ** 2))

        def capabilities(self):
            return avi.LogDensityOrder(0)

    _, _, _, q0 = _reference_model(np.float64, 1)
    with pytest.raises(ValueError, match="first-order"):
        avi.optimize(_alg(stepsize=1.0), 1, Order0(), q0)


@DTYPES
@pytest.mark.parametrize("order", [1, 2])
def test_output_dtype(order, dtype):
    _, prob, _, q0 = _reference_model(dtype, order)
    q, info, _ = avi.optimize(_alg(), 10, prob, q0)
    assert q.location.dtype == dtype and q.scale.dtype == dtype and len(info) == 10
    assert np.all(np.triu(q.scale, 1) == 0.0) and np.all(np.diag(q.scale) > 0.0)


@pytest.mark.parametrize("order", [1, 2])
def test_convergence(order):
    """test/algorithms/klminwassfwdbwd.jl:77-90 (the reference asks 1/2 of the initial distance, this project 0.1)"""
    d, prob, _, q0 = _reference_model(np.float64, order)
    q, info, _ = avi.optimize(avi.PhiloxRNG(SEED), _alg(), 1000, prob, q0)
    mu_true, L_true = np.full(d, 5.0), 0.3 * np.eye(d)
    d0 = np.sum((q0.location - mu_true) ** 2) + np.sum((q0.scale - L_true) ** 2)
    dl = np.sum((q.location - mu_true) ** 2) + np.sum((q.scale - L_true) ** 2)
    print(f"[wass convergence] order {order}: ratio {dl / d0:.1e}")
    assert len(info) == 1000 and dl <= 0.1 * d0


def test_subsampling_determinism_and_one_step():
    prob = _logreg(1)
    d = prob.dimension()
    q0 = avi.FullRankGaussian(np.zeros(d), np.eye(d))
    sub = avi.ReshufflingBatchSubsampling(np.arange(8), 3)
    alg = _alg(stepsize=1e-2, subsampling=sub)
    q1, info1, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 10, prob, q0)
    q2, info2, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 10, prob, q0)
    assert np.array_equal(q1.location, q2.location) and np.array_equal(q1.scale, q2.scale)
    assert [i["elbo"] for i in info1] == [i["elbo"] for i in info2]
    assert all("epoch" in i and "step" in i for i in info1)
    assert np.isfinite(avi.estimate_objective(avi.PhiloxRNG(SEED), alg, q0, prob, n_samples=100))
    # one step = the estimator on the rows the subsampling selects + the update
    rng = avi.PhiloxRNG(SEED)
    state = avi.init(rng, alg, q0, prob)
    state, _, info = avi.step(rng, alg, state, None)
    replay = avi.PhiloxRNG(SEED)
    batch, _, sub_inf = SUB.step_subsampling(replay, sub, SUB.init_subsampling(replay, sub))
    assert info["epoch"] == sub_inf["epoch"] and info["step"] == sub_inf["step"]
    ctx = avi.MiviContext(np.float64, avi.FULLRANK, d, 10, 0, SEED)
    ctx.set_problem(avi.subsample(prob, batch))
    p = ctx.to_device(avi.destructure(q0)[0]).clone()
    st = ctx.wass_init(p)
    logpi, g, H = ctx.gauss_expected_grad_hess(p, replay.next_index(), 10, second_order=False)
    ent = ctx.wass_update(p, st, g, H, 1e-2)
    ctx.synchronize()
    assert torch.equal(p, state["params"]) and torch.equal(st, state["wass"]) and float((logpi + ent).item()) == info["elbo"]
    assert replay.counter == rng.counter
    ctx.close()


def test_subsampling_convergence():
    """test/algorithms/klminwassfwdbwd.jl:138-156 on test/models/subsamplednormals.jl (restated in tests/natgrad_ref.py): batch size 1,
    stepsize 1e-3, 10 samples, T = 1000; the posterior is N(mean(mus), 1 / n_data).  The reference's bound is 1/2 of the initial distance;
    the device's run is also held to the float64 restatement driven by the SAME batches and draws (the trajectories' rule)."""
    n_data, T, n = 8, 1000, 10
    model = NR.SubsampledNormals(np.random.default_rng(3).normal(size=n_data))
    mu_true, L_true = np.array([model.mus.mean()]), np.array([[np.sqrt(1.0 / n_data)]])
    q0 = avi.FullRankGaussian(np.zeros(1), np.eye(1))
    sub = avi.ReshufflingBatchSubsampling(np.arange(n_data), 1)
    alg = _alg(subsampling=sub)
    q, info, state = avi.optimize(avi.PhiloxRNG(SEED), alg, T, model, q0)
    d0 = np.sum((q0.location - mu_true) ** 2) + np.sum((q0.scale - L_true) ** 2)
    dl = np.sum((q.location - mu_true) ** 2) + np.sum((q.scale - L_true) ** 2)
    ctx, p0 = state["ctx"], state["params"]
    ends = []
    for update in (R.update_literal, R.update_iterated):
        rp = avi.PhiloxRNG(SEED)                                             # replays the batches and the estimate indices the run saw
        st = SUB.init_subsampling(rp, sub)
        qo, Sigma = O.MvLocationScale(np.zeros(1), np.eye(1)), np.eye(1)
        for t in range(T):
            batch, st, _ = SUB.step_subsampling(rp, sub, st)
            u = _f64(ctx.sample(p0, rp.next_index())[1].cpu().numpy())
            _, g, H = O.gaussian_expectation_gradient_and_hessian(qo, model.subsample(batch), u)
            m_new, C_new, Sigma = update(qo.location, Sigma, g, H, alg.stepsize)[:3]
            qo = O.MvLocationScale(m_new, C_new)
        ends.append(qo)
    q_a, q_b = ends
    tol = max(10.0 * max(rel_err(q_b.location, q_a.location), rel_err(q_b.scale, q_a.scale)), TOL64[1])
    errs = (rel_err(q.location, q_a.location), rel_err(q.scale, q_a.scale))
    ref_ratio = (np.sum((q_a.location - mu_true) ** 2) + np.sum((q_a.scale - L_true) ** 2)) / d0
    print(f"[wass subsampling convergence] ratio {dl / d0:.4f} (restatement {ref_ratio:.4f}); m {errs[0]:.1e} C {errs[1]:.1e} (tolerance {tol:.1e})")
    assert len(info) == T and max(errs) <= tol
    assert dl <= 0.5 * d0


# ---- refusals and the failure path ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    d, n = 6, 4
    rng = np.random.default_rng(5)
    prob, _ = make_problem(rng, "diag", d)
    mf = avi.MiviContext(np.float64, avi.MEANFIELD, d, n, 0, SEED)
    mf.set_problem(prob)
    pm = mf.to_device(np.concatenate([np.zeros(d), np.ones(d)])).clone()
    sm = mf.to_device(np.arange(1.0 * d * d)).clone()
    assert _refused(lambda: mf.wass_steps(pm, sm, 0, 1, 0.1)) == 6
    assert _refused(lambda: mf.wass_update(pm, sm, mf.empty(d), mf.empty(d * d), 0.1)) == 6
    assert _refused(lambda: mf.wass_init(pm, sm)) == 6
    mf.synchronize()
    assert np.array_equal(sm.cpu().numpy(), np.arange(1.0 * d * d)) and np.array_equal(pm.cpu().numpy()[d:], np.ones(d))
    mf.close()
    q, _ = make_family(rng, d, avi.FULLRANK)
    params, _ = avi.destructure(q)

    def untouched(ctx, call, status):
        p = ctx.to_device(params).clone()
        st = ctx.wass_init(p)
        st0 = st.clone()
        assert _refused(lambda: call(p, st)) == status
        ctx.synchronize()
        assert np.array_equal(p.cpu().numpy(), params) and torch.equal(st, st0)   # refused before anything ran
        return p, st

    shard = avi.MiviContext(np.float64, avi.FULLRANK, d, n, 0, SEED, m_offset=n, m_total=2 * n)
    shard.set_problem(prob)
    untouched(shard, lambda p, st: shard.wass_steps(p, st, 0, 1, 0.1), 6)
    shard.close()
    bare = avi.MiviContext(np.float64, avi.FULLRANK, d, n, 0, SEED)
    untouched(bare, lambda p, st: bare.wass_steps(p, st, 0, 1, 0.1), 5)                    # no target
    bare.close()
    order1 = NR.SubsampledNormals(np.arange(3.0))                                           # second order without a Hessian (a gradient-only plugin)
    first = avi.MiviContext(np.float64, avi.FULLRANK, order1.dimension(), n, 0, SEED)
    first.set_problem(order1)
    q3, _ = make_family(rng, order1.dimension(), avi.FULLRANK)
    p3 = first.to_device(avi.destructure(q3)[0]).clone()
    s3 = first.wass_init(p3)
    p3_0, s3_0 = p3.clone(), s3.clone()
    assert _refused(lambda: first.wass_steps(p3, s3, 0, 2, 0.1, second_order=True)) == 6
    first.synchronize()
    assert torch.equal(p3, p3_0) and torch.equal(s3, s3_0)
    elbo = first.wass_steps(p3, s3, 0, 2, 1e-3)                                             # the first-order branch works there
    first.synchronize()
    assert bool(torch.isfinite(elbo).all())
    first.close()


@pytest.mark.parametrize("d", [5, 70])
def test_a_nan_hessian_is_a_status(d):
    """A NaN in H: |E_0|_F is not a number, the iteration stops itself there and sets the sticky flag of MIVI_ERR_NONFINITE; no pivot of the
    NaN Sigma' is a number either, which sets that of MIVI_ERR_NONPOSITIVE_SCALE, the one a status read reports first.  The call returns,
    nothing loops; a following valid update on fresh buffers is correct."""
    eta = 0.1
    params, st0, g, H = _case(np.float64, "second", d, eta)
    bad = H.copy()
    bad[d // 2, 1] = np.nan
    ctx = _ctx(np.float64, d)
    p, st = ctx.to_device(params).clone(), ctx.to_device(st0).clone()
    ctx.wass_update(p, st, ctx.to_device(g), ctx.to_device(_flat(bad)), eta)
    assert _refused(ctx.synchronize) in (2, 3)
    ctx.synchronize()                                                        # the flag is cleared by the read
    assert _refused(lambda: ctx.wass_update_host(params, st0, g, bad, eta)) in (2, 3)
    p2, st2 = ctx.to_device(params).clone(), ctx.to_device(st0).clone()
    ctx.wass_update(p2, st2, ctx.to_device(g), ctx.to_device(_flat(H)), eta)
    ctx.synchronize()
    m_ref, C_ref, S_ref = _reference(np.float64, "second", d, eta)
    got = p2.cpu().numpy()
    assert rel_err(got[:d], m_ref) <= TOL64[0] and rel_err(_mat(got[d:], d), C_ref) <= TOL64[1] and rel_err(_mat(st2.cpu().numpy(), d), S_ref) <= TOL64[1]
    ctx.close()
