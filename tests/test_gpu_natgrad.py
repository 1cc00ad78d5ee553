"""KLMinNaturalGradDescent on the device (src/algorithms/klminnaturalgraddescent.jl): the state and update kernels of csrc/kernels_natgrad.hip
against the numpy restatement tests/natgrad_ref.py, the fused steps of mivi_natgrad_steps against the single calls, trajectories against the
restatement driven by the device's own draws, the algorithm's surface (mirroring test/algorithms/klminnaturalgraddescent.jl), the refusals and
the failure path.

Kernels by size: d <= avi.NATGRAD_SMALL_D (44) the one-workgroup kernel; above it 64 x 64 tiles in one to four panels -- so the sizes cover
44 | 45, 63 | 64 | 65, 127 .. 130, 192 and 256.

Criteria.  f64: relative l2 1e-12 on m', 1e-11 on C', S', Sigma' and the entropy (tests/test_gpu_parity.py TOL[np.float64]) on inputs with
kappa(S') about 15.  The spd4 class, kappa(S') = 1e8, is held to d kappa_2(S') 2^-53: the first-order bound on the Cholesky factor of a matrix
known to d x unit roundoff (Higham, Accuracy and Stability of Numerical Algorithms, sections 10.1 and 10.3: backward error gamma_d, factor
sensitivity kappa_2), the criterion of this project for a factorisation of an ill-conditioned matrix in float64.  f32: both numbers of
tests/solve_ref.block_ratios(got, yard, ref64, d) -- yard = natgrad_ref in float32 (lower_scale for C'), ref64 = natgrad_ref in float64, both
on the f32-stored inputs -- at most F32_FACTOR = 8 (tests/test_gpu_solve_yardstick.py) for each of m', C', S', Sigma'; values (elbo,
entropy) relative 1e-5.  H = -C^-T (I + 0.3 N / sqrt(d)) C^-1: congruent with the precision, which keeps the upper-mirrored S' positive
definite; symmetric N for the spd2 / spd4 / ar999 classes, where the reference itself throws on a non-symmetric one.
Trajectories (f64): 1e-10 on parameters, state and elbo after 10 steps.

The one-workgroup kernel computes in the context's type; the tile path computes in float64 for either type (S' rounded to float32 would
leave C' kappa(S') x 6e-8 from the exact result, more than 8 distances of the float32 restatement on the ar999 class whatever the order of
the sums).  A float32 numpy emulation of the tile kernels' documented order (tests/natgrad_ref.emulate_tiles) is exact in float64; see
tests/test_natgrad_ref_host.py.

Worst ratios measured on the MI355X (whole, worst 64-row block), over m', C', S', Sigma':
    init and update, random H, every size, both rules (both kernels)   3.65  3.65   (Sigma' at d = 2, the one-workgroup kernel in float32)
    conditioning classes at d = 70 / 256 (tile path)                   default 0.52 0.57   graded 0.37 0.60   spd2 0.52 0.52   ar999 0.40 0.55
    one step of a trajectory (d = 5 and d = 33, one-workgroup kernel)  1.23  1.23   (C', dense33 Stein)
    f64, every size: m' 2.6e-16, C' 2.4e-16, entropy 2.2e-16, state 6.6e-16 relative l2; spd4: m' 8.9e-8, C' 8.3e-7
    f64 trajectories after 10 steps: parameters 2.7e-16, state 4.1e-16, elbo 8.8e-16
    convergence (T = 1000): 0.0016 (first order), 0.0027 (second order), 0.0015 (subsampling, batch size 1) of the initial distance; bound 0.1"""
import functools

import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import subsampling as SUB
from oracle import oracle as O
from tests import natgrad_ref as R
from tests.helpers import SEED, make_family, make_problem, rel_err
from tests.measure_space_cases import DTYPES, TOL64, VALUE_RTOL
from tests.measure_space_cases import dense_ctx as _dense_ctx, flat as _flat, logreg as _logreg, reference_model as _reference_model
from tests.measure_space_cases import hold, refused as _refused, trajectory_case as _trajectory_case

pytestmark = pytest.mark.gpu
_hold = functools.partial(hold, "natgrad")

SIZES = (1, 2, 5, 10, 31, 32, 33, 48, 49, 63, 64, 65, 127, 128, 129, 130, 192, 256, avi.NATGRAD_SMALL_D, avi.NATGRAD_SMALL_D + 1)
RULES = pytest.mark.parametrize("ensure", [True, False], ids=["ensure", "plain"])


def _mat(v, d):
    return np.asarray(v).reshape(d, d, order="F")


def _check_state(what, dtype, d, got, ref, yard, tol64=TOL64[1]):
    """[S; Sigma] of the device against the restatement's (S, Sigma) pairs; both bitwise symmetric."""
    for name, k in (("S", 0), ("Sigma", 1)):
        M = _mat(got[k * d * d:(k + 1) * d * d], d)
        assert np.array_equal(M, M.T), (what, name)
        if dtype == np.float64:
            print(f"[natgrad f64] {what} {d} {name}: {rel_err(M, ref[k]):.1e}")
            assert rel_err(M, ref[k]) <= tol64, (what, name)
        else:
            _hold(f"{what} {name}", d, M, yard[k], ref[k])


@functools.lru_cache(maxsize=None)
def _init_on_device(dtype, d, seed_kind):
    """(params, S0, Sigma0, state0) with the state from mivi_natgrad_init, checked against the restatement once per input."""
    if isinstance(seed_kind, str):
        m, C, _, _ = R.conditioning_case(seed_kind, d, dtype)
        q = avi.FullRankGaussian(m, C)
    else:
        q, _ = make_family(np.random.default_rng(seed_kind), d, avi.FULLRANK, dtype)
    params, _ = avi.destructure(q)
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, 1, 0, SEED)
    pd = ctx.to_device(params).clone()
    st0 = ctx.natgrad_init(pd).cpu().numpy().copy()
    ctx.synchronize()
    assert np.array_equal(pd.cpu().numpy(), params)                        # init only reads the parameters
    ctx.close()
    return params, _mat(st0[:d * d], d), _mat(st0[d * d:], d), st0


def _device_update(dtype, d, params, st0, g, H, eta, ensure):
    """(params', state', entropy) of mivi_natgrad_update; asserts g and H come back bit-identical and the _host form equals the device form."""
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, 1, 0, SEED)
    pd, sd, gd, Hd = ctx.to_device(params).clone(), ctx.to_device(st0).clone(), ctx.to_device(g), ctx.to_device(_flat(H))
    ent = ctx.natgrad_update(pd, sd, gd, Hd, eta, ensure)
    ctx.synchronize()
    assert np.array_equal(gd.cpu().numpy(), g) and np.array_equal(Hd.cpu().numpy(), _flat(H))
    ph, sh, eh = ctx.natgrad_update_host(params, st0, g, H, eta, ensure)
    got, st, ent = pd.cpu().numpy(), sd.cpu().numpy(), ent.cpu().numpy()[0]
    ctx.close()
    assert got.dtype == dtype and st.dtype == dtype
    assert np.array_equal(got, ph) and np.array_equal(st, sh) and ent == eh
    return got, st, ent


def _check_update(what, dtype, d, params, S0, P0, st0, g, H, eta, ensure, tol64=TOL64, value=True):
    got, st, ent = _device_update(dtype, d, params, st0, g, H, eta, ensure)
    C_got = _mat(got[d:], d)
    assert np.all(np.triu(C_got, 1) == 0.0)                                 # exact zeros above the diagonal
    m_ref, S_ref, P_ref, _ = R.update(params[:d], S0, P0, g, H, eta, ensure, np.float64)
    C_ref = R.lower_scale(S_ref)
    ent_ref = float(R.entropy(C_ref))
    if dtype == np.float64:
        print(f"[natgrad f64] {what} {d}: m {rel_err(got[:d], m_ref):.1e} C {rel_err(C_got, C_ref):.1e} ent {abs(ent - ent_ref) / abs(ent_ref):.1e}")
        assert rel_err(got[:d], m_ref) <= tol64[0]
        assert rel_err(C_got, C_ref) <= tol64[1]
        assert abs(ent - ent_ref) <= tol64[1] * abs(ent_ref)
        _check_state(what, dtype, d, st, (S_ref, P_ref), None, tol64[1])
    else:
        m_y, S_y, P_y, _ = R.update(params[:d], S0, P0, g, H, eta, ensure, np.float32)
        _hold(f"{what} m", d, got[:d], m_y, m_ref)
        _hold(f"{what} C", d, C_got, R.lower_scale(S_y, np.float32), C_ref)
        _check_state(what, dtype, d, st, (S_ref, P_ref), (S_y, P_y))
        print(f"[natgrad f32] {what} {d}: entropy {abs(float(ent) - ent_ref) / max(abs(ent_ref), 1.0):.1e}")
        assert not value or abs(float(ent) - ent_ref) <= VALUE_RTOL * max(abs(ent_ref), 1.0)


# ---- init and update parity ------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("d", SIZES)
def test_init_matches_restatement(d, dtype):
    params, S0, P0, st0 = _init_on_device(dtype, d, 700 + d)
    C = np.tril(_mat(params[d:], d))
    _check_state("init", dtype, d, st0, R.init_state(C, np.float64), R.init_state(C, np.float32))


@RULES
@DTYPES
@pytest.mark.parametrize("d", SIZES)
def test_update_matches_restatement(d, dtype, ensure):
    params, S0, P0, st0 = _init_on_device(dtype, d, 700 + d)
    rng = np.random.default_rng(800 + d)
    g = rng.normal(size=d).astype(dtype)
    H = R.congruent_hessian(_mat(params[d:], d), rng).astype(dtype)          # random, non-symmetric
    _check_update("random", dtype, d, params, S0, P0, st0, g, H, 0.3, ensure)


@RULES
@pytest.mark.parametrize("eta", [0.1, 0.5])
@pytest.mark.parametrize("d", [70, 256])
@pytest.mark.parametrize("kind", ["default", "graded", "spd2", "ar999"])
def test_update_f32_yardstick_on_every_conditioning(kind, d, eta, ensure):
    _, _, g, H = R.conditioning_case(kind, d, np.float32)
    params, S0, P0, st0 = _init_on_device(np.float32, d, kind)
    # (the yardstick alone: sum log C'_ii moves by kappa(S') x the float32 rounding of S' itself, 0.03 for ar999 -- more than 1e-5 of any entropy)
    _check_update(kind, np.float32, d, params, S0, P0, st0, g, H, eta, ensure, value=False)


@RULES
@pytest.mark.parametrize("eta", [0.1, 0.5])
@pytest.mark.parametrize("d", [70, 256])
def test_update_f64_on_spd4(d, eta, ensure):
    _, _, g, H = R.conditioning_case("spd4", d, np.float64)
    params, S0, P0, st0 = _init_on_device(np.float64, d, "spd4")
    S_ref = R.update(params[:d], S0, P0, g, H, eta, ensure, np.float64)[1]
    tol = d * np.linalg.cond(S_ref) * 2.0 ** -53
    print(f"[natgrad f64] spd4 {d}: kappa(S') {np.linalg.cond(S_ref):.1e} tolerance {tol:.1e}")
    _check_update("spd4", np.float64, d, params, S0, P0, st0, g, H, eta, ensure, (tol, tol))


# ---- fusion and repeatability ----------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("second", [False, True], ids=["stein", "order2"])
@pytest.mark.parametrize("d,n", [(5, 10), (70, 64)])
def test_steps_are_the_single_calls_bitwise(d, n, second, dtype):
    ctx, params, _, _ = _dense_ctx(d, n, dtype, second)
    eta, idx = 0.02, 11
    p1 = ctx.to_device(params).clone()
    s1 = ctx.natgrad_init(p1)
    s0 = s1.clone()
    elbo1 = []
    for t in range(3):
        logpi, g, H = ctx.gauss_expected_grad_hess(p1, idx + t, n, second_order=second)
        elbo1.append((logpi + ctx.natgrad_update(p1, s1, g, H, eta, True)).clone())
    p3, s3 = ctx.to_device(params).clone(), s0.clone()
    e3 = ctx.natgrad_steps(p3, s3, idx, 3, eta, True, n_samples=n, second_order=second)
    again, s_again = ctx.to_device(params).clone(), s0.clone()
    e_again = ctx.natgrad_steps(again, s_again, idx, 3, eta, True, n_samples=n, second_order=second)
    ctx.synchronize()
    assert torch.equal(p1, p3) and torch.equal(s1, s3) and torch.equal(torch.cat(elbo1), e3)        # count = 3 is three {estimator, update}
    assert torch.equal(p3, again) and torch.equal(s3, s_again) and torch.equal(e3, e_again)            # and two runs agree bit for bit
    assert not torch.equal(p3, ctx.to_device(params)) and bool(torch.isfinite(e3).all())
    ctx.close()


# ---- trajectories ------------------------------------------------------------------------------------------------------------------------------
@RULES
@pytest.mark.parametrize("second", [False, True], ids=["stein", "order2"])
@pytest.mark.parametrize("model", ["reference", "dense33"])
def test_trajectory_f64(model, second, ensure):
    ctx, d, n, eta, params, q_o, tgt = _trajectory_case(model, np.float64, second)
    T, idx0 = 10, 5
    p = ctx.to_device(params).clone()
    st = ctx.natgrad_init(p)
    draws = [ctx.sample(p, idx0 + t)[1].cpu().numpy().copy() for t in range(T)]   # eps is a function of (seed, index) alone
    elbo = ctx.natgrad_steps(p, st, idx0, T, eta, ensure, n_samples=n, second_order=second)
    ctx.synchronize()
    elbo = elbo.cpu().numpy()
    q_ref, (S_ref, P_ref), elbo_ref = R.steps(q_o, tgt, draws, eta, second, ensure)
    got, ref, st_h = p.cpu().numpy(), O.destructure(q_ref), st.cpu().numpy()
    errs = (rel_err(got, ref), rel_err(st_h, R.state_flat(S_ref, P_ref)), float(np.max(np.abs(elbo - np.array(elbo_ref)) / np.abs(elbo_ref))))
    print(f"[natgrad trajectory] {model} second={second} ensure={ensure}: params {errs[0]:.1e} state {errs[1]:.1e} elbo {errs[2]:.1e}")
    assert max(errs) <= 1e-10
    ctx.close()


@pytest.mark.parametrize("second", [False, True], ids=["stein", "order2"])
@pytest.mark.parametrize("model", ["reference", "dense33"])
def test_trajectory_f32(model, second):
    """elbo of 10 steps against the float64 restatement from the same f32-stored start; parameters and state after ONE step by the yardstick,
    with the update's inputs (g, H) taken from the device's own estimator call so that the comparison is the update's."""
    ctx, d, n, eta, params, q_o, tgt = _trajectory_case(model, np.float32, second)
    T, idx0 = 10, 5
    p = ctx.to_device(params).clone()
    st = ctx.natgrad_init(p)
    st0 = st.cpu().numpy().copy()
    _, g, H = ctx.gauss_expected_grad_hess(p, idx0, n, second_order=second)
    g, H = g.cpu().numpy().copy(), H.cpu().numpy().copy()
    elbo, draws = [], []
    for t in range(T):
        draws.append(ctx.sample(p, idx0 + t)[1].cpu().numpy().astype(np.float64))
        elbo.append(ctx.natgrad_steps(p, st, idx0 + t, 1, eta, True, n_samples=n, second_order=second).clone())
        if t == 0:
            ctx.synchronize()
            S0, P0 = _mat(st0[:d * d], d), _mat(st0[d * d:], d)
            ref = R.update(params[:d], S0, P0, g, H, eta, True, np.float64)
            yard = R.update(params[:d], S0, P0, g, H, eta, True, np.float32)
            got, st_h = p.cpu().numpy(), st.cpu().numpy()
            _hold(f"one step {model} second={second} m", d, got[:d], yard[0], ref[0])
            _hold(f"one step {model} second={second} C", d, _mat(got[d:], d), R.lower_scale(yard[1], np.float32), R.lower_scale(ref[1]))
            _check_state(f"one step {model} second={second}", np.float32, d, st_h, ref[1:3], yard[1:3])
    ctx.synchronize()
    _, _, elbo_ref = R.steps(q_o, tgt, draws, eta, second, True)
    assert np.max(np.abs(torch.cat(elbo).cpu().numpy() - np.array(elbo_ref)) / np.abs(elbo_ref)) <= VALUE_RTOL
    ctx.close()


# ---- the algorithm's surface (test/algorithms/klminnaturalgraddescent.jl) --------------------------------------------------------------------
def _alg(**kw):
    return avi.KLMinNaturalGradDescent(stepsize=kw.pop("stepsize", 1e-3), n_samples=10, **kw)


def test_callback_iterations():
    _, prob, _, q0 = _reference_model(np.float64, 2)
    seen = []

    def callback(rng, iteration, q, info):
        seen.append((iteration, len(q), info["elbo"]))
        return {"iteration_check": iteration, "elbo": "shadowed"}

    _, info, _ = avi.optimize(_alg(), 10, prob, q0, callback=callback)
    assert [i["iteration_check"] for i in info] == list(range(1, 11)) == [s[0] for s in seen]
    assert all(isinstance(i["elbo"], float) and np.isfinite(i["elbo"]) for i in info)   # merge(info', info): the step's own entries win


def test_estimate_objective_at_the_target():
    d, prob, _, _ = _reference_model(np.float64, 2)
    q_true = avi.FullRankGaussian(np.full(d, 5.0), 0.3 * np.eye(d))
    assert np.isfinite(avi.estimate_objective(_alg(), q_true, prob))
    assert abs(avi.estimate_objective(avi.PhiloxRNG(SEED), _alg(), q_true, prob, n_samples=10 ** 5)) <= 1e-2


@RULES
@pytest.mark.parametrize("order", [1, 2])
def test_determinism_and_routes(order, ensure):
    _, prob, _, q0 = _reference_model(np.float64, order)
    alg = _alg(ensure_posdef=ensure)
    q1, info1, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 20, prob, q0)
    q2, info2, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 20, prob, q0)
    assert np.array_equal(q1.location, q2.location) and np.array_equal(q1.scale, q2.scale)
    q3, info3, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 20, prob, q0, device_loop=False)             # the host-driven `step` loop
    assert np.array_equal(q1.location, q3.location) and np.array_equal(q1.scale, q3.scale)
    assert [i["elbo"] for i in info1] == [i["elbo"] for i in info3] == [i["elbo"] for i in info2]
    assert [i["iteration"] for i in info1] == list(range(1, 21))
    rng = avi.PhiloxRNG(SEED)                                                                            # warm start: 12 + 8 = 20
    _, _, st12 = avi.optimize(rng, alg, 12, prob, q0)
    p12, s12 = st12["params"].clone(), st12["natgrad"].clone()
    q4, info4, st = avi.optimize(rng, alg, 8, prob, q0, state=st12)
    assert torch.equal(st12["params"], p12) and torch.equal(st12["natgrad"], s12) and st12["iteration"] == 12   # the caller's state is left as it was
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
    """test/algorithms/klminnaturalgraddescent.jl:75-90"""
    d, prob, _, q0 = _reference_model(np.float64, order)
    q, info, _ = avi.optimize(avi.PhiloxRNG(SEED), _alg(), 1000, prob, q0)
    mu_true, L_true = np.full(d, 5.0), 0.3 * np.eye(d)
    d0 = np.sum((q0.location - mu_true) ** 2) + np.sum((q0.scale - L_true) ** 2)
    dl = np.sum((q.location - mu_true) ** 2) + np.sum((q.scale - L_true) ** 2)
    print(f"[natgrad convergence] order {order}: ratio {dl / d0:.4f}")
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
    st = ctx.natgrad_init(p)
    logpi, g, H = ctx.gauss_expected_grad_hess(p, replay.next_index(), 10, second_order=False)
    ent = ctx.natgrad_update(p, st, g, H, 1e-2, True)
    ctx.synchronize()
    assert torch.equal(p, state["params"]) and torch.equal(st, state["natgrad"]) and float((logpi + ent).item()) == info["elbo"]
    assert replay.counter == rng.counter
    ctx.close()


def test_subsampling_convergence():
    """test/algorithms/klminnaturalgraddescent.jl:138-156 on test/models/subsamplednormals.jl (restated in tests/natgrad_ref.py):
    batch size 1, stepsize 1e-2, T = 1000; the posterior is N(mean(mus), 1 / n_data)."""
    n_data = 8
    model = R.SubsampledNormals(np.random.default_rng(3).normal(size=n_data))
    mu_true, L_true = np.array([model.mus.mean()]), np.array([[np.sqrt(1.0 / n_data)]])
    q0 = avi.FullRankGaussian(np.zeros(1), np.eye(1))
    alg = _alg(stepsize=1e-2, subsampling=avi.ReshufflingBatchSubsampling(np.arange(n_data), 1))
    q, info, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 1000, model, q0)
    d0 = np.sum((q0.location - mu_true) ** 2) + np.sum((q0.scale - L_true) ** 2)
    dl = np.sum((q.location - mu_true) ** 2) + np.sum((q.scale - L_true) ** 2)
    print(f"[natgrad subsampling convergence] ratio {dl / d0:.4f}")
    assert len(info) == 1000 and dl <= 0.1 * d0


# ---- refusals and the failure path ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    d, n = 6, 4
    rng = np.random.default_rng(5)
    prob, _ = make_problem(rng, "diag", d)
    mf = avi.MiviContext(np.float64, avi.MEANFIELD, d, n, 0, SEED)
    mf.set_problem(prob)
    pm = mf.to_device(np.concatenate([np.zeros(d), np.ones(d)])).clone()
    sm = mf.to_device(np.arange(2.0 * d * d)).clone()
    assert _refused(lambda: mf.natgrad_steps(pm, sm, 0, 1, 0.1)) == 6
    assert _refused(lambda: mf.natgrad_update(pm, sm, mf.empty(d), mf.empty(d * d), 0.1)) == 6
    assert _refused(lambda: mf.natgrad_init(pm, sm)) == 6
    assert np.array_equal(sm.cpu().numpy(), np.arange(2.0 * d * d)) and np.array_equal(pm.cpu().numpy()[d:], np.ones(d))
    mf.close()
    q, _ = make_family(rng, d, avi.FULLRANK)
    params, _ = avi.destructure(q)

    def untouched(ctx, call, status):
        p = ctx.to_device(params).clone()
        st = ctx.natgrad_init(p)
        st0 = st.clone()
        assert _refused(lambda: call(p, st)) == status
        ctx.synchronize()
        assert np.array_equal(p.cpu().numpy(), params) and torch.equal(st, st0)   # refused before anything ran
        return p, st

    shard = avi.MiviContext(np.float64, avi.FULLRANK, d, n, 0, SEED, m_offset=n, m_total=2 * n)
    shard.set_problem(prob)
    untouched(shard, lambda p, st: shard.natgrad_steps(p, st, 0, 1, 0.1), 6)
    shard.close()
    bare = avi.MiviContext(np.float64, avi.FULLRANK, d, n, 0, SEED)
    untouched(bare, lambda p, st: bare.natgrad_steps(p, st, 0, 1, 0.1), 5)                 # no target
    bare.close()
    bij = avi.MiviContext(np.float64, avi.FULLRANK, d, n, 0, SEED)
    bij.set_problem(avi.TransformedProblem(avi.FunnelConstrainedProblem(d, 1.5, order=2), avi.StackedBijector([(0, 1, "exp"), (1, d, "identity")])))
    pb, sb = untouched(bij, lambda p, st: bij.natgrad_steps(p, st, 0, 2, 0.1, second_order=True), 6)   # no Hessian under the bijector
    elbo = bij.natgrad_steps(pb, sb, 0, 2, 1e-3)                                            # the first-order branch works under the bijector
    bij.synchronize()
    assert bool(torch.isfinite(elbo).all())
    bij.close()


@pytest.mark.parametrize("d", [5, 70])
def test_a_precision_that_is_not_positive_definite_is_a_status(d):
    """Plain rule with H = +10 I from q0 = N(0, I): S' = (1 - eta) I - 10 eta I is negative definite -- reported (the reference throws
    PosDefException), nothing faults, and a following valid update on fresh buffers is correct."""
    rng = np.random.default_rng(40 + d)
    q0 = avi.FullRankGaussian(np.zeros(d), np.eye(d))
    params, _ = avi.destructure(q0)
    g, H = rng.normal(size=d), 10.0 * np.eye(d)
    ctx = avi.MiviContext(np.float64, avi.FULLRANK, d, 10, 0, SEED)
    p = ctx.to_device(params).clone()
    st = ctx.natgrad_init(p)
    st0 = st.cpu().numpy().copy()
    ctx.natgrad_update(p, st, ctx.to_device(g), ctx.to_device(_flat(H)), 0.5, False)
    assert _refused(ctx.synchronize) == 3
    ctx.synchronize()                                                       # the flag is cleared by the read
    assert _refused(lambda: ctx.natgrad_update_host(params, st0, g, H, 0.5, False)) == 3
    p2, st2 = ctx.to_device(params).clone(), ctx.to_device(st0).clone()     # fresh buffers, a valid update
    H_ok = R.congruent_hessian(np.eye(d), rng)
    ent = ctx.natgrad_update(p2, st2, ctx.to_device(g), ctx.to_device(_flat(H_ok)), 0.3, False)
    ctx.synchronize()
    m_ref, S_ref, P_ref, _ = R.update(np.zeros(d), np.eye(d), np.eye(d), g, H_ok, 0.3, False)
    C_ref = R.lower_scale(S_ref)
    got = p2.cpu().numpy()
    assert rel_err(got[:d], m_ref) <= TOL64[0] and rel_err(_mat(got[d:], d), C_ref) <= TOL64[1]
    assert rel_err(st2.cpu().numpy(), R.state_flat(S_ref, P_ref)) <= TOL64[1]
    assert abs(float(ent.item()) - float(R.entropy(C_ref))) <= TOL64[1] * abs(float(R.entropy(C_ref)))
    ctx.close()
