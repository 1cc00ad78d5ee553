"""KLMinSqrtNaturalGradDescent on the device (src/algorithms/klminsqrtnaturalgraddescent.jl): the update kernels of csrc/kernels_ngd.hip
against the numpy restatement tests/ngd_ref.py, the fused steps of mivi_sqrt_ngd_steps against the single calls, trajectories against the
restatement driven by the device's own draws, the algorithm's surface (mirroring test/algorithms/klminsqrtnaturalgraddescent.jl) and the refusals.

Kernels by size: d <= 48 the one-workgroup kernel; above it 64 x 64 tiles -- so the sizes cover 48 | 49 and 63 | 64 | 65, 128 | 129 | 130.

Criteria.  f64: relative l2 1e-12 on m', 1e-11 on C' and the entropy (tests/test_gpu_parity.py TOL[np.float64]).  f32: both numbers of
tests/solve_ref.block_ratios(got, yard, ref64, d) -- yard = ngd_ref in float32, ref64 = ngd_ref in float64, both on the f32-stored inputs -- at most
F32_FACTOR = 8 (tests/test_gpu_solve_yardstick.py), over every solve_ref.KINDS scale matrix at d = 70 and d = 256 with H = -(P + 0.3 mean|P| N),
P = (C C')^-1; values (elbo, entropy) relative 1e-5.  Trajectories (f64): 1e-10 on parameters and elbo after 10 steps.

Worst ratios measured on the MI355X (whole, worst 64-row block):
    case                                                          whole   worst block   (worst case)
    update, conditioning classes at d = 70 / 256 (tile kernels)   1.44    1.92          (spd2 70 whole, ar999 256 per block)
        default 0.50 0.58 / 0.53 0.66    spd2 1.44 1.46 / 1.24 1.31    spd4 1.26 1.28 / 1.17 1.20    ar999 0.67 1.06 / 1.43 1.92    graded 1.29 1.58 / 1.12 1.23
    update, random H, every size (both kernels)                   1.02    1.44          (d = 65 whole, d = 129 per block)
    one step of a trajectory (d = 5 one-workgroup, d = 33 tiles)  0.50    0.95          (dense33 Stein whole, reference model per block)
    f64: m' 6.2e-17, C' 6.4e-16, entropy 2.2e-16 relative l2; trajectories after 10 steps: parameters 1.1e-16, elbo 5.2e-16
    convergence (T = 1000): 0.0019 (first order) and 0.0026 (second order) of the initial distance, against the bound 0.1
A float32 numpy emulation of the kernels' order -- C'((-H)C), every product summed in 32-wide K blocks, the matvecs accumulated in float64 --
gives at most 1.39 (whole) and 1.59 (worst block) on the ten conditioning cases, so the factor 8 is admissible for this algorithm."""
import functools
import zlib

import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import subsampling as SUB
from advancedvi_jl_amd._lib import MiviError
from oracle import oracle as O
from tests import ngd_ref as N
from tests import solve_ref as S
from tests.helpers import SEED, make_family, make_problem, rel_err
from tests.measure_space_cases import DTYPES, TOL64, VALUE_RTOL
from tests.measure_space_cases import dense_ctx as _dense_ctx, flat as _flat, logreg as _logreg, reference_model as _reference_model
from tests.measure_space_cases import hold, refused as _refused, trajectory_case as _trajectory_case

pytestmark = pytest.mark.gpu
_hold = functools.partial(hold, "ngd")

SIZES = (1, 2, 5, 31, 32, 33, 48, 49, 63, 64, 65, 128, 129, 130, 256)


def _device_update(dtype, d, params, g, H, eta):
    """(params', entropy, host-form params', host-form entropy) of mivi_sqrt_ngd_update[_host]; asserts g and H come back bit-identical."""
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, 1, 0, SEED)
    pd, gd, Hd = ctx.to_device(params).clone(), ctx.to_device(g), ctx.to_device(_flat(H))
    ent = ctx.sqrt_ngd_update(pd, gd, Hd, eta)
    ctx.synchronize()
    assert np.array_equal(gd.cpu().numpy(), g) and np.array_equal(Hd.cpu().numpy(), _flat(H))
    ph, eh = ctx.sqrt_ngd_update_host(params, g, H, eta)
    out = pd.cpu().numpy(), ent.cpu().numpy()[0], ph, eh
    ctx.close()
    return out


def _check_update(what, dtype, d, params, g, H, eta):
    got, ent, got_h, ent_h = _device_update(dtype, d, params, g, H, eta)
    assert got.dtype == dtype
    assert np.array_equal(got, got_h) and ent == ent_h                      # the _host form is the device form
    assert np.all(np.triu(got[d:].reshape(d, d, order="F"), 1) == 0.0)      # exact zeros above the diagonal
    ref, ent_ref = N.update_flat(params, g, H, eta, np.float64)
    if dtype == np.float64:
        print(f"[ngd f64] {what} {d}: m {rel_err(got[:d], ref[:d]):.1e} C {rel_err(got[d:], ref[d:]):.1e} ent {abs(ent - ent_ref) / abs(ent_ref):.1e}")
        assert rel_err(got[:d], ref[:d]) <= TOL64[0]
        assert rel_err(got[d:], ref[d:]) <= TOL64[1]
        assert abs(ent - ent_ref) <= TOL64[1] * abs(ent_ref)
    else:
        yard, _ = N.update_flat(params, g, H, eta, np.float32)
        _hold(what, d, got, yard, ref)
        assert abs(float(ent) - float(ent_ref)) <= VALUE_RTOL * max(abs(float(ent_ref)), 1.0)


# ---- update parity ---------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("d", SIZES)
def test_update_matches_restatement(d, dtype):
    rng = np.random.default_rng(700 + d)
    q, _ = make_family(rng, d, avi.FULLRANK, dtype)
    params, _ = avi.destructure(q)
    g = rng.normal(size=d).astype(dtype)
    H = (rng.normal(size=(d, d)) - np.eye(d)).astype(dtype)   # random, non-symmetric
    _check_update("random", dtype, d, params, g, H, 0.05)


@pytest.mark.parametrize("d", [70, 256])
@pytest.mark.parametrize("kind", S.KINDS)
def test_update_f32_yardstick_on_every_conditioning(kind, d):
    rng = np.random.default_rng(zlib.crc32(kind.encode()) + d)
    C = S.scale_matrix(kind, d, rng).astype(np.float32)
    mu = rng.normal(size=d).astype(np.float32)
    params, _ = avi.destructure(avi.FullRankGaussian(mu, C))
    P = np.linalg.inv(C.astype(np.float64) @ C.astype(np.float64).T)
    H = (-(P + 0.3 * np.mean(np.abs(P)) * rng.normal(size=(d, d)))).astype(np.float32)
    g = rng.normal(size=d).astype(np.float32)
    # (at this step size the update itself -- the float64 restatement too -- takes some C'_ii of the ill-conditioned classes below zero: the
    # sticky flag is then the correct answer, it must agree with the result's own diagonal, and the yardstick is held all the same)
    ctx = avi.MiviContext(np.float32, avi.FULLRANK, d, 1, 0, SEED)
    pd = ctx.to_device(params).clone()
    ctx.sqrt_ngd_update(pd, ctx.to_device(g), ctx.to_device(_flat(H)), 0.1)
    try:
        ctx.synchronize()
        flagged = False
    except MiviError as e:
        assert e.status == 3
        flagged = True
    got = pd.cpu().numpy()
    ctx.close()
    assert flagged == bool(np.any(np.diag(got[d:].reshape(d, d, order="F")) <= 0.0))
    assert np.all(np.triu(got[d:].reshape(d, d, order="F"), 1) == 0.0)
    ref, _ = N.update_flat(params, g, H, 0.1, np.float64)
    yard, _ = N.update_flat(params, g, H, 0.1, np.float32)
    _hold(kind, d, got, yard, ref)


# ---- fusion and repeatability ----------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("second", [False, True], ids=["stein", "order2"])
@pytest.mark.parametrize("d,n", [(33, 17), (256, 64)])
def test_steps_are_the_single_calls_bitwise(d, n, second, dtype):
    ctx, params, _, _ = _dense_ctx(d, n, dtype, second)
    eta, idx = 0.05, 11
    p1 = ctx.to_device(params).clone()
    logpi, g, H = ctx.gauss_expected_grad_hess(p1, idx, n, second_order=second)
    ent = ctx.sqrt_ngd_update(p1, g, H, eta)
    elbo1 = logpi + ent
    p2 = ctx.to_device(params).clone()
    elbo2 = ctx.sqrt_ngd_steps(p2, idx, 1, eta, n_samples=n, second_order=second)
    ctx.synchronize()
    assert torch.equal(p1, p2) and torch.equal(elbo1, elbo2)                  # count = 1 is estimator + update
    assert not torch.equal(p2, ctx.to_device(params)) and bool(torch.isfinite(elbo2).all())
    p6 = ctx.to_device(params).clone()
    e6 = ctx.sqrt_ngd_steps(p6, idx, 6, eta, n_samples=n, second_order=second)
    p1x6 = ctx.to_device(params).clone()
    e1x6 = torch.cat([ctx.sqrt_ngd_steps(p1x6, idx + t, 1, eta, n_samples=n, second_order=second).clone() for t in range(6)])
    again = ctx.to_device(params).clone()
    e_again = ctx.sqrt_ngd_steps(again, idx, 6, eta, n_samples=n, second_order=second)
    ctx.synchronize()
    assert torch.equal(p6, p1x6) and torch.equal(e6, e1x6)                    # count = 6 is six calls
    assert torch.equal(p6, again) and torch.equal(e6, e_again)                # and two runs from one state agree bit for bit
    assert torch.equal(e6[:1], elbo2)
    ctx.close()


# ---- trajectories ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second", [False, True], ids=["stein", "order2"])
@pytest.mark.parametrize("model", ["reference", "dense33"])
def test_trajectory_f64(model, second):
    ctx, d, n, eta, params, q_o, tgt = _trajectory_case(model, np.float64, second)
    T, idx0 = 10, 5
    p = ctx.to_device(params).clone()
    draws = [ctx.sample(p, idx0 + t)[1].cpu().numpy().copy() for t in range(T)]   # eps is a function of (seed, index) alone
    elbo = ctx.sqrt_ngd_steps(p, idx0, T, eta, n_samples=n, second_order=second)
    ctx.synchronize()
    q_ref, elbo_ref = N.steps(q_o, tgt, draws, eta, second)
    got, ref = p.cpu().numpy(), O.destructure(q_ref)
    print(f"[ngd trajectory] {model} second={second}: params {rel_err(got, ref):.1e} elbo {rel_err(elbo.cpu().numpy(), elbo_ref):.1e}")
    assert rel_err(got, ref) <= 1e-10
    assert np.max(np.abs(elbo.cpu().numpy() - np.array(elbo_ref)) / np.abs(elbo_ref)) <= 1e-10
    ctx.close()


@pytest.mark.parametrize("second", [False, True], ids=["stein", "order2"])
@pytest.mark.parametrize("model", ["reference", "dense33"])
def test_trajectory_f32(model, second):
    """elbo of 10 steps against the float64 restatement from the same f32-stored start; the parameters after ONE step by the yardstick, with the
    update's inputs (g, H) taken from the device's own estimator call so that the comparison is the update's."""
    ctx, d, n, eta, params, q_o, tgt = _trajectory_case(model, np.float32, second)
    T, idx0 = 10, 5
    p = ctx.to_device(params).clone()
    draws = [ctx.sample(p, idx0 + t)[1].cpu().numpy().astype(np.float64) for t in range(T)]
    _, g, H = ctx.gauss_expected_grad_hess(p, idx0, n, second_order=second)
    g, H = g.cpu().numpy().copy(), H.cpu().numpy().copy()
    elbo = ctx.sqrt_ngd_steps(p, idx0, 1, eta, n_samples=n, second_order=second).clone()
    ctx.synchronize()
    ref, _ = N.update_flat(params, g, H, eta, np.float64)
    yard, _ = N.update_flat(params, g, H, eta, np.float32)
    _hold(f"one step {model} second={second}", d, p.cpu().numpy(), yard, ref)
    elbo = torch.cat([elbo, ctx.sqrt_ngd_steps(p, idx0 + 1, T - 1, eta, n_samples=n, second_order=second)])
    ctx.synchronize()
    _, elbo_ref = N.steps(q_o, tgt, draws, eta, second)
    assert np.max(np.abs(elbo.cpu().numpy() - np.array(elbo_ref)) / np.abs(elbo_ref)) <= VALUE_RTOL
    ctx.close()


# ---- the algorithm's surface (test/algorithms/klminsqrtnaturalgraddescent.jl) ----------------------------------------------------------------
def _alg(**kw):
    return avi.KLMinSqrtNaturalGradDescent(stepsize=kw.pop("stepsize", 1e-3), n_samples=10, **kw)


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


@pytest.mark.parametrize("order", [1, 2])
def test_determinism_and_routes(order):
    _, prob, _, q0 = _reference_model(np.float64, order)
    q1, info1, _ = avi.optimize(avi.PhiloxRNG(SEED), _alg(), 20, prob, q0)
    q2, info2, _ = avi.optimize(avi.PhiloxRNG(SEED), _alg(), 20, prob, q0)
    assert np.array_equal(q1.location, q2.location) and np.array_equal(q1.scale, q2.scale)
    q3, info3, _ = avi.optimize(avi.PhiloxRNG(SEED), _alg(), 20, prob, q0, device_loop=False)          # the host-driven `step` loop
    assert np.array_equal(q1.location, q3.location) and np.array_equal(q1.scale, q3.scale)
    assert [i["elbo"] for i in info1] == [i["elbo"] for i in info3] == [i["elbo"] for i in info2]
    assert [i["iteration"] for i in info1] == list(range(1, 21))
    rng = avi.PhiloxRNG(SEED)                                                                            # warm start: 12 + 8 = 20
    _, _, st12 = avi.optimize(rng, _alg(), 12, prob, q0)
    p12 = st12["params"].clone()
    q4, info4, st = avi.optimize(rng, _alg(), 8, prob, q0, state=st12)
    assert torch.equal(st12["params"], p12) and st12["iteration"] == 12                                  # the caller's state is left as it was
    assert st["iteration"] == 20 and [i["iteration"] for i in info4] == list(range(1, 9))
    assert np.array_equal(q1.location, q4.location) and np.array_equal(q1.scale, q4.scale)


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
    assert np.all(np.triu(q.scale, 1) == 0.0)


@pytest.mark.parametrize("order", [1, 2])
def test_convergence(order):
    """test/algorithms/klminsqrtnaturalgraddescent.jl:77-90"""
    d, prob, _, q0 = _reference_model(np.float64, order)
    q, info, _ = avi.optimize(avi.PhiloxRNG(SEED), _alg(), 1000, prob, q0)
    mu_true, L_true = np.full(d, 5.0), 0.3 * np.eye(d)
    d0 = np.sum((q0.location - mu_true) ** 2) + np.sum((q0.scale - L_true) ** 2)
    dl = np.sum((q.location - mu_true) ** 2) + np.sum((q.scale - L_true) ** 2)
    print(f"[ngd convergence] order {order}: ratio {dl / d0:.4f}")
    assert len(info) == 1000 and dl <= 0.1 * d0


@pytest.mark.parametrize("order", [1, 2])
def test_subsampling(order):
    prob = _logreg(order)
    d = prob.dimension()
    q0 = avi.FullRankGaussian(np.zeros(d), np.eye(d))
    sub = avi.ReshufflingBatchSubsampling(np.arange(8), 3)
    alg = _alg(stepsize=1e-2, subsampling=sub)
    q1, info1, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 10, prob, q0)
    q2, info2, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 10, prob, q0)
    if order == 1:
        assert np.array_equal(q1.location, q2.location) and np.array_equal(q1.scale, q2.scale)
        assert [i["elbo"] for i in info1] == [i["elbo"] for i in info2]
    else:
        # the second-order branch of the logistic regression sums its Hessian with f64 atomics (csrc/kernels_hess2.hip, as it did before this
        # algorithm): the estimator, hence the run, repeats to the rounding of a reordered f64 sum, not bit for bit
        assert rel_err(q1.location, q2.location) <= 1e-12 and rel_err(q1.scale, q2.scale) <= 1e-12
        assert rel_err([i["elbo"] for i in info1], [i["elbo"] for i in info2]) <= 1e-12
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
    logpi, g, H = ctx.gauss_expected_grad_hess(p, replay.next_index(), 10, second_order=order == 2)
    ent = ctx.sqrt_ngd_update(p, g, H, 1e-2)
    ctx.synchronize()
    if order == 1:
        assert torch.equal(p, state["params"]) and float((logpi + ent).item()) == info["elbo"]
    else:
        assert rel_err(p.cpu().numpy(), state["params"].cpu().numpy()) <= 1e-12 and abs(float((logpi + ent).item()) - info["elbo"]) <= 1e-12 * abs(info["elbo"])
    assert replay.counter == rng.counter
    ctx.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    d, n = 6, 4
    rng = np.random.default_rng(5)
    prob, _ = make_problem(rng, "diag", d)
    mf = avi.MiviContext(np.float64, avi.MEANFIELD, d, n, 0, SEED)
    mf.set_problem(prob)
    pm = mf.to_device(np.concatenate([np.zeros(d), np.ones(d)]))
    assert _refused(lambda: mf.sqrt_ngd_steps(pm, 0, 1, 0.1)) == 6
    assert _refused(lambda: mf.sqrt_ngd_update(pm, mf.empty(d), mf.empty(d * d), 0.1)) == 6
    mf.close()
    q, _ = make_family(rng, d, avi.FULLRANK)
    params, _ = avi.destructure(q)
    shard = avi.MiviContext(np.float64, avi.FULLRANK, d, n, 0, SEED, m_offset=n, m_total=2 * n)
    shard.set_problem(prob)
    ps = shard.to_device(params).clone()
    assert _refused(lambda: shard.sqrt_ngd_steps(ps, 0, 1, 0.1)) == 6
    shard.close()
    bij = avi.MiviContext(np.float64, avi.FULLRANK, d, n, 0, SEED)
    bij.set_problem(avi.TransformedProblem(avi.FunnelConstrainedProblem(d, 1.5, order=2), avi.StackedBijector([(0, 1, "exp"), (1, d, "identity")])))
    pb = bij.to_device(params).clone()
    assert _refused(lambda: bij.sqrt_ngd_steps(pb, 0, 2, 0.1, second_order=True)) == 6
    assert np.array_equal(pb.cpu().numpy(), params)                      # refused before anything ran
    elbo = bij.sqrt_ngd_steps(pb, 0, 2, 1e-3)                             # the first-order branch works under the bijector
    bij.synchronize()
    assert bool(torch.isfinite(elbo).all())
    bij.close()


@pytest.mark.parametrize("d", [5, 70])
def test_nonpositive_scale_is_a_status(d):
    """stepsize 1 on N(5, 0.3^2 I) from q0 = N(0, I): C'_ii = 1 - (1 / 0.09 - 1) / 2 < 0 -- reported, nothing faults."""
    prob = avi.DiagNormalProblem(np.full(d, 5.0), np.full(d, 0.3), order=2)
    q0 = avi.FullRankGaussian(np.zeros(d), np.eye(d))
    params, _ = avi.destructure(q0)
    ctx = avi.MiviContext(np.float64, avi.FULLRANK, d, 10, 0, SEED)
    ctx.set_problem(prob)
    p = ctx.to_device(params).clone()
    ctx.sqrt_ngd_steps(p, 0, 1, 1.0, second_order=True)
    assert _refused(ctx.synchronize) == 3
    ctx.synchronize()                                                     # the flag is cleared by the read
    assert _refused(lambda: ctx.sqrt_ngd_update_host(params, np.zeros(d), -np.eye(d) / 0.09, 1.0)) == 3
    ctx.close()
    with pytest.raises(MiviError) as e:
        avi.optimize(avi.PhiloxRNG(SEED), avi.KLMinSqrtNaturalGradDescent(stepsize=1.0, n_samples=10), 3, prob, q0)
    assert e.value.status == 3
