"""FisherMinBatchMatch on the device (src/algorithms/fisherminbatchmatch.jl): the objective, state and update kernels of csrc/kernels_bam.hip
against the numpy restatement tests/bam_ref.py, mivi_bam_steps against the single calls, trajectories against the restatement driven by the
device's own draws, the algorithm's surface (mirroring test/algorithms/fisherminbatchmatch.jl), the refusals and the failure path.

Sizes: d in {3, 10, 44, 45, 64, 65, 130} (one to three 64-row panels, sizes that are no multiple of the tile) and B in {2, 5, 32,
BAM_MAX_SAMPLES}: B < d, B = d and B > d (a singular K whose clamped eigenvalues contribute nothing), odd B (a padded Jacobi problem).

Criteria.  The device builds the rank-B form; the reference of every update check is the LITERAL expression (scipy's sqrtm), which is not
code under test.  f64 at lambda in {0.25, 4}: relative l2 1e-12 on m', 1e-11 on C' and Sigma' (TOL64).  f32: both numbers of
tests/solve_ref.block_ratios(got, yard, ref64, d) at most F32_FACTOR = 8, yard the literal expression in float32, ref64 the same in float64,
both on the f32-stored inputs; values relative 1e-5.  At iteration 1 (lambda = d B) the subtraction Sigma + Zt Zt' - Y Y' cancels about
log10(lambda) digits and K squares the conditioning, in either form: the tolerance of a fixture is ten times the distance between the two
CPU forms on it (the factor for another summation order), floored at TOL64.  Trajectories: the same rule on the two forms' trajectories.

Subsampling with batch size 1 (the reference asks 1/2 of the initial distance): the float64 restatement (tests/bam_ref.py, neither form
is code under test) ends between 0.10 and 0.11 of it whatever the seed, at n_samples 10 and 32 -- the algorithm's own fixed point under
that subsampling, not a rounding matter; tests/test_bam_ref_host.py pins the range.  The device's run is held to the restatement driven
by the same batches and draws, and to 0.12.  Without subsampling the project's bound 0.1 holds.

Measured on the MI355X (relative l2 unless said otherwise):
    moments, every target and size       f64 1.0e-15 (elbo, dense 10 x 5), f32 2.0e-7 (elbo, dense 3 x 64); u bitwise
    estimate_fisher, n = 2 / 7 / 16389   f64 9.5e-16, f32 1.1e-7; at the target f64 6.8e-31 (bound 8.7e-28), f32 9.2e-14 (bound 2.2e-10)
    update, lambda 0.25 and 4, f64       m' 1.9e-13, C' 8.1e-13, Sigma' 1.0e-12 (all at d = 130, B = 2, lambda = 4), entropy 3.3e-15
    update, lambda 0.25 and 4, f32       yardstick ratios 0.69 (whole), 0.73 (worst 64-row block)
    update at iteration 1, f64           within ten times the CPU forms' distance everywhere; the largest distances, at d = 130, B = 64
                                         (lambda = 8320): m' 1.5e-8, C' 2.3e-7, Sigma' 3.1e-7 (tolerances 1.6e-7, 2.3e-6, 3.1e-6); the
                                         least margin at d = B = 64 (lambda = 4096): m' 1.4e-9 of 1.4e-9, C' 7.1e-10 of 1.3e-9, Sigma'
                                         1.8e-9 of 2.3e-9 -- the two CPU forms happen to agree to 1.4e-10 there, ten times closer than
                                         at the neighbouring sizes
    10-step f64 trajectories             d = 5, B = 32: 1.2e-14 (elbo 4.1e-12); d = 20, B = 8: 1.1e-11 (tolerance 2.1e-10)
    moments behind the second-generation sampling kernels (f32, d = 64 / 128, n = 128 / 256): 2.0e-7; estimate_fisher there 1.5e-7
    convergence, T = 1000                f64 2.5e-32, f32 1.0e-17 of the initial distance; subsampling, batch size 1: 0.1059, the
                                         restatement on the same batches and draws 0.1059 (m 1.2e-15, C 0 from it)"""
import functools

import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import subsampling as SUB
from tests import bam_ref as R
from tests import natgrad_ref as NR
from tests.helpers import SEED, OraclePlugin, make_family, make_problem, rel_err
from tests.measure_space_cases import DTYPES, TOL64, VALUE_RTOL
from tests.measure_space_cases import dense_ctx as _dense_ctx, flat as _flat, logreg as _logreg, reference_model as _reference_model
from tests.measure_space_cases import hold, refused as _refused

pytestmark = pytest.mark.gpu
_hold = functools.partial(hold, "bam")

BMAX = avi.BAM_MAX_SAMPLES
DS = (3, 10, 44, 45, 64, 65, 130)
BS = (2, 5, 32, BMAX)
SHAPES = pytest.mark.parametrize("d,B", [(d, B) for d in DS for B in BS])


def _mat(v, d):
    return np.asarray(v).reshape(d, -1, order="F")


def _f64(x):
    return np.asarray(x, dtype=np.float64)


# ---- the objective -----------------------------------------------------------------------------------------------------------------------------
def _target(kind, d, dtype):
    rng = np.random.default_rng(300 + d)
    if kind == "callback":
        _, tgt = make_problem(rng, "dense", d, dtype)
        return OraclePlugin(tgt), tgt
    return make_problem(rng, {"logreg": "logreg0"}.get(kind, kind), d, dtype)


def _check_moments(d, B, kind, dtype, lds_route=False):
    prob, tgt = _target(kind, d, dtype)
    q, _ = make_family(np.random.default_rng(310 + d), d, avi.FULLRANK, dtype)
    params, _ = avi.destructure(q)
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, B, 0, SEED)
    ctx.set_problem(prob)
    assert (ctx.fullrank_route(B)[0] != 0) == lds_route                      # which sampling kernels the objective's first stage runs
    p = ctx.to_device(params).clone()
    z, eps = ctx.sample(p, 7)
    z, eps = _f64(z.cpu().numpy()), eps.cpu().numpy().copy()
    u, G, f, lp, elbo = ctx.bam_moments(p, 7, B)
    ctx.synchronize()
    assert np.array_equal(p.cpu().numpy(), params)
    u, G = _mat(u.cpu().numpy(), d), _mat(G.cpu().numpy(), d)
    assert u.dtype == dtype and np.array_equal(u, eps)                       # bitwise the eps of mivi_sample
    C = np.tril(_f64(_mat(params[d:], d)))
    G_ref = np.stack([tgt.logdensity_and_gradient(z[:, b])[1] for b in range(B)], axis=1)
    lp_ref = float(np.mean([tgt.logdensity_and_gradient(z[:, b])[0] for b in range(B)]))
    f_ref, elbo_ref = R.fisher(C, _f64(u), G_ref), lp_ref + R.entropy(C)
    tol = TOL64[1] if dtype == np.float64 else VALUE_RTOL
    errs = (rel_err(_f64(G), G_ref), abs(float(f.item()) - f_ref) / max(abs(f_ref), 1.0), abs(float(lp.item()) - lp_ref) / max(abs(lp_ref), 1.0),
            abs(float(elbo.item()) - elbo_ref) / max(abs(elbo_ref), 1.0))
    print(f"[bam moments] {kind} {d} {B} {np.dtype(dtype).name}: G {errs[0]:.1e} fisher {errs[1]:.1e} logpi {errs[2]:.1e} elbo {errs[3]:.1e}")
    assert max(errs) <= tol
    uh, Gh, fh, lh, eh = ctx.bam_moments_host(params, 7, B)                  # the _host form equals the device form
    assert np.array_equal(uh, u) and np.array_equal(Gh, G) and (fh, lh, eh) == (f.item(), lp.item(), elbo.item())
    ctx.close()


@DTYPES
@pytest.mark.parametrize("kind", ["diag", "dense", "logreg", "callback"])
@SHAPES
def test_moments(d, B, kind, dtype):
    _check_moments(d, B, kind, dtype)


@pytest.mark.parametrize("kind", ["diag", "dense"])
@pytest.mark.parametrize("d,B", [(64, 128), (128, 256)])
def test_moments_behind_the_second_generation_sampling_kernels(d, B, kind):
    """An f32 context with d a multiple of 64, a multiple of 128 samples and a built-in Gaussian target samples through the LDS-resident
    product kernels (run_estimate_lds); the objective reads the draws and gradients they leave.  (The objective has no rank bound.)"""
    _check_moments(d, B, kind, np.float32, lds_route=True)


@DTYPES
@pytest.mark.parametrize("n", [2, 7, 16389])
def test_estimate_fisher(n, dtype):
    """Any n_samples (16389 crosses the 16384-column chunk boundary) against the oracle's target at the device's own draws; at the exact
    posterior of the dense Gaussian u + C' G = u - L' P L u vanishes: what is left is rounding, entrywise at most d kappa(L) eps |u|."""
    _check_fisher(10, n, dtype)


def test_estimate_fisher_behind_the_second_generation_sampling_kernels():
    _check_fisher(64, 128, np.float32, lds_route=True)


def _check_fisher(d, n, dtype, lds_route=False):
    prob, tgt = make_problem(np.random.default_rng(41), "dense", d, dtype)
    q, _ = make_family(np.random.default_rng(42), d, avi.FULLRANK, dtype)
    params, _ = avi.destructure(q)
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, n, 0, SEED)
    ctx.set_problem(prob)
    assert (ctx.fullrank_route(min(n, 16384))[0] != 0) == lds_route
    z, eps = ctx.sample(params, 3)
    z, eps = _f64(z.cpu().numpy()), _f64(eps.cpu().numpy())
    got = float(ctx.estimate_fisher(params, 3, n).item())
    ctx.synchronize()
    ref = R.fisher(np.tril(_f64(_mat(params[d:], d))), eps, -tgt.prec @ (z - tgt.mean[:, None]))
    print(f"[bam fisher] n {n} {np.dtype(dtype).name}: {abs(got - ref) / ref:.1e}")
    assert abs(got - ref) <= (TOL64[1] if dtype == np.float64 else VALUE_RTOL) * ref
    assert ctx.estimate_fisher_host(params, 3, n) == dtype(got)
    exact, _ = avi.destructure(avi.FullRankGaussian(prob.mean, prob.L))
    at_target = float(ctx.estimate_fisher(exact, 3, n).item())
    ctx.synchronize()
    bound = d * (d * np.linalg.cond(tgt.L) * np.finfo(dtype).eps) ** 2 * float(np.mean(np.sum(eps ** 2, axis=0)))
    print(f"[bam fisher] n {n} {np.dtype(dtype).name} at the target: {at_target:.1e} (bound {bound:.1e})")
    assert 0.0 <= at_target <= bound
    ctx.close()


# ---- init and update -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(dtype, d, B):
    """(params, Sigma0 flat from mivi_bam_init, u, G) in dtype: a random iterate, draws and RANDOM gradients."""
    m, C, u, G = R.random_case(d, B, 1000 * d + B, dtype)
    params, _ = avi.destructure(avi.FullRankGaussian(m.astype(dtype), C.astype(dtype)))
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, B, 0, SEED)
    ctx.set_problem(avi.DiagNormalProblem(np.zeros(d, dtype), np.ones(d, dtype)))   # (the entries refuse a context without a target)
    pd = ctx.to_device(params).clone()
    st0 = ctx.bam_init(pd).cpu().numpy().copy()
    ctx.synchronize()
    assert np.array_equal(pd.cpu().numpy(), params)                          # init only reads the parameters
    ctx.close()
    return params, st0, u.astype(dtype), G.astype(dtype)


@DTYPES
@pytest.mark.parametrize("d", DS)
def test_init_is_the_covariance(d, dtype):
    params, st0, _, _ = _case(dtype, d, 2)
    C = np.tril(_mat(params[d:], d))
    S = _mat(st0, d)
    assert S.dtype == dtype and np.array_equal(S, S.T)
    if dtype == np.float64:
        assert rel_err(S, C @ C.T) <= TOL64[1]
    else:
        _hold("init Sigma", d, S, C @ C.T, _f64(C) @ _f64(C).T)


def _device_update(dtype, d, B, lam):
    """(params', Sigma', entropy) of mivi_bam_update; u and G come back bit-identical and the _host form equals the device form."""
    params, st0, u, G = _case(dtype, d, B)
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, B, 0, SEED)
    ctx.set_problem(avi.DiagNormalProblem(np.zeros(d, dtype), np.ones(d, dtype)))
    pd, sd, ud, Gd = ctx.to_device(params).clone(), ctx.to_device(st0).clone(), ctx.to_device(_flat(u)), ctx.to_device(_flat(G))
    ent = ctx.bam_update(pd, sd, ud, Gd, B, lam)
    ctx.synchronize()
    assert np.array_equal(ud.cpu().numpy(), _flat(u)) and np.array_equal(Gd.cpu().numpy(), _flat(G))
    ph, sh, eh = ctx.bam_update_host(params, st0, u, G, lam)
    got, st, ent = pd.cpu().numpy(), sd.cpu().numpy(), ent.cpu().numpy()[0]
    ctx.close()
    assert got.dtype == dtype and st.dtype == dtype
    assert np.array_equal(got, ph) and np.array_equal(st, sh) and ent == eh
    C, S = _mat(got[d:], d), _mat(st, d)
    assert np.all(np.triu(C, 1) == 0.0) and np.all(np.diag(C) > 0.0)         # exact zeros above the diagonal
    assert np.array_equal(S, S.T)                                            # bitwise-mirrored triangles
    return got[:d], C, S, ent


def _reference(dtype, d, B, lam, yard=False):
    params, st0, u, G = _case(dtype, d, B)
    m, C, S0 = _f64(params[:d]), np.tril(_f64(_mat(params[d:], d))), _f64(_mat(st0, d))
    z = C @ _f64(u) + m[:, None]
    if yard:
        return R.update_literal(m, S0, z, _f64(G), lam, np.float32)
    return R.update_literal(m, S0, z, _f64(G), lam), R.discrepancy(m, S0, z, _f64(G), lam)


@DTYPES
@pytest.mark.parametrize("lam", [0.25, 4.0])
@SHAPES
def test_update_matches_the_literal_expression(d, B, lam, dtype):
    m, C, S, ent = _device_update(dtype, d, B, lam)
    (m_ref, C_ref, S_ref), _ = _reference(dtype, d, B, lam)
    ent_ref = R.entropy(C_ref)
    if dtype == np.float64:
        errs = (rel_err(m, m_ref), rel_err(C, C_ref), rel_err(S, S_ref), abs(ent - ent_ref) / max(abs(ent_ref), 1.0))
        print(f"[bam f64] {d} {B} lambda {lam}: m {errs[0]:.1e} C {errs[1]:.1e} Sigma {errs[2]:.1e} entropy {errs[3]:.1e}")
        assert errs[0] <= TOL64[0] and max(errs[1:]) <= TOL64[1]
    else:
        m_y, C_y, S_y = _reference(dtype, d, B, lam, yard=True)
        _hold(f"lambda {lam} B {B} m", d, m, m_y, m_ref)
        _hold(f"lambda {lam} B {B} C", d, C, C_y, C_ref)
        _hold(f"lambda {lam} B {B} Sigma", d, S, S_y, S_ref)
        assert abs(float(ent) - ent_ref) <= VALUE_RTOL * max(abs(ent_ref), 1.0)


@SHAPES
def test_update_at_iteration_one(d, B):
    """lambda = d B: the tolerance is ten times the two CPU forms' distance on this fixture, floored at TOL64."""
    lam = float(d * B)
    m, C, S, _ = _device_update(np.float64, d, B, lam)
    (m_ref, C_ref, S_ref), disc = _reference(np.float64, d, B, lam)
    errs = (rel_err(m, m_ref), rel_err(C, C_ref), rel_err(S, S_ref))
    tols = tuple(max(10.0 * x, t) for x, t in zip(disc, (TOL64[0], TOL64[1], TOL64[1])))
    print(f"[bam iteration 1] {d} {B}: m {errs[0]:.1e} ({tols[0]:.1e}) C {errs[1]:.1e} ({tols[1]:.1e}) Sigma {errs[2]:.1e} ({tols[2]:.1e})")
    assert all(e <= t for e, t in zip(errs, tols))


# ---- steps --------------------------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("d,n", [(5, 32), (70, BMAX), (64, BMAX), (130, 5)])
def test_steps_are_the_single_calls_bitwise(d, n, dtype):
    ctx, params, _, _ = _dense_ctx(d, n, dtype, False)
    idx, it0 = 11, 4
    p1 = ctx.to_device(params).clone()
    s1 = ctx.bam_init(p1)
    s0 = s1.clone()
    f1, e1 = [], []
    for t in range(3):
        u, G, f, _, e = ctx.bam_moments(p1, idx + t, n)
        f1.append(f.clone())
        e1.append(e.clone())
        ctx.bam_update(p1, s1, u, G, n, float(dtype(d * n / (it0 + t))))
    p3, s3 = ctx.to_device(params).clone(), s0.clone()
    f3, e3 = ctx.bam_steps(p3, s3, idx, it0, 3, n)
    again, s_again = ctx.to_device(params).clone(), s0.clone()
    f_again, e_again = ctx.bam_steps(again, s_again, idx, it0, 3, n)
    ctx.synchronize()
    assert torch.equal(p1, p3) and torch.equal(s1, s3) and torch.equal(torch.cat(f1), f3) and torch.equal(torch.cat(e1), e3)
    assert torch.equal(p3, again) and torch.equal(s3, s_again) and torch.equal(f3, f_again) and torch.equal(e3, e_again)
    assert not torch.equal(p3, ctx.to_device(params)) and bool(torch.isfinite(e3).all()) and bool(torch.isfinite(f3).all())
    ctx.close()


@pytest.mark.parametrize("d,n", [(5, 32), (20, 8)])
def test_trajectory_f64(d, n):
    ctx, params, q_o, tgt = _dense_ctx(d, n, np.float64, False)
    T, idx0 = 10, 5
    p = ctx.to_device(params).clone()
    st = ctx.bam_init(p)
    draws = [_f64(ctx.sample(p, idx0 + t)[1].cpu().numpy()) for t in range(T)]   # eps is a function of (seed, index) alone
    fisher, elbo = ctx.bam_steps(p, st, idx0, 1, T, n)
    ctx.synchronize()
    m0, C0 = _f64(params[:d]), np.tril(_f64(_mat(params[d:], d)))
    (m_a, C_a, S_a), info_a = R.steps(m0, C0, draws, tgt, update=R.update_literal)
    (m_b, C_b, S_b), _ = R.steps(m0, C0, draws, tgt, update=R.update_lowrank)
    got, S = p.cpu().numpy(), _mat(st.cpu().numpy(), d)
    disc = max(rel_err(m_b, m_a), rel_err(C_b, C_a), rel_err(S_b, S_a))
    tol = max(10.0 * disc, TOL64[1])
    errs = (rel_err(got[:d], m_a), rel_err(_mat(got[d:], d), C_a), rel_err(S, S_a),
            float(np.max(np.abs(elbo.cpu().numpy() - np.array([i["elbo"] for i in info_a])) / np.abs([i["elbo"] for i in info_a]))),
            rel_err(fisher.cpu().numpy(), np.array([i["covweighted_fisher"] for i in info_a])))
    print(f"[bam trajectory] {d} {n}: m {errs[0]:.1e} C {errs[1]:.1e} Sigma {errs[2]:.1e} elbo {errs[3]:.1e} fisher {errs[4]:.1e} (tolerance {tol:.1e})")
    assert max(errs) <= tol
    ctx.close()


# ---- the algorithm's surface (test/algorithms/fisherminbatchmatch.jl) -----------------------------------------------------------------------------
def _alg(**kw):
    return avi.FisherMinBatchMatch(n_samples=kw.pop("n_samples", 10), **kw)


def test_callback_iterations():
    _, prob, _, q0 = _reference_model(np.float64, 1)
    seen = []

    def callback(rng, iteration, q, state):
        seen.append((iteration, q.location.copy(), state["iteration"]))
        return {"iteration_check": iteration, "elbo": "shadowed"}

    _, info, _ = avi.optimize(_alg(), 10, prob, q0, callback=callback)
    assert [i["iteration_check"] for i in info] == list(range(1, 11)) == [s[0] for s in seen] == [s[2] for s in seen]
    assert np.array_equal(seen[0][1], q0.location) and not np.array_equal(seen[1][1], q0.location)   # q: the iterate the step started from
    assert all(isinstance(i["elbo"], float) and np.isfinite(i["elbo"]) and i["covweighted_fisher"] >= 0.0 for i in info)


def test_estimate_objective_at_the_target():
    d, prob, _, _ = _reference_model(np.float64, 1)
    q_true = avi.FullRankGaussian(np.full(d, 5.0), 0.3 * np.eye(d))
    assert abs(avi.estimate_objective(avi.PhiloxRNG(SEED), _alg(), q_true, prob, n_samples=1000)) <= 1e-24
    q0 = avi.FullRankGaussian(np.zeros(d), np.eye(d))
    assert avi.estimate_objective(_alg(), q0, prob) > 1.0


def test_determinism_and_routes():
    _, prob, _, q0 = _reference_model(np.float64, 1)
    alg = _alg()
    q1, info1, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 20, prob, q0)
    q2, info2, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 20, prob, q0)
    assert np.array_equal(q1.location, q2.location) and np.array_equal(q1.scale, q2.scale)
    q3, info3, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 20, prob, q0, device_loop=False)             # the host-driven `step` loop
    assert np.array_equal(q1.location, q3.location) and np.array_equal(q1.scale, q3.scale)
    for key in ("elbo", "covweighted_fisher", "iteration"):
        assert [i[key] for i in info1] == [i[key] for i in info3] == [i[key] for i in info2]
    assert [i["iteration"] for i in info1] == list(range(1, 21))
    rng = avi.PhiloxRNG(SEED)                                                                            # warm start: 12 + 8 = 20
    _, _, st12 = avi.optimize(rng, alg, 12, prob, q0)
    p12, s12 = st12["params"].clone(), st12["bam"].clone()
    q4, info4, st = avi.optimize(rng, alg, 8, prob, q0, state=st12)
    assert torch.equal(st12["params"], p12) and torch.equal(st12["bam"], s12) and st12["iteration"] == 12   # the caller's state is left as it was
    assert st["iteration"] == 20 and [i["iteration"] for i in info4] == list(range(1, 9))
    assert np.array_equal(q1.location, q4.location) and np.array_equal(q1.scale, q4.scale)
    rng = avi.PhiloxRNG(SEED)                                                                            # ... on either route
    _, _, st12 = avi.optimize(rng, alg, 12, prob, q0, device_loop=False)
    q5, _, _ = avi.optimize(rng, alg, 8, prob, q0, state=st12, device_loop=False)
    assert np.array_equal(q1.location, q5.location) and np.array_equal(q1.scale, q5.scale)


@DTYPES
def test_output_dtype(dtype):
    _, prob, _, q0 = _reference_model(dtype, 1)
    q, info, _ = avi.optimize(_alg(), 10, prob, q0)
    assert q.location.dtype == dtype and q.scale.dtype == dtype and len(info) == 10
    assert np.all(np.triu(q.scale, 1) == 0.0) and np.all(np.diag(q.scale) > 0.0)


@DTYPES
def test_convergence(dtype):
    d, prob, _, q0 = _reference_model(dtype, 1)
    q, info, _ = avi.optimize(avi.PhiloxRNG(SEED), _alg(), 1000, prob, q0)
    mu_true, L_true = np.full(d, 5.0), 0.3 * np.eye(d)
    d0 = np.sum((_f64(q0.location) - mu_true) ** 2) + np.sum((_f64(q0.scale) - L_true) ** 2)
    dl = np.sum((_f64(q.location) - mu_true) ** 2) + np.sum((_f64(q.scale) - L_true) ** 2)
    print(f"[bam convergence] {np.dtype(dtype).name}: ratio {dl / d0:.1e}")
    assert len(info) == 1000 and dl <= 0.1 * d0


def test_subsampling_determinism_and_one_step():
    prob = _logreg(1)
    d = prob.dimension()
    q0 = avi.FullRankGaussian(np.zeros(d), np.eye(d))
    sub = avi.ReshufflingBatchSubsampling(np.arange(8), 3)
    alg = _alg(subsampling=sub)
    q1, info1, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 10, prob, q0)
    q2, info2, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 10, prob, q0)
    assert np.array_equal(q1.location, q2.location) and np.array_equal(q1.scale, q2.scale)
    assert [i["elbo"] for i in info1] == [i["elbo"] for i in info2]
    assert all("epoch" in i and "step" in i for i in info1)
    rng = avi.PhiloxRNG(SEED)                                                # one step = the objective on the selected rows + the update
    state = avi.init(rng, alg, q0, prob)
    state, _, info = avi.step(rng, alg, state, None)
    replay = avi.PhiloxRNG(SEED)
    batch, _, sub_inf = SUB.step_subsampling(replay, sub, SUB.init_subsampling(replay, sub))
    assert info["epoch"] == sub_inf["epoch"] and info["step"] == sub_inf["step"]
    ctx = avi.MiviContext(np.float64, avi.FULLRANK, d, 10, 0, SEED)
    ctx.set_problem(avi.subsample(prob, batch))
    p = ctx.to_device(avi.destructure(q0)[0]).clone()
    st = ctx.bam_init(p)
    u, G, f, _, e = ctx.bam_moments(p, replay.next_index(), 10)
    ctx.bam_update(p, st, u, G, 10, d * 10 / 1)
    ctx.synchronize()
    assert torch.equal(p, state["params"]) and torch.equal(st, state["bam"])
    assert float(e.item()) == info["elbo"] and float(f.item()) == info["covweighted_fisher"]
    assert replay.counter == rng.counter
    ctx.close()


def test_subsampling_convergence():
    """test/algorithms/fisherminbatchmatch.jl "subsampling / convergence" on test/models/subsamplednormals.jl (restated in
    tests/natgrad_ref.py): the default algorithm, batch size 1, T = 1000; the posterior is N(mean(mus), 1 / n_data).  The device's run is
    held to the float64 restatement driven by the SAME batches and draws (the trajectories' rule: ten times the two CPU forms' distance,
    floored at TOL64), and to 0.12 of the initial distance: the restatement's own end, 0.10 to 0.11 whatever the seed
    (tests/test_bam_ref_host.py pins that range), plus a tenth."""
    n_data, T = 8, 1000
    model = NR.SubsampledNormals(np.random.default_rng(3).normal(size=n_data))
    mu_true, L_true = np.array([model.mus.mean()]), np.array([[np.sqrt(1.0 / n_data)]])
    q0 = avi.FullRankGaussian(np.zeros(1), np.eye(1))
    sub = avi.ReshufflingBatchSubsampling(np.arange(n_data), 1)
    alg = avi.FisherMinBatchMatch(subsampling=sub)
    draws = []

    def callback(rng, iteration, q, state):
        draws.append(_f64(state["u_buf"].cpu().numpy()).reshape(1, alg.n_samples, order="F"))

    q, info, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, T, model, q0, callback=callback)
    d0 = np.sum((q0.location - mu_true) ** 2) + np.sum((q0.scale - L_true) ** 2)
    dl = np.sum((q.location - mu_true) ** 2) + np.sum((q.scale - L_true) ** 2)
    ends = []
    for update in (R.update_literal, R.update_lowrank):
        rp = avi.PhiloxRNG(SEED)                                             # replays the batches the run saw
        st = SUB.init_subsampling(rp, sub)
        m, C, S = np.zeros(1), np.eye(1), np.eye(1)
        for t in range(T):
            batch, st, _ = SUB.step_subsampling(rp, sub, st)
            rp.next_index()
            (m, C, S), _ = R.step(m, C, S, draws[t], model.subsample(batch), t + 1, update)
        ends.append((m, C))
    (m_a, C_a), (m_b, C_b) = ends
    tol = max(10.0 * max(rel_err(m_b, m_a), rel_err(C_b, C_a)), TOL64[1])
    errs = (rel_err(q.location, m_a), rel_err(q.scale, C_a))
    ref_ratio = (np.sum((m_a - mu_true) ** 2) + np.sum((C_a - L_true) ** 2)) / d0
    print(f"[bam subsampling convergence] ratio {dl / d0:.4f} (restatement {ref_ratio:.4f}); m {errs[0]:.1e} C {errs[1]:.1e} (tolerance {tol:.1e})")
    assert len(info) == T == len(draws) and max(errs) <= tol
    assert dl <= 0.12 * d0


# ---- refusals and the failure path -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    d, n = 6, 4
    rng = np.random.default_rng(5)
    prob, _ = make_problem(rng, "diag", d)
    mf = avi.MiviContext(np.float64, avi.MEANFIELD, d, n, 0, SEED)
    mf.set_problem(prob)
    pm = mf.to_device(np.concatenate([np.zeros(d), np.ones(d)])).clone()
    sm = mf.to_device(np.arange(1.0 * d * d)).clone()
    un, Gn = mf.empty(d * n), mf.empty(d * n)
    for call in (lambda: mf.bam_init(pm, sm), lambda: mf.bam_moments(pm, 0, n), lambda: mf.estimate_fisher(pm, 0, n),
                 lambda: mf.bam_update(pm, sm, un, Gn, n, 1.0), lambda: mf.bam_steps(pm, sm, 0, 1, 1, n)):
        assert _refused(call) == 6
    assert np.array_equal(sm.cpu().numpy(), np.arange(1.0 * d * d)) and np.array_equal(pm.cpu().numpy()[d:], np.ones(d))
    mf.close()
    q, _ = make_family(rng, d, avi.FULLRANK)
    params, _ = avi.destructure(q)
    good = avi.MiviContext(np.float64, avi.FULLRANK, d, n, 0, SEED)
    good.set_problem(prob)
    st_good = good.bam_init(good.to_device(params)).cpu().numpy().copy()
    good.synchronize()

    def every_entry(ctx, status, n=n):
        p, st = ctx.to_device(params).clone(), ctx.to_device(st_good).clone()
        u, G = ctx.empty(d * max(n, 1)), ctx.empty(d * max(n, 1))
        for call in (lambda: ctx.bam_init(p, st), lambda: ctx.bam_moments(p, 0, n), lambda: ctx.estimate_fisher(p, 0, n),
                     lambda: ctx.bam_update(p, st, u, G, n, 1.0), lambda: ctx.bam_steps(p, st, 0, 1, 1, n)):
            assert _refused(call) == status
        ctx.synchronize()
        assert np.array_equal(p.cpu().numpy(), params) and np.array_equal(st.cpu().numpy(), st_good)   # refused before anything ran

    shard = avi.MiviContext(np.float64, avi.FULLRANK, d, n, 0, SEED, m_offset=n, m_total=2 * n)
    shard.set_problem(prob)
    every_entry(shard, 6)
    shard.close()
    bare = avi.MiviContext(np.float64, avi.FULLRANK, d, n, 0, SEED)
    every_entry(bare, 5)                                                     # no target
    bare.close()
    bij = avi.MiviContext(np.float64, avi.FULLRANK, d, n, 0, SEED)
    bij.set_problem(avi.TransformedProblem(avi.FunnelConstrainedProblem(d, 1.5), avi.StackedBijector([(0, 1, "exp"), (1, d, "identity")])))
    every_entry(bij, 6)                                                      # the algorithm requires unconstrained support
    bij.close()
    p, st = good.to_device(params).clone(), good.to_device(st_good).clone()
    for bad_n, status in ((1, 1), (0, 1), (BMAX + 1, 6)):                    # the corrected covariance needs two samples; the rank bound
        u, G = good.empty(d * (bad_n + 1)), good.empty(d * (bad_n + 1))
        assert _refused(lambda: good.bam_update(p, st, u, G, bad_n, 1.0)) == status
        assert _refused(lambda: good.bam_steps(p, st, 0, 1, 1, bad_n)) == status
        if bad_n < 2:
            assert _refused(lambda: good.bam_moments(p, 0, bad_n)) == status
            assert _refused(lambda: good.estimate_fisher(p, 0, bad_n)) == status
    good.synchronize()
    assert np.array_equal(p.cpu().numpy(), params) and np.array_equal(st.cpu().numpy(), st_good)
    assert float(good.estimate_fisher(p, 0, BMAX + 1).item()) > 0.0          # the objective has no rank bound
    good.synchronize()
    good.close()


@pytest.mark.parametrize("d", [5, 70])
def test_a_nan_gradient_is_a_status(d):
    """A NaN in G: the eigenproblem cannot converge and no pivot is a number -- the sticky flag, the call returns, nothing loops; a following
    valid update on fresh buffers is correct."""
    B = 8
    params, st0, u, G = _case(np.float64, d, B)
    bad = G.copy()
    bad[d // 2, 3] = np.nan
    ctx = avi.MiviContext(np.float64, avi.FULLRANK, d, B, 0, SEED)
    ctx.set_problem(avi.DiagNormalProblem(np.zeros(d), np.ones(d)))
    p, st = ctx.to_device(params).clone(), ctx.to_device(st0).clone()
    ctx.bam_update(p, st, ctx.to_device(_flat(u)), ctx.to_device(_flat(bad)), B, 4.0)
    assert _refused(ctx.synchronize) in (2, 3)
    ctx.synchronize()                                                        # the flag is cleared by the read
    assert _refused(lambda: ctx.bam_update_host(params, st0, u, bad, 4.0)) in (2, 3)
    p2, st2 = ctx.to_device(params).clone(), ctx.to_device(st0).clone()
    ctx.bam_update(p2, st2, ctx.to_device(_flat(u)), ctx.to_device(_flat(G)), B, 4.0)
    ctx.synchronize()
    (m_ref, C_ref, S_ref), _ = _reference(np.float64, d, B, 4.0)
    got = p2.cpu().numpy()
    assert rel_err(got[:d], m_ref) <= TOL64[0] and rel_err(_mat(got[d:], d), C_ref) <= TOL64[1] and rel_err(_mat(st2.cpu().numpy(), d), S_ref) <= TOL64[1]
    ctx.close()
