"""GPU tests of the RealNVP normalizing-flow family (MIVI_REALNVP; docs/src/tutorials/flows.md, defined in include/mivi.h): libmivi
through the C ABI against tests/flow_ref.py on the same Philox stream.

The rule is that of tests/test_gpu_lowrank.py: the error against the reference (the numpy evaluation in float64 for float32 contexts, in
long double for float64 contexts; tests/test_flow_ref_host.py pins it to torch autograd) is at most 8 x the error of the same evaluation
in the context's dtype, floored at that file's tolerances -- 1e-6 / 1e-14 relative l2 for samples, value relative and gradient relative l2
1e-5 / 2e-5 (f32), 1e-12 / 1e-11 (f64).  The gradient is held to it as a whole AND per parameter block (each W_j and b_j of each net),
the block's floor being its share of the whole-gradient allowance (flow_ref.block_report)."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import _lib
from oracle import oracle as O
from tests import flow_ref as R
from tests.helpers import SEED, OraclePlugin, make_family, make_problem, rel_err

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
KINDS = [avi.MonteCarloEntropy(), avi.StickingTheLandingEntropy()]
IDX = R.CASE_IDX
MID = (5, (16, 7), 2, 33)


def _id(case):
    return f"{case[0]}-{'x'.join(map(str, case[1]))}-{case[2]}-{case[3]}"


def make_ctx(case, ent, dtype, prob=None, n_mc=None):
    d, hidden, L, M = case
    ctx = avi.MiviContext(dtype, avi.REALNVP, d, n_mc or M, ent.code, SEED, flow=(hidden, L))
    if prob is not None:
        ctx.set_problem(prob)
    return ctx


def make_target(case, kind, dtype, plugin=False, bijector=False):
    d, _, _, M = case
    rng = np.random.default_rng(4321 + d + 7 * M)
    prob, tgt = make_problem(rng, kind, d, dtype)
    if plugin:
        prob = OraclePlugin(tgt)
    if bijector:   # Stacked([exp on the first three coordinates, identity on the rest]) around the target
        blocks = [(0, 3, "exp"), (3, d, "identity")]
        prob, tgt = avi.TransformedProblem(prob, avi.StackedBijector(blocks)), O.StackedBijectorTarget(tgt, blocks)
    return prob, tgt


_REF = {}


def reference(key, case, params, tgt, eps, kind, dtype):
    """(reference, yardstick) of a case: computed once, shared and never modified."""
    if key not in _REF:
        arch = case[:3]
        ell, G = R.target_columns(tgt, R.estimate_gradient(params, arch, tgt, eps, kind)["Z"])
        _REF[key] = (R.evaluate(params, arch, G, ell, eps, kind, R.ref_dtype(dtype)), R.evaluate(params, arch, G, ell, eps, kind, dtype))
    return _REF[key]


def run_case(case, ent, dtype, kind="diag", plugin=False, bijector=False):
    d, hidden, L, M = case
    arch = case[:3]
    params = R.case_params(case, dtype)
    prob, tgt = make_target(case, kind, dtype, plugin, bijector)
    ctx = make_ctx(case, ent, dtype, prob)
    assert ctx.params_len == params.shape[0] == avi.flow_layout(d, hidden, L)[1] and ctx.partials_len == 0
    Z, eps = ctx.sample(params, IDX)
    assert eps.shape == (d, M)
    mf = avi.MiviContext(dtype, avi.MEANFIELD, d, M, ent.code, SEED)   # the draws ARE the mean-field family's stream: bit for bit
    assert torch.equal(eps, mf.sample(np.concatenate([np.zeros(d, dtype), np.ones(d, dtype)]), IDX)[1])
    mf.close()
    eps, Z = eps.cpu().numpy().astype(np.float64), Z.cpu().numpy().astype(np.float64)
    value, grad = ctx.estimate_gradient(params, IDX)
    ctx.synchronize()
    value, grad = float(value.item()), grad.cpu().numpy().astype(np.float64)
    ctx.close()
    key = (case, kind, ent.code, np.dtype(dtype).name, plugin, bijector)
    ref, yard = reference(key, case, params, tgt, eps, ent.code, dtype)
    stol = R.STOL[np.dtype(dtype)]
    assert rel_err(eps, O.philox_normal(SEED, IDX, d, 0, M, f64=dtype == np.float64)) < stol   # ... and the oracle's restatement of it
    refZ, refv, refg = (np.asarray(ref[k], dtype=np.float64) for k in ("Z", "value", "grad"))
    z_err, z_bound = rel_err(Z, refZ), max(stol, 8 * rel_err(yard["Z"], refZ))
    vt, _ = R.TOL[np.dtype(dtype)]
    v_err, v_bound = abs(value - float(refv)), max(vt * abs(float(refv)), 8 * abs(float(yard["value"]) - float(refv)))
    print(f"[flow] {key}: Z err {z_err:.3e} (bound {z_bound:.3e}), value err {v_err:.3e} (bound {v_bound:.3e})")
    rows = R.block_report(grad, ref["grad"], yard["grad"], arch, dtype)
    for name, err, bound in rows:
        print(f"[flow]   grad {name}: err {err:.3e} (bound {bound:.3e})")
    assert z_err <= z_bound
    assert v_err <= v_bound, (value, float(refv))
    assert not R.violations(rows), R.violations(rows)
    return ref, yard


# ---- parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ent", KINDS, ids=lambda e: type(e).__name__)
@pytest.mark.parametrize("case", list(R.CASES), ids=_id)
def test_diag_target_both_estimators_all_shapes(case, ent, dtype):
    run_case(case, ent, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ent", KINDS, ids=lambda e: type(e).__name__)
@pytest.mark.parametrize("kind,plugin,bijector", [("dense", False, False), ("logreg0", False, False), ("funnel", False, False),
                                                  ("diag", True, False), ("dense", False, True)],
                         ids=["dense", "logreg", "funnel", "plugin", "stacked"])
def test_targets_plugin_and_bijector(kind, plugin, bijector, ent, dtype):
    run_case(MID, ent, dtype, kind=kind, plugin=plugin, bijector=bijector)


# ---- known answers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_parameters_on_the_standard_normal_value_and_stl_gradient_vanish(dtype):
    """q = pi: every -ell + log q term is 0, and the sticking-the-landing gradient is 0 (the reference's "STL gradient is 0 at q = pi")."""
    case = (5, (16, 7), 2, 33)
    d = case[0]
    ctx = make_ctx(case, avi.StickingTheLandingEntropy(), dtype, avi.DiagNormalProblem(np.zeros(d, dtype), np.ones(d, dtype)))
    params = np.zeros(ctx.params_len, dtype=dtype)
    Z, eps = ctx.sample(params, IDX)
    assert torch.equal(Z, eps)
    value, grad = ctx.estimate_gradient(params, IDX)
    ctx.synchronize()
    vt, gt = R.TOL[np.dtype(dtype)]
    scale = 0.5 * d * (1.0 + math.log(2.0 * math.pi))   # the size of the two terms that cancel
    print(f"[flow] q = pi: value {float(value.item()):.3e}, |grad| {float(grad.norm().item()):.3e}")
    assert abs(float(value.item())) <= vt * scale
    assert float(grad.norm().item()) <= gt
    ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_logpdf_of_own_samples_and_constrained_logpdf(dtype):
    case = MID
    d = case[0]
    params = R.case_params(case, dtype)
    ctx = make_ctx(case, avi.MonteCarloEntropy(), dtype)
    Z, eps = ctx.sample(params, IDX)
    arch, e64 = case[:3], eps.cpu().numpy().astype(np.float64)
    zeros = np.zeros_like(e64)
    ref = R.evaluate(params, arch, zeros, zeros[0], e64, 2, R.ref_dtype(dtype))
    yard = R.evaluate(params, arch, zeros, zeros[0], e64, 2, dtype)
    want = np.asarray(ref["logq"], dtype=np.float64)
    vt = R.TOL[np.dtype(dtype)][0]
    bound = max(vt * np.abs(want).max(), 8 * np.abs(np.asarray(yard["logq"], dtype=np.float64) - want).max())
    got = ctx.logpdf(params, Z).cpu().numpy().astype(np.float64)
    got_h = ctx.logpdf_host(params, Z.cpu().numpy())
    print(f"[flow] logpdf of own samples: err {np.abs(got - want).max():.3e} (bound {bound:.3e})")
    assert np.abs(got - want).max() <= bound and np.array_equal(got_h.astype(np.float64), got)
    # through Stacked([exp on three coordinates, identity]): log q(b(x)) - logabsdetjac(binv, b(x)), b(x) = z
    ctx.set_bijector(avi.StackedBijector([(0, 3, "exp"), (3, d, "identity")]))
    X, eta = ctx.sample_constrained(params, IDX, want_eta=True)
    assert torch.equal(eta, Z) and torch.equal(X[3:], Z[3:]) and bool((X[:3] > 0).all())
    got_c = ctx.logpdf_constrained(params, X).cpu().numpy().astype(np.float64)
    z64 = np.asarray(ref["Z"], dtype=np.float64)
    want_c = want - z64[:3].sum(axis=0)
    bound_c = bound + 16 * np.finfo(dtype).eps * np.abs(z64[:3]).sum(axis=0).max()   # log(exp(z)) and the sum of three, in dtype
    print(f"[flow] constrained logpdf: err {np.abs(got_c - want_c).max():.3e} (bound {bound_c:.3e})")
    assert np.abs(got_c - want_c).max() <= bound_c
    ctx.close()


# ---- contracts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [MID, (5, (8,), 2, 600)], ids=_id)
def test_batched_entries_and_repeated_calls_are_bitwise(case, dtype):
    params = R.case_params(case, dtype)
    prob, _ = make_target(case, "dense", dtype)
    ctx = make_ctx(case, avi.StickingTheLandingEntropy(), dtype, prob)
    p, n = ctx.to_device(params), 3
    singles = [tuple(t.clone() for t in ctx.estimate_gradient(p, 7 + i)) for i in range(n)]
    again = [tuple(t.clone() for t in ctx.estimate_gradient(p, 7 + i)) for i in range(n)]
    values, grads = ctx.estimate_gradient_each(p, 7, n)
    v_last, g_last = ctx.empty(1), ctx.empty(ctx.params_len)
    ctx.estimate_gradient_n(p, 7, n, v_last, g_last)
    ctx.synchronize()
    for i, (v, g) in enumerate(singles):
        assert torch.equal(again[i][0], v) and torch.equal(again[i][1], g)
        assert torch.equal(values[i:i + 1], v) and torch.equal(grads[i], g)
    assert torch.equal(v_last, singles[-1][0]) and torch.equal(g_last, singles[-1][1])
    vh, gh = ctx.estimate_gradient_host(params, 7)
    assert vh == singles[0][0].item() and np.array_equal(gh, singles[0][1].cpu().numpy())
    ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_estimate_objective_any_n_samples(dtype):
    case = MID
    d, arch = case[0], case[:3]
    params = R.case_params(case, dtype)
    prob, tgt = make_target(case, "diag", dtype)
    ctx = make_ctx(case, avi.MonteCarloEntropy(), dtype, prob, n_mc=16)
    vt = 1e-5 if dtype == np.float32 else 1e-11   # (tests/test_gpu_lowrank.py::test_estimate_objective_any_n_samples_every_entropy)
    for n in (1, 33, 40000):
        eps = O.philox_normal(SEED, 2, d, 0, n, f64=dtype == np.float64).astype(np.float64)
        with torch.no_grad():
            Z, lq = R.forward(torch.tensor(params.astype(np.float64)), arch, torch.tensor(eps))
        ell = np.array([tgt.logdensity(Z[:, k].numpy().copy()) for k in range(n)])
        want = float(np.mean(-ell + lq.numpy()))
        for ent in KINDS:
            got = float(ctx.estimate_objective(params, 2, n_samples=n, entropy=ent.code).item())
            print(f"[flow] estimate_objective n = {n}, kind {ent.code}: {got} against {want}")
            assert abs(got - want) <= vt * abs(want), (n, got, want)
        if n == 33:
            assert abs(float(ctx.estimate_objective_host(params, 2, n_samples=n)) - want) <= vt * abs(want)
    with pytest.raises(avi.MiviError) as e:   # a closed-form kind needs entropy(q)
        ctx.estimate_objective(params, 2, n_samples=8, entropy=avi.ClosedFormEntropy.code)
    assert e.value.status == _lib.ERR_UNSUPPORTED and "MonteCarloEntropy" in str(e.value)
    ctx.close()


def test_rand_logpdf_and_transformed_distribution_take_the_flow():
    q = avi.RealNVP(5, [16, 7], 2, rng=4)
    assert len(q) == 5 and q.hidden_dims == (16, 7) and q.n_layers == 2 and q.eltype == np.float64 and q.family == avi.REALNVP
    flat, re_ = avi.destructure(q)
    assert np.array_equal(re_(flat).params, q.params) and re_(flat).hidden_dims == q.hidden_dims
    rng = avi.PhiloxRNG(SEED)
    idx = rng.counter
    Z = avi.rand(rng, q, 7)
    assert tuple(Z.shape) == (5, 7) and rng.counter == idx + 1
    ctx = make_ctx((5, (16, 7), 2, 7), avi.MonteCarloEntropy(), np.float64)
    assert torch.equal(Z, ctx.sample(flat, idx, want_eps=False))
    lq = avi.logpdf(q, Z)
    assert torch.equal(lq, ctx.logpdf(flat, Z))
    assert avi.logpdf(q, Z[:, 0].cpu().numpy()) == float(lq[0].item())
    qt = avi.TransformedDistribution(q, avi.StackedBijector([(0, 1, "exp"), (1, 5, "identity")]))
    X = avi.rand(avi.PhiloxRNG(SEED), qt, 7)
    assert bool((X[0] > 0).all()) and torch.equal(X[1:], Z[1:])
    want = lq - Z[0]
    assert torch.allclose(avi.logpdf(qt, X), want, rtol=0, atol=1e-12 * float(want.abs().max()))
    ctx.close()


def test_gaussian_contexts_are_unchanged_by_a_flow_context():
    d, M = 64, 32
    rng = np.random.default_rng(3)
    q, _ = make_family(rng, d, avi.MEANFIELD, np.float32)
    prob, _ = make_problem(rng, "diag", d, np.float32)
    params, _ = avi.destructure(q)

    def gaussian():
        ctx = avi.MiviContext(np.float32, avi.MEANFIELD, d, M, avi.StickingTheLandingEntropy.code, SEED)
        ctx.set_problem(prob)
        v, g = ctx.estimate_gradient(params, 5)
        ctx.synchronize()
        out = v.clone(), g.clone()
        ctx.close()
        return out

    before = gaussian()
    run_case(MID, avi.StickingTheLandingEntropy(), np.float32)
    after = gaussian()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


# ---- loops ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("opt", [avi.Descent(1e-3), avi.Adam(0.01), avi.DoWG()], ids=lambda o: type(o).__name__)
@pytest.mark.parametrize("averager", [avi.NoAveraging(), avi.PolynomialAveraging()], ids=lambda a: type(a).__name__)
def test_device_loop_equals_host_loop(averager, opt, dtype):
    d, hidden, L, M = MID
    prob, _ = make_target(MID, "dense", dtype)
    q0 = avi.RealNVP(d, hidden, L, eltype=dtype, rng=1)
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), entropy=avi.StickingTheLandingEntropy(), optimizer=opt, n_samples=M, averager=averager,
                                  operator=avi.IdentityOperator())
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # no location-scale IdentityOperator warning for a flow
        q_dev, info_dev, st = avi.optimize(avi.PhiloxRNG(SEED), alg, 20, prob, q0)
        q_host, info_host, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 20, prob, q0, device_loop=False)
    assert isinstance(q_dev, avi.RealNVPFlow) and len(info_dev) == 20
    a, b = avi.destructure(q_dev)[0], avi.destructure(q_host)[0]
    assert not np.array_equal(a, q0.params)
    if isinstance(opt, avi.DoG):   # DoG / DoWG: the two norms are summed in another order on the device
        assert rel_err(a, b) < (1e-5 if dtype == np.float32 else 1e-12)
    else:
        assert np.array_equal(a, b)
        assert [i["elbo"] for i in info_dev] == [i["elbo"] for i in info_host]


class MultDegen:
    """docs/src/tutorials/flows.md:28-50: alpha ~ LogNormal(0, 1), beta ~ Normal(0, 10), y_i ~ Normal(alpha beta, 1); `logdensity` alone."""

    def __init__(self, y):
        self.y = np.asarray(y, dtype=np.float64)

    def logdensity(self, theta):
        alpha, beta = theta[0], theta[1]
        la = np.log(alpha)
        logprior_alpha = -la - 0.5 * math.log(2 * math.pi) - 0.5 * la * la
        logprior_beta = -math.log(10.0) - 0.5 * math.log(2 * math.pi) - 0.5 * beta * beta / 100.0
        loglike = sum(-0.5 * math.log(2 * math.pi) - 0.5 * (yi - alpha * beta) * (yi - alpha * beta) for yi in self.y)
        return logprior_alpha + logprior_beta + loglike

    def dimension(self):
        return 2

    def capabilities(self):
        return avi.LogDensityOrder(0)


def _improves(info, n):
    elbo = np.array([i["elbo"] for i in info])
    assert len(elbo) == n and np.all(np.isfinite(elbo))
    assert elbo[-50:].mean() > elbo[:50].mean(), (elbo[:50].mean(), elbo[-50:].mean())


def test_tutorial_end_to_end_on_the_banana_posterior():
    """flows.md: RealNVP(2, [16, 16], 3), Adam(1e-2), 8 samples, sticking the landing, IdentityOperator, behind Stacked([exp, identity]);
    the model has `logdensity` alone, so the steps run on the host loop through AutoMIVI(target_ad="forwarddiff")."""
    prob = avi.TransformedProblem(MultDegen([3.0]), avi.StackedBijector([(0, 1, "exp"), (1, 2, "identity")]))
    q0 = avi.RealNVP(2, [16, 16], 3)
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(target_ad="forwarddiff"), entropy=avi.StickingTheLandingEntropy(), optimizer=avi.Adam(1e-2),
                                  n_samples=8, averager=avi.NoAveraging(), operator=avi.IdentityOperator())
    q, info, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 300, prob, q0)
    assert isinstance(q, avi.RealNVPFlow)
    _improves(info, 300)


def test_constrained_funnel_on_the_device_loop():
    d = 2
    prob = avi.TransformedProblem(avi.FunnelConstrainedProblem(d, 1.5), avi.StackedBijector([(0, 1, "exp"), (1, d, "identity")]))
    q0 = avi.RealNVP(d, [16, 16], 3)
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), entropy=avi.StickingTheLandingEntropy(), optimizer=avi.Adam(1e-2), n_samples=8,
                                  averager=avi.NoAveraging(), operator=avi.IdentityOperator())
    q, info, st = avi.optimize(avi.PhiloxRNG(SEED), alg, 300, prob, q0)
    _improves(info, 300)
    q_host, info_host, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 300, prob, q0, device_loop=False)
    assert np.array_equal(q.params, q_host.params)   # the steps DID run in the device loop's graph, and it is the host-driven loop


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _create_flow(d=4, n_mc=4, entropy=2, L=2, hidden=(8,), m_offset=0, m_total=0, family=3, entry="mivi_create_flow"):
    lib = _lib.load()
    cfg = _lib.MiviConfig(_lib.F32, family, d, n_mc, entropy, 0, C.c_uint64(1), m_offset, m_total, None, 0, 0)
    hid = list(hidden) + [0] * (3 - len(hidden))
    arch = _lib.MiviFlow(L, len(hidden), (C.c_int32 * 3)(*hid[:3]))
    h = C.c_void_p()
    st = lib.mivi_create_flow(C.byref(cfg), C.byref(arch), C.byref(h)) if entry == "mivi_create_flow" else lib.mivi_create(C.byref(cfg), C.byref(h))
    if st == 0:
        lib.mivi_destroy(h)
    return st


def test_create_checks_limits_estimators_and_entry():
    assert C.sizeof(_lib.MiviConfig) == 56 and C.sizeof(_lib.MiviFlow) == 20
    assert _create_flow() == 0 and _create_flow(d=2, L=1, hidden=(1,)) == 0 and _create_flow(d=128, L=32, hidden=(64, 64, 64)) == 0
    assert _create_flow(entry="mivi_create") == _lib.ERR_BAD_ARG          # family 3 goes through mivi_create_flow
    assert _create_flow(family=avi.MEANFIELD) == _lib.ERR_BAD_ARG       # ... and only family 3 does
    for bad in (dict(d=1), dict(d=129), dict(L=0), dict(L=33), dict(hidden=(0,)), dict(hidden=(65,)), dict(hidden=(8, 8, 70)), dict(n_mc=0)):
        assert _create_flow(**bad) == _lib.ERR_BAD_ARG, bad
    for ent in (0, 1, 4):
        assert _create_flow(entropy=ent) == _lib.ERR_UNSUPPORTED, ent
    assert _create_flow(entropy=3) == 0
    assert _create_flow(m_offset=4) == _lib.ERR_UNSUPPORTED and _create_flow(m_total=8) == _lib.ERR_UNSUPPORTED and _create_flow(m_total=4) == 0


def test_unsupported_entries_refuse_the_family():
    """Every entry outside the family's surface returns MIVI_ERR_UNSUPPORTED with a message naming the entry and the family."""
    case = (8, (8,), 2, 4)
    d, M = case[0], case[3]
    ctx = make_ctx(case, avi.MonteCarloEntropy(), np.float32, avi.DiagNormalProblem(np.zeros(d, np.float32), np.ones(d, np.float32)))
    lib, h = ctx.lib, ctx.h
    buf = ctx.empty(4 * (d * d + d * M) + ctx.params_len + 64)
    host = np.zeros(4 * (d * d + d * M) + ctx.params_len + 64, dtype=np.float32)
    P, Hp = ctx._p(buf), host.ctypes.data
    dbl = (C.c_double * 8)()
    loop = _lib.MiviLoop(0, 0, 0, 2, 0.1, 0.9, 0.999, 1e-8, 0.0, 8.0, None, None, 0, 0, None)
    many = _lib.MiviMany(1, None, None, None, None, None, None, None, 0, None)
    rows = np.zeros((2, 2), dtype=np.int64)
    sched = _lib.MiviBatchSchedule(rows.ctypes.data, None, 2, 2, 0, 1.0)
    calls = {
        "mivi_estimate_score_gradient": lambda: lib.mivi_estimate_score_gradient(h, P, 0, P, P, P),
        "mivi_estimate_score_gradient_host": lambda: lib.mivi_estimate_score_gradient_host(h, Hp, 0, Hp, Hp, Hp),
        "mivi_gauss_expected_grad_hess": lambda: lib.mivi_gauss_expected_grad_hess(h, P, 0, 0, P, P, P),
        "mivi_gauss_expected_grad_hess2": lambda: lib.mivi_gauss_expected_grad_hess2(h, P, 0, 0, P, P, P),
        "mivi_gauss_expected_grad_hess_host": lambda: lib.mivi_gauss_expected_grad_hess_host(h, Hp, 0, 0, Hp, Hp, Hp),
        "mivi_sqrt_ngd_update": lambda: lib.mivi_sqrt_ngd_update(h, P, P, P, 0.1, P),
        "mivi_sqrt_ngd_steps": lambda: lib.mivi_sqrt_ngd_steps(h, P, 0, 1, 0, 0, 0.1, P),
        "mivi_natgrad_init": lambda: lib.mivi_natgrad_init(h, P, P),
        "mivi_natgrad_update": lambda: lib.mivi_natgrad_update(h, P, P, P, P, 0.1, 1, P),
        "mivi_natgrad_steps": lambda: lib.mivi_natgrad_steps(h, P, P, 0, 1, 0, 0, 0.1, 1, P),
        "mivi_bam_init": lambda: lib.mivi_bam_init(h, P, P),
        "mivi_bam_moments": lambda: lib.mivi_bam_moments(h, P, 0, 4, P, P, P, P, P),
        "mivi_estimate_fisher": lambda: lib.mivi_estimate_fisher(h, P, 0, 4, P),
        "mivi_bam_update": lambda: lib.mivi_bam_update(h, P, P, P, P, 4, 1.0, P),
        "mivi_bam_steps": lambda: lib.mivi_bam_steps(h, P, P, 0, 1, 1, 4, P, P),
        "mivi_wass_init": lambda: lib.mivi_wass_init(h, P, P),
        "mivi_wass_update": lambda: lib.mivi_wass_update(h, P, P, P, P, 0.1, P),
        "mivi_wass_steps": lambda: lib.mivi_wass_steps(h, P, P, 0, 1, 0, 0, 0.1, P),
        "mivi_estimate_partials": lambda: lib.mivi_estimate_partials(h, P, 0, P),
        "mivi_finalize": lambda: lib.mivi_finalize(h, P, P, P, P),
        "mivi_estimate_gradient_dist": lambda: lib.mivi_estimate_gradient_dist(h, P, 0, P, P),
        "mivi_estimate_gradient_dist_n": lambda: lib.mivi_estimate_gradient_dist_n(h, P, 0, 2, P, P),
        "mivi_prox_scale_entropy": lambda: lib.mivi_prox_scale_entropy(h, P, 0.1, None, 0),
        "mivi_set_base_dist": lambda: lib.mivi_set_base_dist(h, 1, 0.0),
        "mivi_optimize_loop_many": lambda: lib.mivi_optimize_loop_many(h, P, C.byref(loop), C.byref(many)),
        "mivi_logpdf": lambda: lib.mivi_logpdf(h, P, P, 1, P, P),
        "mivi_logreg_set_batch_schedule": lambda: lib.mivi_logreg_set_batch_schedule(h, C.byref(sched)),
        "mivi_logreg_seek_batch": lambda: lib.mivi_logreg_seek_batch(h, 0),
        "mivi_optimize_loop_batches": lambda: lib.mivi_optimize_loop_batches(h, P, C.byref(loop), 0),
    }
    for name, call in calls.items():
        assert call() == _lib.ERR_UNSUPPORTED, name
        msg = lib.mivi_last_error(h).decode()
        assert "RealNVP" in msg and name.replace("_host", "") in msg, (name, msg)
    for op in (1, 2):   # ClipScale and the proximal operator: no method for a family without a scale
        with pytest.raises(avi.MiviError) as e:
            ctx.optimize_loop(buf, 2, 0, 0, rule=0, op=op, eta=0.1)
        assert e.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(avi.MiviError) as e:
        ctx.clip_scale(buf, 1e-5)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    ctx.close()


def test_python_combinations_without_a_method_raise_type_errors():
    d = 4
    q = avi.RealNVP(d, [8], 2, eltype=np.float32)
    prob = avi.DiagNormalProblem(np.zeros(d, np.float32), np.ones(d, np.float32))
    rng = lambda: avi.PhiloxRNG(SEED)   # noqa: E731
    ident = dict(operator=avi.IdentityOperator(), entropy=avi.StickingTheLandingEntropy())
    with pytest.raises(TypeError, match="IdentityOperator"):
        avi.optimize(rng(), avi.KLMinRepGradDescent(avi.AutoMIVI(), entropy=avi.StickingTheLandingEntropy(), operator=avi.ClipScale()), 2, prob, q)
    with pytest.raises(TypeError, match="IdentityOperator"):
        avi.optimize(rng(), avi.KLMinRepGradProxDescent(avi.AutoMIVI(), optimizer=avi.Descent(0.1)), 2, prob, q)
    with pytest.raises(TypeError, match="StickingTheLandingEntropy"):
        avi.optimize(rng(), avi.KLMinRepGradDescent(avi.AutoMIVI(), entropy=avi.ClosedFormEntropy(), operator=avi.IdentityOperator()), 2, prob, q)
    with pytest.raises(TypeError, match="KLMinRepGradDescent"):
        avi.optimize(rng(), avi.KLMinScoreGradDescent(avi.AutoMIVI(), n_samples=4, operator=avi.IdentityOperator()), 2, prob, q)
    with pytest.raises(TypeError, match="optimize"):
        avi.optimize_many([rng(), rng()], avi.KLMinRepGradDescent(avi.AutoMIVI(), **ident), 2, prob, q)
    for alg in (avi.KLMinSqrtNaturalGradDescent, avi.KLMinNaturalGradDescent, avi.KLMinWassFwdBwd):
        with pytest.raises(TypeError, match="KLMinRepGradDescent"):
            avi.optimize(rng(), alg(0.1), 2, prob, q)
    with pytest.raises(TypeError, match="KLMinRepGradDescent"):
        avi.optimize(rng(), avi.FisherMinBatchMatch(), 2, prob, q)


def test_subsampled_optimize_on_a_flow_keeps_the_host_loop():
    """The batch schedule refuses the family, so `optimize` with subsampling over the built-in logistic regression runs host-driven
    steps (mivi_logreg_select_rows per step): the result is that of device_loop=False, and the context never holds a schedule."""
    d = 5
    prob, _ = make_problem(np.random.default_rng(2), "logreg0", d, np.float64)
    q0 = avi.RealNVP(d, [8], 2, rng=2)
    sub = avi.ReshufflingBatchSubsampling(np.arange(64), 16)
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), entropy=avi.StickingTheLandingEntropy(), optimizer=avi.Adam(1e-2), n_samples=4,
                                  averager=avi.NoAveraging(), operator=avi.IdentityOperator(), subsampling=sub)
    q, info, st = avi.optimize(avi.PhiloxRNG(SEED), alg, 6, prob, q0)
    q_host, info_host, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 6, prob, q0, device_loop=False)
    assert np.array_equal(q.params, q_host.params) and [i["elbo"] for i in info] == [i["elbo"] for i in info_host]
    assert len(info) == 6 and all(np.isfinite(i["elbo"]) for i in info)


def test_zero_weights_first_descent_step_moves_only_the_output_layers():
    """With every weight zero nothing reaches a hidden layer's parameters: the first step moves output-layer entries alone."""
    d, hidden, L = 5, (16, 7), 2
    q0 = avi.RealNVPFlow(d, hidden, L, np.zeros(avi.flow_layout(d, hidden, L)[1]))
    prob, _ = make_target(MID, "dense", np.float64)
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), entropy=avi.MonteCarloEntropy(), optimizer=avi.Descent(1e-2), n_samples=8,
                                  averager=avi.NoAveraging(), operator=avi.IdentityOperator())
    q, _, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 1, prob, q0)
    moved = q.params != 0
    assert moved.any()
    for name, sl in R.blocks((d, hidden, L)):
        if not name.endswith(str(len(hidden) + 1)):
            assert not moved[sl].any(), name
