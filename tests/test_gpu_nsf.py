"""GPU tests of the neural spline flow family (MIVI_NSF, defined in include/mivi.h): libmivi through the C ABI against tests/nsf_ref.py on
the same Philox stream.

The rule is that of tests/test_gpu_flow.py (nsf_ref.report): for float32 contexts the error against the numpy evaluation in float64
(tests/test_nsf_ref_host.py pins it to torch autograd) is at most 8 x the error of the same evaluation in float32, floored at
flow_ref's tolerances; for float64 contexts the reference is the evaluation in long double and the bound of the value and the gradient
flow_ref.TOL alone (the sample and log q: 8 x the float64 evaluation's own error, floored, as in tests/test_gpu_flow.py).  The
gradient is held to it as a whole AND per parameter block (each W_j and b_j of each layer's net).  Every case keeps its spline inputs
off the knots and its hidden units off the kink (nsf_ref.CASES; pinned on the CPU), so nothing here is skipped."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import _lib
from oracle import oracle as O
from tests import nsf_ref as N
from tests.helpers import SEED, OraclePlugin, make_problem, rel_err

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
KINDS = [avi.MonteCarloEntropy(), avi.StickingTheLandingEntropy()]
IDX = N.CASE_IDX
MID = N.MID


def _id(case):
    return f"{case[0]}-{'x'.join(map(str, case[1]))}-{case[2]}-K{case[3]}-B{case[4]}-{case[5]}"


def make_ctx(case, ent, dtype, prob=None, n_mc=None):
    d, hidden, L, K, B, M = case
    ctx = avi.MiviContext(dtype, avi.NSF, d, n_mc or M, ent.code, SEED, flow=(hidden, L, K, B))
    if prob is not None:
        ctx.set_problem(prob)
    return ctx


def make_target(case, kind, dtype, plugin=False, bijector=False):
    d, M = case[0], case[5]
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
        arch = N.arch_of(case)
        zeros = np.zeros(eps.shape)
        ell, G = N.target_columns(tgt, N.evaluate(params, arch, zeros, zeros[0], eps, N.MONTE_CARLO, np.float64)["Z"])
        _REF[key] = (N.evaluate(params, arch, G, ell, eps, kind, N.wider(dtype)),
                     N.evaluate(params, arch, G, ell, eps, kind, dtype))
    return _REF[key]


def run_case(case, ent, dtype, kind="diag", plugin=False, bijector=False):
    d, hidden, L, K, B, M = case
    arch = N.arch_of(case)
    params = N.case_params(case, dtype)
    prob, tgt = make_target(case, kind, dtype, plugin, bijector)
    ctx = make_ctx(case, ent, dtype, prob)
    assert ctx.params_len == params.shape[0] == avi.nsf_layout(d, hidden, L, K)[1] == N.nsf_layout(d, hidden, L, K)[1] and ctx.partials_len == 0
    Z, eps = ctx.sample(params, IDX)
    assert eps.shape == (d, M)
    eps, Z = eps.cpu().numpy().astype(np.float64), Z.cpu().numpy().astype(np.float64)
    assert rel_err(eps, O.philox_normal(SEED, IDX, d, 0, M, f64=dtype == np.float64)) < N.STOL[np.dtype(dtype)]
    value, grad = ctx.estimate_gradient(params, IDX)
    ctx.synchronize()
    got = dict(Z=Z, value=float(value.item()), grad=grad.cpu().numpy().astype(np.float64))
    ctx.close()
    key = (case, kind, ent.code, np.dtype(dtype).name, plugin, bijector)
    ref, yard = reference(key, case, params, tgt, eps, ent.code, dtype)
    rows = N.report(got, ref, yard, arch, dtype)
    print(f"[nsf] {key}: worst ratios {N.worst_ratios(rows)}")
    for name, err, bound in rows:
        print(f"[nsf]   {name}: err {err:.3e} (bound {bound:.3e})")
    assert not N.violations(rows), N.violations(rows)


# ---- parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ent", KINDS, ids=lambda e: type(e).__name__)
@pytest.mark.parametrize("case", list(N.CASES), ids=_id)
def test_diag_target_both_estimators_all_shapes(case, ent, dtype):
    run_case(case, ent, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ent", KINDS, ids=lambda e: type(e).__name__)
@pytest.mark.parametrize("kind,plugin,bijector", [("dense", False, False), ("logreg0", False, False), ("funnel", False, False),
                                                  ("diag", True, False), ("dense", False, True)],
                         ids=["dense", "logreg", "funnel", "plugin", "stacked"])
def test_targets_plugin_and_bijector(kind, plugin, bijector, ent, dtype):
    run_case(MID, ent, dtype, kind=kind, plugin=plugin, bijector=bijector)


# ---- rand and logpdf ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [MID, (4, (8,), 2, 4, 0.5, 64)], ids=_id)
def test_rand_and_logpdf_of_own_samples(case, dtype):
    d, M, arch = case[0], case[5], N.arch_of(case)
    params = N.case_params(case, dtype)
    ctx = make_ctx(case, avi.MonteCarloEntropy(), dtype)
    Z, eps = ctx.sample(params, IDX)
    # the draws ARE the mean-field family's stream, bit for bit; z does not depend on whether eps is asked for, nor on the context
    mf = avi.MiviContext(dtype, avi.MEANFIELD, d, M, 2, SEED)
    assert torch.equal(eps, mf.sample(np.concatenate([np.zeros(d, dtype), np.ones(d, dtype)]), IDX)[1])
    mf.close()
    assert torch.equal(Z, ctx.sample(params, IDX, want_eps=False))
    fresh = make_ctx(case, avi.StickingTheLandingEntropy(), dtype)
    Z2, eps2 = fresh.sample(params, IDX)
    assert torch.equal(Z2, Z) and torch.equal(eps2, eps)
    fresh.close()
    e64 = eps.cpu().numpy().astype(np.float64)
    zeros = np.zeros_like(e64)
    ref = N.evaluate(params, arch, zeros, zeros[0], e64, 2, N.wider(dtype))
    yard = N.evaluate(params, arch, zeros, zeros[0], e64, 2, dtype)
    got = ctx.logpdf(params, Z)
    got_h = ctx.logpdf_host(params, Z.cpu().numpy())
    rows = N.report(dict(Z=Z.cpu().numpy(), logq=got.cpu().numpy()), ref, yard, arch, dtype)
    print(f"[nsf] rand / logpdf of own samples {_id(case)} {np.dtype(dtype).name}: {rows}")
    assert not N.violations(rows), rows
    assert np.array_equal(got_h, got.cpu().numpy())
    ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_logpdf_of_points_in_the_tails_and_constrained_logpdf(dtype):
    case = MID
    d, B, arch = case[0], case[4], N.arch_of(case)
    params = N.case_params(case, dtype)
    ctx = make_ctx(case, avi.MonteCarloEntropy(), dtype)
    # every coordinate outside [-B, B] (and exactly on +-B): every layer is the identity there, log q is the standard normal's
    gen = np.random.default_rng(11)
    far = (gen.choice([-1.0, 1.0], size=(d, 21)) * (B + gen.uniform(0.0, 4.0, size=(d, 21)))).astype(dtype)
    far[:, 0], far[:, 1] = B, -B
    want = -0.5 * (far.astype(np.float64) ** 2).sum(axis=0) - 0.5 * d * math.log(2 * math.pi)
    got = ctx.logpdf(params, far).cpu().numpy().astype(np.float64)
    vt = N.TOL[np.dtype(dtype)][0]
    assert np.abs(got - want).max() <= vt * np.abs(want).max(), np.abs(got - want).max()
    # some coordinates inside, some in the tails, against the inverse layers of the reference
    mixed = (gen.normal(size=(d, 40)) * 2.5).astype(dtype)
    assert (np.abs(mixed) > B).any() and (np.abs(mixed) < B).any()
    _, ref = N.inverse_np(params, arch, mixed, N.wider(dtype))
    _, yard = N.inverse_np(params, arch, mixed, dtype)
    rows = N.report(dict(logq=ctx.logpdf(params, mixed).cpu().numpy()), dict(logq=ref), dict(logq=yard), arch, dtype)
    print(f"[nsf] logpdf at mixed points {np.dtype(dtype).name}: {rows}")
    assert not N.violations(rows), rows
    # through Stacked([exp on three coordinates, identity]): log q(b(x)) - logabsdetjac(binv, b(x)), b(x) = z
    Z = ctx.sample(params, IDX, want_eps=False)
    lq = ctx.logpdf(params, Z).cpu().numpy().astype(np.float64)
    ctx.set_bijector(avi.StackedBijector([(0, 3, "exp"), (3, d, "identity")]))
    X, eta = ctx.sample_constrained(params, IDX, want_eta=True)
    assert torch.equal(eta, Z) and torch.equal(X[3:], Z[3:]) and bool((X[:3] > 0).all())
    got_c = ctx.logpdf_constrained(params, X).cpu().numpy().astype(np.float64)
    z64 = Z.cpu().numpy().astype(np.float64)
    want_c = lq - z64[:3].sum(axis=0)
    bound_c = 16 * np.finfo(dtype).eps * (np.abs(lq).max() + np.abs(z64[:3]).sum(axis=0).max())   # log(exp(z)), its inverse layers and the sum, in dtype
    print(f"[nsf] constrained logpdf: err {np.abs(got_c - want_c).max():.3e} (bound {bound_c:.3e})")
    assert np.abs(got_c - want_c).max() <= bound_c
    ctx.close()


def test_rand_logpdf_and_transformed_distribution_take_the_flow():
    q = avi.NeuralSplineFlow(5, [8], 4, 3.0, 3, rng=4)
    assert len(q) == 5 and q.hidden_dims == (8,) and q.n_layers == 3 and q.n_bins == 4 and q.bound == 3.0
    assert q.eltype == np.float64 and q.family == avi.NSF and isinstance(q, avi.SplineFlow)
    assert set(q.blocks()) == {(l, j, k) for l in (1, 2, 3) for j in (1, 2) for k in "Wb"} and q.blocks()[(1, 2, "W")].shape == (3 * 11, 8)
    flat, re_ = avi.destructure(q)
    back = re_(flat)
    assert np.array_equal(back.params, q.params) and (back.hidden_dims, back.n_layers, back.n_bins, back.bound) == ((8,), 3, 4, 3.0)
    rng = avi.PhiloxRNG(SEED)
    idx = rng.counter
    Z = avi.rand(rng, q, 7)
    assert tuple(Z.shape) == (5, 7) and rng.counter == idx + 1
    ctx = make_ctx((5, (8,), 3, 4, 3.0, 7), avi.MonteCarloEntropy(), np.float64)
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


# ---- contracts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [MID, (8, (16,), 4, 8, 30.0, 1040)], ids=_id)
def test_batched_entries_repeated_calls_and_a_fresh_context_are_bitwise(case, dtype):
    params = N.case_params(case, dtype)
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
    fresh = make_ctx(case, avi.StickingTheLandingEntropy(), dtype, prob)
    vf, gf = fresh.estimate_gradient(params, 7)
    fresh.synchronize()
    assert torch.equal(vf, singles[0][0]) and torch.equal(gf, singles[0][1])
    fresh.close()
    ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_estimate_objective_any_n_samples(dtype):
    case = MID
    d, arch = case[0], N.arch_of(case)
    params = N.case_params(case, dtype)
    prob, tgt = make_target(case, "diag", dtype)
    ctx = make_ctx(case, avi.MonteCarloEntropy(), dtype, prob, n_mc=16)
    vt = 1e-5 if dtype == np.float32 else 1e-11   # (tests/test_gpu_flow.py::test_estimate_objective_any_n_samples)
    for n in (1, 33, 5000):
        eps = O.philox_normal(SEED, 2, d, 0, n, f64=dtype == np.float64).astype(np.float64)
        zeros = np.zeros_like(eps)
        fw = N.evaluate(params, arch, zeros, zeros[0], eps, 2, np.float64)
        ell, _ = N.target_columns(tgt, fw["Z"])
        want = float(np.mean(-ell + fw["logq"]))
        for ent in KINDS:
            got = float(ctx.estimate_objective(params, 2, n_samples=n, entropy=ent.code).item())
            print(f"[nsf] estimate_objective n = {n}, kind {ent.code}: {got} against {want}")
            assert abs(got - want) <= vt * abs(want), (n, got, want)
        if n == 33:
            assert abs(float(ctx.estimate_objective_host(params, 2, n_samples=n)) - want) <= vt * abs(want)
    with pytest.raises(avi.MiviError) as e:   # a closed-form kind needs entropy(q)
        ctx.estimate_objective(params, 2, n_samples=8, entropy=avi.ClosedFormEntropy.code)
    assert e.value.status == _lib.ERR_UNSUPPORTED and "MonteCarloEntropy" in str(e.value)
    ctx.close()


# ---- loops ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("opt", [avi.Descent(1e-3), avi.Adam(0.01)], ids=lambda o: type(o).__name__)
def test_device_loop_equals_host_driven_steps(opt, dtype):
    d, hidden, L, K, B, M = MID
    prob, _ = make_target(MID, "dense", dtype)
    q0 = avi.NeuralSplineFlow(d, hidden, K, B, L, eltype=dtype, rng=1)
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), entropy=avi.StickingTheLandingEntropy(), optimizer=opt, n_samples=M, averager=avi.NoAveraging(),
                                  operator=avi.IdentityOperator())
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # no location-scale IdentityOperator warning for a flow
        q_dev, info_dev, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 20, prob, q0)
        q_host, info_host, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 20, prob, q0, device_loop=False)
    assert isinstance(q_dev, avi.SplineFlow) and len(info_dev) == 20
    a, b = avi.destructure(q_dev)[0], avi.destructure(q_host)[0]
    assert not np.array_equal(a, q0.params)
    assert np.array_equal(a, b)
    assert [i["elbo"] for i in info_dev] == [i["elbo"] for i in info_host]


class Banana:
    """log pi(z) = -1/2 (z_1 / 2)^2 - 1/2 (z_2 - z_1^2 / 4)^2 (up to a constant): a bent Gaussian no location-scale family fits."""

    def dimension(self):
        return 2

    def logdensity(self, z):
        return -0.125 * z[0] * z[0] - 0.5 * (z[1] - 0.25 * z[0] * z[0]) ** 2

    def logdensity_and_gradient(self, z):
        r = z[1] - 0.25 * z[0] * z[0]
        return self.logdensity(z), np.array([-0.25 * z[0] + 0.5 * z[0] * r, -r])


def test_a_short_optimize_lowers_the_objective_on_a_banana_plugin_target():
    q0 = avi.NeuralSplineFlow(2, [16, 16], 8, 6.0, 3)
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), entropy=avi.StickingTheLandingEntropy(), optimizer=avi.Adam(1e-2), n_samples=8,
                                  averager=avi.NoAveraging(), operator=avi.IdentityOperator())
    q, info, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 150, OraclePlugin(Banana()), q0)
    assert isinstance(q, avi.SplineFlow)
    elbo = np.array([i["elbo"] for i in info])
    assert len(elbo) == 150 and np.all(np.isfinite(elbo))
    assert elbo[-40:].mean() > elbo[:40].mean(), (elbo[:40].mean(), elbo[-40:].mean())


def test_subsampled_optimize_on_a_spline_flow_keeps_the_host_loop():
    d = 5
    prob, _ = make_problem(np.random.default_rng(2), "logreg0", d, np.float64)
    q0 = avi.NeuralSplineFlow(d, [8], 4, 3.0, 2, rng=2)
    sub = avi.ReshufflingBatchSubsampling(np.arange(64), 16)
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), entropy=avi.StickingTheLandingEntropy(), optimizer=avi.Adam(1e-2), n_samples=4,
                                  averager=avi.NoAveraging(), operator=avi.IdentityOperator(), subsampling=sub)
    q, info, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 6, prob, q0)
    q_host, info_host, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 6, prob, q0, device_loop=False)
    assert np.array_equal(q.params, q_host.params) and [i["elbo"] for i in info] == [i["elbo"] for i in info_host]
    assert len(info) == 6 and all(np.isfinite(i["elbo"]) for i in info)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _create(d=4, n_mc=4, entropy=2, L=2, hidden=(8,), K=4, B=3.0, m_offset=0, m_total=0, family=4, entry="mivi_create_spline_flow", dtype=_lib.F32):
    lib = _lib.load()
    cfg = _lib.MiviConfig(dtype, family, d, n_mc, entropy, 0, C.c_uint64(1), m_offset, m_total, None, 0, 0)
    hid = list(hidden) + [0] * (3 - len(hidden))
    h = C.c_void_p()
    if entry == "mivi_create_spline_flow":
        st = lib.mivi_create_spline_flow(C.byref(cfg), C.byref(_lib.MiviSplineFlow(L, len(hidden), (C.c_int32 * 3)(*hid[:3]), K, B)), C.byref(h))
    elif entry == "mivi_create_flow":
        st = lib.mivi_create_flow(C.byref(cfg), C.byref(_lib.MiviFlow(L, len(hidden), (C.c_int32 * 3)(*hid[:3]))), C.byref(h))
    else:
        st = lib.mivi_create(C.byref(cfg), C.byref(h))
    if st == 0:
        lib.mivi_destroy(h)
    return st


def test_create_checks_limits_estimators_and_entry():
    assert C.sizeof(_lib.MiviSplineFlow) == 32
    assert _create() == 0 and _create(dtype=_lib.F64) == 0 and _create(d=2, L=1, hidden=(1,), K=2) == 0
    assert _create(d=128, L=32, hidden=(64, 64, 64), K=16, B=1e-3) == 0
    assert _create(entry="mivi_create") == _lib.ERR_BAD_ARG and _create(entry="mivi_create_flow") == _lib.ERR_BAD_ARG   # family 4 has its own entry
    for fam in (avi.MEANFIELD, avi.FULLRANK, avi.LOWRANK, avi.REALNVP):
        assert _create(family=fam) == _lib.ERR_BAD_ARG, fam       # ... and only family 4 goes through it
    for bad in (dict(d=1), dict(d=129), dict(L=0), dict(L=33), dict(hidden=(0,)), dict(hidden=(65,)), dict(hidden=(8, 8, 70)), dict(n_mc=0),
                dict(K=1), dict(K=17), dict(K=0), dict(B=0.0), dict(B=-1.0), dict(B=math.inf), dict(B=math.nan), dict(entropy=5), dict(entropy=-1)):
        assert _create(**bad) == _lib.ERR_BAD_ARG, bad
    for ent in (0, 1, 4):
        assert _create(entropy=ent) == _lib.ERR_UNSUPPORTED, ent
    assert _create(entropy=3) == 0
    assert _create(m_offset=4) == _lib.ERR_UNSUPPORTED and _create(m_total=8) == _lib.ERR_UNSUPPORTED and _create(m_total=4) == 0
    with pytest.raises(avi.MiviError, match="entropy"):
        avi.MiviContext(np.float32, avi.NSF, 4, 4, 0, SEED, flow=((8,), 2, 4, 3.0))
    with pytest.raises(avi.MiviError, match="sharded"):
        avi.MiviContext(np.float32, avi.NSF, 4, 4, 2, SEED, m_offset=4, flow=((8,), 2, 4, 3.0))
    with pytest.raises(ValueError):
        avi.MiviContext(np.float32, avi.NSF, 4, 4, 2, SEED, flow=((8,), 2))
    for bad in (dict(n_bins=1), dict(n_bins=17), dict(bound=0.0), dict(bound=math.inf)):
        with pytest.raises(ValueError):
            avi.NeuralSplineFlow(4, [8], **{**dict(n_bins=4, bound=3.0, n_layers=2), **bad})


def test_unsupported_entries_refuse_the_family():
    """Every entry RealNVP is refused on refuses this family, with a message naming the entry and the family's own name."""
    case = (8, (8,), 2, 4, 3.0, 4)
    d, M = case[0], case[5]
    ctx = make_ctx(case, avi.MonteCarloEntropy(), np.float32, avi.DiagNormalProblem(np.zeros(d, np.float32), np.ones(d, np.float32)))
    lib, h = ctx.lib, ctx.h
    buf = ctx.empty(4 * (d * d + d * M) + ctx.params_len + 64)
    host = np.zeros(4 * (d * d + d * M) + ctx.params_len + 64, dtype=np.float32)
    P, Hp = ctx._p(buf), host.ctypes.data
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
        assert "neural spline flow" in msg and "MIVI_NSF" in msg and "RealNVP" not in msg and name.replace("_host", "") in msg, (name, msg)
    for op in (1, 2):   # ClipScale and the proximal operator: no method for a family without a scale
        with pytest.raises(avi.MiviError) as e:
            ctx.optimize_loop(buf, 2, 0, 0, rule=0, op=op, eta=0.1)
        assert e.value.status == _lib.ERR_UNSUPPORTED and "neural spline flow" in str(e.value)
    with pytest.raises(avi.MiviError) as e:
        ctx.clip_scale(buf, 1e-5)
    assert e.value.status == _lib.ERR_UNSUPPORTED and "mivi_clip_scale" in str(e.value) and "neural spline flow" in str(e.value)
    assert ctx.lib.mivi_set_base_dist(h, 0, 0.0) == 0   # the normal base changes nothing
    ctx.close()


def test_python_combinations_without_a_method_raise_type_errors():
    d = 4
    q = avi.NeuralSplineFlow(d, [8], 4, 3.0, 2, eltype=np.float32)
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
    with pytest.raises(TypeError, match="NeuralSplineFlow"):
        avi.optimize(rng(), avi.KLMinRepGradDescent(avi.AutoMIVI(), entropy=avi.StickingTheLandingEntropy(), operator=avi.ClipScale()), 2, prob, q)
