"""The RealNVP flow kernels -- k_flow_forward (rand, and the inverse of logpdf), k_flow_vjp, k_flow_finish (csrc/kernels_flow.hip) -- held
PER ENTRY to a float32 yardstick, at the smallest shapes that reach each mechanism the gradient tests of tests/test_gpu_flow.py do not:
several tiles per slice (the accumulate branch, the reuse of the LDS blocks, a partial last tile that is a slice's third), depth 32
(flow_layer_off and the [L + 1][capM][d] planes at large l), the widest net with every [64][16] block full, odd d at the limit, the
inverse at points that are not the context's own samples, saturated tanh, and a hidden unit at exactly 0.  tests/test_gpu_flow.py bounds
the l2 distance of the gradient as a whole and per parameter block: one entry of a 64 x 64 weight block off by a relative 1e-3, and one
row of it off by 1e-4, both pass that (tests/test_flow_ref_host.py prints the figures: this file's entry ratio 3.2e2 / 4.3e2 and
5.3e2 / 4.7e2 against the factor 8).

Criterion (tests/flow_ref.py): ref is `evaluate` in the next wider type (float64 for an f32 context, np.longdouble for f64) on the
device's own draws, env per entry the largest distance from it of eight sample orders of `evaluate` in the element type (the kernels'
own order among them), S the first-order magnitude of a running error analysis of the documented formulas with the error of x^{l-1}
carried into layer l, u = 2^-24 / 2^-53, and every ratio |got - ref| / max(env, u S) -- per entry, per row of each W_j and per b_j in
l2, the whole gradient in l2, the value, Z and log q per entry -- is at most F32_FACTOR = 8 of tests/measure_space_cases.py.  The
per-block criterion of tests/test_gpu_flow.py (flow_ref.block_report) is asserted beside it.  Every case's inputs keep every leakyrelu
off its kink by the carried-error condition |pre| >= 8 x 8 x u x S_pre and the earlier 1e-4 of |W| |h| + |b| (pinned on the host), so no
entry is skipped anywhere (the share skipped is 0).
    forward    ctx.sample on every case x dtype: eps bit for bit the mean-field stream, Z finite and per entry
    estimate   estimate_gradient, both estimators, diagonal target on every case, dense target on the two many-tile cases and on
               (64, (64, 64), 4, 16); float32 everywhere, float64 once per case with sticking the landing.  The many-tile cases assert
               n_mc > 1024 and 64 slices by flow_ref.flow_slices, and estimate_gradient_host, the last of estimate_gradient_n(IDX - 2, 3),
               estimate_gradient_each and the sequence A, B, A of two parameter vectors on one context are bitwise the single call.
               The dead units' incoming-weight entries are held per entry and are not all zero.
    descent    one Descent step of optimize_steps at (5, (8,), 2, 1040), the gradient recovered as (p - p') / eta, eta = 2^12
    inverse    ctx.logpdf bitwise equal to logpdf_host, per point against max(|yard - ref|, u S), yard the element-type evaluation through
               the inverse layers: (a) the context's own samples on every case, (b) the class far, z = 30 x normal draws, n = 1, 15, 17,
               33, 1040 on two shapes, (c) logpdf_constrained through Stacked([exp on three coordinates, identity]); finite wherever the
               reference is
Each case prints `[flow yardstick] route class case kind: whole, row, entry, value`.

Worst ratios measured on the MI355X per route and class (whole, row, entry, value; forward and inverse have one number), with the case
that gave each:
    route                      cases  whole   row   entry  value   (worst cases)
    forward f32                  12     -      -    3.93     -     ((64, (64, 64), 4, 16); damped 1.76, dead 1.77, sat4 1.53, sat16 1.70)
    forward f64                  12     -      -    3.88     -     ((64, (64, 64), 4, 16); damped 1.80)
    estimate f32 default         18    0.90   2.52  4.26   0.45    ((64, (64, 64), 4, 16) diag MC, three times; value (5, (8,), 2, 1040) dense MC)
    estimate f32 damped           6    0.68   2.66  5.46   0.14    ((128, (64, 64, 64), 32, 1) diag MC)
    estimate f32 sat4             2    0.42   1.72  2.07   0.14    (MC)          against sech^2(pre): 0.60 1.96 2.68 0.14
    estimate f32 sat16            2    0.36   1.04  1.65   0.12    (MC)          against sech^2(pre): 0.50 1.60 5.18 0.12 (STL: 1.13 -> 5.18)
    estimate f32 dead             2    0.54   1.27  1.89   0.03    (the dead units' rows alone, per entry: 1.45; f64 0.85)
    estimate f64 (all classes)   12    0.88   2.80  4.40   2.25    ((64, (64, 64), 4, 16); (128, (64, 64, 64), 32, 1), twice; (6, (4,), 1, 2049))
    descent                       1    0.36   0.60  0.90   0.16    ((5, (8,), 2, 1040) diag STL)
    inverse f32 own/far/stacked  23     -      -     -     1.50 / 3.19 / 1.05   (far: (17, (33, 20, 7), 3, .) n = 1040)
    inverse f64 own/far/stacked  23     -      -     -     3.32 / 2.81 / 2.22   (own: (5, (8,), 2, 1040))
No ratio exceeds the factor (worst 5.46: one entry of 1.06 M where M = 1 leaves a single evaluation in the envelope; the host emulation
scores 5.29 there) and csrc/kernels_flow.hip did not have to change: the accumulate branch, the zero columns of a later partial tile,
flow_layer_off at l = 32 and 1 - s^2 at saturation all hold.  Saturation: the rows "against sech^2(pre)" are the same device entries
held to a criterion whose reference, envelope and S take sech^2 from the pre-activation, i.e. with the documented formula's own
amplification 2 / (1 - s^2) taken out: 1 - s^2 from the rounded s costs up to a factor 4.6 on an entry at x 16 and stays inside the factor.
The whole file (113 cases) takes 6 seconds; the slowest case 0.33 s.
Host figures (tests/test_flow_ref_host.py): the float32 evaluation under 16 sample orders outside the envelope -- whole 0.80, row 1.49,
entry 2.31, value 0.45; the emulation of the kernels' order (K = 4 groups, float64 tile partials, slices in order) -- whole 0.59, row
1.97, entry 5.29 (M = 1 at 1.06 M entries: one evaluation in the envelope), value 0.45, Z 2.76, log q 1.20; the faults (worst ratio,
Monte-Carlo / sticking the landing): tile_overwrites 9.1e5 / 9.7e5, kink_slope_1 4.7e8 / 5.8e8, one_entry 3.2e2 / 4.3e2 (not seen by
block_report), one_row 5.3e2 / 4.7e2 (not seen by block_report), layer_off 1.7e9 / 1.7e9, sech_from_f32_s_twice 2.3e5 / 3.2e5."""
import zlib

import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from oracle import oracle as O
from tests import flow_ref as R
from tests.helpers import SEED, make_problem
from tests.measure_space_cases import F32_FACTOR

pytestmark = pytest.mark.gpu

IDX = R.CASE_IDX
YARD = list(R.YARD_CASES)
ENTS = {R.MONTE_CARLO: avi.MonteCarloEntropy(), R.STL: avi.StickingTheLandingEntropy()}
MID = (5, (16, 7), 2, 33, "default")
WIDE64 = (64, (64, 64), 4, 16, "default")
dt_id = lambda t: "f32" if t == np.float32 else "f64"   # noqa: E731
_crit, _fwd = {}, {}


def yid(c):
    return f"{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}-{c[3]}-{c[4]}"


def make_ctx(case, ent, dtype, prob=None, n_mc=None):
    d, hidden, L, M = case[:4]
    ctx = avi.MiviContext(dtype, avi.REALNVP, d, n_mc or M, ent, SEED, flow=(hidden, L))
    if prob is not None:
        ctx.set_problem(prob)
    return ctx


def make_target(case, kind, dtype):
    d, M = case[0], case[3]
    return make_problem(np.random.default_rng(4321 + d + 7 * M), kind, d, dtype)


def criterion(case, target, ent, dtype, params, tgt, eps, sech=False):
    """flow_ref.criterion of one setup, computed once and left unchanged; a second route must have drawn the same numbers"""
    key = (case, target, ent, np.dtype(dtype).name, sech, zlib.crc32(params.tobytes()))
    if key not in _crit:
        _crit[key] = (zlib.crc32(eps.tobytes()), R.criterion(params, case[:3], tgt, eps, ent, dtype, sech))
    assert _crit[key][0] == zlib.crc32(eps.tobytes()), "the draws of this estimate differ between two routes"
    return _crit[key][1]


def hold(route, case, target, ent, dtype, params, tgt, eps, value, grad, extra=None, Z=None):
    """print the case's line and assert every ratio, finite results and the per-block criterion of tests/test_gpu_flow.py"""
    arch = case[:3]
    cr = criterion(case, target, ent, dtype, params, tgt, eps)
    got = dict(grad=np.asarray(grad), value=float(value))
    if Z is not None:
        got["Z"] = Z
    r = R.all_ratios(got, cr, arch, dtype, extra)
    print(f"[flow yardstick] {route}-{dt_id(dtype)} {case[4]} {yid(case)}/{target} ent{ent}: {r['whole']:.2f}, {r['row']:.2f}, {r['entry']:.2f}, {r['value']:.2f}")
    assert np.all(np.isfinite(got["grad"])) and np.isfinite(got["value"])
    assert max(r.values()) <= F32_FACTOR, (route, case, target, ent, r)
    if extra is None:
        rows = R.block_report(got["grad"], cr["ref"]["grad"], cr["yard"]["grad"], arch, dtype)
        assert not R.violations(rows), R.violations(rows)
    return cr, r


# ---- forward ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=dt_id)
@pytest.mark.parametrize("case", YARD, ids=yid)
def test_forward(case, dtype):
    d, hidden, L, M, cls = case
    arch, u = case[:3], R.unit(dtype)
    params = R.yard_params(case, dtype)
    ctx = make_ctx(case, R.MONTE_CARLO, dtype)
    assert ctx.params_len == params.shape[0] == R.flow_layout(d, hidden, L)[1]
    Z, eps = ctx.sample(params, IDX)
    mf = avi.MiviContext(dtype, avi.MEANFIELD, d, M, R.MONTE_CARLO, SEED)   # the draws ARE the mean-field family's stream: bit for bit
    assert torch.equal(eps, mf.sample(np.concatenate([np.zeros(d, dtype), np.ones(d, dtype)]), IDX)[1])
    mf.close()
    Z, eps = Z.cpu().numpy().copy(), eps.cpu().numpy().copy()
    ctx.close()
    want = O.philox_normal(SEED, IDX, d, 0, M, f64=dtype == np.float64)   # ... and the oracle's restatement of it (tests/test_gpu_flow.py)
    assert np.linalg.norm(eps - want) < R.STOL[np.dtype(dtype)] * np.linalg.norm(want)
    zeros, wide = np.zeros(eps.shape), R.wider(dtype)
    ref = R.evaluate(params, arch, zeros, zeros[0], eps, R.MONTE_CARLO, wide)["Z"]
    yard = R.evaluate(params, arch, zeros, zeros[0], eps, R.MONTE_CARLO, dtype)["Z"]
    S = R.magnitude(params, arch, None, eps, None)["Z"]
    r = R.entry_ratio(Z, ref, S, u, env=np.abs(yard.astype(wide) - ref))
    print(f"[flow yardstick] forward-{dt_id(dtype)} {cls} {yid(case)} max|Z| {np.max(np.abs(Z)):.3g}: 0.00, 0.00, {r:.2f}, 0.00")
    assert np.all(np.isfinite(Z)) and r <= F32_FACTOR, (case, r)


# ---- estimate ----------------------------------------------------------------------------------------------------------------------------
def run_estimate(case, target, ent, dtype):
    d, hidden, L, M, cls = case
    arch = case[:3]
    params = R.yard_params(case, dtype)
    prob, tgt = make_target(case, target, dtype)
    ctx = make_ctx(case, ent, dtype, prob)
    p = ctx.to_device(params)
    Z, eps = ctx.sample(p, IDX)
    Z, eps = Z.cpu().numpy().copy(), eps.cpu().numpy().copy()
    v, g = ctx.estimate_gradient(p, IDX)
    ctx.synchronize()
    v1, g1 = v.clone(), g.clone()
    cr, r = hold("estimate", case, target, ent, dtype, params, tgt, eps, float(v1.item()), g1.cpu().numpy(), Z=Z)
    if cls in ("sat4", "sat16") and dtype == np.float32:   # the same entries with 1 - s^2 taken as sech^2(pre) in the reference: the formula's own amplification removed
        alt = criterion(case, target, ent, dtype, params, tgt, eps, sech=True)
        ra = R.all_ratios(dict(grad=g1.cpu().numpy(), value=float(v1.item())), alt, arch, dtype)
        print(f"[flow yardstick] estimate-f32 {cls} {yid(case)}/{target} ent{ent} against sech^2(pre): {ra['whole']:.2f}, {ra['row']:.2f}, {ra['entry']:.2f}, {ra['value']:.2f}")
    if cls == "dead":
        rows, gh = R.dead_rows(case), g1.cpu().numpy()
        rd = R.entry_ratio(gh[rows], cr["ref"]["grad"][rows], cr["S"]["grad"][rows], R.unit(dtype), env=cr["env"]["grad"][rows])
        print(f"[flow yardstick] estimate-{dt_id(dtype)} dead rows ent{ent}: 0.00, 0.00, {rd:.2f}, 0.00")
        assert rd <= F32_FACTOR and np.any(gh[rows] != 0) and np.all(np.asarray(cr["ref"]["grad"][rows], dtype=np.float64) != 0)
    if case in R.MANY_TILES:   # several tiles per slice DID run; every other route and a warm context give the same bits
        assert M > 1024 and ctx.n_mc == M and R.flow_slices(M, ctx.params_len) == 64 == min((M + 15) // 16, 64)
        vh, gh = ctx.estimate_gradient_host(params, IDX)
        assert vh == v1.item() and np.array_equal(gh, g1.cpu().numpy())
        vl, gl = ctx.empty(1), ctx.empty(ctx.params_len)
        ctx.estimate_gradient_n(p, IDX - 2, 3, vl, gl)
        vals, grads = ctx.estimate_gradient_each(p, IDX - 2, 3)
        ctx.synchronize()
        assert torch.equal(vl, v1) and torch.equal(gl, g1) and torch.equal(vals[2:3], v1) and torch.equal(grads[2], g1)
        pb = ctx.to_device(R.yard_params(case, dtype, R.YARD_CASES[case] + 1))   # A, then B, then A again on the warm context
        vb, gb = (t.clone() for t in ctx.estimate_gradient(pb, IDX))
        va, ga = (t.clone() for t in ctx.estimate_gradient(p, IDX))
        ctx.synchronize()
        assert not torch.equal(gb, g1) and torch.equal(va, v1) and torch.equal(ga, g1)
        fresh = make_ctx(case, ent, dtype, prob)   # ... and B on a context that never saw A
        vf, gf = fresh.estimate_gradient(pb, IDX)
        fresh.synchronize()
        assert torch.equal(vf, vb) and torch.equal(gf, gb)
        fresh.close()
    ctx.close()


ESTIMATE = [(c, "diag", e, np.float32) for c in YARD for e in ENTS] + [(c, "dense", e, np.float32) for c in R.MANY_TILES + [WIDE64] for e in ENTS]
ESTIMATE += [(c, "diag", R.STL, np.float64) for c in YARD]


@pytest.mark.parametrize("case,target,ent,dtype", ESTIMATE, ids=[f"{yid(c)}-{t}-ent{e}-{dt_id(dt)}" for c, t, e, dt in ESTIMATE])
def test_estimate(case, target, ent, dtype):
    run_estimate(case, target, ent, dtype)


# ---- one Descent step of the device loop -------------------------------------------------------------------------------------------------
def test_one_descent_step_runs_the_many_tile_vjp():
    case, target, ent, dtype, eta = (5, (8,), 2, 1040, "default"), "diag", R.STL, np.float32, 2.0 ** 12
    params = R.yard_params(case, dtype)
    prob, tgt = make_target(case, target, dtype)
    ctx = make_ctx(case, ent, dtype, prob)
    p = ctx.to_device(params).clone()
    eps = ctx.sample(p, IDX)[1].cpu().numpy().copy()
    elbo = ctx.empty(1)
    ctx.optimize_steps(p, None, IDX, 0, 1, 0, eta, 0.0, elbo)   # (rule 0: Descent; clip_epsilon <= 0: no operator)
    ctx.synchronize()
    after = p.cpu().numpy().astype(np.float64)
    value = -float(elbo.item())
    ctx.close()
    g = (params.astype(np.float64) - after) / eta
    hold("descent", case, target, ent, dtype, params, tgt, eps, value, g, extra=R.U32 * np.abs(after) / eta)


# ---- inverse -----------------------------------------------------------------------------------------------------------------------------
def hold_logpdf(what, case, dtype, params, points, got, got_h, ladj_rows=0):
    """got against inverse_np in the wider type at the stored points, per point; ladj_rows: the points are x = exp(eta) on the first rows"""
    arch, u, wide = case[:3], R.unit(dtype), R.wider(dtype)
    assert np.array_equal(got, got_h, equal_nan=True), what

    def logq(t):
        P = np.asarray(points).astype(t)
        if not ladj_rows:
            return R.inverse_np(params, arch, P, t)
        eta = P.copy()
        eta[:ladj_rows] = np.log(P[:ladj_rows])
        return R.inverse_np(params, arch, eta, t) - eta[:ladj_rows].sum(axis=0)

    ref, yard = logq(wide), logq(dtype)
    P64 = np.asarray(points, dtype=np.float64)
    if ladj_rows:
        eta, E = P64.copy(), np.zeros_like(P64)
        eta[:ladj_rows] = np.log(P64[:ladj_rows])
        E[:ladj_rows] = np.abs(eta[:ladj_rows])
        S = R.magnitude(params, arch, None, None, None, Zin=eta, EZin=E)["logq"] + np.abs(eta[:ladj_rows]).sum(axis=0)
    else:
        S = R.magnitude(params, arch, None, None, None, Zin=P64)["logq"]
    fin = np.isfinite(np.asarray(ref, dtype=np.float64))
    assert fin.all() and np.all(np.isfinite(got[fin])), what   # no point is skipped (share 0)
    r = R.entry_ratio(got, ref, S, u, env=np.abs(yard.astype(wide) - ref))
    print(f"[flow yardstick] inverse-{dt_id(dtype)} {what} {yid(case)} n {got.size}: 0.00, 0.00, 0.00, {r:.2f}")
    assert r <= F32_FACTOR, (what, case, r)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=dt_id)
@pytest.mark.parametrize("case", YARD, ids=yid)
def test_inverse_at_own_samples(case, dtype):
    params = R.yard_params(case, dtype)
    ctx = make_ctx(case, R.MONTE_CARLO, dtype)
    p = ctx.to_device(params)
    Z = ctx.sample(p, IDX)[0]
    got, got_h = ctx.logpdf(p, Z).cpu().numpy().copy(), ctx.logpdf_host(params, Z.cpu().numpy())
    Zh = Z.cpu().numpy().copy()
    ctx.close()
    hold_logpdf("own", case, dtype, params, Zh, got, got_h)


FAR = [(c, n) for c in (MID, (17, (33, 20, 7), 3, 16, "default")) for n in (1, 15, 17, 33, 1040)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=dt_id)
@pytest.mark.parametrize("case,n", FAR, ids=[f"{yid(c)}-n{n}" for c, n in FAR])
def test_inverse_far_from_the_flows_mass(case, n, dtype):
    """class far: default parameters, z = 30 x normal draws -- (z - t) e^-s does not land back on an O(1) eps"""
    d = case[0]
    params = R.yard_params(case, dtype)
    Zin = (30.0 * np.random.default_rng(77 + d + n).normal(size=(d, n))).astype(dtype)
    ctx = make_ctx(case, R.MONTE_CARLO, dtype)
    got, got_h = ctx.logpdf(params, Zin).cpu().numpy().copy(), ctx.logpdf_host(params, Zin)
    ctx.close()
    assert got.shape == (n,)
    hold_logpdf("far", case, dtype, params, Zin, got, got_h)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=dt_id)
def test_inverse_through_a_stacked_bijector(dtype):
    case = MID
    d = case[0]
    params = R.yard_params(case, dtype)
    ctx = make_ctx(case, R.MONTE_CARLO, dtype)
    ctx.set_bijector(avi.StackedBijector([(0, 3, "exp"), (3, d, "identity")]))
    X, eta = ctx.sample_constrained(params, IDX, want_eta=True)
    assert torch.equal(X[3:], eta[3:]) and bool((X[:3] > 0).all())
    got = ctx.logpdf_constrained(params, X).cpu().numpy().copy()
    got_h = ctx.logpdf_constrained_host(params, X.cpu().numpy())
    Xh = X.cpu().numpy().copy()
    ctx.close()
    hold_logpdf("stacked", case, dtype, params, Xh, got, got_h, ladj_rows=3)
