"""The neural spline flow kernels -- k_nsf_forward (rand, and the inverse of logpdf), k_nsf_vjp and RealNVP's finish kernel
(csrc/kernels_nsf.hip) -- held PER ENTRY to a float32 yardstick, at the smallest shapes that reach each mechanism the gradient tests of
tests/test_gpu_nsf.py do not: both bins of K = 2 and all sixteen of K = 16 with both tails, every chunk geometry of the output layer
(8 coordinates in exactly 64 rows, 3 + 3 + 2 coordinates in 60-row chunks, 2 coordinates in exactly 64 rows, 35- and 47-row chunks, a
layer walked in three chunks whose last is partial), a bound that rounds in float32, several tiles per slice, depth 32, every limit at
once (d = 128, three hidden layers of 64, K = 16, L = 32: 6.6 M parameters and a capped slice count), odd d at the limit, the slice cap
binding with a second tile in slice 0, peaked softmaxes, a hidden unit at exactly 0, and inputs exactly on the knots.
tests/test_gpu_nsf.py bounds the l2 distance of the gradient as a whole and per parameter block; what that lets through is printed by
tests/test_nsf_ref_host.py (test_per_entry_criterion_sees_injected_faults).

Criterion (tests/nsf_ref.py, tests/flow_ref.py's on this family's layout): ref is `evaluate` in the next wider type on the device's own
draws, env per entry the largest distance from it of eight sample orders of `evaluate` in the element type (the kernels' own among
them), S the first-order magnitude of a running error analysis of the documented formulas with the error of x^{l-1} carried into layer
l and through the spline (knots as running sums, xi = (a - X0) / w dividing the carried errors by the bin's width), u = 2^-24 / 2^-53,
and every ratio |got - ref| / max(env, u S) -- per entry, per row of each W_j and per b_j in l2, per coordinate group of the output layer
(the 3K - 1 rows of one coordinate), the whole gradient in l2, the value, Z and log q per entry -- is at most F32_FACTOR = 8 of
tests/measure_space_cases.py.  The per-block criterion of tests/test_gpu_nsf.py (nsf_ref.report) is asserted beside it.  Every case's
inputs keep every spline input off its knots by |a - knot| >= 8 x 8 x u x S and the earlier 1e-5 / 1e-11 of the bin's width, and every
leakyrelu off its kink by flow_ref's rule (pinned on the host), so no entry is skipped anywhere (the share skipped is 0).  The `open`
case alone (172 k spline inputs: 17 of them are expected within 8 x 8 x u x S of a knot at any seed) keeps the 1e-5 of the bin's width
and, on the host, that no input lies in another bin in float32 than in float64 (nsf_ref.open_case_holds).
    forward    ctx.sample on every case x dtype: eps bit for bit the mean-field stream, Z finite and per entry
    estimate   estimate_gradient, both estimators, diagonal target on every case, dense target on the two many-tile cases; float32
               everywhere, float64 once per case with sticking the landing (not the `open` case).  The many-tile and the slice-cap
               cases assert that estimate_gradient_host, the last of estimate_gradient_n(IDX - 2, 3), estimate_gradient_each, A, B, A
               on a warm context and B on a fresh one are bitwise the single call.  The dead units' incoming entries and, in the
               edge cases (K = 2; K = 16 with B = 1), the b_out entries of the raw slopes are held per entry; the slope of a knot no
               sample is beside is exactly 0 on the device.
    descent    one Descent step of optimize_steps at (5, (8,), 2, 4, 3.0, 1040), the gradient recovered as (p - p') / eta, eta = 2^12
    inverse    ctx.logpdf bitwise equal to logpdf_host, per point against max(|yard - ref|, u S): (a) the context's own samples on
               every case, (b) 2.5 B x normal draws (inside and tails mixed), n = 1, 15, 17, 33, 1040 on two shapes, (c) through
               Stacked([exp on three coordinates, identity])
    knots      the class `flat` (every knot a dyadic number): points built from exact knot values -B + j 2B / K, +-B among them, and
               generic values beside them, through logpdf directly and as the forward image of such eps; log q per point and
               finiteness alone (log y' has a parameter gradient that jumps at a knot: no gradient is asserted there)
Each case prints `[nsf yardstick] route class case kind: whole, row, group, entry, value`.

Worst ratios measured on the MI355X per route and class (whole, row, group, entry, value; forward and inverse have one number), with the
case that gave each:
    route                      cases  whole   row   group  entry  value   (worst cases)
    forward f32                  15     -      -      -    2.37     -     ((128, (64,), 6, 16, 3.0, 449) open)
    forward f64                  14     -      -      -    1.74     -     ((6, (4,), 1, 8, 3.0, 2049))
    estimate f32 default         24    0.31   1.67   1.01  2.11   0.52    (whole K = 3; row K = 7; group, entry (127, (64,), 2, 16, 3.0, 2) MC; value 2049)
    estimate f32 damped           4    0.88   3.87   2.53  4.08   0.00    ((128, (64, 64, 64), 32, 16, 3.0, 1): whole MC, the others STL)
    estimate f32 peaked           2    0.21   0.45   0.28  0.58   0.01    (MC)
    estimate f32 dead             2    0.08   0.64   0.22  0.85   0.02    (the dead units' rows alone, per entry: 0.21; f64 0.06)
    estimate f32 open             2    0.34   2.39   1.12  2.90   0.11    (row MC, entry STL; Z 2.37)
    edge slopes f32 / f64       4 / 2    -      -      -   1.10 / 0.54  -   (K = 16, B = 1: 12 edge entries; 6 of its 90 knots have no sample beside them, those exactly 0)
    estimate f64 (all classes)   14    0.42   5.29   2.52  5.44   0.43    ((128, (64, 64, 64), 32, 16, 3.0, 1), row, group and entry; whole d = 127; value 2049)
    descent                       1    0.00   0.20   0.02  0.49   0.13    ((5, (8,), 2, 4, 3.0, 1040) diag STL)
    inverse f32 own/mixed/stacked/knots   15 / 10 / 1 / 4    -   1.89 / 1.63 / 0.33 / 0.38   (own: K = 16, B = 1; mixed: the same shape, n = 1040)
    inverse f64 own/mixed/stacked/knots   14 / 10 / 1 / 4    -   1.78 / 2.69 / 0.97 / 0.88   (mixed: (5, (8,), 3, 4, 3.0, .) n = 1040)
No ratio exceeds the factor (worst 5.44, float64: one entry of 6.6 M where M = 1 leaves a single evaluation in the envelope; float32
4.08 at the same shape) and csrc/kernels_nsf.hip did not have to change: the edge bins' d_0 = 1 / d_1 = 1 branches, every chunk geometry,
the accumulators of nsf_input_vjp across three chunks with a partial last one, the capped slice count with a second tile in slice 0,
(T)a.B and T(2) * B at B = 2.7, v >= knot at xi = 0 and the inverse's root at dy = 0 all hold.  The peaked class stays at 0.58: no
second line against a criterion without the formula's own amplification was needed (its ramp leaves the narrow bins at the end of
[-B, B], where no draw falls: nsf_ref.BINS_OUT_OF_REACH).
The whole file (133 cases) takes 26 seconds; the slowest case 4.1 s (the float64 estimate at every limit; the open case 3.7 s, nearly
all of it the host-side criterion: its envelope holds the identity and the kernels' order alone -- with all eight orders the criterion
took 12 s per estimator on the CPU).
Host figures (tests/test_nsf_ref_host.py, 184 tests in 47 s): |float32 evaluation - float64| / (u S) where no error is carried in (one
layer) at most Z 2.17, log q 2.14, gradient 3.11, and at full depth 2.17, 1.85, 3.16; the float32 evaluation under 16 sample orders outside
the envelope -- whole 0.27, row 1.00, group 1.00, entry 1.12, value 0.21; the emulation of the kernels' order (groups of four, the chunk
walk, float64 tile partials, slices in order) -- whole 0.39, row 2.42, group 1.63, entry 2.85 (the open case; 2.51 at every limit), value
0.21, Z 2.78, log q 1.19; the faults (worst ratio, Monte-Carlo / sticking the landing; `report`): one_entry 3008 x 64: 18.9 / 94.8, 160 x 16:
230 / 168, NOT seen; one_row 19.9 / 12.8 and 36.1 / 23.7, NOT seen; edge_slope 3.8e6 / 8.9e5 (K = 2), 2.6e6 / 7.0e5 (K = 16), seen;
stale_chunk_rows 2.2e5 / 1.7e5 and 1.7e6 / 1.1e6, seen; acc_reset 7.3e5 / 5.3e5 and 6.6e5 / 2.8e5, seen; slice_cap 5.8e6 / 2.6e6 (2049
samples) and 1.4e5 (the open case), seen; B_unrounded 0.68 / 0.30: UNDER the factor, as one rounding of w and h has to be -- the B = 2.7
case rests on logpdf being bitwise logpdf_host and on the per-entry rule alone."""
import zlib

import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from oracle import oracle as O
from tests import flow_ref as R
from tests import nsf_ref as N
from tests.helpers import SEED, make_problem
from tests.measure_space_cases import F32_FACTOR

pytestmark = pytest.mark.gpu

IDX = N.CASE_IDX
YARD = list(N.YARD_CASES)
ENTS = (N.MONTE_CARLO, N.STL)
MID = (5, (8,), 3, 4, 3.0, 17, "default")
EDGE = [(2, (8,), 2, 2, 3.0, 33, "default"), (6, (16, 16), 2, 16, 1.0, 33, "default")]
DESCENT = (5, (8,), 2, 4, 3.0, 1040, "default")
dt_id = lambda t: "f32" if t == np.float32 else "f64"   # noqa: E731
_crit = {}


def yid(c):
    return f"{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}-K{c[3]}-B{c[4]}-{c[5]}-{c[6]}"


def make_ctx(case, ent, dtype, prob=None, n_mc=None):
    d, hidden, L, K, B, M = case[:6]
    ctx = avi.MiviContext(dtype, avi.NSF, d, n_mc or M, ent, SEED, flow=(hidden, L, K, B))
    if prob is not None:
        ctx.set_problem(prob)
    return ctx


def make_target(case, kind, dtype):
    d, M = case[0], case[5]
    return make_problem(np.random.default_rng(4321 + d + 7 * M), kind, d, dtype)


def criterion(case, target, ent, dtype, params, tgt, eps):
    """nsf_ref.criterion of one setup, computed once and left unchanged; a second route must have drawn the same numbers.  The `open`
    case's envelope is the identity and the kernels' order alone (nsf_ref.envelope's `which`)."""
    key = (case, target, ent, np.dtype(dtype).name, zlib.crc32(params.tobytes()))
    if key not in _crit:
        which = (0, 1) if case[6] == "open" else None
        _crit[key] = (zlib.crc32(eps.tobytes()), N.criterion(params, case[:5], tgt, eps, ent, dtype, which))
    assert _crit[key][0] == zlib.crc32(eps.tobytes()), "the draws of this estimate differ between two routes"
    return _crit[key][1]


def hold(route, case, target, ent, dtype, params, tgt, eps, value, grad, extra=None, Z=None):
    """print the case's line and assert every ratio, finite results and the per-block criterion of tests/test_gpu_nsf.py"""
    arch = case[:5]
    cr = criterion(case, target, ent, dtype, params, tgt, eps)
    got = dict(grad=np.asarray(grad), value=float(value))
    if Z is not None:
        got["Z"] = Z
    r = N.all_ratios(got, cr, arch, dtype, extra)
    print(f"[nsf yardstick] {route}-{dt_id(dtype)} {case[6]} {yid(case)}/{target} ent{ent}: {r['whole']:.2f}, {r['row']:.2f}, {r['group']:.2f}, "
          f"{r['entry']:.2f}, {r['value']:.2f}" + (f" (Z {r['Z']:.2f})" if "Z" in r else ""))
    assert np.all(np.isfinite(got["grad"])) and np.isfinite(got["value"])
    assert max(r.values()) <= F32_FACTOR, (route, case, target, ent, r)
    if extra is None:
        rows = N.report(got, cr["ref"], cr["yard"], arch, dtype)
        assert not N.violations(rows), N.violations(rows)
    return cr, r


# ---- forward ---------------------------------------------------------------------------------------------------------------------------
FORWARD = [(c, t) for c in YARD for t in N.yard_dtypes(c)]


@pytest.mark.parametrize("case,dtype", FORWARD, ids=[f"{yid(c)}-{dt_id(t)}" for c, t in FORWARD])
def test_forward(case, dtype):
    d, hidden, L, K, B, M, cls = case
    arch, u = case[:5], N.unit(dtype)
    params = N.yard_params(case, dtype)
    ctx = make_ctx(case, N.MONTE_CARLO, dtype)
    assert ctx.params_len == params.shape[0] == N.nsf_layout(d, hidden, L, K)[1]
    Z, eps = ctx.sample(params, IDX)
    mf = avi.MiviContext(dtype, avi.MEANFIELD, d, M, N.MONTE_CARLO, SEED)   # the draws ARE the mean-field family's stream: bit for bit
    assert torch.equal(eps, mf.sample(np.concatenate([np.zeros(d, dtype), np.ones(d, dtype)]), IDX)[1])
    mf.close()
    Z, eps = Z.cpu().numpy().copy(), eps.cpu().numpy().copy()
    ctx.close()
    want = O.philox_normal(SEED, IDX, d, 0, M, f64=dtype == np.float64)
    assert np.linalg.norm(eps - want) <= N.STOL[np.dtype(dtype)] * np.linalg.norm(want)
    zeros, wide = np.zeros(eps.shape), N.wider(dtype)
    ref = N.evaluate(params, arch, zeros, zeros[0], eps, N.MONTE_CARLO, wide)["Z"]
    yard = N.evaluate(params, arch, zeros, zeros[0], eps, N.MONTE_CARLO, dtype)["Z"]
    S = N.magnitude(params, arch, None, eps, None)["Z"]
    r = N.entry_ratio(Z, ref, S, u, env=np.abs(yard.astype(wide) - ref))
    print(f"[nsf yardstick] forward-{dt_id(dtype)} {cls} {yid(case)} max|Z| {np.max(np.abs(Z)):.3g}: 0.00, 0.00, 0.00, {r:.2f}, 0.00")
    assert np.all(np.isfinite(Z)) and r <= F32_FACTOR, (case, r)


# ---- estimate ----------------------------------------------------------------------------------------------------------------------------
def run_estimate(case, target, ent, dtype):
    d, hidden, L, K, B, M, cls = case
    arch, P = case[:5], 3 * K - 1
    params = N.yard_params(case, dtype)
    prob, tgt = make_target(case, target, dtype)
    ctx = make_ctx(case, ent, dtype, prob)
    p = ctx.to_device(params)
    Z, eps = ctx.sample(p, IDX)
    Z, eps = Z.cpu().numpy().copy(), eps.cpu().numpy().copy()
    v, g = ctx.estimate_gradient(p, IDX)
    ctx.synchronize()
    v1, g1 = v.clone(), g.clone()
    gh = g1.cpu().numpy()
    cr, r = hold("estimate", case, target, ent, dtype, params, tgt, eps, float(v1.item()), gh, Z=Z)
    u, ref_g = N.unit(dtype), np.asarray(cr["ref"]["grad"], dtype=np.float64)
    if cls == "dead":
        rows = N.dead_rows(case)
        rd = N.entry_ratio(gh[rows], cr["ref"]["grad"][rows], cr["S"]["grad"][rows], u, env=cr["env"]["grad"][rows])
        print(f"[nsf yardstick] estimate-{dt_id(dtype)} dead rows ent{ent}: 0.00, 0.00, 0.00, {rd:.2f}, 0.00")
        assert rd <= F32_FACTOR and np.any(gh[rows] != 0) and np.all(ref_g[rows] != 0)
    if case in EDGE:   # the raw slopes' biases: beside a hit edge bin non-zero, of a knot no sample is beside exactly 0
        hits, ent_idx = N.slope_hits(params, arch, eps), N.edge_slope_entries(case)
        edge = np.array(sorted(set(ent_idx.values())), dtype=np.int64)
        re_ = N.entry_ratio(gh[edge], cr["ref"]["grad"][edge], cr["S"]["grad"][edge], u, env=cr["env"]["grad"][edge])
        n_zero = 0
        for (l, i, j), n in hits.items():
            e = ent_idx[(l, i, "lo")] + j - 1
            if n == 0:
                n_zero += 1
                assert gh[e] == 0.0 and ref_g[e] == 0.0, (l, i, j)
            elif j in (1, K - 1):
                assert ref_g[e] != 0.0 and gh[e] != 0.0, (l, i, j)
        print(f"[nsf yardstick] estimate-{dt_id(dtype)} edge slopes {yid(case)} ent{ent} ({edge.size} entries, {n_zero} knots without a sample): 0.00, 0.00, 0.00, {re_:.2f}, 0.00")
        assert re_ <= F32_FACTOR
    if case in N.MANY_TILES or case in N.SLICE_CAPPED:   # several tiles per slice / the capped slice count DID run; every route gives the same bits
        tiles, ns = (M + 15) // 16, R.flow_slices(M, ctx.params_len)
        assert ctx.n_mc == M and ctx.params_len == params.shape[0]
        if case in N.MANY_TILES:
            assert M > 1024 and ns == 64 < tiles
        elif M > 1:
            assert ns == (1 << 25) // ctx.params_len < tiles and ns < 64   # the third term binds: slice 0 owns a second tile
        else:
            assert (1 << 25) // ctx.params_len == 5 < 64   # (one sample: one tile; the cap sizes the partials buffer)
        vh, ghost = ctx.estimate_gradient_host(params, IDX)
        assert vh == v1.item() and np.array_equal(ghost, gh)
        vl, gl = ctx.empty(1), ctx.empty(ctx.params_len)
        ctx.estimate_gradient_n(p, IDX - 2, 3, vl, gl)
        vals, grads = ctx.estimate_gradient_each(p, IDX - 2, 3)
        ctx.synchronize()
        assert torch.equal(vl, v1) and torch.equal(gl, g1) and torch.equal(vals[2:3], v1) and torch.equal(grads[2], g1)
        pb = ctx.to_device(N.yard_params(case, dtype, N.YARD_CASES[case] + 1))   # A, then B, then A again on the warm context
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


ESTIMATE = [(c, "diag", e, np.float32) for c in YARD for e in ENTS] + [(c, "dense", e, np.float32) for c in N.MANY_TILES for e in ENTS]
ESTIMATE += [(c, "diag", N.STL, np.float64) for c in YARD if np.float64 in N.yard_dtypes(c)]


@pytest.mark.parametrize("case,target,ent,dtype", ESTIMATE, ids=[f"{yid(c)}-{t}-ent{e}-{dt_id(dt)}" for c, t, e, dt in ESTIMATE])
def test_estimate(case, target, ent, dtype):
    run_estimate(case, target, ent, dtype)


# ---- one Descent step of the device loop -------------------------------------------------------------------------------------------------
def test_one_descent_step_runs_the_many_tile_vjp():
    case, target, ent, dtype, eta = DESCENT, "diag", N.STL, np.float32, 2.0 ** 12
    params = N.yard_params(case, dtype)
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
def hold_logpdf(what, case, dtype, params, points, got, got_h, ladj_rows=0, knots_met=True):
    """got against inverse_np in the wider type at the stored points, per point; ladj_rows: the points are x = exp(eta) on the first rows.
    knots_met: the points keep the knot condition of the inverse (asserted); False on the class flat, whose points lie ON the knots."""
    arch, u, wide = case[:5], N.unit(dtype), N.wider(dtype)
    assert np.array_equal(got, got_h, equal_nan=True), what

    def logq(t):
        Pt = np.asarray(points).astype(t)
        if not ladj_rows:
            return N.inverse_np(params, arch, Pt, t)[1]
        eta = Pt.copy()
        eta[:ladj_rows] = np.log(Pt[:ladj_rows])
        return N.inverse_np(params, arch, eta, t)[1] - eta[:ladj_rows].sum(axis=0)

    ref, yard = logq(wide), logq(dtype)
    P64 = np.asarray(points, dtype=np.float64)
    if ladj_rows:
        eta, E = P64.copy(), np.zeros_like(P64)
        eta[:ladj_rows] = np.log(P64[:ladj_rows])
        E[:ladj_rows] = np.abs(eta[:ladj_rows])
        m = N.magnitude(params, arch, None, None, None, Zin=eta, EZin=E)
        S = m["logq"] + np.abs(eta[:ladj_rows]).sum(axis=0)
    else:
        m = N.magnitude(params, arch, None, None, None, Zin=P64)
        S = m["logq"]
    fin = np.isfinite(np.asarray(ref, dtype=np.float64))
    assert fin.all() and np.all(np.isfinite(got[fin])), what   # no point is skipped (share 0)
    if knots_met:
        assert m["knot"] >= N.KINK_FACTOR * u, (what, m["knot"] / (N.KINK_FACTOR * u))
    r = N.entry_ratio(got, ref, S, u, env=np.abs(yard.astype(wide) - ref))
    print(f"[nsf yardstick] inverse-{dt_id(dtype)} {what} {yid(case)} n {got.size}: 0.00, 0.00, 0.00, 0.00, {r:.2f}")
    assert r <= F32_FACTOR, (what, case, r)


@pytest.mark.parametrize("case,dtype", FORWARD, ids=[f"{yid(c)}-{dt_id(t)}" for c, t in FORWARD])
def test_inverse_at_own_samples(case, dtype):
    params = N.yard_params(case, dtype)
    ctx = make_ctx(case, N.MONTE_CARLO, dtype)
    p = ctx.to_device(params)
    Z = ctx.sample(p, IDX)[0]
    got, got_h = ctx.logpdf(p, Z).cpu().numpy().copy(), ctx.logpdf_host(params, Z.cpu().numpy())
    Zh = Z.cpu().numpy().copy()
    ctx.close()
    hold_logpdf("own", case, dtype, params, Zh, got, got_h, knots_met=False)   # (the forward inputs keep the condition; their images need not on Y)


MIXED = [(c, n) for c in (MID, (6, (16, 16), 2, 16, 1.0, 33, "default")) for n in (1, 15, 17, 33, 1040)]


def mixed_points(case, n, dtype):
    d, B = case[0], case[4]
    return (2.5 * B * np.random.default_rng(77 + d + n).normal(size=(d, n))).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=dt_id)
@pytest.mark.parametrize("case,n", MIXED, ids=[f"{yid(c)}-n{n}" for c, n in MIXED])
def test_inverse_at_points_inside_and_in_the_tails(case, n, dtype):
    """2.5 B x normal draws: coordinates inside (-B, B) and in the identity tails mixed within a point"""
    B = case[4]
    params = N.yard_params(case, dtype)
    Zin = mixed_points(case, n, dtype)
    assert n < 15 or ((np.abs(Zin) > B).any() and (np.abs(Zin) < B).any())
    ctx = make_ctx(case, N.MONTE_CARLO, dtype)
    got, got_h = ctx.logpdf(params, Zin).cpu().numpy().copy(), ctx.logpdf_host(params, Zin)
    ctx.close()
    assert got.shape == (n,)
    hold_logpdf("mixed", case, dtype, params, Zin, got, got_h)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=dt_id)
def test_inverse_through_a_stacked_bijector(dtype):
    case = MID
    d = case[0]
    params = N.yard_params(case, dtype)
    ctx = make_ctx(case, N.MONTE_CARLO, dtype)
    ctx.set_bijector(avi.StackedBijector([(0, 3, "exp"), (3, d, "identity")]))
    X, eta = ctx.sample_constrained(params, IDX, want_eta=True)
    assert torch.equal(X[3:], eta[3:]) and bool((X[:3] > 0).all())
    got = ctx.logpdf_constrained(params, X).cpu().numpy().copy()
    got_h = ctx.logpdf_constrained_host(params, X.cpu().numpy())
    Xh = X.cpu().numpy().copy()
    ctx.close()
    hold_logpdf("stacked", case, dtype, params, Xh, got, got_h, ladj_rows=3, knots_met=False)


# ---- on the knots ------------------------------------------------------------------------------------------------------------------------
def knot_points(case, dtype):
    """d x n: every column mixes exact knot values -B + j 2B / K (j = 0 .. K: +-B among them) with generic values beside them"""
    d, K, B = case[0], case[3], case[4]
    knots = -B + np.arange(K + 1) * (2 * B / K)
    gen = np.random.default_rng(5 + K)
    cols = []
    for j in range(K + 1):
        for shift in range(d):
            col = gen.uniform(-1.2 * B, 1.2 * B, size=d)
            col[shift] = knots[j]
            col[(shift + 1) % d] = knots[(j + 3) % (K + 1)]
            cols.append(col)
    cols.append(np.resize(knots, d))
    cols.append(np.resize(knots[::-1], d))
    out = np.stack(cols, axis=1).astype(dtype)
    assert np.array_equal(out[0, 0:1].astype(np.float64), knots[0:1]) and np.isin(out, knots.astype(dtype)).sum() >= 2 * (K + 1) * d
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=dt_id)
@pytest.mark.parametrize("case", N.FLAT_CASES, ids=yid)
def test_inputs_exactly_on_the_knots(case, dtype):
    """v >= knot with xi = 0, and the inverse's 2 qc / (-qb - sqrt(...)) with dy = 0: y and log y' are continuous across a knot, so the
    side the reference takes does not matter; log q per point and finiteness alone"""
    arch, K, B = case[:5], case[3], case[4]
    params = N.yard_params(case, dtype)
    assert not params[[e for _, j, _, off, shape in N.nsf_layout(*case[:4])[0] if j == len(case[1]) + 1 for e in range(off, off + int(np.prod(shape)))]].any()
    pts = knot_points(case, dtype)
    zeros = np.zeros(pts.shape)
    image = N.evaluate(params, arch, zeros, zeros[0], pts, N.MONTE_CARLO, np.float64)["Z"].astype(dtype)   # the forward image of eps on the knots
    knots = (-B + np.arange(K + 1) * (2 * B / K)).astype(dtype)
    assert np.isin(image, knots).sum() >= np.isin(pts, knots).sum() // 2   # a knot of X maps to the knot of Y: exactly, in every type
    ctx = make_ctx(case[:5] + (pts.shape[1],) + case[6:], N.MONTE_CARLO, dtype)
    for what, P_ in (("knots", pts), ("knots-image", image)):
        got, got_h = ctx.logpdf(params, P_).cpu().numpy().copy(), ctx.logpdf_host(params, P_)
        hold_logpdf(what, case, dtype, params, P_, got, got_h, knots_met=False)
    ctx.close()
