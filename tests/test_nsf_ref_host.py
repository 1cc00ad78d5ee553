"""CPU tests of tests/nsf_ref.py, the reference of the neural spline flow family (MIVI_NSF): the hand-written numpy backward formulas
against torch autograd, the inverse against the forward pass, the margins of the GPU cases, the float32 evaluation against its own
criterion under other sample orders, and the criterion against injected faults."""
import math

import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from tests import flow_ref as R
from tests import nsf_ref as N
from tests.helpers import make_problem

KINDS = [N.MONTE_CARLO, N.STL]


def _cid(case):
    return f"{case[0]}-{'x'.join(map(str, case[1]))}-{case[2]}-K{case[3]}-B{case[4]}-{case[5]}"


def _inputs(case, seed=7, spread=1.0):
    d, M = case[0], case[5]
    rng = np.random.default_rng(seed)
    _, tgt = make_problem(rng, "dense", d)
    return N.case_params(case, np.float64, seed), spread * rng.normal(size=(d, M)), tgt


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [(2, (8,), 2, 2, 3.0, 4), (5, (8,), 3, 4, 3.0, 17), (6, (16, 16), 2, 16, 3.0, 9), (7, (9, 5, 6), 4, 5, 1.0, 40),
                                  (4, (8,), 2, 4, 0.5, 64)], ids=_cid)
def test_numpy_evaluation_equals_autograd(case, kind):
    arch = N.arch_of(case)
    params, eps, tgt = _inputs(case)
    ag = N.estimate_gradient(params, arch, tgt, eps, kind)
    ell, G = N.target_columns(tgt, ag["Z"])
    ev = N.evaluate(params, arch, G, ell, eps, kind)
    assert np.abs(ev["Z"] - ag["Z"]).max() <= 1e-13 * max(1.0, np.abs(ag["Z"]).max())
    assert np.abs(ev["logq"] - ag["logq"]).max() <= 1e-12 * np.abs(ag["logq"]).max()
    assert abs(ev["value"] - ag["value"]) <= 1e-12 * abs(ag["value"])
    assert np.linalg.norm(ev["grad"] - ag["grad"]) <= 1e-11 * np.linalg.norm(ag["grad"])
    assert np.linalg.norm(ag["grad"]) > 0 and all(np.linalg.norm(ag["grad"][sl]) > 0 for _, sl in N.blocks(arch))


@pytest.mark.parametrize("case", [(5, (8,), 3, 4, 3.0, 17), (6, (16, 16), 2, 16, 3.0, 9), (4, (8,), 2, 4, 0.5, 64)], ids=_cid)
def test_inverse_of_forward_and_logpdf_of_forward(case):
    arch = N.arch_of(case)
    params, eps, _ = _inputs(case, spread=1.5)
    assert (np.abs(eps) > case[4]).any() and (np.abs(eps) < case[4]).any()   # both the bins and the identity tails
    with torch.no_grad():
        p, e = torch.tensor(params), torch.tensor(eps)
        Z, lq = N.forward(p, arch, e)
        back, _ = N.inverse(p, arch, Z)
        assert float((back - e).abs().max()) <= 1e-12 and float((N.logpdf(p, arch, Z) - lq).abs().max()) <= 1e-12 * float(lq.abs().max())
    zeros = np.zeros_like(eps)
    ev = N.evaluate(params, arch, zeros, zeros[0], eps, N.MONTE_CARLO)
    e_np, lq_np = N.inverse_np(params, arch, ev["Z"])
    assert np.abs(e_np - eps).max() <= 1e-12 and np.abs(lq_np - ev["logq"]).max() <= 1e-12 * np.abs(ev["logq"]).max()
    assert np.abs(ev["Z"] - Z.numpy()).max() <= 1e-13 * np.abs(ev["Z"]).max()


def test_zero_parameters_are_the_standard_normal():
    """softmax(0) = 1 / K and softplus(0) = log 2 are NOT the identity spline; with the slope parameters at log(e - 1) they are."""
    case = (5, (8,), 3, 4, 3.0, 17)
    arch = N.arch_of(case)
    p = np.zeros(N.nsf_layout(5, (8,), 3, 4)[1])
    for l, j, k, off, shape in N.nsf_layout(5, (8,), 3, 4)[0]:
        if k == "b" and j == 2:
            b = p[off:off + shape[0]].reshape(-1, 11)
            b[:, 8:] = math.log(math.e - 1.0)
    eps = 1.5 * np.random.default_rng(0).normal(size=(5, 17))
    zeros = np.zeros_like(eps)
    ev = N.evaluate(p, arch, zeros, zeros[0], eps, N.MONTE_CARLO)
    assert np.abs(ev["Z"] - eps).max() <= 1e-14
    assert np.abs(ev["logq"] - (-0.5 * (eps * eps).sum(axis=0) - 2.5 * math.log(2 * math.pi))).max() <= 1e-13


@pytest.mark.parametrize("case", list(N.CASES), ids=_cid)
def test_cases_keep_their_margins(case):
    """Every spline input off its knots and off +-B, every leakyrelu off its kink, on the draws the GPU tests use: no GPU test skips."""
    for dtype in (np.float32, np.float64):
        knot, kink = N.margin(N.case_params(case, dtype), N.arch_of(case), N.case_draws(case, dtype))
        print(f"[nsf] {_cid(case)} {np.dtype(dtype).name}: knot margin {knot:.3e}, kink margin {kink:.3e}")
        assert knot >= N.KNOT_MARGIN[np.dtype(dtype)] and kink >= N.KINK_MARGIN[np.dtype(dtype)]
    if case[4] == 0.5:
        assert np.mean(np.abs(N.case_draws(case, np.float64)) >= 0.5) > 0.5   # most inputs in the identity tails


@pytest.mark.parametrize("case", list(N.CASES), ids=_cid)
def test_no_spline_input_changes_its_bin_between_the_precisions(case):
    """The margins are stated on the float64 pass; here the pass in the context's dtype is laid beside the wider one, layer by layer: no
    spline input lies in another bin, and the two passes' inputs are closer to one another than the nearest knot is -- also 32 layers
    deep, where the kink margin of flow_ref is not stated to hold."""
    for dtype in (np.float32, np.float64):
        params, eps = N.case_params(case, dtype), N.case_draws(case, dtype)
        changed, far = N.bin_changes(params, N.arch_of(case), eps, dtype)
        knot, _ = N.margin(params, N.arch_of(case), eps)
        print(f"[nsf] {_cid(case)} {np.dtype(dtype).name}: {changed} changed bins, passes {far:.3e} of a bin apart, knot margin {knot:.3e}")
        assert changed == 0 and far < knot


def _criterion_inputs(case, kind):
    arch = N.arch_of(case)
    params = N.case_params(case, np.float32)
    eps = N.case_draws(case, np.float32)
    _, tgt = make_problem(np.random.default_rng(5), "diag", case[0], np.float32)
    zeros = np.zeros(eps.shape)
    ell, G = N.target_columns(tgt, N.evaluate(params, arch, zeros, zeros[0], eps, N.MONTE_CARLO)["Z"])
    ref = N.evaluate(params, arch, G, ell, eps, kind, np.float64)
    yard = N.evaluate(params, arch, G, ell, eps, kind, np.float32)
    return arch, params, eps, G, ell, ref, yard


_CRIT = {}


def _crit(case, kind):
    if (case, kind) not in _CRIT:
        _CRIT[(case, kind)] = _criterion_inputs(case, kind)
    return _CRIT[(case, kind)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", list(N.CASES), ids=_cid)
def test_float32_evaluation_under_other_sample_orders_stays_under_half_the_factor(case, kind):
    arch, params, eps, G, ell, ref, yard = _crit(case, kind)
    worst = {}
    for o in R.orders(case[5], len(params)):
        got = N.evaluate(params, arch, G, ell, eps, kind, np.float32, order=o)
        rows = N.report(got, ref, yard, arch, np.float32, factor=N.FACTOR // 2)
        assert not N.violations(rows), N.violations(rows)
        for k, v in N.worst_ratios(rows).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"[nsf] {_cid(case)} kind {kind}: worst ratio against HALF the factor over the orders {worst}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fault", [f for f in N.BLOCK_FAULTS if f != "inverse_bin_on_X"])
def test_criterion_sees_injected_faults(fault, kind):
    # the tails need inputs in them; a lost chunk needs several chunks per layer (K = 16: one coordinate per chunk, the last of three
    # is lost); a lost tile needs a second tile; the others strike at the partial-second-tile case
    case = {"tails_not_identity": (4, (8,), 2, 4, 0.5, 64), "lost_chunk": (6, (16, 16), 2, 16, 3.0, 33)}.get(fault, N.MID)
    if fault == "lost_chunk":
        assert all(len(N.masks(case[0], l)[0]) > N.chunk_coords(case[3]) for l in (1, 2))
    arch, params, eps, G, ell, ref, yard = _crit(case, kind)
    bad = N.evaluate(params, arch, G, ell, eps, kind, np.float32, fault=fault)
    rows = N.report(bad, ref, yard, arch, np.float32)
    assert N.violations(rows), (fault, rows)
    clean = N.report(N.evaluate(params, arch, G, ell, eps, kind, np.float32, order=R.orders(case[5])[2]), ref, yard, arch, np.float32)
    assert not N.violations(clean)


def test_criterion_sees_the_inverse_searching_its_bin_on_X():
    case = N.MID
    arch = N.arch_of(case)
    params = N.case_params(case, np.float32)
    Z = (np.random.default_rng(3).normal(size=(case[0], 40)) * 1.5).astype(np.float32)
    _, ref = N.inverse_np(params, arch, Z, np.float64)
    _, yard = N.inverse_np(params, arch, Z, np.float32)
    _, bad = N.inverse_np(params, arch, Z, np.float32, fault="inverse_bin_on_X")
    assert N.violations(N.report(dict(logq=bad), dict(logq=ref), dict(logq=yard), arch, np.float32))
    assert not N.violations(N.report(dict(logq=yard), dict(logq=ref), dict(logq=yard), arch, np.float32))


@pytest.mark.parametrize("d,hidden,L,K", [(2, (8,), 2, 2), (5, (16, 7), 3, 4), (127, (64, 64, 64), 2, 16)])
def test_package_layout_and_constructor_match_the_written_out_layout(d, hidden, L, K):
    lay, n = N.nsf_layout(d, hidden, L, K)
    assert (list(avi.nsf_layout(d, hidden, L, K)[0]), avi.nsf_layout(d, hidden, L, K)[1]) == (lay, n)
    q = avi.NeuralSplineFlow(d, hidden, K, 3.0, L, eltype=np.float32, rng=3)
    assert q.params.shape == (n,) and q.params.dtype == np.float32 and len(q) == d and q.eltype == np.float32
    for l, j, k, off, shape in lay:
        blk = q.params[off:off + int(np.prod(shape))]
        if k == "b":
            assert not blk.any()
        else:
            assert np.abs(blk).max() <= math.sqrt(6.0 / sum(shape)) and blk.std() > 0
            assert np.array_equal(q.blocks()[(l, j, "W")], blk.reshape(shape, order="F"))
    flat, re_ = avi.destructure(q)
    assert np.array_equal(re_(flat).params, q.params) and re_(flat).n_bins == K and re_(flat).bound == 3.0


def test_chunks_of_the_output_layer():
    """coordinates per chunk and rows per full chunk for every K the header admits: whole coordinates in one [64][16] block"""
    assert [N.chunk_coords(K) for K in (2, 4, 8, 16)] == [12, 5, 2, 1]
    assert [N.chunk_coords(K) for K in range(2, 17)] == [12, 8, 5, 4, 3, 3, 2, 2, 2, 2, 1, 1, 1, 1, 1]
    rows = {K: N.chunk_coords(K) * (3 * K - 1) for K in range(2, 17)}
    assert rows == {2: 60, 3: 64, 4: 55, 5: 56, 6: 51, 7: 60, 8: 46, 9: 52, 10: 58, 11: 64, 12: 35, 13: 38, 14: 41, 15: 44, 16: 47}
    assert all(N.chunk_coords(K) >= 1 and r <= 64 and r + (3 * K - 1) > 64 for K, r in rows.items())   # no further coordinate would fit
    # the chunk walks of the yardstick's cases: (coordinates of a layer, K) -> coordinates per chunk
    walk = lambda nA, K: [min(N.chunk_coords(K), nA - i) for i in range(0, nA, N.chunk_coords(K))]   # noqa: E731
    assert walk(9, 3) == [8, 1] and walk(8, 7) == [3, 3, 2] and walk(3, 11) == [2, 1] and walk(2, 12) == [1, 1] and walk(3, 16) == [1, 1, 1]
    assert walk(64, 16) == [1] * 64 and len(N.masks(18, 1)[0]) == 9 and len(N.masks(16, 1)[0]) == 8 and len(N.masks(6, 1)[0]) == 3


# ---- the per-entry criterion (tests/test_gpu_nsf_yardstick.py) -------------------------------------------------------------------------
# The figures these tests print are quoted in the module docstring of tests/test_gpu_nsf_yardstick.py.
from oracle import oracle as O  # noqa: E402,F401
from tests.measure_space_cases import F32_FACTOR  # noqa: E402

YARD = list(N.YARD_CASES)
HOST_YARD = [c for c in YARD if c[6] != "open"]   # (the open case: its own tests below, one estimator, the reduced envelope)
_YC = {}


def yid(c):
    return f"{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}-K{c[3]}-B{c[4]}-{c[5]}-{c[6]}"


def _ycrit(case, kind, dtype=np.float32):
    """(params, eps, criterion) of a YARD_CASES entry on the draws of estimate CASE_IDX with the diagonal target; computed once"""
    key = (case, kind, np.dtype(dtype).name)
    if key not in _YC:
        p, eps = N.yard_params(case, dtype), N.yard_draws(case, dtype)
        _, tgt = make_problem(np.random.default_rng(5), "diag", case[0], dtype)
        _YC[key] = (p, eps, N.criterion(p, case[:5], tgt, eps, kind, dtype, (0, 1) if case[6] == "open" else None))
    return _YC[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case,seed", [((5, (8,), 3, 4, 3.0, 17, "dead"), None), ((5, (8,), 3, 4, 3.0, 17, "peaked"), None), ((18, (8,), 2, 3, 3.0, 17, "default"), None),
                                       ((16, (16,), 2, 7, 3.0, 33, "default"), None), ((4, (6, 5), 3, 5, 1.5, 7, "dead"), 0), ((4, (8,), 8, 4, 3.0, 5, "damped"), 4),
                                       ((6, (16,), 2, 11, 3.0, 9, "default"), 3), ((4, (8,), 2, 4, 2.0, 9, "flat"), 0)], ids=lambda v: yid(v) if isinstance(v, tuple) else "")
def test_new_evaluate_features_equal_autograd(case, seed, kind):
    """the classes' parameters (a dead unit: torch's leaky_relu has slope 0.01 at 0 too), the chunk walk with its accumulated input VJP,
    the kernels' order and the tile sums, all in float64 against torch autograd"""
    d, M, arch = case[0], case[5], case[:5]
    p = N.yard_params(case, np.float64, seed)
    rng = np.random.default_rng(11 + d)
    eps = rng.normal(size=(d, M))
    _, tgt = make_problem(rng, "dense", d)
    ref = N.estimate_gradient(p, arch, tgt, eps, kind)
    ell, G = N.target_columns(tgt, ref["Z"])
    scale = np.linalg.norm(ref["grad"])
    for kw in (dict(), dict(emulate=True), dict(tile_sums=True), dict(order=R.kernel_order(M, len(p)))):
        ev = N.evaluate(p, arch, G, ell, eps, kind, np.float64, **kw)
        assert np.linalg.norm(ev["Z"] - ref["Z"]) <= 1e-9 * np.linalg.norm(ref["Z"]), kw
        assert np.linalg.norm(ev["logq"] - ref["logq"]) <= 1e-9 * np.linalg.norm(ref["logq"]), kw
        assert abs(ev["value"] - ref["value"]) <= 1e-9 * abs(ref["value"]), kw
        assert np.linalg.norm(ev["grad"] - ref["grad"]) <= 1e-9 * scale, kw
    if case[6] == "dead":
        rows = N.dead_rows(case)
        assert rows.size and np.all(ref["grad"][rows] != 0.0)


def test_slices_of_the_capped_and_many_tile_cases():
    """flow_slices' third term, 2^25 / n_params, binds on the two capped cases; the many-tile cases give slice 0 a second and a third tile"""
    n = {c: N.nsf_layout(*c[:4])[1] for c in YARD}
    big, opn = N.SLICE_CAPPED
    assert n[big] > 6.5e6 and (1 << 25) // n[big] == 5 < 64 and R.flow_slices(1, n[big]) == 1 and R.flow_slices(1040, n[big]) == 5
    assert n[opn] == 1198080 and (1 << 25) // n[opn] == 28 and R.flow_slices(449, n[opn]) == 28 < (449 + 15) // 16 == 29 and 28 < 64
    assert list(R.kernel_order(449, n[opn])[:32]) == list(range(16)) + list(range(448, 449)) + list(range(16, 31))   # slice 0: the tiles 0 and 28
    for c in N.MANY_TILES:
        assert c[5] > 1024 and R.flow_slices(c[5], n[c]) == 64
    assert len(N.MANY_TILES) == 2 and list(R.kernel_order(1040)[:32]) == list(range(16)) + list(range(1024, 1040)) and 2049 - 128 * 16 == 1


@pytest.mark.parametrize("case", HOST_YARD, ids=yid)
def test_yard_cases_meet_the_knot_the_kink_and_the_bin_conditions(case):
    """On both dtypes' draws: every spline input off the knots of its own bin and off +-B by 8 x 8 x u x S of that difference (the carried
    error of the input and of the knot's running sum) and by the earlier KNOT_MARGIN of the bin's width; flow_ref's kink rule; every bin
    hit (nsf_ref.bins_hit, with the two cases whose draws cannot reach an edge bin).  The share skipped is 0."""
    K = case[3]
    for dtype in N.yard_dtypes(case):
        knot, kink, hits = N.rooms(case, dtype)
        print(f"[nsf criterion] {yid(case)} {np.dtype(dtype).name}: knot room {knot:.3g}, kink room {kink:.3g}, inputs per bin {hits[:K].tolist()}, in the tails {hits[K]}")
        assert knot >= 1.0 and kink >= 1.0 and N.bins_hit(case, hits)
        changed, _ = N.bin_changes(N.yard_params(case, dtype), case[:5], N.yard_draws(case, dtype), dtype)
        assert changed == 0
    if case[6] == "dead":
        p = N.yard_params(case, np.float32)
        nets = N._nets(p, case[:5], lambda v, o, i: v.reshape((o, i), order="F"))
        for l, j, u_ in N.dead_units(case):
            W, b = nets[l][j - 1]
            assert not W[u_].any() and b[u_] == 0 and nets[l][j][0][:, u_].all()
    if case[6] == "peaked":
        b = N.yard_params(case, np.float64)[[off for l, j, k, off, _ in N.nsf_layout(*case[:4])[0] if (l, j, k) == (1, 2, "b")][0]:][:3 * K - 1]
        assert b[K - 1] - b[0] == 8.0 and set(np.abs(b[2 * K:])) == {4.0}
    if K == 2 or (K == 16 and case[4] == 1.0):
        assert hits[0] >= 2 and hits[K - 1] >= 2 and (K == 2 or hits[K] >= 2)
    if case[4] == 2.7:
        assert float(np.float32(2.7)) != 2.7 and float(np.float32(5.4)) == 2 * float(np.float32(2.7))


def test_the_open_case_keeps_the_margin_of_the_bin_width():
    """the open case's conditions (nsf_ref.open_case_holds): the carried-error knot condition cannot hold on 172 k inputs"""
    met, knot, changed, kink = N.open_case_holds(N.OPEN_CASE)
    print(f"[nsf criterion] {yid(N.OPEN_CASE)} float32: knot margin {knot:.3g} of a bin width, {changed} changed bins, kink room {kink:.3g}")
    assert met and knot >= N.KNOT_MARGIN[np.dtype(np.float32)] and changed == 0 and kink >= 1.0


CROSS_CHECK = 4.0   # the multiple of u S the float32 evaluation's own error stays under where no error is carried in (measured: 3.11)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", HOST_YARD, ids=yid)
def test_magnitude_against_the_float32_evaluations_actual_error(case, kind):
    """S cross-checked where a layer's inputs carry no error: the one-layer flow on the case's first layer and its draws.  The float32
    evaluation's actual error per entry -- of Z, of log q, of the value, of every gradient entry (sums as documented: tile_sums) -- stays
    within CROSS_CHECK x u S; measured over the cases and both estimators: Z 2.67, log q 2.19, gradient 3.11 (the width rows of the
    3008-row output layer of d = 127).  Printed beside it, not asserted: the same multiples at the case's full depth, where the carried
    errors add in quadrature and an outlier among millions of entries passes u S (the criterion is max(env, u S), and env holds it)."""
    p, eps, cr = _ycrit(case, kind)
    arch, u = case[:5], N.unit(np.float32)
    one = arch[:2] + (1,) + arch[3:]
    p1 = p[:N.nsf_layout(case[0], case[1], 1, case[3])[1]]
    _, tgt = make_problem(np.random.default_rng(5), "diag", case[0], np.float32)
    zeros = np.zeros(eps.shape)
    ell, G = N.target_columns(tgt, N.evaluate(p1, one, zeros, zeros[0], eps, N.MONTE_CARLO, np.float64)["Z"])
    ref, y = (N.evaluate(p1, one, G, ell, eps, kind, t, tile_sums=t == np.float32) for t in (np.float64, np.float32))
    S = N.magnitude(p1, one, tgt, eps, kind)
    mult = {k: N.entry_ratio(y[k], ref[k], S[k], u) for k in ("Z", "logq", "grad")}
    mult["value"] = N.value_ratio(y["value"], 0.0, ref["value"], S["value"], u)
    full = N.evaluate(p, arch, cr["G"], cr["ell"], eps, kind, np.float32, tile_sums=True)
    deep = {k: N.entry_ratio(full[k], cr["ref"][k], cr["S"][k], u) for k in ("Z", "logq", "grad")}
    print(f"[nsf criterion] |f32 - f64| / (u S) {yid(case)} kind {kind}: one layer " + " ".join(f"{n} {v:.2f}" for n, v in mult.items())
          + " | full depth " + " ".join(f"{n} {v:.2f}" for n, v in deep.items()))
    assert max(mult.values()) < CROSS_CHECK < F32_FACTOR


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", HOST_YARD, ids=yid)
def test_float32_evaluation_stays_inside_its_own_criterion(case, kind):
    """The criterion is not tighter than rounding: the envelope's own orders give at most 1, 16 further orders stay below half the
    factor and the emulation of the kernels' order (groups of four, the chunk walk, float64 tile partials, slices in order) below it."""
    p, eps, cr = _ycrit(case, kind)
    arch, M = case[:5], case[5]
    for o in R.orders(M, len(p)):
        r = N.all_ratios(N.evaluate(p, arch, cr["G"], cr["ell"], eps, kind, np.float32, order=o, tile_sums=True), cr, arch, np.float32)
        assert max(r.values()) <= 1.0 + 1e-12, r
    worst = {}
    for k in range(16 if M > 1 else 0):
        y = N.evaluate(p, arch, cr["G"], cr["ell"], eps, kind, np.float32, order=np.random.default_rng(2000 + k).permutation(M), tile_sums=True)
        worst = {n: max(worst.get(n, 0.0), v) for n, v in N.all_ratios(y, cr, arch, np.float32).items()}
    emu = N.all_ratios(N.evaluate(p, arch, cr["G"], cr["ell"], eps, kind, np.float32, emulate=True), cr, arch, np.float32)
    print(f"[nsf criterion] {yid(case)} kind {kind}: further orders " + " ".join(f"{n} {v:.2f}" for n, v in worst.items())
          + " | kernel order " + " ".join(f"{n} {v:.2f}" for n, v in emu.items()))
    assert max(worst.values(), default=0.0) <= F32_FACTOR / 2 and max(emu.values()) <= F32_FACTOR
    rows = N.report(N.evaluate(p, arch, cr["G"], cr["ell"], eps, kind, np.float32, emulate=True), cr["ref"], cr["yard"], arch, np.float32)
    assert not N.violations(rows), N.violations(rows)


def test_the_open_case_under_the_kernels_order():
    """the slice cap binding with a second tile in slice 0: the emulation with 28 slices stays inside the criterion whose envelope is the
    identity and the kernels' order (sticking the landing; the Monte-Carlo estimator runs on the device)"""
    case, kind = N.OPEN_CASE, N.STL
    p, eps, cr = _ycrit(case, kind)
    arch = case[:5]
    emu = N.all_ratios(N.evaluate(p, arch, cr["G"], cr["ell"], eps, kind, np.float32, emulate=True), cr, arch, np.float32)
    bad = N.all_ratios(N.evaluate(p, arch, cr["G"], cr["ell"], eps, kind, np.float32, emulate=True, fault="slice_cap"), cr, arch, np.float32)
    print(f"[nsf criterion] {yid(case)} kind {kind}: kernel order " + " ".join(f"{n} {v:.2f}" for n, v in emu.items())
          + " | fault slice_cap " + " ".join(f"{n} {v:.3g}" for n, v in bad.items()))
    assert max(emu.values()) <= F32_FACTOR and max(bad["whole"], bad["row"], bad["entry"]) > F32_FACTOR


BIG = (128, (64, 64, 64), 32, 16, 3.0, 1, "damped")
WIDE = (127, (64,), 2, 16, 3.0, 2, "default")   # its W_out of layer 1 is 3008 x 64
FAULT_CASES = [("one_entry", WIDE), ("one_row", WIDE), ("one_entry", (16, (16,), 2, 7, 3.0, 33, "default")), ("one_row", (16, (16,), 2, 7, 3.0, 33, "default")),
               ("edge_slope", (2, (8,), 2, 2, 3.0, 33, "default")), ("edge_slope", (6, (16, 16), 2, 16, 1.0, 33, "default")),
               ("stale_chunk_rows", (16, (16,), 2, 7, 3.0, 33, "default")), ("stale_chunk_rows", (18, (8,), 2, 3, 3.0, 17, "default")),
               ("acc_reset", (16, (16,), 2, 7, 3.0, 33, "default")), ("acc_reset", (6, (16,), 2, 11, 3.0, 33, "default")),
               ("slice_cap", (6, (4,), 1, 8, 3.0, 2049, "default")), ("B_unrounded", (5, (8,), 3, 4, 2.7, 17, "default")),
               ("lost_chunk", (4, (8,), 2, 12, 3.0, 17, "default")), ("lost_tile", (5, (8,), 2, 4, 3.0, 1040, "default"))]
NOT_SEEN_BY_REPORT = ("one_entry", "one_row")
UNDER_THE_FACTOR = ("B_unrounded",)   # 2B in float64 moves w and h by one rounding: no criterion of rounding size can see it (figure printed)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fault,case", FAULT_CASES, ids=[f"{f}-{yid(c)}" for f, c in FAULT_CASES])
def test_per_entry_criterion_sees_injected_faults(fault, case, kind):
    """Each fault on the smallest case that can show it (one_entry and one_row at a 3008 x 64 output block and at a 160 x 16 one; at
    (128, (64, 64, 64), 32, 16, 3.0, 1) one sample leaves a single evaluation in the envelope and u S of a sticking-the-landing entry 32
    layers deep is 1.4e-4 of it: one_entry scores 16 / 7.15 there and is not listed).  Printed beside it: whether the per-block criterion of tests/test_gpu_nsf.py
    (`report`) sees it.  slice_cap strikes where the slice count is capped and a slice owns several tiles; the M = 1 case has one tile,
    so the many-tile case stands in for it here and the open case has its own test above."""
    p, eps, cr = _ycrit(case, kind)
    arch = case[:5]
    kw = dict(emulate=True) if fault in ("stale_chunk_rows", "acc_reset", "slice_cap") else {}
    got = N.evaluate(p, arch, cr["G"], cr["ell"], eps, kind, np.float32, fault=fault, **kw)
    r = N.all_ratios(got, cr, arch, np.float32)
    seen = bool(N.violations(N.report(got, cr["ref"], cr["yard"], arch, np.float32)))
    print(f"[nsf criterion] fault {fault} on {yid(case)} kind {kind}: " + " ".join(f"{n} {v:.3g}" for n, v in r.items()) + f" | report sees it: {seen}")
    if fault in UNDER_THE_FACTOR:
        assert max(r.values()) <= F32_FACTOR and not seen
        return
    assert max(r["whole"], r["row"], r["group"], r["entry"]) > F32_FACTOR, r
    assert seen == (fault not in NOT_SEEN_BY_REPORT), (fault, seen)   # what the per-block l2 criterion lets through (the reason for the new file)


@pytest.mark.parametrize("n", [1, 15, 17, 33, 1040])
@pytest.mark.parametrize("case", [(5, (8,), 3, 4, 3.0, 17, "default"), (6, (16, 16), 2, 16, 1.0, 33, "default")], ids=yid)
def test_points_of_the_inverse_tests_keep_the_knot_condition(case, n):
    """the 2.5 B x normal points of tests/test_gpu_nsf_yardstick.py (restated: the generator and its seed) keep every inverse spline input
    off the knots of Y by 8 x 8 x u x S, in both dtypes; and the float32 inverse stays inside max(|yard - ref|, u S) trivially (ratio 1)"""
    d, B = case[0], case[4]
    for dtype in (np.float32, np.float64):
        pts = (2.5 * B * np.random.default_rng(77 + d + n).normal(size=(d, n))).astype(dtype)
        m = N.magnitude(N.yard_params(case, dtype), case[:5], None, None, None, Zin=pts)
        room = m["knot"] / (N.KINK_FACTOR * N.unit(dtype))
        print(f"[nsf criterion] inverse points {yid(case)} n {n} {np.dtype(dtype).name}: knot room {room:.3g}")
        assert room >= 1.0 and np.all(np.isfinite(m["logq"]))
