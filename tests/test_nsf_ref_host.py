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
@pytest.mark.parametrize("fault", [f for f in N.FAULTS if f != "inverse_bin_on_X"])
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
    assert [N.chunk_coords(K) for K in (2, 4, 8, 16)] == [12, 5, 2, 1]
