"""Host tests of tests/flow_ref.py, the restatement the GPU tests of the RealNVP family (tests/test_gpu_flow.py) are held against: the
numpy evaluation with its hand-written backward sweeps equals torch autograd on the literal definition, the cases' inputs keep every
leakyrelu away from its kink, and the per-block criterion admits the yardstick under other summation orders and sees injected faults.
Second half: the per-entry criterion of tests/test_gpu_flow_yardstick.py -- its parameter classes against autograd, the kink condition with
the carried error on every case, the float32 evaluation inside its own criterion, and the faults it sees where the per-block one does not."""
import math

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import flow_ref as R
from tests.helpers import SEED, make_problem


def _inputs(d, hidden, L, M, seed=7):
    arch = (d, tuple(hidden), L)
    rng = np.random.default_rng(seed + d + 10 * L)
    p = R.case_params((d, tuple(hidden), L, M), np.float64, seed)
    eps = rng.normal(size=(d, M))
    _, tgt = make_problem(rng, "dense", d)
    return arch, p, eps, tgt


@pytest.mark.parametrize("kind", [R.MONTE_CARLO, R.STL])
@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("d", [2, 3, 5, 17])
def test_numpy_evaluation_equals_autograd(d, L, kind):
    arch, p, eps, tgt = _inputs(d, (9, 6), L, 11)
    ref = R.estimate_gradient(p, arch, tgt, eps, kind)
    ell, G = R.target_columns(tgt, ref["Z"])
    ev = R.evaluate(p, arch, G, ell, eps, kind, np.float64)
    assert np.linalg.norm(ev["Z"] - ref["Z"]) <= 1e-9 * np.linalg.norm(ref["Z"])
    assert abs(ev["value"] - ref["value"]) <= 1e-9 * abs(ref["value"])
    assert np.linalg.norm(ev["grad"] - ref["grad"]) <= 1e-9 * np.linalg.norm(ref["grad"])
    assert np.linalg.norm(ref["grad"]) > 0


@pytest.mark.parametrize("d,hidden,L", [(2, (16, 16), 3), (5, (7,), 2), (17, (33, 20, 7), 3)])
def test_logpdf_of_forward_is_the_forwards_log_q(d, hidden, L):
    arch, p, eps, _ = _inputs(d, hidden, L, 9)
    pt, et = torch.tensor(p), torch.tensor(eps)
    z, lq = R.forward(pt, arch, et)
    back, _ = R.inverse(pt, arch, z)
    assert torch.allclose(back, et, rtol=0, atol=1e-12)
    assert torch.allclose(R.logpdf(pt, arch, z), lq, rtol=0, atol=1e-12)


def test_zero_parameters_are_the_standard_normal():
    arch, p, eps, _ = _inputs(5, (8, 4), 3, 6)
    z, lq = R.forward(torch.zeros_like(torch.tensor(p)), arch, torch.tensor(eps))
    assert torch.equal(z, torch.tensor(eps))
    want = -0.5 * (eps * eps).sum(axis=0) - 2.5 * math.log(2 * math.pi)
    assert np.allclose(lq.numpy(), want, rtol=0, atol=1e-14)


@pytest.mark.parametrize("case", list(R.CASES), ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}-{c[3]}")
def test_cases_keep_every_leakyrelu_off_its_kink(case):
    """A condition on the inputs, not a tolerance on the code: a float32 pre-activation differs from the float64 one by at most
    (fan-in + 2) 2^-24 <= 4e-6 of its scale per layer, so 1e-4 keeps a factor 8 over three layers and no leakyrelu branch can differ
    between the device and the reference (1e-12 for float64 likewise)."""
    d, hidden, L, M = case
    for dtype, need in ((np.float32, 1e-4), (np.float64, 1e-12)):
        eps = O.philox_normal(SEED, R.CASE_IDX, d, 0, M, f64=dtype == np.float64)
        assert R.margin(R.case_params(case, dtype), (d, hidden, L), eps) >= need


def _criterion_inputs(kind, case=(5, (16, 7), 2, 33)):
    d, hidden, L, M = case
    arch = (d, hidden, L)
    p = R.case_params(case, np.float32)
    eps = O.philox_normal(SEED, R.CASE_IDX, d, 0, M)
    _, tgt = make_problem(np.random.default_rng(5), "diag", d, np.float32)
    ref64 = R.estimate_gradient(p, arch, tgt, eps, kind)
    ell, G = R.target_columns(tgt, ref64["Z"])
    ref = R.evaluate(p, arch, G, ell, eps, kind, np.float64)
    yard = R.evaluate(p, arch, G, ell, eps, kind, np.float32)
    return arch, p, eps, G, ell, ref, yard


@pytest.mark.parametrize("kind", [R.MONTE_CARLO, R.STL])
def test_block_criterion_admits_other_sample_orders(kind):
    arch, p, eps, G, ell, ref, yard = _criterion_inputs(kind)
    for k in range(16):
        order = np.random.default_rng(100 + k).permutation(eps.shape[1])
        got = R.evaluate(p, arch, G, ell, eps, kind, np.float32, order=order)
        assert not R.violations(R.block_report(got["grad"], ref["grad"], yard["grad"], arch, np.float32)), k


@pytest.mark.parametrize("kind,fault", [(2, "lost_block"), (3, "lost_block"), (2, "lost_tile"), (3, "lost_tile"), (2, "swap_masks"),
                                        (3, "swap_masks"), (2, "no_kappa"), (2, "kappa_sign"), (3, "no_u")])
def test_block_criterion_sees_injected_faults(kind, fault):
    # (exchanged masks keep the nets' shapes only where both halves are equal: the tutorial's shape)
    arch, p, eps, G, ell, ref, yard = _criterion_inputs(kind, (2, (16, 16), 3, 8)) if fault == "swap_masks" else _criterion_inputs(kind)
    got = R.evaluate(p, arch, G, ell, eps, kind, np.float32, fault=fault)
    assert R.violations(R.block_report(got["grad"], ref["grad"], yard["grad"], arch, np.float32))


@pytest.mark.parametrize("d,hidden,L", [(2, (16, 16), 3), (5, (16, 7), 2), (17, (33, 20, 7), 3), (128, (64,), 2)])
def test_package_layout_and_constructor_match_the_written_out_layout(d, hidden, L):
    """families.flow_layout / avi.RealNVP against the layout flow_ref writes out from include/mivi.h: offsets, shapes, the weights' draws."""
    import advancedvi_jl_amd as avi
    assert avi.flow_layout(d, hidden, L) == R.flow_layout(d, hidden, L)
    q = avi.RealNVP(d, hidden, L, rng=3)
    want = R.case_params((d, hidden, L, 1), np.float64, 3)
    for name, sl in R.blocks((d, hidden, L)):
        assert np.array_equal(q.params[sl], want[sl] if ".W" in name else np.zeros(sl.stop - sl.start)), name
    assert len(q.params) == R.flow_layout(d, hidden, L)[1]


# ---- the per-entry criterion (tests/test_gpu_flow_yardstick.py) -----------------------------------------------------------------------
# Figures printed by these tests (float32, diagonal target; worst over both estimators), as tests/test_gpu_flow_yardstick.py quotes them:
#   further orders   the float32 evaluation under 16 sample orders outside the envelope's eight: whole 0.80, row 1.49, entry 2.31,
#                    value 0.45 (Z and log q do not depend on the order: 1.00).  The envelope's OWN eight orders give at most 1 by
#                    construction, which is asserted; an order outside them can exceed any envelope that is not padded, so "at most 1"
#                    cannot hold for them: the assertion is half the criterion's factor (and the whole factor for the emulation).
#   kernel order     the emulation (K = 4 groups, float64 tile partials, slices in order): whole 0.59, row 1.97, entry 5.29 (the 1.06 M
#                    entries of (128, (64, 64, 64), 32, 1), where M = 1 leaves one evaluation in the envelope), value 0.45, Z 2.76, log q 1.20
from tests.measure_space_cases import F32_FACTOR  # noqa: E402

YARD = list(R.YARD_CASES)
_CRIT = {}


def yid(c):
    return f"{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}-{c[3]}-{c[4]}"


def _crit(case, kind, dtype=np.float32):
    """(params, eps, criterion) of a YARD_CASES entry on the draws of estimate CASE_IDX with the diagonal target; computed once"""
    key = (case, kind, np.dtype(dtype).name)
    if key not in _CRIT:
        d = case[0]
        p = R.yard_params(case, dtype)
        eps = O.philox_normal(SEED, R.CASE_IDX, d, 0, case[3], f64=dtype == np.float64)
        _, tgt = make_problem(np.random.default_rng(5), "diag", d, dtype)
        _CRIT[key] = (p, eps, R.criterion(p, case[:3], tgt, eps, kind, dtype))
    return _CRIT[key]


@pytest.mark.parametrize("kind", [R.MONTE_CARLO, R.STL])
@pytest.mark.parametrize("case,seed", [((5, (16, 7), 2, 33, "dead"), None), ((5, (16, 7), 2, 33, "sat4"), None), ((5, (16, 7), 2, 33, "sat16"), None),
                                       ((4, (6, 5), 3, 7, "dead"), 0), ((9, (8,), 8, 5, "damped"), 4)], ids=lambda v: yid(v) if isinstance(v, tuple) else "")
def test_new_evaluate_features_equal_autograd(case, seed, kind):
    """the classes' parameters (a dead unit: torch's leaky_relu has slope 0.01 at 0 too; saturated tanh; damped at L = 8), sech^2 from the
    pre-activation, the kernels' order and the tile sums, all in float64 against torch autograd"""
    d, M, arch = case[0], case[3], case[:3]
    p = R.yard_params(case, np.float64, seed)
    rng = np.random.default_rng(11 + d)
    eps = rng.normal(size=(d, M))
    _, tgt = make_problem(rng, "dense", d)
    ref = R.estimate_gradient(p, arch, tgt, eps, kind)
    ell, G = R.target_columns(tgt, ref["Z"])
    scale = np.linalg.norm(ref["grad"])
    for kw in (dict(), dict(sech_from_pre=True), dict(emulate=True), dict(tile_sums=True), dict(order=R.kernel_order(M))):
        ev = R.evaluate(p, arch, G, ell, eps, kind, np.float64, **kw)
        assert np.linalg.norm(ev["Z"] - ref["Z"]) <= 1e-9 * np.linalg.norm(ref["Z"]), kw
        assert np.linalg.norm(ev["logq"] - ref["logq"]) <= 1e-9 * np.linalg.norm(ref["logq"]), kw
        assert abs(ev["value"] - ref["value"]) <= 1e-9 * abs(ref["value"]), kw
        assert np.linalg.norm(ev["grad"] - ref["grad"]) <= 1e-9 * scale, kw
    z = torch.tensor(ref["Z"])
    assert np.allclose(R.inverse_np(p, arch, ref["Z"]), R.logpdf(torch.tensor(p), arch, z).numpy(), rtol=1e-10, atol=1e-10)
    if case[4] == "dead":
        rows = R.dead_rows(case)
        assert rows.size and np.all(ref["grad"][rows] != 0.0)
        live = R.evaluate(p, arch, G, ell, eps, kind, np.float64, fault="kink_slope_1")["grad"]
        assert np.allclose(100.0 * ref["grad"][rows], live[rows], rtol=1e-9, atol=0)   # 0.01 x what a live unit would get


def test_kernel_order_and_slices():
    for M in (1, 16, 17, 1024, 1040, 2049):
        assert np.array_equal(np.sort(R.kernel_order(M)), np.arange(M))
    assert R.flow_slices(1024) == 64 and R.flow_slices(1040) == 64 and R.flow_slices(600) == 38 and R.flow_slices(1, 1 << 20) == 1
    assert list(R.kernel_order(1040)[:32]) == list(range(16)) + list(range(1024, 1040))   # slice 0: the tiles 0 and 64
    assert len(R.orders(33)) == R.N_ORDERS and len(R.orders(1)) == 1
    for case in R.MANY_TILES:   # several tiles per slice, and a partial last tile that is a slice's third
        assert case[3] > 1024 and R.flow_slices(case[3], R.flow_layout(*case[:3])[1]) == 64
    assert len(R.MANY_TILES) == 2 and (2049 + 15) // 16 == 129 and 128 % 64 == 0 and 2049 - 128 * 16 == 1


@pytest.mark.parametrize("case", YARD, ids=yid)
def test_yard_cases_meet_the_kink_condition(case):
    """A condition on the inputs that holds at depth: every hidden pre-activation that rounding can move has |pre| >= 8 x 8 x u x S_pre, S_pre
    from flow_ref.magnitude with the carried error of the layer's input, and the earlier 1e-4 / 1e-12 of |W| |h| + |b| (the stronger of the
    two on every case: S_pre is 2 .. 15 x that scale).  The seeds are the first with room KINK_ROOM; the condition itself is room >= 1."""
    d, hidden, L, M, cls = case
    for dtype in (np.float32, np.float64):
        eps = O.philox_normal(SEED, R.CASE_IDX, d, 0, M, f64=dtype == np.float64)
        room = R.kink_room(R.yard_params(case, dtype), (d, hidden, L), eps, dtype)
        print(f"[flow criterion] kink room {yid(case)} {np.dtype(dtype).name}: {room:.3g}")
        assert room >= 1.0
    if cls == "dead":   # the dead units' pre-activations ARE exactly 0 in float32 and float64
        p = R.yard_params(case, np.float32)
        for l, net, j, u_ in R.dead_units(case):
            nets = R._nets(p, case[:3], lambda v, o, i: v.reshape((o, i), order="F"))
            W, b = nets[l][net][j - 1]
            assert not W[u_].any() and b[u_] == 0 and nets[l][net][j][0][:, u_].all()


@pytest.mark.parametrize("kind", [R.MONTE_CARLO, R.STL])
@pytest.mark.parametrize("case", YARD, ids=yid)
def test_float32_evaluation_stays_inside_its_own_criterion(case, kind):
    """The criterion is not tighter than rounding: the envelope's own orders give at most 1, 16 further orders and the emulation of the
    kernels' order stay below the factor with room (figures above)."""
    p, eps, cr = _crit(case, kind)
    arch, M = case[:3], case[3]
    for o in R.orders(M, len(p)):
        r = R.all_ratios(R.evaluate(p, arch, cr["G"], cr["ell"], eps, kind, np.float32, order=o, tile_sums=True), cr, arch, np.float32)
        assert max(r.values()) <= 1.0 + 1e-12, r
    worst = {}
    for k in range(16 if M > 1 else 0):
        y = R.evaluate(p, arch, cr["G"], cr["ell"], eps, kind, np.float32, order=np.random.default_rng(2000 + k).permutation(M), tile_sums=True)
        worst = {n: max(worst.get(n, 0.0), v) for n, v in R.all_ratios(y, cr, arch, np.float32).items()}
    emu = R.all_ratios(R.evaluate(p, arch, cr["G"], cr["ell"], eps, kind, np.float32, emulate=True), cr, arch, np.float32)
    print(f"[flow criterion] {yid(case)} kind {kind}: further orders " + " ".join(f"{n} {v:.2f}" for n, v in worst.items())
          + " | kernel order " + " ".join(f"{n} {v:.2f}" for n, v in emu.items()))
    assert max(worst.values(), default=0.0) <= F32_FACTOR / 2 and max(emu.values()) <= F32_FACTOR


FAULT_CASES = [("tile_overwrites", (5, (8,), 2, 1040, "default")), ("kink_slope_1", (5, (16, 7), 2, 33, "dead")),
               ("one_entry", (64, (64, 64), 4, 16, "default")), ("one_row", (64, (64, 64), 4, 16, "default")),
               ("layer_off", (17, (33, 20, 7), 3, 16, "default")), ("sech_from_f32_s_twice", (3, (5,), 1, 1, "default")),
               ("lost_tile", (5, (16, 7), 2, 33, "default")), ("lost_block", (3, (5,), 1, 1, "default"))]


@pytest.mark.parametrize("kind", [R.MONTE_CARLO, R.STL])
@pytest.mark.parametrize("fault,case", FAULT_CASES, ids=[f for f, _ in FAULT_CASES])
def test_per_entry_criterion_sees_injected_faults(fault, case, kind):
    """Each fault on the smallest case that can show it (tile_overwrites needs several tiles per slice, one_entry / one_row a 64 x 64
    block, layer_off three layers).  Printed beside it: whether the per-block criterion of tests/test_gpu_flow.py sees it.  Measured
    (kind 2 / 3, the worst ratio; block_report): tile_overwrites 9.1e5 / 9.7e5, seen; kink_slope_1 4.7e8 / 5.8e8, seen; one_entry
    3.2e2 / 4.3e2, NOT seen; one_row 5.3e2 / 4.7e2, NOT seen; layer_off 1.7e9 / 1.7e9, seen; sech_from_f32_s_twice 2.3e5 / 3.2e5, seen."""
    p, eps, cr = _crit(case, kind)
    arch = case[:3]
    got = R.evaluate(p, arch, cr["G"], cr["ell"], eps, kind, np.float32, fault=fault)
    r = R.all_ratios(got, cr, arch, np.float32)
    seen = bool(R.violations(R.block_report(got["grad"], cr["ref"]["grad"], cr["yard"]["grad"], arch, np.float32)))
    print(f"[flow criterion] fault {fault} on {yid(case)} kind {kind}: " + " ".join(f"{n} {v:.3g}" for n, v in r.items()) + f" | block_report sees it: {seen}")
    assert max(r["whole"], r["row"], r["entry"]) > F32_FACTOR, r
    if fault in ("one_entry", "one_row"):   # what the per-block l2 criterion lets through (the reason for this file)
        assert not seen and r["entry"] > 10 * F32_FACTOR
