"""Host tests of tests/flow_ref.py, the restatement the GPU tests of the RealNVP family (tests/test_gpu_flow.py) are held against: the
numpy evaluation with its hand-written backward sweeps equals torch autograd on the literal definition, the cases' inputs keep every
leakyrelu away from its kink, and the per-block criterion admits the yardstick under other summation orders and sees injected faults."""
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
