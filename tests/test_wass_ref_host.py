"""KLMinWassFwdBwd without a GPU (src/algorithms/klminwassfwdbwd.jl): the two forms of tests/wass_ref.py -- the reference's literal
expression and the products-only Newton-Schulz form csrc/kernels_wass.hip is documented to build, neither of them code under test -- agree
on the fixtures the GPU tests use (conditions on the fixtures), the findings the device form stands on (the stop rule and its round counts,
the stagnation stop, no mirroring inside the iteration), the reference's convergence test on its own model, and the boundary (header,
library, ctypes table, constructor, init's refusals).

Measured (float64 numpy, relative l2 against update_literal):
    second / stein, d in {3 .. 130}, eta in {1e-3, 0.1, 1}    C' at most 1.3e-13, Sigma' at most 8.0e-14; 9 to 33 rounds
    singular (d in {10, 65})                                  C' 4e-16 .. 1.6e-7, Sigma' 5e-16 .. 3.6e-9, each within ten times the distance of
                                                              update_literal and the per-eigenvalue form (C' 1.2e-10 .. 1.5e-7); 12 to 59 rounds
    the mirrored-triangle variant (second, d = 64, eta = 1)   Sigma' 7.5e-3
    tightened to 1e-14 on a singular fixture                  Y and Z run away: the result is not finite or not positive definite
    1000 steps on normal_meanfield                            2.8e-6 (Hessians), 1.4e-5 (Stein) of the initial squared distance"""
import os
import re

import numpy as np
import pytest

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import _lib
from oracle import oracle as O
from tests import wass_ref as R
from tests.helpers import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("mivi_wass_init", "mivi_wass_update", "mivi_wass_update_host", "mivi_wass_steps")
DS = (3, 10, 44, 45, 64, 65, 130)          # tests/test_gpu_wass.py
ETAS = (1e-3, 0.1, 1.0)
FORMS_TOL = 1e-11


def _forms(kind, d, eta):
    m, C, g, H = R.fixture(kind, d, eta)
    Sigma = R.hermitian(C @ C.T)
    return R.update_literal(m, Sigma, g, H, eta), R.update_iterated(m, Sigma, g, H, eta), (m, Sigma, g, H)


@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("kind", ["second", "stein"])
def test_the_two_forms_agree(kind, d, eta):
    lit, it, (_, _, _, H) = _forms(kind, d, eta)
    assert (np.linalg.norm(H - H.T) > 1e-3 * np.linalg.norm(H)) == (kind == "stein")
    errs = tuple(rel_err(it[i], lit[i]) for i in range(3))
    print(f"[wass forms] {kind} {d} eta {eta}: m {errs[0]:.1e} C {errs[1]:.1e} Sigma {errs[2]:.1e} rounds {it[3]}")
    assert max(errs) <= FORMS_TOL
    assert it[3] < R.MAX_ROUNDS
    assert np.min(np.linalg.eigvalsh(it[2])) >= eta * (1.0 - 1e-12)          # Sigma' >= eta I


@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("d", [10, 65])
def test_singular_forms_agree_to_the_branch_point(d, eta):
    """M = I + eta H' singular: A has an eigenvalue that is zero up to rounding, where the square root is not differentiable.  The iterated
    form is as far from the literal one as the per-eigenvalue form of the same expression is, up to the factor ten."""
    lit, it, (m, Sigma, g, H) = _forms("singular", d, eta)
    assert np.linalg.svd(np.eye(d) + eta * H.T, compute_uv=False)[-1] <= 1e-14
    spec = R.update_spectral(m, Sigma, g, H, eta)
    errs = tuple(rel_err(it[i], lit[i]) for i in range(3))
    yard = tuple(rel_err(spec[i], lit[i]) for i in range(3))
    print(f"[wass singular] {d} eta {eta}: C {errs[1]:.1e} (forms {yard[1]:.1e}) Sigma {errs[2]:.1e} (forms {yard[2]:.1e}) rounds {it[3]}")
    assert errs[0] <= 1e-15 and errs[1] <= 10.0 * yard[1] and errs[2] <= 10.0 * yard[2]
    assert it[3] < R.MAX_ROUNDS
    assert np.min(np.linalg.eigvalsh(it[2])) >= eta * (1.0 - 1e-9)


def test_mirroring_inside_the_iteration_is_not_accurate():
    """Forming the lower triangles of Z Y, Y E and E Z alone and mirroring them in every round halves the work and breaks the coupling."""
    m, C, g, H = R.fixture("second", 64, 1.0)
    Sigma = R.hermitian(C @ C.T)
    lit = R.update_literal(m, Sigma, g, H, 1.0)
    err = rel_err(R.update_iterated(m, Sigma, g, H, 1.0, mirror=True)[2], lit[2])
    print(f"[wass mirrored] Sigma {err:.1e}")
    assert err > 1e3 * FORMS_TOL
    assert rel_err(R.update_iterated(m, Sigma, g, H, 1.0)[2], lit[2]) <= FORMS_TOL


def test_the_stagnation_stop_is_part_of_the_method():
    """Rounding left A a slightly NEGATIVE eigenvalue in M's null direction here: r_k turns round at k = 12 and the rule stops there.
    Iterating on to a tighter residual lets Y and Z run away along that direction: what comes out is not finite or not a covariance."""
    m, C, g, H = R.fixture("singular", 10, 0.1)
    Sigma = R.hermitian(C @ C.T)
    assert R.update_iterated(m, Sigma, g, H, 0.1)[3] < 16
    try:
        _, C_new, _, rounds = R.update_iterated(m, Sigma, g, H, 0.1, tol=1e-14)
    except np.linalg.LinAlgError:   # finite, and not positive definite
        C_new, rounds = None, R.MAX_ROUNDS
    print(f"[wass past stagnation] rounds {rounds}")
    assert C_new is None and rounds == R.MAX_ROUNDS


@pytest.mark.parametrize("capability", [1, 2])
def test_reference_convergence(capability):
    """test/algorithms/klminwassfwdbwd.jl on its own model (test/models/normal.jl `normal_meanfield`: d = 5, mu = 5, sigma = 0.3),
    q0 = N(0, I), stepsize 1e-3, 10 samples, 1000 iterations; the update is the iterated form."""
    d, T, n = 5, 1000, 10
    mu_true, L_true = np.full(d, 5.0), 0.3 * np.eye(d)
    tgt = O.DiagNormalTarget(mu_true, np.full(d, 0.3))
    rng = np.random.default_rng(0x38BEF07C)
    q0 = O.MvLocationScale(np.zeros(d), np.eye(d))
    q, _, elbos = R.steps(q0, tgt, [rng.normal(size=(d, n)) for _ in range(T)], 1e-3, capability == 2, update=R.update_iterated)
    d0 = np.sum((q0.location - mu_true) ** 2) + np.sum((q0.scale - L_true) ** 2)
    dl = np.sum((q.location - mu_true) ** 2) + np.sum((q.scale - L_true) ** 2)
    print(f"[wass convergence] capability {capability}: ratio {dl / d0:.1e}")
    assert np.all(np.isfinite(elbos))
    assert dl <= 0.1 * d0


def test_header_library_ctypes_and_exports(lib):
    hdr = open(os.path.join(ROOT, "include", "mivi.h")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"mivi_status_t\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "klminwassfwdbwd.jl" in hdr
    assert int(re.search(r"#define\s+MIVI_WASS_MAX_ROUNDS\s+(\d+)", hdr).group(1)) == R.MAX_ROUNDS
    alg = avi.KLMinWassFwdBwd(1e-3, n_samples=10)
    assert alg.stepsize == 1e-3 and alg.n_samples == 10 and alg.subsampling is None
    assert "KLMinWassFwdBwd(stepsize=0.001, n_samples=10" in repr(alg)
    assert isinstance(alg, avi.measure_space.ALGORITHMS) and "wass" in avi.measure_space.STATE_BUFFERS
    with pytest.raises(ValueError):
        avi.KLMinWassFwdBwd(1e-3, n_samples=0)


def test_init_rejects_order0_and_meanfield():
    """klminwassfwdbwd.jl:65-71 (and the LowerTriangular dispatch of :59): raised before any device is touched."""
    class Order0:
        def dimension(self):
            return 3

        def logdensity(self, z):
            return -0.5 * float(np.sum(np.asarray(z) ** 2))

    alg = avi.KLMinWassFwdBwd(stepsize=1.0, n_samples=10)
    q0 = avi.FullRankGaussian(np.zeros(3), np.eye(3))
    with pytest.raises(ValueError, match="`KLMinWassFwdBwd` requires at least first-order"):
        avi.init(avi.PhiloxRNG(1), alg, q0, Order0())
    with pytest.raises(ValueError, match="first-order"):
        avi.optimize(alg, 1, Order0(), q0)
    with pytest.raises(TypeError, match="KLMinWassFwdBwd"):
        avi.init(avi.PhiloxRNG(1), alg, avi.MeanFieldGaussian(np.zeros(3), np.ones(3)), avi.DiagNormalProblem(np.zeros(3), np.ones(3)))
