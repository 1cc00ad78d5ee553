"""Host-side checks of KLMinNaturalGradDescent (src/algorithms/klminnaturalgraddescent.jl): the numpy restatement of its update
(tests/natgrad_ref.py) -- what Hermitian reads, the library's lower scale against the reference's upper one, the exact-Newton fixed point,
what ensure_posdef buys, the reference's convergence test on its own model -- the emulation of the tile kernels' documented order, and the
boundary (header, ctypes table, exports).  No GPU compute."""
import os
import re

import numpy as np
import pytest

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import _lib
from oracle import oracle as O
from tests import natgrad_ref as R
from tests import solve_ref as S
from tests.helpers import make_family

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("mivi_natgrad_init", "mivi_natgrad_update", "mivi_natgrad_update_host", "mivi_natgrad_steps")


def _case(d, seed, symmetric=False):
    rng = np.random.default_rng(seed)
    _, q = make_family(rng, d, avi.FULLRANK)
    C = np.tril(q.scale)
    S0, P0 = R.init_state(C)
    return q.location, C, S0, P0, rng.normal(size=d), R.congruent_hessian(C, rng, symmetric), rng


@pytest.mark.parametrize("ensure", [True, False])
def test_hermitian_takes_the_upper_triangle(ensure):
    m, C, S0, P0, g, H, _ = _case(7, 21)
    eta = 0.3
    assert np.linalg.norm(H - H.T) > 1e-3 * np.linalg.norm(H)
    S_new = R.update(m, S0, P0, g, H, eta, ensure)[1]
    Gh = S0 + H
    E = S0 - eta * Gh + eta ** 2 / 2 * Gh @ P0 @ Gh if ensure else (1 - eta) * S0 - eta * H
    explicit = np.triu(E) + np.triu(E, 1).T
    assert np.allclose(S_new, explicit, rtol=1e-13, atol=1e-15) and np.array_equal(S_new, S_new.T)
    assert np.linalg.norm(S_new - 0.5 * (E + E.T)) > 1e-3 * np.linalg.norm(S_new)


@pytest.mark.parametrize("d", [1, 5, 33, 70])
def test_lower_scale_is_the_cholesky_factor_of_the_covariance(d):
    m, C, S0, P0, g, H, _ = _case(d, 22 + d)
    _, S_new, Sigma_new, U = R.update(m, S0, P0, g, H, 0.2, True)
    Cl = R.lower_scale(S_new)
    assert np.all(np.triu(Cl, 1) == 0.0) and np.all(np.diag(Cl) > 0.0)
    assert np.all(np.tril(U, -1) == 0.0)                                  # the reference's scale is upper triangular
    assert np.allclose(Cl, np.linalg.cholesky(Sigma_new), rtol=1e-10, atol=1e-13)
    assert np.allclose(U @ U.T, Cl @ Cl.T, rtol=1e-10, atol=1e-13)
    assert abs(R.entropy(Cl) - R.entropy(U)) <= 1e-12 * abs(R.entropy(Cl))


def test_exact_newton_fixed_point():
    """Dense Gaussian target N(mu, P^-1): g = -P (m - mu), H = -P; the plain rule with eta = 1 lands on S' = P, m' = mu in one step."""
    rng = np.random.default_rng(23)
    d = 9
    _, q = make_family(rng, d, avi.FULLRANK)
    A = rng.normal(size=(d, d))
    P = A @ A.T / d + np.eye(d)
    mu = rng.normal(size=d)
    S0, P0 = R.init_state(q.scale)
    m_new, S_new, Sigma_new, _ = R.update(q.location, S0, P0, -P @ (q.location - mu), -P, 1.0, False)
    assert np.allclose(S_new, P, rtol=1e-13, atol=1e-14)
    assert np.allclose(m_new, mu, rtol=1e-11, atol=1e-12)
    assert np.allclose(Sigma_new, np.linalg.inv(P), rtol=1e-11, atol=1e-13)


def test_ensure_posdef_does_what_its_name_says():
    """S - eta Gh + eta^2/2 Gh Sigma Gh = S/2 + (I - eta Gh Sigma) S (I - eta Sigma Gh)/2 for symmetric Gh: an indefinite symmetric H breaks the
    plain rule's Cholesky and not the ensured rule's."""
    m, C, S0, P0, g, _, rng = _case(8, 24)
    H = 10.0 * np.diag(np.where(np.arange(8) % 2 == 0, 1.0, -1.0)) * np.linalg.norm(S0, 2)
    with pytest.raises(np.linalg.LinAlgError):
        R.update(m, S0, P0, g, H, 0.5, False)
    _, S_new, _, _ = R.update(m, S0, P0, g, H, 0.5, True)
    assert np.min(np.linalg.eigvalsh(S_new)) > 0.0
    Gh, I = S0 + H, np.eye(8)
    assert np.allclose(S_new, 0.5 * S0 + 0.5 * (I - 0.5 * Gh @ P0) @ S0 @ (I - 0.5 * P0 @ Gh), rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("ensure", [True, False], ids=["ensure", "plain"])
@pytest.mark.parametrize("capability", [1, 2])
def test_reference_convergence(capability, ensure):
    """test/algorithms/klminnaturalgraddescent.jl:75-90 on its own model (test/models/normal.jl `normal_meanfield`: d = 5, mu = 5,
    sigma = 0.3), q0 = N(0, I), stepsize 1e-3, 10 samples, 1000 iterations."""
    d, T, n = 5, 1000, 10
    mu_true, L_true = np.full(d, 5.0), 0.3 * np.eye(d)
    tgt = O.DiagNormalTarget(mu_true, np.full(d, 0.3))
    rng = np.random.default_rng(0x38BEF07C)
    q0 = O.MvLocationScale(np.zeros(d), np.eye(d))
    q, _, elbos = R.steps(q0, tgt, lambda q: rng.normal(size=(d, n)), 1e-3, capability == 2, ensure, n_steps=T)
    d0 = np.sum((q0.location - mu_true) ** 2) + np.sum((q0.scale - L_true) ** 2)
    dl = np.sum((q.location - mu_true) ** 2) + np.sum((q.scale - L_true) ** 2)
    print(f"[natgrad convergence] capability {capability} ensure {ensure}: ratio {dl / d0:.4f}")
    assert np.all(np.isfinite(elbos))
    assert dl <= 0.1 * d0


@pytest.mark.parametrize("d", [70, 256])
@pytest.mark.parametrize("kind", ["default", "graded", "spd2", "ar999"])
def test_emulation_of_the_tile_path(kind, d):
    """The tile kernels' documented order (R.emulate_tiles) is the reference's update: in float64 it agrees with the restatement to
    1e-16 .. 4e-12 on these cases, in step with their conditioning.  The same order in float32 is printed by the yardstick, not asserted: the
    device's tile path computes in float64 (csrc/kernels_natgrad.hip), because with kappa(S') = 1e5 no float32 factorisation of a float32 S'
    holds the factor 8 (LAPACK's own reaches 7 to 10 there)."""
    m, C, g, H = R.conditioning_case(kind, d)
    S0, P0 = R.init_state(C, np.float32)
    for eta in (0.1, 0.5):
        for ensure in (True, False):
            ref = R.update(m, S0, P0, g, H, eta, ensure, np.float64)
            yard = R.update(m, S0, P0, g, H, eta, ensure, np.float32)
            emu = R.emulate_tiles(m, S0, P0, g, H, eta, ensure, np.float32)
            e64 = R.emulate_tiles(m, S0, P0, g, H, eta, ensure, np.float64)
            C_ref, C_yard = R.lower_scale(ref[1]), R.lower_scale(yard[1], np.float32)
            for name, got, y, r, g64 in (("m", emu[0], yard[0], ref[0], e64[0]), ("C", emu[3], C_yard, C_ref, e64[3]),
                                         ("S", emu[1], yard[1], ref[1], e64[1]), ("Sigma", emu[2], yard[2], ref[2], e64[2])):
                whole, block = S.block_ratios(got, y, r, d)
                print(f"[natgrad emulation] {kind} {d} eta {eta} ensure {ensure} {name}: {whole:.2f}, {block:.2f}")
                assert np.linalg.norm(g64 - r) <= 1e-10 * np.linalg.norm(r), (name, eta, ensure)


def test_header_ctypes_and_exports():
    hdr = open(os.path.join(ROOT, "include", "mivi.h")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"mivi_status_t\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
    assert "klminnaturalgraddescent.jl" in hdr
    assert int(re.search(r"#define\s+MIVI_NATGRAD_SMALL_D\s+(\d+)", hdr).group(1)) == avi.NATGRAD_SMALL_D
    alg = avi.KLMinNaturalGradDescent(1e-3, n_samples=10)
    assert alg.n_samples == 10 and alg.ensure_posdef is True and alg.subsampling is None
    assert avi.KLMinNaturalGradDescent(stepsize=0.5, ensure_posdef=False).ensure_posdef is False
    with pytest.raises(ValueError):
        avi.KLMinNaturalGradDescent(1e-3, n_samples=0)


def test_init_rejects_order0_and_meanfield():
    """klminnaturalgraddescent.jl:73-79 (and the LowerTriangular dispatch of :67): raised before any device is touched."""
    class Order0:
        def dimension(self):
            return 3

        def logdensity(self, z):
            return -0.5 * float(np.sum(np.asarray(z) ** 2))

    alg = avi.KLMinNaturalGradDescent(stepsize=1.0, n_samples=10)
    q0 = avi.FullRankGaussian(np.zeros(3), np.eye(3))
    with pytest.raises(ValueError, match="`KLMinNaturalGradDescent` requires at least first-order"):
        avi.init(avi.PhiloxRNG(1), alg, q0, Order0())
    with pytest.raises(ValueError, match="first-order"):
        avi.optimize(alg, 1, Order0(), q0)
    with pytest.raises(TypeError):
        avi.init(avi.PhiloxRNG(1), alg, avi.MeanFieldGaussian(np.zeros(3), np.ones(3)), avi.DiagNormalProblem(np.zeros(3), np.ones(3)))
