"""Host-side checks of KLMinSqrtNaturalGradDescent (src/algorithms/klminsqrtnaturalgraddescent.jl): the numpy restatement of its update
(tests/ngd_ref.py) -- fixed point, orientation of H, the reference's convergence test on its own model -- and the boundary (header,
ctypes table, exports, Julia glue).  No GPU compute."""
import os
import re

import numpy as np
import pytest

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import _lib
from oracle import oracle as O
from tests import ngd_ref as N
from tests.helpers import make_family

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("mivi_sqrt_ngd_update", "mivi_sqrt_ngd_update_host", "mivi_sqrt_ngd_steps")


def test_fixed_point():
    """g = 0 and H = -Sigma^-1 with C C' = Sigma: A = C' Sigma^-1 C - I = 0, so (m, C) stays where it is, to rounding."""
    rng = np.random.default_rng(11)
    d = 9
    _, q = make_family(rng, d, avi.FULLRANK)
    C = np.tril(q.scale)
    H = -np.linalg.inv(C @ C.T)
    m_new, C_new, ent = N.update(q.location, C, np.zeros(d), H, 0.3)
    assert np.array_equal(m_new, q.location)
    assert np.linalg.norm(C_new - C) <= 1e-13 * np.linalg.norm(C)
    assert abs(ent - O.entropy_closed_form(q)) <= 1e-12 * abs(ent)


def test_hessian_orientation():
    """A non-symmetric H (what the Stein branch returns) is used as it comes: its transpose and its symmetrisation give other C'."""
    rng = np.random.default_rng(12)
    d = 7
    _, q = make_family(rng, d, avi.FULLRANK)
    g = rng.normal(size=d)
    H = rng.normal(size=(d, d)) - np.eye(d)
    base = N.update(q.location, q.scale, g, H, 0.05)[1]
    C = np.tril(q.scale)
    expect = C - 0.05 * C @ (np.tril(C.T @ (-H) @ C - np.eye(d)) - 0.5 * np.diag(np.diag(C.T @ (-H) @ C - np.eye(d))))
    assert np.allclose(base, expect, rtol=1e-13, atol=1e-15)
    assert np.all(np.triu(base, 1) == 0.0)
    for other in (H.T, 0.5 * (H + H.T)):
        C_other = N.update(q.location, q.scale, g, other, 0.05)[1]
        assert np.linalg.norm(C_other - base) > 1e-3 * np.linalg.norm(base)


def test_update_flat_and_dtype():
    rng = np.random.default_rng(13)
    d = 6
    _, q = make_family(rng, d, avi.FULLRANK)
    g, H = rng.normal(size=d), rng.normal(size=(d, d)) - np.eye(d)
    p64, e64 = N.update_flat(O.destructure(q), g, H, 0.05)
    m, C, e = N.update(q.location, q.scale, g, H, 0.05)
    assert np.array_equal(p64, np.concatenate([m, C.reshape(-1, order="F")])) and e64 == e
    p32, e32 = N.update_flat(O.destructure(q), g, H, 0.05, np.float32)
    assert p32.dtype == np.float32 and isinstance(e32, np.float32)
    assert np.linalg.norm(p32 - p64) <= 1e-5 * np.linalg.norm(p64)


@pytest.mark.parametrize("capability", [1, 2])
def test_reference_convergence(capability):
    """test/algorithms/klminsqrtnaturalgraddescent.jl:77-90 on its own model (test/models/normal.jl `normal_meanfield`: d = 5, mu = 5,
    sigma = 0.3), q0 = N(0, I), stepsize 1e-3, 10 samples, 1000 iterations."""
    d, T, n = 5, 1000, 10
    mu_true, L_true = np.full(d, 5.0), 0.3 * np.eye(d)
    tgt = O.DiagNormalTarget(mu_true, np.full(d, 0.3))
    rng = np.random.default_rng(0x38BEF07C)
    q0 = O.MvLocationScale(np.zeros(d), np.eye(d))
    q, elbos = N.steps(q0, tgt, lambda q: rng.normal(size=(d, n)), 1e-3, capability == 2, n_steps=T)
    d0 = np.sum((q0.location - mu_true) ** 2) + np.sum((q0.scale - L_true) ** 2)
    dl = np.sum((q.location - mu_true) ** 2) + np.sum((q.scale - L_true) ** 2)
    print(f"[ngd convergence] capability {capability}: ratio {dl / d0:.4f}")
    assert np.all(np.isfinite(elbos))
    assert dl <= 0.1 * d0


def test_header_ctypes_and_exports():
    hdr = open(os.path.join(ROOT, "include", "mivi.h")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"mivi_status_t\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
    assert "klminsqrtnaturalgraddescent.jl" in hdr
    assert avi.KLMinSqrtNaturalGradDescent(1e-3, n_samples=10).n_samples == 10
    assert avi.KLMinSqrtNaturalGradDescent(stepsize=0.5).subsampling is None
    julia = open(os.path.join(ROOT, "advancedvi.jl_amd", "julia", "MIVI.jl")).read()
    for name in NEW_ENTRIES:
        assert name in julia, name


def test_init_rejects_order0_and_meanfield():
    """klminsqrtnaturalgraddescent.jl:64-70 (and the LowerTriangular dispatch of :58): raised before any device is touched."""
    class Order0:
        def dimension(self):
            return 3

        def logdensity(self, z):
            return -0.5 * float(np.sum(np.asarray(z) ** 2))

    alg = avi.KLMinSqrtNaturalGradDescent(stepsize=1.0, n_samples=10)
    q0 = avi.FullRankGaussian(np.zeros(3), np.eye(3))
    with pytest.raises(ValueError, match="first-order"):
        avi.init(avi.PhiloxRNG(1), alg, q0, Order0())
    with pytest.raises(ValueError, match="first-order"):
        avi.optimize(alg, 1, Order0(), q0)
    with pytest.raises(TypeError):
        avi.init(avi.PhiloxRNG(1), alg, avi.MeanFieldGaussian(np.zeros(3), np.ones(3)), avi.DiagNormalProblem(np.zeros(3), np.ones(3)))
