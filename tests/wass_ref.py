"""numpy restatement of KLMinWassFwdBwd's update (src/algorithms/klminwassfwdbwd.jl:105-114) and of a loop of its steps on the oracle's
estimators -- a helper of tests/test_wass_ref_host.py and tests/test_gpu_wass.py, not a test.

    update_literal(m, Sigma, g, H, eta, dtype) -> (m', C', Sigma')
                                the reference's lines in the reference's order, every operation rounded to `dtype`:
                                    m' = m - eta (-g);  M = I - eta (-H');  Sh = Hermitian(M Sigma M')                               (:105-107)
                                    Sigma' = (Sh + 2 eta I + sqrt(Hermitian(Sh (Sh + 4 eta I)))) / 2;  C' = cholesky(Sigma').L       (:110-111)
                                the square root is eigh of the upper-mirrored product, U sqrt(w) U', with eigenvalues that rounding made
                                negative CLAMPED at zero: the reference's sqrt(::Hermitian) would turn complex there and cholesky would
                                throw; the clamp is what lets the singular fixtures have a literal value at all
    update_spectral(...)        the same Sigma' as a function of Sh's eigenvalues: U diag((w + 2 eta + sqrt(w (w + 4 eta))) / 2) U'.  On a
                                singular M it differs from update_literal by the square root's own branch point at w = 0; the distance of
                                the two is the yardstick of the singular fixtures
    update_iterated(...) -> (m', C', Sigma', rounds)
                                the form csrc/kernels_wass.hip is DOCUMENTED to build (no kernel code): the coupled Newton-Schulz iteration
                                    A = Hermitian(Sh (Sh + 4 eta I)), c = |A|_F, Y_0 = A (1/c), Z_0 = I
                                    E_k = I - Z_k Y_k, r_k = |E_k|_F, Y_k+1 = Y_k + Y_k E_k / 2, Z_k+1 = Z_k + E_k Z_k / 2
                                stopped at the first k with r_k <= 64 d eps, or from k >= 4 with r_k >= r_k-1, or with r_k >= r_k-1 / 2
                                and r_k < 1e-6; sqrt(A) = sqrt(c) (Y_k + Y_k') / 2.  `rounds` is that k (MAX_ROUNDS: never stopped).
                                mirror=True: the variant that forms only the lower triangles of Z Y, Y E and E Z and mirrors them in every
                                round -- kept to pin that it is NOT accurate.  tol: that threshold alone, no stagnation stop (to pin that iterating on runs away)
    entropy(C, dtype)           d/2 (1 + log 2 pi) + sum log C_ii
    steps(q, tgt, draws, eta, second_order, update)
                                iterations of :80-122 in float64 on oracle.gaussian_expectation_gradient_and_hessian[_order2], Sigma
                                carried from step to step
    fixture(kind, d, eta, dtype) -> (m, C, g, H)
                                kind `second`: H symmetric negative definite; `stein`: H non-symmetric; `singular`: H symmetric with an
                                eigenvalue of -1/eta in a general direction, so that M is singular to rounding"""
import zlib

import numpy as np
from scipy.linalg import cholesky

from oracle import oracle as O
from tests.natgrad_ref import entropy, hermitian   # noqa: F401  (entropy is part of this module's surface)

MAX_ROUNDS = 64   # MIVI_WASS_MAX_ROUNDS
EPS = float(np.finfo(np.float64).eps)


def _half(m, Sigma, g, H, eta, dt):
    """(m', Sh, eta) in dt."""
    m, g = np.asarray(m).astype(dt), np.asarray(g).astype(dt)
    Sigma, H = np.asarray(Sigma).astype(dt), np.asarray(H).astype(dt)
    eta = dt(eta)
    eye = np.eye(m.shape[0], dtype=dt)
    m_new = (m - eta * (-g)).astype(dt)
    M = (eye - eta * (-H.T)).astype(dt)
    Sh = hermitian(((M @ Sigma).astype(dt) @ M.T).astype(dt))
    return m_new, Sh, eta, eye


def _finish(m_new, Sh, root, eta, eye, dt):
    Sigma_new = hermitian((((Sh + dt(2) * eta * eye) + root) / dt(2)).astype(dt))
    C_new = np.tril(cholesky(Sigma_new, lower=True, check_finite=False)).astype(dt)
    return m_new, C_new, Sigma_new


def _product(Sh, eta, eye, dt):
    return hermitian((Sh @ (Sh + dt(4) * eta * eye).astype(dt)).astype(dt))


def update_literal(m, Sigma, g, H, eta, dtype=np.float64):
    dt = np.dtype(dtype).type
    m_new, Sh, eta, eye = _half(m, Sigma, g, H, eta, dt)
    w, U = np.linalg.eigh(_product(Sh, eta, eye, dt))
    root = hermitian(((U * np.sqrt(np.maximum(w, dt(0))).astype(dt)) @ U.T).astype(dt))
    return _finish(m_new, Sh, root, eta, eye, dt)


def update_spectral(m, Sigma, g, H, eta):
    dt = np.float64
    m_new, Sh, eta, eye = _half(m, Sigma, g, H, eta, dt)
    w, U = np.linalg.eigh(Sh)
    w = np.maximum(w, 0.0)
    Sigma_new = hermitian((U * ((w + 2.0 * eta + np.sqrt(w * (w + 4.0 * eta))) / 2.0)) @ U.T)
    return m_new, np.tril(cholesky(Sigma_new, lower=True, check_finite=False)), Sigma_new


def _lower_mirrored(A):
    return np.tril(A) + np.tril(A, -1).T


def update_iterated(m, Sigma, g, H, eta, mirror=False, tol=None, max_rounds=MAX_ROUNDS):
    dt = np.float64
    m_new, Sh, eta, eye = _half(m, Sigma, g, H, eta, dt)
    d = eye.shape[0]
    A = _product(Sh, eta, eye, dt)
    c = float(np.sqrt(np.sum(A * A)))
    Y, Z = A * (1.0 / c), eye.copy()
    first = 64.0 * d * EPS if tol is None else tol
    sym = _lower_mirrored if mirror else (lambda X: X)
    r_prev, rounds = np.inf, max_rounds
    with np.errstate(all="ignore"):
        for k in range(max_rounds):
            E = sym(eye - Z @ Y)
            r = float(np.sqrt(np.sum(E * E)))
            stagnated = tol is None and k >= 4 and (r >= r_prev or (r >= 0.5 * r_prev and r < 1e-6))
            if not np.isfinite(r) or r <= first or stagnated:
                rounds = k
                break
            Y, Z = sym(Y + 0.5 * (Y @ E)), sym(Z + 0.5 * (E @ Z))
            r_prev = r
    root = np.sqrt(c) * (0.5 * (Y + Y.T))
    if not np.all(np.isfinite(root)):
        return m_new, None, None, rounds
    return _finish(m_new, Sh, root, eta, eye, dt) + (rounds,)


def steps(q, tgt, draws, eta, second_order, update=update_literal):
    """Iterations of `step` in float64.  draws: a list of d x n matrices, one per iteration.  Returns (q_final, Sigma, [elbo_t])."""
    est = O.gaussian_expectation_gradient_and_hessian_order2 if second_order else O.gaussian_expectation_gradient_and_hessian
    C = np.tril(np.asarray(q.scale, dtype=np.float64))
    Sigma = hermitian(C @ C.T)
    elbos = []
    for u in draws:
        logpi, g, H = est(q, tgt, np.asarray(u, dtype=np.float64))
        m_new, C_new, Sigma = update(q.location, Sigma, g, H, eta)[:3]
        q = O.MvLocationScale(m_new, C_new)
        elbos.append(float(logpi + entropy(C_new)))
    return q, Sigma, elbos


KINDS = ("second", "stein", "singular")


def fixture(kind, d, eta, dtype=np.float64):
    """(m, C, g, H) in dtype: a Wishart-like covariance C C' (C lower triangular, positive diagonal) and a Hessian of the given kind."""
    # (`singular`: how small the eigenvalue of A in M's null direction comes out -- anything from 0 to 1e-16 |A|, either sign -- is rounding's
    # choice, and with it the round count and the distance of any two forms; this seed's six fixtures cover 12 to 59 rounds)
    rng = np.random.default_rng(zlib.crc32(kind.encode()) + 1000 * d + int(round(1000 * eta)) + (100000 if kind == "singular" else 0))
    C = np.tril(rng.normal(size=(d, d)) / np.sqrt(d))
    C[np.diag_indices(d)] = rng.uniform(0.5, 1.5, d)
    m, g = rng.normal(size=d), rng.normal(size=d)
    B = rng.normal(size=(d, d))
    H = -(B @ B.T / d + 0.5 * np.eye(d))
    if kind == "stein":
        H = H + 0.3 * rng.normal(size=(d, d)) / np.sqrt(d)
    elif kind == "singular":   # H = Q diag(w) Q with Q a Householder reflection and w_0 = -1/eta: M = I + eta H' has a null direction
        v = rng.normal(size=d)
        Q = np.eye(d) - 2.0 * np.outer(v, v) / (v @ v)
        w = -rng.uniform(0.5, 2.0, d)
        w[0] = -1.0 / eta
        H = (Q * w) @ Q
        H = 0.5 * (H + H.T)
    elif kind != "second":
        raise ValueError(kind)
    return m.astype(dtype), C.astype(dtype), g.astype(dtype), H.astype(dtype)
