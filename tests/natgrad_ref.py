"""numpy restatement of KLMinNaturalGradDescent's state and update (src/algorithms/klminnaturalgraddescent.jl:83-87, :129-145) and of a loop
of its steps on the oracle's estimators -- a helper of tests/test_natgrad_ref_host.py and tests/test_gpu_natgrad.py, not a test.

    hermitian(A)                              Julia's Hermitian(A): the UPPER triangle of A, mirrored (not the symmetric part)
    init_state(C, dtype)                      (S, Sigma) of `init`: Sigma = Hermitian(C C'), S = Hermitian(C^-T C^-1)                 (:83-87)
    update(m, S, Sigma, g, H, eta, ensure_posdef, dtype) -> (m', S', Sigma', U)
                                              the reference's lines in the reference's order, left to right, every operation rounded to `dtype`:
                                                  Gh = S - (-H);  S' = Hermitian(S - eta Gh + eta^2 / 2 Gh Sigma Gh)                  (:129-130)
                                                  or S' = Hermitian((1 - eta) S + eta (-H))                                           (:132)
                                                  m' = m - eta (S' \\ (-g))         two substitutions on scipy.linalg.cholesky(S')     (:134)
                                                  L = cholesky(S').L;  U = (L^-1)'  solve_triangular on the identity                  (:136-138)
                                                  Sigma' = Hermitian(U U')                                                            (:139)
                                              U is the reference's UPPER-triangular scale
    lower_scale(S', dtype)                    the library's scale: S' = Lr' Lr with Lr lower triangular (the Cholesky factorisation of the
                                              index-reversed matrix), C' = Lr^-1 -- lower triangular, positive diagonal, C' C'' = S'^-1, hence
                                              the lower Cholesky factor of Sigma'
    entropy(C, dtype)                         d/2 (1 + log 2 pi) + sum log C_ii (src/families/location_scale.jl:52-57; U and C' share it only up
                                              to rounding -- the device reports the one of C')
    steps(q, tgt, draws, eta, second_order, ensure_posdef)
                                              iterations of :95-153 in float64 on oracle.gaussian_expectation_gradient_and_hessian[_order2] with
                                              q' = (m', lower_scale(S')), the state (S, Sigma) carried from step to step

np.float64 is the reference result; np.float32 is the same arithmetic on float32 arrays, the yardstick an f32 context is held against
(tests/solve_ref.block_ratios)."""
import zlib

import numpy as np
from scipy.linalg import cholesky, solve_triangular

from oracle import oracle as O
from tests import solve_ref as SR

LOG2PI = float(np.log(2.0 * np.pi))


def hermitian(A):
    A = np.asarray(A)
    return np.triu(A) + np.triu(A, 1).T


def init_state(C, dtype=np.float64):
    dt = np.dtype(dtype).type
    C = np.tril(np.asarray(C)).astype(dt)
    d = C.shape[0]
    Sigma = hermitian((C @ C.T).astype(dt))
    Cinv = solve_triangular(C, np.eye(d, dtype=dt), lower=True, check_finite=False).astype(dt)
    S = hermitian((Cinv.T @ Cinv).astype(dt))
    return S, Sigma


def update(m, S, Sigma, g, H, eta, ensure_posdef=True, dtype=np.float64):
    dt = np.dtype(dtype).type
    m, g = np.asarray(m).astype(dt), np.asarray(g).astype(dt)
    S, Sigma, H = np.asarray(S).astype(dt), np.asarray(Sigma).astype(dt), np.asarray(H).astype(dt)
    d = m.shape[0]
    eta = dt(eta)
    if ensure_posdef:
        Gh = (S - (-H)).astype(dt)
        S_new = hermitian(((S - eta * Gh) + (((eta * eta / dt(2)) * Gh) @ Sigma) @ Gh).astype(dt))
    else:
        S_new = hermitian(((dt(1) - eta) * S + eta * (-H)).astype(dt))
    L = cholesky(S_new, lower=True, check_finite=False).astype(dt)   # raises numpy.linalg.LinAlgError where the reference throws PosDefException
    y = solve_triangular(L, -g, lower=True, check_finite=False).astype(dt)
    x = solve_triangular(L, y, lower=True, trans="T", check_finite=False).astype(dt)
    m_new = (m - eta * x).astype(dt)
    U = solve_triangular(L, np.eye(d, dtype=dt), lower=True, check_finite=False).astype(dt).T
    Sigma_new = hermitian((U @ U.T).astype(dt))
    return m_new, S_new, Sigma_new, U


def lower_scale(S_new, dtype=np.float64):
    dt = np.dtype(dtype).type
    S_new = np.asarray(S_new).astype(dt)
    d = S_new.shape[0]
    Lr = cholesky(S_new[::-1, ::-1], lower=True, check_finite=False).astype(dt)[::-1, ::-1].T   # S' = Lr' Lr, Lr lower triangular
    return np.tril(solve_triangular(np.ascontiguousarray(Lr), np.eye(d, dtype=dt), lower=True, check_finite=False)).astype(dt)


def entropy(C, dtype=np.float64):
    dt = np.dtype(dtype).type
    d = np.asarray(C).shape[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        return dt(dt(d * 0.5 * (1.0 + LOG2PI)) + np.sum(np.log(np.diag(np.asarray(C).astype(dt))), dtype=dt))


def state_flat(S, Sigma):
    """[S; Sigma] as the device holds it: both d x d column-major."""
    return np.concatenate([np.asarray(S).reshape(-1, order="F"), np.asarray(Sigma).reshape(-1, order="F")])


def steps(q, tgt, draws, eta, second_order, ensure_posdef=True, n_steps=None):
    """Iterations of `step` in float64.  draws: a list of d x n matrices (one per iteration) or a callable q -> d x n matrix.
    Returns (q_final, (S, Sigma), [elbo_t])."""
    est = O.gaussian_expectation_gradient_and_hessian_order2 if second_order else O.gaussian_expectation_gradient_and_hessian
    n_steps = len(draws) if n_steps is None else n_steps
    S, Sigma = init_state(q.scale)
    elbos = []
    for t in range(n_steps):
        u = draws(q) if callable(draws) else draws[t]
        logpi, g, H = est(q, tgt, np.asarray(u, dtype=np.float64))
        m_new, S, Sigma, _ = update(q.location, S, Sigma, g, H, eta, ensure_posdef, np.float64)
        C_new = lower_scale(S)
        q = O.MvLocationScale(m_new, C_new)
        elbos.append(float(logpi + entropy(C_new)))
    return q, (S, Sigma), elbos


def emulate_tiles(m, S, Sigma, g, H, eta, ensure_posdef=True, dtype=np.float32, tile=64):
    """What csrc/kernels_natgrad.hip's tile path is DOCUMENTED to do, in `dtype` numpy (no code of the kernels): S' from W = Sigma Gh and
    Gh W, upper triangle mirrored, padded with the identity; S' = Lr' Lr by 64-row panels from the last one, each panel's diagonal tile
    factored and inverted (Dinv_k) and the rest of the panel formed as a product with that inverse; C' = Lr^-1 block row by block row from
    the products M_ik = Dinv_i Lr_ik; Sigma' = C' C''; m' = m - eta x with x = C' C'' (-g) refined once (r = -g - S' x, x += C' C'' r), the
    matrix-vector sums in float64.  Returns (m', S', Sigma', C')."""
    dt = np.dtype(dtype).type
    m, g = np.asarray(m).astype(dt), np.asarray(g).astype(dt)
    S, Sigma, H = np.asarray(S).astype(dt), np.asarray(Sigma).astype(dt), np.asarray(H).astype(dt)
    d = m.shape[0]
    eta = dt(eta)
    if ensure_posdef:
        Gh = (S + H).astype(dt)
        W = (Sigma @ Gh).astype(dt)
        S_new = hermitian(((S - eta * Gh) + (eta * eta / dt(2)) * (Gh @ W).astype(dt)).astype(dt))
    else:
        S_new = hermitian(((dt(1) - eta) * S - eta * H).astype(dt))
    nT = (d + tile - 1) // tile
    n = nT * tile
    A = np.eye(n, dtype=dt)
    A[:d, :d] = S_new
    blk = lambda M, i, j: M[i * tile:(i + 1) * tile, j * tile:(j + 1) * tile]
    Lr, Dinv = np.zeros((n, n), dt), [None] * nT
    for k in range(nT - 1, -1, -1):
        for j in range(k + 1):
            acc = np.zeros((tile, tile), dt)
            for i in range(k + 1, nT):
                acc = (acc + blk(Lr, i, k).T @ blk(Lr, i, j)).astype(dt)
            blk(Lr, k, j)[:] = blk(A, k, j) - acc
        U = np.tril(blk(Lr, k, k))
        U = U + np.tril(U, -1).T
        Lkk = np.ascontiguousarray(cholesky(U[::-1, ::-1], lower=True, check_finite=False).astype(dt)[::-1, ::-1].T)
        Dinv[k] = np.tril(solve_triangular(Lkk, np.eye(tile, dtype=dt), lower=True, check_finite=False)).astype(dt)
        blk(Lr, k, k)[:] = Lkk
        for j in range(k):
            blk(Lr, k, j)[:] = (Dinv[k].T @ blk(Lr, k, j)).astype(dt)
    X = np.zeros((n, n), dt)
    for i in range(nT):
        blk(X, i, i)[:] = Dinv[i]
        for j in range(i):
            acc = np.zeros((tile, tile), dt)
            for k in range(j, i):
                acc = (acc + (Dinv[i] @ blk(Lr, i, k)).astype(dt) @ blk(X, k, j)).astype(dt)
            blk(X, i, j)[:] = -acc
    C_new = X[:d, :d]
    Sig = np.tril((C_new @ C_new.T).astype(dt))
    Sigma_new = Sig + np.tril(Sig, -1).T
    C64, g64 = C_new.astype(np.float64), g.astype(np.float64)
    x = C64 @ (C64.T @ (-g64))
    x = x + C64 @ (C64.T @ (-g64 - S_new.astype(np.float64) @ x))
    m_new = (m - eta * x.astype(dt)).astype(dt)
    return m_new, S_new, Sigma_new, C_new


def congruent_hessian(C, rng, symmetric=False):
    """H = -C^-T (I + 0.3 N / sqrt(d)) C^-1 in float64: a perturbation congruent with the precision, which keeps the upper-mirrored S'
    positive definite where an additive one does not."""
    C = np.tril(np.asarray(C, dtype=np.float64))
    d = C.shape[0]
    N = rng.normal(size=(d, d))
    if symmetric:
        N = 0.5 * (N + N.T)
    Ci = solve_triangular(C, np.eye(d), lower=True, check_finite=False)
    return -(Ci.T @ (np.eye(d) + 0.3 * N / np.sqrt(d)) @ Ci)


def conditioning_case(kind, d, dtype=np.float32):
    """(m, C, g, H) of the conditioning classes (tests/solve_ref.scale_matrix): spd2 / spd4 / ar999 take a symmetric H (with a non-symmetric one
    the upper-mirrored S' of these classes is not positive definite and the reference itself throws)."""
    rng = np.random.default_rng(zlib.crc32(kind.encode()) + d)
    C = SR.scale_matrix(kind, d, rng).astype(dtype)
    m, g = rng.normal(size=d).astype(dtype), rng.normal(size=d).astype(dtype)
    H = congruent_hessian(C, rng, symmetric=kind in ("spd2", "spd4", "ar999")).astype(dtype)
    return m, C, g, H


class SubsampledNormals:
    """test/models/subsamplednormals.jl restated as a plugin target: 1-d, a sum of unit-variance normals, the likelihood rescaled by
    n_data / n on subsampling; its posterior is N(mean(mus), 1 / n_data)."""

    def __init__(self, mus, likeadj=1.0, order=1):
        self.mus, self.likeadj, self.order = np.asarray(mus, dtype=np.float64), float(likeadj), int(order)

    def dimension(self):
        return 1

    def capabilities(self):
        import advancedvi_jl_amd as avi
        return avi.LogDensityOrder(self.order)

    def logdensity_and_gradient(self, x):
        r = float(x[0]) - self.mus
        return self.likeadj * float(np.sum(-0.5 * r * r - 0.5 * np.log(2 * np.pi))), np.array([-self.likeadj * np.sum(r)])

    def subsample(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        return SubsampledNormals(self.mus[idx], self.mus.size / idx.size, self.order)
