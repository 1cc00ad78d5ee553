"""numpy float64 restatement of FisherMinBatchMatch (src/algorithms/fisherminbatchmatch.jl, AdvancedVI.jl v0.7.0): the objective of
rand_batch_match_samples_with_objective! (:81-111), the update of `step` (:143-155) in BOTH forms -- the literal expression with
scipy.linalg.sqrtm of the non-symmetric I + 4 U V, and the rank-B form the device builds (csrc/kernels_bam.hip) -- and whole steps.

    zbar, Cz = mean_and_cov(z)     gbar, Gamma = mean_and_cov(G)     (corrected, 1 / (B - 1))
    U = lambda Gamma + lambda/(1+lambda) gbar gbar'        V = Sigma + lambda Cz + lambda/(1+lambda) (m - zbar)(m - zbar)'
    Sigma' = 2 V (I + sqrt(I + 4 U V))^-1       m' = m/(1+lambda) + lambda/(1+lambda) (Sigma' gbar + zbar)       C' = cholesky(Sigma').L

Rank-B form: alpha = sqrt(lambda/(B-1)), beta = sqrt(lambda/((1+lambda) B)), Q_b = alpha (g_b - gbar) + beta gbar (U = Q Q'),
Zt_b = alpha (z_b - zbar) + beta (zbar - m) (V = Sigma + Zt Zt'), R = V Q, K = Q' V Q = E diag(w) E' (w clamped at 0), a = 1/2 + sqrt(w + 1/4),
Sigma' = V - (R E) diag(a^-2) (R E)'.  Neither form is code under test."""
import numpy as np
from scipy.linalg import sqrtm

LOG2PI = float(np.log(2.0 * np.pi))


def entropy(C):
    d = C.shape[0]
    return 0.5 * d * (1.0 + LOG2PI) + float(np.sum(np.log(np.diag(C))))


def moments(m, C, u, target):
    """(z, G, fisher, logpi_avg) at the draws u (d x B): :89-110."""
    z = C @ u + m[:, None]
    B = u.shape[1]
    G = np.empty_like(z)
    logpi = 0.0
    for b in range(B):
        l, g = target.logdensity_and_gradient(z[:, b])
        G[:, b] = g
        logpi += l
    return z, G, fisher(C, u, G), logpi / B


def fisher(C, u, G):
    return float(np.sum((-u - C.T @ G) ** 2) / u.shape[1])


def _uv(m, Sigma, z, G, lam):
    B = z.shape[1]
    zbar, gbar = z.mean(axis=1), G.mean(axis=1)
    Cz = (z - zbar[:, None]) @ (z - zbar[:, None]).T / (B - 1)
    Gam = (G - gbar[:, None]) @ (G - gbar[:, None]).T / (B - 1)
    mmz = m - zbar
    w = lam / (1 + lam)
    U = lam * Gam + w * np.outer(gbar, gbar)
    V = Sigma + lam * Cz + w * np.outer(mmz, mmz)
    return U, V, zbar, gbar


def _finish(m, Sp, zbar, gbar, lam):
    Sp = (Sp + Sp.T) / 2
    mp = m / (1 + lam) + lam / (1 + lam) * (Sp @ gbar + zbar)
    return mp, np.linalg.cholesky(Sp), Sp


def update_literal(m, Sigma, z, G, lam, dtype=np.float64):
    """(m', C', Sigma') by the reference's own expression (:150-155).  dtype = np.float32: the same expression with every array held in
    float32 (numpy then rounds each operation to float32; the square root is scipy's on the float32 matrix) -- the float32 yardstick."""
    m, Sigma, z, G = (np.asarray(x, dtype=dtype) for x in (m, Sigma, z, G))
    lam = dtype(lam)
    U, V, zbar, gbar = _uv(m, Sigma, z, G, lam)
    d = len(m)
    eye = np.eye(d, dtype=dtype)
    root = np.real(sqrtm(eye + dtype(4.0) * (U @ V))).astype(dtype)
    Sp = dtype(2.0) * V @ np.linalg.inv(eye + root)
    return _finish(m, Sp, zbar, gbar, lam)


def update_lowrank(m, Sigma, z, G, lam):
    """(m', C', Sigma') by the rank-B form."""
    B = z.shape[1]
    zbar, gbar = z.mean(axis=1), G.mean(axis=1)
    al, be = np.sqrt(lam / (B - 1)), np.sqrt(lam / ((1.0 + lam) * B))
    Q = al * (G - gbar[:, None]) + be * gbar[:, None]
    Zt = al * (z - zbar[:, None]) + be * (zbar - m)[:, None]
    M = Zt.T @ Q
    SQ = Sigma @ Q
    R = SQ + Zt @ M
    K = Q.T @ SQ + M.T @ M
    w, E = np.linalg.eigh(0.5 * (K + K.T))
    a = 0.5 + np.sqrt(np.maximum(w, 0.0) + 0.25)
    Y = (R @ E) / a
    Sp = Sigma + Zt @ Zt.T - Y @ Y.T
    return _finish(m, Sp, zbar, gbar, lam)


def step(m, C, Sigma, u, target, iteration, update=update_lowrank, dtype=np.float64):
    """One `step` (:113-167) from the draws u: ((m', C', Sigma'), info) with info at the iterate the step starts from.  dtype: the type
    lambda is converted to (:148) and, float32, the type the new iterate is rounded to."""
    d, B = u.shape
    z, G, f, logpi = moments(m, C, u, target)
    lam = float(dtype(d * B / iteration))
    mp, Cp, Sp = update(m, Sigma, z, G, lam)
    info = dict(iteration=iteration, covweighted_fisher=f, elbo=logpi + entropy(C))
    if dtype != np.float64:
        mp, Cp, Sp = (x.astype(dtype).astype(np.float64) for x in (mp, Cp, Sp))
    return (mp, Cp, Sp), info


def steps(m, C, draws, target, iteration0=1, update=update_lowrank, dtype=np.float64):
    """len(draws) steps from (m, C), Sigma = C C' (:76); returns ((m, C, Sigma), [info])."""
    Sigma, infos = C @ C.T, []
    for t, u in enumerate(draws):
        (m, C, Sigma), info = step(m, C, Sigma, u, target, iteration0 + t, update, dtype)
        infos.append(info)
    return (m, C, Sigma), infos


def random_case(d, B, seed, dtype=np.float64):
    """An iterate (m, C, Sigma = C C'), draws u and RANDOM gradients G (not a target's), stored in dtype and returned in float64."""
    rng = np.random.default_rng(seed)
    m = rng.normal(size=d)
    C = np.tril(rng.normal(size=(d, d)) * (0.3 / np.sqrt(d)))
    C[np.diag_indices(d)] = rng.uniform(0.5, 1.5, size=d)
    u = rng.normal(size=(d, B))
    G = rng.normal(size=(d, B))
    m, C, u, G = (x.astype(dtype).astype(np.float64) for x in (m, C, u, G))
    return m, C, u, G


def discrepancy(m, Sigma, z, G, lam):
    """The relative l2 distances between the two forms' (m', C', Sigma')."""
    a, b = update_literal(m, Sigma, z, G, lam), update_lowrank(m, Sigma, z, G, lam)
    return tuple(float(np.linalg.norm(x - y) / np.linalg.norm(x)) for x, y in zip(a, b))
