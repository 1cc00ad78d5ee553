"""numpy restatement of KLMinSqrtNaturalGradDescent's update (src/algorithms/klminsqrtnaturalgraddescent.jl:108-119) and of a loop of its
steps on the oracle's estimators -- a helper of tests/test_ngd_ref_host.py and tests/test_gpu_sqrt_ngd.py, not a test.

    update(m, C, g, H, eta, dtype)      the four lines of `step`, every operation rounded to `dtype`:
                                            A  = C' * (-H) * C - I                        (:108, evaluated left to right like Julia)
                                            T  = LowerTriangular(tril(A) - Diagonal(diag(A)) / 2)   (:109)
                                            m' = m - eta * C * (C' * -g)                  (:111)
                                            C' = C - eta * C * T                          (:112)
                                        and entropy(q') = d/2 (1 + log 2 pi) + sum log C'_ii (src/families/location_scale.jl:52-57)
    steps(q, tgt, draws, eta, second)   iterations of :79-127 in float64 on oracle.gaussian_expectation_gradient_and_hessian[_order2], one
                                        d x n matrix of standard-normal draws per iteration (a list, or a callable of the current q)

np.float64 is the reference result; np.float32 is the same arithmetic on float32 arrays, the yardstick an f32 context is held against
(tests/solve_ref.block_ratios)."""
import numpy as np

from oracle import oracle as O

LOG2PI = float(np.log(2.0 * np.pi))


def update(m, C, g, H, eta, dtype=np.float64):
    """(m', C', entropy(q')) of one update in `dtype`.  H is used as it comes: not symmetrised, not transposed."""
    dt = np.dtype(dtype).type
    m, g = np.asarray(m).astype(dt), np.asarray(g).astype(dt)
    C, H = np.tril(np.asarray(C)).astype(dt), np.asarray(H).astype(dt)
    d = m.shape[0]
    eta = dt(eta)
    A = ((C.T @ (-H)) @ C - np.eye(d, dtype=dt)).astype(dt)
    T = (np.tril(A) - np.diag(np.diag(A)) / dt(2)).astype(dt)
    m_new = (m - eta * (C @ (C.T @ (-g)))).astype(dt)
    C_new = np.tril(C - eta * (C @ T)).astype(dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        entropy = dt(d * 0.5 * (1.0 + LOG2PI)) + np.sum(np.log(np.diag(C_new)), dtype=dt)
    return m_new, C_new, dt(entropy)


def update_flat(params, g, H, eta, dtype=np.float64):
    """The same on the flat parameter vector [m; vec(C)] (column-major): (params', entropy(q'))."""
    p = np.asarray(params)
    d = np.asarray(g).shape[0]
    m_new, C_new, ent = update(p[:d], p[d:].reshape(d, d, order="F"), g, H, eta, dtype)
    return np.concatenate([m_new, C_new.reshape(-1, order="F")]), ent


def steps(q, tgt, draws, eta, second_order, n_steps=None):
    """Iterations of `step` in float64.  draws: a list of d x n matrices (one per iteration) or a callable q -> d x n matrix.
    Returns (q_final, [elbo_t])."""
    est = O.gaussian_expectation_gradient_and_hessian_order2 if second_order else O.gaussian_expectation_gradient_and_hessian
    n_steps = len(draws) if n_steps is None else n_steps
    elbos = []
    for t in range(n_steps):
        u = draws(q) if callable(draws) else draws[t]
        logpi, g, H = est(q, tgt, np.asarray(u, dtype=np.float64))
        m_new, C_new, ent = update(q.location, q.scale, g, H, eta, np.float64)
        q = O.MvLocationScale(m_new, C_new)
        elbos.append(float(logpi + ent))
    return q, elbos
