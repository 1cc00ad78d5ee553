"""numpy restatement of everything that sits on the triangular solve C^T X = R of the full-rank family -- a helper of the solve
yardstick tests (tests/test_solve_ref_host.py, tests/test_gpu_solve_yardstick.py, tests/test_gpu_stein.py), not a test.

    scale_matrix                 the classes of lower-triangular scale matrices C the solves are held on
    stl_gradient                 oracle.estimate_gradient (oracle/oracle.py:496-541) for the full-rank family and the diagonal-Gaussian
                                 target, in closed form and vectorised over the samples
    stein_hessian                oracle.gaussian_expectation_gradient_and_hessian (oracle/oracle.py:447-467)
    logreg_hessian_order2        the sample average of LogRegTarget.logdensity_gradient_and_hessian (oracle/oracle.py:251-264)
    emulate_block_inverse_solve  what csrc/kernels_stl.hip / csrc/stl_dinv.h (64 x 64 blocks) and k_stl_prep + k_stl_solve_la16
                                 (32 x 32 blocks) are DOCUMENTED to do, in float32 numpy; no code of the kernels
    emulate_engine_solve         the batch engine's C^-T planes (csrc/fr_planes.h): two-way f16 splits, three products
    block_ratios                 the criterion: distance to the float64 result relative to the float32 yardstick's, whole and per 64-row block

Every function of the first group takes `dtype`, like tests/scoregrad_ref.py: np.float64 is the reference result, np.float32 the same
arithmetic rounded to float32 at every step (the solve then is LAPACK's substitution, scipy.linalg.solve_triangular on float32 arrays)
-- the yardstick an f32 context is held against."""
import numpy as np
from scipy.linalg import solve_triangular

from oracle import oracle as O

LOG2PI = float(np.log(2.0 * np.pi))
KINDS = ("default", "spd2", "spd4", "ar999", "graded")
F32_FLOOR = 2.0 ** -24     # output rounding of an f32 result: the yardstick's distance is never taken smaller than this x |ref|
DIRECT = {O.ENT_CLOSED_FORM: 1.0, O.ENT_CLOSED_FORM_ZERO_GRAD: 0.0, O.ENT_MONTE_CARLO: 1.0, O.ENT_STL: 0.0, O.ENT_STL_ZERO_GRAD: -1.0}


# ---- the classes of scale matrices -----------------------------------------------------------------------------------------------------
def _default(d, rng):
    """tests/helpers.py make_family's C: diagonal in [0.5, 1.5], off-diagonal N(0, 0.3^2 / d); kappa_2 about 4."""
    C = np.tril(rng.normal(size=(d, d)) * (0.3 / np.sqrt(d)))
    C[np.diag_indices(d)] = rng.uniform(0.5, 1.5, size=d)
    return C


def scale_matrix(kind, d, rng):
    """A lower-triangular float64 C of class `kind` (the caller casts it to the context's dtype).
        default   make_family's                                                                   kappa_2(C) about 4
        spd2/4    chol(Q diag(lambda) Q'), Q from the QR of a normal matrix, lambda log-spaced in
                  [1e-4, 1] / [1e-8, 1]: what a converged fit to a correlated target holds          kappa_2(C) = 1e2 / 1e4
        ar999     chol(rho^|i - j|), rho = 0.999                                                    kappa_2(C) <= (1 + rho) / (1 - rho)
        graded    diag(10^U(-3, 3)) default: rows spanning six decades"""
    if kind == "default":
        return _default(d, rng)
    if kind in ("spd2", "spd4"):
        Q, _ = np.linalg.qr(rng.normal(size=(d, d)))
        lam = np.logspace(-4.0 if kind == "spd2" else -8.0, 0.0, d)
        S = (Q * lam) @ Q.T
        return np.linalg.cholesky(0.5 * (S + S.T))
    if kind == "ar999":
        i = np.arange(d)
        return np.linalg.cholesky(0.999 ** np.abs(i[:, None] - i[None, :]))
    if kind == "graded":
        return (10.0 ** rng.uniform(-3.0, 3.0, size=d))[:, None] * _default(d, rng)
    raise ValueError(kind)


# ---- the three public results, in `dtype` ------------------------------------------------------------------------------------------------
def _split(params, d, dtype):
    p = np.asarray(params, dtype=np.float64)
    return p[:d].astype(dtype), np.tril(p[d:].reshape(d, d, order="F")).astype(dtype)


def _diag_target(tgt, Z, dtype):
    """(log pi(z_m), grad log pi(z_m)) of oracle.DiagNormalTarget for the columns of Z, in `dtype`."""
    m, s = tgt.mean.astype(dtype), tgt.std.astype(dtype)
    R = (Z - m[:, None]) / s[:, None]
    ell = -dtype(0.5) * np.sum(R * R, axis=0, dtype=dtype) - np.sum(np.log(s), dtype=dtype) - dtype(0.5 * Z.shape[0] * LOG2PI)
    return ell.astype(dtype), (-(R / s[:, None])).astype(dtype)


def solve_ct(C, R):
    """X of C^T X = R by substitution (LAPACK trtrs in the arrays' own precision)."""
    return solve_triangular(C, R, trans="T", lower=True, check_finite=False)


def stl_gradient(params, d, tgt, eps, ent, dtype=np.float64):
    """dict(value, grad, X) of oracle.estimate_gradient(params, d, FULLRANK, tgt, eps, ent) for a DiagNormalTarget, with X = C^-T eps."""
    dtype = np.dtype(dtype).type
    mu, C = _split(params, d, dtype)
    E = np.asarray(eps).astype(dtype)
    M = E.shape[1]
    Z = C @ E + mu[:, None]
    ell, G = _diag_target(tgt, Z, dtype)
    diag = np.diag(C)
    logdet = np.sum(np.log(diag), dtype=dtype)
    if ent in (O.ENT_CLOSED_FORM, O.ENT_CLOSED_FORM_ZERO_GRAD):
        entropy = dtype(d * 0.5 * (1.0 + LOG2PI)) + logdet
    else:
        entropy = np.mean(dtype(0.5) * np.sum(E * E, axis=0, dtype=dtype), dtype=dtype) + dtype(0.5 * d * LOG2PI) + logdet
    X = solve_ct(C, E).astype(dtype)
    W = G + X if ent in (O.ENT_STL, O.ENT_STL_ZERO_GRAD) else G
    g_mu = -np.sum(W, axis=1, dtype=dtype) / dtype(M)
    gC = -np.tril(W @ E.T) / dtype(M) - dtype(DIRECT[ent]) * np.diag(dtype(1.0) / diag)
    grad = np.concatenate([g_mu, gC.reshape(-1, order="F")]).astype(dtype)
    return dict(value=dtype(-(np.mean(ell, dtype=dtype) + entropy)), grad=grad, X=X)


def stein_hessian(q, tgt, u, dtype=np.float64):
    """(logpi_avg, grad, hess) of oracle.gaussian_expectation_gradient_and_hessian(q, tgt, u): hess = C^-T (u g' / n).  A DiagNormalTarget
    is evaluated in `dtype`; any other target column by column in float64 and rounded to `dtype`."""
    dtype = np.dtype(dtype).type
    mu, C = q.location.astype(dtype), np.tril(q.scale).astype(dtype)
    U = np.asarray(u).astype(dtype)
    n = U.shape[1]
    Z = C @ U + mu[:, None]
    if isinstance(tgt, O.DiagNormalTarget):
        ell, G = _diag_target(tgt, Z, dtype)
    else:
        vg = [tgt.logdensity_and_gradient(Z[:, b].astype(np.float64)) for b in range(n)]
        ell, G = np.array([v for v, _ in vg]).astype(dtype), np.stack([g for _, g in vg], axis=1).astype(dtype)
    G = G / dtype(n)
    hess = solve_ct(C, (U @ G.T).astype(dtype)).astype(dtype)
    return dtype(np.sum(ell / dtype(n), dtype=dtype)), np.sum(G, axis=1, dtype=dtype), hess


def logreg_hessian_order2(params, d, X, y, variant, likeadj, eps, dtype=np.float64):
    """The (d x d) sample average of oracle.LogRegTarget(X, y, variant, likeadj).logdensity_gradient_and_hessian over z = C eps + mu,
    theta = [beta (p); s]: -likeadj X' diag(mean_m pi (1 - pi)) X - mean(e^-2s) I, the border 2 mean(beta e^-2s), the corner
    mean(-2 beta'beta e^-2s + hyper'').  (y does not enter a logistic regression's Hessian.)"""
    dtype = np.dtype(dtype).type
    mu, C = _split(params, d, dtype)
    E = np.asarray(eps).astype(dtype)
    M, p = E.shape[1], d - 1
    Xd = np.asarray(X).astype(dtype)
    Z = C @ E + mu[:, None]
    B, s = Z[:p], Z[p]
    pi = (dtype(1.0) / (dtype(1.0) + np.exp(-(Xd @ B)))).astype(dtype)
    wbar = np.sum(pi * (dtype(1.0) - pi), axis=1, dtype=dtype) / dtype(M)
    is2 = np.exp(dtype(-2.0) * s).astype(dtype)
    H = np.zeros((d, d), dtype=dtype)
    H[:p, :p] = -dtype(likeadj) * ((Xd.T * wbar) @ Xd) - (np.sum(is2, dtype=dtype) / dtype(M)) * np.eye(p, dtype=dtype)
    H[:p, p] = H[p, :p] = np.sum(dtype(2.0) * B * is2, axis=1, dtype=dtype) / dtype(M)
    if variant == "logsigma_normal":
        hyper = dtype(-2.0 / 9.0) * np.exp(dtype(2.0) * s)
    elif variant == "lognormal_exp_bijector":
        hyper = np.full(M, -1.0 / 9.0, dtype=dtype)
    else:
        raise ValueError(variant)
    H[p, p] = np.sum(dtype(-2.0) * np.sum(B * B, axis=0, dtype=dtype) * is2 + hyper, dtype=dtype) / dtype(M)
    return H


# ---- emulations of the documented algorithms (float32 throughout) ------------------------------------------------------------------------
def truncate_bits(A, keep_bits):
    """float32 A with its significands cut to `keep_bits` significant bits (24: unchanged)."""
    A = np.ascontiguousarray(A, dtype=np.float32)
    if keep_bits >= 24:
        return A
    mask = np.uint32((0xFFFFFFFF << (24 - keep_bits)) & 0xFFFFFFFF)
    return (A.view(np.uint32) & mask).view(np.float32)


def _inverse_by_doubling(L):
    """The inverse of a lower-triangular float32 block: [A 0; C B]^-1 = [A^-1 0; -B^-1 C A^-1  B^-1], halves first."""
    n = L.shape[0]
    if n == 1:
        return (np.float32(1.0) / L).astype(np.float32)
    h = (n + 1) // 2
    A, B = _inverse_by_doubling(L[:h, :h]), _inverse_by_doubling(L[h:, h:])
    out = np.zeros((n, n), dtype=np.float32)
    out[:h, :h], out[h:, h:] = A, B
    out[h:, :h] = -(B @ (L[h:, :h] @ A))
    return out


def _block_back_substitution(C, R, bs, keep_bits):
    d = C.shape[0]
    X = np.zeros_like(R)
    starts = list(range(0, d, bs))
    for lo in reversed(starts):
        hi = min(lo + bs, d)
        Dinv = truncate_bits(_inverse_by_doubling(C[lo:hi, lo:hi]), keep_bits)
        rhs = R[lo:hi] - C[hi:, lo:hi].T @ X[hi:] if hi < d else R[lo:hi]
        X[lo:hi] = Dinv.T @ rhs
    return X


def emulate_block_inverse_solve(C, R, bs, keep_bits=24):
    """X of C^T X = R the way the library's f32 solves are documented to work: the bs x bs diagonal blocks inverted by recursive doubling,
    block back-substitution on the inverses, every product a float32 matrix product.  bs = 64 (csrc/kernels_stl.hip) first takes one level
    of recursion, X2 = C22^-T R2, X1 = Y1 - F^T X2 with Y1 = C11^-T R1 and F^T = C11^-T C21^T formed explicitly; bs = 32 is
    k_stl_prep + k_stl_solve_la16.  keep_bits < 24 truncates the inverted blocks (what losing a plane of their split does)."""
    if bs not in (64, 32):
        raise ValueError(bs)
    C = np.tril(np.asarray(C)).astype(np.float32)
    R = np.asarray(R).astype(np.float32)
    d = C.shape[0]
    if bs == 32 or d % 128:
        return _block_back_substitution(C, R, bs, keep_bits)
    n = d // 2
    X2 = _block_back_substitution(C[n:, n:], R[n:], bs, keep_bits)
    Y1 = _block_back_substitution(C[:n, :n], R[:n], bs, keep_bits)
    Ft = _block_back_substitution(C[:n, :n], np.ascontiguousarray(C[n:, :n].T), bs, keep_bits)
    return np.concatenate([Y1 - Ft @ X2, X2], axis=0)


def _pow2_scale(amax):
    """the power of two s with s amax in [2^13, 2^14) (csrc/fr_planes.h fb_scale_of)"""
    _, e = np.frexp(np.maximum(amax, np.float32(2.0 ** -102)))   # amax in [2^(e-1), 2^e)
    return np.ldexp(np.float32(1.0), 14 - e).astype(np.float32)


def _f16_planes(x):
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float32), lo.astype(np.float32)


def emulate_engine_solve(C, eps):
    """X = C^-T eps the way the batch engine is documented to form it (csrc/fr_planes.h, api_batch.hip): C^-T once per call from the
    block-inverse solve on the identity, each of its rows scaled by a power of two and kept as hi = f16(x), lo = f16(x - hi); eps scaled by
    2^11 and split the same way; the product lo.hi + hi.lo + hi.hi accumulated in float32, then unscaled."""
    d = np.asarray(C).shape[0]
    T = emulate_block_inverse_solve(C, np.eye(d, dtype=np.float32), 64)
    s = _pow2_scale(np.max(np.abs(T), axis=1))
    th, tl = _f16_planes(T * s[:, None])
    eh, el = _f16_planes(np.asarray(eps).astype(np.float32) * np.float32(2048.0))
    acc = tl @ eh + th @ el + th @ eh
    return (acc / s[:, None] * np.float32(1.0 / 2048.0)).astype(np.float32)


def stl_gradient_with_solve(params, d, tgt, eps, ent, X):
    """stl_gradient(dtype = float32) with the solve's result replaced by X: what an emulated solve does to the gradient."""
    mu, C = _split(params, d, np.float32)
    E = np.asarray(eps).astype(np.float32)
    M = E.shape[1]
    _, G = _diag_target(tgt, C @ E + mu[:, None], np.float32)
    W = G + np.asarray(X).astype(np.float32)
    gC = -np.tril(W @ E.T) / np.float32(M) - np.float32(DIRECT[ent]) * np.diag(np.float32(1.0) / np.diag(C))
    return np.concatenate([-np.sum(W, axis=1, dtype=np.float32) / np.float32(M), gC.reshape(-1, order="F")]).astype(np.float32)


# ---- the criterion ------------------------------------------------------------------------------------------------------------------------
def _row_groups(a, d):
    """the d-row matrices of a result: (dmu as d x 1, dC as d x d) of a flat gradient, else the array itself as d x k (column-major if flat)"""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1 and a.size == d + d * d:
        return [a[:d].reshape(d, 1), a[d:].reshape(d, d, order="F")]
    if a.ndim == 1:
        return [a.reshape(d, -1, order="F")]
    assert a.shape[0] == d, a.shape
    return [a]


def _ratio(got, yard, ref):
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(yard - ref), F32_FLOOR * np.linalg.norm(ref), np.finfo(np.float64).tiny))


def block_ratios(got, yard, ref64, d, block=64):
    """(whole, worst block): |got - ref| / max(|yard - ref|, 2^-24 |ref|) over the whole result, and the largest such ratio over the
    `block`-row blocks (a short last block allowed) of every d-row matrix in it -- the rows of dmu and the rows of dC of a gradient, a
    Hessian or a solution as a matrix with d rows.  X grows upward through the back-substitution, so an error confined to one block row
    disappears in the whole-vector norm; the floor keeps a yardstick that happens to be lucky from tightening the bound."""
    g, y, r = _row_groups(got, d), _row_groups(yard, d), _row_groups(ref64, d)
    whole = _ratio(np.concatenate([a.ravel() for a in g]), np.concatenate([a.ravel() for a in y]), np.concatenate([a.ravel() for a in r]))
    worst = 0.0
    for a, b, c in zip(g, y, r):
        for lo in range(0, d, block):
            if np.linalg.norm(c[lo:lo + block]) > 0.0 or np.linalg.norm(a[lo:lo + block]) > 0.0:
                worst = max(worst, _ratio(a[lo:lo + block], b[lo:lo + block], c[lo:lo + block]))
    return whole, worst
