"""Reference of the non-normal base distributions of MvLocationScale (Laplace(), TDist(nu); docs/src/families.md:59-101) for the tests,
from the oracle alone (oracle.philox_bits, the oracle's targets): the two draw streams of include/mivi.h, log phi / psi / H(phi), and one
RepGradELBO estimate (value and gradient, both families, all five entropy estimators) in closed form -- in numpy float64 and, as the
yardstick the f32 kernels are held to, with every array in a chosen dtype.

A base is ("laplace", None) or ("t", nu).  Draws `U` are d x M.  Parameters: [m; sigma] (mean-field) or [m; vec C] (full-rank).

The f32 criterion (tests/test_gpu_solve_yardstick.py): |got - ref64| <= F32_FACTOR max(|yard32 - ref64|, 2^-24 |ref64|) in l2, `ratio`."""
import math

import numpy as np
from scipy import special

from oracle import oracle as O

CLOSED_FORM, CLOSED_FORM_ZERO_GRAD, MONTE_CARLO, STL, STL_ZERO_GRAD = range(5)
DIRECT = {CLOSED_FORM: 1.0, CLOSED_FORM_ZERO_GRAD: 0.0, MONTE_CARLO: 1.0, STL: 0.0, STL_ZERO_GRAD: -1.0}
LAPLACE = ("laplace", None)


def tdist(nu):
    return ("t", float(nu))


def base_of(dist):
    """the tuple of a families.Laplace() / families.TDist(nu)"""
    return LAPLACE if dist.code == 1 else tdist(dist.nu)


# ---- the streams ---------------------------------------------------------------------------------------------------------------------
def laplace_from_bits(words, f64=False, dtype=np.float64):
    """words (d x M, uint32) -> draws: sign + if the top bit is set, magnitude -ln v with v = (((w >> 8) & 0x7fffff) + 0.5) 2^-23 (f32
    stream) or ((w & 0x7fffffff) + 0.5) 2^-31 (f64 stream); the uniforms are exact in `dtype`, the logarithm is evaluated in it."""
    w = np.asarray(words, dtype=np.uint32)
    if f64:
        v = ((w & np.uint32(0x7FFFFFFF)).astype(np.float64) + 0.5) * 2.0 ** -31
    else:
        v = (((w >> np.uint32(8)) & np.uint32(0x7FFFFF)).astype(np.float64) + 0.5) * 2.0 ** -23
    mag = -np.log(v.astype(dtype))
    return np.where((w >> np.uint32(31)) != 0, mag, -mag).astype(dtype)


def _uniform(w, f64):
    """Box-Muller's word -> uniform map (oracle.box_muller_from_bits)"""
    w = np.asarray(w, dtype=np.uint32)
    if f64:
        return (w.astype(np.float64) + 0.5) * 2.0 ** -32
    return ((w >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def tdist_parts(words2, nu, f64=False, dtype=np.float64):
    """words2 (2d x M): rows 2i -> U, 2i + 1 -> V.  (a, r, c) of Bailey's polar form T = r c: a = -(2/nu) ln U, r = sqrt(nu expm1(a)),
    c = cos(2 pi V), every operation in `dtype`."""
    u = _uniform(words2[0::2], f64).astype(dtype)
    v = _uniform(words2[1::2], f64).astype(dtype)
    nu_t = dtype(nu)
    a = (dtype(-2.0) / nu_t) * np.log(u)
    r = np.sqrt(nu_t * np.expm1(a))
    c = np.cos(dtype(2.0 * np.pi) * v)
    return a, r, c


def draws(base, seed, idx, d, m_lo, m_hi, f64=False, dtype=np.float64):
    """U[:, m_lo:m_hi] of estimate `idx` (d x (m_hi - m_lo)), evaluated in `dtype` on the stream of an f64 (f64=True) or f32 context."""
    if base[0] == "laplace":
        return laplace_from_bits(O.philox_bits(seed, idx, d, m_lo, m_hi), f64, dtype)
    _, r, c = tdist_parts(O.philox_bits(seed, idx, 2 * d, m_lo, m_hi), base[1], f64, dtype)
    return (r * c).astype(dtype)


def draw_scale(base, seed, idx, d, m_lo, m_hi, f64=False):
    """Per element, what a faithful evaluation's absolute error is proportional to (float64): times a few unit roundoffs it bounds the error
    of the draw.  Laplace: one logarithm -> |x|.  TDist: ln U, the product a = -(2/nu) ln U (three roundings), expm1 (condition number
    <= 1 + a), the product with nu, sqrt (halves), cos (absolute), the final product: |dT| <= r (5.5 + 1.5 a) delta to first order."""
    if base[0] == "laplace":
        return np.abs(draws(base, seed, idx, d, m_lo, m_hi, f64))
    a, r, _ = tdist_parts(O.philox_bits(seed, idx, 2 * d, m_lo, m_hi), base[1], f64)
    return r * (5.5 + 1.5 * a)


# ---- densities -----------------------------------------------------------------------------------------------------------------------
def log_norm(base):
    """the constant of log phi"""
    if base[0] == "laplace":
        return -math.log(2.0)
    nu = base[1]
    return float(special.gammaln(0.5 * (nu + 1.0)) - special.gammaln(0.5 * nu) - 0.5 * math.log(nu * math.pi))


def logphi(base, x):
    x = np.asarray(x)
    dt = x.dtype.type
    if base[0] == "laplace":
        return -np.abs(x) - dt(math.log(2.0))
    nu = dt(base[1])
    return dt(log_norm(base)) - dt(0.5) * (nu + dt(1.0)) * np.log1p(x * x / nu)


def psi(base, x):
    """(log phi)'"""
    x = np.asarray(x)
    dt = x.dtype.type
    if base[0] == "laplace":
        return -np.sign(x)
    nu = dt(base[1])
    return -(nu + dt(1.0)) * x / (nu + x * x)


def entropy(base):
    """H(phi)"""
    if base[0] == "laplace":
        return 1.0 + math.log(2.0)
    nu = base[1]
    return float(0.5 * (nu + 1.0) * (special.digamma(0.5 * (nu + 1.0)) - special.digamma(0.5 * nu)) + 0.5 * math.log(nu)
                 + special.betaln(0.5 * nu, 0.5))


# ---- one estimate --------------------------------------------------------------------------------------------------------------------
def split(params, d, family):
    """(m, sigma) or (m, C)"""
    if family == O.MEANFIELD:
        return params[:d], params[d:]
    return params[:d], np.tril(params[d:].reshape(d, d, order="F"))


def target_eval(tgt, Z, dtype=np.float64):
    """(ell (M), G (d x M)) at the columns of Z.  dtype float32: the diagonal Gaussian in float32 arithmetic; any other target in float64 at
    the float32 samples, rounded -- the yardstick then carries the rounding of Z and of everything downstream."""
    if dtype != np.float64 and isinstance(tgt, O.DiagNormalTarget):
        mean, std = tgt.mean.astype(dtype), tgt.std.astype(dtype)
        r = (Z - mean[:, None]) / std[:, None]
        ell = dtype(-0.5) * np.sum(r * r, axis=0) - np.sum(np.log(std)) - dtype(0.5 * len(mean) * O.LOG2PI)
        return ell.astype(dtype), (-r / std[:, None]).astype(dtype)
    Z64 = np.asarray(Z, dtype=np.float64)
    cols = [tgt.logdensity_and_gradient(Z64[:, k].copy()) for k in range(Z64.shape[1])]
    return np.array([c[0] for c in cols]).astype(dtype), np.stack([c[1] for c in cols], axis=1).astype(dtype)


def estimate_gradient(params, d, family, tgt, U, kind, base, dtype=np.float64):
    """dict(value, grad, Z) of estimate_gradient! (repgradelbo.jl:151-177) with the base phi, in closed form (families.md:31-39: the
    entropy of a location-scale family is d H(phi) + log|C|):
        W = G (+ C^-T (-psi(U)) for the sticking-the-landing estimators);  dm = -mean W;  dC = -tril(W U') / M - c_H diag(1 / C_ii)
        value = -(mean ell + d H(phi) + sum log C_ii)  (closed form)  or  -(mean ell - mean sum log phi(u) + sum log C_ii)
    with every array in `dtype`."""
    p = np.asarray(params).astype(dtype)
    U = np.asarray(U).astype(dtype)
    m, S = split(p, d, family)
    M = U.shape[1]
    mf = family == O.MEANFIELD
    Z = (S[:, None] * U if mf else S @ U) + m[:, None]
    ell, G = target_eval(tgt, Z, dtype)
    diag = S if mf else np.diag(S)
    logdet = np.sum(np.log(diag))
    if kind in (CLOSED_FORM, CLOSED_FORM_ZERO_GRAD):
        ent = dtype(d * entropy(base)) + logdet
    else:
        ent = np.mean(np.sum(-logphi(base, U), axis=0)) + logdet
    W = G
    if kind in (STL, STL_ZERO_GRAD):
        rhs = -psi(base, U)
        if mf:
            W = G + rhs / S[:, None]
        elif dtype == np.float64:
            W = G + np.linalg.solve(S.T, rhs)
        else:
            W = G + _back_substitute(S, rhs)
    g_m = -np.sum(W, axis=1) / dtype(M)
    if mf:
        g_s = -np.sum(W * U, axis=1) / dtype(M) - dtype(DIRECT[kind]) / diag
        grad = np.concatenate([g_m, g_s])
    else:
        gC = -np.tril(W @ U.T) / dtype(M) - dtype(DIRECT[kind]) * np.diag(dtype(1.0) / diag)
        grad = np.concatenate([g_m, gC.reshape(-1, order="F")])
    value = -(np.mean(ell) + ent)
    return dict(value=float(value), grad=grad.astype(np.float64), Z=np.asarray(Z, dtype=np.float64))


def _back_substitute(C, B):
    """C^-T B by back substitution in C's dtype (row by row from the bottom: what a solve in that precision does)"""
    d = C.shape[0]
    X = np.zeros_like(B)
    for i in range(d - 1, -1, -1):
        X[i] = (B[i] - C[i + 1:, i] @ X[i + 1:]) / C[i, i]
    return X


def ratio(got, yard, ref):
    """|got - ref| / max(|yard - ref|, 2^-24 |ref|)  (tests/solve_ref.py: the floor keeps a lucky yardstick from tightening the bound)"""
    got, yard, ref = (np.asarray(a, dtype=np.float64).ravel() for a in (got, yard, ref))
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(yard - ref), 2.0 ** -24 * np.linalg.norm(ref), np.finfo(np.float64).tiny))
