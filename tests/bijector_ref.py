"""numpy restatement of the extended Stacked bijector (mivi_set_bijector_stacked_ex: identity / exp / truncated(lb, ub) / ordered blocks)
around any oracle target -- a helper of tests/test_bijector_ref_host.py and tests/test_gpu_bijector_kinds.py, not a test.
oracle.StackedBijectorTarget knows identity / exp only, so the new kinds are restated here.

eta is the unconstrained coordinate the family draws, x = binv(eta) what the target sees, ladj = logabsdetjac(binv, eta) per sample,
g = grad_x log pi(x):
    exp                 x = e^eta                      ladj = eta                                     d/d eta = e^eta g + 1
    truncated(lb, ub)   x = lb + (ub - lb) sigma(eta)  ladj = log(ub - lb) - |eta| - 2 log1p(e^-|eta|)  d/d eta = (ub - lb) s (1 - s) g + (1 - 2 s)
    truncated(lb, inf)  x = lb + e^eta                 ladj = eta                                     d/d eta = e^eta g + 1
    truncated(-inf, ub) x = ub - e^eta                 ladj = eta                                     d/d eta = -e^eta g + 1
    ordered [b, e)      x_b = eta_b, x_k = x_{k-1} + e^eta_k   ladj = sum_{k>b} eta_k   d/d eta_b = S_b, d/d eta_k = e^eta_k S_k + 1,  S_k = sum_{j>=k} g_j

Every function takes `dtype`: np.float64 is the reference result, np.float32 the same arithmetic at the precision of an f32 context
(every intermediate rounded to float32; e^eta and sigma(eta) taken from eta, never from differences of x) -- the yardstick the GPU
parity tests hold the f32 library against.  The inner target is evaluated in float64 at the samples as `dtype` holds them and rounded
(tests/basedist_ref.py target_eval: the diagonal Gaussian in `dtype` arithmetic)."""
import numpy as np

from oracle import oracle as O
from tests import basedist_ref as B

LOG2PI = float(np.log(2.0 * np.pi))
KINDS = ("identity", "exp", "truncated", "ordered")


def layout(d):
    """The block layouts of the tests (d in 5, 37, 300).  Coordinate 0 is lower-bounded above zero (the constrained funnel's scale).
    d >= 37: the three bound cases, an exp block, two ADJACENT ordered blocks, ordered blocks of length 1 and 2, a truncated(-inf, inf)
    block and uncovered coordinates; d = 300 adds an ordered block that straddles row 256 (the forward scan's carry) and one that
    straddles rows 43 | 44 with another ordered block ending right in front of it (the mirrored backward scan's carry, and no leak into
    the neighbour)."""
    if d < 37:
        return [(0, 1, "truncated", (0.25, np.inf)), (1, 3, "ordered"), (3, 4, "truncated", (-1.0, 2.0))]
    blocks = [(0, 1, "truncated", (0.25, np.inf)), (1, 3, "truncated", (-np.inf, 1.5)), (3, 6, "ordered"), (6, 9, "ordered"),
              (9, 12, "truncated", (-1.0, 2.0)), (12, 14, "exp"), (14, 15, "ordered"), (15, 17, "ordered"),
              (17, 20, "truncated", (-np.inf, np.inf)), (20, 22, "identity")]
    if d >= 300:   # the backward pass walks the column from its last row: ITS chunk boundary lies between rows 44 and 43
        blocks += [(36, 40, "ordered"), (40, 48, "ordered"), (250, 270, "ordered"), (280, 290, "truncated", (-3.0, -1.0))]
    return blocks


def cancellation_case(which, dtype=np.float64):
    """(d, blocks, mean-field location, scale, diagonal-Gaussian target mean, std) of the two inputs on which a backward pass that
    differences the stored x loses the Jacobian factor in float32:
        "lower"    truncated(1000, inf) on [0, 4), eta ~ N(-5, 1): x - lb = e^eta ~ 7e-3 next to ulp(1000) = 6e-5
        "ordered"  an ordered block [0, 5) with x_0 ~ 100 and eta_k ~ N(-6, 0.5): x_k - x_{k-1} ~ 2.5e-3 next to ulp(100) = 7.6e-6
    The targets are wide (std 1) and ten units away, so g ~ +-10 is insensitive to the rounding of x itself."""
    if which == "lower":
        d, blocks = 5, [(0, 4, "truncated", (1000.0, np.inf))]
        loc, scale = np.array([-5.0, -5.2, -4.8, -5.1, 0.3]), np.array([1.0, 1.0, 1.0, 1.0, 0.7])
        mean, std = np.array([1010.0, 1010.0, 1010.0, 1010.0, 0.0]), np.ones(5)
    elif which == "ordered":
        d, blocks = 6, [(0, 5, "ordered")]
        loc, scale = np.array([100.0, -6.0, -6.1, -5.9, -6.0, 0.3]), np.array([0.5, 0.5, 0.5, 0.5, 0.5, 0.7])
        mean, std = np.array([90.0, 90.0, 90.0, 90.0, 90.0, 0.0]), np.ones(6)
    else:
        raise ValueError(which)
    return d, blocks, loc.astype(dtype), scale.astype(dtype), mean.astype(dtype), std.astype(dtype)


def normalise(blocks):
    """[(lo, hi, kind, (lb, ub))] with the bounds of a block that has none set to (-inf, inf)"""
    out = []
    for blk in blocks:
        lo, hi, kind = int(blk[0]), int(blk[1]), blk[2]
        if kind not in KINDS:
            raise ValueError(kind)
        lb, ub = (float(blk[3][0]), float(blk[3][1])) if kind == "truncated" else (-np.inf, np.inf)
        out.append((lo, hi, kind, (lb, ub)))
    return out


def _sigmoid_parts(h):
    """(p, t): t = e^-|eta|, p = t / (1 + t) = min(sigma, 1 - sigma) -- no saturated difference anywhere"""
    t = np.exp(-np.abs(h))
    return t / (h.dtype.type(1) + t), t


def forward(blocks, eta, dtype=np.float64):
    """(x (d x M), ladj (M)) for the columns of eta"""
    dt = np.dtype(dtype).type
    h = np.asarray(eta).astype(dt)
    x, ladj = h.copy(), np.zeros(h.shape[1], dtype=dt)
    for lo, hi, kind, (lb, ub) in normalise(blocks):
        e = h[lo:hi]
        if kind == "exp" or (kind == "truncated" and np.isfinite(lb) and not np.isfinite(ub)):
            x[lo:hi] = (dt(lb) if kind == "truncated" else dt(0)) + np.exp(e)
            ladj = ladj + np.sum(e, axis=0, dtype=dt)
        elif kind == "truncated" and np.isfinite(ub) and not np.isfinite(lb):
            x[lo:hi] = dt(ub) - np.exp(e)
            ladj = ladj + np.sum(e, axis=0, dtype=dt)
        elif kind == "truncated" and np.isfinite(lb):
            w = dt(ub) - dt(lb)
            p, t = _sigmoid_parts(e)
            x[lo:hi] = np.where(e >= 0, dt(ub) - w * p, dt(lb) + w * p)
            ladj = ladj + np.sum(np.log(w) - np.abs(e) - dt(2) * np.log1p(t), axis=0, dtype=dt)
        elif kind == "ordered" and hi - lo >= 2:
            inc = np.concatenate([e[:1], np.exp(e[1:])], axis=0)
            x[lo:hi] = np.cumsum(inc, axis=0, dtype=dt)
            ladj = ladj + np.sum(e[1:], axis=0, dtype=dt)
    return x.astype(dt), ladj.astype(dt)


def backward(blocks, eta, G, dtype=np.float64):
    """J' G + d ladj / d eta for the columns of eta, G = grad_x log pi at x = binv(eta)"""
    dt = np.dtype(dtype).type
    h, g = np.asarray(eta).astype(dt), np.asarray(G).astype(dt)
    out = g.copy()
    for lo, hi, kind, (lb, ub) in normalise(blocks):
        e, gb = h[lo:hi], g[lo:hi]
        if kind == "exp" or (kind == "truncated" and np.isfinite(lb) and not np.isfinite(ub)):
            out[lo:hi] = np.exp(e) * gb + dt(1)
        elif kind == "truncated" and np.isfinite(ub) and not np.isfinite(lb):
            out[lo:hi] = -np.exp(e) * gb + dt(1)
        elif kind == "truncated" and np.isfinite(lb):
            w = dt(ub) - dt(lb)
            p, _ = _sigmoid_parts(e)
            out[lo:hi] = w * p * (dt(1) - p) * gb + np.where(e >= 0, dt(2) * p - dt(1), dt(1) - dt(2) * p)
        elif kind == "ordered" and hi - lo >= 2:
            S = np.cumsum(gb[::-1], axis=0, dtype=dt)[::-1]
            out[lo:hi] = np.concatenate([S[:1], np.exp(e[1:]) * S[1:] + dt(1)], axis=0)
    return out.astype(dt)


def inverse(blocks, x, dtype=np.float64):
    """(eta = b(x) (d x M), ladj = logabsdetjac(binv, eta) (M), inside (M, bool)) for the columns of x; eta / ladj are meaningless where
    a column lies outside the support"""
    dt = np.dtype(dtype).type
    x = np.asarray(x).astype(dt)
    h, ladj, inside = x.copy(), np.zeros(x.shape[1], dtype=dt), np.ones(x.shape[1], dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for lo, hi, kind, (lb, ub) in normalise(blocks):
            xb = x[lo:hi]
            if kind == "exp" or (kind == "truncated" and np.isfinite(lb) and not np.isfinite(ub)):
                t = xb - (dt(lb) if kind == "truncated" else dt(0))
            elif kind == "truncated" and np.isfinite(ub) and not np.isfinite(lb):
                t = dt(ub) - xb
            elif kind == "truncated" and np.isfinite(lb):
                w = dt(ub) - dt(lb)
                u = (xb - dt(lb)) / w
                inside &= np.all((u > 0) & (u < 1), axis=0)
                lu, l1 = np.log(u), np.log1p(-u)
                h[lo:hi] = lu - l1
                ladj = ladj + np.sum(np.log(w) + lu + l1, axis=0, dtype=dt)
                continue
            elif kind == "ordered" and hi - lo >= 2:
                t = xb[1:] - xb[:-1]
                inside &= np.all(t > 0, axis=0)
                h[lo + 1:hi] = np.log(t)
                ladj = ladj + np.sum(np.log(t), axis=0, dtype=dt)
                continue
            else:
                continue
            inside &= np.all(t > 0, axis=0)
            h[lo:hi] = np.log(t)
            ladj = ladj + np.sum(np.log(t), axis=0, dtype=dt)
    return h.astype(dt), ladj.astype(dt), inside


class BijectorTarget:
    """TransformedLogDensityProblem(inner, binv): logdensity(eta) = logdensity(inner, binv(eta)) + logabsdetjac(binv, eta), the bijector's
    arithmetic in `dtype` -- the drop-in for oracle.StackedBijectorTarget wherever a restatement takes a target object."""

    def __init__(self, inner, blocks, dtype=np.float64):
        self.inner, self.blocks, self.dtype = inner, list(blocks), np.dtype(dtype).type

    def dimension(self):
        return self.inner.dimension()

    def logdensity_and_gradient(self, eta):
        h = np.asarray(eta, dtype=np.float64).reshape(-1, 1)
        x, ladj = forward(self.blocks, h, self.dtype)
        v, g = self.inner.logdensity_and_gradient(x[:, 0].astype(np.float64))
        g = backward(self.blocks, h, np.asarray(g, dtype=np.float64).reshape(-1, 1), self.dtype)
        return float(v) + float(ladj[0]), g[:, 0].astype(np.float64)

    def logdensity(self, eta):
        h = np.asarray(eta, dtype=np.float64).reshape(-1, 1)
        x, ladj = forward(self.blocks, h, self.dtype)
        return float(self.inner.logdensity(x[:, 0].astype(np.float64))) + float(ladj[0])


def target_eval(inner, blocks, Z, dtype=np.float64):
    """(ell (M), G (d x M)) of the transformed problem at the columns of Z (= eta), every array in `dtype`"""
    dt = np.dtype(dtype).type
    x, ladj = forward(blocks, Z, dt)
    ell, G = B.target_eval(inner, x, dt)
    return (ell.astype(dt) + ladj).astype(dt), backward(blocks, Z, G, dt)


def samples(params, d, family, eps, dtype=np.float64):
    """rand(rng, q, M) on the draws eps (location_scale.jl:71-87), in `dtype`"""
    dt = np.dtype(dtype).type
    p, E = np.asarray(params).astype(dt), np.asarray(eps).astype(dt)
    m, S = B.split(p, d, family)
    return ((S[:, None] * E if family == O.MEANFIELD else S @ E) + m[:, None]).astype(dt)


def estimate_gradient(params, d, family, inner, blocks, eps, ent, dtype=np.float64):
    """dict(value, grad, Z, X) of oracle.estimate_gradient(params, d, family, <inner under the bijector>, eps, ent) with a normal base,
    every array in `dtype` (oracle/oracle.py estimate_gradient; float32: the back substitution of tests/basedist_ref.py)."""
    dt = np.dtype(dtype).type
    p, E = np.asarray(params).astype(dt), np.asarray(eps).astype(dt)
    m, S = B.split(p, d, family)
    M = E.shape[1]
    mf = family == O.MEANFIELD
    Z = samples(p, d, family, E, dt)
    ell, G = target_eval(inner, blocks, Z, dt)
    diag = S if mf else np.diag(S)
    logdet = np.sum(np.log(diag), dtype=dt)
    if ent in (O.ENT_CLOSED_FORM, O.ENT_CLOSED_FORM_ZERO_GRAD):
        entropy = dt(0.5 * d * (1.0 + LOG2PI)) + logdet
    else:
        entropy = np.mean(dt(0.5) * np.sum(E * E, axis=0, dtype=dt), dtype=dt) + dt(0.5 * d * LOG2PI) + logdet
    W = G
    if ent in (O.ENT_STL, O.ENT_STL_ZERO_GRAD):
        if mf:
            W = G + E / S[:, None]
        elif dt is np.float64:
            W = G + np.linalg.solve(S.T, E)
        else:
            W = G + B._back_substitute(S, E)
    direct = dt(B.DIRECT[ent])
    g_m = -np.sum(W, axis=1, dtype=dt) / dt(M)
    if mf:
        grad = np.concatenate([g_m, -np.sum(W * E, axis=1, dtype=dt) / dt(M) - direct / diag])
    else:
        gC = -np.tril(W @ E.T) / dt(M) - direct * np.diag(dt(1.0) / diag)
        grad = np.concatenate([g_m, gC.reshape(-1, order="F")])
    value = -(np.mean(ell, dtype=dt) + entropy)
    x, _ = forward(blocks, Z, dt)
    return dict(value=float(value), grad=grad.astype(np.float64), Z=np.asarray(Z, dtype=np.float64), X=np.asarray(x, dtype=np.float64))


def logpdf_constrained(params, d, family, blocks, X, dtype=np.float64):
    """logpdf(TransformedDistribution(q, binv), x) for the columns of X, Gaussian q: log q(b(x)) - logabsdetjac(binv, b(x)); -inf outside
    the support.  The bijector's arithmetic in `dtype`, log q through tests/scoregrad_ref.py logpdf_cols."""
    from tests import scoregrad_ref as R
    dt = np.dtype(dtype).type
    eta, ladj, inside = inverse(blocks, X, dt)
    lq = R.logpdf_cols(params, d, family, np.where(inside[None, :], eta, dt(0)), dt)
    return np.where(inside, (np.asarray(lq).astype(dt) - ladj).astype(dt), dt(-np.inf))
