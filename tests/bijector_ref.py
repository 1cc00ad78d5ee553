"""numpy restatement of the extended Stacked bijector (mivi_set_bijector_stacked_ex: identity / exp / truncated(lb, ub) / ordered blocks)
around any oracle target, and the per-entry criterion its kernels are held to (second half: magnitudes, envelope, ratios, layouts with
`stages`, parameter classes) -- a helper of tests/test_bijector_ref_host.py, tests/test_gpu_bijector_kinds.py and
tests/test_gpu_bijector_yardstick.py, not a test.
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


def forward(blocks, eta, dtype=np.float64, acc=None):
    """(x (d x M), ladj (M)) for the columns of eta.  acc: None -- every step in `dtype`; a wider type -- the precisions csrc/kernels_bijector.hip
    documents: e^eta in `dtype` on the exp-like rows, everything else (the bound's addition, the sigmoid, the scan, the sum of ladj) in `acc`
    from the stored eta and rounded to `dtype` once.  The bounds are host doubles: their difference is taken before it is rounded."""
    dt = np.dtype(dtype).type
    wt = dt if acc is None else np.dtype(acc).type
    h = np.asarray(eta).astype(dt)
    hw = h.astype(wt)
    x, ladj = h.copy(), np.zeros(h.shape[1], dtype=wt)
    for lo, hi, kind, (lb, ub) in normalise(blocks):
        e, ew = h[lo:hi], hw[lo:hi]
        if kind == "exp" or (kind == "truncated" and np.isfinite(lb) and not np.isfinite(ub)):
            x[lo:hi] = (wt(lb) if kind == "truncated" else wt(0)) + np.exp(e).astype(wt)
            ladj = ladj + np.sum(ew, axis=0, dtype=wt)
        elif kind == "truncated" and np.isfinite(ub) and not np.isfinite(lb):
            x[lo:hi] = wt(ub) - np.exp(e).astype(wt)
            ladj = ladj + np.sum(ew, axis=0, dtype=wt)
        elif kind == "truncated" and np.isfinite(lb):
            w = wt(ub - lb)
            p, t = _sigmoid_parts(ew)
            x[lo:hi] = np.where(ew >= 0, wt(ub) - w * p, wt(lb) + w * p)
            ladj = ladj + np.sum(np.log(w) - np.abs(ew) - wt(2) * np.log1p(t), axis=0, dtype=wt)
        elif kind == "ordered" and hi - lo >= 2:
            inc = np.concatenate([ew[:1], np.exp(ew[1:])], axis=0)
            x[lo:hi] = np.cumsum(inc, axis=0, dtype=wt)
            ladj = ladj + np.sum(ew[1:], axis=0, dtype=wt)
    return x.astype(dt), ladj.astype(dt)


def backward(blocks, eta, G, dtype=np.float64, acc=None):
    """J' G + d ladj / d eta for the columns of eta, G = grad_x log pi at x = binv(eta); acc as in forward (the exp-like rows: e^eta in
    `dtype`, then one fused multiply-add)"""
    dt = np.dtype(dtype).type
    wt = dt if acc is None else np.dtype(acc).type
    h, g = np.asarray(eta).astype(dt), np.asarray(G).astype(dt)
    hw, gw = h.astype(wt), g.astype(wt)
    out = g.copy()
    for lo, hi, kind, (lb, ub) in normalise(blocks):
        e, ew, gb = h[lo:hi], hw[lo:hi], gw[lo:hi]
        if kind == "exp" or (kind == "truncated" and np.isfinite(lb) and not np.isfinite(ub)):
            out[lo:hi] = np.exp(e).astype(wt) * gb + wt(1)
        elif kind == "truncated" and np.isfinite(ub) and not np.isfinite(lb):
            out[lo:hi] = -np.exp(e).astype(wt) * gb + wt(1)
        elif kind == "truncated" and np.isfinite(lb):
            w = wt(ub - lb)
            p, _ = _sigmoid_parts(ew)
            out[lo:hi] = w * p * (wt(1) - p) * gb + np.where(ew >= 0, wt(2) * p - wt(1), wt(1) - wt(2) * p)
        elif kind == "ordered" and hi - lo >= 2:
            S = np.cumsum(gb[::-1], axis=0, dtype=wt)[::-1]
            out[lo:hi] = np.concatenate([S[:1], np.exp(ew[1:]) * S[1:] + wt(1)], axis=0)
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


def inner_eval(inner, x, dtype):
    """(ell (M), G (d x M)) of a DiagNormalTarget / DenseNormalTarget at the columns of x with EVERY step in `dtype` (np.longdouble too):
    solve_ref._diag_target, product_ref._target -- the inner target of the per-entry criterion (tests/basedist_ref.py target_eval evaluates
    the dense target in float64 whatever `dtype` is, which makes a float32 yardstick of it kinder than float32 arithmetic)."""
    from tests import product_ref as Pr
    return Pr._target(inner, x, np.dtype(dtype).type)


def estimate_gradient(params, d, family, inner, blocks, eps, ent, dtype=np.float64, order=None):
    """dict(value, grad, Z, X) of oracle.estimate_gradient(params, d, family, <inner under the bijector>, eps, ent) with a normal base,
    every array in `dtype` (oracle/oracle.py estimate_gradient; float32: the back substitution of tests/basedist_ref.py).
    With `order` (a permutation of the M sample columns applied before every sum over the samples) or dtype np.longdouble this is
    `gradient` below, the evaluation of the per-entry criterion; without, the yardstick of tests/test_gpu_bijector_kinds.py as it was."""
    dt = np.dtype(dtype).type
    if order is not None or dt is np.longdouble:
        return gradient(params, d, family, inner, blocks, eps, ent, dt, order)
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


def _transformed(inner, blocks, Z, dt, probe=None, mutate=None):
    """(ell + ladj (M), W = J' G + d ladj (d x M)) at the columns of Z with the kernels' documented precisions: the bijector's steps with
    acc = float64 in a float32 evaluation (forward), the inner target by inner_eval, every step in `dt`.
    probe: (ell, G) in place of the inner target's values; mutate: the faults of the host test (gradient)."""
    acc = np.float64 if dt is np.float32 else None
    x, ladj = forward(blocks, Z, dt, acc)
    if mutate and "forward" in mutate:
        x, ladj = mutate["forward"](x.copy(), ladj.copy(), Z)
    if probe is not None:
        ell, Gx = np.asarray(probe[0]).astype(dt), np.asarray(probe[1]).astype(dt)
    else:
        ell, Gx = inner_eval(inner, x, dt)
    W = backward(blocks, Z, Gx, dt, acc)
    if mutate and "backward" in mutate:
        W = mutate["backward"](W.copy(), Z, Gx, x).astype(dt)
    return (ell + ladj).astype(dt), W


def gradient(params, d, family, inner, blocks, eps, ent, dtype=np.float64, order=None, probe=None, mutate=None):
    """dict(value, grad, Z, W), all in `dtype` (np.float32, np.float64 or np.longdouble): the estimate of estimate_gradient as the
    per-entry criterion evaluates it -- _transformed for the target, `order` (a permutation of the sample columns) applied before every sum
    over the samples.  probe: (ell (M), G (d x M)) in place of the inner target's values, what a recording plugin hands back
    (tests/test_gpu_bijector_yardstick.py).  mutate: dict of faults for the host test's teeth: "forward": f(x, ladj, Z) -> (x, ladj),
    "backward": f(W, Z, G, x) -> W."""
    dt = np.dtype(dtype).type
    p, E = np.asarray(params).astype(dt), np.asarray(eps).astype(dt)
    m, S = B.split(p, d, family)
    M = E.shape[1]
    o = np.arange(M) if order is None else np.asarray(order)
    mf = family == O.MEANFIELD
    Z = samples(p, d, family, E, dt)
    ell, G = _transformed(inner, blocks, Z, dt, probe, mutate)
    diag = S if mf else np.diag(S)
    logdet = np.sum(np.log(diag), dtype=dt)
    if ent in (O.ENT_CLOSED_FORM, O.ENT_CLOSED_FORM_ZERO_GRAD):
        entropy = dt(0.5 * d * (1.0 + LOG2PI)) + logdet
    else:
        entropy = np.mean((dt(0.5) * np.sum(E * E, axis=0, dtype=dt))[o], dtype=dt) + dt(0.5 * d * LOG2PI) + logdet
    W = G
    if ent in (O.ENT_STL, O.ENT_STL_ZERO_GRAD):
        W = G + (E / S[:, None] if mf else np.linalg.solve(S.T, E) if dt is np.float64 else B._back_substitute(S, E))
    direct = dt(B.DIRECT[ent])
    Wo, Eo = np.ascontiguousarray(W[:, o]), np.ascontiguousarray(E[:, o])
    g_m = -np.sum(Wo, axis=1, dtype=dt) / dt(M)
    if mf:
        grad = np.concatenate([g_m, -np.sum(Wo * Eo, axis=1, dtype=dt) / dt(M) - direct / diag])
    else:
        grad = np.concatenate([g_m, (-np.tril(Wo @ Eo.T) / dt(M) - direct * np.diag(dt(1.0) / diag)).reshape(-1, order="F")])
    return dict(value=dt(-(np.mean(ell[o], dtype=dt) + entropy)), grad=grad.astype(dt), Z=Z, W=W)


def score_gradient(params, d, family, inner, blocks, eps, dtype=np.float64, order=None):
    """dict(value, elbo, grad) of one ScoreGradELBO estimate (tests/scoregrad_ref.py closed_form) of the target behind the bijector, all in
    `dtype`, log pi(x) + ladj by _transformed, `order` applied before every sum over the samples:
        f = log q - (log pi + ladj),  w = f - mean f,  value = mean w^2 / 2,  elbo = -mean f
        dm = C^-T (E w) / M,  dsigma = (E .* E) w / sigma / M  or  dC = tril(C^-T E diag(w) E') / M"""
    dt = np.dtype(dtype).type
    p, E = np.asarray(params).astype(dt), np.asarray(eps).astype(dt)
    m, S = B.split(p, d, family)
    M = E.shape[1]
    o = np.arange(M) if order is None else np.asarray(order)
    mf = family == O.MEANFIELD
    lp, _ = _transformed(inner, blocks, samples(p, d, family, E, dt), dt)
    diag = S if mf else np.diag(S)
    lq = (-dt(0.5) * np.sum(E * E, axis=0, dtype=dt) - np.sum(np.log(diag), dtype=dt) - dt(0.5 * d * LOG2PI)).astype(dt)
    f = (lq - lp).astype(dt)
    fbar = np.mean(f[o], dtype=dt)
    w = (f - fbar).astype(dt)
    value = np.mean((w * w)[o], dtype=dt) / dt(2)
    Eo, wo = np.ascontiguousarray(E[:, o]), w[o]
    if mf:
        grad = np.concatenate([(Eo @ wo) / S / dt(M), ((Eo * Eo) @ wo) / S / dt(M)])
    else:
        R = Eo * wo[None, :]
        X = (np.linalg.solve(S.T, R) if dt is np.float64 else B._back_substitute(S, R)).astype(dt)
        grad = np.concatenate([np.sum(X, axis=1, dtype=dt) / dt(M), (np.tril(X @ Eo.T) / dt(M)).reshape(-1, order="F")])
    return dict(value=dt(value), elbo=dt(-fbar), grad=grad.astype(dt))


def documented_scan(d, blocks, eta, dtype=np.float64):
    """[(lo, hi, x (hi - lo x M))] for the ordered blocks of two rows and more: the forward scan as k_bijx_fwd is documented to run it, in
    `dtype` throughout (an f64 context): hillis_steele_prefix inside every 256-row chunk, the previous chunk's last value added to it"""
    h = np.asarray(eta).astype(dtype)
    out = []
    for lo, hi, kind, _ in normalise(blocks):
        if kind != "ordered" or hi - lo < 2:
            continue
        inc = np.concatenate([h[lo:lo + 1], np.exp(h[lo + 1:hi])], axis=0)
        x, carry, a = np.empty_like(inc), None, lo
        while a < hi:
            b = min(hi, (a // 256 + 1) * 256)
            part = hillis_steele_prefix(inc[a - lo:b - lo], dtype)
            x[a - lo:b - lo] = part if carry is None else carry + part
            carry, a = x[b - lo - 1], b
        out.append((lo, hi, x))
    return out


def hillis_steele_prefix(v, dtype=np.float64):
    """Inclusive prefix sums of the columns of v (n <= 256 rows, one segment) in the order seg_scan256 of csrc/kernels_bijector.hip is
    documented to use: log2(256) rounds, in round `off` every row i >= off adds the previous round's value of row i - off -- every prefix
    is associated differently, so in `dtype` the result need not be monotone although every term after the first is positive."""
    x = np.asarray(v).astype(dtype).copy()
    off = 1
    while off < 256:
        prev = x.copy()
        x[off:] = prev[off:] + prev[:-off]
        off *= 2
    return x


def logpdf_constrained(params, d, family, blocks, X, dtype=np.float64):
    """logpdf(TransformedDistribution(q, binv), x) for the columns of X, Gaussian q: log q(b(x)) - logabsdetjac(binv, b(x)); -inf outside
    the support.  The bijector's arithmetic in `dtype`, log q through tests/scoregrad_ref.py logpdf_cols."""
    from tests import scoregrad_ref as R
    dt = np.dtype(dtype).type
    eta, ladj, inside = inverse(blocks, X, dt)
    if dt is np.longdouble:
        lq = _logq_wide(params, d, family, np.where(inside[None, :], eta, dt(0)))
    else:
        lq = R.logpdf_cols(params, d, family, np.where(inside[None, :], eta, dt(0)), dt)
    return np.where(inside, (np.asarray(lq).astype(dt) - ladj).astype(dt), dt(-np.inf))


# ==== the per-entry criterion (tests/test_bijector_ref_host.py, tests/test_gpu_bijector_yardstick.py) =========================================
# Follows tests/meanfield_ref.py: ref is the evaluation in the next wider type, env per entry the largest distance of eight summation orders
# of the evaluation in the element type, S the first-order magnitude (every operand replaced by its absolute value, every subtraction by an
# addition, a stored intermediate one rounding), and a result is held to F x max(env, u S).  The magnitudes, per row of a column:
#     forward   identity |eta|;  LOWER / UPPER / exp |bound| + e^eta;  two-sided max(|lb|, |ub|) + w p;  ordered |x_b| + sum_{k <= i} e^eta_k
#               ladj: sum |eta_i| over the rows that contribute, and |log w| + |eta| + 2 log1p(t) on the two-sided rows
#     backward  identity |g|;  LOWER / UPPER / exp e^eta |g| + 1;  two-sided w p (1 - p) |g| + |1 - 2 p|;  head sum_j |g_j|;
#               ordered e^eta_k sum_{j >= k} |g_j| + 1
#     gradient  |W| = backward magnitude of the target's gradient magnitude ((|x| + |m|) / s^2, |P| (|x| + |m|)), + |C^-T| |eps| under
#               sticking the landing;  dm_i = mean |W|_i;  dsigma_i = mean |W|_i |eps_i| + |direct| / sigma_i;
#               dC_ij = mean |W|_i |eps_j| (+ |direct| / C_ii on the diagonal)
from tests import meanfield_ref as Mf  # noqa: E402

U32, U64 = Mf.U32, Mf.U64
wider, orders = Mf.wider, Mf.orders
STL = Mf.STL
CLASSES = ("default", "wide", "far")


def _case(kind, lb, ub):
    """identity / lower / upper / both / ordered of a normalised block"""
    if kind == "exp":
        return "lower"
    if kind == "truncated":
        if np.isfinite(lb) and np.isfinite(ub):
            return "both"
        return "lower" if np.isfinite(lb) else "upper" if np.isfinite(ub) else "identity"
    return kind


def row_codes(d, blocks):
    """per row: "identity", "lower", "upper", "both", "head" or "ordered" (an ordered block of one row is an identity row), as
    mivi_set_bijector_stacked_ex codes them"""
    code = ["identity"] * d
    for lo, hi, kind, (lb, ub) in normalise(blocks):
        c = _case(kind, lb, ub)
        for i in range(lo, hi):
            code[i] = c if c != "ordered" else "identity" if hi - lo < 2 else "head" if i == lo else "ordered"
    return code


def magnitude_forward(blocks, eta):
    """(Sx (d x M), Sladj (M)), float64"""
    h = np.asarray(eta, dtype=np.float64)
    ha = np.abs(h)
    Sx, Sl = ha.copy(), np.zeros(h.shape[1])
    for lo, hi, kind, (lb, ub) in normalise(blocks):
        c, e, ea = _case(kind, lb, ub), h[lo:hi], ha[lo:hi]
        if c in ("lower", "upper"):
            Sx[lo:hi] = abs(0.0 if kind == "exp" else lb if c == "lower" else ub) + np.exp(e)
            Sl += np.sum(ea, axis=0)
        elif c == "both":
            p, t = _sigmoid_parts(e)
            Sx[lo:hi] = max(abs(lb), abs(ub)) + (ub - lb) * p
            Sl += np.sum(abs(np.log(ub - lb)) + ea + 2.0 * np.log1p(t), axis=0)
        elif c == "ordered" and hi - lo >= 2:
            Sx[lo:hi] = np.cumsum(np.concatenate([ea[:1], np.exp(e[1:])], axis=0), axis=0)
            Sl += np.sum(ea[1:], axis=0)
    return Sx, Sl


def magnitude_backward(blocks, eta, G):
    """(d x M), float64"""
    h, ga = np.asarray(eta, dtype=np.float64), np.abs(np.asarray(G, dtype=np.float64))
    out = ga.copy()
    for lo, hi, kind, (lb, ub) in normalise(blocks):
        c, e, gb = _case(kind, lb, ub), h[lo:hi], ga[lo:hi]
        if c in ("lower", "upper"):
            out[lo:hi] = np.exp(e) * gb + 1.0
        elif c == "both":
            p, _ = _sigmoid_parts(e)
            out[lo:hi] = (ub - lb) * p * (1.0 - p) * gb + np.abs(1.0 - 2.0 * p)
        elif c == "ordered" and hi - lo >= 2:
            Sa = np.cumsum(gb[::-1], axis=0)[::-1]
            out[lo:hi] = np.concatenate([Sa[:1], np.exp(e[1:]) * Sa[1:] + 1.0], axis=0)
    return out


def _inner_magnitude(inner, xa):
    """(ell_a (M), Ga (d x M)) of a diagonal / dense Gaussian at the magnitudes xa of its argument (tests/meanfield_ref.py)"""
    return Mf._magnitude_target(inner, xa, None, xa.shape[0])


def magnitude(params, d, family, inner, blocks, eps, ent, probe=None):
    """dict(grad, value): S of every gradient entry (zero above the diagonal of dC) and of the value, float64"""
    p, E = np.asarray(params, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    m, Sc = B.split(p, d, family)
    mf = family == O.MEANFIELD
    Ea = np.abs(E)
    Z = samples(p, d, family, E)
    Sx, Sl = magnitude_forward(blocks, Z)
    if probe is not None:
        ell_a, Ga = np.abs(np.asarray(probe[0], dtype=np.float64)), np.abs(np.asarray(probe[1], dtype=np.float64))
    else:
        ell_a, Ga = _inner_magnitude(inner, Sx)
    Wa = magnitude_backward(blocks, Z, Ga)
    diag = np.abs(Sc if mf else np.diag(Sc))
    if ent in STL:
        Wa = Wa + (Ea / diag[:, None] if mf else np.abs(np.linalg.inv(Sc)).T @ Ea)
    M = E.shape[1]
    direct = abs(B.DIRECT[ent])
    if mf:
        grad = np.concatenate([np.mean(Wa, axis=1), np.mean(Wa * Ea, axis=1) + direct / diag])
    else:
        grad = np.concatenate([np.mean(Wa, axis=1), (np.tril(Wa @ Ea.T) / M + direct * np.diag(1.0 / diag)).reshape(-1, order="F")])
    closed = ent in (O.ENT_CLOSED_FORM, O.ENT_CLOSED_FORM_ZERO_GRAD)
    ent_a = np.sum(np.abs(np.log(diag))) + (0.5 * d * (1.0 + LOG2PI) if closed else np.mean(0.5 * np.sum(E * E, axis=0)) + 0.5 * d * LOG2PI)
    return dict(grad=grad, value=float(np.mean(ell_a + Sl) + ent_a))


def magnitude_logpdf_constrained(params, d, family, blocks, X):
    """per column, float64: sum_i (u_i^2 / 2 + |u_i| (|C^-1| |eta|)_i + |log C_ii|) + d log(2 pi) / 2 + the inverse's |ladj terms|,
    u = C^-1 (eta - mu) (mean-field: C = diag(sigma)); the middle term is the rounding of the stored eta to the element type"""
    p, X = np.asarray(params, dtype=np.float64), np.asarray(X, dtype=np.float64)
    m, Sc = B.split(p, d, family)
    eta, _, inside = inverse(blocks, X)
    eta = np.where(inside[None, :], eta, 0.0)
    Ci = np.diag(1.0 / Sc) if family == O.MEANFIELD else np.linalg.inv(Sc)
    diag = Sc if family == O.MEANFIELD else np.diag(Sc)
    u = np.abs(Ci @ (eta - m[:, None]))
    S = np.sum(0.5 * u * u + u * (np.abs(Ci) @ np.abs(eta)), axis=0) + np.sum(np.abs(np.log(diag))) + 0.5 * d * LOG2PI
    for lo, hi, kind, (lb, ub) in normalise(blocks):
        c, xb = _case(kind, lb, ub), X[lo:hi]
        with np.errstate(all="ignore"):
            if c == "lower":
                S = S + np.sum(np.abs(np.log(xb - (0.0 if kind == "exp" else lb))), axis=0)
            elif c == "upper":
                S = S + np.sum(np.abs(np.log(ub - xb)), axis=0)
            elif c == "both":
                q = (xb - lb) / (ub - lb)
                S = S + np.sum(abs(np.log(ub - lb)) + np.abs(np.log(q)) + np.abs(np.log1p(-q)), axis=0)
            elif c == "ordered" and hi - lo >= 2:
                S = S + np.sum(np.abs(np.log(xb[1:] - xb[:-1])), axis=0)
    return np.where(inside, S, np.inf)


def _logq_wide(params, d, family, eta):
    """log q of a Gaussian location-scale family at the columns of eta in np.longdouble (numpy's solvers stop at float64: forward substitution)"""
    ld = np.longdouble
    p = np.asarray(params).astype(ld)
    m, Sc = B.split(p, d, family)
    R = np.asarray(eta).astype(ld) - m[:, None]
    if family == O.MEANFIELD:
        U, diag = R / Sc[:, None], Sc
    else:
        U, diag = np.zeros_like(R), np.diag(Sc)
        for i in range(d):
            U[i] = (R[i] - Sc[i, :i] @ U[:i]) / Sc[i, i]
    return -ld(0.5) * np.sum(U * U, axis=0) - ld(0.5 * d) * np.log(ld(2) * np.pi) - np.sum(np.log(diag))


def logpdf_yard(params, d, family, blocks, X, dtype):
    """logpdf_constrained as DESIGN.md documents the device's: the inverse and every sum in float64 from the stored points, eta rounded to
    the element type between the two"""
    from tests import scoregrad_ref as R
    eta, ladj, inside = inverse(blocks, np.asarray(X, dtype=np.float64))
    eta = np.where(inside[None, :], eta, 0.0).astype(dtype).astype(np.float64)
    lq = R.logpdf_cols(np.asarray(params, dtype=np.float64), d, family, eta)
    return np.where(inside, np.asarray(lq, dtype=np.float64) - ladj, -np.inf)


def envelope(params, d, family, inner, blocks, eps, ent, dtype=np.float32, ref=None, probe=None):
    """dict(grad, value): per entry max_k |yard_k - ref| over orders(M), yard_k = gradient(..., dtype, order_k)"""
    wide = wider(dtype)
    ref = gradient(params, d, family, inner, blocks, eps, ent, wide, probe=probe) if ref is None else ref
    env_g, env_v = np.zeros(ref["grad"].size, dtype=wide), wide(0.0)
    for o in orders(np.asarray(eps).shape[1]):
        y = gradient(params, d, family, inner, blocks, eps, ent, dtype, o, probe)
        env_g = np.maximum(env_g, np.abs(y["grad"].astype(wide) - ref["grad"]))
        env_v = max(env_v, abs(wide(y["value"]) - ref["value"]))
    return dict(grad=env_g, value=env_v)


def score_envelope(params, d, family, inner, blocks, eps, dtype=np.float32, ref=None):
    """dict(grad, value, elbo): envelope for score_gradient"""
    wide = wider(dtype)
    ref = score_gradient(params, d, family, inner, blocks, eps, wide) if ref is None else ref
    env = dict(grad=np.zeros(ref["grad"].size, dtype=wide), value=wide(0.0), elbo=wide(0.0))
    for o in orders(np.asarray(eps).shape[1]):
        y = score_gradient(params, d, family, inner, blocks, eps, dtype, o)
        env["grad"] = np.maximum(env["grad"], np.abs(y["grad"].astype(wide) - ref["grad"]))
        for k in ("value", "elbo"):
            env[k] = max(env[k], abs(wide(y[k]) - ref[k]))
    return env


def score_magnitude(params, d, family, inner, blocks, eps):
    """dict(grad, value, elbo), float64: fa_m = |log pi|_a + S(ladj) + |log q|_a (the magnitudes of `magnitude`), wa = fa + mean fa;
    dm_i = mean_m (|C^-T| |eps|)_im wa_m,  dsigma_i = mean_m eps_im^2 wa_m / sigma_i,  dC_ij = mean_m (|C^-T| (|eps| wa))_im |eps_jm|;
    value mean wa^2 / 2, elbo mean fa"""
    p, E = np.asarray(params, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    m, Sc = B.split(p, d, family)
    mf = family == O.MEANFIELD
    Ea = np.abs(E)
    Sx, Sl = magnitude_forward(blocks, samples(p, d, family, E))
    ell_a, _ = _inner_magnitude(inner, Sx)
    diag = np.abs(Sc if mf else np.diag(Sc))
    fa = ell_a + Sl + 0.5 * np.sum(E * E, axis=0) + np.sum(np.abs(np.log(diag))) + 0.5 * d * LOG2PI
    wa = fa + np.mean(fa)
    M = E.shape[1]
    if mf:
        grad = np.concatenate([(Ea @ wa) / diag / M, ((E * E) @ wa) / diag / M])
    else:
        Xa = np.abs(np.linalg.inv(Sc)).T @ (Ea * wa[None, :])
        grad = np.concatenate([np.sum(Xa, axis=1) / M, (np.tril(Xa @ Ea.T) / M).reshape(-1, order="F")])
    return dict(grad=grad, value=float(np.mean(wa * wa) / 2.0), elbo=float(np.mean(fa)))


def ratios(got, env, ref, S_mag, d, family, u, extra=None):
    """dict(whole, block, row, entry) of a flat gradient, every number ||got - ref|| / (max(||env||, u ||S||) + ||extra||) over a set of entries:
        whole  all of them
        entry  each entry of dm
        row    mean-field: each entry of dsigma;  full-rank: each ROW of dC (what row i of W produces)
        block  mean-field: rows 4b .. 4b + 3 of dm and of dsigma (meanfield_ref.ratios);  full-rank: the 64-row blocks of dm and of dC"""
    ld = np.longdouble
    err = np.abs(np.asarray(got).astype(ld) - np.asarray(ref).astype(ld))
    en, fl = np.asarray(env).astype(ld), ld(u) * np.asarray(S_mag).astype(ld)
    ex = np.zeros(err.size, dtype=ld) if extra is None else np.asarray(extra).astype(ld)
    tiny = ld(np.finfo(np.float64).tiny)
    norm = lambda a: np.sqrt(np.sum(a * a))   # noqa: E731
    over = lambda a, b, c, x: float(norm(a) / (max(norm(b), norm(c)) + norm(x) + tiny))   # noqa: E731
    entry = float(np.max(err[:d] / (np.maximum(en[:d], fl[:d]) + ex[:d] + tiny)))
    whole = over(err, en, fl, ex)
    if family == O.MEANFIELD:
        _, quad, _ = Mf.ratios(got, env, ref, S_mag, d, u, extra)
        row = float(np.max(err[d:] / (np.maximum(en[d:], fl[d:]) + ex[d:] + tiny)))
        return dict(whole=whole, block=quad, row=row, entry=entry)
    mats = [a[d:].reshape(d, d, order="F") for a in (err, en, fl, ex)]
    row = max(over(*[A[i, :i + 1] for A in mats]) for i in range(d))
    block = max(max(over(*[A[lo:lo + 64] for A in mats]), over(*[a[lo:min(lo + 64, d)] for a in (err, en, fl, ex)])) for lo in range(0, d, 64))
    return dict(whole=whole, block=block, row=row, entry=entry)


value_ratio = Mf.value_ratio


def entry_ratio(got, ref, S_mag, u, env=None):
    """the worst |got - ref| / max(env, u S) over an array (forward, backward, logpdf: nothing to permute, env is then left out)"""
    ld = np.longdouble
    err = np.abs(np.asarray(got).astype(ld) - np.asarray(ref).astype(ld))
    den = ld(u) * np.asarray(S_mag).astype(ld)
    if env is not None:
        den = np.maximum(den, np.asarray(env).astype(ld))
    return float(np.max(err / (den + ld(np.finfo(np.float64).tiny)))) if err.size else 0.0


# ---- layouts and what each reaches ---------------------------------------------------------------------------------------------------------
LAYOUTS = {
    # forward chunk 1 is row 256 alone, mirrored chunk 1 row 0 alone; [0, 3) crosses the mirrored boundary 1 | 0, [250, 257) forward row 256
    # and ends at d - 1 with [240, 250) directly in front of it (adjacent heads); lengths 1 and 2; every bounded kind, exp, uncovered rows
    "257": (257, [(0, 3, "ordered"), (3, 5, "truncated", (0.25, np.inf)), (5, 7, "truncated", (-np.inf, 1.5)), (7, 10, "truncated", (-1.0, 2.0)),
                  (10, 13, "exp"), (13, 14, "ordered"), (14, 16, "ordered"), (16, 18, "identity"), (20, 22, "truncated", (-np.inf, np.inf)),
                  (100, 104, "truncated", (-3.0, -1.0)), (240, 250, "ordered"), (250, 257, "ordered")]),
    "513": (513, [(0, 513, "ordered")]),                       # both scans pass a whole chunk with no head in it
    "512": (512, [(0, 256, "ordered"), (256, 512, "ordered")]),   # adjacent AT the chunk boundary: nothing may cross it
    "300": (300, layout(300)),
    "5": (5, layout(5)),
    "2": (2, [(0, 2, "ordered")]),
    "1-identity": (1, [(0, 1, "identity")]),
    "1-exp": (1, [(0, 1, "exp")]),
    "1-lower": (1, [(0, 1, "truncated", (0.25, np.inf))]),
    "1-upper": (1, [(0, 1, "truncated", (-np.inf, 1.5))]),
    "1-both": (1, [(0, 1, "truncated", (-1.0, 2.0))]),
    "1-ordered": (1, [(0, 1, "ordered")]),
    "legacy257": (257, [(0, 128, "identity"), (128, 257, "exp")]),   # k_bij_fwd / k_bij_bwd of csrc/kernels_targets.hip
}


def stages(d, blocks):
    """What a layout reaches in k_bijx_fwd / k_bijx_bwd, restated from their documented shape: 256 rows per chunk, forward from row 0,
    backward from row d - 1; a forward segment starts at every row that is not a non-first row of an ordered block, a mirrored one at every
    row whose successor is none.  dict:
        chunks         the chunk count of either scan
        legacy         identity / exp blocks only (the kernels of csrc/kernels_targets.hip, no scan)
        fwd_cross      ordered blocks with rows 256 k - 1 | 256 k both inside (the forward carry enters them)
        bwd_cross      ordered blocks with rows d - 256 k | d - 256 k - 1 both inside (the mirrored carry)
        fwd_headless   forward chunks with no segment start (the carry is added on every row of them), bwd_headless the mirrored ones
        at_row0, at_end, at_chunk_start, at_chunk_end   ordered blocks that start at row 0 / end at row d - 1 / start at a forward chunk's
                       first row / end at a forward chunk's last row
        adjacent       pairs of ordered blocks with no row between them"""
    nb = normalise(blocks)
    code = row_codes(d, blocks)
    ords = [(lo, hi) for lo, hi, kind, _ in nb if kind == "ordered" and hi - lo >= 2]
    chunks = (d + 255) // 256
    cuts = [256 * k for k in range(1, chunks) if 256 * k < d]
    mcuts = [d - 256 * k for k in range(1, chunks) if d - 256 * k > 0]   # rows c | c - 1 are in different mirrored chunks
    fwd_head = [c != "ordered" for c in code]
    bwd_head = [i + 1 >= d or code[i + 1] != "ordered" for i in range(d)]
    return dict(
        chunks=chunks,
        legacy=all(kind in ("identity", "exp") for _, _, kind, _ in nb),
        fwd_cross=[(lo, hi) for lo, hi in ords if any(lo < c < hi for c in cuts)],
        bwd_cross=[(lo, hi) for lo, hi in ords if any(lo < c < hi for c in mcuts)],
        fwd_headless=[k for k in range(chunks) if not any(fwd_head[256 * k:min(256 * k + 256, d)])],
        bwd_headless=[k for k in range(chunks) if not any(bwd_head[max(d - 256 * k - 256, 0):d - 256 * k])],
        at_row0=[b for b in ords if b[0] == 0], at_end=[b for b in ords if b[1] == d],
        at_chunk_start=[b for b in ords if b[0] % 256 == 0], at_chunk_end=[b for b in ords if b[1] % 256 == 0 or b[1] == d],
        adjacent=[(a, b) for a in ords for b in ords if a[1] == b[0]])


# ---- parameter classes -------------------------------------------------------------------------------------------------------------------------
def _x_spread(blocks, loc, sig):
    """(x at the location (d), the size of x's movement under eta = loc +- sig (d)), float64"""
    x0 = forward(blocks, loc[:, None])[0][:, 0]
    hi, lo = forward(blocks, (loc + sig)[:, None])[0][:, 0], forward(blocks, (loc - sig)[:, None])[0][:, 0]
    return x0, np.maximum(np.abs(hi - x0), np.abs(lo - x0))


def make_case(cls, name, family, target, dtype=np.float64):
    """dict(d, blocks, params, inner, loc, scale) of one (class, layout, family, target) in the element type `dtype`, seeded by its names:
        default  tests/helpers.py make_family / make_problem at their own scales
        wide     locations spread so that eta covers [-30, 30] on the exp-like and ordered rows and [-20, 20] on the two-sided rows, scales
                 0.05 x the default's; the first two-sided row sits AT eta = 0 with scale 2^-20, so its draws fall on both sides of zero
                 within 1e-5 (eta = 0 itself and +- one spacing are not reachable from a draw; the host test evaluates them directly); the
                 diagonal target is moved to x(loc) and widened to the movement of x, so that g stays O(1 .. 1e3) and finite in float32.
                 Layout 513 narrows the ordered rows to N(-3, 0.3): x stays below about 30
        far      cancellation_case made general: |lb|, |ub| and every ordered head in 10^U(2, 6) (the two-sided widths in 10^U(0, 2)),
                 eta ~ N(-7, 0.3) on every bounded / ordered row (increments e^eta ~ 1e-3); the target ten units from x(loc) with std 1
    target: "diag" or "dense" (wide / far: the diagonal one only)."""
    import zlib

    from tests.helpers import make_family, make_problem
    d, blocks = LAYOUTS[name]
    blocks = [tuple(b) for b in blocks]
    rng = np.random.default_rng(zlib.crc32(f"{cls} {name} {family} {target}".encode()))
    dt = np.dtype(dtype).type
    _, q = make_family(rng, d, family)
    loc, Sc = q.location.copy(), q.scale.copy()
    _, inner = make_problem(rng, target, d)
    code = row_codes(d, blocks)
    if cls != "default" and target != "diag":
        raise ValueError("the classes wide and far move the diagonal target only")
    if cls == "wide":
        Sc = Sc * 0.05
        for want, span in (("lower", 30.0), ("upper", 30.0), ("ordered", 30.0), ("both", 20.0)):
            rows = [i for i in range(d) if code[i] == want]
            if rows:
                loc[rows] = rng.permutation(np.linspace(-span, span, len(rows))) if len(rows) > 1 else span
        if name == "513":
            loc[1:] = rng.normal(-3.0, 0.3, size=d - 1)
        both = [i for i in range(d) if code[i] == "both"]
        if both:
            i = both[0]
            loc[i] = 0.0
            if family == O.MEANFIELD:
                Sc[i] = 2.0 ** -20
            else:
                Sc[i, :] = 0.0
                Sc[i, i] = 2.0 ** -20
        sig = Sc if family == O.MEANFIELD else np.sqrt(np.sum(Sc * Sc, axis=1))
        x0, spread = _x_spread(blocks, loc, 3.0 * sig)
        inner = O.DiagNormalTarget(x0 + rng.normal(size=d), rng.uniform(0.5, 2.0, size=d) * np.maximum(1.0, spread))
    elif cls == "far":
        new = []
        for lo, hi, kind, (lb, ub) in normalise(blocks):
            c = _case(kind, lb, ub)
            big = float(rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(2.0, 6.0))
            if c == "lower":
                new.append((lo, hi, "truncated", (big, np.inf)))
            elif c == "upper":
                new.append((lo, hi, "truncated", (-np.inf, big)))
            elif c == "both":
                new.append((lo, hi, "truncated", (big, big + float(10.0 ** rng.uniform(0.0, 2.0)))))
            else:
                new.append((lo, hi, kind) if kind != "truncated" else (lo, hi, kind, (lb, ub)))
            if c in ("lower", "upper", "both") or (c == "ordered" and hi - lo >= 2):
                loc[lo:hi] = rng.normal(-7.0, 0.3, size=hi - lo)
                if c == "ordered":
                    loc[lo] = big
        blocks = new
        Sc = Sc * 0.5
        x0 = forward(blocks, loc[:, None])[0][:, 0]
        inner = O.DiagNormalTarget(x0 + 10.0 * rng.choice([-1.0, 1.0], size=d), np.ones(d))
    elif cls != "default":
        raise ValueError(cls)
    params = np.concatenate([loc, Sc if family == O.MEANFIELD else Sc.reshape(-1, order="F")]).astype(dt)
    if isinstance(inner, O.DiagNormalTarget):
        inner = O.DiagNormalTarget(inner.mean.astype(dt), inner.std.astype(dt))
    else:
        inner = O.DenseNormalTarget(inner.mean.astype(dt), inner.L.astype(dt))
    return dict(d=d, blocks=blocks, params=params, inner=inner, family=family)


def graded_probe(d, blocks, M, rng, dtype=np.float32):
    """(ell (M), G (d x M)) for the recording plugin, representable in `dtype`: |G| = 10^U(-3, 3), the signs alternating along the rows of
    every ordered block (so that the suffix sums cancel), random elsewhere"""
    G = 10.0 ** rng.uniform(-3.0, 3.0, size=(d, M)) * rng.choice([-1.0, 1.0], size=(d, M))
    for lo, hi, kind, _ in normalise(blocks):
        if kind == "ordered":
            G[lo:hi] = np.abs(G[lo:hi]) * ((-1.0) ** np.arange(hi - lo))[:, None]
    return rng.normal(size=M).astype(dtype), G.astype(dtype)


# ---- the cases of tests/test_gpu_bijector_yardstick.py (tests/test_bijector_ref_host.py runs the reference alone on the same list) -----------
FAMILIES = (O.MEANFIELD, O.FULLRANK)
SMALL = ("5", "2", "1-identity", "1-exp", "1-lower", "1-upper", "1-both", "1-ordered")
ESTIMATE_LAYOUTS = ("257", "513", "512", "300", "legacy257") + SMALL
M_EST = 33


def estimate_cases():
    """[(class, layout, family, target, entropy kind, M)]: both families x every layout x {diag, dense} x kinds {0, 3} on `default` (d <= 5 at
    M = 1 too); all five kinds on `default` and `wide` and kinds {0, 3} on `far` at d = 257 with the diagonal target"""
    out = [("default", n, f, t, e, M) for f in FAMILIES for n in ESTIMATE_LAYOUTS for t in ("diag", "dense") for e in (0, 3)
           for M in ((M_EST, 1) if n in SMALL else (M_EST,))]
    out += [("default", "257", f, "diag", e, M_EST) for f in FAMILIES for e in (1, 2, 4)]
    out += [("wide", "257", f, "diag", e, M_EST) for f in FAMILIES for e in (0, 1, 2, 3, 4)]
    out += [("far", "257", f, "diag", e, M_EST) for f in FAMILIES for e in (0, 3)]
    return out


def assert_layouts_reach_their_mechanisms():
    """the shape list does what LAYOUTS' comments say (tests/test_bijector_ref_host.py and tests/test_gpu_bijector_yardstick.py both call it)"""
    st = {n: stages(d, b) for n, (d, b) in LAYOUTS.items()}
    a = st["257"]
    assert a["chunks"] == 2 and a["fwd_cross"] == [(250, 257)] and a["bwd_cross"] == [(0, 3)] and a["at_row0"] == [(0, 3)] and a["at_end"] == [(250, 257)]
    assert a["adjacent"] == [((240, 250), (250, 257))] and a["fwd_headless"] == [1] and a["bwd_headless"] == [1] and not a["legacy"]
    codes = set(row_codes(*LAYOUTS["257"]))
    assert codes == {"identity", "lower", "upper", "both", "head", "ordered"}
    assert any(hi - lo == 1 and k == "ordered" for lo, hi, k, _ in normalise(LAYOUTS["257"][1])) and any(hi - lo == 2 and k == "ordered" for lo, hi, k, _ in normalise(LAYOUTS["257"][1]))
    b = st["513"]
    assert b["chunks"] == 3 and b["fwd_headless"] == [1, 2] and b["bwd_headless"] == [1, 2] and b["fwd_cross"] == b["bwd_cross"] == [(0, 513)]
    c = st["512"]
    assert c["chunks"] == 2 and c["fwd_cross"] == [] and c["bwd_cross"] == [] and c["adjacent"] == [((0, 256), (256, 512))]
    assert c["at_chunk_start"] == c["at_chunk_end"] == [(0, 256), (256, 512)] and c["fwd_headless"] == [] and c["bwd_headless"] == []
    e = st["300"]
    assert e["fwd_cross"] == [(250, 270)] and e["bwd_cross"] == [(40, 48)] and ((36, 40), (40, 48)) in e["adjacent"]
    assert st["legacy257"]["legacy"] and st["legacy257"]["chunks"] == 2 and set(row_codes(*LAYOUTS["legacy257"])) == {"identity", "lower"}
    assert [row_codes(*LAYOUTS[n])[0] for n in SMALL[2:]] == ["identity", "lower", "lower", "upper", "both", "identity"]
    assert row_codes(*LAYOUTS["2"]) == ["head", "ordered"] and not any(st[n]["legacy"] for n in ("5", "2", "1-lower", "1-upper", "1-both", "1-ordered"))
