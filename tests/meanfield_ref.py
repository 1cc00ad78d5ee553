"""numpy restatement of the mean-field RepGradELBO estimate (csrc/kernels_meanfield.hip) and the per-entry criterion its kernels are held to
-- a helper of tests/test_meanfield_ref_host.py and tests/test_gpu_meanfield_yardstick.py, not a test.  It reuses oracle/ and
tests/solve_ref.py / tests/product_ref.py wherever it can.

    family_and_target   the parameter classes (mu, sigma, m, s) the kernels are held on
    gradient            oracle.estimate_gradient(params, d, MEANFIELD, tgt, eps, ent) for the five entropy kinds, every rounding in `dtype`,
                        with an optional permutation of the sample columns applied before every row sum: np.longdouble / np.float64 is the
                        reference of an f64 / f32 context, np.float64 / np.float32 its yardstick
    envelope            per entry the largest |yard_k - ref| over the identity order and seven seeded permutations of the columns
    magnitude           S_i: the expression of every entry in float64 with every operand replaced by its absolute value and every
                        subtraction by an addition -- the first-order rounding scale, the floor of the criterion
    ratios, value_ratio the criterion: entry, quad (a workgroup's four rows of dmu and of dsigma) and whole-gradient ratios
    n_cc                the shape rule of mf_main_impl restated: (column chunks, columns per chunk) of a single call
    emulate             the diagonal-target estimate in float32 numpy with the summation order the kernels are DOCUMENTED to use, and the
                        injectable faults of the host test; no code of the kernels

Why an envelope: a mean-field gradient entry belongs to one workgroup (rows 4b .. 4b + 3) and nothing mixes rows, so the criterion has to be
per entry -- and the error of ONE float32 evaluation on a single entry is a random draw that is often near zero: as a denominator it put an
emulation of the shipped summation order at 45 times "the yardstick".  The largest of eight orders put the same emulation at 2.0 or less.
Why a floor: with M = 1, or on rows where z - m cancels, all eight orders can agree with the reference by chance; u S_i is what one rounding
of the largest intermediate costs.

S_i per target (za = |mu| + |sigma eps| is the magnitude of z; `mean` is over the samples; Wa is the magnitude of W):
    diagonal Gaussian   Wa = (za + |m|) / s^2
    dense Gaussian      Wa = |P| (za + |m|)
    funnel              c = 1 + 2 za_0 (what a rounding of the argument of exp(-2 z_0) does to the factor), rows >= 1: Wa = c za exp(-2 z_0);
                        row 0: Wa = 2 + za_0 / sigma_v^2 + (d - 1) + c sum_i za_i^2 exp(-2 z_0)
    exp bijector rows   x = exp(z), c = 1 + za: Wa = c x (x + |m|) / s^2 + 1 (the other rows: the inner target's)
    every target        + |eps| / sigma under sticking the landing;  S(dmu) = mean Wa,  S(dsigma) = mean Wa |eps| + |direct| / sigma
The value's S is the same substitution in -(mean ell + entropy)."""
import math

import numpy as np

from oracle import oracle as O
from tests import product_ref as Pr
from tests import solve_ref as S

assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "the f64 reference needs an extended-precision np.longdouble"

LOG2PI = S.LOG2PI
DIRECT = S.DIRECT
STL = (O.ENT_STL, O.ENT_STL_ZERO_GRAD)
CLOSED = (O.ENT_CLOSED_FORM, O.ENT_CLOSED_FORM_ZERO_GRAD)
CLASSES = ("default", "graded", "far", "near")
FUNNEL_CLASSES = ("funnel", "wide")
N_PERM = 7
U32, U64 = 2.0 ** -24, 2.0 ** -53


# ---- parameter classes -------------------------------------------------------------------------------------------------------------------
def family_and_target(kind, d, rng):
    """(mu, sigma, m, s) in float64 (the caller casts to the context's dtype; m = s = None for the funnel classes):
        default  tests/helpers.py make_family / make_problem: mu, m ~ N(0, 1), sigma ~ U(0.5, 1.5), s ~ U(0.5, 2)
        graded   sigma = 10^U(-3, 3), s = 10^U(-2, 2): rows spanning six decades, so one row's fault vanishes in the whole-gradient norm
        far      mu = m + 1e3 N(0, 1): large values, nothing cancels
        near     mu = m (1 + 1e-3 N), sigma = s (1 + 1e-3 N): z - m cancels and, under sticking the landing, so does W = -(z - m) / s^2 +
                 eps / sigma -- a column lost from a row then changes the entry by about 1e-3 of a term, by construction nearly invisible
                 under the entropy kinds 3 and 4 (the host test exempts exactly that pair)
        funnel   make_family with mu_scale = 0.3 (what the funnel tests use)
        wide     the same with sigma_0 = 1.5: exp(-2 z_0) spans decades across the samples"""
    if kind in FUNNEL_CLASSES:
        mu, sigma = 0.3 * rng.normal(size=d), rng.uniform(0.5, 1.5, size=d)
        if kind == "wide":
            sigma[0] = 1.5
        return mu, sigma, None, None
    mu, sigma = rng.normal(size=d), rng.uniform(0.5, 1.5, size=d)
    m, s = rng.normal(size=d), rng.uniform(0.5, 2.0, size=d)
    if kind == "default":
        return mu, sigma, m, s
    if kind == "graded":
        return mu, 10.0 ** rng.uniform(-3.0, 3.0, size=d), m, 10.0 ** rng.uniform(-2.0, 2.0, size=d)
    if kind == "far":
        return m + 1e3 * rng.normal(size=d), sigma, m, s
    if kind == "near":
        return m * (1.0 + 1e-3 * rng.normal(size=d)), s * (1.0 + 1e-3 * rng.normal(size=d)), m, s
    raise ValueError(kind)


# ---- the reference and the yardstick ---------------------------------------------------------------------------------------------------------
def _target(tgt, Z, dtype):
    """(log pi(z_m) (M), grad log pi(z_m) (d x M)) for the columns of Z, every step in `dtype`"""
    d = Z.shape[0]
    if hasattr(tgt, "blocks") and hasattr(tgt, "inner"):   # tests/bijector_ref.py BijectorTarget: its steps at the kernels' documented precisions
        from tests import bijector_ref as BR
        acc = np.float64 if dtype is np.float32 else None
        X, ladj = BR.forward(tgt.blocks, Z, dtype, acc)
        ell, G = _target(tgt.inner, X, dtype)
        return (ell + ladj).astype(dtype), BR.backward(tgt.blocks, Z, G, dtype, acc)
    if isinstance(tgt, O.StackedBijectorTarget):   # x = exp(eta) on the masked rows: logdensity + sum eta, gradient x g + 1
        mask = tgt.mask[:, None]
        with np.errstate(over="ignore"):
            X = np.where(mask, np.exp(Z), Z).astype(dtype)
        ell, G = _target(tgt.inner, X, dtype)
        ell = ell + np.sum(np.where(mask, Z, dtype(0.0)), axis=0, dtype=dtype)
        return ell.astype(dtype), np.where(mask, X * G + dtype(1.0), G).astype(dtype)
    if isinstance(tgt, O.DiagNormalTarget):
        return S._diag_target(tgt, Z, dtype)
    if isinstance(tgt, O.DenseNormalTarget):
        return Pr._target(tgt, Z, dtype)
    if isinstance(tgt, O.FunnelStackedTarget):     # oracle.FunnelStackedTarget.logdensity_and_gradient, vectorised over the columns
        n, sv = d - 1, tgt.sigma_v
        sv2 = dtype(sv * sv)
        e1, X = Z[0], Z[1:]
        inv_s2 = np.exp(dtype(-2.0) * e1).astype(dtype)
        sx2 = np.sum(X * X, axis=0, dtype=dtype)
        ell = (-e1 - dtype(math.log(sv)) - dtype(0.5 * LOG2PI) - e1 * e1 / (dtype(2.0) * sv2)) + (-dtype(n) * e1 - dtype(0.5 * n * LOG2PI) - dtype(0.5) * sx2 * inv_s2) + e1
        G = np.empty_like(Z)
        G[0] = (dtype(-1.0) - e1 / sv2) + (-dtype(n) + sx2 * inv_s2) + dtype(1.0)
        G[1:] = -X * inv_s2
        return ell.astype(dtype), G
    raise TypeError(type(tgt))


def _rowsum(A, order, dtype):
    return np.sum(np.ascontiguousarray(A if order is None else A[:, order]), axis=1, dtype=dtype)


def gradient(params, d, tgt, eps, ent, dtype=np.float64, order=None):
    """dict(value, grad) of oracle.estimate_gradient(params, d, MEANFIELD, tgt, eps, ent) in closed form, every rounding in `dtype`
    (np.float32, np.float64 or np.longdouble), for a DiagNormalTarget, a FunnelStackedTarget, a DenseNormalTarget, or a
    StackedBijectorTarget (identity / exp blocks) around one of them.  order: a permutation of the M sample columns applied before each
    row sum (and the sum of the ell_m); the terms are the same, only their summation order changes."""
    dtype = np.dtype(dtype).type
    p = np.asarray(params)
    mu, sg = p[:d].astype(dtype), p[d:2 * d].astype(dtype)
    E = np.asarray(eps).astype(dtype)
    M = E.shape[1]
    Z = (mu[:, None] + sg[:, None] * E).astype(dtype)
    ell, G = _target(tgt, Z, dtype)
    W = (G + E / sg[:, None]).astype(dtype) if ent in STL else G
    logdet = np.sum(np.log(sg), dtype=dtype)
    if ent in CLOSED:
        entropy = dtype(d * 0.5 * (1.0 + LOG2PI)) + logdet
    else:
        he = dtype(0.5) * np.sum(E * E, axis=0, dtype=dtype)
        entropy = np.sum(he if order is None else he[order], dtype=dtype) / dtype(M) + dtype(0.5 * d * LOG2PI) + logdet
    g_mu = -_rowsum(W, order, dtype) / dtype(M)
    g_sg = -_rowsum(W * E, order, dtype) / dtype(M) - dtype(DIRECT[ent]) / sg
    mean_ell = np.sum(ell if order is None else ell[order], dtype=dtype) / dtype(M)
    return dict(value=dtype(-(mean_ell + entropy)), grad=np.concatenate([g_mu, g_sg]).astype(dtype))


def wider(dtype):
    return {np.float32: np.float64, np.float64: np.longdouble}[np.dtype(dtype).type]


def orders(M):
    """the identity and N_PERM seeded permutations of the sample columns"""
    return [None] + [np.random.default_rng(1000 + k).permutation(M) for k in range(N_PERM)]


def envelope(params, d, tgt, eps, ent, dtype=np.float32, ref=None):
    """dict(grad (2d), value): per entry max_k |yard_k - ref| over the orders of `orders(M)`, yard_k = gradient(..., dtype, order_k) and
    ref = gradient(..., the next wider type) unless given."""
    wide = wider(dtype)
    ref = gradient(params, d, tgt, eps, ent, wide) if ref is None else ref
    env_g, env_v = np.zeros(2 * d, dtype=wide), wide(0.0)
    for o in orders(np.asarray(eps).shape[1]):
        y = gradient(params, d, tgt, eps, ent, dtype, o)
        env_g = np.maximum(env_g, np.abs(y["grad"].astype(wide) - ref["grad"]))
        env_v = max(env_v, abs(wide(y["value"]) - ref["value"]))
    return dict(grad=env_g, value=env_v)


def _magnitude_target(tgt, za, Z, d):
    """(ell_a (M), Wa (d x M)): the magnitudes of log pi and its gradient (module docstring)"""
    if hasattr(tgt, "blocks") and hasattr(tgt, "inner"):   # tests/bijector_ref.py BijectorTarget and its magnitudes
        from tests import bijector_ref as BR
        Sx, Sl = BR.magnitude_forward(tgt.blocks, Z)
        ell_a, Ga = _magnitude_target(tgt.inner, Sx, None, d)
        return ell_a + Sl, BR.magnitude_backward(tgt.blocks, Z, Ga)
    if isinstance(tgt, O.StackedBijectorTarget):
        mask = tgt.mask[:, None]
        with np.errstate(over="ignore"):
            X = np.where(mask, np.exp(Z), 0.0)     # (read on the exp rows only)
        c = np.where(mask, 1.0 + za, 1.0)
        inner = tgt.inner
        if not isinstance(inner, O.DiagNormalTarget):
            raise TypeError(type(inner))
        m, s = np.abs(inner.mean)[:, None], inner.std[:, None]
        xa = np.where(mask, X * c, za)
        ell_a = 0.5 * np.sum(((xa + m) / s) ** 2, axis=0) + np.sum(np.abs(np.log(inner.std))) + 0.5 * d * LOG2PI + np.sum(np.where(mask, za, 0.0), axis=0)
        return ell_a, np.where(mask, c * X * (X + m) / s ** 2 + 1.0, (za + m) / s ** 2)
    if isinstance(tgt, O.DiagNormalTarget):
        m, s = np.abs(tgt.mean)[:, None], tgt.std[:, None]
        return 0.5 * np.sum(((za + m) / s) ** 2, axis=0) + np.sum(np.abs(np.log(tgt.std))) + 0.5 * d * LOG2PI, (za + m) / s ** 2
    if isinstance(tgt, O.DenseNormalTarget):
        Ra = za + np.abs(tgt.mean)[:, None]
        Wa = np.abs(Pr.dense_precision(tgt.L)) @ Ra
        return 0.5 * np.sum(Ra * Wa, axis=0) + abs(float(np.sum(np.log(np.diag(tgt.L))))) + 0.5 * d * LOG2PI, Wa
    if isinstance(tgt, O.FunnelStackedTarget):
        n, sv2 = d - 1, tgt.sigma_v ** 2
        e1a, inv_s2 = za[0], np.exp(-2.0 * Z[0])
        c = 1.0 + 2.0 * e1a
        sx2a = np.sum(za[1:] ** 2, axis=0)
        Wa = np.empty_like(za)
        Wa[0] = 2.0 + e1a / sv2 + n + c * sx2a * inv_s2
        Wa[1:] = c * za[1:] * inv_s2
        ell_a = (2.0 + n) * e1a + abs(math.log(tgt.sigma_v)) + 0.5 * LOG2PI + e1a * e1a / (2.0 * sv2) + 0.5 * n * LOG2PI + 0.5 * c * sx2a * inv_s2
        return ell_a, Wa
    raise TypeError(type(tgt))


def magnitude(params, d, tgt, eps, ent):
    """dict(grad (2d), value): S_i of every gradient entry and of the value, float64 (module docstring)"""
    p = np.asarray(params, dtype=np.float64)
    mu, sg = p[:d], p[d:2 * d]
    E = np.asarray(eps, dtype=np.float64)
    Ea = np.abs(E)
    za = np.abs(mu)[:, None] + np.abs(sg)[:, None] * Ea
    ell_a, Wa = _magnitude_target(tgt, za, mu[:, None] + sg[:, None] * E, d)
    if ent in STL:
        Wa = Wa + Ea / np.abs(sg)[:, None]
    grad = np.concatenate([np.mean(Wa, axis=1), np.mean(Wa * Ea, axis=1) + abs(DIRECT[ent]) / np.abs(sg)])
    ent_a = np.sum(np.abs(np.log(sg))) + (d * 0.5 * (1.0 + LOG2PI) if ent in CLOSED else np.mean(0.5 * np.sum(E * E, axis=0)) + 0.5 * d * LOG2PI)
    return dict(grad=grad, value=float(np.mean(ell_a) + ent_a))


# ---- the criterion -----------------------------------------------------------------------------------------------------------------------------
def _norm(a):
    return np.sqrt(np.sum(a * a))


def ratios(got, yard_env, ref, S_mag, d, u, extra=None):
    """(whole, quad, entry) of a mean-field gradient of 2d entries, all differences in np.longdouble:
        entry  the worst |got_i - ref_i| / (max(env_i, u S_i) + extra_i)
        quad   the same with l2 norms over rows 4b .. 4b + 3 of dmu and of dsigma, the worst over b: ||got - ref|| / (max(||env||, u ||S||) + ||extra||)
        whole  the same over the whole gradient
    extra: an allowance added to every denominator (the rounding of a stored parameter when the gradient is recovered from a Descent step)."""
    ld = np.longdouble
    err = np.abs(np.asarray(got).astype(ld) - np.asarray(ref).astype(ld))
    env, fl = np.asarray(yard_env).astype(ld), ld(u) * np.asarray(S_mag).astype(ld)
    ex = np.zeros(2 * d, dtype=ld) if extra is None else np.asarray(extra).astype(ld)
    tiny = ld(np.finfo(np.float64).tiny)

    def over(sl):
        return float(_norm(err[sl]) / (max(_norm(env[sl]), _norm(fl[sl])) + _norm(ex[sl]) + tiny))

    entry = float(np.max(err / (np.maximum(env, fl) + ex + tiny)))
    quad = max(over(slice(h + lo, h + min(lo + 4, d))) for h in (0, d) for lo in range(0, d, 4))
    return over(slice(0, 2 * d)), quad, entry


def value_ratio(got, env, ref, S_mag, u):
    ld = np.longdouble
    return float(abs(ld(got) - ld(ref)) / (max(ld(env), ld(u) * ld(S_mag)) + ld(np.finfo(np.float64).tiny)))


# ---- the documented summation orders, float32 numpy ---------------------------------------------------------------------------------------------
def n_cc(d, M):
    """(column chunks, columns per chunk) of a single call: mf_main_impl's shape rule restated.  More than one chunk: the columns are split
    over gridDim.y workgroups per row quad and k_mf_colreduce adds the chunks' f64 partials."""
    d4 = (d + 3) // 4
    n = 1
    if M > 256 and d4 < 512:
        n = max(1, min((M + 255) // 256, (1024 + d4 - 1) // d4))
    cols = ((M + n - 1) // n + 255) // 256 * 256
    return (M + cols - 1) // cols, cols


def _workgroup_sum(A, cols):
    """Row sums of the float32 d x M array A the way a row quad's workgroups are documented to form them: per chunk of `cols` columns each
    of 256 threads adds columns tid, tid + 256, ... sequentially in float32, a pairwise tree over the 64 lanes of a wave in float32, the
    four waves and then the chunks in float64.  (d) float64."""
    d, M = A.shape
    total = np.zeros(d, dtype=np.float64)
    for lo in range(0, M, cols):
        chunk = A[:, lo:min(lo + cols, M)]
        K = (chunk.shape[1] + 255) // 256
        pad = np.zeros((d, K * 256), dtype=np.float32)
        pad[:, :chunk.shape[1]] = chunk
        pad = pad.reshape(d, K, 256)
        acc = pad[:, 0].copy()
        for k in range(1, K):
            acc = acc + pad[:, k]
        acc = acc.reshape(d, 4, 64)
        while acc.shape[2] > 1:
            acc = acc[:, :, 0::2] + acc[:, :, 1::2]
        waves = acc[:, :, 0].astype(np.float64)
        part = waves[:, 0]
        for j in range(1, 4):
            part = part + waves[:, j]
        total = total + part
    return total


FAULTS = ("drop_column", "drop_last_chunk", "drop_stl", "wrong_sigma", "local_count")


def emulate(params, d, tgt, eps, ent, route, fault=None):
    """dict(value, grad) in float32 of the diagonal-target estimate with the DOCUMENTED arithmetic of csrc/kernels_meanfield.hip:
    z = fma(sigma, eps, mu), u = (z - m) (1 / s), g = -u (1 / s), W = g + eps (1 / sigma) under sticking the landing; the row sums of
    _workgroup_sum; the entries finished in float64 by mf_grad_entry (-sum / M, minus direct / sigma on the scale rows) and rounded once.
    route: "single" (one chunk: k_mf_main with n_cc == 1), "split" (chunks of n_cc(d, M) columns: k_mf_main + k_mf_colreduce) or "loop" (one
    chunk however large M is: k_mf_sgd_loop, sixteen sequential terms per thread at M = 4096).
    fault: None, or one of
        ("drop_column", row, column)   one sample column left out of one row's two sums
        ("drop_last_chunk",)           the last chunk's columns left out of the last row quad (route "split")
        ("drop_stl", row)              the eps / sigma term left out of one row
        ("wrong_sigma",)               row d - 1 computed with row d - 2's sigma
        ("local_count", quad)          one row quad divides by the first chunk's column count instead of M (route "split")"""
    if not isinstance(tgt, O.DiagNormalTarget):
        raise TypeError(type(tgt))
    f32 = np.float32
    p = np.asarray(params).astype(f32)
    mu, sg = p[:d].copy(), p[d:2 * d].copy()
    E = np.asarray(eps).astype(f32)
    M = E.shape[1]
    chunks, cols = n_cc(d, M) if route == "split" else (1, max(M, 1))
    if route == "split" and chunks == 1:
        raise ValueError("this shape does not split its columns")
    kind = fault[0] if fault else None
    sg_used = sg.copy()
    if kind == "wrong_sigma":
        sg_used[d - 1] = sg[d - 2]
    tm = tgt.mean.astype(f32)
    tis = (1.0 / tgt.std.astype(f32).astype(np.float64)).astype(f32)
    Z = (mu.astype(np.float64)[:, None] + sg_used.astype(np.float64)[:, None] * E.astype(np.float64)).astype(f32)   # one fused multiply-add
    U = (Z - tm[:, None]) * tis[:, None]
    W = -U * tis[:, None]
    if ent in STL:
        X = E * (f32(1.0) / sg_used)[:, None]
        if kind == "drop_stl":
            X[fault[1]] = 0.0
        W = W + X
    WE = W * E
    if kind == "drop_column":
        W[fault[1], fault[2]] = WE[fault[1], fault[2]] = 0.0
    if kind == "drop_last_chunk":
        if chunks == 1:
            raise ValueError("drop_last_chunk needs the split route")
        W[4 * ((d - 1) // 4):, (chunks - 1) * cols:] = 0.0
        WE[4 * ((d - 1) // 4):, (chunks - 1) * cols:] = 0.0
    inv_m = np.full(d, 1.0 / M)
    if kind == "local_count":
        if chunks == 1:
            raise ValueError("local_count needs the split route")
        inv_m[4 * fault[1]:4 * fault[1] + 4] = 1.0 / min(cols, M)
    sgd = sg_used.astype(np.float64)
    g_mu = -_workgroup_sum(W, cols) * inv_m
    g_sg = -_workgroup_sum(WE, cols) * inv_m - DIRECT[ent] / sgd
    # the value: a row quad's workgroup adds the ell terms of its four rows per column, rows first; every partial in float64 from there
    d4 = (d + 3) // 4
    T = np.zeros((4 * d4, M), dtype=f32)
    T[:d] = f32(-0.5) * U * U
    H = np.zeros((4 * d4, M), dtype=f32)
    H[:d] = f32(0.5) * E * E
    quad = lambda A: ((A[0::4] + A[1::4]) + A[2::4]) + A[3::4]
    s_ell = float(np.sum(_workgroup_sum(quad(T), cols)))
    s_he = float(np.sum(_workgroup_sum(quad(H), cols)))
    const = -float(np.sum(np.log(tgt.std.astype(f32).astype(np.float64)))) - 0.5 * d * LOG2PI
    logdet = float(np.sum(np.log(sgd)))
    entropy = (d * 0.5 * (1.0 + LOG2PI) if ent in CLOSED else s_he / M + 0.5 * d * LOG2PI) + logdet
    return dict(value=f32(-((s_ell + M * const) / M + entropy)), grad=np.concatenate([g_mu, g_sg]).astype(f32))
