"""Reference of the low-rank Gaussian family for the tests: the reference package's own expressions restated in float64 torch
(src/families/location_scale_low_rank.jl, src/algorithms/entropy.jl, src/algorithms/repgradelbo.jl), gradients by autograd, and a
numpy Woodbury evaluation in a chosen dtype -- the yardstick the device kernels are held to.

Parameters: [m (d); D (d); vec U (d x r, column-major)].  Draws: `eps` ((d + r) x M), rows 0 .. d-1 = u1, rows d .. d+r-1 = u2.
Targets are the oracle's (oracle/oracle.py: logdensity_and_gradient on a float64 column).

The second half is the per-entry criterion of tests/test_gpu_lowrank_yardstick.py and tests/test_lowrank_ref_host.py -- a helper, not a
test, and no code of the kernels; tests/meanfield_ref.py (targets in a chosen type, orders, value_ratio) and tests/solve_ref.py are reused:
    classes             the parameter classes (mu, D, U, m, s) the kernels are held on
    reference           the Woodbury evaluation with every step in one type: np.float64 for a float32 context, np.longdouble for a float64
                        context (a plain r x r Cholesky, two triangular solves and the logdet from the factor's diagonal: numpy's linalg
                        does not take np.longdouble)
    yardstick           the same evaluation with the precisions the header of csrc/kernels_lowrank.hip and DESIGN.md "Low-rank family"
                        document, with an optional permutation of the sample columns before every sum over M.  (woodbury_eval above, every
                        array in one type, stays for tests/test_gpu_lowrank.py)
    envelope            per entry the largest |yard_k - ref| over the identity order and N_PERM seeded permutations
    magnitude           S_i: the expression of every entry in float64 with every operand replaced by its absolute value and every
                        subtraction by an addition -- the first-order rounding scale, the floor of the criterion
    ratios, value_ratio the criterion: entry, block (what one VJP workgroup owns) and whole-gradient ratios
    stages              the launchers' shape rules restated
    emulate             the yardstick's arithmetic with one injectable fault

Why an envelope and a floor: tests/meanfield_ref.py.  Here every sum over M is float64 on the device, so the eight orders differ by far
less than the float32 roundings of E, Z, t, V and G that they share; the envelope is then nearly ONE evaluation's error per entry, often
near zero, and the floor u S_i -- one rounding of the largest intermediate -- is what carries the criterion on most entries.

S_i (za = |m| + D |u1| + |U| |u2| is the magnitude of z; Wa that of grad log pi, per target as in tests/meanfield_ref.py; `mean` is over
the samples; |A^-1|, |U|, |x|, |t| are entrywise; cH = 1, 0, 1, 0, -1 for the entropy kinds 0 .. 4):
    Va                  (|t| + |U| |x| / D) / D                                  the magnitude of V = D^-1 (t - D^-1 U x)
    cotangent Ca        Wa (closed-form kinds, and the first product of kind 2);  Wa + Va (kinds 3, 4);  Va with a1 -> |u1| + D Va,
                        a2 -> |u2| + |x| (the second product of kind 2)
    S(dm_i)             mean Ca
    S(dD_i)             mean Ca |a1| + |cH| (1 / D_i + (|U| |A^-1| |U'|)_ii / D_i^3)
    S(dU_ik)            mean Ca |a2_k| + |cH| (|U| |A^-1|)_ik / D_i^2
    S(value)            the same substitution in -(mean ell + H) or -(mean ell) + mean log q: mean ell_a + d/2 (1 + log 2 pi) or d/2 log 2 pi
                        + sum |log D| + sum |log L_jj| and, for log q, 1/2 (|t|^2 + |s|' |x|) for the quadratic form"""
import numpy as np
import torch

from tests import meanfield_ref as Mf
from tests import solve_ref as S

LOG2PI = float(np.log(2.0 * np.pi))
CLOSED_FORM, CLOSED_FORM_ZERO_GRAD, MONTE_CARLO, STL, STL_ZERO_GRAD = range(5)


def split(params, d, r):
    """(m, D, U) views of the flat parameter vector (numpy or torch)."""
    U = params[2 * d:].reshape(r, d).T if isinstance(params, torch.Tensor) else params[2 * d:].reshape(d, r, order="F")
    return params[:d], params[d:2 * d], U


# ---- the literal reference expressions (torch, float64) ----------------------------------------------------------------------------
def entropy(m, D, U):
    """location_scale_low_rank.jl:34-43 with dist = Normal(0, 1): n entropy(dist) + (2 sum log D + logdet(I + U' (U ./ D^2))) / 2."""
    n = m.shape[0]
    UtDinvU = U.T @ (U / (D * D)[:, None])
    logdet_sigma = 2.0 * torch.sum(torch.log(D)) + torch.logdet(torch.eye(U.shape[1], dtype=U.dtype) + UtDinvU)
    return n * 0.5 * (1.0 + LOG2PI) + logdet_sigma / 2.0


def logpdf(m, D, U, z):
    """location_scale_low_rank.jl:45-68, the differentiable path: cholesky(Diagonal(D .* D) + U U'); mean(dist) = 0.
    z: one sample (d) or the samples as columns (d x M -> M values; the factor is the same for every column)."""
    L = torch.linalg.cholesky(torch.diag(D * D) + U @ U.T)
    zc = z[:, None] if z.dim() == 1 else z
    w = torch.linalg.solve_triangular(L, zc - m[:, None], upper=False)
    out = torch.sum(-0.5 * w * w - 0.5 * LOG2PI, dim=0) - torch.sum(torch.log(torch.diagonal(L)))
    return out[0] if z.dim() == 1 else out


def rand(m, D, U, eps):
    """location_scale_low_rank.jl:79-86: scale_diag .* u_diag + scale_factors * u_fact .+ location."""
    d = m.shape[0]
    return D[:, None] * eps[:d] + U @ eps[d:] + m[:, None]


class _Target(torch.autograd.Function):
    """mean-free per-column log density of an oracle target, differentiable through its own gradient."""

    @staticmethod
    def forward(ctx, Z, tgt):
        Zn = Z.detach().numpy()
        ell, G = np.empty(Zn.shape[1]), np.empty_like(Zn)
        for k in range(Zn.shape[1]):
            ell[k], G[:, k] = tgt.logdensity_and_gradient(Zn[:, k].copy())
        ctx.save_for_backward(torch.from_numpy(G))
        return torch.from_numpy(ell)

    @staticmethod
    def backward(ctx, g):
        (G,) = ctx.saved_tensors
        return G * g[None, :], None


def estimate_entropy(kind, Z, q, q_stop):
    """src/algorithms/entropy.jl; q, q_stop = (m, D, U)."""
    if kind == CLOSED_FORM:
        return entropy(*q)
    if kind == CLOSED_FORM_ZERO_GRAD:
        return entropy(*q_stop)
    if kind == MONTE_CARLO:
        return torch.mean(-logpdf(*q, Z))
    stl = torch.mean(-logpdf(*q_stop, Z))
    if kind == STL:
        return stl
    if kind == STL_ZERO_GRAD:
        return stl - entropy(*q) + entropy(*q_stop)
    raise ValueError(kind)


def forward(params, d, r, tgt, eps, kind):
    """estimate_repgradelbo_ad_forward (repgradelbo.jl:142-149): -(energy + entropy), q_stop = the same parameters detached (:162)."""
    q = split(params, d, r)
    q_stop = split(params.detach(), d, r)
    Z = rand(*q, eps)
    energy = torch.mean(_Target.apply(Z, tgt))
    return -(energy + estimate_entropy(kind, Z, q, q_stop)), Z


def estimate_gradient(params, d, r, tgt, eps, kind):
    """dict(value, grad, Z): the float64 reference of mivi_estimate_gradient on the low-rank family."""
    p = torch.tensor(np.asarray(params, dtype=np.float64), requires_grad=True)
    e = torch.tensor(np.asarray(eps, dtype=np.float64))
    val, Z = forward(p, d, r, tgt, e, kind)
    (g,) = torch.autograd.grad(val, p)
    return dict(value=float(val.detach()), grad=g.numpy().copy(), Z=Z.detach().numpy().copy())


def estimate_objective(params, d, r, tgt, eps, kind):
    """estimate_objective (repgradelbo.jl:112-118): the value with q_stop = q."""
    with torch.no_grad():
        p = torch.tensor(np.asarray(params, dtype=np.float64))
        Z = rand(*split(p, d, r), torch.tensor(np.asarray(eps, dtype=np.float64)))
        ell = np.array([tgt.logdensity(Z[:, k].numpy().copy()) for k in range(Z.shape[1])])
        q = split(p, d, r)
        return float(-(ell.mean() + estimate_entropy(kind, Z, q, q)))


# ---- the Woodbury evaluation (numpy, dtype of choice): what the device kernels compute ------------------------------------------------
def woodbury_logq(params, d, r, eps, dtype=np.float64):
    """(log q per column, V = Sigma^-1 (z - m), x = A^-1 s) by Woodbury with A = I + U' D^-2 U, every array in `dtype`."""
    p = np.asarray(params, dtype=dtype)
    m, D, U = split(p, d, r)
    e = np.asarray(eps, dtype=dtype)
    u1, u2 = e[:d], e[d:]
    Dc = D[:, None]
    A = np.eye(r, dtype=dtype) + U.T @ (U / (Dc * Dc))
    t = u1 + (U @ u2) / Dc
    s = U.T @ (t / Dc)
    x = np.linalg.solve(A, s).astype(dtype)
    logdet_a = dtype(np.linalg.slogdet(A)[1])
    quad = np.sum(t * t, axis=0) - np.sum(s * x, axis=0)
    logq = dtype(-0.5 * d * LOG2PI) - np.sum(np.log(D)) - dtype(0.5) * logdet_a - dtype(0.5) * quad
    V = (t - (U @ x) / Dc) / Dc
    return logq, V, x


def woodbury_eval(params, d, r, G, ell, eps, kind, dtype=np.float64):
    """dict(value, grad) of one estimate from G = grad log pi (d x M) and ell (M) at the samples, in `dtype`: the closed-form entropy and
    its gradient through A^-1, log q and V by Woodbury, the three cotangent products of the VJP."""
    p = np.asarray(params, dtype=dtype)
    m, D, U = split(p, d, r)
    e = np.asarray(eps, dtype=dtype)
    G, ell = np.asarray(G, dtype=dtype), np.asarray(ell, dtype=dtype)
    u1, u2 = e[:d], e[d:]
    M = e.shape[1]
    Dc = D[:, None]
    A = np.eye(r, dtype=dtype) + U.T @ (U / (Dc * Dc))
    Ainv = np.linalg.inv(A).astype(dtype)
    H = dtype(0.5 * d * (1.0 + LOG2PI)) + np.sum(np.log(D)) + dtype(0.5) * dtype(np.linalg.slogdet(A)[1])
    UA = U @ Ainv
    dH_U = UA / (Dc * Dc)
    dH_D = 1 / D - np.sum(UA * U, axis=1) / D ** 3

    def vjp(C, a1, a2):
        return C.mean(axis=1), (C * a1).mean(axis=1), (C @ a2.T) / dtype(M)

    closed = kind in (CLOSED_FORM, CLOSED_FORM_ZERO_GRAD)
    if closed:
        value = -ell.mean() - H
        gm, gD, gU = vjp(G, u1, u2)
        if kind == CLOSED_FORM:
            gD, gU = gD + dH_D, gU + dH_U
    else:
        logq, V, x = woodbury_logq(p, d, r, e, dtype)
        value = -ell.mean() + logq.mean()
        if kind == MONTE_CARLO:
            gm, gD, gU = vjp(G, u1, u2)
            _, vD, vU = vjp(V, u1 - Dc * V, u2 - U.T @ V)
            gD, gU = gD + vD + dH_D, gU + vU + dH_U
        else:
            gm, gD, gU = vjp(G + V, u1, u2)
            if kind == STL_ZERO_GRAD:
                gD, gU = gD - dH_D, gU - dH_U
    grad = -np.concatenate([gm, gD, gU.reshape(-1, order="F")])
    return dict(value=float(value), grad=grad.astype(np.float64))


# ======================================================================================================================================
# The per-entry criterion of tests/test_gpu_lowrank_yardstick.py and tests/test_lowrank_ref_host.py (no code of the kernels)
# ======================================================================================================================================
CLASSES = ("default", "graded", "steep", "zero", "far")
CLOSED = (CLOSED_FORM, CLOSED_FORM_ZERO_GRAD)
STLS = (STL, STL_ZERO_GRAD)
DIRECT = S.DIRECT                      # the coefficient cH of the closed-form entropy's gradient per entropy kind
N_PERM, U32, U64, wider, orders = Mf.N_PERM, Mf.U32, Mf.U64, Mf.wider, Mf.orders
ROWS_SAMPLE, ROWS_VJP, COLS_VJP, MAX_SLICES = 256, 64, 16, 8   # rows per workgroup of k_lowr_sample / k_lowr_xv, of k_lowr_vjp; its factor columns; kLowrMaxSlices
FAULTS = ("drop_column", "drop_slice", "row_block_1_keeps_t", "clamped_factor_column", "gram_f32", "logq_from_block_1")


def classes(kind, d, r, rng):
    """(mu, D, U, m, s) in float64 (the caller casts to the context's dtype); the target is the diagonal Gaussian N(m, s^2) unless the case
    brings its own:
        default  tests/test_gpu_lowrank.py make_lowrank / make_problem: mu, m ~ N(0, 1), D ~ U(0.5, 1.5), U ~ 0.7 N(0, 1), s ~ U(0.5, 2)
        graded   D = 10^U(-2, 2), U_ik = +-D_i 10^U(-1, 1), s = 10^U(-1, 1): entries spanning nine decades
        steep    default with D scaled by 1e-2: dominant factors, cond(A) about 1e4 |U|^2, t - D^-1 U x cancels
        zero     U = 0, the docs' initial point (A = I)
        far      mu = m + 1e3 N(0, 1)"""
    mu, D, U = rng.normal(size=d), rng.uniform(0.5, 1.5, size=d), 0.7 * rng.normal(size=(d, r))
    m, s = rng.normal(size=d), rng.uniform(0.5, 2.0, size=d)
    if kind == "graded":
        D = 10.0 ** rng.uniform(-2.0, 2.0, size=d)
        U = rng.choice([-1.0, 1.0], size=(d, r)) * D[:, None] * 10.0 ** rng.uniform(-1.0, 1.0, size=(d, r))
        s = 10.0 ** rng.uniform(-1.0, 1.0, size=d)
    elif kind == "steep":
        D = 1e-2 * D
    elif kind == "zero":
        U = np.zeros((d, r))
    elif kind == "far":
        mu = m + 1e3 * rng.normal(size=d)
    elif kind != "default":
        raise ValueError(kind)
    return mu, D, U, m, s


def flat(mu, D, U, dtype=np.float64):
    return np.concatenate([mu, D, np.asarray(U).reshape(-1, order="F")]).astype(dtype)


# ---- r x r linear algebra in any dtype (numpy's linalg does not take np.longdouble), r <= 64 ---------------------------------------------
def _cholesky(A):
    r = A.shape[0]
    L = np.zeros_like(A)
    for j in range(r):
        L[j, j] = np.sqrt(A[j, j] - np.sum(L[j, :j] * L[j, :j], dtype=A.dtype))
        if j + 1 < r:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _solve_lower(L, B):
    X = np.array(B, dtype=L.dtype, copy=True)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def _solve_lower_t(L, B):
    X = np.array(B, dtype=L.dtype, copy=True)
    for i in range(L.shape[0] - 1, -1, -1):
        X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


# ---- one evaluation: the per-column pieces, then the sums over the samples ---------------------------------------------------------------
def lowr_vjp_slices(M):
    return max(1, min((M + 31) // 32, MAX_SLICES))


def _slice_bounds(M):
    ns = lowr_vjp_slices(M)
    mb = (M + ns - 1) // ns
    return [(z * mb, min((z + 1) * mb, M)) for z in range(ns)]


def _pieces(params, d, r, tgt, eps, kind, store, acc, fault=None, variant=False):
    """Everything of one estimate but the sums over the samples.  store: the type of E, Z, t, V, G and of the K = r sample product; acc: the
    type of everything of size r and of every sum over d (the reference: store = acc).  variant: the independent evaluation of the host
    test -- the K = r product accumulated column by column, divisions by D where this multiplies by 1 / D, A^-1 by np.linalg.inv."""
    store, acc = np.dtype(store).type, np.dtype(acc).type
    fk = fault[0] if fault else None
    p = np.asarray(params).astype(store)
    m, D, U = split(p, d, r)
    E = np.asarray(eps).astype(store)
    u1, u2 = E[:d], E[d:]
    M = E.shape[1]
    Dc = D[:, None]
    if variant:
        Bp = np.zeros((d, M), dtype=store)
        for k in range(r):
            Bp = (Bp + U[:, k:k + 1] * u2[k:k + 1]).astype(store)
    else:
        Bp = (U @ u2).astype(store)
    Z = (Dc * u1 + Bp + m[:, None]).astype(store)
    ell, G = Mf._target(tgt, Z, store)
    Da, Ua = D.astype(acc), U.astype(acc)
    Dac = Da[:, None]
    idc = acc(1.0) / Dac
    gt = np.float32 if fk == "gram_f32" else acc
    Ug = U.astype(gt) * (gt(1.0) / D.astype(gt))[:, None]
    A = (np.eye(r, dtype=gt) + Ug.T @ Ug).astype(acc)
    if variant:
        Ainv, hld = np.linalg.inv(A), acc(0.5 * np.linalg.slogdet(A)[1])
    else:
        L = _cholesky(A)
        Ainv = _solve_lower_t(L, _solve_lower(L, np.eye(r, dtype=acc)))
        hld = np.sum(np.log(np.diag(L)), dtype=acc)
    sld = np.sum(np.log(Da), dtype=acc)
    UA = Ua @ Ainv
    out = dict(M=M, kind=kind, acc=acc, ell=ell.astype(acc), Z=Z, H=acc(0.5 * d * (1.0 + LOG2PI)) + sld + hld,
               dH_D=(idc[:, 0] - np.sum(UA * Ua, axis=1, dtype=acc) * idc[:, 0] ** 3) if not variant else (1 / Da - np.sum(UA * Ua, axis=1) / Da / Da / Da),
               dH_U=UA * idc * idc if not variant else UA / Dac / Dac, logq=None)
    u1a, u2a, Ga = u1.astype(acc), u2.astype(acc), G.astype(acc)
    if kind in CLOSED:
        out["trip"] = [(Ga, u1a, u2a, True)]
        return out
    t = (u1 + Bp / Dc).astype(store)
    ta = t.astype(acc)
    s = (Ua * idc).T @ ta if not variant else (Ua / Dac).T @ ta
    x = Ainv @ s
    logq = acc(-0.5 * d * LOG2PI) - sld - hld - acc(0.5) * (np.sum(ta * ta, axis=0, dtype=acc) - np.sum(s * x, axis=0, dtype=acc))
    V = ((ta - idc * (Ua @ x)) * idc if not variant else (ta - (Ua @ x) / Dac) / Dac).astype(store)
    if fk == "row_block_1_keeps_t":
        V[ROWS_SAMPLE:] = t[ROWS_SAMPLE:]
    if fk == "logq_from_block_1":
        logq[8:] = 0.0
    Va = V.astype(acc)
    out["logq"] = logq
    out["trip"] = [(Ga, u1a, u2a, True), (Va, u1a - Dac * Va, u2a - x, False)] if kind == MONTE_CARLO else [(Ga + Va, u1a, u2a, True)]
    return out


def _assemble(pc, d, r, order=None, fault=None):
    """dict(value, grad) from the pieces: the sums over the samples in pc's accumulation type, the columns permuted by `order` first"""
    acc, M, kind = pc["acc"], pc["M"], pc["kind"]
    fk = fault[0] if fault else None
    base = np.arange(M) if order is None else np.asarray(order)
    keep = base
    if fk == "drop_slice":
        lo, hi = _slice_bounds(M)[-1]
        keep = keep[(keep < lo) | (keep >= hi)]
    gm, gD, gU = np.zeros(d, dtype=acc), np.zeros(d, dtype=acc), np.zeros((d, r), dtype=acc)
    for C, a1, a2, with_m in pc["trip"]:
        Ck, a1k, a2k = np.ascontiguousarray(C[:, keep]), np.ascontiguousarray(a1[:, keep]), np.ascontiguousarray(a2[:, keep])
        if with_m:
            gm = gm + np.sum(Ck, axis=1, dtype=acc)
        gD = gD + np.sum(Ck * a1k, axis=1, dtype=acc)
        gU = gU + Ck @ a2k.T
        if fk == "drop_column":   # the last column of slice fault[2], lost from the 64-row block fault[1] (its dm, dD and first factor-column block)
            rows, c = slice(fault[1] * ROWS_VJP, min((fault[1] + 1) * ROWS_VJP, d)), _slice_bounds(M)[fault[2]][1] - 1
            if with_m:
                gm[rows] -= C[rows, c]
            gD[rows] -= C[rows, c] * a1[rows, c]
            gU[rows, :COLS_VJP] -= C[rows, c:c + 1] * a2[None, :COLS_VJP, c]
    if fk == "clamped_factor_column":
        gU[:, r - 1] *= 2.0
    cH, Mt = acc(DIRECT[kind]), acc(M)
    grad = np.concatenate([-gm / Mt, -gD / Mt - cH * pc["dH_D"], (-gU / Mt - cH * pc["dH_U"]).reshape(-1, order="F")])
    mean_ell = np.sum(pc["ell"][base], dtype=acc) / Mt
    value = -(mean_ell + pc["H"]) if kind in CLOSED else -mean_ell + np.sum(pc["logq"][base], dtype=acc) / Mt
    return dict(value=value, grad=grad)


def reference(params, d, r, tgt, eps, kind, dtype):
    """dict(value, grad): the Woodbury evaluation with every step in `dtype` -- np.float64 for a float32 context, np.longdouble for a
    float64 context (wider(context dtype))."""
    return _assemble(_pieces(params, d, r, tgt, eps, kind, dtype, dtype), d, r)


def _store(out, dtype):
    """the device rounds the finished entries and the value once to the context's type"""
    return dict(value=np.dtype(dtype).type(out["value"]), grad=out["grad"].astype(dtype))


def yardstick(params, d, r, tgt, eps, kind, dtype, order=None):
    """the same evaluation with the precisions the header of csrc/kernels_lowrank.hip and DESIGN.md "Low-rank family" document: E, Z, t, V,
    G, the target and the K = r sample product in `dtype`; everything of size r and every sum over d or M in float64; the results rounded
    once to `dtype`.  order: a permutation of the sample columns applied before every sum over M."""
    return _store(_assemble(_pieces(params, d, r, tgt, eps, kind, dtype, np.float64), d, r, order), dtype)


def emulate(params, d, r, tgt, eps, kind, dtype=np.float32, fault=None, order=None, variant=False):
    """the yardstick's arithmetic with one injectable fault -- one for each documented mechanism the GPU file's shapes exist for:
        ("drop_column", b, z)        the last column of slice z lost from the 64-row block b (its dm, dD and first 16 factor columns)
        ("drop_slice",)              the last slice's partials never added (slice 7 of 8 where M > 224)
        ("row_block_1_keeps_t",)     V = t on rows >= 256: only row block 0 of k_lowr_xv wrote V
        ("clamped_factor_column",)   column r - 1's sums stored twice: dU[:, r - 1]'s sample part doubled
        ("gram_f32",)                A = I + U' D^-2 U accumulated in float32 (what "in the element type" is on a float32 context; the host
                                     test scores it on a float64 context, where the header's "f64 for either element type" is at stake --
                                     on a float32 context it stays inside the criterion, tests/test_lowrank_ref_host.py has the figures)
        ("logq_from_block_1",)       log q of the columns >= 8 taken as zero: only the first column tile of row block 0 wrote it
    variant: the host test's independent evaluation (see _pieces)"""
    return _store(_assemble(_pieces(params, d, r, tgt, eps, kind, dtype, np.float64, fault, variant), d, r, order, fault), dtype)


def envelope(params, d, r, tgt, eps, kind, dtype=np.float32, ref=None):
    """dict(grad, value): per entry max_k |yard_k - ref| over the identity order and N_PERM seeded permutations of the sample columns"""
    wide = wider(dtype)
    ref = reference(params, d, r, tgt, eps, kind, wide) if ref is None else ref
    pc = _pieces(params, d, r, tgt, eps, kind, dtype, np.float64)
    env_g, env_v = np.zeros(ref["grad"].size, dtype=wide), wide(0.0)
    for o in orders(np.asarray(eps).shape[1]):
        y = _store(_assemble(pc, d, r, o), dtype)
        env_g = np.maximum(env_g, np.abs(y["grad"].astype(wide) - ref["grad"]))
        env_v = max(env_v, abs(wide(y["value"]) - ref["value"]))
    return dict(grad=env_g, value=env_v)


def magnitude(params, d, r, tgt, eps, kind):
    """dict(grad, value): S_i of every gradient entry and of the value in float64 (the table of the module docstring)"""
    p = np.asarray(params, dtype=np.float64)
    m, D, U = split(p, d, r)
    E = np.asarray(eps, dtype=np.float64)
    u1, u2 = E[:d], E[d:]
    Dc, Ua, u1a, u2a = D[:, None], np.abs(U), np.abs(u1), np.abs(u2)
    za = np.abs(m)[:, None] + Dc * u1a + Ua @ u2a
    ell_a, Wa = Mf._magnitude_target(tgt, za, Dc * u1 + U @ u2 + m[:, None], d)
    A = np.eye(r) + (U / Dc).T @ (U / Dc)
    Ainv_a = np.abs(np.linalg.inv(A))
    hld_a = float(np.sum(np.abs(np.log(np.diag(np.linalg.cholesky(A))))))
    sld_a = float(np.sum(np.abs(np.log(D))))
    UAa = Ua @ Ainv_a
    cH = abs(DIRECT[kind])
    dD = cH * (1.0 / D + np.sum(UAa * Ua, axis=1) / D ** 3)
    dU = cH * UAa / (Dc * Dc)
    if kind in CLOSED:
        gm, gD, gU = Wa.mean(axis=1), (Wa * u1a).mean(axis=1), Wa @ u2a.T / E.shape[1]
        value = float(np.mean(ell_a)) + 0.5 * d * (1.0 + LOG2PI) + sld_a + hld_a
    else:
        t = u1 + (U @ u2) / Dc
        s = (U / Dc).T @ t
        x = np.linalg.solve(A, s)
        xa = np.abs(x)
        Va = (np.abs(t) + (Ua @ xa) / Dc) / Dc
        if kind == MONTE_CARLO:
            gm = Wa.mean(axis=1)
            gD = (Wa * u1a + Va * (u1a + Dc * Va)).mean(axis=1)
            gU = (Wa @ u2a.T + Va @ (u2a + xa).T) / E.shape[1]
        else:
            Ca = Wa + Va
            gm, gD, gU = Ca.mean(axis=1), (Ca * u1a).mean(axis=1), Ca @ u2a.T / E.shape[1]
        logq_a = 0.5 * d * LOG2PI + sld_a + hld_a + 0.5 * (np.sum(t * t, axis=0) + np.sum(np.abs(s) * xa, axis=0))
        value = float(np.mean(ell_a) + np.mean(logq_a))
    return dict(grad=np.concatenate([gm, gD + dD, (gU + dU).reshape(-1, order="F")]), value=value)


# ---- the criterion -----------------------------------------------------------------------------------------------------------------------
def blocks(d, r):
    """the index sets one VJP workgroup owns: 64 consecutive rows of dm, of dD and of each factor column"""
    return [slice(h * d + lo, h * d + min(lo + ROWS_VJP, d)) for h in range(2 + r) for lo in range(0, d, ROWS_VJP)]


def ratios(got, env, ref, S_mag, d, r, u, extra=None):
    """(whole, block, entry) of a low-rank gradient of 2d + dr entries, all differences in np.longdouble:
        entry  the worst |got_i - ref_i| / (max(env_i, u S_i) + extra_i)
        block  the same quotient of l2 norms over each set of `blocks(d, r)`, the worst
        whole  the same over all entries
    extra: an allowance added to every denominator (the rounding of a stored parameter when the gradient is recovered from a Descent step)"""
    ld = np.longdouble
    err = np.abs(np.asarray(got).astype(ld) - np.asarray(ref).astype(ld))
    e, fl = np.asarray(env).astype(ld), ld(u) * np.asarray(S_mag).astype(ld)
    ex = np.zeros(err.size, dtype=ld) if extra is None else np.asarray(extra).astype(ld)
    tiny = ld(np.finfo(np.float64).tiny)

    def over(sl):
        return float(Mf._norm(err[sl]) / (max(Mf._norm(e[sl]), Mf._norm(fl[sl])) + Mf._norm(ex[sl]) + tiny))

    entry = float(np.max(err / (np.maximum(e, fl) + ex + tiny)))
    return over(slice(0, err.size)), max(over(sl) for sl in blocks(d, r)), entry


value_ratio = Mf.value_ratio


def stages(d, r, M):
    """the shape rules of csrc/kernels_lowrank.hip's launchers restated: which route and how many blocks, passes, slices and tails a shape
    (d, r, M) takes"""
    ns = lowr_vjp_slices(M)
    bounds = _slice_bounds(M)
    return dict(gram_kernel=r > 4,                                        # k_lowr_gram forms A; else the prep workgroup, one wave per entry
                gram_tiles=(r + 3) // 4, gram_ragged_tile=r > 4 and r % 4 != 0,
                row_blocks_256=(d + 255) // 256,                          # k_lowr_sample, k_lowr_xv; also the passes of every i += 256 loop over d
                passes_64=(d + 63) // 64,                                 # the prep workgroup's own Gram: a wave's passes over d
                row_blocks_64=(d + 63) // 64,                             # k_lowr_vjp
                factor_blocks=(r + COLS_VJP - 1) // COLS_VJP, last_factor_block=r - (r - 1) // COLS_VJP * COLS_VJP,
                cholesky_beyond_16=r > 17,                                # the trailing update's 16 x 16 threads take a second pass
                slices=ns, slice_columns=[hi - lo for lo, hi in bounds],
                column_tiles_8=(M + 7) // 8, last_tile_8=M - (M - 1) // 8 * 8, column_tiles_4=(M + 3) // 4, last_tile_4=M - (M - 1) // 4 * 4,
                philox_tail=(d + r) % 4, u2_straddles_block=d % 4 != 0 and (d % 4) + r > 4)


# the shapes (d, r, M) of tests/test_gpu_lowrank_yardstick.py: the smallest that reach each mechanism (its table; `stages` restates the rules)
SHAPES = [(257, 4, 9), (257, 5, 33), (65, 17, 257), (513, 33, 40), (300, 64, 300), (3, 2, 5), (2, 5, 9), (1, 1, 1)]
