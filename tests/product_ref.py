"""numpy restatement of the three products every estimate of the full-rank family runs -- Z = m + C eps, dC = tril(W eps') / M and, for the
dense-Gaussian target, W = -P (Z - m) -- a helper of the product yardstick tests (tests/test_product_ref_host.py,
tests/test_gpu_product_yardstick.py), not a test.  It reuses tests/solve_ref.py wherever it can.

    scale_matrix            solve_ref.scale_matrix plus the class `colgraded`
    dense_precision         P of the dense-Gaussian target from its stored factor L, as mivi_set_target_dense_gauss forms it
    gradient                oracle.estimate_gradient for the entropy kinds without a solve (0, 1, 2) and both Gaussian targets, in `dtype`:
                            np.float64 is the reference, np.float32 the same expression rounded to float32 at every step (products are numpy
                            float32 matrix products) -- the yardstick
    emulate_f16_products    the gradient with its products formed the way the batch engine is DOCUMENTED to (csrc/fr_planes.h,
                            csrc/kernels_fullrank_batch.hip): two-way f16 planes of power-of-two scaled operands, three products per
                            16-k group, the accumulator re-based at the 128-wide block boundaries; float32 numpy, no code of the kernels
    emulate_bf16x3_products the same for the second-generation single-call kernels (csrc/kernels_fullrank_lds.hip): exact three-way bf16
                            split by truncation, six products per 16-k group, K cut into contiguous runs whose partial tiles are summed
    ratios                  the criterion: solve_ref.block_ratios (whole, worst 64-row block) plus the worst 64-COLUMN block of dC

Both emulations take `drop = (product, term, block)`: the named term (`lo.hi`, `hi.lo`, ...) is left out of the product `sample`, `vjp`
or `dense` -- in every row of its result (block None) or in the rows of one 64-row block of it only."""
import numpy as np
from scipy.linalg import solve_triangular

from oracle import oracle as O
from tests import solve_ref as S

KINDS = S.KINDS + ("colgraded",)
NO_SOLVE = (O.ENT_CLOSED_FORM, O.ENT_CLOSED_FORM_ZERO_GRAD, O.ENT_MONTE_CARLO)
F16_TERMS = (("lo", "hi"), ("hi", "lo"), ("hi", "hi"))                                                       # csrc/fr_planes.h fb_group
BF16X3_TERMS = (("lo", "hi"), ("hi", "lo"), ("mid", "mid"), ("mid", "hi"), ("hi", "mid"), ("hi", "hi"))      # mfma_bf16x3
EPS_SCALE = np.float32(2048.0)                                                                               # kEpsScale


def scale_matrix(kind, d, rng):
    """solve_ref.scale_matrix, and
        colgraded  default diag(10^U(-3, 3)): COLUMNS spanning six decades -- entries of very different size inside one row, the case the
                   planes' per-row scale has to carry"""
    if kind == "colgraded":
        return S._default(d, rng) * (10.0 ** rng.uniform(-3.0, 3.0, size=d))[None, :]
    return S.scale_matrix(kind, d, rng)


# ---- the reference and the yardstick -------------------------------------------------------------------------------------------------------
def dense_precision(L):
    """P = L^-T L^-1 in float64 from the stored lower factor, the way mivi_set_target_dense_gauss forms it (L^-1 by forward substitution,
    then the product); the oracle inverts L L' instead."""
    L = np.tril(np.asarray(L, dtype=np.float64))
    Li = solve_triangular(L, np.eye(L.shape[0]), lower=True, check_finite=False)
    P = Li.T @ Li
    return 0.5 * (P + P.T)


def _target(tgt, Z, dtype, product=None):
    """(log pi(z_m), W = grad log pi(z_m)) for the columns of Z in `dtype`.  Dense target: W = product(P, Z - m) if given, else -(P (Z - m))."""
    if isinstance(tgt, O.DiagNormalTarget):
        return S._diag_target(tgt, Z, dtype)
    d = Z.shape[0]
    P, m = dense_precision(tgt.L).astype(dtype), tgt.mean.astype(dtype)
    R = (Z - m[:, None]).astype(dtype)
    W = (-(P @ R)).astype(dtype) if product is None else product(P, R)
    const = dtype(-np.sum(np.log(np.diag(tgt.L))) - 0.5 * d * S.LOG2PI)
    return (dtype(0.5) * np.sum(R * W, axis=0, dtype=dtype) + const).astype(dtype), W


def _assemble(C, E, ell, g_mu, gC, ent, dtype):
    """value and flat gradient from the estimate's pieces (oracle/oracle.py estimate_gradient), in `dtype`"""
    d, M = E.shape
    diag = np.diag(C)
    logdet = np.sum(np.log(diag), dtype=dtype)
    if ent in (O.ENT_CLOSED_FORM, O.ENT_CLOSED_FORM_ZERO_GRAD):
        entropy = dtype(d * 0.5 * (1.0 + S.LOG2PI)) + logdet
    else:
        entropy = np.mean(dtype(0.5) * np.sum(E * E, axis=0, dtype=dtype), dtype=dtype) + dtype(0.5 * d * S.LOG2PI) + logdet
    gC = gC - dtype(S.DIRECT[ent]) * np.diag(dtype(1.0) / diag)
    grad = np.concatenate([g_mu, gC.reshape(-1, order="F")]).astype(dtype)
    return dict(value=dtype(-(np.mean(ell, dtype=dtype) + entropy)), grad=grad)


def gradient(params, d, tgt, eps, ent, dtype=np.float64):
    """dict(value, grad) of oracle.estimate_gradient(params, d, FULLRANK, tgt, eps, ent), ent in (0, 1, 2), for a DiagNormalTarget
    (solve_ref.stl_gradient) or a DenseNormalTarget (W = -P (Z - m), P = dense_precision(L) rounded to `dtype`)."""
    if ent not in NO_SOLVE:
        raise ValueError(ent)
    if isinstance(tgt, O.DiagNormalTarget):
        r = S.stl_gradient(params, d, tgt, eps, ent, dtype)
        return dict(value=r["value"], grad=r["grad"])
    dtype = np.dtype(dtype).type
    mu, C = S._split(params, d, dtype)
    E = np.asarray(eps).astype(dtype)
    M = E.shape[1]
    ell, W = _target(tgt, C @ E + mu[:, None], dtype)
    return _assemble(C, E, ell, -np.sum(W, axis=1, dtype=dtype) / dtype(M), -np.tril(W @ E.T) / dtype(M), ent, dtype)


# ---- emulations of the documented schemes (float32 throughout) ---------------------------------------------------------------------------------
def _chain(acc, A, B, terms, k_lo, k_hi, dropped):
    """acc += A B over k in [k_lo, k_hi), 16 k at a time, the `terms` (plane of A, plane of B) of a group in their order; dropped: None or
    (term name, row slice or None)"""
    for k in range(k_lo, k_hi, 16):
        ke = min(k + 16, k_hi)
        for a, b in terms:
            t = A[a][:, k:ke] @ B[b][k:ke]
            if dropped is not None and dropped[0] == f"{a}.{b}":
                if dropped[1] is None:
                    continue
                t[dropped[1]] = np.float32(0.0)
            acc += t
    return acc


def _dropped(drop, product, terms):
    if drop is None or drop[0] != product:
        return None
    _, term, block = drop
    if term not in [f"{a}.{b}" for a, b in terms]:
        raise ValueError(term)
    return term, (None if block is None else slice(64 * block, 64 * block + 64))


def _planes16(x):
    hi, lo = S._f16_planes(np.ascontiguousarray(x, dtype=np.float32))
    return dict(hi=hi, lo=lo)


def _rebased_product(A_blocks, inv_blocks, B, axis, shape, dropped):
    """sum_b (A_b B_b) inv_b the way the engine is documented to form it (k_fb_vjp, k_fb_prod<FB_DENSE_G>): ONE float32 accumulator in the unit
    of the current block's scale, multiplied at every block boundary by the power-of-two ratio of the neighbouring scales -- clamped to 2^40
    per boundary and 2^80 in all -- and by the last unit's inverse at the end.  A_blocks[b], B[b]: the plane dicts of block b (its own k
    range); inv_blocks[b]: the inverse scales along `axis` of the result (0: per row, 1: per column)."""
    acc = np.zeros(shape, dtype=np.float32)
    wide = (lambda v: v[:, None]) if axis == 0 else (lambda v: v[None, :])
    u, grow = inv_blocks[0].copy(), np.ones_like(inv_blocks[0])
    for b, (Ab, Bb) in enumerate(zip(A_blocks, B)):
        if b:
            with np.errstate(all="ignore"):
                ratio = u / inv_blocks[b]
            ratio = np.where(ratio <= np.float32(2.0 ** 40), ratio, np.float32(2.0 ** 40)).astype(np.float32)
            cap = (ratio > 1.0) & (grow * ratio > np.float32(2.0 ** 80))
            ratio = np.where(cap, np.maximum(np.float32(2.0 ** 80) / grow, np.float32(1.0)), ratio).astype(np.float32)
            grow = np.where(ratio > 1.0, grow * ratio, grow).astype(np.float32)
            acc *= wide(ratio)
            u = (u / ratio).astype(np.float32)
        _chain(acc, Ab, Bb, F16_TERMS, 0, Ab["hi"].shape[1], dropped)
    return acc * wide(u)


def emulate_f16_products(params, d, tgt, eps, ent, drop=None):
    """The float32 gradient with the batch engine's documented arithmetic (csrc/fr_planes.h): every operand element the two-way f16 split
    hi = f16(s x), lo = f16(s x - hi) of its power-of-two scaled value -- s = 2^11 for eps, fb_scale_of(row maximum) for the parameter
    operands tril(C) and P, fb_scale_of(maximum of the tile) per (row, 128-sample block) for W and per (sample, 128-row block) for R = Z - m
    -- and per 16-k group the three products lo.hi, hi.lo, hi.hi accumulated in float32, smallest first.  d/dmu sums hi + lo of W's planes."""
    f32 = np.float32
    mu, C = S._split(params, d, f32)
    E = np.asarray(eps).astype(f32)
    M = E.shape[1]
    Ep = _planes16(E * EPS_SCALE)
    EpT = dict(hi=np.ascontiguousarray(Ep["hi"].T), lo=np.ascontiguousarray(Ep["lo"].T))
    # Z = mu + tril(C) eps: one scale per row of C
    cs = S._pow2_scale(np.max(np.abs(C), axis=1))
    acc = _chain(np.zeros((d, M), dtype=f32), _planes16(C * cs[:, None]), Ep, F16_TERMS, 0, d, _dropped(drop, "sample", F16_TERMS))
    Z = mu[:, None] + acc * ((f32(1.0) / cs) * (f32(1.0) / EPS_SCALE))[:, None]

    def dense_product(P, R):
        # G = -P R: one scale per row of P, one per (sample, 128-row block) of R
        ps = S._pow2_scale(np.max(np.abs(P), axis=1))
        Pp = _planes16(P * ps[:, None])
        A_blocks, B_blocks, inv = [], [], []
        for lo in range(0, d, 128):
            rs = S._pow2_scale(np.max(np.abs(R[lo:lo + 128]), axis=0))
            A_blocks.append({k: v[:, lo:lo + 128] for k, v in Pp.items()})
            B_blocks.append(_planes16(R[lo:lo + 128] * rs[None, :]))
            inv.append((f32(1.0) / rs).astype(f32))
        G = _rebased_product(A_blocks, inv, B_blocks, 1, (d, M), _dropped(drop, "dense", F16_TERMS))
        return (-(G * (f32(1.0) / ps)[:, None])).astype(f32)

    ell, W = _target(tgt, Z.astype(f32), f32, dense_product)
    # dC = tril(W eps'): one scale per (row, 128-sample block) of W, the draws' planes once more
    A_blocks, B_blocks, inv = [], [], []
    g_mu = np.zeros(d, dtype=f32)
    for lo in range(0, M, 128):
        ws = S._pow2_scale(np.max(np.abs(W[:, lo:lo + 128]), axis=1))
        Wp = _planes16(W[:, lo:lo + 128] * ws[:, None])
        A_blocks.append(Wp)
        B_blocks.append({k: v[lo:lo + 128] for k, v in EpT.items()})
        inv.append((f32(1.0) / ws).astype(f32))
        g_mu += np.sum((Wp["hi"] + Wp["lo"]) * inv[-1][:, None], axis=1, dtype=f32)
    acc = _rebased_product(A_blocks, inv, B_blocks, 0, (d, d), _dropped(drop, "vjp", F16_TERMS)) * (f32(1.0) / EPS_SCALE)
    return _assemble(C, E, ell, -g_mu / f32(M), -np.tril(acc) / f32(M), ent, f32)


def _trunc_bf16(x):
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _planes_bf16x3(x):
    """x = hi + mid + lo exactly: three bf16 pieces by truncation, all of one sign (split3_bf16)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = _trunc_bf16(x)
    r = x - hi
    mid = _trunc_bf16(r)
    return dict(hi=hi, mid=mid, lo=_trunc_bf16(r - mid))


def _runs_product(A, B, shape, runs, dropped):
    """A B with K cut into `runs` contiguous runs of 32-k sub-stages, each run its own float32 chain of six-product groups, the partial
    tiles summed in run order (the epilogues of k_fr_prod32 / k_fr_prod64 / k_fr_vjp32 / k_fr_vjp64)"""
    K = A["hi"].shape[1]
    total = np.zeros(shape, dtype=np.float32)
    for part in np.array_split(np.arange(0, K, 32), runs):
        if part.size:
            total += _chain(np.zeros(shape, dtype=np.float32), A, B, BF16X3_TERMS, int(part[0]), min(int(part[-1]) + 32, K), dropped)
    return total


def emulate_bf16x3_products(params, d, tgt, eps, ent, drop=None):
    """The float32 gradient with the second-generation single-call kernels' documented arithmetic (csrc/kernels_fullrank_lds.hip): every
    operand element split exactly into three bf16 pieces by truncation, per 16-k group the six products lo.hi, hi.lo, mid.mid, mid.hi,
    hi.mid, hi.hi accumulated in float32; eight waves share a product tile's K range, four (d M <= 1024 x 512) or eight a VJP tile's."""
    f32 = np.float32
    mu, C = S._split(params, d, f32)
    E = np.asarray(eps).astype(f32)
    M = E.shape[1]
    Ep = _planes_bf16x3(E)
    Z = mu[:, None] + _runs_product(_planes_bf16x3(C), Ep, (d, M), 8, _dropped(drop, "sample", BF16X3_TERMS))

    def dense_product(P, R):
        return (-_runs_product(_planes_bf16x3(P), _planes_bf16x3(R), (d, M), 8, _dropped(drop, "dense", BF16X3_TERMS))).astype(f32)

    ell, W = _target(tgt, Z.astype(f32), f32, dense_product)
    EpT = {k: np.ascontiguousarray(v.T) for k, v in Ep.items()}
    acc = _runs_product(_planes_bf16x3(W), EpT, (d, d), 4 if d * M <= 1024 * 512 else 8, _dropped(drop, "vjp", BF16X3_TERMS))
    return _assemble(C, E, ell, -np.sum(W, axis=1, dtype=f32) / f32(M), -np.tril(acc) / f32(M), ent, f32)


# ---- the criterion -----------------------------------------------------------------------------------------------------------------------------
def ratios(got, yard, ref64, d):
    """(whole, rows, cols) of a flat gradient: solve_ref.block_ratios' two numbers -- the whole gradient and the worst 64-row block of dmu and
    dC -- and the same number over the 64-COLUMN blocks of dC (block_ratios on dC').  A lost 128-sample block or k-stage of the VJP spreads
    over the rows of dC; a lost column block of tril(W eps') stays in its columns, where only this number sees it."""
    whole, rows = S.block_ratios(got, yard, ref64, d)
    t = [np.asarray(a, dtype=np.float64)[d:].reshape(d, d, order="F").T for a in (got, yard, ref64)]
    return whole, rows, S.block_ratios(t[0], t[1], t[2], d)[1]
