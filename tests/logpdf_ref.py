"""numpy restatement of Distributions.logpdf(q, z) at the caller's points for every family and base -- a helper of
tests/test_logpdf_ref_host.py and tests/test_gpu_logpdf.py, not a test.

    logpdf_cols                  (logq (n), U (d x n)) for the columns of Z, every array in `dtype`: np.float64 is the reference, np.float32
                                 the yardstick an f32 context is held against (LAPACK substitution, base terms and sums in float32)
    emulate_forward_block_solve  what csrc/kernels_logpdf.hip (k_lp_fwd16 on k_stl_prep's inverted diagonal blocks) is DOCUMENTED to do,
                                 in numpy (float32 values, float64 sums); no code of the kernel
    emulate_logq                 log q of the emulated solve: the sum of the Gaussian terms accumulated in float64, as the kernel's tail
    points                       the two point sets of a yardstick case
    logq_ratio                   the criterion on log q as an n-vector

Families are the library's codes (0 mean-field, 1 full-rank, 2 low-rank).  A base is None (Normal) or tests/basedist_ref.py's tuple."""
import zlib

import numpy as np
import torch
from scipy.linalg import solve_triangular

from tests import basedist_ref as B
from tests import lowrank_ref as LR
from tests import solve_ref as S

MEANFIELD, FULLRANK, LOWRANK = 0, 1, 2
LOG2PI = float(np.log(2.0 * np.pi))
BLOCK = 32   # rows of a diagonal block of k_lp_fwd16
# the f32 yardstick cases (kind, d, n) of tests/test_gpu_logpdf.py; tests/test_logpdf_ref_host.py shows the criterion admissible on each.
# (2400, 32) is past the size at which 16 columns of X fit LDS: there X lives in the call's f64 scratch.
YARDSTICK_CASES = [(k, d, n) for k in S.KINDS for d, n in ((64, 32), (200, 96), (256, 64), (1024, 32))] + [(k, 2400, 32) for k in ("default", "graded")]


def yardstick_setup(kind, d, dtype=np.float32):
    """(C, mu, params) of a yardstick case in `dtype`: C of class `kind` (tests/solve_ref.py scale_matrix), mu ~ N(0, 1), seeded by the case"""
    rng = np.random.default_rng(zlib.crc32(kind.encode()) + d)
    C = S.scale_matrix(kind, d, rng).astype(dtype)
    mu = rng.normal(size=d).astype(dtype)
    return C, mu, np.concatenate([mu, C.reshape(-1, order="F")])


def _logphi(base, U):
    dt = U.dtype.type
    if base is None:
        return -dt(0.5) * U * U - dt(0.5 * LOG2PI)
    return B.logphi(base, U)


def logpdf_cols(params, d, family, Z, base, dtype, rank=0):
    """(logq, U): location_scale.jl:59-63 -- U = scale \\ (Z - location), logq = sum(logpdf.(dist, U)) - logdet(scale) per column -- with
    every array and sum in `dtype`; low-rank: the literal dense expression of tests/lowrank_ref.logpdf (float64 torch), U = None."""
    dtype = np.dtype(dtype).type
    p = np.asarray(params, dtype=np.float64)
    Z = np.asarray(Z)
    Z = Z.reshape(d, -1) if Z.ndim == 1 else Z
    if family == LOWRANK:
        m, D, U = LR.split(torch.from_numpy(p), d, rank)
        return LR.logpdf(m, D, U, torch.from_numpy(Z.astype(np.float64))).numpy().astype(dtype), None
    mu = p[:d].astype(dtype)
    R = Z.astype(dtype) - mu[:, None]
    if family == MEANFIELD:
        diag = p[d:].astype(dtype)
        U = (R / diag[:, None]).astype(dtype)
    else:
        C = np.tril(p[d:].reshape(d, d, order="F")).astype(dtype)
        diag = np.diag(C)
        U = solve_triangular(C, R, lower=True, check_finite=False).astype(dtype)
    logq = np.sum(_logphi(base, U), axis=0, dtype=dtype) - np.sum(np.log(diag), dtype=dtype)
    return logq.astype(dtype), U


def emulate_forward_block_solve(C, R, bs=BLOCK, keep_bits=24, rounded=True):
    """X of C X = R the way k_lp_fwd16 is documented to work: the bs x bs diagonal blocks inverted in float32 (by doubling,
    tests/solve_ref.py), block forward substitution on the inverses, X_b = Dinv_b (R_b - C[b, :b] X[:b]): C and Dinv are float32 values,
    every sum is accumulated in float64 (R = z - mu arrives in float64 too: pass it so) and X is kept in float64, rounded to float32
    once on its way out (rounded=False: the float64 X, what the kernel sums log phi over).  keep_bits < 24 truncates the inverted blocks."""
    C = np.tril(np.asarray(C)).astype(np.float32).astype(np.float64)
    R = np.asarray(R, dtype=np.float64)
    d = C.shape[0]
    X = np.zeros(R.shape, dtype=np.float64)
    for lo in range(0, d, bs):
        hi = min(lo + bs, d)
        Dinv = S.truncate_bits(S._inverse_by_doubling(C[lo:hi, lo:hi].astype(np.float32)), keep_bits).astype(np.float64)
        X[lo:hi] = Dinv @ (R[lo:hi] - C[lo:hi, :lo] @ X[:lo] if lo else R[lo:hi])
    return X.astype(np.float32) if rounded else X


def emulate_logq(C, X):
    """the Gaussian log q of an emulated solve (its float64 X): the sums over the rows and log det C in float64, rounded to float32"""
    X64 = np.asarray(X, dtype=np.float64)
    d = X64.shape[0]
    logdet = np.sum(np.log(np.diag(np.asarray(C)).astype(np.float32).astype(np.float64)))
    return (-(0.5 * np.sum(X64 * X64, axis=0) + 0.5 * d * LOG2PI) - logdet).astype(np.float32)


def points(C, mu, U, rng):
    """the two point sets of a case from draws U: z = C u + mu (float64 arithmetic on the stored parameters, rounded to their dtype), and
    the same plus 3 N(0, 1) -- on an ill-conditioned C the standardised values of the second set are large"""
    dt = np.asarray(C).dtype
    Z = np.asarray(C, dtype=np.float64) @ np.asarray(U, dtype=np.float64) + np.asarray(mu, dtype=np.float64)[:, None]
    return Z.astype(dt), (Z + 3.0 * rng.normal(size=Z.shape)).astype(dt)


def logq_ratio(got, yard, ref):
    """|got - ref|_2 / max(|yard - ref|_2, 2^-24 |ref|_2) over the n values"""
    got, yard, ref = (np.asarray(a, dtype=np.float64) for a in (got, yard, ref))
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(yard - ref), S.F32_FLOOR * np.linalg.norm(ref), np.finfo(np.float64).tiny))
