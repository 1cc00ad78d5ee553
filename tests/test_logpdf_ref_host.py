"""Host-side checks of tests/logpdf_ref.py, the reference and yardstick of tests/test_gpu_logpdf.py, and of MvLocationScaleLowRank.entropy.

    * logpdf_cols in float64 IS the oracle's logpdf (oracle/oracle.py), tests/lowrank_ref.logpdf and, for the Gaussian families, scipy's
      multivariate_normal.logpdf: 1e-10 relative.
    * ADMISSIBLE: the emulation of the documented forward solve (32-row diagonal blocks inverted in float32, block forward substitution on
      the inverses, every sum and X itself in float64, rounded to float32 on the way out) stays within 4.0 x the float32 LAPACK yardstick on every
      (kind, d, n) of the GPU yardstick and on both point sets -- the standardised points whole and per 64-row block, and log q as an
      n-vector.  Largest seen: 1.06 / 1.06 / 1.10.
    * TEETH: with the inverted blocks cut to 16 significant bits the standardised points leave F32_FACTOR = 8 on every case and point set,
      whole (9.4 at the least: ar999 1024 x 32) and per block (42 at the least), and log q leaves it on every case of the perturbed point
      set (135 at the least).  On the unperturbed set log q is asserted too except at ar999 1024 x 32, where the damage of a 16-bit
      inverse to the sum of squares is 6.9: |u|^2 of O(1) standardised values averages the block errors out, so that one quantity of that
      one case is not claimed to have teeth there.  Nothing is dropped from the GPU yardstick, and the factor is what it was.
    * MvLocationScaleLowRank.entropy() equals tests/lowrank_ref.entropy and the dense 1/2 logdet(2 pi e Sigma).
No GPU."""
import numpy as np
import pytest
import torch
from scipy.stats import multivariate_normal

import advancedvi_jl_amd as avi
from oracle import oracle as O
from tests import basedist_ref as B
from tests import logpdf_ref as L
from tests import lowrank_ref as LR
from tests import solve_ref as S
from tests.helpers import make_family

F32_FACTOR = 8.0     # tests/test_gpu_solve_yardstick.py
ADMISSIBLE = 4.0
NO_LOGQ_TEETH = {("ar999", 1024, 32)}   # unperturbed point set only (docstring)


def _lowrank(rng, d, r, dtype=np.float64):
    return avi.LowRankGaussian(rng.normal(size=d).astype(dtype), rng.uniform(0.5, 1.5, size=d).astype(dtype), (0.7 * rng.normal(size=(d, r))).astype(dtype))


@pytest.mark.parametrize("family", [avi.MEANFIELD, avi.FULLRANK])
def test_float64_helper_is_the_oracle_and_scipy(family):
    rng = np.random.default_rng(5 + family)
    d, n = 13, 6
    q, q_o = make_family(rng, d, family)
    params, _ = avi.destructure(q)
    Z = rng.normal(size=(d, n)) * 2.0
    logq, U = L.logpdf_cols(params, d, family, Z, None, np.float64)
    Cd = np.diag(q_o.scale) if family == avi.MEANFIELD else np.tril(q_o.scale)
    mvn = multivariate_normal(mean=q_o.location, cov=Cd @ Cd.T)
    for k in range(n):
        ref = O.logpdf(q_o, Z[:, k])
        assert abs(logq[k] - ref) <= 1e-10 * abs(ref)
        assert abs(logq[k] - mvn.logpdf(Z[:, k])) <= 1e-10 * abs(ref)
    assert np.allclose(Cd @ U + q_o.location[:, None], Z, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("d,r", [(10, 1), (12, 4), (5, 8)])
def test_float64_helper_is_the_lowrank_reference_and_scipy(d, r):
    rng = np.random.default_rng(d + r)
    q = _lowrank(rng, d, r)
    params, _ = avi.destructure(q)
    Z = rng.normal(size=(d, 7)) * 2.0
    logq, U = L.logpdf_cols(params, d, avi.LOWRANK, Z, None, np.float64, rank=r)
    assert U is None
    m, D, Uf = LR.split(torch.tensor(params), d, r)
    mvn = multivariate_normal(mean=q.location, cov=q.cov())
    for k in range(Z.shape[1]):
        ref = float(LR.logpdf(m, D, Uf, torch.tensor(Z[:, k])))
        assert abs(logq[k] - ref) <= 1e-10 * abs(ref)
        assert abs(logq[k] - mvn.logpdf(Z[:, k])) <= 1e-10 * abs(ref)


@pytest.mark.parametrize("base", [B.LAPLACE, B.tdist(3.0), B.tdist(0.7)], ids=["laplace", "t3", "t0.7"])
def test_base_terms_are_basedist_ref(base):
    rng = np.random.default_rng(11)
    d, n = 9, 4
    q, _ = make_family(rng, d, avi.FULLRANK)
    params, _ = avi.destructure(q)
    Z = rng.normal(size=(d, n)) * 3.0
    logq, U = L.logpdf_cols(params, d, avi.FULLRANK, Z, base, np.float64)
    C = np.tril(params[d:].reshape(d, d, order="F"))
    ref = B.logphi(base, np.linalg.solve(C, Z - params[:d, None])).sum(axis=0) - np.log(np.diag(C)).sum()
    assert np.allclose(logq, ref, rtol=1e-10, atol=0.0)


def _case_results(kind, d, n, keep_bits):
    """per point set: (whole, worst block) of the standardised points and the ratio of log q, of the emulation against the f32 yardstick"""
    C, mu, params = L.yardstick_setup(kind, d)
    rng = np.random.default_rng(d + n)
    U = rng.normal(size=(d, n)).astype(np.float32)
    out = []
    for Z in L.points(C, mu, U, rng):
        lq_ref, U_ref = L.logpdf_cols(params, d, L.FULLRANK, Z, None, np.float64)
        lq_yard, U_yard = L.logpdf_cols(params, d, L.FULLRANK, Z, None, np.float32)
        X = L.emulate_forward_block_solve(C, Z.astype(np.float64) - mu.astype(np.float64)[:, None], L.BLOCK, keep_bits, rounded=False)
        out.append(S.block_ratios(X.astype(np.float32), U_yard, U_ref, d) + (L.logq_ratio(L.emulate_logq(C, X), lq_yard, lq_ref),))
    return out


@pytest.mark.parametrize("kind,d,n", L.YARDSTICK_CASES, ids=[f"{k}-{d}x{n}" for k, d, n in L.YARDSTICK_CASES])
def test_criterion_is_admissible_and_has_teeth(kind, d, n):
    for which, (whole, block, lq) in enumerate(_case_results(kind, d, n, 24)):
        print(f"[logpdf emulation] {kind} {d} {n} set {which}: {whole:.2f}, {block:.2f}, logq {lq:.2f}")
        assert whole <= ADMISSIBLE and block <= ADMISSIBLE and lq <= ADMISSIBLE, (kind, d, n, which, whole, block, lq)
    for which, (whole, block, lq) in enumerate(_case_results(kind, d, n, 16)):
        print(f"[logpdf emulation, 16-bit inverses] {kind} {d} {n} set {which}: {whole:.2f}, {block:.2f}, logq {lq:.2f}")
        assert whole > F32_FACTOR and block > F32_FACTOR, (kind, d, n, which, whole, block)
        if which == 1 or (kind, d, n) not in NO_LOGQ_TEETH:
            assert lq > F32_FACTOR, (kind, d, n, which, lq)


@pytest.mark.parametrize("d,r,dtype", [(10, 1, np.float64), (30, 3, np.float64), (5, 8, np.float64), (30, 3, np.float32)])
def test_lowrank_entropy(d, r, dtype):
    rng = np.random.default_rng(d * 7 + r)
    q = _lowrank(rng, d, r, dtype)
    got = q.entropy()
    assert isinstance(got, dtype)
    q64 = avi.LowRankGaussian(q.location.astype(np.float64), q.scale_diag.astype(np.float64), q.scale_factors.astype(np.float64))
    params, _ = avi.destructure(q64)
    ref = float(LR.entropy(*LR.split(torch.tensor(params), d, r)))
    dense = 0.5 * np.linalg.slogdet(2.0 * np.pi * np.e * q64.cov())[1]
    tol = 1e-12 if dtype == np.float64 else 1e-5
    assert abs(float(got) - ref) <= tol * abs(ref) and abs(ref - dense) <= 1e-11 * abs(dense)
