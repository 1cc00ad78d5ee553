"""Host checks of the low-rank family: the reference restatement (tests/lowrank_ref.py) against itself -- the Woodbury evaluation the
device kernels implement equals the literal `cholesky(Sigma)` / `logdet` path, autograd equals finite differences -- and the Python
mirror of src/families/location_scale_low_rank.jl (destructure / Restructure, mean / var / cov, the draw split).  No GPU."""
import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from oracle import oracle as O
from tests import lowrank_ref as R
from tests.helpers import SEED, make_problem


def make_lowrank(rng, d, r, dtype=np.float64, zero_factors=False):
    mu = rng.normal(size=d).astype(dtype)
    D = rng.uniform(0.5, 1.5, size=d).astype(dtype)
    U = (np.zeros((d, r)) if zero_factors else 0.7 * rng.normal(size=(d, r))).astype(dtype)
    return avi.LowRankGaussian(mu, D, U)


@pytest.mark.parametrize("d,r,M", [(10, 1, 1), (10, 2, 7), (30, 3, 10)])
def test_woodbury_equals_the_literal_path(d, r, M):
    rng = np.random.default_rng(d + r)
    q = make_lowrank(rng, d, r)
    params, _ = avi.destructure(q)
    eps = rng.normal(size=(d + r, M))
    p = torch.tensor(params)
    m, D, U = R.split(p, d, r)
    Z = R.rand(m, D, U, torch.tensor(eps))
    logq, V, x = R.woodbury_logq(params, d, r, eps)
    lit = np.array([float(R.logpdf(m, D, U, Z[:, k])) for k in range(M)])
    assert np.allclose(logq, lit, rtol=1e-12, atol=1e-12)
    Sigma = np.diag(q.scale_diag ** 2) + q.scale_factors @ q.scale_factors.T
    assert np.allclose(V, np.linalg.solve(Sigma, Z.numpy() - q.location[:, None]), rtol=1e-11, atol=1e-12)
    assert np.allclose(q.scale_factors.T @ V, x, rtol=1e-11, atol=1e-12)   # U' V = x: what the Monte-Carlo entropy's VJP uses
    # closed-form entropy: logdet(I + U' D^-2 U) against logdet(Sigma)
    ent = float(R.entropy(m, D, U))
    assert abs(ent - (0.5 * d * (1 + R.LOG2PI) + 0.5 * np.linalg.slogdet(Sigma)[1])) < 1e-11


@pytest.mark.parametrize("kind", range(5))
@pytest.mark.parametrize("target", ["diag", "dense", "funnel"])
def test_woodbury_estimators_equal_autograd(kind, target):
    """The five estimators as the kernels assemble them (value and the table of gradients) against autograd of the literal expressions."""
    d, r, M = 12, 3, 5
    rng = np.random.default_rng(17)
    q = make_lowrank(rng, d, r)
    params, _ = avi.destructure(q)
    _, tgt = make_problem(rng, target, d)
    eps = rng.normal(size=(d + r, M))
    ref = R.estimate_gradient(params, d, r, tgt, eps, kind)
    cols = [tgt.logdensity_and_gradient(ref["Z"][:, k].copy()) for k in range(M)]
    ell, G = np.array([c[0] for c in cols]), np.stack([c[1] for c in cols], axis=1)
    got = R.woodbury_eval(params, d, r, G, ell, eps, kind)
    assert abs(got["value"] - ref["value"]) <= 1e-12 * max(1.0, abs(ref["value"]))
    assert np.linalg.norm(got["grad"] - ref["grad"]) <= 1e-11 * max(1.0, np.linalg.norm(ref["grad"]))
    assert abs(R.estimate_objective(params, d, r, tgt, eps, kind) - ref["value"]) <= 1e-12 * max(1.0, abs(ref["value"]))


def test_autograd_equals_finite_differences():
    d, r, M = 6, 2, 3
    rng = np.random.default_rng(3)
    q = make_lowrank(rng, d, r)
    params, _ = avi.destructure(q)
    _, tgt = make_problem(rng, "dense", d)
    eps = rng.normal(size=(d + r, M))
    e = torch.tensor(eps)
    for kind in (R.CLOSED_FORM, R.MONTE_CARLO):   # (the other three stop gradients: no finite-difference counterpart of the whole value)
        ref = R.estimate_gradient(params, d, r, tgt, eps, kind)
        h, fd = 1e-6, np.zeros_like(params)
        for i in range(params.size):
            pp, pm = params.copy(), params.copy()
            pp[i] += h
            pm[i] -= h
            with torch.no_grad():
                fd[i] = (float(R.forward(torch.tensor(pp), d, r, tgt, e, kind)[0]) - float(R.forward(torch.tensor(pm), d, r, tgt, e, kind)[0])) / (2 * h)
        assert np.linalg.norm(fd - ref["grad"]) <= 1e-6 * max(1.0, np.linalg.norm(ref["grad"]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("r", [1, 2])
def test_family_mirror(r, dtype):
    """test/families/location_scale_low_rank.jl: d = 10, r in {1, 2}; lengths and round trip of destructure / Restructure."""
    d = 10
    rng = np.random.default_rng(r)
    q = make_lowrank(rng, d, r, dtype)
    assert q.family == avi.LOWRANK == 2 and q.rank == r and len(q) == d and q.eltype == np.dtype(dtype)
    flat, re = avi.destructure(q)
    assert flat.dtype == np.dtype(dtype) and flat.shape == (2 * d + d * r,)
    assert np.array_equal(flat[:d], q.location) and np.array_equal(flat[d:2 * d], q.scale_diag)
    assert np.array_equal(flat[2 * d:3 * d], q.scale_factors[:, 0])   # column-major factors
    q2 = re(flat)
    assert isinstance(q2, avi.MvLocationScaleLowRank) and q2.rank == r
    for a, b in ((q2.location, q.location), (q2.scale_diag, q.scale_diag), (q2.scale_factors, q.scale_factors)):
        assert a.dtype == np.dtype(dtype) and np.array_equal(a, b)
    with pytest.raises(ValueError):
        re(flat[:-1])
    Sigma = np.diag(q.scale_diag.astype(np.float64) ** 2) + q.scale_factors.astype(np.float64) @ q.scale_factors.astype(np.float64).T
    tol = 1e-6 if dtype == np.float32 else 1e-14
    assert np.array_equal(q.mean(), q.location)
    assert np.allclose(q.var(), np.diag(Sigma), rtol=tol) and np.allclose(q.cov(), Sigma, rtol=tol, atol=tol)
    assert q.mean().dtype == q.var().dtype == q.cov().dtype == np.dtype(dtype)


def test_family_rejects_bad_shapes():
    with pytest.raises(ValueError):
        avi.LowRankGaussian(np.zeros(4), np.ones(3), np.zeros((4, 2)))
    with pytest.raises(ValueError):
        avi.LowRankGaussian(np.zeros(4), np.ones(4), np.zeros((4, 0)))
    with pytest.raises(ValueError):
        avi.LowRankGaussian(np.zeros(4), np.ones(4), np.zeros((4, 65)))
    with pytest.raises(TypeError):
        avi.LowRankGaussian(np.zeros(4, dtype=np.int64), np.ones(4), np.zeros((4, 1)))


def test_draw_split_of_the_one_stream():
    """The draws of an estimate are ONE Philox stream of d + r rows per column: rows 0 .. d-1 are u1, rows d .. d+r-1 are u2, and a column
    is a pure function of (seed, index, global column)."""
    d, r, idx = 10, 3, 5
    E = O.philox_normal(SEED, idx, d + r, 0, 9)
    assert E.shape == (d + r, 9)
    assert np.array_equal(O.philox_normal(SEED, idx, d + r, 4, 9), E[:, 4:])          # columns regenerate alone
    assert not np.array_equal(E[:d], O.philox_normal(SEED, idx, d, 0, 9))              # (not the d-row stream: the block index runs over d + r rows)
    q = make_lowrank(np.random.default_rng(0), d, r)
    params, _ = avi.destructure(q)
    Z = R.rand(*R.split(torch.tensor(params), d, r), torch.tensor(E)).numpy()
    assert np.allclose(Z, q.scale_diag[:, None] * E[:d] + q.scale_factors @ E[d:] + q.location[:, None], rtol=1e-14)
