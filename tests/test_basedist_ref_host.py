"""Host checks of the base-distribution yardstick (tests/basedist_ref.py) and of the Python mirror of MvLocationScale(location, scale, dist):
the two streams have the right law, log phi / psi / H(phi) are scipy's, and the closed-form estimate equals torch autograd of the literal
reference forward (repgradelbo.jl:142-149, entropy.jl, location_scale.jl:52-63).  No GPU."""
import math

import numpy as np
import pytest
import torch
from scipy import stats

import advancedvi_jl_amd as avi
from oracle import oracle as O
from tests import basedist_ref as B
from tests.helpers import SEED, make_family, make_problem
from tests.lowrank_ref import _Target

BASES = [B.LAPLACE, B.tdist(1.0), B.tdist(3.0), B.tdist(5.5)]
IDS = ["laplace", "t1", "t3", "t5.5"]


def _scipy(base):
    return stats.laplace if base[0] == "laplace" else stats.t(base[1])


# ---- distribution ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32stream", "f64stream"])
@pytest.mark.parametrize("base", BASES, ids=IDS)
def test_streams_have_the_law(base, f64):
    """Kolmogorov-Smirnov against scipy at 2 x 10^5 draws of a fixed seed (deterministic: p > 1e-3 holds for these streams); adjacent rows --
    for TDist the two variates of one Philox block -- are uncorrelated within 4 / sqrt(N)."""
    d, M = 50, 4000
    U = B.draws(base, SEED, 7, d, 0, M, f64=f64)
    assert U.shape == (d, M) and np.all(np.isfinite(U))
    p = stats.kstest(U.ravel(), _scipy(base).cdf).pvalue
    print(f"[basedist ks] {base} f64={f64}: p = {p:.4f}")
    assert p > 1e-3
    if base[0] == "laplace" or base[1] > 4.0:   # the sample correlation itself, where its standard error is 1 / sqrt(N) (finite fourth moment)
        assert abs(np.corrcoef(U[0::2].ravel(), U[1::2].ravel())[0, 1]) < 4.0 / math.sqrt(U[0::2].size)
        assert abs(np.corrcoef(U[1:-1:2].ravel(), U[2::2].ravel())[0, 1]) < 4.0 / math.sqrt(U[2::2].size)
    # every base, heavy tails included: the correlation of the normal scores (the Pearson coefficient of Cauchy draws has no law to hold it to)
    S = stats.norm.ppf(_scipy(base).cdf(U).clip(1e-12, 1 - 1e-12))
    a, b = S[0::2].ravel(), S[1::2].ravel()       # rows 2k, 2k + 1: one Philox block (TDist), half a block (Laplace)
    n = a.size
    assert abs(np.corrcoef(a, b)[0, 1]) < 4.0 / math.sqrt(n)
    a, b = S[1:-1:2].ravel(), S[2::2].ravel()     # rows 2k + 1, 2k + 2: across blocks
    assert abs(np.corrcoef(a, b)[0, 1]) < 4.0 / math.sqrt(a.size)
    a, b = S[:, 0::2].ravel(), S[:, 1::2].ravel()  # adjacent columns
    assert abs(np.corrcoef(a, b)[0, 1]) < 4.0 / math.sqrt(a.size)


def test_streams_are_a_function_of_the_global_column():
    for base in (B.LAPLACE, B.tdist(3.0)):
        for d in (1, 7, 10):
            whole = B.draws(base, SEED, 3, d, 0, 9)
            assert np.array_equal(whole[:, 4:9], B.draws(base, SEED, 3, d, 4, 9))
            assert not np.array_equal(whole, B.draws(base, SEED, 4, d, 0, 9))


def test_float32_evaluation_is_close_to_float64():
    for base in (B.LAPLACE, B.tdist(3.0), B.tdist(5.5)):
        U64 = B.draws(base, SEED, 1, 33, 0, 64)
        U32 = B.draws(base, SEED, 1, 33, 0, 64, dtype=np.float32)
        assert U32.dtype == np.float32
        assert np.all(np.abs(U32 - U64) <= 8 * 2.0 ** -24 * B.draw_scale(base, SEED, 1, 33, 0, 64) + 1e-30)


# ---- densities -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", BASES, ids=IDS)
def test_densities_are_scipys(base):
    x = np.concatenate([np.linspace(-30, 30, 241), [1e-3, -1e-3, 400.0, -400.0]])
    x = x[x != 0.0]
    assert np.allclose(B.logphi(base, x), _scipy(base).logpdf(x), rtol=1e-12, atol=1e-12)
    assert abs(B.entropy(base) - float(_scipy(base).entropy())) < 1e-12
    h = 1e-6 * np.maximum(1.0, np.abs(x))
    fd = (B.logphi(base, x + h) - B.logphi(base, x - h)) / (2 * h)
    assert np.allclose(B.psi(base, x), fd, rtol=1e-6, atol=1e-8)
    # the mirror's host statistics are the same numbers
    dist = avi.Laplace() if base[0] == "laplace" else avi.TDist(base[1])
    assert abs(dist.entropy() - B.entropy(base)) < 1e-12
    assert B.base_of(dist) == base


# ---- gradient --------------------------------------------------------------------------------------------------------------------------
def _torch_dist(base):
    if base[0] == "laplace":
        return torch.distributions.Laplace(torch.tensor(0.0, dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64))
    return torch.distributions.StudentT(torch.tensor(base[1], dtype=torch.float64))


def _literal_forward(params, d, family, tgt, U, kind, base):
    """estimate_repgradelbo_ad_forward (repgradelbo.jl:142-149) with estimate_entropy of entropy.jl on MvLocationScale(m, C, dist):
    logpdf(q, z) = sum logpdf.(dist, C \\ (z - m)) - logdet C (location_scale.jl:59-63), entropy(q) = d H(dist) + logdet C (:52-57);
    q_stop = the same parameters detached (:162)."""
    dist = _torch_dist(base)

    def unpack(p):
        if family == O.MEANFIELD:
            return p[:d], torch.diag(p[d:])
        return p[:d], torch.tril(p[d:].reshape(d, d).T)

    def logpdf(q, Z):
        m, C = q
        z_std = torch.linalg.solve_triangular(C, Z - m[:, None], upper=False)
        return torch.sum(dist.log_prob(z_std), dim=0) - torch.sum(torch.log(torch.diagonal(C)))

    def entropy(q):
        return d * B.entropy(base) + torch.sum(torch.log(torch.diagonal(q[1])))

    q, q_stop = unpack(params), unpack(params.detach())
    Z = q[1] @ U + q[0][:, None]
    energy = torch.mean(_Target.apply(Z, tgt))
    if kind == B.CLOSED_FORM:
        ent = entropy(q)
    elif kind == B.CLOSED_FORM_ZERO_GRAD:
        ent = entropy(q_stop)
    elif kind == B.MONTE_CARLO:
        ent = torch.mean(-logpdf(q, Z))
    else:
        ent = torch.mean(-logpdf(q_stop, Z))
        if kind == B.STL_ZERO_GRAD:
            ent = ent - entropy(q) + entropy(q_stop)
    return -(energy + ent)


@pytest.mark.parametrize("kind", range(5))
@pytest.mark.parametrize("target", ["diag", "dense"])
@pytest.mark.parametrize("base", [B.LAPLACE, B.tdist(3.0)], ids=["laplace", "t3"])
@pytest.mark.parametrize("family", [avi.MEANFIELD, avi.FULLRANK], ids=["mf", "fr"])
def test_closed_form_gradient_equals_autograd_of_the_literal_forward(family, base, target, kind):
    d, M = 7, 5
    rng = np.random.default_rng(23 + family)
    q, _ = make_family(rng, d, family)
    _, tgt = make_problem(rng, target, d)
    params, _ = avi.destructure(q)
    U = B.draws(base, SEED, 2, d, 0, M)
    got = B.estimate_gradient(params, d, family, tgt, U, kind, base)
    p = torch.tensor(params, requires_grad=True)
    val = _literal_forward(p, d, family, tgt, torch.tensor(U), kind, base)
    (g,) = torch.autograd.grad(val, p)
    g = g.numpy()
    val = float(val.detach())
    assert abs(got["value"] - val) <= 1e-10 * abs(val)
    assert np.linalg.norm(got["grad"] - g) <= 1e-10 * np.linalg.norm(g)


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------
def test_dist_survives_destructure_and_restructure():
    rng = np.random.default_rng(0)
    for family in (avi.MEANFIELD, avi.FULLRANK):
        q0, _ = make_family(rng, 5, family)
        for dist in (avi.Normal(), avi.Laplace(), avi.TDist(4.5)):
            q = avi.MvLocationScale(q0.location, q0.scale, dist)
            flat, re = avi.destructure(q)
            q2 = re(flat)
            assert q2.dist == dist and type(q2.dist) is type(dist) and q2.family == family
            assert np.array_equal(q2.location, q.location) and np.array_equal(q2.scale, q.scale)


def test_two_argument_use_is_unchanged():
    rng = np.random.default_rng(1)
    q0, q_o = make_family(rng, 6, avi.FULLRANK)
    q = avi.MvLocationScale(q0.location, q0.scale)
    assert isinstance(q.dist, avi.Normal) and q.dist.code == 0 and q.dist == avi.Normal() and q.dist != avi.Laplace()
    flat, re = avi.destructure(q)
    assert np.array_equal(flat, O.destructure(q_o)) and re(flat).dist == avi.Normal()
    assert avi.FullRankGaussian(q0.location, q0.scale).dist == avi.Normal()
    assert abs(float(q.entropy()) - O.entropy_closed_form(q_o)) < 1e-12   # the Gaussian's closed-form entropy
    assert np.allclose(q.cov(), q_o.scale @ q_o.scale.T) and np.array_equal(q.mean(), q.location)


def test_host_statistics_are_the_references():
    """location_scale.jl:52-57, 98-113: entropy = d H(dist) + logdet C; mean = m + C fill(mean(dist)); var = var(dist) diag(C C'); cov."""
    rng = np.random.default_rng(2)
    for family in (avi.MEANFIELD, avi.FULLRANK):
        q0, _ = make_family(rng, 5, family)
        C = np.diag(q0.scale) if family == avi.MEANFIELD else q0.scale
        for dist, sp in ((avi.Laplace(), stats.laplace), (avi.TDist(5.5), stats.t(5.5)), (avi.Normal(), stats.norm)):
            q = avi.MvLocationScale(q0.location, q0.scale, dist)
            assert abs(float(q.entropy()) - (5 * float(sp.entropy()) + np.sum(np.log(np.diag(C))))) < 1e-12
            assert np.allclose(q.mean(), q0.location)
            assert np.allclose(q.var(), float(sp.var()) * np.diag(C @ C.T), rtol=1e-12)
            assert np.allclose(q.cov(), float(sp.var()) * (C @ C.T), rtol=1e-12)
    assert avi.TDist(5.0).var() == 5.0 / 3.0 and avi.TDist(2.0).var() == math.inf and avi.TDist(1.5).var() == math.inf
    assert math.isnan(avi.TDist(1.0).var()) and math.isnan(avi.TDist(0.5).var())
    assert avi.Laplace().var() == 2.0 and avi.Laplace().mean() == 0.0 and avi.Normal().var() == 1.0


def test_bad_degrees_of_freedom_raise():
    for nu in (0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError):
            avi.TDist(nu)
    with pytest.raises(TypeError):
        avi.MvLocationScale(np.zeros(3), np.ones(3), "laplace")


def test_score_gradient_and_measure_space_refuse_a_non_normal_base():
    """Raised by the Python mirror before any library call (no device is needed to get them)."""
    d = 4
    prob = avi.DiagNormalProblem(np.zeros(d), np.ones(d))
    for dist in (avi.Laplace(), avi.TDist(3.0)):
        q = avi.MvLocationScale(np.zeros(d), np.eye(d), dist)
        params, re = avi.destructure(q)
        with pytest.raises(TypeError, match="base distribution"):
            avi.init(avi.PhiloxRNG(SEED), avi.ScoreGradELBO(4), avi.AutoMIVI(), q, prob, params, re)
        with pytest.raises(TypeError, match="base distribution"):   # sharded estimates: the library refuses the base there
            avi.distributed.DistributedRepGradELBO(q, prob, 8, avi.ClosedFormEntropy(), SEED)
        for alg in (avi.KLMinSqrtNaturalGradDescent, avi.KLMinNaturalGradDescent, avi.KLMinWassFwdBwd, avi.FisherMinBatchMatch):
            with pytest.raises(TypeError, match="base distribution"):
                avi.init(avi.PhiloxRNG(SEED), alg(0.1) if alg is not avi.FisherMinBatchMatch else alg(), q, prob)
