"""avi.optimize_many without a GPU: which runs can share a launch is a pure host decision (optimize.many_plan), and the argument checks
that come before any library call."""
import numpy as np
import pytest

import advancedvi_jl_amd as avi
OPT = avi._optimize   # the module (the package exports the function `optimize` under that name)


def _diag(d, dtype=np.float32, shift=0.0):
    return avi.DiagNormalProblem(np.full(d, shift, dtype), np.ones(d, dtype))


def _logreg(n, p, dtype=np.float32, variant="logsigma_normal", seed=0):
    rng = np.random.default_rng(seed)
    return avi.LogRegProblem(rng.normal(size=(n, p)).astype(dtype), (rng.uniform(size=n) < 0.5).astype(np.uint8), variant=variant)


def _fr(d, dtype=np.float32):
    return avi.FullRankGaussian(np.zeros(d, dtype), np.eye(d, dtype=dtype))


def _mf(d, dtype=np.float32):
    return avi.MeanFieldGaussian(np.zeros(d, dtype), np.ones(d, dtype))


def _alg(opt=None, M=1, averager=None, operator=None, entropy=None):
    return avi.KLMinRepGradDescent(avi.AutoMIVI(), n_samples=M, optimizer=opt or avi.Adam(1e-3), averager=averager or avi.NoAveraging(),
                                   operator=operator or avi.ClipScale(), entropy=entropy)


def test_same_types_and_shapes_form_one_group():
    K = 4
    # a step-size sweep over restarts on different targets: one group
    algs = [_alg(avi.Adam(10.0 ** -k)) for k in range(1, K + 1)]
    key = OPT.many_plan(algs, [_diag(10, shift=k) for k in range(K)], [_fr(10)] * K)
    assert key is not None and key[-1][0] == "A"
    # DoG / DoWG: alpha is their step size
    assert OPT.many_plan([_alg(avi.DoWG(1e-6)), _alg(avi.DoWG(1e-3))], [_diag(10)] * 2, [_fr(10)] * 2) is not None
    # logistic regressions of one shape, both families
    for q in (_fr(6), _mf(6)):
        key = OPT.many_plan([_alg(M=2)] * 3, [_logreg(40, 5, seed=k) for k in range(3)], [q] * 3)
        assert key is not None and key[-1][:3] == ("B", 40, 5)
    # the proximal algorithm groups with itself
    prox = avi.KLMinRepGradProxDescent(avi.AutoMIVI(), optimizer=avi.DoWG(), n_samples=1)
    assert OPT.many_plan([prox] * 2, [_logreg(208, 60, variant="lognormal_exp_bijector")] * 2, [_fr(61)] * 2) is not None
    # the largest admitted shapes (fr_small_loop_ok; 512 with sticking-the-landing)
    assert OPT.many_plan([_alg(M=24)] * 2, [_diag(32)] * 2, [_fr(32)] * 2) is not None
    assert OPT.many_plan([_alg(M=16, entropy=avi.StickingTheLandingEntropy())] * 2, [_diag(32)] * 2, [_fr(32)] * 2) is not None


@pytest.mark.parametrize("what", ["rule", "operator", "averager", "entropy", "n_samples", "d", "dtype", "problem-type", "family", "lr-rows", "lr-variant",
                                  "adam-betas"])
def test_differing_types_or_shapes_run_sequentially(what):
    a, b = _alg(), _alg()
    pa, pb, qa, qb = _diag(10), _diag(10), _fr(10), _fr(10)
    if what == "rule":
        b = _alg(avi.Descent(1e-3))
    elif what == "operator":
        b = _alg(operator=avi.IdentityOperator())
    elif what == "averager":
        b = _alg(averager=avi.PolynomialAveraging())
    elif what == "entropy":
        b = _alg(entropy=avi.StickingTheLandingEntropy())
    elif what == "n_samples":
        b = _alg(M=2)
    elif what == "d":
        pb, qb = _diag(11), _fr(11)
    elif what == "dtype":
        pb, qb = _diag(10, np.float64), _fr(10, np.float64)
    elif what == "problem-type":
        pa, pb, qa, qb = _diag(6), _logreg(40, 5), _fr(6), _fr(6)
    elif what == "family":
        pa, pb, qa, qb = _logreg(40, 5), _logreg(40, 5), _fr(6), _mf(6)
    elif what == "lr-rows":
        pa, pb, qa, qb = _logreg(40, 5), _logreg(41, 5), _fr(6), _fr(6)
    elif what == "lr-variant":
        pa, pb, qa, qb = _logreg(40, 5), _logreg(40, 5, variant="lognormal_exp_bijector"), _fr(6), _fr(6)
    elif what == "adam-betas":
        b = _alg(avi.Adam(1e-3, beta=(0.8, 0.999)))
    assert OPT.many_plan([a, a], [pa, pa], [qa, qa]) is not None   # each side alone would share a launch ...
    assert OPT.many_plan([b, b], [pb, pb], [qb, qb]) is not None
    assert OPT.many_plan([a, b], [pa, pb], [qa, qb]) is None       # ... together they do not


def test_configurations_outside_the_two_classes_run_sequentially():
    two = lambda alg, prob, q: OPT.many_plan([alg] * 2, [prob] * 2, [q] * 2)   # noqa: E731
    assert two(_alg(), _diag(64), _fr(64)) is None                                   # d > 32
    assert two(_alg(M=25), _diag(32), _fr(32)) is None                               # d n_mc > 768
    assert two(_alg(M=17, entropy=avi.StickingTheLandingEntropy()), _diag(32), _fr(32)) is None   # ... > 512 with sticking-the-landing
    assert two(_alg(), _diag(10), _mf(10)) is None                                   # mean-field with the Gaussian target
    assert two(_alg(avi.COCOB()), _diag(10), _fr(10)) is None                        # COCOB
    assert two(_alg(entropy=avi.StickingTheLandingEntropy()), _logreg(40, 5), _fr(6)) is None   # sticking-the-landing on the regression
    assert two(_alg(M=8), _logreg(208, 60), _fr(61)) is None                         # (d - 1) n_mc > 256
    assert two(_alg(), _logreg(40, 70), _fr(71)) is None                             # d > 64
    assert two(_alg(), avi.FunnelProblem(10), _mf(10)) is None                       # the funnel
    assert two(_alg(), avi.TransformedProblem(_diag(10), avi.StackedBijector([(0, 10, "exp")])), _fr(10)) is None   # a bijector
    assert two(_alg(), _diag(10), avi.MvLocationScale(np.zeros(10, np.float32), np.eye(10, dtype=np.float32), avi.Laplace())) is None
    assert two(avi.KLMinScoreGradDescent(avi.AutoMIVI(), optimizer=avi.Adam(), averager=avi.NoAveraging(), operator=avi.ClipScale()),
               _diag(10), _fr(10)) is None
    assert OPT.many_plan([], [], []) is None


def test_argument_checks_need_no_library(monkeypatch):
    from advancedvi_jl_amd import _lib

    def no_library():
        raise AssertionError("the library must not be loaded by an argument error")
    monkeypatch.setattr(_lib, "load", no_library)
    rngs = [avi.PhiloxRNG(1), avi.PhiloxRNG(2)]
    with pytest.raises(ValueError, match="at least one"):
        avi.optimize_many([], _alg(), 3, _diag(4), _fr(4))
    with pytest.raises(TypeError, match="PhiloxRNG"):
        avi.optimize_many([1, 2], _alg(), 3, _diag(4), _fr(4))
    r = avi.PhiloxRNG(1)
    with pytest.raises(ValueError, match="of its own"):
        avi.optimize_many([r, r], _alg(), 3, _diag(4), _fr(4))
    with pytest.raises(ValueError, match="3 entries for 2"):
        avi.optimize_many(rngs, [_alg()] * 3, 3, _diag(4), _fr(4))
    with pytest.raises(ValueError, match="probs holds"):
        avi.optimize_many(rngs, _alg(), 3, [_diag(4)] * 3, _fr(4))
    with pytest.raises(ValueError, match="q_inits holds"):
        avi.optimize_many(rngs, _alg(), 3, _diag(4), [_fr(4)])
    with pytest.raises(ValueError, match="max_iter"):
        avi.optimize_many(rngs, _alg(), -1, _diag(4), _fr(4))
    with pytest.raises(ValueError, match="states"):
        avi.optimize_many(rngs, _alg(), 3, _diag(4), _fr(4), states={"params": None})
    with pytest.raises(ValueError, match="states"):
        avi.optimize_many(rngs, _alg(), 3, _diag(4), _fr(4), states=[{}])
