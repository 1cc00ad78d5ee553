"""RepGradELBO objective: host-side mirror of src/algorithms/repgradelbo.jl + src/algorithms/entropy.jl
+ src/algorithms/abstractobjective.jl (AdvancedVI.jl v0.7.0) over libmivi.

Same names, argument meaning and error behaviour as the reference for the hot path:
    RepGradELBO(n_samples; entropy)                      repgradelbo.jl:21-24, 72-74
    init(rng, obj, adtype, q, prob, params, restructure) repgradelbo.jl:41-70
    estimate_gradient_(rng, obj, adtype, out, state, params, restructure) -> (out, state, info)
                                                         repgradelbo.jl:151-177  (Julia's `estimate_gradient!`)
    estimate_objective(rng, obj, q, prob; n_samples)     repgradelbo.jl:112-122
    set_objective_state_problem(state, prob)             repgradelbo.jl:31-39
The AD backend argument is the drop-in seam: `AutoMIVI()` selects the analytic-VJP HIP
path that replaces AD of `estimate_repgradelbo_ad_forward` (repgradelbo.jl:142-149)."""
from __future__ import annotations

import logging

import numpy as np

from . import problems as P
from .context import MiviContext
from .families import COUPLING_FLOWS, FLOW_NAMES, MvLocationScale, MvLocationScaleLowRank, destructure, flow_arch as _flow_arch


_log = logging.getLogger("advancedvi_jl_amd")


# --- entropy estimators (src/algorithms/entropy.jl) -----------------------------------------------
class AbstractEntropyEstimator:
    code = -1

    def __repr__(self):
        return f"{type(self).__name__}()"


class ClosedFormEntropy(AbstractEntropyEstimator):              # entropy.jl:25-29
    code = 0


class ClosedFormEntropyZeroGradient(AbstractEntropyEstimator):  # entropy.jl:11-15
    code = 1


class MonteCarloEntropy(AbstractEntropyEstimator):              # entropy.jl:40-46
    code = 2


class StickingTheLandingEntropy(AbstractEntropyEstimator):      # entropy.jl:57-65
    code = 3


class StickingTheLandingEntropyZeroGradient(AbstractEntropyEstimator):  # entropy.jl:78-90
    code = 4


class AutoMIVI:
    """ADTypes.AbstractADType subtype selecting libmivi's closed-form VJP instead of an AD backend for the ESTIMATOR.
    `target_ad`: the backend that differentiates an ORDER-0 target's `logdensity` on the host (the reference differentiates through it
    with `adtype` itself, repgradelbo.jl:50-57; here the estimator needs no AD, so only the target's own gradient is left to provide):
    "forwarddiff" (dual numbers, `forwarddiff.py`) or None = reject order-0 targets."""

    def __init__(self, device: int = 0, target_ad="forwarddiff"):
        self.device = device
        self.target_ad = target_ad


class PhiloxRNG:
    """The `rng` threaded through the reference API.  State = (seed, next estimate index): one
    estimate consumes one index, replacing the one `rand(rng, Normal, d, M)` draw per estimate
    (src/families/location_scale.jl:76,86).  Copyable => warm starts are reproducible."""

    def __init__(self, seed: int = 0x38BEF07CF9CC549D, counter: int = 0):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.counter = int(counter)

    def next_index(self) -> int:
        i = self.counter
        self.counter += 1
        return i

    def copy(self):
        return PhiloxRNG(self.seed, self.counter)


_default_rng = PhiloxRNG(0x9E3779B97F4A7C15)


def default_rng():
    return _default_rng


class DiffResult:
    """DiffResults.MutableDiffResult(value, (gradient,)): the caller-owned output buffer
    (src/algorithms/common.jl:51), device resident."""

    def __init__(self, value, gradient):
        self.value_t = value        # torch tensor [1]
        self.gradient_t = gradient  # torch tensor [params_len]

    def value(self):
        return self.value_t.item()

    def gradient(self):
        return self.gradient_t


class RepGradELBO:
    """RepGradELBO(n_samples; entropy=ClosedFormEntropy()): repgradelbo.jl:21-24,72-74."""

    def __init__(self, n_samples: int, entropy: AbstractEntropyEstimator = None):
        if not isinstance(n_samples, (int, np.integer)) or n_samples < 1:
            raise ValueError("n_samples must be a positive Int")
        self.n_samples = int(n_samples)
        self.entropy = entropy if entropy is not None else ClosedFormEntropy()
        if not isinstance(self.entropy, AbstractEntropyEstimator):
            raise TypeError("entropy must be an AbstractEntropyEstimator")

    def __repr__(self):  # Base.show, repgradelbo.jl:76-82
        return f"RepGradELBO(entropy={self.entropy}, n_samples={self.n_samples})"


class RepGradELBOState:
    """RepGradELBOState(problem, obj_ad_prep): the prepared estimator (repgradelbo.jl:26-29);
    `obj_ad_prep` is the libmivi context instead of an AD preparation."""

    def __init__(self, problem, ctx: MiviContext):
        self.problem = problem
        self.obj_ad_prep = ctx


class ScoreGradELBO:
    """ScoreGradELBO(n_samples): scoregradelbo.jl:15-17 -- the score-function gradient of the ELBO with the VarGrad (leave-one-out) control
    variate.  It evaluates the target's `logdensity` only, so it is the objective for targets without a gradient."""

    def __init__(self, n_samples: int):
        if not isinstance(n_samples, (int, np.integer)) or n_samples < 1:
            raise ValueError("n_samples must be a positive Int")
        self.n_samples = int(n_samples)

    def __repr__(self):  # Base.show, scoregradelbo.jl:52-56
        return f"ScoreGradELBO(n_samples={self.n_samples})"


class ScoreGradELBOState:
    """ScoreGradELBOState(problem, obj_ad_prep): scoregradelbo.jl:19-22; `obj_ad_prep` is the libmivi context."""

    def __init__(self, problem, ctx: MiviContext):
        self.problem = problem
        self.obj_ad_prep = ctx


def _order0(prob) -> bool:
    """capability < LogDensityOrder{1}() (repgradelbo.jl:50-51), looking through a TransformedProblem like README.md:115-119."""
    inner = prob.prob if isinstance(prob, P.TransformedProblem) else prob
    return not isinstance(inner, P.BUILTIN) and P.capabilities(inner) < P.LogDensityOrder(1)


def _ad_problem(adtype, prob, announce=True):
    """The capability dispatch of `init` / `set_objective_state_problem` (repgradelbo.jl:31-39, 50-62).  Order >= 1: the problem's own
    `logdensity_and_gradient` is used (the MixedADLogDensityProblem route).  Order 0: the reference differentiates through `logdensity`
    with the AD backend; AutoMIVI's estimator has none, so the TARGET is wrapped in ADgradient(adtype.target_ad, prob) -- what
    README.md:168-174 does by hand -- and the reference's @info is emitted."""
    if not _order0(prob):
        return prob
    kind = getattr(adtype, "target_ad", None)
    cap = P.capabilities(prob.prob if isinstance(prob, P.TransformedProblem) else prob)
    if kind is None:
        raise TypeError(
            f"The capability of the supplied LogDensityProblem {cap} is less than LogDensityOrder{{1}}(): "
            "AutoMIVI(target_ad=None) has no AD backend to differentiate `logdensity`; supply `logdensity_and_gradient` "
            "or construct AutoMIVI(target_ad=\"forwarddiff\").")
    if announce:
        _log.info("The capability of the supplied `LogDensityProblem` %s is less than %s. `AdvancedVI` will attempt to directly "
                  "differentiate through `LogDensityProblems.logdensity`. If this is not intended, please supply a log-density problem "
                  "with capability at least %s", cap, P.LogDensityOrder(1), P.LogDensityOrder(1))
    if isinstance(prob, P.TransformedProblem):   # the bijector stays on the device; AD only sees the constrained-scale target
        return P.TransformedProblem(P.ADgradient(kind, prob.prob), prob.bijector)
    return P.ADgradient(kind, prob)


_NO_FLOW_ENTROPY = ("a normalizing flow ({}) has no entropy(q): {} cannot be used with it -- use `MonteCarloEntropy()` or "
                    "`StickingTheLandingEntropy()` (docs/src/tutorials/flows.md:213)")


def _make_ctx(rng, obj, adtype, q, prob, n_mc=None, entropy=None):
    if not isinstance(q, (MvLocationScale, MvLocationScaleLowRank) + COUPLING_FLOWS):
        raise TypeError("libmivi implements the RepGradELBO path for MvLocationScale, MvLocationScaleLowRank, RealNVP and NeuralSplineFlow families only")
    ent = entropy or obj.entropy
    if isinstance(q, COUPLING_FLOWS) and ent.code not in (MonteCarloEntropy.code, StickingTheLandingEntropy.code):
        raise TypeError(_NO_FLOW_ENTROPY.format(FLOW_NAMES[q.family], f"`{type(ent).__name__}`"))
    device = getattr(adtype, "device", 0)
    ctx = MiviContext(q.eltype, q.family, len(q), n_mc or obj.n_samples,
                      ent.code, rng.seed, device=device, rank=getattr(q, "rank", 0), flow=_flow_arch(q))
    try:
        ctx.set_base_dist(getattr(q, "dist", None))   # MvLocationScale(location, scale, dist); the low-rank family: Normal() only
        ctx.set_problem(prob)
    except Exception:
        ctx.close()
        raise
    return ctx


def _make_score_ctx(rng, obj, adtype, q, prob):
    if isinstance(q, COUPLING_FLOWS):
        raise TypeError(f"ScoreGradELBO is not implemented for a normalizing flow ({FLOW_NAMES[q.family]}): use RepGradELBO (KLMinRepGradDescent) with "
                        "`MonteCarloEntropy()` or `StickingTheLandingEntropy()`")
    if isinstance(q, MvLocationScaleLowRank):
        raise TypeError("ScoreGradELBO is not implemented for the low-rank family (MvLocationScaleLowRank): use RepGradELBO "
                        "(KLMinRepGradDescent), or a MeanFieldGaussian / FullRankGaussian")
    if not isinstance(q, MvLocationScale):
        raise TypeError("libmivi implements the ScoreGradELBO path for MvLocationScale families only")
    if q.dist.code != 0:
        raise TypeError(f"ScoreGradELBO is not implemented for the base distribution {q.dist!r}: use RepGradELBO (KLMinRepGradDescent), "
                        "or a family with dist = Normal()")
    ctx = MiviContext(q.eltype, q.family, len(q), obj.n_samples, MonteCarloEntropy.code, rng.seed, device=getattr(adtype, "device", 0))
    ctx.set_problem(prob, values_only=True)
    return ctx


def init(rng, obj, adtype, q, prob, params, restructure):
    """AdvancedVI.init(rng, obj::RepGradELBO, adtype, q, prob, params, restructure): repgradelbo.jl:41-70.
    The capability dispatch of :50-62: order >= 1 problems are used through `logdensity_and_gradient`; an order-0 problem (only
    `logdensity`: the README model, README.md:64-66, and the benchmark target, bench/benchmarks.jl:39-41) is differentiated on the host
    by `adtype.target_ad` with the reference's @info -- see `_ad_problem`."""
    if not isinstance(adtype, AutoMIVI):
        raise TypeError("adtype must be AutoMIVI() for the libmivi path")
    if isinstance(obj, ScoreGradELBO):
        # scoregradelbo.jl:34-50: no capability dispatch, no ADgradient wrapping, no @info -- only `logdensity` is ever evaluated, so an
        # order-0 problem is used as it is (the value-only callback)
        st = ScoreGradELBOState(prob, _make_score_ctx(rng, obj, adtype, q, prob))
        st.adtype = adtype
        return st
    ad_prob = _ad_problem(adtype, prob)
    st = RepGradELBOState(ad_prob, _make_ctx(rng, obj, adtype, q, ad_prob))
    st.adtype = adtype
    return st


def set_objective_state_problem(state, prob):
    """repgradelbo.jl:31-39 (the same capability dispatch as `init`, without the @info); scoregradelbo.jl:24-32 for a ScoreGradELBOState
    (the problem is used as it is)."""
    if isinstance(state, ScoreGradELBOState):
        state.obj_ad_prep.set_problem(prob, values_only=True)
        st = ScoreGradELBOState(prob, state.obj_ad_prep)
        st.adtype = getattr(state, "adtype", None)
        return st
    adtype = getattr(state, "adtype", None)
    ad_prob = _ad_problem(adtype, prob, announce=False) if adtype is not None else prob
    state.obj_ad_prep.set_problem(ad_prob)
    st = RepGradELBOState(ad_prob, state.obj_ad_prep)
    st.adtype = adtype
    return st


def estimate_gradient_(rng, obj, adtype, out: DiffResult, state, params, restructure,
                       *args):
    """`estimate_gradient!`: repgradelbo.jl:151-177.  Writes -elbo and its gradient into `out`
    (both device resident), returns (out, state, info) with info = {"elbo": -value}.  `info["elbo"]`
    is a 0-dim device tensor so the call stays asynchronous; `float()` it to synchronise.
    obj::ScoreGradELBO (scoregradelbo.jl:96-117): `out.value` is the VarGrad objective, `info["elbo"]` the separate scalar
    mean(log pi - log q) over the same samples."""
    ctx = state.obj_ad_prep
    if isinstance(obj, ScoreGradELBO):
        elbo = ctx.empty(1)
        ctx.estimate_score_gradient(params, rng.next_index(), out.value_t, elbo, out.gradient_t)
        return out, state, {"elbo": elbo[0]}
    ctx.estimate_gradient(params, rng.next_index(), out.value_t, out.gradient_t)
    info = {"elbo": -out.value_t[0]}
    return out, state, info


def estimate_objective(rng, obj, q, prob=None, n_samples: int = None, adtype=None, _ctx_cache={}):
    """estimate_objective(rng, obj::RepGradELBO, q, prob; n_samples): repgradelbo.jl:112-118 (q_stop := q).
    Returns the NEGATIVE elbo as a Python float."""
    if isinstance(rng, (RepGradELBO, ScoreGradELBO)):  # estimate_objective(obj, q, prob): default rng, repgradelbo.jl:120-122
        rng, obj, q, prob = default_rng(), rng, obj, q
    if isinstance(obj, ScoreGradELBO):
        # scoregradelbo.jl:58-65: -mean(log pi - log q) -- the value route with the Monte-Carlo entropy (values of the target only)
        n = int(n_samples) if n_samples is not None else obj.n_samples
        return estimate_objective(rng, RepGradELBO(n, entropy=MonteCarloEntropy()), q, prob, adtype=adtype)
    n = int(n_samples) if n_samples is not None else obj.n_samples
    ctx = _make_ctx(rng, obj, adtype or AutoMIVI(), q, prob, n_mc=min(n, 16384))
    try:
        params, _ = destructure(q)
        v = ctx.estimate_objective(params, rng.next_index(), n_samples=n, entropy=obj.entropy.code)
        return float(v.item())
    finally:
        ctx.close()


class TransformedDistribution:
    """Bijectors.TransformedDistribution(q, binv) (docs/src/tutorials/basic.md:210-247, constrained.md:228-231): the variational
    approximation on the constrained scale -- `q` a fitted family on the unconstrained scale, `bijector` the P.StackedBijector whose
    inverse maps its draws to the support.  rand(rng, qt, n) samples it, logpdf(qt, x) scores constrained points."""

    def __init__(self, q, bijector: P.StackedBijector):
        if not isinstance(bijector, P.StackedBijector):
            raise TypeError("TransformedDistribution(q, bijector): bijector must be a StackedBijector")
        for lo, hi, _ in bijector.blocks:
            if lo < 0 or hi > len(q) or lo > hi:
                raise ValueError(f"bijector block [{lo}, {hi}) lies outside the {len(q)} coordinates of q")
        # (not `dist`: on a family that attribute is the BASE distribution, and a helper handed this object must not take one for the other)
        self.q = q
        self.bijector = bijector

    def __len__(self):
        return len(self.q)


def _plain_entropy(q):
    """the estimator code of a context that only samples or scores q (never read there): a flow context admits no closed-form kind"""
    return MonteCarloEntropy.code if isinstance(q, COUPLING_FLOWS) else 0


def rand(rng, q, num_samples: int, device: int = 0):
    """rand(rng, q, num_samples): d x num_samples samples (location_scale.jl:71-87, location_scale_low_rank.jl:66-100), returned as a
    device tensor (column m = sample m).  q::TransformedDistribution: the draws of q.q pushed through the bijector (constrained)."""
    qt, q = (q, q.q) if isinstance(q, TransformedDistribution) else (None, q)
    ctx = MiviContext(q.eltype, q.family, len(q), num_samples, _plain_entropy(q), rng.seed, device=device, rank=getattr(q, "rank", 0),
                      flow=_flow_arch(q))
    try:
        ctx.set_base_dist(getattr(q, "dist", None))
        params, _ = destructure(q)
        if qt is not None:
            ctx.set_bijector(qt.bijector)
            return ctx.sample_constrained(params, rng.next_index()).clone()
        return ctx.sample(params, rng.next_index(), want_eps=False).clone()
    finally:
        ctx.close()


def logpdf(q, z, device: int = 0):
    """logpdf(q, z): Distributions.logpdf of the variational family at the caller's points (location_scale.jl:59-63,
    location_scale_low_rank.jl:45-68) -- MvLocationScale with a diagonal or triangular scale and any `dist`, MvLocationScaleLowRank.
    z of shape (d,): a Python float.  z of shape (d, n), numpy or device tensor: a device tensor of n values in q.eltype.
    q::TransformedDistribution: z are constrained points, the value is log q.q(b(z)) - logabsdetjac(binv, b(z)); -inf outside the support."""
    qt, q = (q, q.q) if isinstance(q, TransformedDistribution) else (None, q)
    ctx = MiviContext(q.eltype, q.family, len(q), 1, _plain_entropy(q), 0, device=device, rank=getattr(q, "rank", 0), flow=_flow_arch(q))
    try:
        ctx.set_base_dist(getattr(q, "dist", None))
        params, _ = destructure(q)
        single = getattr(z, "ndim", None) == 1 or (not hasattr(z, "ndim") and np.ndim(z) == 1)
        if single and len(z) != len(q):
            raise ValueError(f"logpdf: z has {len(z)} entries, q has dimension {len(q)}")
        if qt is not None:
            ctx.set_bijector(qt.bijector)
        out = ctx.logpdf_constrained(params, z) if qt is not None else ctx.logpdf(params, z)
        ctx.synchronize()   # (a non-positive scale diagonal raises here, like the reference's DomainError)
        return float(out.item()) if single else out
    finally:
        ctx.close()


def gaussian_expectation_gradient_and_hessian_(rng, q: MvLocationScale, n_samples: int, grad_buf, hess_buf, prob,
                                               adtype=None, _ctx=None):
    """`gaussian_expectation_gradient_and_hessian!(rng, q, n_samples, grad_buf, hess_buf, prob)`:
    src/algorithms/gauss_expected_grad_hess.jl:20-60, the Stein / Price-identity branch (what a target with
    `logdensity_and_gradient` takes, :32-60).  `grad_buf` (d) / `hess_buf` (d*d, column-major) are device tensors
    that are overwritten, or None to allocate.  Returns (logpi_avg: float, grad (d), hess (d, d)) -- `hess` is not
    symmetrised, like the reference's.  A target whose `capabilities` exceed LogDensityOrder(1) -- a plugin with
    `logdensity_gradient_and_hessian`, or a built-in Gaussian problem constructed with order=2 -- takes the reference's second-order
    branch (:61-83): the sample average of the Hessians, no Stein identity (mivi_gauss_expected_grad_hess2)."""
    if not isinstance(q, MvLocationScale) or q.family != 1:
        raise TypeError("gaussian_expectation_gradient_and_hessian_ expects a Gaussian with a triangular scale "
                        "(gauss_expected_grad_hess.jl:22)")
    ctx = _ctx
    if ctx is None:
        ctx = MiviContext(q.eltype, q.family, len(q), min(int(n_samples), 16384), 0, rng.seed,
                          device=getattr(adtype, "device", 0))
        ctx.set_problem(prob)
    try:
        params, _ = destructure(q)
        from .problems import LogDensityOrder, capabilities
        second = LogDensityOrder(1) < capabilities(prob)          # (the reference's branch test, gauss_expected_grad_hess.jl:31-32)
        logpi, g, H = ctx.gauss_expected_grad_hess(params, rng.next_index(), int(n_samples), grad_buf, hess_buf, second_order=second)
        return float(logpi.item()), g, H
    finally:
        if _ctx is None:
            ctx.close()
