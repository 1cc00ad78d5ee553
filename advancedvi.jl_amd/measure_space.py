"""Measure-space algorithms: KLMinSqrtNaturalGradDescent, KLMinNaturalGradDescent, FisherMinBatchMatch and KLMinWassFwdBwd, the host-side
mirrors of src/algorithms/klminsqrtnaturalgraddescent.jl, klminnaturalgraddescent.jl, fisherminbatchmatch.jl and klminwassfwdbwd.jl
(AdvancedVI.jl v0.7.0) over libmivi.

    KLMinSqrtNaturalGradDescent(stepsize, n_samples=1, subsampling=None)     :39-44
    init(rng, alg, q_init, prob)                                             :55-75
    step(rng, alg, state, callback) -> (state, False, info)                  :79-127
    output(alg, state) = state.q, the last iterate                           :77
    estimate_objective([rng,] alg, q, prob; n_samples)                       :146-165

The variational parameters [m; vec(C)] stay resident in HBM between steps.  A step is the tuned inner estimator
(mivi_gauss_expected_grad_hess / _hess2, chosen by the target's capability like gauss_expected_grad_hess.jl:31-32) followed by
mivi_sqrt_ngd_update; `optimize` without a callback and without subsampling runs whole chunks of steps inside mivi_sqrt_ngd_steps, with
bitwise the same iterates as the host-driven `step` loop.

KLMinNaturalGradDescent(stepsize, n_samples=1, ensure_posdef=True, subsampling=None) (klminnaturalgraddescent.jl:56-62; init :64-91, step
:95-153, output :93, estimate_objective :172-192) is the same loop around mivi_natgrad_update / mivi_natgrad_steps; besides the parameters
its state carries the device buffer [S; Sigma] (precision and covariance, :83-87, mivi_natgrad_init).  The two algorithms differ in their
update call and that one buffer; everything else below is shared.  Scale convention: the reference's new scale is upper triangular (the
adjoint of the inverse of a lower Cholesky factor of S'); this library's iterate carries the LOWER Cholesky factor C' of Sigma' = S'^-1 --
the same distribution, the same recursion in (m, S, Sigma); only the pairing of draws with samples differs.

FisherMinBatchMatch(n_samples=32, subsampling=None) (fisherminbatchmatch.jl:40-44; init :56-77, step :113-167, output :79, estimate_objective
:186-195) minimises the covariance-weighted Fisher divergence ("batch and match"): gradients only, no step size.  Its step is
mivi_bam_moments followed by mivi_bam_update (whole chunks inside mivi_bam_steps); its state carries the device buffer Sigma (:76).  Its
new scale is the lower Cholesky factor of Sigma', as in the reference.  `info` carries `covweighted_fisher` and `elbo`, both at the iterate
the step STARTED from (:157-158).  The callback is called as the reference's CODE calls it (:163) -- callback(rng=, iteration=, q=, state=)
with q the iterate the step started from and the new state -- which disagrees with the reference's docstring for `optimize` (q the new
iterate, `info` instead of `state`); the code is what users' callbacks run against.

KLMinWassFwdBwd(stepsize, n_samples=1, subsampling=None) (klminwassfwdbwd.jl:39-44; init :56-76, step :80-122, output :78,
estimate_objective :141-160) is stochastic proximal gradient descent in Wasserstein space: the loop of the two natural-gradient algorithms
around mivi_wass_update / mivi_wass_steps; its state carries the device buffer Sigma (:75, mivi_wass_init).  Its new scale is the lower
Cholesky factor of Sigma', as in the reference, and its callback receives the new iterate and `info` (:118)."""
from __future__ import annotations

from . import objectives as O
from . import problems as P
from . import subsampling as S
from .context import BAM_MAX_SAMPLES, MiviContext
from .families import FLOW_FAMILIES, FLOW_NAMES, FULLRANK, MvLocationScale, destructure


class KLMinSqrtNaturalGradDescent:
    """KL minimisation by discretising the natural-gradient flow under the square-root parameterisation
    (klminsqrtnaturalgraddescent.jl:2-44).  Needs a full-rank Gaussian family and a target with at least first-order capability; a target
    with second-order capability has its Hessians used, otherwise the Stein identity on gradients."""

    def __init__(self, stepsize, n_samples: int = 1, subsampling=None, device: int = 0):
        if not isinstance(n_samples, int) or n_samples < 1:
            raise ValueError("n_samples must be a positive Int")
        self.stepsize = float(stepsize)
        self.n_samples = int(n_samples)
        self.subsampling = subsampling
        self.device = int(device)

    def __repr__(self):
        return f"KLMinSqrtNaturalGradDescent(stepsize={self.stepsize}, n_samples={self.n_samples}, subsampling={self.subsampling})"


class KLMinNaturalGradDescent:
    """KL minimisation by natural-gradient descent on the Gaussian's precision, also known as variational online Newton
    (klminnaturalgraddescent.jl:2-62).  Needs a full-rank Gaussian family and a target with at least first-order capability; a target with
    second-order capability has its Hessians used, otherwise the Stein identity on gradients.  `ensure_posdef` selects the update of the
    precision that stays positive definite for any Hessian estimate (:129-130) over the plain convex combination (:132); like the reference,
    the first-order branch does not require it.  The scale of the iterates is the lower Cholesky factor of the covariance (the reference's is
    an upper-triangular factor of the same covariance: see the module docstring)."""

    def __init__(self, stepsize, n_samples: int = 1, ensure_posdef: bool = True, subsampling=None, device: int = 0):
        if not isinstance(n_samples, int) or n_samples < 1:
            raise ValueError("n_samples must be a positive Int")
        self.stepsize = float(stepsize)
        self.n_samples = int(n_samples)
        self.ensure_posdef = bool(ensure_posdef)
        self.subsampling = subsampling
        self.device = int(device)

    def __repr__(self):
        return (f"KLMinNaturalGradDescent(stepsize={self.stepsize}, n_samples={self.n_samples}, ensure_posdef={self.ensure_posdef}, "
                f"subsampling={self.subsampling})")


class FisherMinBatchMatch:
    """Covariance-weighted Fisher divergence minimisation by the batch-and-match updates (fisherminbatchmatch.jl:2-44).  Needs a full-rank
    Gaussian family, unconstrained support and a target with at least first-order capability; 2 <= n_samples <= BAM_MAX_SAMPLES."""

    def __init__(self, n_samples: int = 32, subsampling=None, device: int = 0):
        if not isinstance(n_samples, int) or n_samples < 2:
            raise ValueError("n_samples must be an Int of at least 2 (the corrected sample covariance needs two samples)")
        if n_samples > BAM_MAX_SAMPLES:
            raise ValueError(f"n_samples must be at most {BAM_MAX_SAMPLES} (MIVI_BAM_MAX_SAMPLES)")
        self.n_samples = int(n_samples)
        self.subsampling = subsampling
        self.device = int(device)

    def __repr__(self):
        return f"FisherMinBatchMatch(n_samples={self.n_samples}, subsampling={self.subsampling})"


class KLMinWassFwdBwd:
    """KL minimisation by stochastic proximal gradient descent (forward-backward splitting) in Wasserstein space (klminwassfwdbwd.jl:2-44).
    Needs a full-rank Gaussian family and a target with at least first-order capability; a target with second-order capability has its
    Hessians used, otherwise the Stein identity on gradients."""

    def __init__(self, stepsize, n_samples: int = 1, subsampling=None, device: int = 0):
        if not isinstance(n_samples, int) or n_samples < 1:
            raise ValueError("n_samples must be a positive Int")
        self.stepsize = float(stepsize)
        self.n_samples = int(n_samples)
        self.subsampling = subsampling
        self.device = int(device)

    def __repr__(self):
        return f"KLMinWassFwdBwd(stepsize={self.stepsize}, n_samples={self.n_samples}, subsampling={self.subsampling})"


ALGORITHMS = (KLMinSqrtNaturalGradDescent, KLMinNaturalGradDescent, FisherMinBatchMatch, KLMinWassFwdBwd)
STATE_BUFFERS = ("natgrad", "bam", "wass")   # the device buffers, besides the parameters, that a step advances in place


def _second_order(prob) -> bool:
    """LogDensityOrder{1}() < capabilities(prob): the branch test of gauss_expected_grad_hess.jl:31-32."""
    return P.LogDensityOrder(1) < P.capabilities(prob)


def _update(alg, ctx, state, grad, hess):
    """The algorithm's update of state["params"] (and of its own state buffer) in place; returns entropy(q') as a 1-element device tensor."""
    if isinstance(alg, KLMinNaturalGradDescent):
        return ctx.natgrad_update(state["params"], state["natgrad"], grad, hess, alg.stepsize, alg.ensure_posdef)
    if isinstance(alg, KLMinWassFwdBwd):
        return ctx.wass_update(state["params"], state["wass"], grad, hess, alg.stepsize)
    return ctx.sqrt_ngd_update(state["params"], grad, hess, alg.stepsize)


def _device_steps(alg, ctx, state, idx0, n, second):
    """`n` whole steps inside the library; returns their elbo (a device tensor) -- batch and match: (elbo, fisher)."""
    if isinstance(alg, FisherMinBatchMatch):
        fisher, elbo = ctx.bam_steps(state["params"], state["bam"], idx0, state["iteration"] + 1, n, alg.n_samples)
        return elbo, fisher
    if isinstance(alg, KLMinNaturalGradDescent):
        return ctx.natgrad_steps(state["params"], state["natgrad"], idx0, n, alg.stepsize, alg.ensure_posdef, n_samples=alg.n_samples,
                                 second_order=second)
    if isinstance(alg, KLMinWassFwdBwd):
        return ctx.wass_steps(state["params"], state["wass"], idx0, n, alg.stepsize, n_samples=alg.n_samples, second_order=second)
    return ctx.sqrt_ngd_steps(state["params"], idx0, n, alg.stepsize, n_samples=alg.n_samples, second_order=second)


def _own_buffers(state):
    """The state with copies of the device buffers a step advances in place."""
    state = dict(state, params=state["params"].clone())
    for k in STATE_BUFFERS:
        if k in state:
            state[k] = state[k].clone()
    return state


def init(rng, alg, q_init, prob):
    """klminsqrtnaturalgraddescent.jl:55-75 / klminnaturalgraddescent.jl:64-91 / fisherminbatchmatch.jl:56-77 / klminwassfwdbwd.jl:56-76."""
    name = type(alg).__name__
    if getattr(q_init, "family", None) in FLOW_FAMILIES:
        raise TypeError(f"`{name}` updates a Gaussian's location and scale: it has no method for a normalizing flow ({FLOW_NAMES[q_init.family]}) -- use "
                        "`KLMinRepGradDescent` with `StickingTheLandingEntropy()` and `IdentityOperator()`")
    if not isinstance(q_init, MvLocationScale) or q_init.family != FULLRANK:
        raise TypeError(f"`{name}` expects a Gaussian with a lower-triangular scale (FullRankGaussian) as q_init")
    if q_init.dist.code != 0:   # (the reference types these algorithms on FullRankGaussian)
        raise TypeError(f"`{name}` expects a Gaussian q_init (FullRankGaussian): the base distribution {q_init.dist!r} is not Normal()")
    capability = P.capabilities(prob)
    if capability < P.LogDensityOrder(1):   # :64-70 of either file (ArgumentError)
        raise ValueError(f"`{name}` requires at least first-order differentiation capability. The capability of the "
                         f"supplied `LogDensityProblem` is {capability}.")
    sub_st = None if alg.subsampling is None else S.init_subsampling(rng, alg.subsampling)
    params_h, re = destructure(q_init)
    ctx = MiviContext(q_init.eltype, FULLRANK, len(q_init), min(alg.n_samples, 16384), O.ClosedFormEntropy.code, rng.seed, device=alg.device)
    ctx.set_problem(prob)
    d = len(q_init)
    state = dict(q=q_init, prob=prob, iteration=0, sub_st=sub_st, ctx=ctx, params=ctx.to_device(params_h).clone(), restructure=re)
    if isinstance(alg, FisherMinBatchMatch):       # :74-76: u_buf, grad_buf and cov(q), carried from step to step
        state.update(u_buf=ctx.empty(d * alg.n_samples), grad_buf=ctx.empty(d * alg.n_samples), bam=ctx.bam_init(state["params"]))
        return state
    state.update(grad_buf=ctx.empty(d), hess_buf=ctx.empty(d * d))
    if isinstance(alg, KLMinNaturalGradDescent):   # :83-87: prec and qcov, carried from step to step
        state["natgrad"] = ctx.natgrad_init(state["params"])
    if isinstance(alg, KLMinWassFwdBwd):           # klminwassfwdbwd.jl:75: cov(q_init), carried from step to step
        state["wass"] = ctx.wass_init(state["params"])
    return state


def _q_of(state):
    if state["q"] is None:
        state["q"] = state["restructure"](state["params"].cpu().numpy())
    return state["q"]


def output(alg, state):
    """output(alg, state) = state.q: the last iterate, no averaging (klminsqrtnaturalgraddescent.jl:77, klminnaturalgraddescent.jl:93)."""
    return _q_of(state)


def step(rng, alg, state, callback, *objargs):
    """klminsqrtnaturalgraddescent.jl:79-127 / klminnaturalgraddescent.jl:95-153.  The parameters (and [S; Sigma]) live in ONE device buffer
    each that the update advances in place: the state passed in is consumed by the call (use the returned one; `optimize(state=...)` works on a copy of the buffer and leaves its argument as it was)."""
    state = dict(state)
    ctx, params = state["ctx"], state["params"]
    q_start = _q_of(state) if isinstance(alg, FisherMinBatchMatch) and callback is not None else None   # (:163 hands the callback the OLD iterate)
    state["iteration"] += 1
    prob_sub, sub_inf = state["prob"], {}
    if alg.subsampling is not None:   # :96-102
        batch, state["sub_st"], sub_inf = S.step_subsampling(rng, alg.subsampling, state["sub_st"])
        prob_sub = P.subsample(state["prob"], batch)
        ctx.set_problem(prob_sub)
    if isinstance(alg, FisherMinBatchMatch):   # fisherminbatchmatch.jl:139-166
        d, n = ctx.d, alg.n_samples
        u, G, fisher, _, elbo = ctx.bam_moments(params, rng.next_index(), n, state["u_buf"], state["grad_buf"])
        lam = ctx.np_dtype.type(d * n / state["iteration"])   # convert(eltype(mu), d * n_samples / iteration) (:148)
        ctx.bam_update(params, state["bam"], u, G, n, float(lam))
        info = {"iteration": state["iteration"], "covweighted_fisher": float(fisher.item()), "elbo": float(elbo.item()), **sub_inf}
        ctx.synchronize()
        state["q"] = None
        if callback is not None:
            extra = callback(rng=rng, iteration=state["iteration"], q=q_start, state=state)
            if extra is not None:
                info = {**extra, **info}
        return state, False, info
    logpi, grad, _ = ctx.gauss_expected_grad_hess(params, rng.next_index(), alg.n_samples, state["grad_buf"], state["hess_buf"],
                                                  second_order=_second_order(prob_sub))
    entropy = _update(alg, ctx, state, grad, state["hess_buf"])
    elbo = float((logpi + entropy).item())   # (one addition in the context's dtype: what the device step loops record)
    ctx.synchronize()                        # a scale diagonal / pivot that left the positive numbers raises here (MIVI_ERR_NONPOSITIVE_SCALE)
    state["q"] = None                        # materialised lazily by `output` / callbacks (the parameters are device resident)
    info = {"elbo": elbo, **sub_inf}
    if callback is not None:
        extra = callback(rng=rng, iteration=state["iteration"], q=_q_of(state), info=info)
        if extra is not None:
            info = {**extra, **info}
    return state, False, info


def estimate_objective(rng, alg, q=None, prob=None, n_samples=None):
    """estimate_objective([rng,] alg, q, prob; n_samples): klminsqrtnaturalgraddescent.jl:146-165 / klminnaturalgraddescent.jl:172-192 -- the
    negative ELBO with the Monte-Carlo entropy; with subsampling, the average over one pass through the batches."""
    if isinstance(rng, ALGORITHMS):
        rng, alg, q, prob = O.default_rng(), rng, alg, q
    n = int(n_samples) if n_samples is not None else alg.n_samples
    if isinstance(alg, FisherMinBatchMatch):   # fisherminbatchmatch.jl:186-195: the covariance-weighted Fisher divergence (no subsampling there)
        if not isinstance(q, MvLocationScale) or q.family != FULLRANK:
            raise TypeError("`FisherMinBatchMatch` expects a Gaussian with a lower-triangular scale (FullRankGaussian)")
        ctx = MiviContext(q.eltype, FULLRANK, len(q), min(n, 16384), O.ClosedFormEntropy.code, rng.seed, device=alg.device)
        ctx.set_problem(prob)
        value = float(ctx.estimate_fisher(destructure(q)[0], rng.next_index(), n).item())
        ctx.synchronize()
        ctx.close()
        return value
    obj = O.RepGradELBO(n, entropy=O.MonteCarloEntropy())
    adtype = O.AutoMIVI(device=alg.device)
    if alg.subsampling is None:
        return O.estimate_objective(rng, obj, q, prob, adtype=adtype)
    return S.estimate_objective(rng, S.SubsampledObjective(obj, alg.subsampling), q, prob, adtype=adtype)


def _steps_on_device(rng, alg, max_iter, state, show_progress):
    from .optimize import DEVICE_LOOP_CHUNK
    ctx = state["ctx"]
    second = _second_order(state["prob"])
    info_total, done = [], 0
    while done < max_iter:
        n = min(DEVICE_LOOP_CHUNK, max_iter - done)
        out = _device_steps(alg, ctx, state, rng.counter, n, second)
        ctx.synchronize()
        for _ in range(n):
            rng.next_index()
        if isinstance(out, tuple):   # batch and match: the step's own `iteration` (:158) is the state's, as the host-driven loop reports it
            vals, fish = out[0].cpu().numpy(), out[1].cpu().numpy()
            info_total += [{"iteration": done + i + 1, "covweighted_fisher": float(fish[i]), "elbo": float(vals[i])} for i in range(n)]
        else:
            vals = out.cpu().numpy()
            info_total += [{"elbo": float(vals[i]), "iteration": done + i + 1} for i in range(n)]
        state["iteration"] += n
        state["q"] = None
        done += n
        if show_progress:
            print(f"\rOptimizing {done}/{max_iter} elbo={info_total[-1]['elbo']:.6g}", end="" if done < max_iter else "\n")
    return info_total


def optimize(rng, algorithm, max_iter: int, prob=None, q_init=None, *objargs, show_progress=False, state=None, callback=None,
             device_loop=True):
    """optimize([rng,] algorithm, max_iter, prob, q_init; show_progress, state, callback): src/optimize.jl:42-94 for this algorithm.
    Returns (output, info, state)."""
    if isinstance(rng, ALGORITHMS):   # default-rng overload, optimize.jl:83-94
        rng, algorithm, max_iter, prob, q_init = O.default_rng(), rng, algorithm, max_iter, prob
    if state is None:
        state = init(rng, algorithm, q_init, prob)
    else:   # a warm start: the caller's state (its device buffers and cached q) stays what it was
        state = _own_buffers(state)
    if device_loop and callback is None and algorithm.subsampling is None and not objargs and max_iter > 0:
        state = dict(state)
        info_total = _steps_on_device(rng, algorithm, max_iter, state, show_progress)
        return output(algorithm, state), info_total, state
    info_total = []
    for t in range(1, max_iter + 1):
        state, terminate, info = step(rng, algorithm, state, callback, *objargs)
        info = {**info, "iteration": t}
        if terminate:
            break
        if show_progress:
            print(f"\rOptimizing {t}/{max_iter} elbo={info['elbo']:.6g}", end="" if t < max_iter else "\n")
        info_total.append(info)
    return output(algorithm, state), info_total, state
