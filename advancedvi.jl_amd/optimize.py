"""Callers of the hot path: KLMinRepGradDescent (= ADVI), init / step / output and `optimize`.
Host-side mirror of src/algorithms/constructors.jl:44-79, src/algorithms/common.jl:29-120 and
src/optimize.jl:42-94 (AdvancedVI.jl v0.7.0); parameters stay resident in HBM between steps and every
update is a libmivi kernel."""
from __future__ import annotations

import warnings

import numpy as np

from . import objectives as O
from . import subsampling as S
from .families import COUPLING_FLOWS, FLOW_FAMILIES, FLOW_NAMES, LOWRANK, MvLocationScale, MvLocationScaleLowRank, destructure


# --- operators (src/optimization/clip_scale.jl, src/AdvancedVI.jl:173-204) ------------------------
class IdentityOperator:
    def apply(self, ctx, params, optimizer=None, opt_st=None):
        return params


class ClipScale:
    """ClipScale(eps = 1e-5): src/optimization/clip_scale.jl:8-29."""

    def __init__(self, epsilon=1e-5):
        self.epsilon = epsilon

    def apply(self, ctx, params, optimizer=None, opt_st=None):
        if ctx.family in FLOW_FAMILIES:
            raise TypeError(_NO_SCALE_FLOW.format("ClipScale", FLOW_NAMES[ctx.family]))
        ctx.clip_scale(params, self.epsilon)
        return params


_NO_PROX_LOWRANK = ("`ProximalLocationScaleEntropy` has no method for the low-rank family (MvLocationScaleLowRank), as in the reference "
                    "(proximal_location_scale_entropy.jl:44): use `ClipScale`")


_NO_SCALE_FLOW = ("`{}` has no method for a normalizing flow ({}): the family has no scale -- use `IdentityOperator()` "
                  "(docs/src/tutorials/flows.md:212-215)")


class ProximalLocationScaleEntropy:
    """Proximal operator of the entropy of a location-scale family, applied after the optimiser step with that step's
    size: src/optimization/proximal_location_scale_entropy.jl:17-61.  Supports Descent, DoG, DoWG (:26-42); the DoG/DoWG
    step size is read from the optimiser state on the device."""

    def apply(self, ctx, params, optimizer=None, opt_st=None):
        if ctx.family == LOWRANK:
            raise TypeError(_NO_PROX_LOWRANK)
        if ctx.family in FLOW_FAMILIES:
            raise TypeError(_NO_SCALE_FLOW.format("ProximalLocationScaleEntropy", FLOW_NAMES[ctx.family]))
        if isinstance(optimizer, DoG):            # DoWG is a subclass
            ctx.prox_scale_entropy(params, 0.0, opt_st, optimizer.kind)
        elif isinstance(optimizer, Descent):
            ctx.prox_scale_entropy(params, optimizer.eta)
        else:
            raise TypeError(f"`ProximalLocationScaleEntropy` does not support optimization rule {type(optimizer).__name__}.")
        return params


# --- optimisation rules (Optimisers.jl rules used by the reference's tests/bench) -----------------
class Descent:
    def __init__(self, eta=0.1):
        self.eta = eta

    def setup(self, ctx, params):
        return None

    def update(self, ctx, state, params, grad, t):
        ctx.descent_update(params, grad, self.eta)
        return state


class Adam:
    def __init__(self, eta=1e-3, beta=(0.9, 0.999), epsilon=1e-8):
        self.eta, self.beta, self.epsilon = eta, beta, epsilon

    def setup(self, ctx, params):
        import torch
        return torch.zeros(2 * params.numel(), dtype=params.dtype, device=params.device)

    def update(self, ctx, state, params, grad, t):
        ctx.adam_update(params, grad, state, t, self.eta, self.beta[0], self.beta[1], self.epsilon)
        return state


class DoG:
    """src/optimization/rules.jl:48-64."""
    kind = 0

    def __init__(self, alpha=1e-6):
        self.alpha = alpha

    def setup(self, ctx, params):
        st = ctx.dog_state()
        ctx.dog_init(params, st, self.alpha)
        return st

    def update(self, ctx, state, params, grad, t):
        ctx.dog_update(params, grad, state, self.kind)
        return state


class DoWG(DoG):
    """src/optimization/rules.jl:17-34."""
    kind = 1


class COCOB:
    """src/optimization/rules.jl:78-96 (COCOB-Backprop); state (L, G, R, theta, x1) = (0, 0, 0, 0, params) (:84-86).
    Device-resident in `optimize` (mivi_optimize_loop rule 4: a hipGraph of chained estimates + the update kernel, no host round trip per
    step); `update` below is the host-driven `step` loop's launch."""

    def __init__(self, alpha=100):
        self.alpha = alpha

    def setup(self, ctx, params):
        import torch
        n = params.numel()
        st = torch.zeros(5 * n, dtype=params.dtype, device=params.device)
        st[4 * n:] = params
        return st

    def update(self, ctx, state, params, grad, t):
        ctx.cocob_update(params, grad, state, self.alpha)
        return state


# --- averagers (src/optimization/averaging.jl) -----------------------------------------------------
class NoAveraging:
    def init(self, ctx, params):
        return params

    def apply(self, ctx, state, params):
        return params

    def value(self, state):
        return state


class PolynomialAveraging:
    """x_bar_t = (1 - w_t) x_bar_{t-1} + w_t x_t, w_t = (eta+1)/(t+eta): averaging.jl:36-53."""

    def __init__(self, eta=8):
        self.eta = eta

    def init(self, ctx, params):
        return (params.clone(), 1)

    def apply(self, ctx, state, params):
        x_bar, t = state
        w = (self.eta + 1) / (t + self.eta)
        ctx.axpby(x_bar, w, params, 1.0 - w)
        return (x_bar, t + 1)

    def value(self, state):
        return state[0]


class KLMinRepGradDescent:
    """KLMinRepGradDescent(adtype; entropy, optimizer, n_samples, averager, operator): constructors.jl:44-79."""

    def __init__(self, adtype, entropy=None, optimizer=None, n_samples: int = 1, averager=None, operator=None,
                 subsampling=None):
        entropy = entropy if entropy is not None else O.ClosedFormEntropy()
        if not isinstance(entropy, (O.ClosedFormEntropy, O.StickingTheLandingEntropy, O.MonteCarloEntropy)):
            raise TypeError("entropy must be ClosedFormEntropy, StickingTheLandingEntropy or MonteCarloEntropy")
        self.objective = O.RepGradELBO(n_samples, entropy=entropy)
        if subsampling is not None:   # constructors.jl:69-73
            self.objective = S.SubsampledObjective(self.objective, subsampling)
        self.adtype = adtype
        self.optimizer = optimizer if optimizer is not None else DoWG()
        self.averager = averager if averager is not None else PolynomialAveraging()
        self.operator = operator if operator is not None else IdentityOperator()


ADVI = KLMinRepGradDescent


class KLMinRepGradProxDescent(KLMinRepGradDescent):
    """KLMinRepGradProxDescent(adtype; entropy_zerograd, optimizer, n_samples, averager): constructors.jl:122-157.
    The entropy is handled by the proximal operator, so the gradient estimator must ignore it: the entropy estimator is
    one of the two *ZeroGradient kinds; optimizer one of Descent / DoG / DoWG."""

    def __init__(self, adtype, entropy_zerograd=None, optimizer=None, n_samples: int = 1, averager=None, subsampling=None):
        entropy = entropy_zerograd if entropy_zerograd is not None else O.ClosedFormEntropyZeroGradient()
        if not isinstance(entropy, (O.ClosedFormEntropyZeroGradient, O.StickingTheLandingEntropyZeroGradient)):
            raise TypeError("entropy_zerograd must be ClosedFormEntropyZeroGradient or StickingTheLandingEntropyZeroGradient")
        optimizer = optimizer if optimizer is not None else DoWG()
        if not isinstance(optimizer, (Descent, DoG)):
            raise TypeError("optimizer must be Descent, DoG or DoWG")
        self.objective = O.RepGradELBO(n_samples, entropy=entropy)
        if subsampling is not None:   # constructors.jl:145-149
            self.objective = S.SubsampledObjective(self.objective, subsampling)
        self.adtype = adtype
        self.optimizer = optimizer
        self.averager = averager if averager is not None else PolynomialAveraging()
        self.operator = ProximalLocationScaleEntropy()


class KLMinScoreGradDescent:
    """KLMinScoreGradDescent(adtype; optimizer, n_samples, averager, operator): constructors.jl:199-233 -- stochastic gradient descent
    on the score-gradient ELBO (ScoreGradELBO), also known as black-box variational inference.  Needs only `logdensity` of the target."""

    def __init__(self, adtype, optimizer=None, n_samples: int = 1, averager=None, operator=None, **kwargs):
        if "subsampling" in kwargs:   # constructors.jl:222-226 composes with SubsampledObjective
            raise TypeError("KLMinScoreGradDescent(subsampling=...) is not implemented: ScoreGradELBO does not compose with "
                            "SubsampledObjective in this library")
        if kwargs:
            raise TypeError(f"KLMinScoreGradDescent() got an unexpected keyword argument {next(iter(kwargs))!r}")
        self.objective = O.ScoreGradELBO(n_samples)
        self.adtype = adtype
        self.optimizer = optimizer if optimizer is not None else DoWG()
        self.averager = averager if averager is not None else PolynomialAveraging()
        self.operator = operator if operator is not None else IdentityOperator()


BBVI = KLMinScoreGradDescent
PARAM_SPACE_SGD = (KLMinRepGradDescent, KLMinScoreGradDescent)   # the ParamSpaceSGD algorithms: what init / step / optimize accept


def _measure_space(*heads):
    """The measure_space module when one of `heads` is a measure-space algorithm (measure_space.ALGORITHMS: they have a loop of their
    own, no objective / optimiser / averager), else None."""
    from . import measure_space as M
    return M if any(isinstance(h, M.ALGORITHMS) for h in heads) else None


def _obj_init(rng, obj, *a):
    return (S.init if isinstance(obj, S.SubsampledObjective) else O.init)(rng, obj, *a)


def _obj_estimate_gradient(rng, obj, *a):
    return (S.estimate_gradient_ if isinstance(obj, S.SubsampledObjective) else O.estimate_gradient_)(rng, obj, *a)


def _ctx_of(obj_st):
    return obj_st.obj_st.obj_ad_prep if isinstance(obj_st, S.SubsampledObjectiveState) else obj_st.obj_ad_prep


def estimate_objective(rng, alg, q, prob=None, n_samples=None, entropy=None):
    """estimate_objective([rng,] alg, q, prob; n_samples, entropy=MonteCarloEntropy()): common.jl:29-38."""
    M = _measure_space(rng, alg)
    if M is not None:
        return M.estimate_objective(rng, alg, q, prob, n_samples=n_samples)
    if isinstance(rng, PARAM_SPACE_SGD):
        rng, alg, q, prob = O.default_rng(), rng, alg, q
    n = n_samples if n_samples is not None else alg.objective.n_samples
    if isinstance(alg.objective, O.ScoreGradELBO):   # scoregradelbo.jl:58-65 (its own estimator: no entropy choice)
        return O.estimate_objective(rng, alg.objective, q, prob, n_samples=n, adtype=alg.adtype)
    ent = entropy if entropy is not None else O.MonteCarloEntropy()
    if isinstance(alg.objective, S.SubsampledObjective):
        sub = S.SubsampledObjective(O.RepGradELBO(n, entropy=ent), alg.objective.subsampling)
        return S.estimate_objective(rng, sub, q, prob, adtype=alg.adtype)
    return O.estimate_objective(rng, O.RepGradELBO(n, entropy=ent), q, prob, adtype=alg.adtype)


def init(rng, alg, q_init, prob):
    """init(rng, alg::ParamSpaceSGD, q_init, prob): common.jl:40-61."""
    M = _measure_space(alg)
    if M is not None:
        return M.init(rng, alg, q_init, prob)
    if isinstance(q_init, MvLocationScaleLowRank) and isinstance(alg.operator, ProximalLocationScaleEntropy):
        raise TypeError(_NO_PROX_LOWRANK)
    if isinstance(q_init, COUPLING_FLOWS) and isinstance(alg.operator, (ClipScale, ProximalLocationScaleEntropy)):
        raise TypeError(_NO_SCALE_FLOW.format(type(alg.operator).__name__, FLOW_NAMES[q_init.family]))
    if isinstance(q_init, (MvLocationScale, MvLocationScaleLowRank)) and isinstance(alg.operator, IdentityOperator):
        warnings.warn(
            "IdentityOperator is used with a variational family <:MvLocationScale. Optimization can easily fail under "
            "this combination due to singular scale matrices. Consider using the operator `ClipScale` in the algorithm "
            "instead.")
    params_h, re = destructure(q_init)
    obj_st = _obj_init(rng, alg.objective, alg.adtype, q_init, prob, params_h, re)
    ctx = _ctx_of(obj_st)
    params = ctx.to_device(params_h).clone()
    opt_st = alg.optimizer.setup(ctx, params)
    avg_st = alg.averager.init(ctx, params)
    grad_buf = O.DiffResult(ctx.empty(1), ctx.empty(ctx.params_len))
    return dict(prob=prob, q=q_init, params=params, restructure=re, iteration=0, grad_buf=grad_buf, opt_st=opt_st,
                obj_st=obj_st, avg_st=avg_st)


def output(alg, state):
    """output(alg, state) = re(value(averager, avg_st)): common.jl:63-67."""
    M = _measure_space(alg)
    if M is not None:
        return M.output(alg, state)
    return state["restructure"](alg.averager.value(state["avg_st"]).cpu().numpy())


def step(rng, alg, state, callback, *objargs):
    """step(rng, alg::ParamSpaceSGD, state, callback): common.jl:69-120."""
    M = _measure_space(alg)
    if M is not None:
        return M.step(rng, alg, state, callback, *objargs)
    state = dict(state)
    state["iteration"] += 1
    t = state["iteration"]
    ctx = _ctx_of(state["obj_st"])
    params, re = state["params"], state["restructure"]
    grad_buf, obj_st, info = _obj_estimate_gradient(rng, alg.objective, alg.adtype, state["grad_buf"], state["obj_st"],
                                                  params, re, *objargs)
    state["obj_st"] = obj_st
    value = grad_buf.value()          # host sync, like the reference's eager isfinite check
    if not np.isfinite(value):        # common.jl:83-89
        raise RuntimeError(f"The objective value is {value}. This indicates that the optimization run diverged.")
    grad = grad_buf.gradient()
    state["opt_st"] = alg.optimizer.update(ctx, state["opt_st"], params, grad, t)   # Optimisers.update!
    params = alg.operator.apply(ctx, params, alg.optimizer, state["opt_st"])   # apply(operator, typeof(q), opt_st, params, re)
    state["avg_st"] = alg.averager.apply(ctx, state["avg_st"], params)
    state["params"] = params
    state["q"] = None  # materialised lazily by `output` / callbacks (params are device resident)
    if isinstance(alg.objective, O.ScoreGradELBO):   # its value is the VarGrad objective; the elbo is the objective's own statistic
        info = {**info, "elbo": float(info["elbo"])}
    else:
        info = {**{k: v for k, v in info.items() if k != "elbo"}, "elbo": -value}   # subsampling adds (epoch, step)
    if callback is not None:
        extra = callback(rng=rng, iteration=t, restructure=re, params=params,
                         averaged_params=alg.averager.value(state["avg_st"]), gradient=grad, state=state)
        if extra is not None:
            info = {**extra, **info}
    return state, False, info


_RULES = {Descent: 0, Adam: 1, DoG: 2, DoWG: 3, COCOB: 4}
_OPS = {IdentityOperator: 0, ClipScale: 1, ProximalLocationScaleEntropy: 2}
_AVGS = {NoAveraging: 0, PolynomialAveraging: 1}
DEVICE_LOOP_CHUNK = 256   # iterations per mivi_optimize_loop call (bounds the work done past a divergence)


SUBSAMPLED_KERNELS = 0    # tools / tests: the `kernels` of the chunk schedules (0 by size, 1 the fused minibatch kernel, 2 device gather)


def _scheduled_logreg(obj, prob):
    """A SubsampledObjective whose steps can run off a schedule of minibatches resident on the device (MiviContext.set_batch_schedule):
    a plain RepGradELBO inside, reshuffled batches, and the built-in logistic regression (also behind a TransformedProblem) as data."""
    from . import problems as P
    inner = prob.prob if isinstance(prob, P.TransformedProblem) else prob
    return (isinstance(obj, S.SubsampledObjective) and type(obj.objective) is O.RepGradELBO and
            isinstance(obj.subsampling, S.ReshufflingBatchSubsampling) and type(inner) is P.LogRegProblem)


def _device_loop_codes(alg, callback, objargs, prob=None):
    """(rule, op, averager) when a whole `step` can run inside mivi_optimize_loop, else None: no callback (it needs the
    parameters on the host every iteration), a plain RepGradELBO -- or a SubsampledObjective around one over the built-in
    logistic regression `prob` (mivi_optimize_loop_batches) -- and rule / operator / averager of the exact reference
    types (subclasses may override behaviour)."""
    if callback is not None or objargs or not (isinstance(alg.objective, O.RepGradELBO) or _scheduled_logreg(alg.objective, prob)):
        return None
    r, o, a = _RULES.get(type(alg.optimizer)), _OPS.get(type(alg.operator)), _AVGS.get(type(alg.averager))
    if r is None or o is None or a is None or (o == 2 and r in (1, 4)):
        return None
    return r, o, a


def _optimize_on_device(rng, alg, max_iter, state, codes, show_progress):
    """The loop of `optimize` with every iteration on the device (the same parameters as the host-driven loop: bitwise for Descent / Adam on the
    mean-field loops and the graph route, to rounding for the launch-free loops with their own summation order -- DoG / DoWG, the row-owning
    full-rank loops, the small logistic regression).
    Returns None when the target cannot be captured (host-callback targets): the caller then takes the host loop."""
    from ._lib import MiviError
    rule, op, avg = codes
    ctx = _ctx_of(state["obj_st"])
    params = state["params"]
    opt, info_total = alg.optimizer, []
    done = 0
    subsampled = isinstance(alg.objective, S.SubsampledObjective)   # (_device_loop_codes: the built-in logistic regression, batches off a resident schedule)
    import torch

    def _tensors(x):   # the device tensors inside an optimiser / averager state (tensor, tuple of tensors and scalars, None)
        if torch.is_tensor(x):
            return [x]
        if isinstance(x, (tuple, list)):
            return [t for e in x for t in _tensors(e)]
        return []

    while done < max_iter:
        n = min(DEVICE_LOOP_CHUNK, max_iter - done)
        elbo = ctx.empty(n)
        avg_params = state["avg_st"][0] if avg == 1 else None
        # what a divergence inside the chunk must not destroy: the reference throws AT the offending step, before
        # Optimisers.update! (common.jl:83-94), leaving every earlier step applied
        live = [params] + _tensors(state["opt_st"]) + _tensors(state["avg_st"])
        snap = [t.clone() for t in live]
        loop_args = dict(rule=rule, op=op, averager=avg,
                         eta=getattr(opt, "alpha", 0.0) if rule == 4 else getattr(opt, "eta", 0.0), beta=getattr(opt, "beta", (0.9, 0.999)),
                         adam_eps=getattr(opt, "epsilon", 1e-8), clip_epsilon=getattr(alg.operator, "epsilon", 0.0),
                         avg_eta=getattr(alg.averager, "eta", 8), opt_state=state["opt_st"], avg_params=avg_params, elbo=elbo)
        counter0, sub_infos = rng.counter, None   # (the shuffles and the estimates share the counter: a replay starts from it)
        try:
            if subsampled:
                # the chunk's steps planned ahead -- the batches and the estimate indices `estimate_gradient_` would have taken off `rng`
                # one step at a time -- and resident on the device: one upload per chunk, the batch of every step read through it
                sub_st0 = state["obj_st"].sub_st
                rows, est_idx, sub_infos, sub_st1 = S.plan_batches(rng, alg.objective.subsampling, sub_st0, n)
                ctx.set_batch_schedule(rows, est_idx, kernels=SUBSAMPLED_KERNELS)
                ctx.optimize_loop_batches(params, n, counter0, state["iteration"], first_batch=0, **loop_args)
                state["obj_st"] = S.SubsampledObjectiveState(state["obj_st"].prob, sub_st1, state["obj_st"].obj_st)
            else:
                ctx.optimize_loop(params, n, rng.counter, state["iteration"], **loop_args)
        except MiviError as e:
            if e.status == 6 and done == 0:      # MIVI_ERR_UNSUPPORTED: not a device-resident target
                rng.counter = counter0
                return None
            if e.status in (2, 3):               # common.jl:83-89 (a non-positive scale makes the objective NaN)
                # the chunk ran past the bad step: restore its entry state and replay it on the host-driven loop, which raises
                # at the offending iteration with the steps before it applied and rng / iteration advanced consistently
                # (a subsampled chunk: the counter and the subsampling state as well -- the replay shuffles and draws again, and
                # its row selections replace the schedule)
                rng.counter = counter0
                for t_live, t_snap in zip(live, snap):
                    t_live.copy_(t_snap)
                try:
                    ctx.synchronize()            # drop the sticky device flag of the failed chunk
                except MiviError:
                    pass
                try:
                    for k in range(n):
                        new_state, _, info = step(rng, alg, state, None)
                        state.update(new_state)
                        info_total.append({**info, "iteration": done + k + 1})   # (the loop index of THIS call: optimize.jl:64-68)
                except MiviError as e2:          # the host replay met the same device flag: the documented exception type
                    if e2.status in (2, 3):
                        raise RuntimeError("The objective value is not finite. This indicates that the optimization run "
                                           "diverged.") from e2
                    raise
                # the host-driven replay of the chunk completed with finite objectives: the device flag was not reproducible.
                # (mivi_optimize_loop clears every status word it later reads, so a stale flag of an earlier call cannot cause
                # this any more; if it happens, it is worth knowing.)  For Descent / Adam the replayed steps ARE the chunk (bitwise the
                # same arithmetic); for the launch-free loops that agree with the host loop to rounding only (DoG / DoWG's norm sums, the
                # row-owning full-rank loops, the small logistic regression) this chunk then comes from host arithmetic and the run carries
                # on from it -- a flag that does not reproduce is therefore warned about, never silently dropped.
                warnings.warn(f"device optimisation chunk reported status {e.status} ({e}) but its host-driven replay completed with "
                              "finite objectives; continuing from the replayed steps", RuntimeWarning)
                done += n
                continue
            raise
        if not subsampled:   # (the plan of a subsampled chunk has taken the indices already)
            for _ in range(n):
                rng.next_index()
        vals = elbo.cpu().numpy()
        # info = merge(info', (iteration = t,)) with t the loop index of THIS `optimize` call (src/optimize.jl:64-68) -- not the state's
        # cumulative counter, which a warm start carries on (common.jl:75): both routes report the same `info`; subsampling adds (epoch, step)
        info_total += [{**(sub_infos[i] if subsampled else {}), "elbo": float(vals[i]), "iteration": done + i + 1} for i in range(n)]
        state["iteration"] = state["iteration"] + n
        state["avg_st"] = (state["avg_st"][0], state["avg_st"][1] + n) if avg == 1 else params
        done += n
        if show_progress:
            print(f"\rOptimizing {done}/{max_iter} elbo={info_total[-1]['elbo']:.6g}", end="" if done < max_iter else "\n")
    state["q"] = None
    return info_total


def optimize(rng, algorithm, max_iter: int, prob=None, q_init=None, *objargs, show_progress=False, state=None,
             callback=None, device_loop=True):
    """optimize([rng,] algorithm, max_iter, prob, q_init; show_progress, state, callback): src/optimize.jl:42-94.
    Returns (output, info, state).  Without a callback and with a device-resident target every iteration runs inside
    mivi_optimize_loop (`device_loop=False` forces the host-driven `step` loop; both give the same result -- bitwise or to rounding, see
    _optimize_on_device).  With `subsampling=` over the built-in logistic regression the chunks run off a schedule of minibatches resident
    on the device (mivi_optimize_loop_batches; to rounding where the fused minibatch kernel runs, bitwise on the device gather); other
    subsampled models keep the host loop."""
    M = _measure_space(rng, algorithm)
    if M is not None:
        return M.optimize(rng, algorithm, max_iter, prob, q_init, *objargs, show_progress=show_progress, state=state, callback=callback,
                          device_loop=device_loop)
    if isinstance(rng, PARAM_SPACE_SGD):   # default-rng overload, optimize.jl:83-94
        extra = (q_init,) if q_init is not None else ()
        rng, algorithm, max_iter, prob, q_init = O.default_rng(), rng, algorithm, max_iter, prob
        objargs = extra + objargs
    info_total = []
    if state is None:
        state = init(rng, algorithm, q_init, prob)
    codes = _device_loop_codes(algorithm, callback, objargs, state.get("prob")) if device_loop else None
    if isinstance(algorithm.objective, S.SubsampledObjective) and _ctx_of(state["obj_st"]).family in FLOW_FAMILIES:
        codes = None   # the batch schedule has no form for a flow: subsampled steps keep the host loop (mivi_logreg_select_rows per step)
    if codes is not None and max_iter > 0:
        state = dict(state)
        info_dev = _optimize_on_device(rng, algorithm, max_iter, state, codes, show_progress)
        if info_dev is not None:
            return output(algorithm, state), info_dev, state
    for t in range(1, max_iter + 1):
        state, terminate, info = step(rng, algorithm, state, callback, *objargs)
        info = {**info, "iteration": t}
        if terminate:
            break
        if show_progress:
            print(f"\rOptimizing {t}/{max_iter} elbo={info['elbo']:.6g}", end="" if t < max_iter else "\n")
        info_total.append(info)
    return output(algorithm, state), info_total, state


# --- optimize_many: independent runs of one shape, one workgroup each -------------------------------
# the shapes mivi_optimize_loop_many serves (include/mivi.h): fr_small_loop_ok / lr_small_loop_ok of the library, restated for the host
_MANY_FR = dict(d=32, n_mc=64, dm=768, dm_stl=512)
_MANY_LR = dict(d=64, n_mc=64, pm=256, work=1 << 20)


def _many_family(q, state=None):
    """(family, d, dtype string) of a run, or None when the many-run entry cannot carry it: from `q` (an MvLocationScale with the normal
    base), or -- a warm start written as `optimize` allows, q_init = None with a state -- from the state's context (a base other than
    the normal one is then the library's to refuse)."""
    from .families import FULLRANK, MEANFIELD
    if q is None and state is not None:
        ctx = _ctx_of(state["obj_st"])
        fam, d, dt = ctx.family, ctx.d, np.dtype(ctx.np_dtype).str
    elif isinstance(q, MvLocationScale) and getattr(getattr(q, "dist", None), "code", 0) == 0:
        fam, d, dt = q.family, len(q), np.dtype(q.eltype).str
    else:
        return None
    return (fam, d, dt) if fam in (FULLRANK, MEANFIELD) else None


def _many_key(alg, prob, q, state=None):
    """What must agree between runs that share a launch, as a hashable key -- None for a run mivi_optimize_loop_many cannot carry.  Pure
    host arithmetic on types and shapes: no library call, no device.  The step size (eta, or alpha of DoG / DoWG) is not part of the key:
    it is what the runs of a sweep differ in."""
    from . import problems as P
    from .families import FULLRANK
    if type(alg) not in (KLMinRepGradDescent, KLMinRepGradProxDescent) or type(alg.objective) is not O.RepGradELBO:
        return None
    codes = _device_loop_codes(alg, None, ())
    fam = _many_family(q, state)
    if codes is None or codes[0] > 3 or fam is None:
        return None
    family, d, dtype_str = fam
    M, ent = alg.objective.n_samples, alg.objective.entropy
    stl = isinstance(ent, (O.StickingTheLandingEntropy, O.StickingTheLandingEntropyZeroGradient))
    if type(prob) is P.DiagNormalProblem:
        if family != FULLRANK or d > _MANY_FR["d"] or M > _MANY_FR["n_mc"] or d * M > (_MANY_FR["dm_stl"] if stl else _MANY_FR["dm"]):
            return None
        if P.dimension(prob) != d:
            return None
        shape = ("A", d)
    elif type(prob) is P.LogRegProblem:
        if not isinstance(prob.X, np.ndarray) or prob.X.ndim != 2 or P.dimension(prob) != d:
            return None
        n, p = prob.X.shape
        if stl or d < 2 or d > _MANY_LR["d"] or M > _MANY_LR["n_mc"] or p * M > _MANY_LR["pm"] or n * p * M > _MANY_LR["work"]:
            return None
        shape = ("B", n, p, prob.variant, prob.likeadj)
    else:
        return None
    opt = alg.optimizer
    return (type(alg), codes, type(ent), M, getattr(opt, "beta", None), getattr(opt, "epsilon", None),
            getattr(alg.operator, "epsilon", None), getattr(alg.averager, "eta", None), getattr(alg.adtype, "device", 0),
            family, dtype_str, shape)


def many_plan(algorithms, probs, q_inits, states=None):
    """The decision "these runs can share a launch" of optimize_many: the common key of the runs (see _many_key) when every run has one and
    all agree, else None -- the runs are then optimised one after the other.  `states`: the runs' states of a warm start (a run whose
    q_init is None is described by its state)."""
    states = [None] * len(algorithms) if states is None else states
    keys = [_many_key(a, p, q, s) for a, p, q, s in zip(algorithms, probs, q_inits, states)]
    if not keys or keys[0] is None or any(k != keys[0] for k in keys[1:]):
        return None
    return keys[0]


def _per_run(x, K, name):
    """`x` as a list of K: one value for every run, or a list / tuple of exactly K."""
    if isinstance(x, (list, tuple)):
        if len(x) != K:
            raise ValueError(f"optimize_many: {name} holds {len(x)} entries for {K} rngs")
        return list(x)
    return [x] * K


def _optimize_many_on_device(rngs, algs, max_iter, states, key, show_progress):
    """The chunks of optimize_many on mivi_optimize_loop_many.  Returns the runs' info lists, or None when the library does not take the
    group (nothing has been changed then)."""
    import torch
    from ._lib import MiviError
    K = len(rngs)
    rule, op, avg = key[1]
    cls = key[-1][0]
    ctx = _ctx_of(states[0]["obj_st"])
    ctxs = [_ctx_of(st["obj_st"]) for st in states]
    probs = [st["prob"] for st in states]
    infos = [[] for _ in range(K)]
    active = list(range(K))
    y_all = X_all = None
    x_stride = 0
    if cls == "B":
        n, p = probs[0].X.shape
        y_all = torch.as_tensor(np.ascontiguousarray(np.stack([np.asarray(pr.y).reshape(n) for pr in probs]), dtype=np.uint8)).to(ctx.tdevice)
        shared = all(pr.X is probs[0].X or np.array_equal(pr.X, probs[0].X) for pr in probs[1:])
        Xs = [probs[0].X] if shared else [pr.X for pr in probs]
        X_all = torch.as_tensor(np.stack([np.ascontiguousarray(np.asarray(X, dtype=ctx.np_dtype).T).reshape(-1) for X in Xs])).to(ctx.tdevice)
        x_stride = 0 if shared else n * p
    done = 0
    while done < max_iter and active:
        n_st = min(DEVICE_LOOP_CHUNK, max_iter - done)
        sts = [states[k] for k in active]
        Ka = len(active)
        params = torch.stack([st["params"] for st in sts]).contiguous()
        opt_state = torch.stack([st["opt_st"] for st in sts]).contiguous() if rule != 0 else None
        avg_params = torch.stack([st["avg_st"][0] for st in sts]).contiguous() if avg == 1 else None
        elbo = ctx.empty(Ka * n_st)
        t0s = {st["iteration"] for st in sts}
        if len(t0s) != 1:
            raise ValueError("optimize_many: the runs of one launch must have done the same number of iterations")
        opt0 = algs[active[0]].optimizer
        kw = dict(rule=rule, op=op, averager=avg, beta=getattr(opt0, "beta", (0.9, 0.999)), adam_eps=getattr(opt0, "epsilon", 1e-8),
                  clip_epsilon=getattr(algs[active[0]].operator, "epsilon", 0.0), avg_eta=getattr(algs[active[0]].averager, "eta", 8),
                  opt_state=opt_state, avg_params=avg_params, elbo=elbo)
        if cls == "A":
            d = ctx.d
            kw.update(means=np.stack([np.asarray(probs[k].mean, dtype=ctx.np_dtype) for k in active]),
                      stds=np.stack([np.broadcast_to(np.asarray(probs[k].std, dtype=ctx.np_dtype), (d,)) for k in active]))
        else:
            sel = torch.as_tensor(active, device=ctx.tdevice)
            kw.update(y=y_all.index_select(0, sel).contiguous(),
                      X=X_all if x_stride == 0 else X_all.index_select(0, sel).contiguous(), x_stride=x_stride)
        try:
            status = ctx.optimize_loop_many(params, Ka, n_st, [rngs[k].counter for k in active], sts[0]["iteration"],
                                            seeds=[ctxs[k].seed for k in active], etas=[getattr(algs[k].optimizer, "eta", 0.0) for k in active],
                                            **kw)
        except MiviError as e:
            if e.status == 6 and done == 0:   # MIVI_ERR_UNSUPPORTED: the library does not take this group
                return None
            raise
        vals = elbo.cpu().numpy().reshape(Ka, n_st)
        still = []
        # the finished runs' slices back into the runs' own tensors: one batched copy per kind, not one launch per run
        fine = [j for j in range(Ka) if status[j] == 0]
        dst, src = [states[active[j]]["params"] for j in fine], [params[j] for j in fine]
        if rule != 0:
            dst, src = dst + [states[active[j]]["opt_st"] for j in fine], src + [opt_state[j] for j in fine]
        if avg == 1:
            dst, src = dst + [states[active[j]]["avg_st"][0] for j in fine], src + [avg_params[j] for j in fine]
        if dst:
            torch._foreach_copy_(dst, src)
        iters = range(done + 1, done + n_st + 1)
        for j, k in enumerate(active):
            st, rng = states[k], rngs[k]
            if status[j] == 0:
                if avg == 1:
                    st["avg_st"] = (st["avg_st"][0], st["avg_st"][1] + n_st)
                rng.counter += n_st   # (n_st times next_index: one estimate index per step)
                infos[k] += [{"elbo": e, "iteration": i} for e, i in zip(vals[j].tolist(), iters)]
                st["iteration"] += n_st
                st["q"] = None
                still.append(k)
                continue
            # the run diverged inside the chunk: its tensors still hold the chunk's entry state (nothing was copied back), so the host-driven
            # loop replays it and stops where `optimize` would have raised, the steps before it applied (common.jl:83-94)
            try:
                for i in range(n_st):
                    new_state, _, info = step(rng, algs[k], st, None)
                    st.update(new_state)
                    infos[k].append({**info, "iteration": done + i + 1})
            except (RuntimeError, MiviError) as e:
                if isinstance(e, MiviError) and e.status not in (2, 3):
                    raise
                try:
                    ctxs[k].synchronize()   # drop the sticky device flag of the failed estimate
                except MiviError:
                    pass
                st["diverged"] = True
            else:
                warnings.warn(f"optimize_many: run {k} reported status {int(status[j])} on the device but its host-driven replay completed "
                              "with finite objectives; continuing from the replayed steps", RuntimeWarning)
                still.append(k)
        active = still
        done += n_st
        if show_progress:
            print(f"\rOptimizing {done}/{max_iter} ({len(active)} of {K} runs)", end="" if done < max_iter and active else "\n")
    return infos


def optimize_many(rngs, algorithm, max_iter: int, probs, q_inits, *, states=None, show_progress=False):
    """K independent `optimize` calls as one: element k of the returned list is what
    `optimize(rngs[k], algorithm_k, max_iter, probs[k], q_inits[k], state=states[k])` returns -- (output, info, state), with rngs[k]
    advanced alike.  `algorithm`, `probs` and `q_inits`: one value for every run or K of them; `states`: K states or None (with states,
    q_inits may be None as for `optimize`).  Bit for bit where `optimize` runs the problem in one workgroup too: every small full-rank run
    on a DiagNormalProblem, and the regressions that mivi_optimize_loop does not split over workgroups (n p n_samples <= 2^14); for a
    larger regression `optimize` splits the rows over several workgroups and a run here stays one, so the two agree to the rounding of
    the row sums (2e-4 relative in float32, 1e-9 in float64: tests/test_gpu_optimize_many.py).

    Runs of one shape whose whole loop fits a workgroup -- small full-rank families on a DiagNormalProblem, small LogRegProblems (see
    mivi_optimize_loop_many, include/mivi.h) -- with the same rule, operator, averager, estimator and sample count (step sizes may differ)
    share ONE launch per chunk of DEVICE_LOOP_CHUNK iterations, workgroup k = run k.  Every other configuration runs as K `optimize` calls.
    A run that diverges does not raise: its state carries `state["diverged"] = True`, its `info` ends at the last finite step and its
    parameters are those of that step, where `optimize` would have raised; the other runs are not affected."""
    rngs = list(rngs)
    K = len(rngs)
    if K < 1:
        raise ValueError("optimize_many: at least one rng (one run) is needed")
    if not all(isinstance(r, O.PhiloxRNG) for r in rngs):
        raise TypeError("optimize_many: rngs must be PhiloxRNGs, one per run")
    if len({id(r) for r in rngs}) != K:
        raise ValueError("optimize_many: every run needs a PhiloxRNG of its own (the same object was passed twice)")
    if not isinstance(max_iter, (int, np.integer)) or max_iter < 0:
        raise ValueError("optimize_many: max_iter must be a non-negative integer")
    algs = _per_run(algorithm, K, "algorithm")
    probs = _per_run(probs, K, "probs")
    qs = _per_run(q_inits, K, "q_inits")
    flow = next((q for q in qs if isinstance(q, COUPLING_FLOWS)), None)
    if flow is not None:
        raise TypeError(f"optimize_many has no method for a normalizing flow ({FLOW_NAMES[flow.family]}): its runs are small Gaussian families, one "
                        "workgroup each -- call `optimize` once per run")
    if states is None:
        states = [None] * K
    elif isinstance(states, dict) or len(states) != K or not all(isinstance(s, dict) for s in states):
        raise ValueError(f"optimize_many: states must be a list of {K} states, one per run (a state belongs to one run)")
    else:
        states = list(states)

    def sequential(sts):
        return [optimize(rngs[k], algs[k], max_iter, probs[k], qs[k], show_progress=show_progress, state=sts[k]) for k in range(K)]

    if _measure_space(*algs) is not None:
        return sequential(states)
    key = many_plan(algs, [s["prob"] if s is not None else p for s, p in zip(states, probs)], qs, states)
    if key is None or max_iter == 0:
        return sequential(states)
    sts = [dict(s) if s is not None else init(rngs[k], algs[k], qs[k], probs[k]) for k, s in enumerate(states)]
    if len({st["iteration"] for st in sts}) != 1 or len({id(st["params"]) for st in sts}) != K:
        return sequential(sts)
    infos = _optimize_many_on_device(rngs, algs, int(max_iter), sts, key, show_progress)
    if infos is None:
        return sequential(sts)
    return [(output(algs[k], sts[k]), infos[k], sts[k]) for k in range(K)]
