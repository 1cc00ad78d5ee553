"""Target log-density problems: the LogDensityProblems plugin seam of the hot path
(`logdensity`, `logdensity_and_gradient`, `dimension`, `capabilities`; call sites
src/algorithms/repgradelbo.jl:32,50,85 and src/mixedad_logdensity.jl:13-28).

Built-in problems are *descriptors*: their arithmetic lives in libmivi's fused HIP kernels.
Any other object exposing `dimension()` and `logdensity_and_gradient(z) -> (ell, grad)` is a
generic plugin and is evaluated through the host-callback route (batched over the columns of Z,
exactly the `logdensity_and_gradient` contract of src/mixedad_logdensity.jl:28)."""
from __future__ import annotations

import numpy as np


class LogDensityOrder:
    """LogDensityProblems.LogDensityOrder{K}."""

    def __init__(self, k: int):
        self.k = k

    def __lt__(self, other):
        return self.k < other.k

    def __repr__(self):
        return f"LogDensityOrder{{{self.k}}}()"


def dimension(prob) -> int:
    return int(prob.dimension())


def capabilities(prob) -> LogDensityOrder:
    if hasattr(prob, "capabilities"):
        return prob.capabilities()
    return LogDensityOrder(1 if hasattr(prob, "logdensity_and_gradient") else 0)


class ADgradient:
    """LogDensityProblemsAD.ADgradient(kind, prob) (README.md:168-174): an order-0 problem (only `logdensity`) wrapped so that it
    provides `logdensity_and_gradient`.  kind "forwarddiff" = forward-mode dual numbers over numpy (`forwarddiff.py`; BASELINE.json
    configs[0] names ForwardDiff on the CPU).  `logdensity` must be written with numpy ufuncs / the array functions listed there."""

    KINDS = ("forwarddiff",)

    def __init__(self, kind, prob, chunk: int = 64):
        if kind not in self.KINDS:
            raise ValueError(f"ADgradient: unknown backend {kind!r} (available: {self.KINDS})")
        if not hasattr(prob, "logdensity"):
            raise TypeError("ADgradient: the problem must implement logdensity")
        self.kind, self.prob, self.chunk = kind, prob, int(chunk)

    def dimension(self):
        return dimension(self.prob)

    def capabilities(self):
        return LogDensityOrder(1)

    def logdensity(self, x):
        return self.prob.logdensity(x)

    def logdensity_and_gradient(self, x):
        from . import forwarddiff
        return forwarddiff.value_and_gradient(self.prob.logdensity, np.asarray(x, dtype=np.float64), self.chunk)

    def subsample(self, batch):   # AdvancedVI.subsample forwards to the wrapped problem (src/AdvancedVI.jl:313)
        return ADgradient(self.kind, subsample(self.prob, batch), self.chunk)


class DiagNormalProblem:
    """MvNormal(mean, Diagonal(std.^2)) -- test/models/normal.jl:56-75, bench/benchmarks.jl:43-47."""

    def __init__(self, mean, std, order=1):
        self.mean = np.asarray(mean)
        self.std = np.asarray(std)
        self.order = int(order)   # 2: declares logdensity_gradient_and_hessian (constant Hessian -1 / std^2)

    def dimension(self):
        return self.mean.shape[0]

    def capabilities(self):
        return LogDensityOrder(self.order)


class DenseNormalProblem:
    """MvNormal(mean, L L') -- test/models/normal.jl:36-54 (`normal_fullrank`)."""

    def __init__(self, mean, L, order=1):
        self.mean = np.asarray(mean)
        self.L = np.tril(np.asarray(L))
        self.order = int(order)   # 2: declares logdensity_gradient_and_hessian (constant Hessian -(L L')^-1)

    def dimension(self):
        return self.mean.shape[0]

    def capabilities(self):
        return LogDensityOrder(self.order)


class _RowSubset:
    """A minibatch view of a data-set problem (what its `subsample` returns): the rows `batch` (0-based) of `parent`, with the likelihood
    scaled by n_data / n.  The data stay where the parent keeps them; the device reads the rows through mivi_<t>_select_rows."""

    def __init__(self, parent, batch):
        self.parent = parent
        self.batch = np.ascontiguousarray(np.asarray(batch, dtype=np.int64).reshape(-1))
        if self.batch.size == 0:
            raise ValueError("empty batch")
        self.likeadj = parent.likeadj * parent.n_rows() / self.batch.size

    def dimension(self):
        return self.parent.dimension()

    def capabilities(self):
        return self.parent.capabilities()

    def subsample(self, batch):
        return type(self)(self.parent, self.batch[np.asarray(batch, dtype=np.int64)])


class LogRegProblem:
    """Hierarchical logistic regression over theta = [beta; s].
    variant "logsigma_normal": docs/src/tutorials/subsampling.md:26-38
    variant "lognormal_exp_bijector": README.md:42-66 inside the TransformedLogDensityProblem of README.md:91-106.
    X is n x p (features), y in {0,1}; likeadj = n_data / n."""

    VARIANTS = {"logsigma_normal": 0, "lognormal_exp_bijector": 1}

    def __init__(self, X, y, variant="logsigma_normal", likeadj=1.0, order=1):
        self.X = np.asarray(X)
        self.y = np.asarray(y)
        if variant not in self.VARIANTS:
            raise ValueError(f"unknown variant {variant}")
        self.variant = variant
        self.likeadj = float(likeadj)
        self.order = int(order)   # 2: declares logdensity_gradient_and_hessian (the library averages the Hessians: csrc/kernels_hess2.hip)

    def dimension(self):
        return self.X.shape[1] + 1

    def capabilities(self):
        return LogDensityOrder(self.order)

    def n_rows(self):
        X = self.X
        return X.shape[1] if getattr(self, "x_is_colmajor_tensor", False) else X.shape[0]

    def subsample(self, batch):
        """AdvancedVI.subsample(prob, batch): the rows `batch` (0-based) with the likelihood scaled by n_data / n
        (docs/src/tutorials/subsampling.md:37,99-102).  The data stay on the device; see mivi_logreg_select_rows."""
        return LogRegSubset(self, batch)


class LogRegSubset(_RowSubset):
    """A minibatch view of a LogRegProblem (what `subsample` returns); never copies X on the host."""


class SoftmaxRegProblem:
    """Softmax (multinomial logistic) regression over theta = [vec B (p x n_classes, column-major); s], d = p n_classes + 1:
    B[k, c] ~ Normal(0, sigma^2), sigma = exp(s), y_r ~ Categorical(softmax(X[r] B)); the prior on sigma, the Jacobian term and
    likeadj are those of LogRegProblem's variants (mivi_set_target_softmax).  X is n x p, y in {0, ..., n_classes - 1}."""

    VARIANTS = LogRegProblem.VARIANTS
    MAX_CLASSES = 64

    def __init__(self, X, y, n_classes, variant="logsigma_normal", likeadj=1.0):
        # device-resident data: a contiguous (p, n) tensor -- n x p column-major, as the kernels read it -- and a uint8 tensor of labels
        self.on_device = hasattr(X, "data_ptr")
        self.X = X if self.on_device else np.asarray(X)
        self.y = y if self.on_device else np.asarray(y)
        self.p, self.n = (int(X.shape[0]), int(X.shape[1])) if self.on_device else (self.X.shape[1], self.X.shape[0])
        self.n_classes = int(n_classes)
        if variant not in self.VARIANTS:
            raise ValueError(f"unknown variant {variant}")
        self.variant = variant
        self.likeadj = float(likeadj)

    def dimension(self):
        return self.p * self.n_classes + 1

    def capabilities(self):
        return LogDensityOrder(1)

    def n_rows(self):
        return self.n

    def subsample(self, batch):
        """AdvancedVI.subsample(prob, batch): the rows `batch` (0-based) with the likelihood scaled by n_data / n.  The data stay on
        the device and the kernels read the rows through the index vector; see mivi_softmax_select_rows."""
        return SoftmaxRegSubset(self, batch)


class SoftmaxRegSubset(_RowSubset):
    """A minibatch view of a SoftmaxRegProblem (what `subsample` returns); never copies X."""


class BNNProblem:
    """A Bayesian neural network (mivi_set_target_bnn): the MLP p -> hidden_dims -> 1 with tanh hidden layers over
    theta = [vec W_1 (column-major, out x in); b_1; ...; vec W_{H+1}; b_{H+1}], theta_i ~ Normal(0, prior_std^2), and a Bernoulli (logit link,
    y in {0, 1}) or Normal(f, noise) likelihood scaled by likeadj.  X is n x p, y has n entries; one to three hidden layers of width <= 64.
    The multi-output head, p -> hidden_dims -> n_out with n_out <= 64: likelihood="categorical" with n_classes=C (a softmax link, y holds
    the class labels 0 .. C - 1), or likelihood="normal" with a two-dimensional y of shape (n, k), k >= 2 (independent Normal(f_c, noise))."""

    LIKELIHOODS = {"bernoulli": 0, "normal": 1, "categorical": 0}   # (the logit family is code 0 at every number of outputs)

    def __init__(self, X, y, hidden_dims, likelihood="bernoulli", noise=1.0, prior_std=1.0, likeadj=1.0, n_classes=None):
        # device-resident data: a contiguous (p, n) tensor -- n x p column-major, as the kernel reads it -- and a tensor of n labels, both of
        # the context's dtype; the responses of a multi-output Normal are then a contiguous (k, n) tensor, as X is (p, n)
        self.on_device = hasattr(X, "data_ptr")
        self.X = X if self.on_device else np.asarray(X)
        self.y = y if self.on_device else np.asarray(y)
        self.p, self.n = (int(X.shape[0]), int(X.shape[1])) if self.on_device else (self.X.shape[1], self.X.shape[0])
        self.hidden_dims = tuple(int(h) for h in hidden_dims)
        if likelihood not in self.LIKELIHOODS:
            raise ValueError(f"unknown likelihood {likelihood}")
        if (likelihood == "categorical") != (n_classes is not None) or (n_classes is not None and int(n_classes) < 2):
            raise ValueError('likelihood="categorical" takes n_classes >= 2, and no other likelihood takes n_classes')
        self.likelihood = likelihood
        self.n_out = 1
        if likelihood == "categorical":
            self.n_out = int(n_classes)
        elif likelihood == "normal" and len(self.y.shape) == 2:
            self.n_out = int(self.y.shape[0] if self.on_device else self.y.shape[1])
        self.noise, self.prior_std, self.likeadj = float(noise), float(prior_std), float(likeadj)

    def layers(self):
        """[(out, in)] of W_1 .. W_{H+1}"""
        widths = (self.p,) + self.hidden_dims + (self.n_out,)
        return [(widths[l + 1], widths[l]) for l in range(len(widths) - 1)]

    def dimension(self):
        return sum(o * (i + 1) for o, i in self.layers())

    def capabilities(self):
        return LogDensityOrder(1)

    def n_rows(self):
        return self.n

    def subsample(self, batch):
        """AdvancedVI.subsample(prob, batch): the rows `batch` (0-based) with the likelihood scaled by n_data / n.  The data stay on
        the device and the kernel reads the rows through the index vector; see mivi_bnn_select_rows."""
        return BNNSubset(self, batch)

    def unpack(self, theta):
        """theta (d,) -> [(W_l (out, in), b_l (out,))], views where theta is contiguous"""
        theta, out, off = np.asarray(theta), [], 0
        for o, i in self.layers():
            out.append((theta[off:off + o * i].reshape(o, i, order="F"), theta[off + o * i:off + o * (i + 1)]))
            off += o * (i + 1)
        return out

    def predict(self, theta, Xnew, ctx=None):
        """Posterior predictive f of the M networks in theta (d x M: the samples `MiviContext.sample` returns, or a (d, M) array) on the
        rows of Xnew (n_new x p): a device tensor (M, n_new) -- (M, n_new, n_out) of logits, or of the Normal's means, for a multi-output
        head -- by mivi_bnn_forward.  ctx: a context that has this problem set; without one a context of theta's precision is made for
        the call."""
        from . import context as K
        own = ctx is None
        if own:
            f64 = (theta.dtype == K._torch().float64) if hasattr(theta, "data_ptr") else (np.asarray(theta).dtype == np.float64)
            ctx = K.MiviContext(np.float64 if f64 else np.float32, K.MEANFIELD, self.dimension(), 1, 0, 0)
            ctx.set_problem(self)
        try:
            return ctx.bnn_forward(theta, Xnew)
        finally:
            if own:
                ctx.synchronize()
                ctx.close()


class BNNSubset(_RowSubset):
    """A minibatch view of a BNNProblem (what `subsample` returns); never copies X."""


class HierGLMProblem:
    """A hierarchical GLM with varying intercepts (mivi_set_target_hglm): theta = [beta (p); u (n_groups); s], eta_r = x_r . beta +
    u[groups[r]] + offset[r], beta_k ~ Normal(0, prior_std^2), u_g ~ Normal(0, tau^2), tau = exp(s) ~ HalfNormal(tau_scale), and a Bernoulli
    (logit link, y in {0, 1}) or Poisson (log link, y in {0, 1, 2, ...}) likelihood scaled by likeadj.  X is n x p (p <= 256), y and the
    optional offset have n entries, groups holds n ids in {0, ..., n_groups - 1} in any order; a group may have no rows."""

    LIKELIHOODS = {"bernoulli": 0, "poisson": 1}

    def __init__(self, X, y, groups, n_groups, likelihood="bernoulli", offset=None, prior_std=1.0, tau_scale=1.0, likeadj=1.0):
        # device-resident data: a contiguous (p, n) tensor -- n x p column-major, as the kernel reads it -- and tensors of n responses and
        # offsets, all of the context's dtype.  The group ids are host data in either case: the row order is built on the host
        self.on_device = hasattr(X, "data_ptr")
        self.X = X if self.on_device else np.asarray(X)
        self.y = y if self.on_device else np.asarray(y)
        self.offset = offset if offset is None or self.on_device else np.asarray(offset)
        self.groups = np.asarray(groups.cpu() if hasattr(groups, "data_ptr") else groups).reshape(-1)
        self.p, self.n = (int(X.shape[0]), int(X.shape[1])) if self.on_device else (self.X.shape[1], self.X.shape[0])
        if self.groups.size != self.n:
            raise ValueError("HierGLMProblem: one group id per row")
        self.n_groups = int(n_groups)
        if likelihood not in self.LIKELIHOODS:
            raise ValueError(f"unknown likelihood {likelihood}")
        self.likelihood = likelihood
        self.prior_std, self.tau_scale, self.likeadj = float(prior_std), float(tau_scale), float(likeadj)

    def dimension(self):
        return self.p + self.n_groups + 1

    def capabilities(self):
        return LogDensityOrder(1)

    def n_rows(self):
        return self.n

    def subsample(self, batch):
        """AdvancedVI.subsample(prob, batch): the rows `batch` (0-based) with the likelihood scaled by n_data / n.  The data stay on
        the device; the selection is put into group order and the kernel reads the rows through it; see mivi_hglm_select_rows."""
        return HierGLMSubset(self, batch)

    def unpack(self, theta):
        """theta (d,) -> (beta (p,), u (n_groups,), s), views where theta is contiguous"""
        theta = np.asarray(theta)
        return theta[:self.p], theta[self.p:self.p + self.n_groups], theta[self.p + self.n_groups]


class HierGLMSubset(_RowSubset):
    """A minibatch view of a HierGLMProblem (what `subsample` returns); never copies X."""


class PPCAProblem:
    """Probabilistic PCA / a Bayesian factor model (mivi_set_target_ppca): y_rj ~ Normal(mu_j + W_j. . z_r, sigma^2) on the observed entries
    of Y (n x D, D <= 512; `mask` n x D of 0 / 1, None: all observed), z_r ~ Normal(0, I_k) for every row (k <= 32), mu_j ~ Normal(0,
    mean_std^2), sigma = exp(s) ~ HalfNormal(noise_scale) and W_jc ~ Normal(0, prior_std^2) or, with ard, W_jc ~ Normal(0, exp(2 a_c)),
    exp(a_c) ~ HalfNormal(prior_std).  theta = [vec W (D x k, column-major); Z (k x n, z_r contiguous); mu (D); a (k, with ard); s]: every
    row owns k coordinates, which start on a multiple of k -- BlockDiagGaussian blocks of k give each z_r a full covariance.  likeadj scales
    the rows' terms, each row's z_r prior included."""

    def __init__(self, Y, k, mask=None, ard=False, prior_std=1.0, mean_std=10.0, noise_scale=1.0, likeadj=1.0):
        # device-resident data: a contiguous (D, n) tensor of the context's dtype -- n x D column-major, as the kernel reads it -- and a
        # uint8 mask tensor of the same shape
        self.on_device = hasattr(Y, "data_ptr")
        self.Y = Y if self.on_device else np.asarray(Y)
        self.mask = mask if mask is None or self.on_device else np.asarray(mask)
        self.D, self.n = (int(Y.shape[0]), int(Y.shape[1])) if self.on_device else (self.Y.shape[1], self.Y.shape[0])
        if self.mask is not None and tuple(self.mask.shape) != tuple(self.Y.shape):
            raise ValueError("PPCAProblem: the mask has the shape of Y")
        self.k, self.ard = int(k), bool(ard)
        self.prior_std, self.mean_std, self.noise_scale, self.likeadj = float(prior_std), float(mean_std), float(noise_scale), float(likeadj)

    def dimension(self):
        return self.D * self.k + self.n * self.k + self.D + (self.k if self.ard else 0) + 1

    def capabilities(self):
        return LogDensityOrder(1)

    def n_rows(self):
        return self.n

    def subsample(self, batch):
        """AdvancedVI.subsample(prob, batch): the rows `batch` (0-based, no repeats) with their terms -- likelihood and z_r prior -- scaled
        by n_data / n.  The data stay on the device; the kernel reads the rows through the index vector; see mivi_ppca_select_rows."""
        return PPCASubset(self, batch)

    def unpack(self, theta):
        """theta (d,) -> (W (D, k), Z (n, k), mu (D,), a (k,) or None, s), views where theta is contiguous"""
        theta = np.asarray(theta)
        D, k, n = self.D, self.k, self.n
        oz, om = D * k, D * k + n * k
        return (theta[:oz].reshape(k, D).T, theta[oz:om].reshape(n, k), theta[om:om + D], theta[om + D:om + D + k] if self.ard else None,
                theta[-1])


class PPCASubset(_RowSubset):
    """A minibatch view of a PPCAProblem (what `subsample` returns); never copies Y."""


def subsample(model, batch):
    """AdvancedVI.subsample(model, batch): models that do not specialise it are returned unchanged
    (src/AdvancedVI.jl:313; the tutorial's warning at docs/src/tutorials/subsampling.md:106-110)."""
    fn = getattr(model, "subsample", None)
    return fn(batch) if fn is not None else model


class FunnelProblem:
    """Neal's funnel on the constrained scale under Stacked([log-bijector, identity]) (SURVEY.md 8d;
    wrapper pattern of README.md:76-82,102-106)."""

    def __init__(self, d, sigma_v=1.5, order=1):
        self.d = int(d)
        self.sigma_v = float(sigma_v)
        self.order = int(order)   # 2: declares logdensity_gradient_and_hessian (an arrow matrix: csrc/kernels_hess2.hip)

    def dimension(self):
        return self.d

    def capabilities(self):
        return LogDensityOrder(self.order)




class FunnelConstrainedProblem:
    """Neal's funnel on the constrained scale theta = [s; x] (s > 0), WITHOUT a bijector (mivi_set_target_funnel_constrained);
    TransformedProblem(FunnelConstrainedProblem(d, sv), StackedBijector([(0, 1, "exp"), (1, d, "identity")])) is FunnelProblem."""

    def __init__(self, d, sigma_v=1.5, order=1):
        self.d = int(d)
        self.sigma_v = float(sigma_v)
        self.order = int(order)   # 2: declares logdensity_gradient_and_hessian (an arrow matrix: csrc/kernels_hess2.hip)

    def dimension(self):
        return self.d

    def capabilities(self):
        return LogDensityOrder(self.order)


class StackedBijector:
    """inverse(Bijectors.Stacked(bijectors, ranges)) restricted to identity / exp blocks (README.md:76-82):
    blocks = [(begin, end, kind)], 0-based half-open ranges, kind in {"identity", "exp"}.
    Bounded and ordered supports (mivi_set_bijector_stacked_ex): (begin, end, "truncated", (lb, ub)) -- one pair of bounds per block, either
    of which may be infinite (both finite: the scaled logistic map; one: a shifted exp; none: identity) -- and (begin, end, "ordered"), a
    strictly increasing block x_b = eta_b, x_k = x_{k-1} + exp(eta_k).  `.blocks` stays a list of 3-tuples; `.bounds` is the parallel list
    of (lb, ub) pairs ((-inf, +inf) for a block that is not truncated)."""

    KINDS = {"identity": 0, "exp": 1, "truncated": 2, "ordered": 3}
    LEGACY_KINDS = ("identity", "exp")   # what mivi_set_bijector_stacked itself takes

    def __init__(self, blocks):
        self.blocks, self.bounds = [], []
        for blk in blocks:
            blk = tuple(blk)
            if len(blk) not in (3, 4):
                raise ValueError(f"a bijector block is (begin, end, kind) or (begin, end, 'truncated', (lb, ub)), got {blk!r}")
            lo, hi, kind = int(blk[0]), int(blk[1]), str(blk[2])
            if kind not in self.KINDS:
                raise ValueError(f"unknown bijector kind {kind}")
            if (len(blk) == 4) != (kind == "truncated"):
                raise ValueError(f"bounds go with a 'truncated' block and only with one, got {blk!r}")
            lb, ub = -np.inf, np.inf
            if kind == "truncated":
                try:
                    lb, ub = (float(v) for v in blk[3])
                except (TypeError, ValueError):
                    raise ValueError(f"the bounds of a truncated block are a pair (lb, ub), got {blk[3]!r}") from None
                if np.isnan(lb) or np.isnan(ub):
                    raise ValueError("a bound of a truncated block is NaN")
                if not lb < ub:
                    raise ValueError(f"a truncated block needs lb < ub, got ({lb}, {ub})")
            self.blocks.append((lo, hi, kind))
            self.bounds.append((lb, ub))

    @property
    def is_legacy(self):
        """identity / exp blocks only: what mivi_set_bijector_stacked takes"""
        return all(kind in self.LEGACY_KINDS for _, _, kind in self.blocks)


class TransformedProblem:
    """TransformedLogDensityProblem(prob, binv) of README.md:91-119: logdensity(eta) = logdensity(prob, binv(eta)) +
    logabsdetjac(binv, eta).  `prob` is any problem the context accepts (built-in descriptor or LogDensityProblems plugin)."""

    def __init__(self, prob, bijector: StackedBijector):
        self.prob = prob
        self.bijector = bijector

    def dimension(self):
        return self.prob.dimension()

    def capabilities(self):
        return self.prob.capabilities()

    def subsample(self, batch):   # AdvancedVI.subsample forwards to the wrapped problem, as ADgradient's does
        return TransformedProblem(subsample(self.prob, batch), self.bijector)


BUILTIN = (DiagNormalProblem, DenseNormalProblem, LogRegProblem, LogRegSubset, FunnelProblem, FunnelConstrainedProblem, SoftmaxRegProblem,
           SoftmaxRegSubset, BNNProblem, BNNSubset, HierGLMProblem, HierGLMSubset, PPCAProblem, PPCASubset)
