"""Variational family containers mirroring src/families/location_scale.jl and location_scale_low_rank.jl (AdvancedVI.jl v0.7.0).

Only what the RepGradELBO hot path needs: the `MvLocationScale` container with its base distribution
(`Normal()`, `Laplace()`, `TDist(nu)`), the two Gaussian constructors, and `destructure` / restructure.  All arithmetic on samples (rand, entropy, logpdf
inside the estimators) runs in libmivi's HIP kernels."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

MEANFIELD, FULLRANK, LOWRANK, REALNVP, NSF = 0, 1, 2, 3, 4
FLOW_FAMILIES = (REALNVP, NSF)   # the coupling flows: one surface, one set of refusals
FLOW_NAMES = {REALNVP: "RealNVP", NSF: "NeuralSplineFlow"}
LOWRANK_MAX_RANK = 64   # MIVI_LOWRANK_MAX_RANK (include/mivi.h)
FLOW_MAX_D, FLOW_MAX_HIDDEN, FLOW_MAX_LAYERS = 128, 64, 32   # MIVI_FLOW_MAX_* (include/mivi.h)


# --- univariate base distributions of MvLocationScale (docs/src/families.md:59-101): mivi_base_t codes, host statistics ---------------
def _digamma(x: float) -> float:
    """digamma(x), x > 0: the recurrence up to x >= 10, then the asymptotic series."""
    r = 0.0
    while x < 10.0:
        r -= 1.0 / x
        x += 1.0
    i2 = 1.0 / (x * x)
    ser = i2 * (1 / 12 - i2 * (1 / 120 - i2 * (1 / 252 - i2 * (1 / 240 - i2 * (1 / 132 - i2 * (691 / 32760 - i2 / 12))))))
    return r + math.log(x) - 0.5 / x - ser


class Normal:
    """Normal(): the standard normal base (MIVI_BASE_NORMAL), the default of every family."""
    code, nu = 0, 0.0

    def entropy(self):
        return 0.5 * (1.0 + math.log(2.0 * math.pi))

    def mean(self):
        return 0.0

    def var(self):
        return 1.0

    def __eq__(self, other):
        return type(other) is type(self) and other.nu == self.nu

    def __hash__(self):
        return hash((type(self).__name__, self.nu))

    def __repr__(self):
        return f"{type(self).__name__}()"


class Laplace(Normal):
    """Laplace(): location 0, scale 1 (MIVI_BASE_LAPLACE; families.md:88-101)."""
    code = 1

    def entropy(self):
        return 1.0 + math.log(2.0)

    def var(self):
        return 2.0


class TDist(Normal):
    """TDist(nu): Student-t with nu > 0 degrees of freedom (MIVI_BASE_TDIST; families.md:72-86)."""
    code = 2

    def __init__(self, nu):
        nu = float(nu)
        if not (nu > 0.0 and math.isfinite(nu)):
            raise ValueError("TDist: the degrees of freedom nu must be positive and finite")
        self.nu = nu

    def entropy(self):
        nu = self.nu
        a, b = 0.5 * (nu + 1.0), 0.5 * nu
        lbeta = math.lgamma(b) + math.lgamma(0.5) - math.lgamma(a)
        return a * (_digamma(a) - _digamma(b)) + 0.5 * math.log(nu) + lbeta

    def mean(self):   # as Distributions.jl: NaN for nu <= 1
        return 0.0 if self.nu > 1.0 else math.nan

    def var(self):    # as Distributions.jl: nu / (nu - 2), Inf for 1 < nu <= 2, NaN below
        if self.nu > 2.0:
            return self.nu / (self.nu - 2.0)
        return math.inf if self.nu > 1.0 else math.nan

    def __repr__(self):
        return f"TDist({self.nu})"


@dataclass
class MvLocationScale:
    """MvLocationScale(location, scale, dist), dist = Normal() unless given (src/families/location_scale.jl:15-19): z = scale u + location
    with the entries of u i.i.d. from `dist` -- Normal(), Laplace() or TDist(nu).  `scale` is a length-d vector (Diagonal) or a d x d
    lower-triangular matrix (LowerTriangular).  Arrays are numpy (host) float32/float64."""

    location: np.ndarray
    scale: np.ndarray
    dist: Normal = field(default_factory=Normal)

    def __post_init__(self):
        if not isinstance(self.dist, Normal):
            raise TypeError("MvLocationScale: dist must be Normal(), Laplace() or TDist(nu)")
        self.location = np.ascontiguousarray(self.location)
        self.scale = np.asarray(self.scale, dtype=self.location.dtype)
        if self.location.dtype not in (np.float32, np.float64):
            raise TypeError("MvLocationScale: eltype must be Float32 or Float64")
        d = self.location.shape[0]
        if self.scale.shape not in ((d,), (d, d)):
            raise ValueError("scale must be a length-d diagonal or a d x d lower-triangular matrix")

    @property
    def family(self) -> int:
        return MEANFIELD if self.scale.ndim == 1 else FULLRANK

    def __len__(self):  # Base.length(q), location_scale.jl:45
        return self.location.shape[0]

    @property
    def eltype(self):  # Base.eltype, location_scale.jl:49
        return self.location.dtype

    # host statistics (numpy): location_scale.jl:52-57, 98-113
    def _dense_scale(self):
        return np.diag(self.scale) if self.scale.ndim == 1 else self.scale

    def entropy(self):
        diag = self.scale if self.scale.ndim == 1 else np.diagonal(self.scale)
        return self.eltype.type(len(self) * self.eltype.type(self.dist.entropy()) + np.log(diag).sum())   # d H(dist) + logdet(scale)

    def mean(self):
        return self.location + self._dense_scale() @ np.full(len(self), self.dist.mean(), dtype=self.eltype)

    def var(self):
        C = self._dense_scale()
        return self.dist.var() * np.diagonal(C @ C.T)

    def cov(self):
        C = self._dense_scale()
        return self.dist.var() * (C @ C.T)


def MeanFieldGaussian(mu, diag) -> MvLocationScale:
    """MeanFieldGaussian(mu, L::Diagonal): src/families/location_scale.jl:139-141."""
    mu = np.asarray(mu)
    diag = np.asarray(diag)
    if diag.ndim != 1:
        raise TypeError("MeanFieldGaussian expects the diagonal of the scale (Diagonal matrix)")
    return MvLocationScale(mu, diag)


def FullRankGaussian(mu, L) -> MvLocationScale:
    """FullRankGaussian(mu, L::AbstractTriangular): src/families/location_scale.jl:124-128."""
    mu = np.asarray(mu)
    L = np.asarray(L)
    if L.ndim != 2:
        raise TypeError("FullRankGaussian expects a lower-triangular Cholesky factor")
    return MvLocationScale(mu, np.tril(L))


class MvLocationScaleLowRank:
    """MvLocationScaleLowRank(location, scale_diag, scale_factors, dist) with dist = Normal(0, 1)
    (src/families/location_scale_low_rank.jl:22-41): z = scale_diag .* u1 + scale_factors * u2 + location with u1 (d) and u2 (r)
    standard normal, i.e. the covariance scale_diag^2 + scale_factors scale_factors'.  Arrays are numpy (host) float32/float64."""

    def __init__(self, location, scale_diag, scale_factors):
        self.location = np.ascontiguousarray(location)
        if self.location.dtype not in (np.float32, np.float64):
            raise TypeError("MvLocationScaleLowRank: eltype must be Float32 or Float64")
        dt = self.location.dtype
        self.scale_diag = np.ascontiguousarray(scale_diag, dtype=dt)
        self.scale_factors = np.asarray(scale_factors, dtype=dt)
        d = self.location.shape[0]
        if self.location.ndim != 1 or self.scale_diag.shape != (d,) or self.scale_factors.ndim != 2 or self.scale_factors.shape[0] != d:
            raise ValueError("location and scale_diag must be length-d vectors and scale_factors a d x r matrix")
        if not 1 <= self.scale_factors.shape[1] <= LOWRANK_MAX_RANK:
            raise ValueError(f"the rank of scale_factors must be in 1 .. {LOWRANK_MAX_RANK}")

    family = LOWRANK

    @property
    def rank(self) -> int:
        return self.scale_factors.shape[1]

    def __len__(self):  # Base.length(q), location_scale_low_rank.jl:43
        return self.location.shape[0]

    @property
    def eltype(self):  # Base.eltype, location_scale_low_rank.jl:45
        return self.location.dtype

    # host statistics with the base distribution Normal(0, 1): location_scale_low_rank.jl:102-121
    def entropy(self):   # location_scale_low_rank.jl:35-43: d H(Normal) + (2 sum log D + logdet(I + U' D^-2 U)) / 2
        D, U = self.scale_diag, self.scale_factors
        UtDinvU = U.T @ (U / (D * D)[:, None])
        logdet_sigma = 2.0 * np.log(D).sum() + np.linalg.slogdet(np.eye(self.rank, dtype=self.eltype) + UtDinvU)[1]
        return self.eltype.type(len(self) * self.eltype.type(Normal().entropy()) + logdet_sigma / 2.0)

    def mean(self):
        return self.location.copy()   # mean(dist) = 0: the scale terms of :105-107 vanish

    def var(self):
        return self.scale_diag ** 2 + (self.scale_factors ** 2).sum(axis=1)   # var(dist) = 1

    def cov(self):
        return np.diag(self.scale_diag ** 2) + self.scale_factors @ self.scale_factors.T


def LowRankGaussian(mu, D, U) -> MvLocationScaleLowRank:
    """LowRankGaussian(mu, D, U): src/families/location_scale_low_rank.jl:140-145."""
    return MvLocationScaleLowRank(np.asarray(mu), np.asarray(D), np.asarray(U))


def flow_layout(d: int, hidden_dims, n_layers: int):
    """The parameter vector of a RealNVP flow (MIVI_REALNVP, include/mivi.h), block by block: a list of
    (layer l = 1 .. L, net "s" | "t", j = 1 .. H + 1, "W" | "b", offset, shape).  For l = 1 .. L the s net, then the t net; a net is
    [vec W_1 (column-major, out x in); b_1; ...; vec W_{H+1}; b_{H+1}] from |B_l| inputs to |A_l| outputs, A_l the even coordinates
    (0-based) for odd l and the odd ones for even l."""
    blocks, off = [], 0
    for l in range(1, n_layers + 1):
        n_a = (d + 1) // 2 if l % 2 == 1 else d // 2
        widths = [d - n_a, *hidden_dims, n_a]
        for net in ("s", "t"):
            for j in range(1, len(widths)):
                out, inn = widths[j], widths[j - 1]
                blocks.append((l, net, j, "W", off, (out, inn)))
                off += out * inn
                blocks.append((l, net, j, "b", off, (out,)))
                off += out
    return blocks, off


class RealNVPFlow:
    """The RealNVP normalizing flow of docs/src/tutorials/flows.md on a standard-normal base (`@leaf MvNormal`: the base has no
    parameters): L affine coupling layers x[A] <- x[A] .* exp(s(x[B])) + t(x[B]) with alternating masks, s and t fully connected nets
    with leakyrelu hidden layers (tanh on s's output).  `params` is the flat vector of `flow_layout`.  Arrays are numpy float32/float64."""

    family = REALNVP

    def __init__(self, d, hidden_dims, n_layers, params):
        self.d, self.hidden_dims, self.n_layers = int(d), tuple(int(h) for h in hidden_dims), int(n_layers)
        if not 2 <= self.d <= FLOW_MAX_D:
            raise ValueError(f"RealNVP: the dimension must be in 2 .. {FLOW_MAX_D}")
        if not 1 <= len(self.hidden_dims) <= 3 or not all(1 <= h <= FLOW_MAX_HIDDEN for h in self.hidden_dims):
            raise ValueError(f"RealNVP: one to three hidden layers of width 1 .. {FLOW_MAX_HIDDEN}")
        if not 1 <= self.n_layers <= FLOW_MAX_LAYERS:
            raise ValueError(f"RealNVP: n_layers must be in 1 .. {FLOW_MAX_LAYERS}")
        self.params = np.ascontiguousarray(params)
        if self.params.dtype not in (np.float32, np.float64):
            raise TypeError("RealNVP: eltype must be Float32 or Float64")
        if self.params.shape != (flow_layout(self.d, self.hidden_dims, self.n_layers)[1],):
            raise ValueError("flat parameter vector has the wrong length")

    def __len__(self):
        return self.d

    @property
    def eltype(self):
        return self.params.dtype

    def blocks(self):
        """{(l, net, j, "W" | "b"): array view} of the parameter vector (W as an out x in matrix)."""
        return {(l, net, j, k): self.params[off:off + int(np.prod(shape))].reshape(shape, order="F")
                for l, net, j, k, off, shape in flow_layout(self.d, self.hidden_dims, self.n_layers)[0]}


def RealNVP(d, hidden_dims, n_layers, eltype=np.float64, rng=None) -> RealNVPFlow:
    """realnvp(MvNormal(zeros(d), I), hidden_dims, n_layers) of docs/src/tutorials/flows.md:199-207: Glorot-uniform weights from a seeded
    numpy generator (an int seed or a Generator; None: seed 0), zero biases."""
    gen = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(0 if rng is None else rng)
    blocks, n = flow_layout(int(d), tuple(hidden_dims), int(n_layers))
    flat = np.zeros(n, dtype=np.float64)
    for _, _, _, kind, off, shape in blocks:
        if kind == "W":
            lim = math.sqrt(6.0 / (shape[0] + shape[1]))
            flat[off:off + shape[0] * shape[1]] = gen.uniform(-lim, lim, size=shape[0] * shape[1])
    return RealNVPFlow(d, hidden_dims, n_layers, flat.astype(eltype))


NSF_MAX_BINS = 16   # MIVI_NSF_MAX_BINS (include/mivi.h)


def nsf_layout(d: int, hidden_dims, n_layers: int, n_bins: int):
    """The parameter vector of a neural spline flow (MIVI_NSF, include/mivi.h), block by block: a list of
    (layer l = 1 .. L, j = 1 .. H + 1, "W" | "b", offset, shape).  ONE net per layer, [vec W_1 (column-major, out x in); b_1; ...;
    vec W_{H+1}; b_{H+1}] from |B_l| inputs to |A_l| (3K - 1) outputs: coordinate i of A_l owns the output rows i (3K - 1) ...,
    in the order u^w_1..K, u^h_1..K, u^d_1..K-1."""
    blocks, off = [], 0
    for l in range(1, n_layers + 1):
        n_a = (d + 1) // 2 if l % 2 == 1 else d // 2
        widths = [d - n_a, *hidden_dims, n_a * (3 * n_bins - 1)]
        for j in range(1, len(widths)):
            out, inn = widths[j], widths[j - 1]
            blocks.append((l, j, "W", off, (out, inn)))
            off += out * inn
            blocks.append((l, j, "b", off, (out,)))
            off += out
    return blocks, off


class SplineFlow:
    """The neural spline flow (Durkan et al., 2019; `nsf` of NormalizingFlows.jl) on a standard-normal base: RealNVP's masks and layer
    order, the affine map of each coupling layer replaced by a monotone rational-quadratic spline with `n_bins` bins on [-bound, bound]
    (the identity outside), whose widths, heights and slopes one net per layer gives.  `params` is the flat vector of `nsf_layout`."""

    family = NSF

    def __init__(self, d, hidden_dims, n_layers, n_bins, bound, params):
        self.d, self.hidden_dims, self.n_layers = int(d), tuple(int(h) for h in hidden_dims), int(n_layers)
        self.n_bins, self.bound = int(n_bins), float(bound)
        if not 2 <= self.d <= FLOW_MAX_D:
            raise ValueError(f"NeuralSplineFlow: the dimension must be in 2 .. {FLOW_MAX_D}")
        if not 1 <= len(self.hidden_dims) <= 3 or not all(1 <= h <= FLOW_MAX_HIDDEN for h in self.hidden_dims):
            raise ValueError(f"NeuralSplineFlow: one to three hidden layers of width 1 .. {FLOW_MAX_HIDDEN}")
        if not 1 <= self.n_layers <= FLOW_MAX_LAYERS:
            raise ValueError(f"NeuralSplineFlow: n_layers must be in 1 .. {FLOW_MAX_LAYERS}")
        if not 2 <= self.n_bins <= NSF_MAX_BINS:
            raise ValueError(f"NeuralSplineFlow: n_bins must be in 2 .. {NSF_MAX_BINS}")
        if not (self.bound > 0 and math.isfinite(self.bound)):
            raise ValueError("NeuralSplineFlow: bound must be positive and finite")
        self.params = np.ascontiguousarray(params)
        if self.params.dtype not in (np.float32, np.float64):
            raise TypeError("NeuralSplineFlow: eltype must be Float32 or Float64")
        if self.params.shape != (nsf_layout(self.d, self.hidden_dims, self.n_layers, self.n_bins)[1],):
            raise ValueError("flat parameter vector has the wrong length")

    def __len__(self):
        return self.d

    @property
    def eltype(self):
        return self.params.dtype

    def blocks(self):
        """{(l, j, "W" | "b"): array view} of the parameter vector (W as an out x in matrix)."""
        return {(l, j, k): self.params[off:off + int(np.prod(shape))].reshape(shape, order="F")
                for l, j, k, off, shape in nsf_layout(self.d, self.hidden_dims, self.n_layers, self.n_bins)[0]}


def NeuralSplineFlow(d, hidden_dims, n_bins, bound, n_layers, eltype=np.float64, rng=None) -> SplineFlow:
    """nsf(MvNormal(zeros(d), I); hidden_dims, K = n_bins, B = bound, n_layers): Glorot-uniform weights from a seeded numpy generator
    (an int seed or a Generator; None: seed 0), zero biases."""
    gen = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(0 if rng is None else rng)
    blocks, n = nsf_layout(int(d), tuple(hidden_dims), int(n_layers), int(n_bins))
    flat = np.zeros(n, dtype=np.float64)
    for _, _, kind, off, shape in blocks:
        if kind == "W":
            lim = math.sqrt(6.0 / (shape[0] + shape[1]))
            flat[off:off + shape[0] * shape[1]] = gen.uniform(-lim, lim, size=shape[0] * shape[1])
    return SplineFlow(d, hidden_dims, n_layers, n_bins, bound, flat.astype(eltype))


COUPLING_FLOWS = (RealNVPFlow, SplineFlow)


def flow_arch(q):
    """the `flow` argument of MiviContext for q (None unless q is a coupling flow)"""
    if isinstance(q, SplineFlow):
        return (q.hidden_dims, q.n_layers, q.n_bins, q.bound)
    return (q.hidden_dims, q.n_layers) if isinstance(q, RealNVPFlow) else None


class Restructure:
    """The `re` closure returned by Optimisers.destructure; RestructureMeanField for the
    Diagonal case (src/families/location_scale.jl:28-37)."""

    def __init__(self, d: int, family: int, dtype, rank: int = 0, dist=None, flow=None):
        self.d, self.family, self.dtype, self.rank = d, family, dtype, rank
        self.dist = dist if dist is not None else Normal()   # carried through, as re.model.dist (location_scale.jl:32-37)
        self.flow = flow   # REALNVP: (hidden_dims, n_layers); NSF: (hidden_dims, n_layers, n_bins, bound)

    def __call__(self, flat):
        flat = np.asarray(flat, dtype=self.dtype)
        d = self.d
        if self.family == REALNVP:
            return RealNVPFlow(d, self.flow[0], self.flow[1], flat.copy())
        if self.family == NSF:
            return SplineFlow(d, *self.flow, flat.copy())
        if self.family == LOWRANK:
            if flat.shape[0] != 2 * d + d * self.rank:
                raise ValueError("flat parameter vector has the wrong length")
            return MvLocationScaleLowRank(flat[:d].copy(), flat[d:2 * d].copy(), flat[2 * d:].reshape(d, self.rank, order="F").copy())
        if self.family == MEANFIELD:
            if flat.shape[0] != 2 * d:
                raise ValueError("flat parameter vector has the wrong length")
            return MvLocationScale(flat[:d].copy(), flat[d:].copy(), self.dist)
        if flat.shape[0] != d + d * d:
            raise ValueError("flat parameter vector has the wrong length")
        return MvLocationScale(flat[:d].copy(), np.tril(flat[d:].reshape(d, d, order="F")), self.dist)


def destructure(q):
    """Optimisers.destructure(q) -> (flat, re).
    mean-field: [location; diag(scale)], length 2d   (src/families/location_scale.jl:39-43)
    full-rank : [location; vec(scale)] column-major, length d + d^2, strict upper triangle zero
    low-rank  : [location; scale_diag; vec(scale_factors)] column-major, length 2d + d r (the functor's field order,
                src/families/location_scale_low_rank.jl:41).
    RealNVP   : the nets' weights and biases, layer by layer (flow_layout); NeuralSplineFlow likewise (nsf_layout)."""
    d = len(q)
    if q.family == REALNVP:   # the flow's own flat vector (flow_layout)
        return q.params.copy(), Restructure(d, REALNVP, q.eltype, flow=(q.hidden_dims, q.n_layers))
    if q.family == NSF:
        return q.params.copy(), Restructure(d, NSF, q.eltype, flow=flow_arch(q))
    if q.family == LOWRANK:
        flat = np.concatenate([q.location, q.scale_diag, q.scale_factors.reshape(-1, order="F")])
        return flat.astype(q.eltype, copy=False), Restructure(d, LOWRANK, q.eltype, q.rank)
    if q.family == MEANFIELD:
        flat = np.concatenate([q.location, q.scale])
    else:
        flat = np.concatenate([q.location, np.tril(q.scale).reshape(-1, order="F")])
    return flat.astype(q.eltype, copy=False), Restructure(d, q.family, q.eltype, dist=q.dist)
