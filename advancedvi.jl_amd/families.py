"""Variational family containers mirroring src/families/location_scale.jl and location_scale_low_rank.jl (AdvancedVI.jl v0.7.0).

Only what the RepGradELBO hot path needs: the `MvLocationScale` container, the two Gaussian
constructors, and `destructure` / restructure.  All arithmetic on samples (rand, entropy, logpdf
inside the estimators) runs in libmivi's HIP kernels."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

MEANFIELD, FULLRANK, LOWRANK = 0, 1, 2
LOWRANK_MAX_RANK = 64   # MIVI_LOWRANK_MAX_RANK (include/mivi.h)


@dataclass
class MvLocationScale:
    """MvLocationScale(location, scale, dist) with dist = Normal(0, 1)
    (src/families/location_scale.jl:15-19).  `scale` is a length-d vector (Diagonal) or a d x d
    lower-triangular matrix (LowerTriangular).  Arrays are numpy (host) float32/float64."""

    location: np.ndarray
    scale: np.ndarray

    def __post_init__(self):
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
    def mean(self):
        return self.location.copy()   # mean(dist) = 0: the scale terms of :105-107 vanish

    def var(self):
        return self.scale_diag ** 2 + (self.scale_factors ** 2).sum(axis=1)   # var(dist) = 1

    def cov(self):
        return np.diag(self.scale_diag ** 2) + self.scale_factors @ self.scale_factors.T


def LowRankGaussian(mu, D, U) -> MvLocationScaleLowRank:
    """LowRankGaussian(mu, D, U): src/families/location_scale_low_rank.jl:140-145."""
    return MvLocationScaleLowRank(np.asarray(mu), np.asarray(D), np.asarray(U))


class Restructure:
    """The `re` closure returned by Optimisers.destructure; RestructureMeanField for the
    Diagonal case (src/families/location_scale.jl:28-37)."""

    def __init__(self, d: int, family: int, dtype, rank: int = 0):
        self.d, self.family, self.dtype, self.rank = d, family, dtype, rank

    def __call__(self, flat):
        flat = np.asarray(flat, dtype=self.dtype)
        d = self.d
        if self.family == LOWRANK:
            if flat.shape[0] != 2 * d + d * self.rank:
                raise ValueError("flat parameter vector has the wrong length")
            return MvLocationScaleLowRank(flat[:d].copy(), flat[d:2 * d].copy(), flat[2 * d:].reshape(d, self.rank, order="F").copy())
        if self.family == MEANFIELD:
            if flat.shape[0] != 2 * d:
                raise ValueError("flat parameter vector has the wrong length")
            return MvLocationScale(flat[:d].copy(), flat[d:].copy())
        if flat.shape[0] != d + d * d:
            raise ValueError("flat parameter vector has the wrong length")
        return MvLocationScale(flat[:d].copy(), np.tril(flat[d:].reshape(d, d, order="F")))


def destructure(q):
    """Optimisers.destructure(q) -> (flat, re).
    mean-field: [location; diag(scale)], length 2d   (src/families/location_scale.jl:39-43)
    full-rank : [location; vec(scale)] column-major, length d + d^2, strict upper triangle zero
    low-rank  : [location; scale_diag; vec(scale_factors)] column-major, length 2d + d r (the functor's field order,
                src/families/location_scale_low_rank.jl:41)."""
    d = len(q)
    if q.family == LOWRANK:
        flat = np.concatenate([q.location, q.scale_diag, q.scale_factors.reshape(-1, order="F")])
        return flat.astype(q.eltype, copy=False), Restructure(d, LOWRANK, q.eltype, q.rank)
    if q.family == MEANFIELD:
        flat = np.concatenate([q.location, q.scale])
    else:
        flat = np.concatenate([q.location, np.tril(q.scale).reshape(-1, order="F")])
    return flat.astype(q.eltype, copy=False), Restructure(d, q.family, q.eltype)
