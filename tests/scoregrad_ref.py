"""numpy restatement of the score-gradient ELBO objective (ScoreGradELBO, src/algorithms/scoregradelbo.jl) -- a helper of the
score-gradient tests, not a test.  Built on oracle.oracle's families, `logpdf`, targets and `philox_normal`.

    literal_forward   estimate_scoregradelbo_ad_forward, scoregradelbo.jl:87-94, as written: (mean(f^2) - mean(f)^2) / 2 with
                      f = logpdf.(q, samples_stop) - logprob_stop
    closed_form       value / elbo / gradient of estimate_gradient! (scoregradelbo.jl:96-117) with the AD of the forward replaced by
                          value = mean((f - fbar)^2) / 2            elbo = -fbar
                          full rank : dmu = (1/M) C^-T E (f - fbar)      dC = (1/M) tril(C^-T E diag(f - fbar) E')
                          mean field: dmu = (1/M) E (f - fbar) / sigma    dsigma = (1/M) (E .* E) (f - fbar) / sigma
                      on the draws E (d x M), where log q(z_m) = -|eps_m|^2 / 2 - sum log C_ii - (d / 2) log 2 pi.

Every function takes `dtype`: np.float64 is the reference result, np.float32 the same arithmetic at the precision of an f32 context
(samples, per-sample log-densities, f, the weights and the products all rounded to float32) -- the yardstick the GPU parity test holds
the f32 library against."""
import numpy as np

from oracle import oracle as O

LOG2PI = float(np.log(2.0 * np.pi))


def _family(params, d, family, dtype):
    q = O.restructure(np.asarray(params, dtype=np.float64), d, family)
    return q.location.astype(dtype), q.scale.astype(dtype)


def samples(params, d, family, eps, dtype=np.float64):
    """rand(rng, q, M) on the draws eps: location_scale.jl:71-87."""
    mu, S = _family(params, d, family, dtype)
    e = np.asarray(eps).astype(dtype)
    return (S[:, None] * e if S.ndim == 1 else S @ e) + mu[:, None]


def target_values(prob, Z, dtype=np.float64):
    """map(logdensity(prob, .), eachsample(samples)): scoregradelbo.jl:44,108 (the target sees the samples as `dtype` holds them)."""
    return np.array([prob.logdensity(np.asarray(Z[:, m], dtype=np.float64)) for m in range(Z.shape[1])]).astype(dtype)


def logpdf_cols(params, d, family, Z, dtype=np.float64):
    """logpdf.(Ref(q), eachsample(Z)): O.logpdf column by column in float64; the same expression (location_scale.jl:59-63) in `dtype`
    arithmetic otherwise."""
    dtype = np.dtype(dtype).type
    if dtype is np.float64:
        q = O.restructure(np.asarray(params, dtype=np.float64), d, family)
        return np.array([O.logpdf(q, np.asarray(Z[:, m], dtype=np.float64)) for m in range(Z.shape[1])])
    mu, S = _family(params, d, family, dtype)
    R = np.asarray(Z).astype(dtype) - mu[:, None]
    Zs = R / S[:, None] if S.ndim == 1 else np.linalg.solve(np.tril(S), R).astype(dtype)
    diag = S if S.ndim == 1 else np.diag(S)
    half, l2pi = dtype(0.5), dtype(LOG2PI)
    return (np.sum(-half * Zs * Zs - half * l2pi, axis=0, dtype=dtype) - np.sum(np.log(diag), dtype=dtype)).astype(dtype)


def literal_forward(params, d, family, Z_stop, logprob_stop, dtype=np.float64):
    """estimate_scoregradelbo_ad_forward(params, aux): scoregradelbo.jl:87-94, literally."""
    dtype = np.dtype(dtype).type
    lq = logpdf_cols(params, d, family, Z_stop, dtype)
    f = (lq - np.asarray(logprob_stop).astype(dtype)).astype(dtype)
    return (np.mean(f * f, dtype=dtype) - np.mean(f, dtype=dtype) ** 2) / dtype(2)


def closed_form(params, d, family, prob, eps, dtype=np.float64):
    """dict(value, elbo, grad, w, f, Z, logpi) of one ScoreGradELBO estimate on the draws `eps` (d x M)."""
    dtype = np.dtype(dtype).type
    mu, S = _family(params, d, family, dtype)
    E = np.asarray(eps).astype(dtype)
    M = E.shape[1]
    Z = samples(params, d, family, E, dtype)
    lp = target_values(prob, Z, dtype)
    diag = S if S.ndim == 1 else np.diag(S)
    lq = (-dtype(0.5) * np.sum(E * E, axis=0, dtype=dtype) - np.sum(np.log(diag), dtype=dtype) - dtype(0.5 * d * LOG2PI)).astype(dtype)
    f = (lq - lp).astype(dtype)
    fbar = np.mean(f, dtype=dtype)
    w = (f - fbar).astype(dtype)
    value = np.mean(w * w, dtype=dtype) / dtype(2)
    if S.ndim == 1:
        gmu = (E @ w) / S / dtype(M)
        gsc = ((E * E) @ w) / S / dtype(M)
        grad = np.concatenate([gmu, gsc])
    else:
        X = np.linalg.solve(np.tril(S).T, E * w[None, :]).astype(dtype)   # C^-T E diag(w)
        gmu = np.sum(X, axis=1, dtype=dtype) / dtype(M)
        gC = np.tril(X @ E.T) / dtype(M)
        grad = np.concatenate([gmu, gC.reshape(-1, order="F")])
    return dict(value=dtype(value), elbo=dtype(-fbar), grad=grad.astype(dtype), w=w, f=f, Z=Z, logpi=lp)


def philox_draws(seed, idx, d, M, f64=False):
    """The draws of estimate `idx` (what mivi_sample returns as eps): oracle.philox_normal."""
    return O.philox_normal(seed, idx, d, 0, M, f64=f64)
