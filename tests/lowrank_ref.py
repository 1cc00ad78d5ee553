"""Reference of the low-rank Gaussian family for the tests: the reference package's own expressions restated in float64 torch
(src/families/location_scale_low_rank.jl, src/algorithms/entropy.jl, src/algorithms/repgradelbo.jl), gradients by autograd, and a
numpy Woodbury evaluation in a chosen dtype -- the yardstick the device kernels are held to.

Parameters: [m (d); D (d); vec U (d x r, column-major)].  Draws: `eps` ((d + r) x M), rows 0 .. d-1 = u1, rows d .. d+r-1 = u2.
Targets are the oracle's (oracle/oracle.py: logdensity_and_gradient on a float64 column)."""
import numpy as np
import torch

LOG2PI = float(np.log(2.0 * np.pi))
CLOSED_FORM, CLOSED_FORM_ZERO_GRAD, MONTE_CARLO, STL, STL_ZERO_GRAD = range(5)


def split(params, d, r):
    """(m, D, U) views of the flat parameter vector (numpy or torch)."""
    U = params[2 * d:].reshape(r, d).T if isinstance(params, torch.Tensor) else params[2 * d:].reshape(d, r, order="F")
    return params[:d], params[d:2 * d], U


# ---- the literal reference expressions (torch, float64) ----------------------------------------------------------------------------
def entropy(m, D, U):
    """location_scale_low_rank.jl:34-43 with dist = Normal(0, 1): n entropy(dist) + (2 sum log D + logdet(I + U' (U ./ D^2))) / 2."""
    n = m.shape[0]
    UtDinvU = U.T @ (U / (D * D)[:, None])
    logdet_sigma = 2.0 * torch.sum(torch.log(D)) + torch.logdet(torch.eye(U.shape[1], dtype=U.dtype) + UtDinvU)
    return n * 0.5 * (1.0 + LOG2PI) + logdet_sigma / 2.0


def logpdf(m, D, U, z):
    """location_scale_low_rank.jl:45-68, the differentiable path: cholesky(Diagonal(D .* D) + U U'); mean(dist) = 0.
    z: one sample (d) or the samples as columns (d x M -> M values; the factor is the same for every column)."""
    L = torch.linalg.cholesky(torch.diag(D * D) + U @ U.T)
    zc = z[:, None] if z.dim() == 1 else z
    w = torch.linalg.solve_triangular(L, zc - m[:, None], upper=False)
    out = torch.sum(-0.5 * w * w - 0.5 * LOG2PI, dim=0) - torch.sum(torch.log(torch.diagonal(L)))
    return out[0] if z.dim() == 1 else out


def rand(m, D, U, eps):
    """location_scale_low_rank.jl:79-86: scale_diag .* u_diag + scale_factors * u_fact .+ location."""
    d = m.shape[0]
    return D[:, None] * eps[:d] + U @ eps[d:] + m[:, None]


class _Target(torch.autograd.Function):
    """mean-free per-column log density of an oracle target, differentiable through its own gradient."""

    @staticmethod
    def forward(ctx, Z, tgt):
        Zn = Z.detach().numpy()
        ell, G = np.empty(Zn.shape[1]), np.empty_like(Zn)
        for k in range(Zn.shape[1]):
            ell[k], G[:, k] = tgt.logdensity_and_gradient(Zn[:, k].copy())
        ctx.save_for_backward(torch.from_numpy(G))
        return torch.from_numpy(ell)

    @staticmethod
    def backward(ctx, g):
        (G,) = ctx.saved_tensors
        return G * g[None, :], None


def estimate_entropy(kind, Z, q, q_stop):
    """src/algorithms/entropy.jl; q, q_stop = (m, D, U)."""
    if kind == CLOSED_FORM:
        return entropy(*q)
    if kind == CLOSED_FORM_ZERO_GRAD:
        return entropy(*q_stop)
    if kind == MONTE_CARLO:
        return torch.mean(-logpdf(*q, Z))
    stl = torch.mean(-logpdf(*q_stop, Z))
    if kind == STL:
        return stl
    if kind == STL_ZERO_GRAD:
        return stl - entropy(*q) + entropy(*q_stop)
    raise ValueError(kind)


def forward(params, d, r, tgt, eps, kind):
    """estimate_repgradelbo_ad_forward (repgradelbo.jl:142-149): -(energy + entropy), q_stop = the same parameters detached (:162)."""
    q = split(params, d, r)
    q_stop = split(params.detach(), d, r)
    Z = rand(*q, eps)
    energy = torch.mean(_Target.apply(Z, tgt))
    return -(energy + estimate_entropy(kind, Z, q, q_stop)), Z


def estimate_gradient(params, d, r, tgt, eps, kind):
    """dict(value, grad, Z): the float64 reference of mivi_estimate_gradient on the low-rank family."""
    p = torch.tensor(np.asarray(params, dtype=np.float64), requires_grad=True)
    e = torch.tensor(np.asarray(eps, dtype=np.float64))
    val, Z = forward(p, d, r, tgt, e, kind)
    (g,) = torch.autograd.grad(val, p)
    return dict(value=float(val.detach()), grad=g.numpy().copy(), Z=Z.detach().numpy().copy())


def estimate_objective(params, d, r, tgt, eps, kind):
    """estimate_objective (repgradelbo.jl:112-118): the value with q_stop = q."""
    with torch.no_grad():
        p = torch.tensor(np.asarray(params, dtype=np.float64))
        Z = rand(*split(p, d, r), torch.tensor(np.asarray(eps, dtype=np.float64)))
        ell = np.array([tgt.logdensity(Z[:, k].numpy().copy()) for k in range(Z.shape[1])])
        q = split(p, d, r)
        return float(-(ell.mean() + estimate_entropy(kind, Z, q, q)))


# ---- the Woodbury evaluation (numpy, dtype of choice): what the device kernels compute ------------------------------------------------
def woodbury_logq(params, d, r, eps, dtype=np.float64):
    """(log q per column, V = Sigma^-1 (z - m), x = A^-1 s) by Woodbury with A = I + U' D^-2 U, every array in `dtype`."""
    p = np.asarray(params, dtype=dtype)
    m, D, U = split(p, d, r)
    e = np.asarray(eps, dtype=dtype)
    u1, u2 = e[:d], e[d:]
    Dc = D[:, None]
    A = np.eye(r, dtype=dtype) + U.T @ (U / (Dc * Dc))
    t = u1 + (U @ u2) / Dc
    s = U.T @ (t / Dc)
    x = np.linalg.solve(A, s).astype(dtype)
    logdet_a = dtype(np.linalg.slogdet(A)[1])
    quad = np.sum(t * t, axis=0) - np.sum(s * x, axis=0)
    logq = dtype(-0.5 * d * LOG2PI) - np.sum(np.log(D)) - dtype(0.5) * logdet_a - dtype(0.5) * quad
    V = (t - (U @ x) / Dc) / Dc
    return logq, V, x


def woodbury_eval(params, d, r, G, ell, eps, kind, dtype=np.float64):
    """dict(value, grad) of one estimate from G = grad log pi (d x M) and ell (M) at the samples, in `dtype`: the closed-form entropy and
    its gradient through A^-1, log q and V by Woodbury, the three cotangent products of the VJP."""
    p = np.asarray(params, dtype=dtype)
    m, D, U = split(p, d, r)
    e = np.asarray(eps, dtype=dtype)
    G, ell = np.asarray(G, dtype=dtype), np.asarray(ell, dtype=dtype)
    u1, u2 = e[:d], e[d:]
    M = e.shape[1]
    Dc = D[:, None]
    A = np.eye(r, dtype=dtype) + U.T @ (U / (Dc * Dc))
    Ainv = np.linalg.inv(A).astype(dtype)
    H = dtype(0.5 * d * (1.0 + LOG2PI)) + np.sum(np.log(D)) + dtype(0.5) * dtype(np.linalg.slogdet(A)[1])
    UA = U @ Ainv
    dH_U = UA / (Dc * Dc)
    dH_D = 1 / D - np.sum(UA * U, axis=1) / D ** 3

    def vjp(C, a1, a2):
        return C.mean(axis=1), (C * a1).mean(axis=1), (C @ a2.T) / dtype(M)

    closed = kind in (CLOSED_FORM, CLOSED_FORM_ZERO_GRAD)
    if closed:
        value = -ell.mean() - H
        gm, gD, gU = vjp(G, u1, u2)
        if kind == CLOSED_FORM:
            gD, gU = gD + dH_D, gU + dH_U
    else:
        logq, V, x = woodbury_logq(p, d, r, e, dtype)
        value = -ell.mean() + logq.mean()
        if kind == MONTE_CARLO:
            gm, gD, gU = vjp(G, u1, u2)
            _, vD, vU = vjp(V, u1 - Dc * V, u2 - U.T @ V)
            gD, gU = gD + vD + dH_D, gU + vU + dH_U
        else:
            gm, gD, gU = vjp(G + V, u1, u2)
            if kind == STL_ZERO_GRAD:
                gD, gU = gD - dH_D, gU - dH_U
    grad = -np.concatenate([gm, gD, gU.reshape(-1, order="F")])
    return dict(value=float(value), grad=grad.astype(np.float64))
