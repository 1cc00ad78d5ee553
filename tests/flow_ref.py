"""The RealNVP family (MIVI_REALNVP, include/mivi.h) restated twice, for tests/test_flow_ref_host.py and tests/test_gpu_flow.py.

1. The literal definition in float64 torch: `forward`, `inverse`, `logpdf`; gradients by autograd (`estimate_gradient`).  For the
   sticking-the-landing estimator autograd goes through `logpdf` of a DETACHED parameter copy evaluated at z (entropy.jl:57-65).
2. A numpy forward pass with the hand-written backward sweeps of the kernels' documentation, every step in ONE chosen dtype (`evaluate`):
   np.float64 is the reference of float32 contexts, np.longdouble that of float64 contexts, and the same evaluation in the context's
   dtype is the yardstick a device result is held against (at most 8 x its error, floored).  `evaluate` can inject the faults the
   criterion has to see, and sum the samples in another order.

An architecture is the tuple arch = (d, hidden_dims, n_layers).  Samples are columns: eps, Z, G are d x M."""
import math

import numpy as np
import torch


MONTE_CARLO, STL = 2, 3
TILE = 16   # samples per tile of the kernels (what "a lost last sample tile" means)


def masks(d, l):
    """(A_l, B_l), 0-based: the even coordinates transform on odd layers, the odd ones on even layers."""
    A = np.arange(0 if l % 2 == 1 else 1, d, 2)
    return A, np.setdiff1d(np.arange(d), A)


def flow_layout(d, hidden, L):
    """The parameter vector as include/mivi.h states it, written out here so that the reference does not take it from the package under
    test: for l = 1 .. L the s net, then the t net; a net is [vec W_1 (out x in); b_1; ...; vec W_{H+1}; b_{H+1}] from |B_l| inputs to
    |A_l| outputs.  -> ([(l, net, j, "W" | "b", offset, shape)], length)"""
    out, off = [], 0
    for l in range(1, L + 1):
        n_a = len(masks(d, l)[0])
        widths = [d - n_a] + list(hidden) + [n_a]
        for net in "st":
            for j in range(1, len(widths)):
                out.append((l, net, j, "W", off, (widths[j], widths[j - 1])))
                off += widths[j] * widths[j - 1]
                out.append((l, net, j, "b", off, (widths[j],)))
                off += widths[j]
    return out, off


def blocks(arch):
    """[(name, slice)] of the parameter vector: one entry per W_j and b_j of each net of each layer."""
    d, hidden, L = arch
    return [(f"l{l}.{net}.{k}{j}", slice(off, off + int(np.prod(shape)))) for l, net, j, k, off, shape in flow_layout(d, hidden, L)[0]]


def _nets(params, arch, as_matrix):
    """{l: {"s": [(W, b), ...], "t": [...]}} with W = as_matrix(flat block, out, in)"""
    d, hidden, L = arch
    out = {l: {"s": [], "t": []} for l in range(1, L + 1)}
    lay = flow_layout(d, hidden, L)[0]
    for (l, net, j, k, off, shape), (_, _, _, _, boff, bshape) in zip(lay[0::2], lay[1::2]):
        out[l][net].append((as_matrix(params[off:off + shape[0] * shape[1]], *shape), params[boff:boff + bshape[0]]))
    return out


# ---- 1. torch, float64 ------------------------------------------------------------------------------------------------------------
def _t_nets(p, arch):
    return _nets(p, arch, lambda v, o, i: v.reshape(i, o).T)   # vec W column-major, out x in


def _t_net(net, c, tanh):
    h = c
    for j, (W, b) in enumerate(net):
        h = W @ h + b[:, None]
        if j < len(net) - 1:
            h = torch.nn.functional.leaky_relu(h, 0.01)
    return torch.tanh(h) if tanh else h


def forward(p, arch, eps):
    """(z, log q(z)) of the draws eps (d x M)."""
    d, _, L = arch
    nets = _t_nets(p, arch)
    x, ssum = eps, 0.0
    for l in range(1, L + 1):
        A, B = masks(d, l)
        c = x[B]
        s, t = _t_net(nets[l]["s"], c, True), _t_net(nets[l]["t"], c, False)
        y = x.clone()
        y[A] = x[A] * torch.exp(s) + t
        x, ssum = y, ssum + s.sum(0)
    return x, -0.5 * (eps * eps).sum(0) - 0.5 * d * math.log(2.0 * math.pi) - ssum


def inverse(p, arch, z):
    """(eps, sum_l 1' s_l) with z = T(eps)."""
    d, _, L = arch
    nets = _t_nets(p, arch)
    y, ssum = z, 0.0
    for l in range(L, 0, -1):
        A, B = masks(d, l)
        c = y[B]
        s, t = _t_net(nets[l]["s"], c, True), _t_net(nets[l]["t"], c, False)
        x = y.clone()
        x[A] = (y[A] - t) * torch.exp(-s)
        y, ssum = x, ssum + s.sum(0)
    return y, ssum


def logpdf(p, arch, z):
    eps, ssum = inverse(p, arch, z)
    return -0.5 * (eps * eps).sum(0) - 0.5 * arch[0] * math.log(2.0 * math.pi) - ssum


class _Target(torch.autograd.Function):
    """per-column log density of an oracle target, differentiable through its own gradient."""

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


def estimate_gradient(params, arch, tgt, eps, kind):
    """dict(value, grad, Z, logq): the float64 autograd reference of mivi_estimate_gradient; value = mean[-ell(z) + log q(z)]."""
    p = torch.tensor(np.asarray(params, dtype=np.float64), requires_grad=True)
    e = torch.tensor(np.asarray(eps, dtype=np.float64))
    Z, _ = forward(p, arch, e)
    energy = torch.mean(_Target.apply(Z, tgt))
    lq = logpdf(p if kind == MONTE_CARLO else p.detach(), arch, Z)
    val = -energy + torch.mean(lq)
    (g,) = torch.autograd.grad(val, p)
    return dict(value=float(val.detach()), grad=g.numpy().copy(), Z=Z.detach().numpy().copy(), logq=lq.detach().numpy().copy())


def target_columns(tgt, Z):
    """(ell (M), G (d x M)) of an oracle target at the columns of Z."""
    cols = [tgt.logdensity_and_gradient(np.asarray(Z[:, k], dtype=np.float64).copy()) for k in range(Z.shape[1])]
    return np.array([c[0] for c in cols]), np.stack([c[1] for c in cols], axis=1)


# ---- 2. numpy, one dtype ----------------------------------------------------------------------------------------------------------
def _np_forward_net(net, c, dtype, tanh):
    acts, h = [c], c
    for j, (W, b) in enumerate(net):
        h = W @ h + b[:, None]
        if j < len(net) - 1:
            h = np.where(h > 0, h, dtype(0.01) * h)
            acts.append(h)
    return (np.tanh(h) if tanh else h), acts


def _np_backward_net(net, acts, delta, cols=None):
    """delta: the cotangent of the output layer's pre-activation.  -> ([dW_1, db_1, ...] or None without `cols`, the input's cotangent);
    cols: the sample columns the parameter gradient sums, in that order."""
    grads = []
    for j in range(len(net) - 1, -1, -1):
        W = net[j][0]
        if cols is not None:
            grads = [delta[:, cols] @ acts[j][:, cols].T, delta[:, cols].sum(axis=1)] + grads
        delta = W.T @ delta
        if j > 0:
            delta = delta * np.where(acts[j] > 0, W.dtype.type(1), W.dtype.type(0.01))
    return grads, delta


def evaluate(params, arch, G, ell, eps, kind, dtype=np.float64, fault=None, order=None):
    """dict(Z, logq, value, grad): the forward pass and the two backward sweeps with every step in `dtype`, G = grad_z ell and ell given.
    order: a permutation of the samples -- the parameter gradient and the value sum them in that order.
    fault: None | "lost_block" | "lost_tile" | "swap_masks" | "no_kappa" | "kappa_sign" | "no_u"."""
    d, hidden, L = arch
    M = eps.shape[1]
    T = np.dtype(dtype).type
    p = np.asarray(params).astype(dtype)
    nets = _nets(p, arch, lambda v, o, i: v.reshape((o, i), order="F"))
    eps, G, ell = np.asarray(eps).astype(dtype), np.asarray(G).astype(dtype), np.asarray(ell).astype(dtype)
    cols = np.arange(M) if order is None else np.asarray(order)
    if fault == "lost_tile":
        cols = cols[cols < TILE * ((M - 1) // TILE)]
    mk = (lambda l: masks(d, l + 1)) if fault == "swap_masks" else (lambda l: masks(d, l))
    xs, ssum = [eps], np.zeros(M, dtype=dtype)
    for l in range(1, L + 1):
        A, B = mk(l)
        x = xs[-1]
        s, _ = _np_forward_net(nets[l]["s"], x[B], T, True)
        t, _ = _np_forward_net(nets[l]["t"], x[B], T, False)
        y = x.copy()
        y[A] = x[A] * np.exp(s) + t
        xs.append(y)
        ssum = ssum + s.sum(axis=0)
    logq = T(-0.5) * (eps * eps).sum(axis=0) - T(0.5 * d * math.log(2.0 * math.pi)) - ssum
    value = ((-ell + logq)[cols]).sum() / T(M)
    if kind == STL:   # u = grad_z log q(z), the parameters stopped: l = 1 .. L through the inverse layers
        xb = -eps
        for l in range(1, L + 1):
            A, B = mk(l)
            x = xs[l - 1]
            s, acts_s = _np_forward_net(nets[l]["s"], x[B], T, True)
            _, acts_t = _np_forward_net(nets[l]["t"], x[B], T, False)
            ab, ems = xb[A], np.exp(-s)
            _, cs = _np_backward_net(nets[l]["s"], acts_s, (-ab * x[A] - T(1)) * (T(1) - s * s))
            _, ct = _np_backward_net(nets[l]["t"], acts_t, -ab * ems)
            yb = xb.copy()
            yb[A] = ab * ems
            yb[B] = xb[B] + cs + ct
            xb = yb
        g = (-G + (T(0) * xb if fault == "no_u" else xb)) / T(M)
        kappa = T(0)
    else:
        g = -G / T(M)
        kappa = {None: T(-1), "no_kappa": T(0), "kappa_sign": T(1)}.get(fault, T(-1)) / T(M)
    grad = np.zeros(p.shape[0], dtype=dtype)
    names = dict(blocks(arch))
    for l in range(L, 0, -1):
        A, B = mk(l)
        x = xs[l - 1]
        s, acts_s = _np_forward_net(nets[l]["s"], x[B], T, True)
        _, acts_t = _np_forward_net(nets[l]["t"], x[B], T, False)
        es = np.exp(s)
        gs, cs = _np_backward_net(nets[l]["s"], acts_s, (g[A] * x[A] * es + kappa) * (T(1) - s * s), cols)
        gt, ct = _np_backward_net(nets[l]["t"], acts_t, g[A], cols)
        for net, gr in (("s", gs), ("t", gt)):
            for j in range(len(hidden) + 1):
                grad[names[f"l{l}.{net}.W{j + 1}"]] = gr[2 * j].reshape(-1, order="F")
                grad[names[f"l{l}.{net}.b{j + 1}"]] = gr[2 * j + 1]
        gn = g.copy()
        gn[A] = g[A] * es
        gn[B] = g[B] + cs + ct
        g = gn
    if fault == "lost_block":
        grad[blocks(arch)[len(blocks(arch)) // 2][1]] = 0
    return dict(Z=xs[-1], logq=logq, value=value, grad=grad)


def ref_dtype(dtype):
    """the dtype of the reference evaluation for a context of `dtype`"""
    return np.float64 if np.dtype(dtype) == np.float32 else np.longdouble


def margin(params, arch, eps):
    """the smallest |p| / (sum_j |W_ij| |a_j| + |b_i|) over all hidden pre-activations p of all nets (float64): how far every leakyrelu
    is from its kink, in units of the scale its rounding error has."""
    d, hidden, L = arch
    nets = _nets(np.asarray(params, dtype=np.float64), arch, lambda v, o, i: v.reshape((o, i), order="F"))
    x, best = np.asarray(eps, dtype=np.float64), np.inf
    for l in range(1, L + 1):
        A, B = masks(d, l)
        out = {}
        for name in ("s", "t"):
            h = x[B]
            for j, (W, b) in enumerate(nets[l][name]):
                pre = W @ h + b[:, None]
                if j < len(hidden):
                    scale = np.abs(W) @ np.abs(h) + np.abs(b)[:, None]
                    best = min(best, float(np.min(np.abs(pre) / np.maximum(scale, 1e-300))))
                    h = np.where(pre > 0, pre, 0.01 * pre)
                else:
                    out[name] = np.tanh(pre) if name == "s" else pre
        y = x.copy()
        y[A] = x[A] * np.exp(out["s"]) + out["t"]
        x = y
    return best


# ---- the criterion ----------------------------------------------------------------------------------------------------------------
TOL = {np.dtype(np.float32): (1e-5, 2e-5), np.dtype(np.float64): (1e-12, 1e-11)}   # tests/test_gpu_lowrank.py: value relative, gradient relative l2
STOL = {np.dtype(np.float32): 1e-6, np.dtype(np.float64): 1e-14}                 # ... samples and draws, relative l2


def block_report(got, ref, yard, arch, dtype):
    """[(name, error, bound)] for the whole gradient and for every parameter block: the error against the reference is at most 8 x the
    yardstick's, floored at gt x max(|ref_b|, gscale sqrt(n_b / n)) -- the block's share of the whole-gradient allowance gt x gscale."""
    gt = TOL[np.dtype(dtype)][1]
    got, ref, yard = (np.asarray(v, dtype=np.longdouble) for v in (got, ref, yard))
    n, gscale = ref.shape[0], max(float(np.linalg.norm(ref)), 1.0)
    rows = [("all", float(np.linalg.norm(got - ref)), max(gt * gscale, 8 * float(np.linalg.norm(yard - ref))))]
    for name, sl in blocks(arch):
        nb = sl.stop - sl.start
        floor = gt * max(float(np.linalg.norm(ref[sl])), gscale * math.sqrt(nb / n))
        rows.append((name, float(np.linalg.norm(got[sl] - ref[sl])), max(floor, 8 * float(np.linalg.norm(yard[sl] - ref[sl])))))
    return rows


def violations(rows):
    return [r for r in rows if not r[1] <= r[2]]


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
# (d, hidden, L, M): the tutorial's shape; halves of 2 and 1; a partial sample tile; across the 16-tile in every axis with three hidden
# layers; 64 x 64; the maximum halves; many sample slices.  The third entry of a case is the seed of its parameters: the first one at which
# margin() clears 1e-4 with some room on the float32 draws and 1e-12 on the float64 draws of estimate CASE_IDX (tests/test_flow_ref_host.py pins that).
CASE_IDX = 3
CASES = {
    (2, (16, 16), 3, 8): 0,
    (3, (5,), 1, 1): 0,
    (5, (16, 7), 2, 33): 3,
    (17, (33, 20, 7), 3, 16): 13,
    (64, (64, 64), 4, 16): 1173,
    (128, (64,), 2, 16): 96,
    (5, (8,), 2, 600): 51,
}


def case_params(case, dtype, seed=None):
    """Glorot-uniform weights and N(0, 0.1^2) biases from the case's seed, rounded to dtype."""
    d, hidden, L, _ = case
    seed = CASES[case] if seed is None else seed
    lay, n = flow_layout(d, hidden, L)
    p, gen = np.zeros(n), np.random.default_rng(seed)
    for _, _, _, kind, off, shape in lay:   # (the draws avi.RealNVP makes: tests/test_flow_ref_host.py compares the two)
        if kind == "W":
            lim = math.sqrt(6.0 / (shape[0] + shape[1]))
            p[off:off + shape[0] * shape[1]] = gen.uniform(-lim, lim, size=shape[0] * shape[1])
    gen = np.random.default_rng(1000 + seed)
    for name, sl in blocks((d, hidden, L)):
        if ".b" in name:
            p[sl] = 0.1 * gen.normal(size=sl.stop - sl.start)
    return p.astype(dtype)
