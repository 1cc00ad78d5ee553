"""The neural spline flow family (MIVI_NSF, include/mivi.h) restated twice, for tests/test_nsf_ref_host.py, tests/test_gpu_nsf.py and
tests/test_gpu_nsf_yardstick.py (the per-entry criterion: second half of this file -- magnitude, envelope, ratios, YARD_CASES).

1. The literal definition in float64 torch: `forward`, `inverse`, `logpdf`; gradients by autograd (`estimate_gradient`).  For the
   sticking-the-landing estimator autograd goes through `logpdf` of a DETACHED parameter copy evaluated at z (entropy.jl:57-65).
2. A numpy forward pass with hand-written backward formulas through the spline and its softmax / softplus parameterisation, every step
   in ONE chosen dtype (`evaluate`): np.float64 is the reference of float32 contexts, np.longdouble that of float64 contexts, and the same
   evaluation in float32 is the yardstick a float32 device result is held against.  The nets' forward pass is tests/flow_ref.py's own
   (_np_forward_net); the backward pass is that file's with the output layer's input VJP walked in chunks (_backward_net).  `evaluate`
   can inject the faults the criterion has to see, sum the samples in another order, and follow the kernels' own order.

The criterion is that of tests/flow_ref.py (block_report there is written for RealNVP's layout; `report` here is the same rule on this
family's blocks, with that file's TOL / STOL): float32 -- sample, value, log q, the whole gradient and every parameter block within
FACTOR = 8 x the error of the float32 numpy evaluation against float64, floored at flow_ref.TOL; float64 -- value, whole gradient and
every block within flow_ref.TOL alone; the sample and log q, as in tests/test_gpu_flow.py's run_case, within 8 x the float64 evaluation's
own error against long double, floored at STOL / TOL.

An architecture is the tuple arch = (d, hidden_dims, n_layers, n_bins, bound).  Samples are columns: eps, Z, G are d x M."""
import math

import numpy as np
import torch

from tests import flow_ref as R

MONTE_CARLO, STL = R.MONTE_CARLO, R.STL
TILE = R.TILE
FACTOR = 8
masks = R.masks


def nsf_layout(d, hidden, L, K):
    """The parameter vector as include/mivi.h states it, written out here so that the reference does not take it from the package under
    test: for l = 1 .. L ONE net [vec W_1 (out x in, column-major); b_1; ...; vec W_{H+1}; b_{H+1}] from |B_l| inputs to |A_l| (3K - 1)
    outputs.  -> ([(l, j, "W" | "b", offset, shape)], length)"""
    out, off = [], 0
    for l in range(1, L + 1):
        n_a = len(masks(d, l)[0])
        widths = [d - n_a] + list(hidden) + [n_a * (3 * K - 1)]
        for j in range(1, len(widths)):
            out.append((l, j, "W", off, (widths[j], widths[j - 1])))
            off += widths[j] * widths[j - 1]
            out.append((l, j, "b", off, (widths[j],)))
            off += widths[j]
    return out, off


def blocks(arch):
    """[(name, slice)] of the parameter vector: one entry per W_j and b_j of each layer's net."""
    d, hidden, L, K, _ = arch
    return [(f"l{l}.{k}{j}", slice(off, off + int(np.prod(shape)))) for l, j, k, off, shape in nsf_layout(d, hidden, L, K)[0]]


def _nets(params, arch, as_matrix):
    """{l: [(W, b), ...]} with W = as_matrix(flat block, out, in)"""
    d, hidden, L, K, _ = arch
    out = {l: [] for l in range(1, L + 1)}
    lay = nsf_layout(d, hidden, L, K)[0]
    for (l, j, k, off, shape), (_, _, _, boff, bshape) in zip(lay[0::2], lay[1::2]):
        out[l].append((as_matrix(params[off:off + shape[0] * shape[1]], *shape), params[boff:boff + bshape[0]]))
    return out


# ---- 1. torch, float64 ------------------------------------------------------------------------------------------------------------
def _t_spline(theta, K, B, v, inverse):
    """theta (nA, 3K - 1, M), v (nA, M) -> (f(v) or f^-1(v), log f' at the spline's input), the identity outside (-B, B)"""
    uw, uh, ud = theta[:, :K], theta[:, K:2 * K], theta[:, 2 * K:]
    w, h = 2 * B * torch.softmax(uw, dim=1), 2 * B * torch.softmax(uh, dim=1)
    one = torch.ones_like(w[:, :1])
    delta = torch.cat([one, torch.nn.functional.softplus(ud), one], dim=1)
    X = torch.cat([-B * one, -B + torch.cumsum(w, dim=1)], dim=1)
    Y = torch.cat([-B * one, -B + torch.cumsum(h, dim=1)], dim=1)
    inside = (v > -B) & (v < B)
    vs = torch.where(inside, v, torch.zeros_like(v))
    k = ((Y if inverse else X)[:, 1:K] <= vs[:, None, :]).sum(dim=1)
    take = lambda arr, idx: torch.gather(arr, 1, idx[:, None, :])[:, 0]   # noqa: E731
    wk, hk, d0, d1, X0, Y0 = take(w, k), take(h, k), take(delta, k), take(delta, k + 1), take(X, k), take(Y, k)
    s = hk / wk
    t = d1 + d0 - 2 * s
    if inverse:
        dy = vs - Y0
        qa, qb, qc = hk * (s - d0) + dy * t, hk * d0 - dy * t, -s * dy
        xi = 2 * qc / (-qb - torch.sqrt(qb * qb - 4 * qa * qc))
        res = X0 + xi * wk
    else:
        xi = (vs - X0) / wk
    D = s + t * xi * (1 - xi)
    if not inverse:
        res = Y0 + hk * (s * xi * xi + d0 * xi * (1 - xi)) / D
    ld = 2 * torch.log(s) + torch.log(d1 * xi * xi + 2 * s * xi * (1 - xi) + d0 * (1 - xi) ** 2) - 2 * torch.log(D)
    return torch.where(inside, res, v), torch.where(inside, ld, torch.zeros_like(ld))


def _t_net(net, c):
    h = c
    for j, (W, b) in enumerate(net):
        h = W @ h + b[:, None]
        if j < len(net) - 1:
            h = torch.nn.functional.leaky_relu(h, 0.01)
    return h


def _t_sweep(p, arch, x, inverse):
    d, _, L, K, B = arch
    nets = _nets(p, arch, lambda v, o, i: v.reshape(i, o).T)   # vec W column-major, out x in
    ldsum = 0.0
    for l in (range(L, 0, -1) if inverse else range(1, L + 1)):
        A, Bm = masks(d, l)
        theta = _t_net(nets[l], x[Bm]).reshape(len(A), 3 * K - 1, -1)
        y = x.clone()
        y[A], ld = _t_spline(theta, K, B, x[A], inverse)
        x, ldsum = y, ldsum + ld.sum(0)
    return x, ldsum


def forward(p, arch, eps):
    """(z, log q(z)) of the draws eps (d x M)."""
    z, ldsum = _t_sweep(p, arch, eps, False)
    return z, -0.5 * (eps * eps).sum(0) - 0.5 * arch[0] * math.log(2.0 * math.pi) - ldsum


def inverse(p, arch, z):
    """(eps, sum_l sum_i log f'_{l,i}) with z = T(eps)."""
    return _t_sweep(p, arch, z, True)


def logpdf(p, arch, z):
    eps, ldsum = inverse(p, arch, z)
    return -0.5 * (eps * eps).sum(0) - 0.5 * arch[0] * math.log(2.0 * math.pi) - ldsum


def estimate_gradient(params, arch, tgt, eps, kind):
    """dict(value, grad, Z, logq): the float64 autograd reference of mivi_estimate_gradient; value = mean[-ell(z) + log q(z)]."""
    p = torch.tensor(np.asarray(params, dtype=np.float64), requires_grad=True)
    e = torch.tensor(np.asarray(eps, dtype=np.float64))
    Z, _ = forward(p, arch, e)
    energy = torch.mean(R._Target.apply(Z, tgt))
    lq = logpdf(p if kind == MONTE_CARLO else p.detach(), arch, Z)
    val = -energy + torch.mean(lq)
    (g,) = torch.autograd.grad(val, p)
    return dict(value=float(val.detach()), grad=g.numpy().copy(), Z=Z.detach().numpy().copy(), logq=lq.detach().numpy().copy())


target_columns = R.target_columns


# ---- 2. numpy, one dtype ----------------------------------------------------------------------------------------------------------
BLOCK_FAULTS = ("delta_ends", "inverse_bin_on_X", "no_2logD", "lost_chunk", "lost_tile", "tails_not_identity")   # what `report` is pinned to see
FAULTS = BLOCK_FAULTS + ("one_entry", "one_row", "edge_slope", "stale_chunk_rows", "acc_reset", "slice_cap", "B_unrounded")


def _softplus(u):
    return np.maximum(u, 0) + np.log1p(np.exp(-np.abs(u)))


def _sigmoid(u):
    e = np.exp(-np.abs(u))
    return np.where(u > 0, u.dtype.type(1), e) / (1 + e)


def _softmax2B(u, B, T, unrounded=False):
    e = np.exp(u - u.max(axis=1, keepdims=True))
    if unrounded:   # (fault B_unrounded) 2B and the product with it in float64, rounded to T afterwards
        return (np.float64(2.0 * B) * e.astype(np.float64) / e.sum(axis=1, keepdims=True).astype(np.float64)).astype(T)
    return T(2) * T(B) * e / e.sum(axis=1, keepdims=True)


def _take(arr, idx):
    return np.take_along_axis(arr, idx[:, None, :], axis=1)[:, 0]


def _setup(theta, K, B, T, v, on_y, fault):
    """the bin of every (coordinate, sample) and its quantities; theta (nA, 3K - 1, M), v (nA, M); the knots are running sums from -B"""
    uw, uh, ud = theta[:, :K], theta[:, K:2 * K], theta[:, 2 * K:]
    w, h = _softmax2B(uw, B, T, fault == "B_unrounded"), _softmax2B(uh, B, T, fault == "B_unrounded")
    one = np.ones_like(w[:, :1])
    dl = _softplus(ud)
    delta = np.concatenate([dl[:, :1], dl, dl[:, -1:]] if fault == "delta_ends" else [one, dl, one], axis=1)
    X, Y = np.cumsum(np.concatenate([-T(B) * one, w], axis=1), axis=1), np.cumsum(np.concatenate([-T(B) * one, h], axis=1), axis=1)
    inside = (v > -T(B)) & (v < T(B))
    vs = np.where(inside, v, T(0))
    if fault == "tails_not_identity":   # the edge bins' rational functions carried on outside
        inside, vs = np.ones_like(inside), v
    k = ((Y if on_y else X)[:, 1:K] <= vs[:, None, :]).sum(axis=1)
    return dict(w=w, h=h, ud=ud, k=k, inside=inside, v=vs, wk=_take(w, k), hk=_take(h, k), d0=_take(delta, k), d1=_take(delta, k + 1),
                X0=_take(X, k), Y0=_take(Y, k))


def _spline(theta, K, B, T, v, inverse=False, fault=None):
    """-> (f(v) or f^-1(v), log f' at the spline's input a)"""
    with np.errstate(all="ignore"):
        c = _setup(theta, K, B, T, v, inverse and fault != "inverse_bin_on_X", fault)
        wk, hk, d0, d1 = c["wk"], c["hk"], c["d0"], c["d1"]
        s = hk / wk
        t = d1 + d0 - 2 * s
        if inverse:
            dy = c["v"] - c["Y0"]
            qa, qb, qc = hk * (s - d0) + dy * t, hk * d0 - dy * t, -s * dy
            xi = 2 * qc / (-qb - np.sqrt(qb * qb - 4 * qa * qc))
            res = c["X0"] + xi * wk
        else:
            xi = (c["v"] - c["X0"]) / wk
        om = 1 - xi
        p = xi * om
        D = s + t * p
        if not inverse:
            res = c["Y0"] + hk * (s * xi * xi + d0 * p) / D
        ld = 2 * np.log(s) + np.log(d1 * xi * xi + 2 * s * p + d0 * om * om)
        if fault != "no_2logD":
            ld = ld - 2 * np.log(D)
        return np.where(c["inside"], res, v), np.where(c["inside"], ld, T(0))


def _spline_vjp(theta, K, B, T, a, gin, kap, usweep, fault=None):
    """The cotangents of a spline's inputs.  Parameter sweep: gin the cotangent of y, kap that of log f'; -> (that of a, that of theta).
    usweep (u = grad_z log q through the inverse layer a = f^-1(y), log q -= log f'(a)): gin the cotangent of a; with
    abar = gin - d log f'/da, theta receives -(abar / f') df/dtheta - d log f'/dtheta; -> (abar / f', that of y; that of theta)."""
    with np.errstate(all="ignore"):
        c = _setup(theta, K, B, T, a, False, fault)
        w, h, k, wk, hk, d0, d1 = c["w"], c["h"], c["k"], c["wk"], c["hk"], c["d0"], c["d1"]
        xi = (c["v"] - c["X0"]) / wk
        s = hk / wk
        om, m2 = 1 - xi, 1 - 2 * xi
        p = xi * om
        t = d1 + d0 - 2 * s
        D, N, Q = s + t * p, s * xi * xi + d0 * p, d1 * xi * xi + 2 * s * p + d0 * om * om
        hD2 = hk / (D * D)
        g_xi = (2 * d1 * xi + 2 * s * m2 - 2 * d0 * om) / Q - 2 * t * m2 / D
        g_s = 2 / s + 2 * p / Q - 2 * (1 - 2 * p) / D
        g_d0, g_d1 = om * om / Q - 2 * p / D, xi * xi / Q - 2 * p / D
        if fault == "no_2logD":
            g_xi, g_s, g_d0, g_d1 = g_xi + 2 * t * m2 / D, g_s + 2 * (1 - 2 * p) / D, g_d0 + 2 * p / D, g_d1 + 2 * p / D
        y_xi, y_s, y_d0, y_d1, y_h = hD2 * s * Q, hD2 * (xi * xi * D - N * (1 - 2 * p)), hD2 * p * (D - N), -hD2 * N * p, N / D
        if usweep:
            ret = (gin - g_xi / wk) / (s * s * Q / (D * D))
            gy, kap = -ret, -np.ones_like(gin)
        else:
            gy = gin
        c_xi, c_s, c_d0, c_d1 = gy * y_xi + kap * g_xi, gy * y_s + kap * g_s, gy * y_d0 + kap * g_d0, gy * y_d1 + kap * g_d1
        c_a = c_xi / wk
        if not usweep:
            ret = c_a
        c_wk, c_hk = -(c_xi * xi + c_s * s) / wk, gy * y_h + c_s / wk
        j, kk = np.arange(K)[None, :, None], k[:, None, :]
        zero = np.zeros_like(w)
        cw = np.where(j < kk, -c_a[:, None, :], np.where(j == kk, c_wk[:, None, :], zero))
        ch = np.where(j < kk, gy[:, None, :], np.where(j == kk, c_hk[:, None, :], zero))
        cuw = w * (cw - (cw * w).sum(axis=1, keepdims=True) / (T(2) * T(B)))
        cuh = h * (ch - (ch * h).sum(axis=1, keepdims=True) / (T(2) * T(B)))
        jd = np.arange(K - 1)[None, :, None]
        cd = np.where(jd == kk - 1, c_d0[:, None, :], zero[:, :K - 1]) + np.where(jd == kk, c_d1[:, None, :], zero[:, :K - 1])
        if fault == "edge_slope":   # an input in bin 0 (K - 1) sends nothing to the raw slope of knot 1 (K - 1)
            cd = np.where((kk == 0) | (kk == K - 1), zero[:, :K - 1], cd)
        cth = np.concatenate([cuw, cuh, cd * _sigmoid(c["ud"])], axis=1)
        ins = c["inside"]
        return np.where(ins, ret, gin), np.where(ins[:, None, :], cth, T(0))


def chunk_coords(K):
    """coordinates per chunk of the output layer, restated from csrc/kernels_nsf.hip: whole coordinates in one [64][16] block"""
    return 64 // (3 * K - 1)


def fault_block(arch):
    """the largest output-layer weight block of the layout (the first of them): where one_entry / one_row strike"""
    d, hidden, L, K, _ = arch
    lay = [e for e in nsf_layout(d, hidden, L, K)[0] if e[2] == "W" and e[1] == len(hidden) + 1]
    return max(lay, key=lambda e: (e[4][0] * e[4][1], -e[3]))


def _out_vjp(Wt, delta, P, cpc, mm, fault=None):
    """W_out' delta as the kernels form it: chunk after chunk of cpc coordinates (cpc P rows) into one accumulator, the rows of a chunk
    in groups of four from the chunk's first row.  Faults: acc_reset (the accumulator restarted at each chunk: the last chunk alone is
    left), stale_chunk_rows (a partial last chunk also takes the previous chunk's rows beyond its own, a second time)."""
    out = delta.shape[0]
    acc = np.zeros((Wt.shape[0], delta.shape[1]), dtype=delta.dtype)
    step = cpc * P
    for r0 in range(0, out, step):
        r1 = min(r0 + step, out)
        if fault == "acc_reset":
            acc = np.zeros_like(acc)
        acc = acc + mm(np.ascontiguousarray(Wt[:, r0:r1]), delta[r0:r1])
        if fault == "stale_chunk_rows" and r1 - r0 < step and r0 > 0:
            lo = r0 - step + (r1 - r0)
            acc = acc + mm(np.ascontiguousarray(Wt[:, lo:r0]), delta[lo:r0])
    return acc


def _backward_net(net, acts, delta, cols, mm, plan, out_vjp):
    """flow_ref._np_backward_net with the output layer's input VJP formed by `out_vjp` (the chunk walk)"""
    grads = []
    one = delta.dtype.type(1)
    for j in range(len(net) - 1, -1, -1):
        W = net[j][0]
        if plan is not None:
            dW, db = np.zeros(W.shape), np.zeros(W.shape[0])
            for tiles in plan:
                pW, pb = np.zeros(W.shape), np.zeros(W.shape[0])
                for c in tiles:
                    pW, pb = pW + mm(delta[:, c], np.ascontiguousarray(acts[j][:, c].T)).astype(np.float64), pb + delta[:, c].astype(np.float64).sum(axis=1)
                dW, db = dW + pW, db + pb
            grads = [dW.astype(delta.dtype), db.astype(delta.dtype)] + grads
        elif cols is not None:
            grads = [delta[:, cols] @ acts[j][:, cols].T, delta[:, cols].sum(axis=1)] + grads
        delta = out_vjp(np.ascontiguousarray(W.T), delta) if j == len(net) - 1 else mm(np.ascontiguousarray(W.T), delta)
        if j > 0:
            delta = delta * np.where(acts[j] > 0, one, W.dtype.type(0.01))
    return grads, delta


def evaluate(params, arch, G, ell, eps, kind, dtype=np.float64, fault=None, order=None, emulate=False, tile_sums=False):
    """dict(Z, logq, value, grad): the forward pass and the two backward sweeps with every step in `dtype`, G = grad_z ell and ell given.
    order: a permutation of the samples -- the parameter gradient and the value sum them in that order.
    emulate: the kernels' own order -- every product with its inner axis in groups of four (flow_ref._mm4), the output layer walked in
    chunks of chunk_coords(K) coordinates with its input VJP accumulated across the chunks (_out_vjp), the parameter gradient as tile
    partials of 16 samples added in float64 within a slice and then over the slices in slice order (flow_slices with the parameter
    count: the capped slice count), a sample's sum of log y', |eps|^2 and the value's terms in float64.
    tile_sums: the sums over the samples as the kernels are documented to form them, in the order given: 16 samples at a time in `dtype`,
    those partials and the value's terms added in float64 (the envelope's evaluations).
    A hidden pre-activation of exactly 0 (a dead unit) maps to 0 forward and takes the slope 0.01 backward, as the kernels do.
    fault: None or one of FAULTS --
        delta_ends          delta_0 = delta_K taken from softplus (of the neighbouring raw slope) instead of 1
        inverse_bin_on_X    (inverse_np) the inverse searches its bin on X
        no_2logD            the term -2 log D of log f' lost, in the value and in both sweeps
        lost_chunk          the last coordinate chunk of every output layer sends nothing back
        lost_tile           the last sample tile is missing from the parameter gradient and the value
        tails_not_identity  the edge bins' formulas carried on outside (-B, B)
        one_entry, one_row  entry (17, 23) / row 5 of the weight gradient of fault_block(arch) off by a relative 1e-3 / 1e-4
        edge_slope          the cotangent of the raw slope next to bin 0 / bin K - 1 lost for inputs in that bin
        stale_chunk_rows    a partial last chunk's input VJP also takes the previous chunk's rows beyond its own
        acc_reset           the input VJP of the output layer restarted at each chunk
        slice_cap           the tiles beyond the capped slice count are lost (the slices walk no second tile)
        B_unrounded         2B and the product with it taken in float64 inside an evaluation in `dtype`"""
    assert fault is None or fault in FAULTS, fault
    d, hidden, L, K, B = arch
    P, M = 3 * K - 1, eps.shape[1]
    T = np.dtype(dtype).type
    p = np.asarray(params).astype(dtype)
    nets = _nets(p, arch, lambda v, o, i: v.reshape((o, i), order="F"))
    eps, G, ell = np.asarray(eps).astype(dtype), np.asarray(G).astype(dtype), np.asarray(ell).astype(dtype)
    cols = np.arange(M) if order is None else np.asarray(order)
    if fault == "lost_tile":
        cols = cols[cols < TILE * ((M - 1) // TILE)]
    ns, tiles = R.flow_slices(M, p.shape[0]), (M + TILE - 1) // TILE
    if fault == "slice_cap":
        cols = cols[cols // TILE < ns]
    mm = R._mm4 if emulate else np.matmul
    cpc = chunk_coords(K)
    chunk_fault = fault if fault in ("acc_reset", "stale_chunk_rows") else None
    out_vjp = (lambda Wt, dl: _out_vjp(Wt, dl, P, cpc, mm, chunk_fault)) if (emulate or chunk_fault) else (lambda Wt, dl: mm(Wt, dl))
    plan = None
    if emulate:
        plan = [[np.arange(t * TILE, min(t * TILE + TILE, M)) for t in range(s, tiles, ns)] for s in range(ns)]
        if fault in ("lost_tile", "slice_cap"):
            keep = set(cols.tolist())
            plan = [[c for c in sl if c[0] in keep] for sl in plan]
    if tile_sums:
        plan = [[cols[i:i + TILE] for i in range(0, len(cols), TILE)]]
    xs, ldsum = [eps], np.zeros(M, dtype=np.float64 if emulate else dtype)
    for l in range(1, L + 1):
        A, Bm = masks(d, l)
        x = xs[-1]
        theta = R._np_forward_net(nets[l], x[Bm], T, False, mm)[0].reshape(len(A), P, M)
        y = x.copy()
        y[A], ld = _spline(theta, K, B, T, x[A], False, fault)
        xs.append(y)
        ldsum = ldsum + ld.sum(axis=0, dtype=ldsum.dtype)
    if emulate:
        logq = -0.5 * (eps.astype(np.float64) ** 2).sum(axis=0) - 0.5 * d * math.log(2.0 * math.pi) - ldsum
        value = T(((-ell.astype(np.float64) + logq)[cols]).sum() / M)
    else:
        logq = T(-0.5) * (eps * eps).sum(axis=0) - T(0.5 * d * math.log(2.0 * math.pi)) - ldsum
        value = T(((-ell + logq)[cols]).astype(np.float64).sum() / M) if tile_sums else ((-ell + logq)[cols]).sum() / T(M)

    def layer(l):
        A, Bm = masks(d, l)
        x = xs[l - 1]
        out, acts, _ = R._np_forward_net(nets[l], x[Bm], T, False, mm)
        return A, Bm, x, out.reshape(len(A), P, M), acts

    if kind == STL:   # u = grad_z log q(z), the parameters stopped: l = 1 .. L through the inverse layers
        xb = -eps
        for l in range(1, L + 1):
            A, Bm, x, theta, acts = layer(l)
            ret, cth = _spline_vjp(theta, K, B, T, x[A], xb[A], None, True, fault)
            _, cnet = _backward_net(nets[l], acts, cth.reshape(len(A) * P, M), None, mm, None, out_vjp)
            yb = xb.copy()
            yb[A] = ret
            yb[Bm] = xb[Bm] + cnet
            xb = yb
        g, kappa = (-G + xb) / T(M), T(0)
    else:
        g, kappa = -G / T(M), T(-1) / T(M)
    grad = np.zeros(p.shape[0], dtype=dtype)
    names = dict(blocks(arch))
    for l in range(L, 0, -1):
        A, Bm, x, theta, acts = layer(l)
        ret, cth = _spline_vjp(theta, K, B, T, x[A], g[A], np.full_like(g[A], kappa), False, fault)
        if fault == "lost_chunk":
            cth[((len(A) - 1) // cpc) * cpc:] = 0
        gr, cnet = _backward_net(nets[l], acts, cth.reshape(len(A) * P, M), cols, mm, plan, out_vjp)
        for j in range(len(hidden) + 1):
            grad[names[f"l{l}.W{j + 1}"]] = gr[2 * j].reshape(-1, order="F")
            grad[names[f"l{l}.b{j + 1}"]] = gr[2 * j + 1]
        gn = g.copy()
        gn[A] = ret
        gn[Bm] = g[Bm] + cnet
        g = gn
    if fault in ("one_entry", "one_row"):
        _, _, _, off, (no, ni) = fault_block(arch)
        hit = [off + min(17, no - 1) + no * min(23, ni - 1)] if fault == "one_entry" else off + min(5, no - 1) + no * np.arange(ni)
        grad[hit] = grad[hit] * (T(1) + T(1e-3 if fault == "one_entry" else 1e-4))
    return dict(Z=xs[-1], logq=logq, value=value, grad=grad)


def inverse_np(params, arch, Z, dtype=np.float64, fault=None):
    """(eps, log q) at the columns of Z through the inverse layers l = L .. 1 with every step in `dtype`"""
    d, hidden, L, K, B = arch
    T = np.dtype(dtype).type
    nets = _nets(np.asarray(params).astype(dtype), arch, lambda v, o, i: v.reshape((o, i), order="F"))
    y = np.asarray(Z).astype(dtype)
    ldsum = np.zeros(y.shape[1], dtype=dtype)
    for l in range(L, 0, -1):
        A, Bm = masks(d, l)
        theta = R._np_forward_net(nets[l], y[Bm], T, False)[0].reshape(len(A), 3 * K - 1, -1)
        x = y.copy()
        x[A], ld = _spline(theta, K, B, T, y[A], True, fault)
        y, ldsum = x, ldsum + ld.sum(axis=0)
    return y, T(-0.5) * (y * y).sum(axis=0) - T(0.5 * d * math.log(2.0 * math.pi)) - ldsum


wider = R.wider


def margin(params, arch, eps):
    """(knot, kink) over all layers, coordinates and samples, in float64:
    knot   the smallest distance of a spline input to a knot of its own spline or to +-B, relative to the width of the bin it lies in
           (outside (-B, B): relative to the mean bin width 2B / K)
    kink   the smallest |p| / (sum_j |W_ij| |a_j| + |b_i|) over the hidden pre-activations p, as flow_ref.margin computes it.  That
           condition does not carry the error of a layer's input and flow_ref states it for at most four layers; flow_ref.kink_room, which
           does, is written on RealNVP's nets.  The 32-layer case therefore rests on more than this margin: its float32 evaluation is
           compared layer by layer with the float64 one (no spline input changes its bin, tests/test_nsf_ref_host.py) and stays under
           half the factor under eight sample orders."""
    d, hidden, L, K, B = arch
    nets = _nets(np.asarray(params, dtype=np.float64), arch, lambda v, o, i: v.reshape((o, i), order="F"))
    x, knot, kink = np.asarray(eps, dtype=np.float64), np.inf, np.inf
    for l in range(1, L + 1):
        A, Bm = masks(d, l)
        h = x[Bm]
        for j, (W, b) in enumerate(nets[l]):
            pre = W @ h + b[:, None]
            if j < len(hidden):
                scale = np.abs(W) @ np.abs(h) + np.abs(b)[:, None]
                kink = min(kink, float(np.min(np.abs(pre) / np.maximum(scale, 1e-300))))
                h = np.where(pre > 0, pre, 0.01 * pre)
        theta = pre.reshape(len(A), 3 * K - 1, -1)
        a = x[A]
        c = _setup(theta, K, B, np.float64, a, False, None)
        dist = np.where(c["inside"], np.minimum(a - c["X0"], c["X0"] + c["wk"] - a) / c["wk"], np.minimum(np.abs(a - B), np.abs(a + B)) / (2 * B / K))
        knot = min(knot, float(dist.min()))
        y = x.copy()
        y[A], _ = _spline(theta, K, B, np.float64, a)
        x = y
    return knot, kink


def bin_changes(params, arch, eps, dtype):
    """(how many spline inputs of the forward pass in `dtype` lie in another bin, or on the other side of +-B, than in the wider dtype;
    the largest distance between the two passes' spline inputs, relative to the bin's width): what depth does to the knot margin"""
    d, hidden, L, K, B = arch
    runs = {}
    for t in (dtype, wider(dtype)):
        T = np.dtype(t).type
        nets = _nets(np.asarray(params).astype(t), arch, lambda v, o, i: v.reshape((o, i), order="F"))
        x, runs[t] = np.asarray(eps).astype(t), []
        for l in range(1, L + 1):
            A, Bm = masks(d, l)
            theta = R._np_forward_net(nets[l], x[Bm], T, False)[0].reshape(len(A), 3 * K - 1, -1)
            c = _setup(theta, K, B, T, x[A], False, None)
            runs[t].append((x[A], c["wk"], c["k"], c["inside"]))
            y = x.copy()
            y[A], _ = _spline(theta, K, B, T, x[A])
            x = y
    changed, far = 0, 0.0
    for (a, _, k, ins), (a2, w2, k2, ins2) in zip(runs[dtype], runs[wider(dtype)]):
        changed += int(((k != k2) | (ins != ins2)).sum())
        far = max(far, float(np.max(np.abs(a.astype(np.longdouble) - a2) / w2)))
    return changed, far


# ---- the criterion ----------------------------------------------------------------------------------------------------------------
TOL, STOL, violations = R.TOL, R.STOL, R.violations
# a rounding of a spline input or of a knot is a few u of |a| <= B + |tail| against bins of mean width 2B / K: below 1e-6 (2e-15) of a bin
# width over the four layers of the deepest many-sample case; the cases keep ten times that.  The kink condition is flow_ref's.
KNOT_MARGIN = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-11}
KINK_MARGIN = R.OLD_MARGIN


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.linalg.norm(a - b) / max(float(np.linalg.norm(b)), 1e-300))


def report(got, ref, yard, arch, dtype, factor=FACTOR):
    """[(name, error, bound)] of a result dict(grad, value[, Z, logq]) against the reference, `yard` being the evaluation in the context's
    dtype: Z and log q relative l2 / largest entry, the value, the whole gradient and every block (flow_ref.block_report's rule: the
    block's floor is its share of the whole-gradient allowance).  float64: the value and the gradient are held to the floors alone."""
    vt, gt = TOL[np.dtype(dtype)]
    st = STOL[np.dtype(dtype)]
    ld = np.longdouble
    yard = ref if yard is None else yard
    yard_vg = ref if np.dtype(dtype) == np.float64 else yard
    rows = []
    if "Z" in got:
        rows.append(("Z", _rel(got["Z"], ref["Z"]), max(st, factor * _rel(yard["Z"], ref["Z"]))))
    if "logq" in got:
        want = np.asarray(ref["logq"], dtype=ld)
        rows.append(("logq", float(np.abs(np.asarray(got["logq"], dtype=ld) - want).max()),
                     max(vt * float(np.abs(want).max()), factor * float(np.abs(np.asarray(yard["logq"], dtype=ld) - want).max()))))
    if "value" in got:
        rv = float(ref["value"])
        rows.append(("value", abs(float(got["value"]) - rv), max(vt * abs(rv), factor * abs(float(yard_vg["value"]) - rv))))
    if "grad" in got:
        g, r, y = (np.asarray(v, dtype=ld) for v in (got["grad"], ref["grad"], yard_vg["grad"]))
        n, gscale = r.shape[0], max(float(np.linalg.norm(r)), 1.0)
        rows.append(("all", float(np.linalg.norm(g - r)), max(gt * gscale, factor * float(np.linalg.norm(y - r)))))
        for name, sl in blocks(arch):
            floor = gt * max(float(np.linalg.norm(r[sl])), gscale * math.sqrt((sl.stop - sl.start) / n))
            rows.append((name, float(np.linalg.norm(g[sl] - r[sl])), max(floor, factor * float(np.linalg.norm(y[sl] - r[sl])))))
    return rows


def worst_ratios(rows):
    """{class: the largest error / bound} over the rows of `report`: Z, logq, value, all, W_out, b_out, W_hidden, b_hidden"""
    out = {}
    last = max(int(n.split(".")[1][1:]) for n, _, _ in rows if "." in n) if any("." in n for n, _, _ in rows) else 0
    for name, err, bound in rows:
        cls = name if "." not in name else name.split(".")[1][0] + ("_out" if int(name.split(".")[1][1:]) == last else "_hidden")
        out[cls] = max(out.get(cls, 0.0), err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
# (d, hidden, L, K, B, M) -> the seed of its parameters: the first one at which margin() clears KNOT_MARGIN and KINK_MARGIN on the float32
# AND on the float64 draws of estimate CASE_IDX (find_seed; tests/test_nsf_ref_host.py pins it).
CASE_IDX = R.CASE_IDX
CASES = {
    (2, (8,), 2, 2, 3.0, 4): 0,                # the minimum of everything
    (5, (8,), 3, 4, 3.0, 17): 0,               # unequal masks, a partial second tile
    (6, (16, 16), 2, 16, 3.0, 33): 0,          # the widest coordinate chunk: 47 rows, one coordinate at a time
    (127, (64, 64, 64), 2, 8, 3.0, 16): 22,    # the limits, odd d, many chunks
    (4, (8,), 32, 4, 3.0, 16): 1,              # depth
    (4, (8,), 2, 4, 0.5, 64): 0,               # most inputs in the identity tails
    (8, (16,), 4, 8, 30.0, 1040): 128,         # several tiles per slice
}
MID = (5, (8,), 3, 4, 3.0, 17)
DEEP_DAMP = 0.25


def arch_of(case):
    return case[:5]


def case_params(case, dtype, seed=None):
    """Glorot-uniform weights and N(0, 0.1^2) biases from the case's seed, rounded to dtype (flow_ref.case_params on this layout).
    Deeper than four layers the output-layer weights are x DEEP_DAMP, flow_ref's `damped` class: with plain Glorot weights a flow of 32
    layers is not conditioned (on the depth case the sticking-the-landing gradient has norm 5e4 .. 4e8 depending on the seed and the
    float32 evaluation's sample is off by 1.5e-5 relative l2; damped, 1e2 and 9e-7)."""
    d, hidden, L, K, B, _ = case
    seed = CASES[case] if seed is None else seed
    lay, n = nsf_layout(d, hidden, L, K)
    p, gen = np.zeros(n), np.random.default_rng(seed)
    for _, j, kind, off, shape in lay:
        if kind == "W":
            lim = math.sqrt(6.0 / (shape[0] + shape[1]))
            p[off:off + shape[0] * shape[1]] = gen.uniform(-lim, lim, size=shape[0] * shape[1])
            if L > 4 and j == len(hidden) + 1:
                p[off:off + shape[0] * shape[1]] *= DEEP_DAMP
    gen = np.random.default_rng(1000 + seed)
    for name, sl in blocks(arch_of(case)):
        if ".b" in name:
            p[sl] = 0.1 * gen.normal(size=sl.stop - sl.start)
    return p.astype(dtype)


def case_draws(case, dtype):
    from oracle import oracle as O
    from tests.helpers import SEED
    return O.philox_normal(SEED, CASE_IDX, case[0], 0, case[5], f64=np.dtype(dtype) == np.float64)


def margins_hold(case, seed=None):
    for t in (np.float32, np.float64):
        knot, kink = margin(case_params(case, t, seed), arch_of(case), case_draws(case, t))
        if not (knot >= KNOT_MARGIN[np.dtype(t)] and kink >= KINK_MARGIN[np.dtype(t)]):
            return False
    return True


def find_seed(case, limit=20000):
    """the first seed at which both margins hold on both dtypes' draws (how CASES was filled)"""
    return next((s for s in range(limit) if margins_hold(case, s)), None)


# ==== the per-entry criterion (tests/test_nsf_ref_host.py, tests/test_gpu_nsf_yardstick.py) ================================================
# tests/flow_ref.py's, on this family's layout: ref is `evaluate` in the next wider type, env per entry the largest distance of eight
# sample orders of `evaluate` in the element type from it, S the first-order magnitude, u = 2^-24 / 2^-53, and a result is held to
# F32_FACTOR x max(env, u S).  S is flow_ref's running error analysis (every quantity carries its error E in units of u beside its
# value; roundings add in quadrature, _q; the error of x^{l-1} enters layer l through the net's Jacobian per sample and through the
# spline) with the spline of include/mivi.h carried as follows --
#     softmax        e_j = exp(u_j - max): E = e_j (E_uj + E_max + |u_j - max| + 1), 0 at the maximum itself; sum: E = (E_e) + sum;
#                    w_j = 2B e_j / sum: E = w_j (E_e / e_j + E_sum / sum + 3)   (2B, the product, the quotient)
#     knots          X_0 = -B: E = B (the bound's own rounding);  X_k = X_{k-1} + w_k: E^2 = E_{k-1}^2 + E_w^2 + X_k^2 -- a running sum: the
#                    error grows with B + sum w and NOT with the width of the bin the input lies in
#     xi             (a - X_0) / w: E = (E_a + E_X0 + |a - X_0|) / w + xi E_w / w + xi -- the carried errors of a and of X_0 are divided
#                    by w: a narrow bin amplifies them
#     s = h / w, softplus (E = sigmoid E_u + 2 d), t, p = xi (1 - xi)
#     D, N, Q, y, log y', and every product of the VJP (g_*, y_*, c_*, the softmax's and the sigmoid's chain): the CARRIED errors of
#                    (xi, s, d_0, d_1) through the partial derivatives of each rational function (central differences in float64,
#                    relative step 1e-6: a magnitude needs two digits), the roundings made INSIDE each formula as the sum of the
#                    magnitudes of its terms.  D = s + t p cancels where t < 0: its own relative error rD = |terms| / D multiplies
#                    every quotient by D (twice where D^2 divides).
#     inverse        dy = y - Y_0, the discriminant qb^2 - 4 qa qc with its terms' magnitudes, the root, xi = 2 qc / (-qb - root); the
#                    carried errors of (dy, h, s, d_0, d_1) by differences as above
from tests.flow_ref import KINK_FACTOR, N_ORDERS, entry_ratio, orders, unit, value_ratio, _q  # noqa: E402,F401

KINK_ROOM = R.KINK_ROOM
SAMPLE_BLOCK = 32   # samples per pass of `magnitude`: the per-sample Jacobians of a 3008-row output layer are 1.5 MB each


def _rat(xi, s, d0, d1):
    """the rational functions of the spline in one bin, per unit of h where h multiplies"""
    om, m2 = 1 - xi, 1 - 2 * xi
    p = xi * om
    t = d1 + d0 - 2 * s
    D, N, Q = s + t * p, s * xi * xi + d0 * p, d1 * xi * xi + 2 * s * p + d0 * om * om
    D2 = D * D
    return dict(g_xi=(2 * d1 * xi + 2 * s * m2 - 2 * d0 * om) / Q - 2 * t * m2 / D, g_s=2 / s + 2 * p / Q - 2 * (1 - 2 * p) / D,
                g_d0=om * om / Q - 2 * p / D, g_d1=xi * xi / Q - 2 * p / D, yx=s * Q / D2, ys=(xi * xi * D - N * (1 - 2 * p)) / D2,
                yd0=p * (D - N) / D2, yd1=-N * p / D2, yh=N / D, fa=s * s * Q / D2, ld=2 * np.log(s) + np.log(Q) - 2 * np.log(D))


def _xi_inverse(dy, h, s, d0, d1):
    t = d1 + d0 - 2 * s
    qa, qb, qc = h * (s - d0) + dy * t, h * d0 - dy * t, -s * dy
    return dict(xi=2 * qc / (-qb - np.sqrt(qb * qb - 4 * qa * qc)))


def _carried(f, args, errs, rel=1e-6):
    """{name: sqrt(sum_i (d f / d arg_i x E_i)^2)}: the carried errors through f by central differences"""
    out = None
    for i, (a, E) in enumerate(zip(args, errs)):
        step = rel * np.maximum(np.abs(a), 1e-3)
        hi, lo = list(args), list(args)
        hi[i], lo[i] = a + step, a - step
        fh, fl = f(*hi), f(*lo)
        sq = {k: np.square((fh[k] - fl[k]) / (2 * step) * E) for k in fh}
        out = sq if out is None else {k: out[k] + sq[k] for k in sq}
    return {k: np.sqrt(v) for k, v in out.items()}


def _spline_analysis(theta, Eth, K, B, v, Ev, on_y=False):
    """One layer's splines at their inputs v (nA, M) with carried error Ev, raw outputs theta (nA, 3K - 1, M) with error Eth: dict of the
    values and errors the forward pass and the VJP need, `res` / `Eres` (y, or a for on_y: the inverse), `ld` / `Eld`, and `room`: per
    input its distance to either knot of its own bin (outside (-B, B): to +-B), absolute and divided by the S of that difference."""
    with np.errstate(all="ignore"):
        c = _setup(theta, K, B, np.float64, v, on_y, None)
        k, ins, vs = c["k"], c["inside"], c["v"]
        r2, r3 = math.sqrt(2.0), math.sqrt(3.0)

        def soft(u, Eu):
            mx = u.max(axis=1, keepdims=True)
            Emx = np.take_along_axis(Eu, u.argmax(axis=1)[:, None, :], axis=1)
            arg = u - mx
            e = np.exp(arg)
            Ee = np.where(arg == 0, 0.0, e * _q(Eu, Emx, arg, 1.0))
            sm = e.sum(axis=1, keepdims=True)
            Esm = _q(np.sqrt(np.sum(Ee * Ee, axis=1, keepdims=True)), sm)
            w = 2 * B * e / sm
            return w, w * _q(Ee / e, Esm / sm, r3), Esm / sm

        # (the error of the softmax's sum is COMMON to the bins of a spline: in a sum over bins it adds linearly, not in quadrature)
        w, Ew, cw_ = soft(theta[:, :K], Eth[:, :K])
        h, Eh, ch_ = soft(theta[:, K:2 * K], Eth[:, K:2 * K])
        ud, Eud = theta[:, 2 * K:], Eth[:, 2 * K:]
        sig, dl = _sigmoid(ud), _softplus(ud)
        Edl = _q(sig * Eud, r2 * dl)
        zero = np.zeros_like(w[:, :1])
        Edelta = np.concatenate([zero, Edl, zero], axis=1)

        def knots(wd, Ewd, common):
            Xk = np.cumsum(np.concatenate([-B + zero, wd], axis=1), axis=1)
            EX = np.sqrt(np.cumsum(np.concatenate([B * B + zero, Ewd * Ewd + np.square(Xk[:, 1:])], axis=1), axis=1) + np.square(common * (Xk + B)))
            return Xk, EX

        X, EX = knots(w, Ew, cw_)
        Y, EY = knots(h, Eh, ch_)
        wk, hk, d0, d1, X0, Y0 = c["wk"], c["hk"], c["d0"], c["d1"], c["X0"], c["Y0"]
        Ewk, Ehk, Ed0, Ed1, EX0, EY0 = _take(Ew, k), _take(Eh, k), _take(Edelta, k), _take(Edelta, k + 1), _take(EX, k), _take(EY, k)
        # the knot condition: the knots of the axis the bin was searched on; the outermost knots are +-B themselves (E = B)
        Kn, EKn = (Y, EY) if on_y else (X, EX)
        lo, Elo = _take(Kn, k), _take(EKn, k)
        hi, Ehi = np.where(k == K - 1, B, _take(Kn, k + 1)), np.where(k == K - 1, B, _take(EKn, k + 1))
        room_in = np.minimum((vs - lo) / _q(Ev, Elo), (hi - vs) / _q(Ev, Ehi))
        room = np.where(ins, room_in, np.minimum(np.abs(v - B), np.abs(v + B)) / _q(Ev, B))
        s = hk / wk
        Es = s * _q(Ehk / hk, Ewk / wk, 1.0)
        if on_y:
            dy = vs - Y0
            Edy = _q(Ev, EY0, dy)
            t = d1 + d0 - 2 * s
            tm = d1 + d0 + 2 * s
            qa, qb, qc = hk * (s - d0) + dy * t, hk * d0 - dy * t, -s * dy
            disc = qb * qb - 4 * qa * qc
            sq = np.sqrt(disc)
            den = -qb - sq
            xi = 2 * qc / den
            Mqa, Mqb = _q(hk * (s + d0) * r2, np.abs(dy) * tm * r2, qa), _q(hk * d0, np.abs(dy) * tm * r2, qb)
            Mdisc = _q(2 * np.abs(qb) * Mqb, 4 * np.abs(qc) * Mqa, 4 * np.abs(qa * qc) * r3, qb * qb, disc)
            Mden = _q(Mqb, Mdisc / (2 * sq), sq, den)
            Exi = _q(_carried(_xi_inverse, (dy, hk, s, d0, d1), (Edy, Ehk, Es, Ed0, Ed1))["xi"], np.abs(xi) * _q(Mden / np.abs(den), r2))
        else:
            num = vs - X0
            xi = num / wk
            Exi = _q(_q(Ev, EX0, num) / wk, xi * Ewk / wk, xi)
        om, m2 = 1 - xi, 1 - 2 * xi
        p = xi * om
        t, tm = d1 + d0 - 2 * s, d1 + d0 + 2 * s
        D, N, Q = s + t * p, s * xi * xi + d0 * p, d1 * xi * xi + 2 * s * p + d0 * om * om
        rD, rQ, rN = _q((d0 + d1) * p, np.abs(t) * p * r3, D) / D, 2.0, 2.0
        val = _rat(xi, s, d0, d1)
        car = _carried(_rat, (xi, s, d0, d1), (Exi, Es, Ed0, Ed1))
        Eyh = _q(car["yh"], val["yh"] * _q(rN, rD, 1.0))
        part = hk * val["yh"]
        if on_y:
            res = X0 + xi * wk
            Eres = _q(EX0, Exi * wk, xi * Ewk, xi * wk, res)
        else:
            res = Y0 + part
            Eres = _q(EY0, Ehk * val["yh"], hk * Eyh, part, res)
        ls, lQ, lD = np.log(s), np.log(Q), np.log(D)
        Eld = _q(car["ld"], 2 * ls, rQ, lQ, 2 * rD, 2 * lD, 2 * ls + lQ, val["ld"])
        out = dict(c, w=w, Ew=Ew, h=h, Eh=Eh, sig=sig, Eud=Eud, Ewk=Ewk, Ehk=Ehk, Ed0=Ed0, Ed1=Ed1, xi=xi, Exi=Exi, s=s, Es=Es, rD=rD, rQ=rQ,
                   val=val, car=car, Eyh=Eyh, D=D, N=N, Q=Q, p=p, tm=tm)
        out["res"], out["Eres"] = np.where(ins, res, v), np.where(ins, Eres, Ev)
        out["ld"], out["Eld"] = np.where(ins, val["ld"], 0.0), np.where(ins, Eld, 0.0)
        out["room"] = room
        return out


def _vjp_analysis(c, K, B, gin, Egin, kap, usweep):
    """_spline_vjp with errors, on the quantities of _spline_analysis (searched on X): -> (ret, E_ret, cth, E_cth)"""
    with np.errstate(all="ignore"):
        xi, s, d0, d1, wk, hk, k, ins = c["xi"], c["s"], c["d0"], c["d1"], c["wk"], c["hk"], c["k"], c["inside"]
        Exi, Es, Ed0, Ed1, Ewk, Ehk = c["Exi"], c["Es"], c["Ed0"], c["Ed1"], c["Ewk"], c["Ehk"]
        w, h, Ew, Eh = c["w"], c["h"], c["Ew"], c["Eh"]
        val, car, rD, rQ, D, N, Q, p, tm = c["val"], c["car"], c["rD"], c["rQ"], c["D"], c["N"], c["Q"], c["p"], c["tm"]
        om, m2 = 1 - xi, np.abs(1 - 2 * xi)
        r2, r3 = math.sqrt(2.0), math.sqrt(3.0)
        qQ, qD = _q(2.0, rQ), _q(2.0, rD)
        g = {n: val[n] for n in ("g_xi", "g_s", "g_d0", "g_d1")}
        Eg = dict(g_xi=_q(car["g_xi"], (2 * d1 * xi + 2 * s * m2 + 2 * d0 * om) / Q * qQ, 2 * tm * m2 / D * qD),
                  g_s=_q(car["g_s"], 2 / s, 2 * p / Q * qQ, 2 * (1 - 2 * p) / D * qD, g["g_s"]),
                  g_d0=_q(car["g_d0"], om * om / Q * qQ, 2 * p / D * qD, g["g_d0"]),
                  g_d1=_q(car["g_d1"], xi * xi / Q * qQ, 2 * p / D * qD, g["g_d1"]))
        hD2 = hk / (D * D)
        q3 = _q(3.0, 2 * rD)
        y = dict(xi=hk * val["yx"], s=hk * val["ys"], d0=hk * val["yd0"], d1=hk * val["yd1"], h=val["yh"])
        Ey = dict(xi=_q(hk * car["yx"], val["yx"] * Ehk, y["xi"] * _q(2 * rD, rQ, 2.0)),
                  s=_q(hk * car["ys"], val["ys"] * Ehk, hD2 * (xi * xi * D + N) * q3),
                  d0=_q(hk * car["yd0"], val["yd0"] * Ehk, hD2 * p * (D + N) * q3),
                  d1=_q(hk * car["yd1"], val["yd1"] * Ehk, y["d1"] * q3), h=c["Eyh"])
        if usweep:
            fa = val["fa"]
            Efa = _q(car["fa"], fa * _q(2.0, 2 * rD, rQ))
            gw = g["g_xi"] / wk
            inner = gin - gw
            ret = inner / fa
            Eret = _q(_q(Egin, Eg["g_xi"] / wk, gw * Ewk / wk, gw, inner) / fa, ret * Efa / fa, ret)
            gy, Egy, kap, Ekap = -ret, Eret, -np.ones_like(gin), 0.0
        else:
            gy, Egy, Ekap = gin, Egin, 1.0   # (kappa = -1 / M is a rounded quotient)
        cc, Ec = {}, {}
        for n in ("xi", "s", "d0", "d1"):
            a, b = gy * y[n], kap * g["g_" + n]
            cc[n] = a + b
            Ec[n] = _q(Egy * y[n], gy * Ey[n], a, kap * Eg["g_" + n], b * _q(Ekap, 1.0), cc[n])
        c_a = cc["xi"] / wk
        Eca = _q(Ec["xi"] / wk, c_a * Ewk / wk, c_a)
        if not usweep:
            ret, Eret = c_a, Eca
        sm = cc["xi"] * xi + cc["s"] * s
        c_wk = -sm / wk
        Ecwk = _q(_q(Ec["xi"] * xi, cc["xi"] * Exi, cc["xi"] * xi, Ec["s"] * s, cc["s"] * Es, cc["s"] * s, sm) / wk, c_wk * _q(Ewk / wk, 1.0))
        a, b = gy * y["h"], cc["s"] / wk
        c_hk = a + b
        Echk = _q(Egy * y["h"], gy * Ey["h"], a, Ec["s"] / wk, b * _q(Ewk / wk, 1.0), c_hk)
        j, kk = np.arange(K)[None, :, None], k[:, None, :]

        def chain(wd, Ewd, left, Eleft, own, Eown):
            """the softmax's chain rule: c_u_j = w_j (c_w_j - sum_i c_w_i w_i / 2B)"""
            cw = np.where(j < kk, left[:, None, :], np.where(j == kk, own[:, None, :], 0.0))
            Ecw = np.where(j < kk, Eleft[:, None, :], np.where(j == kk, Eown[:, None, :], 0.0))
            terms = cw * wd
            dot = terms.sum(axis=1, keepdims=True) / (2 * B)
            # c_w_j is ONE number (-c_a, or gy) for every j < k and the w_j share their sum's error: both add linearly over j
            Edot = _q(np.abs(Ecw * wd).sum(axis=1, keepdims=True), np.abs(cw * Ewd).sum(axis=1, keepdims=True),
                      r3 * np.abs(terms).sum(axis=1, keepdims=True)) / (2 * B)
            diff = cw - dot
            return wd * diff, _q(Ewd * diff, wd * _q(Ecw, Edot, diff), wd * diff)

        cuw, Ecuw = chain(w, Ew, -c_a, Eca, c_wk, Ecwk)
        cuh, Ecuh = chain(h, Eh, gy, Egy, c_hk, Echk)
        jd = np.arange(K - 1)[None, :, None]
        cd = np.where(jd == kk - 1, cc["d0"][:, None, :], 0.0) + np.where(jd == kk, cc["d1"][:, None, :], 0.0)
        Ecd = np.where(jd == kk - 1, Ec["d0"][:, None, :], 0.0) + np.where(jd == kk, Ec["d1"][:, None, :], 0.0)
        sig = c["sig"]
        cds = cd * sig
        Ecds = _q(Ecd * sig, cd * sig * (1 - sig) * c["Eud"], r3 * cds)
        cth, Ecth = np.concatenate([cuw, cuh, cds], axis=1), np.concatenate([Ecuw, Ecuh, Ecds], axis=1)
        return np.where(ins, ret, gin), np.where(ins, Eret, Egin), np.where(ins[:, None, :], cth, 0.0), np.where(ins[:, None, :], Ecth, 0.0)


def _j_fwd(J, E2):
    """sum_i J[m, o, i]^2 E2[i, m] -> (o, m); a Jacobian shared by all samples has a first axis of 1"""
    return (J[0] * J[0]) @ E2 if J.shape[0] == 1 else np.einsum("moi,im->om", J * J, E2)


def _j_back(J, E2):
    """sum_o J[m, o, i]^2 E2[o, m] -> (i, m)"""
    return (J[0] * J[0]).T @ E2 if J.shape[0] == 1 else np.einsum("moi,om->im", J * J, E2)


def _net_analysis(net, h0, E0):
    """flow_ref._net_analysis without the identity block of the output layer (up to 3008 x 3008 here): Jsuf[-1] is None and means I.
    Where every sample of the block has the same leakyrelu branches (always in the class `open`) the Jacobians are formed once, with a
    first axis of 1, instead of per sample."""
    M = h0.shape[1]
    h, Eloc, J = h0, np.zeros_like(h0), None
    acts, hidden, slopes, shared = [(h0, E0)], [], [], True
    for j, (W, b) in enumerate(net):
        W2 = W * W
        pre = W @ h + b[:, None]
        Eloc_pre = np.sqrt(W2 @ (Eloc * Eloc) + W2 @ (h * h) + (b * b)[:, None])
        if J is None:
            Jpre = W[None]
        else:   # W J_m for every sample m as ONE product (a broadcast batched product is not handed to the BLAS)
            Jpre = np.ascontiguousarray((W @ J.transpose(1, 0, 2).reshape(J.shape[1], -1)).reshape(W.shape[0], J.shape[0], -1).transpose(1, 0, 2))
        Epre = _q(Eloc_pre, np.sqrt(_j_fwd(Jpre, E0 * E0)))
        if j < len(net) - 1:
            slope = np.where(pre > 0, 1.0, 0.01)
            h_new = slope * pre
            own = np.where(pre > 0, 0.0, np.abs(h_new))
            hidden.append((pre, Epre, np.abs(W) @ np.abs(h) + np.abs(b)[:, None]))
            shared = shared and bool(np.all(slope == slope[:, :1]))
            h, Eloc, J = h_new, _q(slope * Eloc_pre, own), (slope[:, :1] if shared else slope).T[:, :, None] * Jpre
            acts.append((h, _q(slope * Epre, own)))
            slopes.append(slope)
    Jsuf = [None] * len(net)
    for j in range(len(net) - 2, -1, -1):
        Wn = net[j + 1][0]
        nxt = Wn[None] if Jsuf[j + 1] is None else (Jsuf[j + 1].reshape(-1, Wn.shape[0]) @ Wn).reshape(Jsuf[j + 1].shape[0], -1, Wn.shape[1])
        Jsuf[j] = nxt * (slopes[j][:, :1] if shared else slopes[j]).T[:, None, :]
    return dict(pre=pre, Epre=Epre, acts=acts, hidden=hidden, slopes=slopes, Jnet=Jpre, Jsuf=Jsuf)


def _net_back(net, an, dlt, Ed, want):
    """flow_ref._net_back, the parameter gradient's S in two pieces that add over sample blocks: ([(sum of squares, sum of |terms|) of
    dW_1, db_1, ...] if want, the input's cotangent, its error); S = sqrt(squares + |terms|^2)"""
    grads, d, Eloc, Ed2 = [], dlt, np.zeros_like(dlt), Ed * Ed
    for j in range(len(net) - 1, -1, -1):
        W, (h, Eh) = net[j][0], an["acts"][j]
        if want:
            Ej2 = Ed2 if an["Jsuf"][j] is None else Eloc * Eloc + _j_back(an["Jsuf"][j], Ed2)
            da = np.abs(d)
            grads = [(Ej2 @ (h * h).T + (d * d) @ (Eh * Eh).T, da @ np.abs(h).T), (Ej2.sum(axis=1), da.sum(axis=1))] + grads
        d, Eloc = W.T @ d, np.sqrt((W * W).T @ (Eloc * Eloc) + (W * W).T @ (d * d))
        if j > 0:
            d, Eloc = d * an["slopes"][j - 1], Eloc * an["slopes"][j - 1]
    return grads, d, _q(Eloc, np.sqrt(_j_back(an["Jnet"], Ed2)))


def _magnitude_block(nets, arch, tgt, E, kind, M, n_params):
    """`magnitude` on a block of samples (columns of E); the sums over the samples are returned as pieces that add over the blocks"""
    d, hidden, L, K, B = arch
    P, Mb = 3 * K - 1, E.shape[1]
    c0 = 0.5 * d * math.log(2.0 * math.pi)
    xs, Exs, El2, Sa, kink, old, worst, knot, fwd = [E], [np.zeros_like(E)], np.zeros(Mb), np.zeros(Mb), np.inf, np.inf, 0.0, np.inf, {}
    hits = np.zeros(K + 1, dtype=np.int64)   # spline inputs per bin; the last entry: in the tails
    for l in range(1, L + 1):
        A, Bm = masks(d, l)
        x, Ex = xs[-1], Exs[-1]
        an = _net_analysis(nets[l], x[Bm], Ex[Bm])
        for pre, Spre, scale in an["hidden"]:
            live = Spre > 0
            if np.any(live):
                kink = min(kink, float(np.min(np.abs(pre[live]) / Spre[live])))
                old = min(old, float(np.min(np.abs(pre[live]) / scale[live])))
                worst = max(worst, float(np.max(Spre[live] / scale[live])))
        sp = _spline_analysis(an["pre"].reshape(len(A), P, Mb), an["Epre"].reshape(len(A), P, Mb), K, B, x[A], Ex[A])
        fwd[l] = (an, sp)
        knot = min(knot, float(sp["room"].min()))
        hits += np.bincount(np.where(sp["inside"], sp["k"], K).ravel(), minlength=K + 1)
        y, Ey = x.copy(), Ex.copy()
        y[A], Ey[A] = sp["res"], sp["Eres"]
        xs.append(y)
        Exs.append(Ey)
        El2, Sa = El2 + np.square(sp["Eld"]).sum(axis=0), Sa + sp["ld"].sum(axis=0)
    Z, EZ = xs[-1], Exs[-1]
    lq = -0.5 * (E * E).sum(axis=0) - c0 - Sa
    S_logq = np.sqrt(0.25 * (E ** 4).sum(axis=0) + El2 + lq * lq)
    out = dict(Z=EZ, logq=S_logq, kink=kink, old_margin=old, S_over_scale=worst, knot=knot, hits=hits)
    if tgt is None:
        return out
    from tests import meanfield_ref as Mf
    ell, G = target_columns(tgt, Z)
    ell_a, Ga = Mf._magnitude_target(tgt, np.abs(Z) + EZ, Z, d)
    if kind == STL:
        xb, Eb = -E, np.zeros_like(E)
        for l in range(1, L + 1):
            A, Bm = masks(d, l)
            an, sp = fwd[l]
            ret, Eret, cth, Ecth = _vjp_analysis(sp, K, B, xb[A], Eb[A], None, True)
            _, cn, Ecn = _net_back(nets[l], an, cth.reshape(len(A) * P, Mb), Ecth.reshape(len(A) * P, Mb), False)
            yb, En = xb.copy(), Eb.copy()
            yb[A], En[A] = ret, Eret
            yb[Bm] = xb[Bm] + cn
            En[Bm] = _q(Eb[Bm], Ecn, yb[Bm])
            xb, Eb = yb, En
        g, Eg, kappa = (-G + xb) / M, _q(Ga, Eb, -G + xb) / M, 0.0
    else:
        g, Eg, kappa = -G / M, Ga / M, -1.0 / M
    sq, lin = np.zeros(n_params), np.zeros(n_params)
    names = dict(blocks(arch))
    for l in range(L, 0, -1):
        A, Bm = masks(d, l)
        an, sp = fwd[l]
        ret, Eret, cth, Ecth = _vjp_analysis(sp, K, B, g[A], Eg[A], np.full_like(g[A], kappa), False)
        gr, cn, Ecn = _net_back(nets[l], an, cth.reshape(len(A) * P, Mb), Ecth.reshape(len(A) * P, Mb), True)
        for j in range(len(hidden) + 1):
            sq[names[f"l{l}.W{j + 1}"]], lin[names[f"l{l}.W{j + 1}"]] = gr[2 * j][0].reshape(-1, order="F"), gr[2 * j][1].reshape(-1, order="F")
            sq[names[f"l{l}.b{j + 1}"]], lin[names[f"l{l}.b{j + 1}"]] = gr[2 * j + 1]
        gn, En = g.copy(), Eg.copy()
        gn[A], En[A] = ret, Eret
        gn[Bm] = g[Bm] + cn
        En[Bm] = _q(Eg[Bm], Ecn, gn[Bm])
        g, Eg = gn, En
    out.update(sq=sq, lin=lin, v_sq=float(np.sum(ell_a * ell_a + S_logq * S_logq)), v_lin=float(np.sum(np.abs(-ell + lq))))
    return out


def magnitude(params, arch, tgt, eps, kind, Zin=None, EZin=None):
    """dict(Z (d x M), logq (M), value, grad, knot, kink, old_margin, S_over_scale, hits), float64: S of every output entry (the comment
    above).  knot: the smallest distance of a spline input to either knot of its own bin, or to +-B outside (-B, B), absolute and divided
    by the S of that difference; kink, old_margin, S_over_scale: flow_ref.magnitude's, on the hidden pre-activations; hits: how many
    spline inputs each bin 0 .. K - 1 received over the layers, and (last) how many lay in the tails.  tgt None: the forward quantities.
    Zin: S (n) of log q at the columns of Zin through the inverse layers instead (dict(logq, knot): the knots are those of Y there);
    EZin: the error the points themselves carry (none: they are stored values)."""
    d, hidden, L, K, B = arch
    p = np.asarray(params, dtype=np.float64)
    nets = _nets(p, arch, lambda v, o, i: v.reshape((o, i), order="F"))
    P = 3 * K - 1
    if Zin is not None:
        Zin = np.asarray(Zin, dtype=np.float64)
        EZ = np.zeros_like(Zin) if EZin is None else np.asarray(EZin, dtype=np.float64)
        S, knot = np.zeros(Zin.shape[1]), np.inf
        for b0 in range(0, Zin.shape[1], SAMPLE_BLOCK):
            y, Ey = Zin[:, b0:b0 + SAMPLE_BLOCK], EZ[:, b0:b0 + SAMPLE_BLOCK]
            El2, Sa = np.zeros(y.shape[1]), np.zeros(y.shape[1])
            for l in range(L, 0, -1):
                A, Bm = masks(d, l)
                an = _net_analysis(nets[l], y[Bm], Ey[Bm])
                sp = _spline_analysis(an["pre"].reshape(len(A), P, -1), an["Epre"].reshape(len(A), P, -1), K, B, y[A], Ey[A], on_y=True)
                knot = min(knot, float(sp["room"].min()))
                x, Ex = y.copy(), Ey.copy()
                x[A], Ex[A] = sp["res"], sp["Eres"]
                y, Ey, El2, Sa = x, Ex, El2 + np.square(sp["Eld"]).sum(axis=0), Sa + sp["ld"].sum(axis=0)
            lq = -0.5 * (y * y).sum(axis=0) - 0.5 * d * math.log(2.0 * math.pi) - Sa
            S[b0:b0 + SAMPLE_BLOCK] = np.sqrt(np.sum(np.square(y * Ey) + 0.25 * y ** 4, axis=0) + El2 + lq * lq)
        return dict(logq=S, knot=knot)
    E = np.asarray(eps, dtype=np.float64)
    M = E.shape[1]
    parts = [_magnitude_block(nets, arch, tgt, E[:, b0:b0 + SAMPLE_BLOCK], kind, M, p.shape[0]) for b0 in range(0, M, SAMPLE_BLOCK)]
    out = dict(Z=np.concatenate([q["Z"] for q in parts], axis=1), logq=np.concatenate([q["logq"] for q in parts]),
               kink=min(q["kink"] for q in parts), old_margin=min(q["old_margin"] for q in parts), knot=min(q["knot"] for q in parts),
               S_over_scale=max(q["S_over_scale"] for q in parts), hits=sum(q["hits"] for q in parts))
    if tgt is not None:
        out["grad"] = np.sqrt(sum(q["sq"] for q in parts) + np.square(sum(q["lin"] for q in parts)))
        out["value"] = float(_q(math.sqrt(sum(q["v_sq"] for q in parts)) / M, sum(q["v_lin"] for q in parts) / M))
    return out


def knot_room(params, arch, eps, dtype, m=None):
    """How many times over the spline inputs meet the knot condition (>= 1: met): |a - knot| >= KINK_FACTOR x u x S of that difference
    (`magnitude`: the carried error of a and the knot's running sum), AND the earlier KNOT_MARGIN of the bin's width (`margin`) --
    whichever is stronger."""
    m = magnitude(params, arch, None, eps, None) if m is None else m
    return min(m["knot"] / (KINK_FACTOR * unit(dtype)), margin(params, arch, eps)[0] / KNOT_MARGIN[np.dtype(dtype)])


def kink_room(params, arch, eps, dtype, m=None):
    """flow_ref.kink_room's rule on this family's nets"""
    m = magnitude(params, arch, None, eps, None) if m is None else m
    if not np.isfinite(m["kink"]):
        return np.inf
    return min(m["kink"] / (KINK_FACTOR * unit(dtype)), m["old_margin"] / R.OLD_MARGIN[np.dtype(dtype)])


def envelope(params, arch, G, ell, eps, kind, dtype=np.float32, ref=None, which=None):
    """dict(Z, logq, value, grad): per entry max_k |evaluate(dtype, order_k) - ref| over orders(M, n_params) (Z and log q do not depend on
    the order).  which: the indices into orders(...) to use (the reduced envelope of the `open` case: the identity and the kernels')."""
    wide = wider(dtype)
    ref = evaluate(params, arch, G, ell, eps, kind, wide) if ref is None else ref
    env = None
    os_ = orders(np.asarray(eps).shape[1], len(params))
    for o in (os_ if which is None else [os_[i] for i in which if i < len(os_)]):
        y = evaluate(params, arch, G, ell, eps, kind, dtype, order=o, tile_sums=True)
        dist = {k: np.abs(np.asarray(y[k]).astype(wide) - ref[k]) for k in ("Z", "logq", "value", "grad")}
        env = dist if env is None else {k: np.maximum(env[k], dist[k]) for k in dist}
    return env


def criterion(params, arch, tgt, eps, kind, dtype, which=None):
    """dict(ref, yard, env, S, G, ell) of one estimate, as flow_ref.criterion"""
    eps = np.asarray(eps)
    zeros = np.zeros(eps.shape)
    Z = evaluate(params, arch, zeros, zeros[0], eps, MONTE_CARLO, np.float64)["Z"]
    ell, G = target_columns(tgt, Z)
    ref = evaluate(params, arch, G, ell, eps, kind, wider(dtype))
    return dict(ref=ref, yard=evaluate(params, arch, G, ell, eps, kind, dtype), G=G, ell=ell,
                env=envelope(params, arch, G, ell, eps, kind, dtype, ref, which), S=magnitude(params, arch, tgt, eps, kind))


def _norm(a):
    return np.sqrt(np.sum(a * a))


def ratios(got, env, ref, S_mag, arch, u, extra=None):
    """dict(whole, row, group, entry) of a flat gradient, every number ||got - ref|| / (max(||env||, u ||S||) + ||extra||) over a set of
    entries: each entry; each row of each W_j and each whole b_j; for the output layer also each coordinate group (the 3K - 1 rows of one
    coordinate of W_out with their 3K - 1 biases); the whole gradient.  extra: flow_ref.ratios'."""
    d, hidden, L, K, _ = arch
    P = 3 * K - 1
    ld = np.longdouble
    err = np.abs(np.asarray(got).astype(ld) - np.asarray(ref).astype(ld))
    en, fl = np.asarray(env).astype(ld), ld(u) * np.asarray(S_mag).astype(ld)
    ex = np.zeros(err.size, dtype=ld) if extra is None else np.asarray(extra).astype(ld)
    tiny = ld(np.finfo(np.float64).tiny)
    over = lambda sl: float(_norm(err[sl]) / (max(_norm(en[sl]), _norm(fl[sl])) + _norm(ex[sl]) + tiny))   # noqa: E731
    row, group = 0.0, 0.0
    lay = nsf_layout(d, hidden, L, K)[0]
    for (l, j, _, off, shape), (_, _, _, boff, _) in zip(lay[0::2], lay[1::2]):
        row = max(row, over(slice(boff, boff + shape[0])))
        n = shape[0] * shape[1]
        sq = lambda a: np.sum((a[off:off + n] ** 2).reshape(shape[1], shape[0]), axis=0)   # noqa: E731  (vec W is column-major: row i is off + i, off + i + out, ...)
        e2, n2, f2, x2 = sq(err), sq(en), sq(fl), sq(ex)
        row = max(row, float(np.max(np.sqrt(e2) / (np.maximum(np.sqrt(n2), np.sqrt(f2)) + np.sqrt(x2) + tiny))))
        if j == len(hidden) + 1:
            b2 = lambda a: (a[boff:boff + shape[0]] ** 2)   # noqa: E731
            grp = lambda w2, a: (w2 + b2(a)).reshape(-1, P).sum(axis=1)   # noqa: E731
            ge, gn, gf, gx = grp(e2, err), grp(n2, en), grp(f2, fl), grp(x2, ex)
            group = max(group, float(np.max(np.sqrt(ge) / (np.maximum(np.sqrt(gn), np.sqrt(gf)) + np.sqrt(gx) + tiny))))
    return dict(whole=over(slice(0, err.size)), row=row, group=group, entry=float(np.max(err / (np.maximum(en, fl) + ex + tiny))))


def all_ratios(got, crit, arch, dtype, extra=None):
    """dict(whole, row, group, entry, value, Z, logq) of a result dict(grad, value[, Z, logq]) against criterion(...)"""
    u, ref, env, S = unit(dtype), crit["ref"], crit["env"], crit["S"]
    out = ratios(got["grad"], env["grad"], ref["grad"], S["grad"], arch, u, extra)
    out["value"] = value_ratio(got["value"], env["value"], ref["value"], S["value"], u)
    for k in ("Z", "logq"):
        if k in got:
            out[k] = entry_ratio(got[k], ref[k], S[k], u, env[k])
    return out


# ---- the cases of the per-entry criterion ---------------------------------------------------------------------------------------------------
# (d, hidden, L, K, B, M, class) -> the seed of its parameters: the first at which knot_room() >= 1 and kink_room() >= KINK_ROOM on the
# float32 AND on the float64 draws of estimate CASE_IDX (find_seed; tests/test_nsf_ref_host.py pins both rooms >= 1).  Classes (yard_params):
#     default   case_params: Glorot weights, biases N(0, 0.1^2)
#     damped    deeper than four layers: the output-layer weights x DEEP_DAMP (case_params does it)
#     peaked    the output layer's biases of the width and of the height rows are the ramp -4 .. 4 over the K bins (the softmax spans
#               e^+-4 within a spline) and those of the slope rows alternate +4, -4 (softplus: 4.02 and 0.018)
#     dead      hidden unit DEAD_UNIT of the first hidden layer of layer 1 and of the last hidden layer of layer L: incoming row and bias
#               exactly 0, the outgoing column not
#     open      the hidden biases + 4: every leakyrelu on its positive branch (where M is too large for any seed to clear the kinks)
#     flat      the output layer's W and b exactly 0: every bin 2B / K wide and high, every slope softplus(0); with K and B powers of two
#               every knot is a dyadic number (the knots-hit-exactly cases)
# What each shape reaches is in the module docstring of tests/test_gpu_nsf_yardstick.py.
DEAD_UNIT = 2
OPEN_CASE = (128, (64,), 6, 16, 3.0, 449, "open")
YARD_CASES = {
    (2, (8,), 2, 2, 3.0, 33, "default"): 0,
    (18, (8,), 2, 3, 3.0, 17, "default"): 0,
    (16, (16,), 2, 7, 3.0, 33, "default"): 0,
    (6, (16,), 2, 11, 3.0, 33, "default"): 0,
    (4, (8,), 2, 12, 3.0, 17, "default"): 0,
    (6, (16, 16), 2, 16, 1.0, 33, "default"): 0,
    (5, (8,), 3, 4, 2.7, 17, "default"): 0,
    (5, (8,), 3, 4, 3.0, 17, "peaked"): 0,
    (5, (8,), 3, 4, 3.0, 17, "dead"): 0,
    (5, (8,), 2, 4, 3.0, 1040, "default"): 4,
    (6, (4,), 1, 8, 3.0, 2049, "default"): 0,
    (4, (8,), 32, 4, 3.0, 16, "damped"): 7,
    (128, (64, 64, 64), 32, 16, 3.0, 1, "damped"): 83,
    (127, (64,), 2, 16, 3.0, 2, "default"): 1635,
    OPEN_CASE: 60,
}
MANY_TILES = [c for c in YARD_CASES if c[5] > 64 * TILE]
SLICE_CAPPED = [(128, (64, 64, 64), 32, 16, 3.0, 1, "damped"), OPEN_CASE]
FLAT_CASES = [(4, (8,), 2, 4, 2.0, 0, "flat"), (4, (8,), 2, 16, 4.0, 0, "flat")]


# Two cases cannot have every bin hit, whatever the seed: a seed moves the parameters, never the draws, and with L <= 2 (or on the first
# visit of a coordinate) the spline inputs ARE the draws.
#   K = 12, M = 17   the 68 draws of estimate CASE_IDX span [-2.03, 2.53]: bin 0 is [-3, -2.5] up to the softmax's +-0.3 and no input
#                    reaches it; the bins 1 .. 11 are asked for
#   peaked           a monotone ramp of -4 .. 4 leaves the three narrowest of four bins 0.002, 0.027 and 0.39 wide at one END of
#                    [-3, 3], where N(0, 1) draws have a density of 0.004: the two widest bins are asked for
# -> the bins (indices) that must receive an input
BINS_OUT_OF_REACH = {(4, (8,), 2, 12, 3.0, 17, "default"): np.arange(1, 12), (5, (8,), 3, 4, 3.0, 17, "peaked"): np.arange(2, 4)}


def yard_dtypes(case):
    """the open case has no float64 context: its long-double evaluation alone takes half a minute"""
    return (np.float32,) if case[6] == "open" else (np.float32, np.float64)


def dead_units(case):
    """[(layer, hidden layer j (1-based), unit)] of the class `dead`"""
    d, hidden, L = case[:3]
    return [(1, 1, DEAD_UNIT), (L, len(hidden), DEAD_UNIT)] if case[6] == "dead" else []


def yard_params(case, dtype, seed=None):
    """the parameters of a YARD_CASES entry (or of FLAT_CASES), rounded to dtype"""
    d, hidden, L, K, B, M, cls = case
    seed = YARD_CASES.get(case, 0) if seed is None else seed
    p = case_params(case[:6], np.float64, seed)
    H, P = len(hidden), 3 * K - 1
    for l, j, kind, off, shape in nsf_layout(d, hidden, L, K)[0]:
        n = int(np.prod(shape))
        if j == H + 1 and cls == "flat":
            p[off:off + n] = 0.0
        if j == H + 1 and cls == "peaked" and kind == "b":
            b = p[off:off + n].reshape(-1, P)
            b[:, :K] = b[:, K:2 * K] = np.linspace(-4.0, 4.0, K)
            b[:, 2 * K:] = np.where(np.arange(K - 1) % 2 == 0, 4.0, -4.0)
        if j <= H and cls == "open" and kind == "b":
            p[off:off + n] += 4.0
        for dl, dj, unit_ in dead_units(case):
            if (l, j) == (dl, dj):
                if kind == "W":
                    p[off + unit_:off + n:shape[0]] = 0.0
                else:
                    p[off + unit_] = 0.0
    return p.astype(dtype)


def dead_rows(case):
    """the indices of the gradient entries of the dead units' incoming weights"""
    d, hidden, L, K = case[:4]
    out = []
    for l, j, kind, off, shape in nsf_layout(d, hidden, L, K)[0]:
        for dl, dj, unit_ in dead_units(case):
            if (l, j, kind) == (dl, dj, "W"):
                out.extend(range(off + unit_, off + shape[0] * shape[1], shape[0]))
    return np.array(out, dtype=np.int64)


def edge_slope_entries(case):
    """{(l, coordinate i, "lo" | "hi"): index of the b_out entry of the raw slope beside bin 0 / bin K - 1}"""
    d, hidden, L, K = case[:4]
    P, out = 3 * K - 1, {}
    for l, j, kind, off, shape in nsf_layout(d, hidden, L, K)[0]:
        if j == len(hidden) + 1 and kind == "b":
            for i in range(shape[0] // P):
                out[(l, i, "lo")], out[(l, i, "hi")] = off + i * P + 2 * K, off + i * P + 3 * K - 2
    return out


def slope_hits(params, arch, eps):
    """{(l, i, knot j = 1 .. K - 1): how many inside spline inputs lie in a bin beside knot j}: float64 forward pass"""
    d, hidden, L, K, B = arch
    nets = _nets(np.asarray(params, dtype=np.float64), arch, lambda v, o, i: v.reshape((o, i), order="F"))
    x, out = np.asarray(eps, dtype=np.float64), {}
    for l in range(1, L + 1):
        A, Bm = masks(d, l)
        theta = R._np_forward_net(nets[l], x[Bm], np.float64, False)[0].reshape(len(A), 3 * K - 1, -1)
        c = _setup(theta, K, B, np.float64, x[A], False, None)
        for i in range(len(A)):
            ks = c["k"][i][c["inside"][i]]
            for j in range(1, K):
                out[(l, i, j)] = int(np.sum((ks == j - 1) | (ks == j)))
        y = x.copy()
        y[A], _ = _spline(theta, K, B, np.float64, x[A])
        x = y
    return out


def yard_draws(case, dtype):
    from oracle import oracle as O
    from tests.helpers import SEED
    return O.philox_normal(SEED, CASE_IDX, case[0], 0, case[5], f64=np.dtype(dtype) == np.float64).astype(dtype)   # (stored values, as the device's are)


def rooms(case, dtype, seed=None):
    """(knot_room, kink_room, hits) of a case on the draws of `dtype`"""
    p, eps, arch = yard_params(case, dtype, seed), yard_draws(case, dtype), case[:5]
    m = magnitude(p, arch, None, eps, None)
    return knot_room(p, arch, eps, dtype, m), kink_room(p, arch, eps, dtype, m), m["hits"]


def bins_hit(case, hits):
    """the condition of section 2 on the bins: every bin hit in the default / peaked / dead classes, the edge bins twice at K = 2 and at
    K = 16, B = 1"""
    K, B, cls = case[3], case[4], case[6]
    if case in BINS_OUT_OF_REACH:
        return bool(np.all(hits[:K][BINS_OUT_OF_REACH[case]] >= 1))
    ok = cls not in ("default", "peaked", "dead") or bool(np.all(hits[:K] >= 1))
    if (K == 2 or (K == 16 and B == 1.0)) and cls == "default":
        ok = ok and hits[0] >= 2 and hits[K - 1] >= 2
    return ok


def open_case_holds(case, seed=None, with_kinks=True):
    """(met, knot margin, changed bins, kink room) of the `open` case on the float32 draws.  Its 172 k spline inputs cannot meet the
    carried-error knot condition at any seed: 64 u S is 2e-5 absolute around each of 15 knots per 6 units, so an input lies that close
    to a knot with probability 1e-4 and 17 of them are expected (measured at seeds 0 and 1: knot_room 0.06 and 0.02).  It keeps the
    earlier condition instead: KNOT_MARGIN of the bin's width, and no spline input in another bin in the float32 pass than in the float64
    one (bin_changes == 0) -- with the kink condition of every other case."""
    t = np.float32
    p, eps, arch = yard_params(case, t, seed), yard_draws(case, t), case[:5]
    knot = margin(p, arch, eps)[0]
    if not knot >= KNOT_MARGIN[np.dtype(t)]:
        return False, knot, None, None
    changed = bin_changes(p, arch, eps, t)[0]
    if changed or not with_kinks:
        return changed == 0, knot, changed, None
    kink = kink_room(p, arch, eps, t)
    return kink >= KINK_ROOM, knot, changed, kink


def find_seed(case, limit=2000, start=0):
    """the first seed at which the knot condition holds, the kink condition holds with room KINK_ROOM, both on both dtypes' draws, and the
    bins are hit as bins_hit asks (how YARD_CASES was filled)"""
    for seed in range(start, limit):
        if case[6] == "open":
            if open_case_holds(case, seed)[0]:
                return seed
            continue
        ok = True
        for t in yard_dtypes(case):
            kn, ki, hits = rooms(case, t, seed)
            if not (kn >= 1.0 and ki >= KINK_ROOM and bins_hit(case, hits)):
                ok = False
                break
        if ok:
            return seed
    return None
