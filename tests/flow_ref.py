"""The RealNVP family (MIVI_REALNVP, include/mivi.h) restated twice, for tests/test_flow_ref_host.py, tests/test_gpu_flow.py and
tests/test_gpu_flow_yardstick.py (the per-entry criterion: second half of this file -- magnitude, envelope, ratios, YARD_CASES).

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
def flow_slices(M, n_params=1):
    """The workgroups of the parameter sweep, restated from csrc/kernels_flow.hip: min(ceil(M / 16), 64) (and at most 2^25 / n_params, so
    that the partials stay under 256 MB).  Slice s owns the tiles s, s + n_slices, ...: a second tile only when M > 64 x 16."""
    return max(1, min((M + TILE - 1) // TILE, 64, (1 << 25) // n_params))


def kernel_order(M, n_params=1):
    """The sample order of the kernels as a permutation: tile t belongs to slice t mod n_slices, a slice's tiles follow one another, then the
    slices in slice order."""
    ns, tiles = flow_slices(M, n_params), (M + TILE - 1) // TILE
    return np.concatenate([np.arange(t * TILE, min(t * TILE + TILE, M)) for s in range(ns) for t in range(s, tiles, ns)])


def _mm4(A, B):
    """A @ B as the matrix core forms it: the inner axis in groups of K = 4, the groups added to the accumulator one after another"""
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=A.dtype)
    for k in range(0, A.shape[1], 4):
        acc = acc + A[:, k:k + 4] @ B[k:k + 4]
    return acc


def _np_forward_net(net, c, dtype, tanh, mm=np.matmul):
    """-> (output (tanh of it: the s net), [the input and the hidden activations], the output layer's pre-activation)"""
    acts, h = [c], c
    for j, (W, b) in enumerate(net):
        h = mm(W, h) + b[:, None]
        if j < len(net) - 1:
            h = np.where(h > 0, h, dtype(0.01) * h)
            acts.append(h)
    return (np.tanh(h) if tanh else h), acts, h


def _np_backward_net(net, acts, delta, cols=None, slope_at_0=0.01, mm=np.matmul, plan=None):
    """delta: the cotangent of the output layer's pre-activation.  -> ([dW_1, db_1, ...] or None without `cols`, the input's cotangent);
    cols: the sample columns the parameter gradient sums, in that order.  plan: [[columns of a tile, ...] per slice] -- the kernels' sum:
    a tile's product by `mm` in the element type, the tiles of a slice and then the slices added in float64."""
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
        delta = mm(np.ascontiguousarray(W.T), delta)
        if j > 0:
            delta = delta * np.where(acts[j] > 0, one, np.where(acts[j] == 0, W.dtype.type(slope_at_0), W.dtype.type(0.01)))
    return grads, delta


def _sech2(s, pre, T, from_pre):
    """1 - s^2 from the rounded s (what the kernels are documented to form), or sech^2 of the pre-activation (equal in exact arithmetic)"""
    if from_pre:
        c = np.cosh(pre)
        return T(1) / (c * c)
    return T(1) - s * s


FAULTS = ("lost_block", "lost_tile", "swap_masks", "no_kappa", "kappa_sign", "no_u",
          "tile_overwrites", "kink_slope_1", "one_entry", "one_row", "layer_off", "sech_from_f32_s_twice")


def fault_block(arch):
    """the first 64 x 64 weight block of the layout (the largest weight block where there is none): where one_entry / one_row strike"""
    lay = [e for e in flow_layout(*arch)[0] if e[3] == "W"]
    return max(lay, key=lambda e: (e[5] == (64, 64), e[5][0] * e[5][1], -e[4]))


def evaluate(params, arch, G, ell, eps, kind, dtype=np.float64, fault=None, order=None, emulate=False, sech_from_pre=False, tile_sums=False):
    """dict(Z, logq, value, grad): the forward pass and the two backward sweeps with every step in `dtype`, G = grad_z ell and ell given.
    order: a permutation of the samples -- the parameter gradient and the value sum them in that order.
    emulate: the kernels' own order -- every product with its inner axis in groups of K = 4 (_mm4), the parameter gradient as tile partials
    of 16 samples added in float64 within a slice and then over the slices in slice order (flow_slices), the value's terms in float64.
    sech_from_pre: the factor 1 - s^2 of both sweeps taken as sech^2 of the s net's output pre-activation.
    tile_sums: the sums over the samples as the kernels are documented to form them, in the order given: the parameter gradient 16 samples
    at a time in `dtype`, those partials and the value's terms added in float64 (the envelope's evaluations; without it the sums are numpy's
    in `dtype`, the yardstick of tests/test_gpu_flow.py, whose own summation error grows with M where the kernels' does not).
    Parameters with a dead unit (dead_units below: incoming weights and bias exactly 0, outgoing weights not) give a hidden pre-activation
    of exactly 0 in every dtype; forward maps it to 0 and backward takes the slope 0.01 there, as the kernels do.
    fault: None or one of FAULTS --
        tile_overwrites        a slice's later tile stores where it should add: the parameter gradient of a slice is its last tile's alone
        kink_slope_1           slope 1 at a pre-activation of exactly 0
        one_entry, one_row     entry (17, 23) / row 5 of the weight gradient of fault_block(arch) off by a relative 1e-3 / 1e-4
        layer_off              layer l >= 3 reads the parameters of layer l - 2
        sech_from_f32_s_twice  1 - s^2 applied twice in the s net's delta of layer 1 (parameter sweep)"""
    assert fault is None or fault in FAULTS, fault
    d, hidden, L = arch
    M = eps.shape[1]
    T = np.dtype(dtype).type
    p = np.asarray(params).astype(dtype)
    nets = _nets(p, arch, lambda v, o, i: v.reshape((o, i), order="F"))
    if fault == "layer_off":
        nets = {l: nets[l - 2] if l >= 3 else nets[l] for l in nets}
    eps, G, ell = np.asarray(eps).astype(dtype), np.asarray(G).astype(dtype), np.asarray(ell).astype(dtype)
    cols = np.arange(M) if order is None else np.asarray(order)
    if fault == "lost_tile":
        cols = cols[cols < TILE * ((M - 1) // TILE)]
    ns, tiles = flow_slices(M, p.shape[0]), (M + TILE - 1) // TILE
    if fault == "tile_overwrites":
        last = {s: max(range(s, tiles, ns)) for s in range(ns)}
        cols = cols[np.array([last[(c // TILE) % ns] == c // TILE for c in cols])]
    mm = _mm4 if emulate else np.matmul
    plan = [[np.arange(t * TILE, min(t * TILE + TILE, M)) for t in range(s, tiles, ns)] for s in range(ns)] if emulate else None
    if tile_sums:   # the documented sum in the given order: 16 samples at a time in the element type, those partials added in float64
        plan = [[cols[i:i + TILE] for i in range(0, len(cols), TILE)]]
    k0 = 1.0 if fault == "kink_slope_1" else 0.01
    mk = (lambda l: masks(d, l + 1)) if fault == "swap_masks" else (lambda l: masks(d, l))
    xs, ssum = [eps], np.zeros(M, dtype=np.float64 if emulate else dtype)
    for l in range(1, L + 1):
        A, B = mk(l)
        x = xs[-1]
        s, _, _ = _np_forward_net(nets[l]["s"], x[B], T, True, mm)
        t, _, _ = _np_forward_net(nets[l]["t"], x[B], T, False, mm)
        y = x.copy()
        y[A] = x[A] * np.exp(s) + t
        xs.append(y)
        ssum = ssum + s.sum(axis=0, dtype=ssum.dtype)
    if emulate:   # (the forward kernel: |eps|^2, the sum of s and log q itself in float64 from the stored element-type values)
        logq = -0.5 * (eps.astype(np.float64) ** 2).sum(axis=0) - 0.5 * d * math.log(2.0 * math.pi) - ssum
        value = T(((-ell.astype(np.float64) + logq)[cols]).sum() / M)
    else:
        logq = T(-0.5) * (eps * eps).sum(axis=0) - T(0.5 * d * math.log(2.0 * math.pi)) - ssum
        value = T(((-ell + logq)[cols]).astype(np.float64).sum() / M) if tile_sums else ((-ell + logq)[cols]).sum() / T(M)
    if kind == STL:   # u = grad_z log q(z), the parameters stopped: l = 1 .. L through the inverse layers
        xb = -eps
        for l in range(1, L + 1):
            A, B = mk(l)
            x = xs[l - 1]
            s, acts_s, pre = _np_forward_net(nets[l]["s"], x[B], T, True, mm)
            _, acts_t, _ = _np_forward_net(nets[l]["t"], x[B], T, False, mm)
            ab, ems = xb[A], np.exp(-s)
            _, cs = _np_backward_net(nets[l]["s"], acts_s, (-ab * x[A] - T(1)) * _sech2(s, pre, T, sech_from_pre), None, k0, mm)
            _, ct = _np_backward_net(nets[l]["t"], acts_t, -ab * ems, None, k0, mm)
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
        s, acts_s, pre = _np_forward_net(nets[l]["s"], x[B], T, True, mm)
        _, acts_t, _ = _np_forward_net(nets[l]["t"], x[B], T, False, mm)
        es = np.exp(s)
        q = _sech2(s, pre, T, sech_from_pre)
        gs, cs = _np_backward_net(nets[l]["s"], acts_s, (g[A] * x[A] * es + kappa) * (q * q if fault == "sech_from_f32_s_twice" and l == 1 else q),
                                  cols, k0, mm, plan)
        gt, ct = _np_backward_net(nets[l]["t"], acts_t, g[A], cols, k0, mm, plan)
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
    if fault in ("one_entry", "one_row"):
        _, _, _, _, off, (no, ni) = fault_block(arch)
        hit = [off + min(17, no - 1) + no * min(23, ni - 1)] if fault == "one_entry" else off + min(5, no - 1) + no * np.arange(ni)
        grad[hit] = grad[hit] * (T(1) + T(1e-3 if fault == "one_entry" else 1e-4))
    return dict(Z=xs[-1], logq=logq, value=value, grad=grad)


def wider(dtype):
    """the dtype of the reference evaluation for a context of `dtype`"""
    return np.float64 if np.dtype(dtype) == np.float32 else np.longdouble


ref_dtype = wider   # (the name tests/test_gpu_flow.py uses)


def inverse_np(params, arch, Z, dtype=np.float64):
    """log q at the columns of Z through the inverse layers l = L .. 1 with every step in `dtype` (the yardstick and the reference of
    mivi_logpdf at points that are not the context's own samples)"""
    d, hidden, L = arch
    T = np.dtype(dtype).type
    nets = _nets(np.asarray(params).astype(dtype), arch, lambda v, o, i: v.reshape((o, i), order="F"))
    y = np.asarray(Z).astype(dtype)
    ssum = np.zeros(y.shape[1], dtype=dtype)
    for l in range(L, 0, -1):
        A, B = masks(d, l)
        s, _, _ = _np_forward_net(nets[l]["s"], y[B], T, True)
        t, _, _ = _np_forward_net(nets[l]["t"], y[B], T, False)
        x = y.copy()
        x[A] = (y[A] - t) * np.exp(-s)
        y, ssum = x, ssum + s.sum(axis=0)
    return T(-0.5) * (y * y).sum(axis=0) - T(0.5 * d * math.log(2.0 * math.pi)) - ssum


def margin(params, arch, eps):
    """the smallest |p| / (sum_j |W_ij| |a_j| + |b_i|) over all hidden pre-activations p of all nets (float64): how far every leakyrelu
    is from its kink, in units of the scale its rounding error has.  (The condition of CASES, at most four layers deep; YARD_CASES are
    held to kink_room below, which carries the error of every layer's input and so stays valid at depth.)"""
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


# ==== the per-entry criterion (tests/test_flow_ref_host.py, tests/test_gpu_flow_yardstick.py) ==================================================
# Follows tests/meanfield_ref.py and tests/bijector_ref.py: ref is `evaluate` in the next wider type, env per entry the largest distance of
# eight sample orders of `evaluate` in the element type from it, S the first-order magnitude, u = 2^-24 / 2^-53, and a result is held to
# F32_FACTOR x max(env, u S).  S is a running error analysis of the documented formulas: every quantity v carries its error E_v in units of
# u beside its value, every product and sum contributing the magnitude of its operands (+ is the sum in quadrature: the roundings are
# independent) --
#     a b        E = E_a |b| + |a| E_b + |a b|               a + b      E = E_a + E_b + |a + b|
#     W h + b    E^2 = W^2 E_h^2 + W^2 h^2 + b^2  (= S_pre^2: the error of the layer's input enters it)
#     leakyrelu  E = slope E_pre (+ |h| below 0)             tanh       E = (1 - s^2) E_pre + |s|        e^s    E = e^s (E_s + 1)
#     1 - s^2    E = 2 |s| E_s + s^2 + (1 - s^2)  (formed from the ROUNDED s: relative to 1 - s^2 it carries 2 / (1 - s^2))
#                sech_from_pre: sech^2(pre) instead, E = (1 - s^2) (2 |s| E_pre + 1)
#     target     E_G = the target's gradient magnitude at |z| + E_z (tests/meanfield_ref.py _magnitude_target), likewise ell
# eps and the parameters are exact (E = 0).  The error of x^{l-1} enters layer l through its nets' input, where it carries through the
# magnitude of the net's own Jacobian per sample (|J| E), and through the products of the layer; the cotangents likewise through |J|'.
# Two choices were forced by depth and are NOT what the other yardsticks do: a worst-case analysis (plain sums, and |W_{H+1}| .. |W_1| E
# instead of |J| E) gives S_pre = 1.5e8 x (|W| |h| + |b|) on (127, (64,), 32, 2) and 3.4e3 x on (64, (64, 64), 4, 16) -- u S is then
# larger than the values and holds nothing, and no input meets the kink condition; with |J| E alone it is still 2e3 .. 8e5 x at L = 32.
# In quadrature S_pre is 2 .. 15 x (|W| |h| + |b|) on every case, and E_Z is 2 .. 6 u of |Z| (median) where the float32 evaluation
# measures 2e-7 .. 5e-7 relative l2, i.e. 3 .. 8 u.
U32, U64 = 2.0 ** -24, 2.0 ** -53
N_ORDERS = 8
KINK_FACTOR = 8 * 8   # |pre| >= 8 x 8 x u x S_pre: a deviation of F32_FACTOR times the allowed one cannot change a leakyrelu branch
OLD_MARGIN = {np.dtype(np.float32): 1e-4, np.dtype(np.float64): 1e-12}   # of |W| |h| + |b|: kept where it is the stronger condition


def unit(dtype):
    return U32 if np.dtype(dtype) == np.float32 else U64


def orders(M, n_params=1):
    """eight sample orders: the identity, the kernels' (kernel_order) and six seeded permutations; one order where M = 1"""
    if M == 1:
        return [None]
    return [None, kernel_order(M, n_params)] + [np.random.default_rng(1000 + k).permutation(M) for k in range(N_ORDERS - 2)]


def _q(*terms):
    """the magnitudes of independent roundings add in quadrature"""
    return np.sqrt(sum(np.square(t) for t in terms))


def _net_analysis(net, h0, E0):
    """One net on its input h0 (n x M) whose carried error is E0: dict of
        pre, Epre   the output layer's pre-activation and its error
        acts        [(h_j, E_j)], the input and the hidden activations
        hidden      [(pre_j, S_pre_j, |W_j| |h_{j-1}| + |b_j|)] of the hidden layers
        slopes, Jnet (M, out, n) = d pre / d h0 per sample, Jsuf [j] (M, out, width_j) = d pre / d pre_j per sample
    The roundings made INSIDE the net carry through |W| (at most four layers); the error of the input carries through the net's own
    Jacobian per sample, |J| E0."""
    M = h0.shape[1]
    h, Eloc, J = h0, np.zeros_like(h0), None
    acts, hidden, slopes = [(h0, E0)], [], []
    for j, (W, b) in enumerate(net):
        W2 = W * W
        pre = W @ h + b[:, None]
        Eloc_pre = np.sqrt(W2 @ (Eloc * Eloc) + W2 @ (h * h) + (b * b)[:, None])
        Jpre = np.broadcast_to(W, (M,) + W.shape) if J is None else W[None] @ J
        Epre = _q(Eloc_pre, np.sqrt(np.einsum("moi,im->om", Jpre * Jpre, E0 * E0)))
        if j < len(net) - 1:
            slope = np.where(pre > 0, 1.0, 0.01)
            h_new = slope * pre
            own = np.where(pre > 0, 0.0, np.abs(h_new))   # (the product with 0.01 rounds)
            hidden.append((pre, Epre, np.abs(W) @ np.abs(h) + np.abs(b)[:, None]))
            h, Eloc, J = h_new, _q(slope * Eloc_pre, own), slope.T[:, :, None] * Jpre
            acts.append((h, _q(slope * Epre, own)))
            slopes.append(slope)
    n_out = net[-1][0].shape[0]
    Jsuf = [None] * len(net)
    Jsuf[-1] = np.broadcast_to(np.eye(n_out), (M, n_out, n_out))
    for j in range(len(net) - 2, -1, -1):
        Jsuf[j] = (Jsuf[j + 1] @ net[j + 1][0][None]) * slopes[j].T[:, None, :]
    return dict(pre=pre, Epre=Epre, acts=acts, hidden=hidden, slopes=slopes, Jnet=Jpre, Jsuf=Jsuf)


def _net_back(net, an, dlt, Ed, want):
    """The backward sweep of one net from the output delta `dlt` (signed, out x M) with error Ed: ([S of dW_1, db_1, ...] if want, the
    input's cotangent, its error).  The sweep's own roundings carry through |W|', Ed through |Jsuf_j|' (see _net_analysis)."""
    grads, d, Eloc, Ed2 = [], dlt, np.zeros_like(dlt), Ed * Ed
    for j in range(len(net) - 1, -1, -1):
        W, (h, Eh) = net[j][0], an["acts"][j]
        if want:
            Ej2 = Eloc * Eloc + np.einsum("mok,om->km", np.square(an["Jsuf"][j]), Ed2)
            d2, h2, da = d * d, h * h, np.abs(d)   # (the sum over the samples may run in any order: its magnitude is the sum of |terms|)
            grads = [np.sqrt(Ej2 @ h2.T + d2 @ (Eh * Eh).T + np.square(da @ np.abs(h).T)), np.sqrt(Ej2.sum(axis=1) + np.square(da.sum(axis=1)))] + grads
        d, Eloc = W.T @ d, np.sqrt((W * W).T @ (Eloc * Eloc) + (W * W).T @ (d * d))
        if j > 0:
            d, Eloc = d * an["slopes"][j - 1], Eloc * an["slopes"][j - 1]
    return grads, d, _q(Eloc, np.sqrt(np.einsum("moi,om->im", np.square(an["Jnet"]), Ed2)))


def _s_of(an, sech_from_pre):
    """(s, E_s, E of the factor 1 - s^2) of an s net's analysis"""
    s = np.tanh(an["pre"])
    Es = _q((1.0 - s * s) * an["Epre"], s)
    return s, Es, _q((1.0 - s * s) * 2.0 * s * an["Epre"], 1.0 - s * s) if sech_from_pre else _q(2.0 * s * Es, s * s, 1.0 - s * s)


def magnitude(params, arch, tgt, eps, kind, sech_from_pre=False, Zin=None, EZin=None):
    """dict(Z (d x M), logq (M), value, grad, kink, old_margin, S_over_scale), float64: S of every output entry (the comment above).
    kink: the smallest |pre| / S_pre over the hidden pre-activations with S_pre > 0 (a dead unit has pre = S_pre = 0 exactly: no rounding
    can move it); old_margin: the same against |W| |h| + |b| alone (`margin`); S_over_scale: the largest S_pre / (|W| |h| + |b|).
    tgt None: the forward quantities alone.
    Zin: S (n) of log q at the columns of Zin through the inverse layers instead (dict(logq) alone; tgt, eps, kind unused); EZin: the
    error the points themselves carry (none: they are stored values)."""
    d, hidden, L = arch
    p = np.asarray(params, dtype=np.float64)
    nets = _nets(p, arch, lambda v, o, i: v.reshape((o, i), order="F"))
    c0 = 0.5 * d * math.log(2.0 * math.pi)
    if Zin is not None:
        y = np.asarray(Zin, dtype=np.float64)
        Ey, El2 = np.zeros_like(y) if EZin is None else np.asarray(EZin, dtype=np.float64), np.zeros(y.shape[1])
        for l in range(L, 0, -1):
            A, B = masks(d, l)
            ans, ant = _net_analysis(nets[l]["s"], y[B], Ey[B]), _net_analysis(nets[l]["t"], y[B], Ey[B])
            s, Es, _ = _s_of(ans, False)
            t, Et = ant["pre"], ant["Epre"]
            ems, diff = np.exp(-s), y[A] - t
            x, Ex = y.copy(), Ey.copy()
            x[A] = diff * ems
            Ex[A] = _q(Ey[A] * ems, Et * ems, x[A], x[A] * Es, x[A], x[A])
            y, Ey, El2 = x, Ex, El2 + (Es * Es).sum(axis=0)
        lq = -0.5 * (y * y).sum(axis=0) - c0
        return dict(logq=np.sqrt(np.sum(np.square(y * Ey) + 0.25 * y ** 4, axis=0) + El2 + lq * lq))
    E = np.asarray(eps, dtype=np.float64)
    M = E.shape[1]
    xs, Exs, El2, Sa, kink, old, worst, fwd = [E], [np.zeros_like(E)], np.zeros(M), np.zeros(M), np.inf, np.inf, 0.0, {}
    for l in range(1, L + 1):
        A, B = masks(d, l)
        x, Ex = xs[-1], Exs[-1]
        ans, ant = _net_analysis(nets[l]["s"], x[B], Ex[B]), _net_analysis(nets[l]["t"], x[B], Ex[B])
        fwd[l] = (ans, ant)
        for an in (ans, ant):
            for pre, Spre, scale in an["hidden"]:
                live = Spre > 0
                if np.any(live):
                    kink = min(kink, float(np.min(np.abs(pre[live]) / Spre[live])))
                    old = min(old, float(np.min(np.abs(pre[live]) / scale[live])))
                    worst = max(worst, float(np.max(Spre[live] / scale[live])))
        s, Es, _ = _s_of(ans, sech_from_pre)
        t, Et = ant["pre"], ant["Epre"]
        es = np.exp(s)
        y, Ey = x.copy(), Ex.copy()
        y[A] = x[A] * es + t
        xe = x[A] * es
        Ey[A] = _q(Ex[A] * es, xe * Es, xe, xe, Et, y[A])   # e^s from the rounded s; e^s itself; the product; t; the sum
        xs.append(y)
        Exs.append(Ey)
        El2, Sa = El2 + (Es * Es).sum(axis=0), Sa + s.sum(axis=0)
    Z, EZ = xs[-1], Exs[-1]
    lq = -0.5 * (E * E).sum(axis=0) - c0 - Sa
    S_logq = np.sqrt(0.25 * (E ** 4).sum(axis=0) + El2 + lq * lq)
    out = dict(Z=EZ, logq=S_logq, kink=kink, old_margin=old, S_over_scale=worst)
    if tgt is None:
        return out
    from tests import meanfield_ref as Mf
    ell, G = target_columns(tgt, Z)
    ell_a, Ga = Mf._magnitude_target(tgt, np.abs(Z) + EZ, Z, d)   # (one stage: the target's own documented magnitudes at |z| + E_z)
    if kind == STL:
        xb, Eb = -E, np.zeros_like(E)
        for l in range(1, L + 1):
            A, B = masks(d, l)
            xA, ExA = xs[l - 1][A], Exs[l - 1][A]
            ans, ant = fwd[l]
            s, Es, Eq = _s_of(ans, sech_from_pre)
            ems, q, ab = np.exp(-s), 1.0 - s * s, xb[A]
            inner = -ab * xA - 1.0
            Ein = _q(Eb[A] * xA, ab * ExA, ab * xA, inner)
            _, cs, Ecs = _net_back(nets[l]["s"], ans, inner * q, _q(Ein * q, inner * Eq, inner * q), False)
            dt_ = -ab * ems
            Edt = _q(Eb[A] * ems, dt_ * Es, dt_, dt_)
            _, ct, Ect = _net_back(nets[l]["t"], ant, dt_, Edt, False)
            yb, En = xb.copy(), Eb.copy()
            yb[A], En[A] = -dt_, Edt
            yb[B] = xb[B] + cs + ct
            En[B] = _q(Eb[B], Ecs, Ect, xb[B] + cs, yb[B])
            xb, Eb = yb, En
        g, Eg, kappa = (-G + xb) / M, _q(Ga, Eb, -G + xb) / M, 0.0
    else:
        g, Eg, kappa = -G / M, Ga / M, -1.0 / M
    S = np.zeros(p.shape[0])
    names = dict(blocks(arch))
    for l in range(L, 0, -1):
        A, B = masks(d, l)
        xA, ExA = xs[l - 1][A], Exs[l - 1][A]
        ans, ant = fwd[l]
        s, Es, Eq = _s_of(ans, sech_from_pre)
        es, q = np.exp(s), 1.0 - s * s
        pr = g[A] * xA * es
        inner = pr + kappa
        Ein = _q(Eg[A] * xA * es, g[A] * ExA * es, pr * Es, pr, pr, pr, inner)
        gs, cs, Ecs = _net_back(nets[l]["s"], ans, inner * q, _q(Ein * q, inner * Eq, inner * q), True)
        gt, ct, Ect = _net_back(nets[l]["t"], ant, g[A], Eg[A], True)
        for net, gr in (("s", gs), ("t", gt)):
            for j in range(len(hidden) + 1):
                S[names[f"l{l}.{net}.W{j + 1}"]] = gr[2 * j].reshape(-1, order="F")
                S[names[f"l{l}.{net}.b{j + 1}"]] = gr[2 * j + 1]
        gn, En = g.copy(), Eg.copy()
        gn[A] = g[A] * es
        En[A] = _q(Eg[A] * es, gn[A] * Es, gn[A], gn[A])
        gn[B] = g[B] + cs + ct
        En[B] = _q(Eg[B], Ecs, Ect, g[B] + cs, gn[B])
        g, Eg = gn, En
    out["grad"] = S
    out["value"] = float(_q(np.sqrt(np.sum(ell_a * ell_a + S_logq * S_logq)) / M, np.mean(np.abs(-ell + lq))))
    return out


def kink_room(params, arch, eps, dtype):
    """How many times over the inputs meet the kink condition (>= 1: met): every hidden pre-activation that rounding can move at all has
    |pre| >= KINK_FACTOR x u x S_pre, S_pre from `magnitude` with the carried error of the layer's input, AND the earlier |pre| >=
    1e-4 (f32) / 1e-12 (f64) of |W| |h| + |b| -- whichever is stronger."""
    m = magnitude(params, arch, None, eps, None)
    return min(m["kink"] / (KINK_FACTOR * unit(dtype)), m["old_margin"] / OLD_MARGIN[np.dtype(dtype)])


def envelope(params, arch, G, ell, eps, kind, dtype=np.float32, ref=None, sech_from_pre=False):
    """dict(Z, logq, value, grad): per entry max_k |evaluate(dtype, order_k) - ref| over orders(M) (Z and log q do not depend on the order)"""
    wide = wider(dtype)
    ref = evaluate(params, arch, G, ell, eps, kind, wide, sech_from_pre=sech_from_pre) if ref is None else ref
    env = None
    for o in orders(np.asarray(eps).shape[1], len(params)):
        y = evaluate(params, arch, G, ell, eps, kind, dtype, order=o, sech_from_pre=sech_from_pre, tile_sums=True)
        dist = {k: np.abs(np.asarray(y[k]).astype(wide) - ref[k]) for k in ("Z", "logq", "value", "grad")}
        env = dist if env is None else {k: np.maximum(env[k], dist[k]) for k in dist}
    return env


def criterion(params, arch, tgt, eps, kind, dtype, sech_from_pre=False):
    """dict(ref, yard, env, S, G, ell) of one estimate: the target's (ell, G) in float64 at the reference's own Z, `evaluate` in the wider
    type, in `dtype` (the yardstick of block_report), the envelope and the magnitude"""
    eps = np.asarray(eps)
    zeros = np.zeros(eps.shape)
    Z = evaluate(params, arch, zeros, zeros[0], eps, MONTE_CARLO, np.float64)["Z"]
    ell, G = target_columns(tgt, Z)
    ref = evaluate(params, arch, G, ell, eps, kind, wider(dtype), sech_from_pre=sech_from_pre)
    return dict(ref=ref, yard=evaluate(params, arch, G, ell, eps, kind, dtype, sech_from_pre=sech_from_pre), G=G, ell=ell,
                env=envelope(params, arch, G, ell, eps, kind, dtype, ref, sech_from_pre), S=magnitude(params, arch, tgt, eps, kind, sech_from_pre))


def all_ratios(got, crit, arch, dtype, extra=None):
    """dict(whole, row, entry, value, Z, logq) of a result dict(grad, value[, Z, logq]) against criterion(...)"""
    u, ref, env, S = unit(dtype), crit["ref"], crit["env"], crit["S"]
    out = ratios(got["grad"], env["grad"], ref["grad"], S["grad"], arch, u, extra)
    out["value"] = value_ratio(got["value"], env["value"], ref["value"], S["value"], u)
    for k in ("Z", "logq"):
        if k in got:
            out[k] = entry_ratio(got[k], ref[k], S[k], u, env[k])
    return out


def _norm(a):
    return np.sqrt(np.sum(a * a))


def ratios(got, env, ref, S_mag, arch, u, extra=None):
    """dict(whole, row, entry) of a flat gradient, every number ||got - ref|| / (max(||env||, u ||S||) + ||extra||) over a set of entries:
    each entry; each row of each W_j and each whole b_j (what one hidden unit's delta, or one bias vector, produces); the whole gradient.
    extra: an allowance added to every denominator (the rounding of a stored parameter when the gradient is recovered from a Descent step)."""
    ld = np.longdouble
    err = np.abs(np.asarray(got).astype(ld) - np.asarray(ref).astype(ld))
    en, fl = np.asarray(env).astype(ld), ld(u) * np.asarray(S_mag).astype(ld)
    ex = np.zeros(err.size, dtype=ld) if extra is None else np.asarray(extra).astype(ld)
    tiny = ld(np.finfo(np.float64).tiny)
    over = lambda sl: float(_norm(err[sl]) / (max(_norm(en[sl]), _norm(fl[sl])) + _norm(ex[sl]) + tiny))   # noqa: E731
    row = 0.0
    for _, _, _, k, off, shape in flow_layout(*arch)[0]:
        if k == "b":
            row = max(row, over(slice(off, off + shape[0])))
        else:   # vec W is column-major, out x in: row i is off + i, off + i + out, ...
            n = shape[0] * shape[1]
            num = np.sqrt(np.sum((err[off:off + n] ** 2).reshape(shape[1], shape[0]), axis=0))
            den = np.maximum(np.sqrt(np.sum((en[off:off + n] ** 2).reshape(shape[1], shape[0]), axis=0)),
                             np.sqrt(np.sum((fl[off:off + n] ** 2).reshape(shape[1], shape[0]), axis=0)))
            den = den + np.sqrt(np.sum((ex[off:off + n] ** 2).reshape(shape[1], shape[0]), axis=0)) + tiny
            row = max(row, float(np.max(num / den)))
    return dict(whole=over(slice(0, err.size)), row=row, entry=float(np.max(err / (np.maximum(en, fl) + ex + tiny))))


def value_ratio(got, env, ref, S_mag, u):
    ld = np.longdouble
    return float(abs(ld(got) - ld(ref)) / (max(ld(env), ld(u) * ld(S_mag)) + ld(np.finfo(np.float64).tiny)))


def entry_ratio(got, ref, S_mag, u, env=None):
    """the worst |got - ref| / max(env, u S) over an array (Z, log q)"""
    ld = np.longdouble
    err = np.abs(np.asarray(got).astype(ld) - np.asarray(ref).astype(ld))
    den = ld(u) * np.asarray(S_mag).astype(ld)
    if env is not None:
        den = np.maximum(den, np.asarray(env).astype(ld))
    return float(np.max(err / (den + ld(np.finfo(np.float64).tiny)))) if err.size else 0.0


# ---- the cases of the per-entry criterion ---------------------------------------------------------------------------------------------------
# (d, hidden, L, M, class) -> the seed of its parameters: the first at which kink_room() >= KINK_ROOM on the float32 AND on the float64 draws
# of estimate CASE_IDX (tests/test_flow_ref_host.py pins kink_room >= 1).  Classes (yard_params):
#     default    case_params: Glorot weights, biases N(0, 0.1^2)
#     damped     the output-layer weights W_{H+1} of both nets x 0.125 (deep flows are conditioned only here: at L = 32 `default` grows to
#                max|Z| ~ 1e4 .. 7e5 and the float32 evaluation itself is off by 0.3 relative l2; at 0.25 d = 127 still reaches max|Z| = 227)
#     sat4, sat16   the s net's W_{H+1} x 4 / x 16: tanh saturates as it does after training
#     dead       one dead unit in the s net of layer 1 (first hidden layer) and one in the t net of layer L (last hidden layer): DEAD
# What each shape reaches is in the module docstring of tests/test_gpu_flow_yardstick.py.
KINK_ROOM = 1.5
DEAD_UNIT = 2   # the hidden unit that is dead
YARD_CASES = {
    (5, (8,), 2, 1040, "default"): 159,               # 65 tiles: slice 0 owns the tiles 0 and 64, both full
    (6, (4,), 1, 2049, "default"): 1,                 # 129 tiles: slice 0 owns three, the third holding one sample
    (128, (64, 64, 64), 32, 1, "damped"): 1824,       # every limit at once; M = 1 keeps the pre-activations at 12 k
    (127, (64,), 32, 2, "damped"): 44,                # odd d at depth: |A_l| differs between odd and even layers
    (9, (8,), 32, 16, "damped"): 4,                   # depth with one full tile
    (17, (33, 20, 7), 3, 16, "default"): 13,
    (64, (64, 64), 4, 16, "default"): 1260,
    (5, (16, 7), 2, 33, "default"): 3,
    (5, (16, 7), 2, 33, "sat4"): 1,
    (5, (16, 7), 2, 33, "sat16"): 1,
    (5, (16, 7), 2, 33, "dead"): 2,
    (3, (5,), 1, 1, "default"): 0,
}
MANY_TILES = [c for c in YARD_CASES if c[3] > 64 * TILE]


def dead_units(case):
    """[(layer, net, hidden layer j (1-based), unit)] of the class `dead`"""
    d, hidden, L, M, cls = case
    return [(1, "s", 1, DEAD_UNIT), (L, "t", len(hidden), DEAD_UNIT)] if cls == "dead" else []


def yard_params(case, dtype, seed=None):
    """the parameters of a YARD_CASES entry, rounded to dtype"""
    d, hidden, L, M, cls = case
    p = case_params((d, hidden, L, M), np.float64, YARD_CASES[case] if seed is None else seed)
    H = len(hidden)
    for l, net, j, kind, off, shape in flow_layout(d, hidden, L)[0]:
        n = int(np.prod(shape))
        if kind == "W" and j == H + 1:
            p[off:off + n] *= {"damped": 0.125, "sat4": 4.0 if net == "s" else 1.0, "sat16": 16.0 if net == "s" else 1.0}.get(cls, 1.0)
        for dl, dnet, dj, unit_ in dead_units(case):   # incoming weights (row `unit_` of W_j) and bias exactly 0; the outgoing column stays
            if (l, net, j) == (dl, dnet, dj):
                if kind == "W":
                    p[off + unit_:off + n:shape[0]] = 0.0
                else:
                    p[off + unit_] = 0.0
    return p.astype(dtype)


def dead_rows(case):
    """the indices of the gradient entries of the dead units' incoming weights"""
    d, hidden, L, M, cls = case
    out = []
    for l, net, j, kind, off, shape in flow_layout(d, hidden, L)[0]:
        for dl, dnet, dj, unit_ in dead_units(case):
            if (l, net, j, kind) == (dl, dnet, dj, "W"):
                out.extend(range(off + unit_, off + shape[0] * shape[1], shape[0]))
    return np.array(out, dtype=np.int64)


def find_seed(case, limit=4000):
    """the first seed at which the kink condition holds with room KINK_ROOM on both dtypes' draws (how YARD_CASES was filled)"""
    from oracle import oracle as O
    from tests.helpers import SEED
    d, hidden, L, M, _ = case
    draws = [(t, O.philox_normal(SEED, CASE_IDX, d, 0, M, f64=t == np.float64)) for t in (np.float32, np.float64)]
    for seed in range(limit):
        if all(kink_room(yard_params(case, t, seed), (d, hidden, L), e, t) >= KINK_ROOM for t, e in draws):
            return seed
    return None
