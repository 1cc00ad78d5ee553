"""Probabilistic PCA target: microseconds per mivi_estimate_gradient on the mean-field family, closed-form entropy, f32 and f64, at
(N, D, k, M) = (150, 4, 2, 10), (10^4, 64, 8, 16) and (10^5, 256, 16, 16) (d = 1 604 353), no mask, no ARD -- in the same process on the
same device,
    (builtin) the built-in target (avi.PPCAProblem: csrc/kernels_ppca.hip),
    (plugin)  the same model as a host plugin (numpy in the context's dtype behind mivi_set_target_callback: Z down, G up, every estimate),
    (torch)   the same estimate composed in torch on device tensors: baddbmm for mu + Z W', two bmm for the gradients of W and Z, written
              out by hand (no autograd tape), draws by torch.randn.
Every figure is device time: two events around CALLS back-to-back calls, divided by CALLS, after WARM warm-up calls (the plugin leg, whose
call is host-bound, is one call without warm-up in the first PLUGIN_ROUNDS rounds); the legs alternate over ROUNDS rounds, the median of
the rounds is reported and their spread (max - min) next to it.  One JSON line per case; `python tools/ppca_bench.py [out.jsonl]` appends
them (profiles/ppca_bench.jsonl)."""
import json, statistics, sys
import numpy as np
sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
import torch
import advancedvi_jl_amd as avi

CALLS, WARM, ROUNDS, PLUGIN_ROUNDS = 20, 3, 5, 2
LOG2PI = float(np.log(2 * np.pi))
MEAN_VAR = 100.0   # mean_std = 10; prior_std = noise_scale = likeadj = 1


def timed(fn, calls, warm=WARM):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def priors(xp, W2, mu, s, N, D, k):
    """the terms of log pi that no row enters, from |W|^2 per sample, mu (.., D) and s"""
    return (-0.5 * W2 - 0.5 * D * k * LOG2PI - 0.5 * (mu * mu).sum(-1) / MEAN_VAR - D * (0.5 * float(np.log(MEAN_VAR)) + 0.5 * LOG2PI)
            + float(np.log(2.0)) - 0.5 * LOG2PI - 0.5 * xp.exp(2 * s) + s - N * 0.5 * k * LOG2PI)


class NumpyModel:
    """The model as a LogDensityProblems plugin over the columns of Z, in Y's dtype, one sample at a time."""

    def __init__(self, Y, k):
        self.Y, self.k = Y, k

    def dimension(self):
        N, D = self.Y.shape
        return D * self.k + N * self.k + D + 1

    def logdensity_and_gradient_batch(self, Z):
        (N, D), k = self.Y.shape, self.k
        oz, om = D * k, D * k + N * k
        ell, G = np.empty(Z.shape[1], Z.dtype), np.empty_like(Z)
        for m in range(Z.shape[1]):
            W, Zl, mu, s = Z[:oz, m].reshape(k, D).T, Z[oz:om, m].reshape(N, k), Z[om:om + D, m], Z[-1, m]
            res, em2 = self.Y - mu - Zl @ W.T, np.exp(-2 * s)
            ss = (res * res).sum()
            ell[m] = -0.5 * ss * em2 - N * D * (s + 0.5 * LOG2PI) - 0.5 * (Zl * Zl).sum() + priors(np, (W * W).sum(), mu, s, N, D, k)
            G[:oz, m], G[oz:om, m] = (em2 * (res.T @ Zl) - W).T.ravel(), (em2 * (res @ W) - Zl).ravel()
            G[om:om + D, m], G[-1, m] = em2 * res.sum(0) - mu / MEAN_VAR, ss * em2 - N * D - np.exp(2 * s) + 1
        return ell, G


def torch_estimate(loc, sig, Y, N, D, k, M):
    E = torch.randn(M, loc.shape[0], device=loc.device, dtype=loc.dtype)
    Z = loc + sig * E   # (M, d): a sample per row, so that the blocks below are views
    oz, om = D * k, D * k + N * k
    W, Zl, mu, s = Z[:, :oz].view(M, k, D), Z[:, oz:om].view(M, N, k), Z[:, om:om + D], Z[:, -1]
    res, em2 = Y - torch.baddbmm(mu[:, None, :], Zl, W), torch.exp(-2 * s)
    ss = (res * res).sum((1, 2))
    ell = -0.5 * ss * em2 - N * D * (s + 0.5 * LOG2PI) - 0.5 * (Zl * Zl).sum((1, 2)) + priors(torch, (W * W).sum((1, 2)), mu, s, N, D, k)
    gW = em2[:, None, None] * torch.bmm(Zl.transpose(1, 2), res) - W          # (M, k, D): theta's layout
    gZ = em2[:, None, None] * torch.bmm(res, W.transpose(1, 2)) - Zl          # (M, N, k)
    G = torch.cat([gW.reshape(M, -1), gZ.reshape(M, -1), em2[:, None] * res.sum(1) - mu / MEAN_VAR, (ss * em2 - N * D - torch.exp(2 * s) + 1)[:, None]], 1)
    value = -ell.mean() - (0.5 * loc.shape[0] * (1 + LOG2PI) + torch.log(sig).sum())
    return value, -G.mean(0), -(G * E).mean(0) - 1 / sig


def case(N, D, k, M, dt, sink=None):
    rng = np.random.default_rng(1)
    Y = (rng.normal(size=(N, k)) @ rng.normal(size=(k, D)) / np.sqrt(k) + 0.3 * rng.normal(size=(N, D))).astype(dt)
    d = D * k + N * k + D + 1
    q = avi.MeanFieldGaussian((rng.normal(size=d) * 0.3).astype(dt), rng.uniform(0.05, 0.2, size=d).astype(dt))
    legs, idx, ctxs = {}, [0], []
    for name, prob in (("builtin", avi.PPCAProblem(Y, k)), ("plugin", NumpyModel(Y, k))):
        c = avi.MiviContext(dt, avi.MEANFIELD, d, M, avi.ClosedFormEntropy.code, 1)
        c.set_problem(prob)
        ctxs.append(c)
        pd, v, g = c.to_device(avi.destructure(q)[0]), c.empty(1), c.empty(c.params_len)

        def leg(c=c, pd=pd, v=v, g=g):
            idx[0] += 1
            c.estimate_gradient(pd, idx[0], v, g)
        legs[name] = leg
    t = [torch.tensor(a, device=torch.device("cuda", 0)) for a in (q.location, q.scale, Y)]
    legs["torch"] = lambda: torch_estimate(*t, N, D, k, M)
    med = {name: [] for name in legs}
    for rnd in range(ROUNDS):
        for name, fn in legs.items():
            if name != "plugin" or rnd < PLUGIN_ROUNDS:
                med[name].append(timed(fn, 1, 0) if name == "plugin" else timed(fn, CALLS))
    rec = {"bench": "ppca_estimate_gradient", "N": N, "D": D, "k": k, "M": M, "d": d, "dtype": np.dtype(dt).name, "family": "meanfield",
           "entropy": "ClosedFormEntropy", "calls": CALLS, "rounds": ROUNDS, "plugin_calls": 1, "plugin_rounds": PLUGIN_ROUNDS}
    for name in legs:
        rec[name + "_us"] = round(statistics.median(med[name]), 2)
        rec[name + "_spread_us"] = round(max(med[name]) - min(med[name]), 2)
    for c in ctxs:
        c.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


if __name__ == "__main__":
    sink = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
    for shape in ((150, 4, 2, 10), (10 ** 4, 64, 8, 16), (10 ** 5, 256, 16, 16)):
        for dt in (np.float32, np.float64):
            case(*shape, dt, sink)
