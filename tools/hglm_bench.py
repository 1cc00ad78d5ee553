"""Hierarchical GLM target: microseconds per mivi_estimate_gradient on the mean-field family, closed-form entropy, f32 and f64, at
(n, p, J, M) = (2 x 10^3, 8, 50, 16), (10^5, 32, 10^3, 64) and (10^6, 64, 10^5, 64), Bernoulli likelihood, no offset, group ids in random
order -- in the same process on the same device,
    (builtin) the built-in target (avi.HierGLMProblem: csrc/kernels_hglm.hip),
    (plugin)  the same model as a host plugin (numpy in the context's dtype behind mivi_set_target_callback: Z down, G up, every estimate),
    (torch)   the same estimate composed in torch on device tensors: X @ B + U[groups], the group sums by index_add_, the gradient
              written out by hand (no autograd tape), draws by torch.randn.
Every figure is device time: two events around CALLS back-to-back calls, divided by CALLS, after WARM warm-up calls (the plugin leg, whose
call is host-bound, is one call without warm-up in the first PLUGIN_ROUNDS rounds); the legs alternate over ROUNDS rounds, the median of
the rounds is reported and their spread (max - min) next to it.  One JSON line per case; `python tools/hglm_bench.py [out.jsonl]` appends
them (profiles/hglm_bench.jsonl)."""
import json, statistics, sys
import numpy as np
sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
import torch
import advancedvi_jl_amd as avi

CALLS, WARM, ROUNDS, PLUGIN_ROUNDS = 20, 3, 5, 2
LOG2PI = float(np.log(2 * np.pi))


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


def terms(xp, X, y, groups, p, J, Z, group_sum):
    """log pi and its gradient over the columns of Z (prior_std = tau_scale = likeadj = 1) in numpy or torch; group_sum(res) -> (J, M)"""
    B, U, s = Z[:p], Z[p:p + J], Z[p + J]
    eta = X @ B + U[groups]
    e = xp.exp(-abs(eta))
    ll = (y[:, None] * eta - (eta + abs(eta)) / 2 - xp.log1p(e)).sum(0)
    res = y[:, None] - xp.where(eta >= 0, 1 / (1 + e), e / (1 + e))
    uu, e2, em2 = (U * U).sum(0), xp.exp(2 * s), xp.exp(-2 * s)
    ell = ll - 0.5 * (B * B).sum(0) - 0.5 * p * LOG2PI - 0.5 * uu * em2 - J * (s + 0.5 * LOG2PI) + float(np.log(2.0)) - 0.5 * LOG2PI - 0.5 * e2 + s
    return ell, X.T @ res - B, group_sum(res) - U * em2, -J + uu * em2 - e2 + 1


class NumpyModel:
    """The model as a LogDensityProblems plugin over the columns of Z, in X's dtype."""

    def __init__(self, X, y, groups, J):
        self.X, self.y, self.groups, self.J = X, y, groups, J
        self.order, counts = np.argsort(groups, kind="stable"), np.bincount(groups, minlength=J)
        self.filled, self.starts = counts > 0, (np.cumsum(counts) - counts)[counts > 0]

    def dimension(self):
        return self.X.shape[1] + self.J + 1

    def logdensity_and_gradient_batch(self, Z):
        def group_sum(res):
            out = np.zeros((self.J, res.shape[1]), res.dtype)
            out[self.filled] = np.add.reduceat(res[self.order], self.starts, axis=0)
            return out
        ell, gB, gU, gs = terms(np, self.X, self.y, self.groups, self.X.shape[1], self.J, Z, group_sum)
        return ell.astype(Z.dtype), np.concatenate([gB, gU, gs[None]]).astype(Z.dtype)


def torch_estimate(mu, sig, X, y, groups, p, J, M):
    E = torch.randn(mu.shape[0], M, device=mu.device, dtype=mu.dtype)
    Z = mu[:, None] + sig[:, None] * E
    ell, gB, gU, gs = terms(torch, X, y, groups, p, J, Z, lambda res: torch.zeros(J, M, device=mu.device, dtype=mu.dtype).index_add_(0, groups, res))
    G = torch.cat([gB, gU, gs[None]])
    value = -ell.mean() - (0.5 * mu.shape[0] * (1 + LOG2PI) + torch.log(sig).sum())
    return value, -G.mean(dim=1), -(G * E).mean(dim=1) - 1 / sig


def case(n, p, J, M, dt, sink=None):
    rng = np.random.default_rng(1)
    X, y, groups = (rng.normal(size=(n, p)) / np.sqrt(p)).astype(dt), rng.integers(0, 2, size=n).astype(dt), rng.integers(0, J, size=n).astype(np.int32)
    d = p + J + 1
    q = avi.MeanFieldGaussian((rng.normal(size=d) * 0.3).astype(dt), rng.uniform(0.05, 0.2, size=d).astype(dt))
    legs, idx, ctxs = {}, [0], []
    for name, prob in (("builtin", avi.HierGLMProblem(X, y, groups, J)), ("plugin", NumpyModel(X, y, groups, J))):
        c = avi.MiviContext(dt, avi.MEANFIELD, d, M, avi.ClosedFormEntropy.code, 1)
        c.set_problem(prob)
        ctxs.append(c)
        pd, v, g = c.to_device(avi.destructure(q)[0]), c.empty(1), c.empty(c.params_len)

        def leg(c=c, pd=pd, v=v, g=g):
            idx[0] += 1
            c.estimate_gradient(pd, idx[0], v, g)
        legs[name] = leg
    dev = torch.device("cuda", 0)
    t = [torch.tensor(a, device=dev) for a in (q.location, q.scale, X, y, groups.astype(np.int64))]
    legs["torch"] = lambda: torch_estimate(*t, p, J, M)
    med = {k: [] for k in legs}
    for rnd in range(ROUNDS):
        for k, fn in legs.items():
            if k != "plugin" or rnd < PLUGIN_ROUNDS:
                med[k].append(timed(fn, 1, 0) if k == "plugin" else timed(fn, CALLS))
    rec = {"bench": "hglm_estimate_gradient", "n": n, "p": p, "J": J, "M": M, "d": d, "dtype": np.dtype(dt).name, "family": "meanfield",
           "entropy": "ClosedFormEntropy", "likelihood": "bernoulli", "calls": CALLS, "rounds": ROUNDS, "plugin_calls": 1, "plugin_rounds": PLUGIN_ROUNDS}
    for k in legs:
        rec[k + "_us"] = round(statistics.median(med[k]), 2)
        rec[k + "_spread_us"] = round(max(med[k]) - min(med[k]), 2)
    for c in ctxs:
        c.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


if __name__ == "__main__":
    sink = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
    for shape in ((2 * 10 ** 3, 8, 50, 16), (10 ** 5, 32, 10 ** 3, 64), (10 ** 6, 64, 10 ** 5, 64)):
        for dt in (np.float32, np.float64):
            case(*shape, dt, sink)
