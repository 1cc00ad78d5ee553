"""Softmax regression target: microseconds per mivi_estimate_gradient on the mean-field family, closed-form entropy, f32 and f64, at
(n, p, C, M) = (10^4, 64, 10, 32), (10^5, 256, 10, 64) and (2 10^4, 32, 64, 16) -- in the same process on the same device,
    (builtin) the built-in target (avi.SoftmaxRegProblem: csrc/kernels_softmax.hip),
    (plugin)  the same model as a host plugin (numpy in the context's dtype behind mivi_set_target_callback: Z down, G up, every estimate),
    (torch)   the same estimate composed in torch on device tensors: X @ B, log_softmax, the explicit X'(Y - P), draws by torch.randn.
Every figure is device time: two events around CALLS back-to-back calls, divided by CALLS, after WARM warm-up calls (the plugin leg, whose
call is host-bound, takes PLUGIN_CALLS); the legs alternate over ROUNDS rounds, the median of the rounds is reported and their spread
(max - min) next to it.  One JSON line per case; `python tools/softmax_bench.py [out.jsonl]` appends them (profiles/softmax_bench.jsonl)."""
import json, statistics, sys
import numpy as np
sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
import torch
import advancedvi_jl_amd as avi

CALLS, PLUGIN_CALLS, WARM, ROUNDS = 20, 2, 3, 5
LOG2PI = float(np.log(2 * np.pi))


def timed(fn, calls):
    for _ in range(min(WARM, calls)):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


class NumpyModel:
    """The model as a LogDensityProblems plugin, batched over the columns of Z, in X's dtype."""

    def __init__(self, X, y, C):
        self.X, self.y, self.C, self.rows = X, y.astype(np.int64), C, np.arange(X.shape[0])

    def dimension(self):
        return self.X.shape[1] * self.C + 1

    def logdensity_and_gradient_batch(self, Z):
        (n, p), C, M = self.X.shape, self.C, Z.shape[1]
        B, s = Z[:p * C].reshape(p, C * M, order="F"), Z[p * C]   # column m C + c of B is class c of sample m
        L = (self.X @ B).reshape(n, M, C)
        L -= L.max(axis=2, keepdims=True)
        P = np.exp(L)
        se = P.sum(axis=2, keepdims=True)
        ll = (L[self.rows, :, self.y] - np.log(se[self.rows, :, 0])).sum(axis=0)
        R = -P / se
        R[self.rows, :, self.y] += 1
        is2, bb = np.exp(-2 * s), (Z[:p * C] ** 2).sum(axis=0)
        G = np.empty_like(Z)
        G[:p * C] = (self.X.T @ R.reshape(n, M * C)).reshape(p * C, M, order="F") - Z[:p * C] * is2
        G[p * C] = -p * C + bb * is2 - np.exp(2 * s) / 9
        return ll - 0.5 * p * C * LOG2PI - p * C * s - 0.5 * bb * is2 - 0.5 * np.log(18 * np.pi) - np.exp(2 * s) / 18, G


def torch_estimate(mu, sig, X, y, rows, C, M):
    n, p = X.shape
    E = torch.randn(mu.shape[0], M, device=mu.device, dtype=mu.dtype)
    Z = mu[:, None] + sig[:, None] * E
    Bm, s = Z[:p * C].T.reshape(M, C, p), Z[p * C]
    logp = torch.log_softmax(torch.matmul(X, Bm.transpose(1, 2)), dim=2)   # (M, n, C)
    ll = logp[:, rows, y].sum(dim=1)
    R = -torch.exp(logp)
    R[:, rows, y] += 1
    is2, bb = torch.exp(-2 * s), (Z[:p * C] ** 2).sum(dim=0)
    G = torch.empty_like(Z)
    G[:p * C] = torch.matmul(X.T, R).transpose(1, 2).reshape(M, p * C).T - Z[:p * C] * is2
    G[p * C] = -p * C + bb * is2 - torch.exp(2 * s) / 9
    ell = ll - 0.5 * p * C * LOG2PI - p * C * s - 0.5 * bb * is2 - 0.5 * np.log(18 * np.pi) - torch.exp(2 * s) / 18
    value = -ell.mean() - (0.5 * mu.shape[0] * (1 + LOG2PI) + torch.log(sig).sum())
    return value, -G.mean(dim=1), -(G * E).mean(dim=1) - 1 / sig


def case(n, p, C, M, dt, sink=None):
    rng = np.random.default_rng(1)
    d = p * C + 1
    X, y = (rng.normal(size=(n, p)) / np.sqrt(p)).astype(dt), rng.integers(0, C, size=n).astype(np.uint8)
    q = avi.MeanFieldGaussian((rng.normal(size=d) * 0.3).astype(dt), rng.uniform(0.05, 0.2, size=d).astype(dt))
    legs, idx, ctxs = {}, [0], []
    for name, prob in (("builtin", avi.SoftmaxRegProblem(X, y, C)), ("plugin", NumpyModel(X, y, C))):
        c = avi.MiviContext(dt, avi.MEANFIELD, d, M, avi.ClosedFormEntropy.code, 1)
        c.set_problem(prob)
        ctxs.append(c)
        pd, v, g = c.to_device(avi.destructure(q)[0]), c.empty(1), c.empty(c.params_len)

        def leg(c=c, pd=pd, v=v, g=g):
            idx[0] += 1
            c.estimate_gradient(pd, idx[0], v, g)
        legs[name] = leg
    dev = torch.device("cuda", 0)
    t = [torch.tensor(a, device=dev) for a in (q.location, q.scale, X)]
    ty, rows = torch.tensor(y.astype(np.int64), device=dev), torch.arange(n, device=dev)
    legs["torch"] = lambda: torch_estimate(t[0], t[1], t[2], ty, rows, C, M)
    med = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            med[k].append(timed(fn, PLUGIN_CALLS if k == "plugin" else CALLS))
    rec = {"bench": "softmax_estimate_gradient", "n": n, "p": p, "C": C, "M": M, "dtype": np.dtype(dt).name, "family": "meanfield",
           "entropy": "ClosedFormEntropy", "calls": CALLS, "plugin_calls": PLUGIN_CALLS, "rounds": ROUNDS}
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
    for shape in ((10 ** 4, 64, 10, 32), (10 ** 5, 256, 10, 64), (2 * 10 ** 4, 32, 64, 16)):
        for dt in (np.float32, np.float64):
            case(*shape, dt, sink)
