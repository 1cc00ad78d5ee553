"""Bayesian neural network target: microseconds per mivi_estimate_gradient on the mean-field family, closed-form entropy, f32 and f64, at
(n, p, hidden, M) = (80, 2, (3, 2), 10) -- the Turing tutorial's --, (10^4, 16, (32, 32), 64) and (10^5, 64, (64, 64, 64), 256), Bernoulli
likelihood -- and, for the multi-output head (categorical likelihood, C classes), at the tutorial's shape with C = 3, the middle one with
C = 10 and (10^5, 16, (64, 64, 64), 256) with C = 64 (the widest three-layer network whose head fits the LDS in f64) -- in the same process
on the same device,
    (builtin) the built-in target (avi.BNNProblem: csrc/kernels_bnn.hip),
    (plugin)  the same model as a host plugin (numpy in the context's dtype behind mivi_set_target_callback: Z down, G up, every estimate),
    (torch)   the same estimate composed in torch on device tensors: per-sample weights through baddbmm (and log_softmax for the head), the gradient by
              autograd, draws by torch.randn.
Every figure is device time: two events around CALLS back-to-back calls, divided by CALLS, after WARM warm-up calls (the plugin leg, whose
call is host-bound and takes seconds at the largest shape, is one call without warm-up in the first PLUGIN_ROUNDS rounds); the legs
alternate over ROUNDS rounds, the median of the rounds is reported and their spread (max - min) next to it.  One JSON line per case;
`python tools/bnn_bench.py [out.jsonl]` appends them (profiles/bnn_bench.jsonl)."""
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


class NumpyModel:
    """The model as a LogDensityProblems plugin over the columns of Z, in X's dtype: one network after the other."""

    def __init__(self, X, y, layers):
        self.X, self.y, self.layers = X, y, layers
        self.rows, self.labels = np.arange(X.shape[0]), y.astype(np.int64)   # (the head: y holds class labels)

    def dimension(self):
        return sum(o * (i + 1) for o, i in self.layers)

    def logdensity_and_gradient_batch(self, Z):
        G, ell = np.empty_like(Z), np.empty(Z.shape[1], Z.dtype)
        for m in range(Z.shape[1]):
            z, acts, Ws, off = Z[:, m], [self.X], [], 0
            for k, (o, i) in enumerate(self.layers):
                W, b = z[off:off + o * i].reshape(o, i, order="F"), z[off + o * i:off + o * (i + 1)]
                Ws.append((W, off))
                a = acts[-1] @ W.T + b
                acts.append(np.tanh(a) if k < len(self.layers) - 1 else a)
                off += o * (i + 1)
            if self.layers[-1][0] > 1:   # categorical: a stable softmax per row
                f = acts.pop()
                f = f - f.max(axis=1, keepdims=True)
                ex = np.exp(f)
                se = ex.sum(axis=1, keepdims=True)
                ell[m] = (f[self.rows, self.labels] - np.log(se[:, 0])).sum() - 0.5 * (z * z).sum() - 0.5 * z.size * LOG2PI
                delta = -(ex / se)
                delta[self.rows, self.labels] += 1
                delta = delta.astype(Z.dtype)
            else:
                f = acts.pop()[:, 0]
                e = np.exp(-np.abs(f))
                ell[m] = (self.y * f - np.maximum(f, 0) - np.log1p(e)).sum() - 0.5 * (z * z).sum() - 0.5 * z.size * LOG2PI
                delta = (self.y - np.where(f >= 0, 1, e) / (1 + e))[:, None].astype(Z.dtype)
            for (W, off), a in zip(reversed(Ws), reversed(acts)):
                G[off:off + W.size, m] = (delta.T @ a).reshape(-1, order="F")
                G[off + W.size:off + W.size + W.shape[0], m] = delta.sum(axis=0)
                delta = (delta @ W) * (1 - a * a)
        return ell, G - Z


def torch_estimate(mu, sig, X, y, layers, M):
    E = torch.randn(mu.shape[0], M, device=mu.device, dtype=mu.dtype)
    Z = (mu[:, None] + sig[:, None] * E).requires_grad_(True)
    a, off = X.expand(M, *X.shape), 0
    for k, (o, i) in enumerate(layers):   # W' per sample, (M, in, out): column-major out x in read as (in, out) row-major
        a = torch.baddbmm(Z[off + o * i:off + o * (i + 1)].T[:, None, :], a, Z[off:off + o * i].T.reshape(M, i, o))
        a = torch.tanh(a) if k < len(layers) - 1 else a
        off += o * (i + 1)
    if layers[-1][0] > 1:   # categorical
        ll = torch.log_softmax(a, dim=2).gather(2, y.long()[None, :, None].expand(M, -1, 1)).sum(dim=(1, 2))
    else:
        f = a[:, :, 0]
        ll = (y * f - torch.nn.functional.softplus(f)).sum(dim=1)
    ell = ll - 0.5 * (Z * Z).sum(dim=0) - 0.5 * mu.shape[0] * LOG2PI
    G, = torch.autograd.grad(ell.sum(), Z)
    value = -ell.detach().mean() - (0.5 * mu.shape[0] * (1 + LOG2PI) + torch.log(sig).sum())
    return value, -G.mean(dim=1), -(G * E).mean(dim=1) - 1 / sig


def case(n, p, hidden, M, dt, sink=None, C=1):
    rng = np.random.default_rng(1)
    X, y = (rng.normal(size=(n, p)) / np.sqrt(p)).astype(dt), rng.integers(0, max(C, 2), size=n).astype(dt)
    builtin = avi.BNNProblem(X, y, hidden, "categorical", n_classes=C) if C > 1 else avi.BNNProblem(X, y, hidden)
    d, layers = builtin.dimension(), builtin.layers()
    q = avi.MeanFieldGaussian((rng.normal(size=d) * 0.3).astype(dt), rng.uniform(0.05, 0.2, size=d).astype(dt))
    legs, idx, ctxs = {}, [0], []
    for name, prob in (("builtin", builtin), ("plugin", NumpyModel(X, y, layers))):
        c = avi.MiviContext(dt, avi.MEANFIELD, d, M, avi.ClosedFormEntropy.code, 1)
        c.set_problem(prob)
        ctxs.append(c)
        pd, v, g = c.to_device(avi.destructure(q)[0]), c.empty(1), c.empty(c.params_len)

        def leg(c=c, pd=pd, v=v, g=g):
            idx[0] += 1
            c.estimate_gradient(pd, idx[0], v, g)
        legs[name] = leg
    dev = torch.device("cuda", 0)
    t = [torch.tensor(a, device=dev) for a in (q.location, q.scale, X, y)]
    legs["torch"] = lambda: torch_estimate(*t, layers, M)
    med = {k: [] for k in legs}
    for rnd in range(ROUNDS):
        for k, fn in legs.items():
            if k != "plugin" or rnd < PLUGIN_ROUNDS:
                med[k].append(timed(fn, 1, 0) if k == "plugin" else timed(fn, CALLS))
    rec = {"bench": "bnn_estimate_gradient", "n": n, "p": p, "hidden": list(hidden), "M": M, "d": d, "dtype": np.dtype(dt).name, "family": "meanfield",
           "entropy": "ClosedFormEntropy", "likelihood": "categorical" if C > 1 else "bernoulli", "n_out": C, "calls": CALLS, "rounds": ROUNDS, "plugin_calls": 1, "plugin_rounds": PLUGIN_ROUNDS}
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
    for shape in ((80, 2, (3, 2), 10), (10 ** 4, 16, (32, 32), 64), (10 ** 5, 64, (64, 64, 64), 256)):
        for dt in (np.float32, np.float64):
            case(*shape, dt, sink)
    for shape, C in (((80, 2, (3, 2), 10), 3), ((10 ** 4, 16, (32, 32), 64), 10), ((10 ** 5, 16, (64, 64, 64), 256), 64)):
        for dt in (np.float32, np.float64):
            case(*shape, dt, sink, C)
