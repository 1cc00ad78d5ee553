"""RealNVP family: microseconds per mivi_estimate_gradient at (d, hidden, L, M) = (2, (16, 16), 3, 8) -- the tutorial's shape -- and
(64, (64, 64), 8, 4096), MonteCarloEntropy and StickingTheLandingEntropy, f32 and f64, diagonal-Gaussian target -- against, in the same
process on the same device,
    (torch)  the same estimate as torch autograd on device tensors (draws by torch.randn; forward, log q and backward by autograd),
    (step)   one Adam step of the device loop (mivi_optimize_loop: STEPS steps per call, divided by STEPS).
Method: two device events around CALLS back-to-back calls on the context's stream after WARM warm-up calls, divided by CALLS (the step leg:
CALLS steps as CALLS / STEPS loop calls); REPEATS repeats per leg, alternating over the legs; the median is reported and the spread of the
repeats (max - min) next to it.  Every leg's call count is in its JSON line.
One JSON line per case; `python tools/flow_bench.py [out.jsonl]` appends them to the file as well (profiles/flow_bench.jsonl)."""
import json, math, statistics, sys
import numpy as np
sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
import torch
import advancedvi_jl_amd as avi

CALLS, WARM, REPEATS, STEPS = 200, 20, 3, 50
SHAPES = [(2, (16, 16), 3, 8), (64, (64, 64), 8, 4096)]


def timed(fn, calls=CALLS, warm=WARM):
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


def torch_nets(p, d, hidden, L):
    out = []
    for l, net, j, kind, off, shape in avi.flow_layout(d, hidden, L)[0]:
        n = int(np.prod(shape))
        v = p[off:off + n]
        if kind == "W":
            out.append([l, net, v.view(shape[1], shape[0]).t(), None])
        else:
            out[-1][3] = v
    return out


def torch_net(layers, c, tanh):
    h = c
    for k, (_, _, W, b) in enumerate(layers):
        h = W @ h + b[:, None]
        if k < len(layers) - 1:
            h = torch.nn.functional.leaky_relu(h, 0.01)
    return torch.tanh(h) if tanh else h


def torch_estimate(p, d, hidden, L, M, stl, mean, istd):
    """One estimate in torch: value and its gradient by autograd (sticking the landing: log q on detached parameters at z)."""
    p = p.detach().requires_grad_(True)
    A = [torch.arange(0 if l % 2 == 1 else 1, d, 2, device=p.device) for l in range(L + 1)]
    B = [torch.arange(1 if l % 2 == 1 else 0, d, 2, device=p.device) for l in range(L + 1)]
    eps = torch.randn(d, M, device=p.device, dtype=p.dtype)

    nets_p = torch_nets(p, d, hidden, L)
    nets_q = torch_nets(p.detach(), d, hidden, L) if stl else nets_p

    def layers(q, l, net):
        return [x for x in (nets_p if q is p else nets_q) if x[0] == l and x[1] == net]

    x = eps
    for l in range(1, L + 1):
        c = x[B[l]]
        y = x.clone()
        y[A[l]] = x[A[l]] * torch.exp(torch_net(layers(p, l, "s"), c, True)) + torch_net(layers(p, l, "t"), c, False)
        x = y
    z = x
    r = (z - mean[:, None]) * istd[:, None]
    ell = -0.5 * (r * r).sum(0)
    q = p.detach() if stl else p
    y, ssum = z, 0.0
    for l in range(L, 0, -1):
        c = y[B[l]]
        s = torch_net(layers(q, l, "s"), c, True)
        x = y.clone()
        x[A[l]] = (y[A[l]] - torch_net(layers(q, l, "t"), c, False)) * torch.exp(-s)
        y, ssum = x, ssum + s.sum(0)
    logq = -0.5 * (y * y).sum(0) - 0.5 * d * math.log(2 * math.pi) - ssum
    value = (-ell + logq).mean()
    (g,) = torch.autograd.grad(value, p)
    return value, g


def case(shape, ent, dt, sink=None):
    d, hidden, L, M = shape
    rng = np.random.default_rng(1)
    mean, std = rng.normal(size=d).astype(dt), rng.uniform(0.5, 2.0, size=d).astype(dt)
    q = avi.RealNVP(d, hidden, L, eltype=dt, rng=1)
    ctx = avi.MiviContext(dt, avi.REALNVP, d, M, ent.code, 1, flow=(hidden, L))
    ctx.set_problem(avi.DiagNormalProblem(mean, std))
    p = ctx.to_device(q.params)
    v, g = ctx.empty(1), ctx.empty(ctx.params_len)
    tm, ti = torch.tensor(mean, device=p.device), torch.tensor(1 / std, device=p.device)
    idx = [0]

    def flow():
        idx[0] += 1
        ctx.estimate_gradient(p, idx[0], v, g)

    def composed():
        torch_estimate(p, d, hidden, L, M, ent.code == 3, tm, ti)

    p_loop, state, elbo = p.clone(), ctx.empty(2 * ctx.params_len).zero_(), ctx.empty(STEPS)

    def steps():
        ctx.optimize_loop(p_loop, STEPS, 0, 0, rule=1, eta=1e-4, opt_state=state, elbo=elbo)

    legs = {"flow": (flow, CALLS, 1), "torch": (composed, CALLS, 1), "step": (steps, CALLS // STEPS, STEPS)}
    med = {k: [] for k in legs}
    for _ in range(REPEATS):
        for k, (fn, calls, per) in legs.items():
            med[k].append(timed(fn, calls, max(WARM // per, 2)) / per)
    rec = {"bench": "flow_estimate_gradient", "d": d, "hidden": list(hidden), "L": L, "M": M, "dtype": "f32" if dt == np.float32 else "f64",
           "entropy": type(ent).__name__, "params": ctx.params_len, "calls": {k: c * per for k, (_, c, per) in legs.items()}, "warmup": WARM, "repeats": REPEATS}
    for k in legs:
        rec[k + "_us"] = round(statistics.median(med[k]), 2)
        rec[k + "_spread_us"] = round(max(med[k]) - min(med[k]), 2)
    ctx.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


if __name__ == "__main__":
    sink = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
    for shape in SHAPES:
        for ent in (avi.MonteCarloEntropy(), avi.StickingTheLandingEntropy()):
            for dt in (np.float32, np.float64):
                case(shape, ent, dt, sink)
