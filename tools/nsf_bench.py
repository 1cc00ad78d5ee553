"""Neural spline flow family: microseconds per mivi_estimate_gradient at (d, hidden, L, K, B, M) = (2, (16, 16), 3, 8, 30, 8) and
(64, (64, 64), 8, 8, 30, 4096), MonteCarloEntropy and StickingTheLandingEntropy, f32 and f64, diagonal-Gaussian target -- against, in the
same process on the same device,
    (torch)    the same estimate as eager torch autograd on device tensors (draws by torch.randn; the flow of tests/nsf_ref.py, which is
               written in torch operations alone, forward, log q through the inverse layers and backward by autograd),
    (realnvp)  mivi_estimate_gradient of the RealNVP family at the same (d, hidden, L, M).
Method (tools/flow_bench.py's): two device events around CALLS back-to-back calls on the context's stream after WARM warm-up calls, divided
by CALLS; REPEATS repeats per leg, alternating over the legs; the median is reported and the spread of the repeats (max - min) next to it.
One JSON line per case; `python tools/nsf_bench.py [out.jsonl]` appends them to the file as well (profiles/nsf_bench.jsonl)."""
import json, statistics, sys
import numpy as np
sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
import torch
import advancedvi_jl_amd as avi
from tests import nsf_ref as N

CALLS, WARM, REPEATS = 100, 10, 3
SHAPES = [(2, (16, 16), 3, 8, 30.0, 8), (64, (64, 64), 8, 8, 30.0, 4096)]


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


_MASKS = {}


def device_masks(d, l):
    """nsf_ref.masks as index tensors that stay on the device (the reference's numpy masks would cost a host copy per layer)"""
    if (d, l % 2) not in _MASKS:
        A = torch.arange(0 if l % 2 == 1 else 1, d, 2, device="cuda")
        _MASKS[(d, l % 2)] = (A, torch.arange(1 if l % 2 == 1 else 0, d, 2, device="cuda"))
    return _MASKS[(d, l % 2)]


N.masks = device_masks


def torch_estimate(p, arch, M, stl, mean, istd):
    """One estimate in torch: value and its gradient by autograd (sticking the landing: log q on detached parameters at z)."""
    p = p.detach().requires_grad_(True)
    eps = torch.randn(arch[0], M, device=p.device, dtype=p.dtype)
    z, _ = N.forward(p, arch, eps)
    r = (z - mean[:, None]) * istd[:, None]
    ell = -0.5 * (r * r).sum(0)
    value = (-ell + N.logpdf(p.detach() if stl else p, arch, z)).mean()
    (g,) = torch.autograd.grad(value, p)
    return value, g


def case(shape, ent, dt, sink=None):
    d, hidden, L, K, B, M = shape
    rng = np.random.default_rng(1)
    mean, std = rng.normal(size=d).astype(dt), rng.uniform(0.5, 2.0, size=d).astype(dt)
    q = avi.NeuralSplineFlow(d, hidden, K, B, L, eltype=dt, rng=1)
    ctx = avi.MiviContext(dt, avi.NSF, d, M, ent.code, 1, flow=(hidden, L, K, B))
    ctx.set_problem(avi.DiagNormalProblem(mean, std))
    p = ctx.to_device(q.params)
    v, g = ctx.empty(1), ctx.empty(ctx.params_len)
    tm, ti = torch.tensor(mean, device=p.device), torch.tensor(1 / std, device=p.device)
    rctx = avi.MiviContext(dt, avi.REALNVP, d, M, ent.code, 1, flow=(hidden, L))
    rctx.set_problem(avi.DiagNormalProblem(mean, std))
    rp = rctx.to_device(avi.RealNVP(d, hidden, L, eltype=dt, rng=1).params)
    rv, rg = rctx.empty(1), rctx.empty(rctx.params_len)
    idx = [0]

    def nsf():
        idx[0] += 1
        ctx.estimate_gradient(p, idx[0], v, g)

    def composed():
        torch_estimate(p, shape[:5], M, ent.code == 3, tm, ti)

    def realnvp():
        idx[0] += 1
        rctx.estimate_gradient(rp, idx[0], rv, rg)

    legs = {"nsf": nsf, "torch": composed, "realnvp": realnvp}
    med = {k: [] for k in legs}
    for _ in range(REPEATS):
        for k, fn in legs.items():
            med[k].append(timed(fn))
    rec = {"bench": "nsf_estimate_gradient", "d": d, "hidden": list(hidden), "L": L, "K": K, "B": B, "M": M, "dtype": "f32" if dt == np.float32 else "f64",
           "entropy": type(ent).__name__, "torch_masks": "device", "params": ctx.params_len, "realnvp_params": rctx.params_len, "calls": CALLS, "warmup": WARM, "repeats": REPEATS}
    for k in legs:
        rec[k + "_us"] = round(statistics.median(med[k]), 2)
        rec[k + "_spread_us"] = round(max(med[k]) - min(med[k]), 2)
    ctx.close()
    rctx.close()
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
