"""mivi_logpdf at d = 1024, f32, for n = 256 and n = 16384 points, on the three families (low-rank: r = 16), beside the same quantity from
torch on the same GPU:
    (mivi)    MiviContext.logpdf into preallocated outputs, log q alone (no std),
    (torch)   full-rank: torch.linalg.solve_triangular(C, Z - mu, upper=False), then -(0.5 sum u^2 + d/2 log 2 pi) - sum log diag C;
              mean-field: (Z - mu) / sigma and the same reductions; low-rank: the Woodbury form with torch products and a
              cholesky_solve on the r x r matrix -- the composition a user would write without this entry.
Every figure is the median of CALLS single calls, each timed by a host clock around {call, device synchronise}, after WARM warm-up calls;
the two legs of a case alternate over ROUNDS rounds, `*_spread_us` = max - min of a leg's round medians.  `rel_diff` is the largest
|mivi - torch| / max(|torch|, d) over the points: the two legs compute the same thing.
One JSON line per case; `python tools/logpdf_bench.py [out.jsonl|-] [calls]` appends them to the file as well (profiles/logpdf_bench.jsonl)."""
import json, math, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import advancedvi_jl_amd as avi

D, RANK, WARM, ROUNDS = 1024, 16, 10, 3
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 100
LOG2PI = math.log(2.0 * math.pi)


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out)


def family_of(name, rng):
    dt = np.float32
    mu = rng.normal(size=D).astype(dt)
    if name == "meanfield":
        return avi.MeanFieldGaussian(mu, rng.uniform(0.5, 1.5, size=D).astype(dt))
    if name == "fullrank":
        C = np.tril(rng.normal(size=(D, D)) * (0.3 / np.sqrt(D)), -1).astype(dt) + np.diag(rng.uniform(0.5, 1.5, size=D).astype(dt))
        return avi.FullRankGaussian(mu, C)
    return avi.LowRankGaussian(mu, rng.uniform(0.5, 1.5, size=D).astype(dt), (0.7 * rng.normal(size=(D, RANK))).astype(dt))


def torch_leg(name, q, Z):
    """() -> log q (n) of the columns of the device tensor Z (d, n) by torch alone"""
    dev = Z.device
    mu = torch.as_tensor(q.location, device=dev)[:, None]
    if name == "meanfield":
        sig = torch.as_tensor(q.scale, device=dev)[:, None]
        cst = -0.5 * D * LOG2PI - float(np.log(q.scale.astype(np.float64)).sum())
        return lambda: -0.5 * (((Z - mu) / sig) ** 2).sum(dim=0) + cst
    if name == "fullrank":
        C = torch.as_tensor(q.scale, device=dev)
        cst = -0.5 * D * LOG2PI - float(np.log(np.diag(q.scale).astype(np.float64)).sum())
        return lambda: -0.5 * (torch.linalg.solve_triangular(C, Z - mu, upper=False) ** 2).sum(dim=0) + cst
    Dg, U = torch.as_tensor(q.scale_diag, device=dev)[:, None], torch.as_tensor(q.scale_factors, device=dev)

    def lowrank():   # the parameter-only part (A, its factor, the log-determinants) is part of the call, as it is of mivi_logpdf
        W = U / Dg
        L = torch.linalg.cholesky(torch.eye(RANK, device=dev) + W.T @ W)
        t = (Z - mu) / Dg
        s = W.T @ t
        quad = (t * t).sum(dim=0) - (s * torch.cholesky_solve(s, L)).sum(dim=0)
        return -0.5 * quad - 0.5 * D * LOG2PI - torch.log(Dg).sum() - torch.log(torch.diagonal(L)).sum()
    return lowrank


def case(name, n, sink=None):
    rng = np.random.default_rng(1)
    q = family_of(name, rng)
    params, _ = avi.destructure(q)
    ctx = avi.MiviContext(np.float32, q.family, D, 256, 0, 1, rank=getattr(q, "rank", 0))
    p = ctx.to_device(params)
    Z = ctx.to_device((q.location[:, None] + 2.0 * rng.normal(size=(D, n))).astype(np.float32).T).t()   # (d, n) view of column-major storage
    out = ctx.empty(n)
    ref = torch_leg(name, q, Z)
    legs = {"mivi": lambda: ctx.logpdf(p, Z, out=out), "torch": ref}
    med = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            med[k].append(timed(fn))
    ctx.logpdf(p, Z, out=out)
    ctx.synchronize()
    a, b = out.double().cpu().numpy(), ref().double().cpu().numpy()
    rec = {"bench": "logpdf", "family": name, "d": D, "n": n, "dtype": "f32", "calls": CALLS, "rounds": ROUNDS,
           "rel_diff": float(np.max(np.abs(a - b) / np.maximum(np.abs(b), D)))}
    if name == "lowrank":
        rec["rank"] = RANK
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
    sink = open(sys.argv[1], "a") if len(sys.argv) > 1 and sys.argv[1] != "-" else None
    for name in ("meanfield", "fullrank", "lowrank"):
        for n in (256, 16384):
            case(name, n, sink)
