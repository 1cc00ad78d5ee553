"""Subsampled optimisation of the built-in logistic regression: microseconds per step of `optimize(..., subsampling=...)`, and per single
estimate on a batch of the resident schedule, f32, at the minibatch shapes (n, p, batch, n_mc)
    (10^5, 64, 256, 8)      mean-field and full-rank
    (2 10^5, 511, 4096, 16) full-rank.
Legs of a case, alternating over ROUNDS rounds in one process on one device:
    default     optimize as a user calls it (the device loop over a resident schedule, kernels by size; on a tree without the schedule
                entries -- the parent commit -- this is the host-driven loop, and it is the only leg: run the tool there for the baseline)
    fused       the device loop with the fused minibatch kernel forced (kernels = 1)
    gather      the device loop with the device gather + the resident-data kernels forced (kernels = 2)
    host        device_loop=False: mivi_logreg_select_rows + the single entries, one host round trip per step
A leg's figure: a warm-up call of WARM steps (it records the graphs and fills the caches), then the host clock around a warm-started
`optimize` of STEPS more steps (it ends in a device-to-host copy), over STEPS; the median over the rounds, `spread` = max - min of them.
estimate_fused / estimate_gather: the median of CALLS single mivi_estimate_gradient calls on batch 1 of a planned schedule, each timed by
a host clock around {call, device synchronise}.  One JSON line per case; `python tools/subsample_bench.py [out.jsonl]` appends them to the
file as well (profiles/subsample_bench.jsonl)."""
import json, statistics, sys, time
import numpy as np
sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
import torch
import advancedvi_jl_amd as avi

OPT = avi._optimize
HAS_SCHEDULE = hasattr(OPT, "SUBSAMPLED_KERNELS")
WARM, STEPS, ROUNDS, CALLS = 256, 512, 3, 200
CASES = [(100_000, 64, 256, 8, "meanfield"), (100_000, 64, 256, 8, "fullrank"), (200_000, 511, 4096, 16, "fullrank")]


def problem(n, p):
    rng = np.random.default_rng(7)
    X = np.empty((n, p), dtype=np.float32, order="F")
    for k in range(p):   # (column by column: no float64 copy of the whole matrix)
        X[:, k] = rng.normal(size=n) / np.sqrt(p)
    y = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    return avi.LogRegProblem(X, y)


def family(d, fam):
    mu = np.zeros(d, np.float32)
    return avi.MeanFieldGaussian(mu, np.full(d, 0.3, np.float32)) if fam == "meanfield" else avi.FullRankGaussian(mu, (0.3 * np.eye(d)).astype(np.float32))


def leg_us_per_step(prob, q0, alg, kernels, device_loop):
    if HAS_SCHEDULE:
        OPT.SUBSAMPLED_KERNELS = kernels
    rng = avi.PhiloxRNG(3)
    _, _, state = avi.optimize(rng, alg, WARM, prob, q0, device_loop=device_loop)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, info, state = avi.optimize(rng, alg, STEPS, prob, None, state=state, device_loop=device_loop)
    torch.cuda.synchronize()
    us = (time.perf_counter() - t0) * 1e6 / STEPS
    ctx = OPT._ctx_of(state["obj_st"])
    route = ctx.batch_route() if HAS_SCHEDULE else 0
    assert np.isfinite(info[-1]["elbo"])
    ctx.close()
    return us, route


def estimate_us(prob, q0, n, batch, n_mc, kernels):
    ctx = avi.MiviContext(np.float32, q0.family, len(q0), n_mc, 0, 3)
    ctx.set_problem(prob)
    rows = np.random.default_rng(5).permutation(n)[:4 * batch].reshape(4, batch)
    ctx.set_batch_schedule(rows, kernels=kernels)
    ctx.seek_batch(1)
    assert ctx.batch_route() == kernels
    p = ctx.to_device(avi.destructure(q0)[0])
    v, g = ctx.empty(1), ctx.empty(ctx.params_len)
    out = []
    for i in range(20 + CALLS):
        t0 = time.perf_counter()
        ctx.estimate_gradient(p, 1 + i, v, g)
        torch.cuda.synchronize()
        if i >= 20:
            out.append((time.perf_counter() - t0) * 1e6)
    ctx.close()
    return statistics.median(out)


def case(n, p, batch, n_mc, fam, sink=None):
    prob, q0 = problem(n, p), family(p + 1, fam)
    sub = avi.ReshufflingBatchSubsampling(np.arange(n), batch)
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), n_samples=n_mc, optimizer=avi.Adam(1e-3), operator=avi.ClipScale(), averager=avi.PolynomialAveraging(),
                                  subsampling=sub)
    legs = {"default": (0, True)}
    if HAS_SCHEDULE:
        legs.update({"fused": (1, True), "gather": (2, True), "host": (0, False)})
    med, routes = {k: [] for k in legs}, {}
    for _ in range(ROUNDS):
        for k, (kernels, dev) in legs.items():
            us, routes[k] = leg_us_per_step(prob, q0, alg, kernels, dev)
            med[k].append(us)
    rec = {"bench": "subsampled_optimize", "tree": "schedule" if HAS_SCHEDULE else "parent", "n": n, "p": p, "batch": batch, "n_mc": n_mc, "family": fam,
           "dtype": "f32", "warm": WARM, "steps": STEPS, "rounds": ROUNDS}
    for k in legs:
        rec[k + "_us_per_step"] = round(statistics.median(med[k]), 2)
        rec[k + "_spread_us"] = round(max(med[k]) - min(med[k]), 2)
    if HAS_SCHEDULE:
        rec["default_route"] = routes["default"]
        rec["estimate_fused_us"] = round(estimate_us(prob, q0, n, batch, n_mc, 1), 2)
        rec["estimate_gather_us"] = round(estimate_us(prob, q0, n, batch, n_mc, 2), 2)
    line = json.dumps(rec)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


if __name__ == "__main__":
    sink = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
    for c in CASES:
        case(*c, sink=sink)
