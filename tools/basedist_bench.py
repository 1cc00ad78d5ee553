"""Base distributions of the full-rank family: microseconds per mivi_estimate_gradient at d = 1024, M = 256, f32, diagonal-Gaussian target,
closed-form and sticking-the-landing entropy, for
    (normal)   Normal() on the first-generation kernels (MIVI_FR_GEN1=1, set below before the library is loaded: the route a non-normal
               base takes is built from those kernels; the default Gaussian route at this shape is the second-generation one),
    (laplace)  Laplace(),
    (tdist3)   TDist(3),
and the draw stage alone through mivi_sample's draw + product on a mean-field context of the same shape (`sample_mf_*`: the draw kernel and
one elementwise pass).  Every figure is the median of CALLS single calls, each timed by a host clock around {call, device synchronise},
after WARM warm-up calls; the legs of a case alternate over ROUNDS rounds, `*_spread_us` = max - min of a leg's round medians.
The draw kernel's OWN time is a kernel time: take it from `rocprofv3 --kernel-trace --stats -- python tools/basedist_bench.py - 20` (a run of
its own, 20 calls per leg; kernels k_bd_draw<float, 1> = Laplace, <float, 2> = TDist, k_eps<float> = the normal draw).
One JSON line per case; `python tools/basedist_bench.py [out.jsonl|-] [calls]` appends them to the file as well (profiles/basedist_bench.jsonl)."""
import json, os, statistics, sys, time
os.environ["MIVI_FR_GEN1"] = "1"
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import advancedvi_jl_amd as avi

D, M, WARM, ROUNDS = 1024, 256, 20, 3
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 200
BASES = {"normal": avi.Normal(), "laplace": avi.Laplace(), "tdist3": avi.TDist(3.0)}
# the draw stage per element: bytes written (U, U^T; + the -psi(U) plane for the sticking-the-landing kinds) and
# transcendental evaluations (the Monte-Carlo entropy's log1p included for TDist)
DRAW_BYTES = {"closed": 8, "stl": 12}
DRAW_TRANSCENDENTALS = {"normal": 2.0, "laplace": 1.0, "tdist3": 5.0}   # Box-Muller: (log, sqrt, sin, cos) per PAIR


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


def case(ent, sink=None):
    dt = np.float32
    rng = np.random.default_rng(1)
    prob = avi.DiagNormalProblem(rng.normal(size=D).astype(dt), rng.uniform(0.5, 2.0, size=D).astype(dt))
    C = np.tril(rng.normal(size=(D, D)) * (0.3 / np.sqrt(D)), -1).astype(dt) + np.diag(rng.uniform(0.5, 1.5, size=D).astype(dt))
    params, _ = avi.destructure(avi.FullRankGaussian(rng.normal(size=D).astype(dt), C))
    params_mf = np.concatenate([params[:D], np.diag(C)]).astype(dt)
    legs, keep = {}, []
    idx = [0]
    for name, dist in BASES.items():
        ctx = avi.MiviContext(dt, avi.FULLRANK, D, M, ent.code, 1)
        ctx.set_base_dist(dist)
        ctx.set_problem(prob)
        p, v, g = ctx.to_device(params), ctx.empty(1), ctx.empty(ctx.params_len)
        mf = avi.MiviContext(dt, avi.MEANFIELD, D, M, ent.code, 1)
        mf.set_base_dist(dist)
        pm = mf.to_device(params_mf)
        keep += [ctx, mf]

        def estimate(ctx=ctx, p=p, v=v, g=g):
            idx[0] += 1
            ctx.estimate_gradient(p, idx[0], v, g)

        def sample_mf(mf=mf, pm=pm):
            idx[0] += 1
            mf.sample(pm, idx[0])

        legs[name] = estimate
        legs["sample_mf_" + name] = sample_mf
    med = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            med[k].append(timed(fn))
    kind = "stl" if ent.code == 3 else "closed"
    rec = {"bench": "basedist_estimate_gradient", "d": D, "M": M, "dtype": "f32", "target": "diag", "family": "fullrank",
           "entropy": type(ent).__name__, "calls": CALLS, "rounds": ROUNDS, "normal_route": "first generation (MIVI_FR_GEN1=1)",
           "draw_bytes_per_element": DRAW_BYTES[kind], "draw_transcendentals_per_element": DRAW_TRANSCENDENTALS}
    for k in legs:
        rec[k + "_us"] = round(statistics.median(med[k]), 2)
        rec[k + "_spread_us"] = round(max(med[k]) - min(med[k]), 2)
    for c in keep:
        c.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


if __name__ == "__main__":
    sink = open(sys.argv[1], "a") if len(sys.argv) > 1 and sys.argv[1] != "-" else None
    for ent in (avi.ClosedFormEntropy(), avi.StickingTheLandingEntropy()):
        case(ent, sink)
