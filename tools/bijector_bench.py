"""mivi_estimate_gradient behind a Stacked bijector at d = 1024, M = 256, f32, diagonal-Gaussian target, mean-field and full-rank, for four
bijectors over all 1024 coordinates:
    exp        one exp block                      (mivi_set_bijector_stacked: k_bij_fwd / k_bij_bwd, the legacy kernels)
    lower      the same coordinates as truncated(0.5, inf)   (kernels_bijector.hip from here on)
    two_sided  truncated(-1, 2)
    ordered    one ordered block of 1024 (the segmented scan across four 256-row chunks)
Every figure is the median of CALLS single calls, each timed by a host clock around {call, device synchronise}, after WARM warm-up calls,
over ROUNDS rounds; `spread_us` = max - min of the round medians.  There is no gate on these numbers: nobody had measured the kernels.
The `exp` line launches exactly what it launched before the new kinds existed, so it is the A/B line: `--lib PATH` times another build of
libmivi.so (one without the new entries takes `--legacy-only`) in a process of its own on the same box.
One JSON line per case; `python tools/bijector_bench.py [--lib PATH] [--legacy-only] [--tag NAME] [out.jsonl|-] [calls]` appends them to
the file as well (profiles/bijector_bench.jsonl).  `lib` in a line is the --tag (default `tree`: the library built in this tree), `note`
says what was timed: every line is ONE process on ONE box, and lines are comparable only with the lines of the same session."""
import json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

args = sys.argv[1:]
LIB = args.pop(args.index("--lib") + 1) if "--lib" in args else None
TAG = args.pop(args.index("--tag") + 1) if "--tag" in args else "tree"
LEGACY_ONLY = "--legacy-only" in args
args = [a for a in args if a not in ("--lib", "--tag", "--legacy-only")]

from advancedvi_jl_amd import _lib  # noqa: E402
if LIB:
    _lib.LIB_PATH = os.path.abspath(LIB)
    if LEGACY_ONLY:   # a build from before the new entries: bind what it exports
        for name in ("mivi_set_bijector_stacked_ex", "mivi_sample_constrained", "mivi_logpdf_constrained", "mivi_logpdf_constrained_host"):
            _lib.SIGNATURES.pop(name, None)
import torch  # noqa: E402
import advancedvi_jl_amd as avi  # noqa: E402

D, M, WARM, ROUNDS = 1024, 256, 20, 5
CALLS = int(args[1]) if len(args) > 1 else 200
BIJECTORS = {
    "exp": [(0, D, "exp")],
    "lower": [(0, D, "truncated", (0.5, np.inf))],
    "two_sided": [(0, D, "truncated", (-1.0, 2.0))],
    "ordered": [(0, D, "ordered")],
}


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


def case(family, name, sink=None):
    rng = np.random.default_rng(1)
    dt = np.float32
    mu = (0.1 * rng.normal(size=D)).astype(dt)
    if name == "ordered":
        mu[1:] -= dt(3.0)   # increments e^eta ~ 0.05: x stays O(50) over 1024 rows
    if family == "meanfield":
        q = avi.MeanFieldGaussian(mu, rng.uniform(0.1, 0.3, size=D).astype(dt))
    else:
        C = np.tril(rng.normal(size=(D, D)) * (0.1 / np.sqrt(D)), -1).astype(dt) + np.diag(rng.uniform(0.1, 0.3, size=D).astype(dt))
        q = avi.FullRankGaussian(mu, C)
    params, _ = avi.destructure(q)
    ctx = avi.MiviContext(dt, q.family, D, M, 0, 1)
    ctx.set_problem(avi.TransformedProblem(avi.DiagNormalProblem(np.ones(D, dt), np.full(D, 2.0, dt)), avi.StackedBijector(BIJECTORS[name])))
    p, v, g = ctx.to_device(params), ctx.empty(1), ctx.empty(ctx.params_len)
    idx = [0]

    def call():
        idx[0] += 1
        ctx.estimate_gradient(p, idx[0], v, g)

    med = [timed(call) for _ in range(ROUNDS)]
    ctx.synchronize()
    assert np.isfinite(float(v.item())) and bool(torch.isfinite(g).all())
    ctx.close()
    rec = {"bench": "bijector", "lib": TAG, "family": family, "bijector": name, "d": D, "M": M, "dtype": "f32", "calls": CALLS, "rounds": ROUNDS,
           "us": round(statistics.median(med), 2), "spread_us": round(max(med) - min(med), 2), "boxes": 1,
           "note": "measured on one box; " + (f"--lib {os.path.basename(LIB)}" if LIB else "the tree's libmivi.so") + (", --legacy-only (exp line alone)" if LEGACY_ONLY else "")}
    line = json.dumps(rec)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


if __name__ == "__main__":
    sink = open(args[0], "a") if args and args[0] != "-" else None
    for family in ("meanfield", "fullrank"):
        for name in (("exp",) if LEGACY_ONLY else tuple(BIJECTORS)):
            case(family, name, sink)
