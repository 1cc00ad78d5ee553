"""mivi_optimize_loop_many: the time of ONE call that runs K independent small fits, workgroup k = run k, against K sequential
mivi_optimize_loop calls (K <= 64; that code is the parent commit's, so it is the baseline), f32, STEPS iterations per call, at
    the reference benchmark's shape   full-rank d = 10, one sample per step, Adam(1e-3) + ClipScale, ClosedFormEntropy and
                                      StickingTheLandingEntropy, target N(5, I) (bench/benchmarks.jl:43-94); per run: seed, target
    the README regression             208 rows x 60 features, one sample per step, DoWG + ProximalLocationScaleEntropy + PolynomialAveraging
                                      (KLMinRepGradProxDescent's defaults), full-rank and mean-field; one shared X, per run: seed, y
for K in 1, 64, 256, 1024, 4096.  A figure is the time between two device events recorded on the context's stream around the whole call
(the upload of the runs' table, the launch, the ELBO records' conversion, the status read), the median of 25 calls (K <= 256; 7 beyond) after WARM warm-up
calls; `spread` = max - min of the repeats; `host_ms` the host clock around the same calls (they end in a device synchronise).  The
many-run and the sequential leg of a K alternate inside one process on one device.  One JSON line per (configuration, K);
`diverged_runs`
counts the runs of the last call whose status word is set (one-sample DoWG in f32 does diverge on some simulated data sets; such a run finishes its
steps carrying NaNs, so the call's time does not depend on it).  Then `avi.optimize_many` itself (records `optimize_many_python`, see bench_python): host time at K in 64, 256, 1024.
`python tools/many_bench.py [out.jsonl]` appends them to the file as well (profiles/many_bench.jsonl)."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import advancedvi_jl_amd as avi  # noqa: E402

STEPS, WARM = 256, 2
REPEATS_SMALL, REPEATS_LARGE = 25, 7   # calls per figure: K <= 256 (windows of 0.7-4 ms) and beyond
PY_KS, PY_REPEATS = (64, 256, 1024), 3
KS = (1, 64, 256, 1024, 4096)
SEQ_MAX_K = 64
ADAM, DOWG = 1, 3


def timed(fn):
    """(device ms between two events around fn(), host ms around it); fn ends in a device synchronise"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def bench_config(name, ctx, p0, rule, op, avg, eta, target_of, sink):
    plen = ctx.params_len
    for K in KS:
        seeds = np.arange(1, K + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15 & 0xFFFFFFFF)
        target = target_of(K)
        p_init = ctx.to_device(np.tile(p0, K))
        route, diverged = [None], [0]

        def state_of(p, runs):
            if rule == ADAM:
                return ctx.empty(2 * runs * plen).zero_()
            one = ctx.dog_state()
            ctx.dog_init(p[:plen], one, 1e-6)
            return one.repeat(runs)

        def many():
            p = p_init.clone()
            st = state_of(p, K)
            ap = p.clone() if avg else None
            elbo = ctx.empty(K * STEPS)
            torch.cuda.synchronize()
            status = None

            def call():
                nonlocal status
                status = ctx.optimize_loop_many(p, K, STEPS, 0, 0, seeds=seeds, rule=rule, op=op, averager=avg, eta=eta, clip_epsilon=1e-5,
                                                opt_state=st, avg_params=ap, elbo=elbo, **target)
            out = timed(call)
            route[0] = ctx.last_loop()
            diverged[0] = int(np.count_nonzero(status))   # (a diverged run finishes its steps carrying NaNs: the call's time does not depend on it)
            assert diverged[0] < K and np.isfinite(elbo.cpu().numpy().reshape(K, STEPS)[status == 0, 0]).all()
            return out

        def sequential():
            ps = [p_init[:plen].clone() for _ in range(K)]
            sts = [state_of(p, 1) for p in ps]
            aps = [p.clone() if avg else None for p in ps]
            elbos = [ctx.empty(STEPS) for _ in range(K)]
            torch.cuda.synchronize()

            def call():
                for k in range(K):
                    ctx.optimize_loop(ps[k], STEPS, 0, 0, rule=rule, op=op, averager=avg, eta=eta, clip_epsilon=1e-5, opt_state=sts[k],
                                      avg_params=aps[k], elbo=elbos[k])
            return timed(call)

        legs = {"many": many}
        if K <= SEQ_MAX_K:
            legs["sequential"] = sequential
        res = {k: [] for k in legs}
        REPEATS = REPEATS_SMALL if K <= 256 else REPEATS_LARGE
        for i in range(WARM + REPEATS):
            for k, fn in legs.items():
                r = fn()
                if i >= WARM:
                    res[k].append(r)
        rec = {"bench": "optimize_many", "config": name, "dtype": "f32", "K": K, "steps": STEPS, "warm": WARM, "repeats": REPEATS,
               "route": route[0], "diverged_runs": diverged[0]}
        for k, rs in res.items():
            dev = [r[0] for r in rs]
            rec[k + "_ms"] = round(statistics.median(dev), 4)
            rec[k + "_spread_ms"] = round(max(dev) - min(dev), 4)
            rec[k + "_host_ms"] = round(statistics.median(r[1] for r in rs), 4)
        rec["many_us_per_run_step"] = round(rec["many_ms"] * 1e3 / (K * STEPS), 4)
        emit(rec, sink)


def emit(rec, sink):
    line = json.dumps(rec)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


def bench_python(name, alg, probs_of, q0, sink):
    """avi.optimize_many itself -- what a user of the Python mirror calls: the host clock around a call of STEPS iterations from scratch
    (it creates the K states: one context per run) and around a second, warm-started call (states=: packing, the launch, the copy-back,
    `info`), beside K sequential `optimize` calls at K = 64; median of PY_REPEATS."""
    for K in PY_KS:
        probs = probs_of(K)
        res = {"many_cold": [], "many_warm": [], "sequential_cold": [], "sequential_warm": []}
        for _ in range(PY_REPEATS):
            rngs = [avi.PhiloxRNG(1000 + k) for k in range(K)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = avi.optimize_many(rngs, alg, STEPS, probs, q0)
            t1 = time.perf_counter()
            out2 = avi.optimize_many(rngs, alg, STEPS, probs, None, states=[o[2] for o in out])
            t2 = time.perf_counter()
            res["many_cold"].append((t1 - t0) * 1e3)
            res["many_warm"].append((t2 - t1) * 1e3)
            route = avi._optimize._ctx_of(out2[0][2]["obj_st"]).last_loop()
            for o in out2:
                avi._optimize._ctx_of(o[2]["obj_st"]).close()
            if K <= SEQ_MAX_K:
                rngs = [avi.PhiloxRNG(1000 + k) for k in range(K)]
                t0 = time.perf_counter()
                out = [avi.optimize(rngs[k], alg, STEPS, probs[k], q0) for k in range(K)]
                t1 = time.perf_counter()
                out2 = [avi.optimize(rngs[k], alg, STEPS, probs[k], None, state=out[k][2]) for k in range(K)]
                t2 = time.perf_counter()
                res["sequential_cold"].append((t1 - t0) * 1e3)
                res["sequential_warm"].append((t2 - t1) * 1e3)
                for o in out2:
                    avi._optimize._ctx_of(o[2]["obj_st"]).close()
        rec = {"bench": "optimize_many_python", "config": name, "dtype": "f32", "K": K, "steps": STEPS, "repeats": PY_REPEATS, "route": route}
        for k, v in res.items():
            if v:
                rec[k + "_host_ms"] = round(statistics.median(v), 3)
                rec[k + "_spread_ms"] = round(max(v) - min(v), 3)
        emit(rec, sink)


def main(sink):
    f32 = np.float32
    # the reference benchmark: normal(n_dims = 10) with mean 5, full-rank, one sample, Adam(1e-3), ClipScale
    d = 10
    for ent_name, ent in (("closed-form", avi.ClosedFormEntropy.code), ("sticking-the-landing", avi.StickingTheLandingEntropy.code)):
        ctx = avi.MiviContext(f32, avi.FULLRANK, d, 1, ent, 3)
        ctx.set_problem(avi.DiagNormalProblem(np.full(d, 5.0, f32), np.ones(d, f32)))
        p0 = avi.destructure(avi.FullRankGaussian(np.zeros(d, f32), np.eye(d, dtype=f32)))[0]
        bench_config(f"fullrank d=10 n_mc=1 Adam+ClipScale {ent_name}", ctx, p0, ADAM, 1, 0, 1e-3,
                     lambda K: dict(means=np.full((K, d), 5.0, f32), stds=np.ones((K, d), f32)), sink)
        ctx.close()
    # the README regression: 208 x 60, theta = [beta; sigma], one sample, the proximal algorithm's defaults
    n, p = 208, 60
    rng = np.random.default_rng(7)
    X = (rng.normal(size=(n, p)) / np.sqrt(p)).astype(f32)   # (logits of order one)
    beta = rng.normal(size=p) * 0.5
    prob = avi.LogRegProblem(X, (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-X.astype(np.float64) @ beta))).astype(np.uint8), variant="lognormal_exp_bijector")
    for fam_name, fam in (("fullrank", avi.FULLRANK), ("meanfield", avi.MEANFIELD)):
        ctx = avi.MiviContext(f32, fam, p + 1, 1, avi.ClosedFormEntropyZeroGradient.code, 3)
        ctx.set_problem(prob)
        q0 = (avi.FullRankGaussian(np.zeros(p + 1, f32), (0.5 * np.eye(p + 1)).astype(f32)) if fam == avi.FULLRANK
              else avi.MeanFieldGaussian(np.zeros(p + 1, f32), np.full(p + 1, 0.5, f32)))
        ys = {}

        def target_of(K, ys=ys, ctx=ctx):
            if K not in ys:   # per-run labels (one data set simulated from the model per run: beta ~ N(0, 0.25 I)), the context's X for every run
                r = np.random.default_rng(K)
                logits = (r.normal(size=(K, p)) * 0.5) @ X.astype(np.float64).T
                ys[K] = torch.as_tensor((r.uniform(size=(K, n)) < 1.0 / (1.0 + np.exp(-logits))).astype(np.uint8)).to(ctx.tdevice)
            return dict(y=ys[K])
        bench_config(f"logreg 208x60 n_mc=1 DoWG+prox+averaging {fam_name}", ctx, avi.destructure(q0)[0], DOWG, 2, 1, 0.0, target_of, sink)
        ctx.close()
    # the Python mirror's optimize_many on the two shapes
    import warnings
    warnings.simplefilter("ignore")
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), n_samples=1, optimizer=avi.Adam(1e-3), operator=avi.ClipScale(), averager=avi.NoAveraging())
    bench_python("fullrank d=10 n_mc=1 Adam+ClipScale closed-form", alg,
                 lambda K: [avi.DiagNormalProblem(np.full(d, 5.0, f32), np.ones(d, f32)) for _ in range(K)],
                 avi.FullRankGaussian(np.zeros(d, f32), np.eye(d, dtype=f32)), sink)
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), n_samples=1, optimizer=avi.Adam(1e-2), operator=avi.ClipScale(), averager=avi.PolynomialAveraging())

    def regressions(K):
        r = np.random.default_rng(K)
        logits = (r.normal(size=(K, p)) * 0.5) @ X.astype(np.float64).T
        ys = (r.uniform(size=(K, n)) < 1.0 / (1.0 + np.exp(-logits))).astype(np.uint8)
        return [avi.LogRegProblem(X, ys[k], variant="lognormal_exp_bijector") for k in range(K)]
    bench_python("logreg 208x60 n_mc=1 Adam+ClipScale+averaging meanfield", alg, regressions,
                 avi.MeanFieldGaussian(np.zeros(p + 1, f32), np.full(p + 1, 0.5, f32)), sink)


if __name__ == "__main__":
    main(open(sys.argv[1], "a") if len(sys.argv) > 1 else None)
