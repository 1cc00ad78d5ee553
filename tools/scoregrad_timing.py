"""Microseconds per mivi_estimate_score_gradient call beside mivi_estimate_gradient with the sticking-the-landing estimator on the
same context shape (the same solve and the same VJP: the difference is the score route's own kernels and the fused routes it gives
up).  hipEvents around `--calls` calls after warm-up, `--repeats` repeats; prints one line per shape with the median and the spread.

    python tools/scoregrad_timing.py [--calls 200] [--repeats 3]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import advancedvi_jl_amd as avi  # noqa: E402


def time_calls(fn, calls, repeats, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    for name, family, d, M in (("full-rank d=1024 n_mc=256 f32 diag (north star)", avi.FULLRANK, 1024, 256),
                               ("mean-field d=1024 n_mc=256 f32 diag", avi.MEANFIELD, 1024, 256)):
        mu = rng.normal(size=d).astype(np.float32)
        if family == avi.MEANFIELD:
            q = avi.MeanFieldGaussian(mu, rng.uniform(0.5, 1.5, d).astype(np.float32))
        else:
            C = np.tril(rng.normal(size=(d, d)) * (0.3 / np.sqrt(d))).astype(np.float32)
            C[np.diag_indices(d)] = rng.uniform(0.5, 1.5, d)
            q = avi.FullRankGaussian(mu, C)
        params, _ = avi.destructure(q)
        ctx = avi.MiviContext(np.float32, family, d, M, avi.StickingTheLandingEntropy.code, 0x38BEF07CF9CC549D)
        ctx.set_problem(avi.DiagNormalProblem(np.full(d, 5.0, np.float32), np.ones(d, np.float32)))
        p = ctx.to_device(params)
        v, e, g = ctx.empty(1), ctx.empty(1), ctx.empty(ctx.params_len)
        idx = [0]

        def score():
            ctx.estimate_score_gradient(p, idx[0], v, e, g)
            idx[0] += 1

        def stl():
            ctx.estimate_gradient(p, idx[0], v, g)
            idx[0] += 1

        for label, fn in (("mivi_estimate_score_gradient", score), ("mivi_estimate_gradient (sticking the landing)", stl)):
            t = time_calls(fn, a.calls, a.repeats)
            ctx.synchronize()
            print(f"{name}: {label}: median {np.median(t):.1f} us/call, min {min(t):.1f}, max {max(t):.1f} ({a.repeats} x {a.calls} calls)")
        ctx.close()


if __name__ == "__main__":
    main()
