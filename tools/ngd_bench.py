"""KLMinSqrtNaturalGradDescent steps on the north-star shape (d = 1024, n = 256, f32, dense-Gaussian target) and on the reference benchmark's
shape (d = 10, n = 1): microseconds per step, median over repeats of 100-step runs after a warm-up, wall clock around a synchronised run.
    (a) mivi_sqrt_ngd_steps in 100-step calls
    (b) the same step composed on the public API that existed before the update kernels: the estimator entry + the update written with torch
        matmuls on the device tensors
    (c) the estimator entry alone
One JSON line per case."""
import json, math, statistics, sys, time
import numpy as np
sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
import torch
import advancedvi_jl_amd as avi

STEPS, REPEATS, WARM = 100, 9, 2


def timed(fn):
    out = []
    for r in range(WARM + REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= WARM:
            out.append((time.perf_counter() - t0) / STEPS * 1e6)
    return statistics.median(out), min(out), max(out)


def case(d, n, dtype, second, eta=1e-3):
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    L = np.tril(np.eye(d) + 1.0 / (2 * d)).astype(dtype)
    prob = avi.DenseNormalProblem(np.full(d, 5, dtype), L, order=2 if second else 1)
    params, _ = avi.destructure(avi.FullRankGaussian(np.zeros(d, dtype), np.eye(d, dtype=dtype)))
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, n, 0, 1)
    ctx.set_problem(prob)
    p0 = ctx.to_device(params)
    p = p0.clone()
    g, H, elbo = ctx.empty(d), ctx.empty(d * d), ctx.empty(STEPS)
    eye = torch.eye(d, dtype=tdt, device=p.device)
    ent0 = 0.5 * d * (1.0 + math.log(2.0 * math.pi))

    def fused():
        p.copy_(p0)
        ctx.sqrt_ngd_steps(p, 0, STEPS, eta, n_samples=n, second_order=second, elbo=elbo)

    def composed():
        p.copy_(p0)
        for i in range(STEPS):
            logpi, gv, Hm = ctx.gauss_expected_grad_hess(p, i, 0, g, H, second_order=second)
            C = p[d:].view(d, d).t()
            A = C.t() @ (-Hm) @ C - eye
            T = torch.tril(A) - torch.diag(torch.diagonal(A)) / 2
            m_new = p[:d] - eta * (C @ (C.t() @ (-gv)))
            C_new = C - eta * (C @ T)
            p[:d] = m_new
            p[d:] = C_new.t().reshape(-1)
            elbo[i] = logpi[0] + ent0 + torch.log(torch.diagonal(C_new)).sum()

    def estimator():
        for i in range(STEPS):
            ctx.gauss_expected_grad_hess(p0, i, 0, g, H, second_order=second)

    a, b, c = timed(fused), timed(composed), timed(estimator)
    ctx.synchronize()
    print(json.dumps(dict(d=d, n=n, dtype=np.dtype(dtype).name, branch="order2" if second else "stein", steps_per_call=STEPS,
                          fused_us=round(a[0], 2), composed_us=round(b[0], 2), estimator_us=round(c[0], 2), update_share_us=round(a[0] - c[0], 2),
                          fused_min_max=[round(a[1], 2), round(a[2], 2)], composed_min_max=[round(b[1], 2), round(b[2], 2)],
                          estimator_min_max=[round(c[1], 2), round(c[2], 2)], elbo_last=float(elbo[-1].item()))), flush=True)
    ctx.close()


if __name__ == "__main__":
    small_only = len(sys.argv) > 1 and sys.argv[1] == "small"
    if not small_only:
        for second in (False, True):
            case(1024, 256, np.float32, second)
    for dtype in (np.float32, np.float64):
        for second in (False, True):
            case(10, 1, dtype, second)
