"""KLMinNaturalGradDescent steps on the north-star shape (d = 1024, n = 256, f32, dense-Gaussian target) and on the reference benchmark's
shape (d = 10, n = 1), both branches and both precision rules: microseconds per step, median over repeats of 100-step runs after a warm-up,
wall clock around a synchronised run (the protocol of tools/ngd_bench.py), all legs in one process.
    (a) mivi_natgrad_steps in 100-step calls
    (b) the same step composed from the estimator entry and torch on the device tensors (torch.linalg.cholesky, solve_triangular, matmuls),
        the reference's lines with the library's lower scale
    (c) the estimator entry alone
At d = 1024 two more legs split the update's share coarsely: (d) mivi_natgrad_update alone on fixed (g, H) and (e) mivi_natgrad_init alone (the
triangular inverse and two products of the same tile path, no factorisation).  The step size is 1e-3 at d = 10 and 1e-4 at d = 1024, where the
Stein branch's Hessian estimate from 256 draws would take S' out of the positive definite matrices at 1e-3; a flagged run is reported as such.
One JSON line per case; `python tools/natgrad_bench.py [small] [out.jsonl]` appends them to the file as well."""
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


def launches(d, ensure):
    nT = (d + 63) // 64
    return 1 if d <= avi.NATGRAD_SMALL_D else 3 * nT + 5 + (2 if ensure else 0)


def case(d, n, dtype, second, ensure, eta=1e-3, sink=None):
    from advancedvi_jl_amd._lib import MiviError
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    L = np.tril(np.eye(d) + 1.0 / (2 * d)).astype(dtype)
    prob = avi.DenseNormalProblem(np.full(d, 5, dtype), L, order=2 if second else 1)
    params, _ = avi.destructure(avi.FullRankGaussian(np.zeros(d, dtype), np.eye(d, dtype=dtype)))
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, n, 0, 1)
    ctx.set_problem(prob)
    p0 = ctx.to_device(params)
    p = p0.clone()
    s0 = ctx.natgrad_init(p0).clone()
    st = s0.clone()
    g, H, elbo = ctx.empty(d), ctx.empty(d * d), ctx.empty(STEPS)
    eye = torch.eye(d, dtype=tdt, device=p.device)
    ent0 = 0.5 * d * (1.0 + math.log(2.0 * math.pi))

    def herm(A):
        return torch.triu(A) + torch.triu(A, 1).t()

    def fused():
        p.copy_(p0)
        st.copy_(s0)
        ctx.natgrad_steps(p, st, 0, STEPS, eta, ensure, n_samples=n, second_order=second, elbo=elbo)

    def composed():
        p.copy_(p0)
        st.copy_(s0)
        for i in range(STEPS):
            logpi, gv, Hm = ctx.gauss_expected_grad_hess(p, i, 0, g, H, second_order=second)
            S, Sig = st[:d * d].view(d, d), st[d * d:].view(d, d)   # (symmetric: the column-major storage read row-major)
            if ensure:
                Gh = S + Hm
                S_new = herm(S - eta * Gh + (eta * eta / 2) * Gh @ Sig @ Gh)
            else:
                S_new = herm((1 - eta) * S - eta * Hm)
            Lr = torch.flip(torch.linalg.cholesky(torch.flip(S_new, (0, 1))), (0, 1)).t()   # S' = Lr' Lr, Lr lower triangular
            C_new = torch.linalg.solve_triangular(Lr, eye, upper=False)
            x = C_new @ (C_new.t() @ (-gv))
            p[:d] = p[:d] - eta * x
            p[d:] = C_new.t().reshape(-1)
            st[:d * d] = S_new.reshape(-1)
            st[d * d:] = (C_new @ C_new.t()).reshape(-1)
            elbo[i] = logpi[0] + ent0 + torch.log(torch.diagonal(C_new)).sum()

    def estimator():
        for i in range(STEPS):
            ctx.gauss_expected_grad_hess(p0, i, 0, g, H, second_order=second)

    def update_alone():
        p.copy_(p0)
        st.copy_(s0)
        for i in range(STEPS):
            ctx.natgrad_update(p, st, g, H, 0.0, ensure)   # (stepsize 0: the same launches and work, the state stays where it is)

    def init_alone():
        for i in range(STEPS):
            ctx.natgrad_init(p0, st)

    a = timed(fused)
    elbo_fused = float(elbo[-1].item())
    try:
        ctx.synchronize()
        flagged = 0
    except MiviError as e:
        flagged = e.status
    try:
        b = timed(composed)
    except Exception as e:   # torch.linalg.cholesky raises where the library flags
        b = (float("nan"),) * 3
        print(f"composed leg failed: {type(e).__name__}", file=sys.stderr)
    c = timed(estimator)
    extra = {}
    if d > avi.NATGRAD_SMALL_D:
        ctx.gauss_expected_grad_hess(p0, 0, 0, g, H, second_order=second)
        u, ini = timed(update_alone), timed(init_alone)
        extra = dict(update_alone_us=round(u[0], 2), init_alone_us=round(ini[0], 2))
    try:
        ctx.synchronize()
    except MiviError as e:
        flagged = flagged or e.status
    line = json.dumps(dict(d=d, n=n, dtype=np.dtype(dtype).name, branch="order2" if second else "stein", ensure_posdef=bool(ensure), steps_per_call=STEPS,
                           launches_per_update=launches(d, ensure), fused_us=round(a[0], 2), composed_us=round(b[0], 2), estimator_us=round(c[0], 2),
                           update_share_us=round(a[0] - c[0], 2), fused_min_max=[round(a[1], 2), round(a[2], 2)],
                           composed_min_max=[round(b[1], 2), round(b[2], 2)], estimator_min_max=[round(c[1], 2), round(c[2], 2)],
                           elbo_last_fused=elbo_fused, elbo_last_composed=float(elbo[-1].item()), stepsize=eta, status=flagged, **extra))
    print(line, flush=True)
    if sink:
        with open(sink, "a") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    small_only = "small" in args
    sink = next((a for a in args if a != "small"), None)
    for second in (False, True):
        for ensure in (True, False):
            case(10, 1, np.float32, second, ensure, sink=sink)
    if not small_only:
        for second in (False, True):
            for ensure in (True, False):
                case(1024, 256, np.float32, second, ensure, eta=1e-4, sink=sink)
