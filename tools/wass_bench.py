"""KLMinWassFwdBwd steps at d = 10, n = 1 and d = 1024, n = 256 (f32, dense-Gaussian target, both branches of the estimator): microseconds per
step, median over 9 repeats of 100-step runs after a warm-up, wall clock around a synchronised run (the protocol of tools/bam_bench.py), all
legs in one process.
    (a) mivi_wass_steps in 100-step calls
    (b) the same step composed from the estimator entry and torch in float64 on the device tensors: the LITERAL expression
        (torch.linalg.eigh of the d x d product, torch.linalg.cholesky, matmuls); at d >= 512 in 10-step runs (an eigh of that size takes
        long enough that 100-step runs would only repeat it)
    (c) the estimator entry alone
and (d) mivi_wass_update alone on the (g, H) of the first step, with the number of rounds the iteration takes on them -- counted by the same
iteration and stop rule restated in torch float64 (the library keeps the count on the device).  One JSON line per case;
`python tools/wass_bench.py [small] [out.jsonl]` appends them to the file as well."""
import json, statistics, sys, time
import numpy as np
sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
import torch
import advancedvi_jl_amd as avi

STEPS, REPEATS, WARM = 100, 9, 2
MAX_ROUNDS = 64   # MIVI_WASS_MAX_ROUNDS


def timed(fn, steps=STEPS):
    out = []
    for r in range(WARM + REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= WARM:
            out.append((time.perf_counter() - t0) / steps * 1e6)
    return statistics.median(out), min(out), max(out)


def herm(A):
    return torch.triu(A) + torch.triu(A, 1).t()


def rounds_of(Sig, Hm, eta):
    """The round the documented iteration stops at on these inputs (float64 torch; include/mivi.h, mivi_wass_update)."""
    d = Sig.shape[0]
    eye = torch.eye(d, dtype=torch.float64, device=Sig.device)
    M = eye + eta * Hm.t()
    Sh = herm(M @ Sig @ M.t())
    A = herm(Sh @ (Sh + 4 * eta * eye))
    Y, Z, r_prev = A / torch.linalg.norm(A), eye.clone(), float("inf")
    for k in range(MAX_ROUNDS):
        E = eye - Z @ Y
        r = float(torch.linalg.norm(E))
        if not np.isfinite(r) or r <= 64 * d * 2.0 ** -52 or (k >= 4 and (r >= r_prev or (r >= 0.5 * r_prev and r < 1e-6))):
            return k
        Y, Z, r_prev = Y + 0.5 * (Y @ E), Z + 0.5 * (E @ Z), r
    return MAX_ROUNDS


def case(d, n, second, eta, dtype=np.float32, sink=None):
    from advancedvi_jl_amd._lib import MiviError
    L = np.tril(np.eye(d) + 1.0 / (2 * d)).astype(dtype)
    prob = avi.DenseNormalProblem(np.full(d, 5, dtype), L, order=2 if second else 1)
    params, _ = avi.destructure(avi.FullRankGaussian(np.zeros(d, dtype), np.eye(d, dtype=dtype)))
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, n, 0, 1)
    ctx.set_problem(prob)
    p0 = ctx.to_device(params)
    p = p0.clone()
    s0 = ctx.wass_init(p0).clone()
    st = s0.clone()
    g, H, elbo = ctx.empty(d), ctx.empty(d * d), ctx.empty(STEPS)
    f64 = torch.float64
    eye = torch.eye(d, dtype=f64, device=p.device)
    eta_t = float(dtype(eta))
    composed_steps = STEPS if d < 512 else 10

    def fused():
        p.copy_(p0)
        st.copy_(s0)
        ctx.wass_steps(p, st, 0, STEPS, eta, n_samples=n, second_order=second, elbo=elbo)

    def composed():
        p.copy_(p0)
        st.copy_(s0)
        for i in range(composed_steps):
            _, gv, Hm = ctx.gauss_expected_grad_hess(p, i, 0, g, H, second_order=second)
            Sig = st.view(d, d).to(f64)
            M = eye + eta_t * Hm.to(f64).t()
            Sh = herm(M @ Sig @ M.t())
            w, U = torch.linalg.eigh(herm(Sh @ (Sh + 4 * eta_t * eye)))
            Sp = herm((Sh + 2 * eta_t * eye + (U * torch.sqrt(torch.clamp(w, min=0.0))) @ U.t()) / 2)
            p[:d] = (p[:d].to(f64) + eta_t * gv.to(f64)).to(p.dtype)
            p[d:] = torch.linalg.cholesky(Sp).t().reshape(-1).to(p.dtype)
            st.copy_(Sp.reshape(-1).to(p.dtype))

    def estimator():
        for i in range(STEPS):
            ctx.gauss_expected_grad_hess(p0, i, 0, g, H, second_order=second)

    def update_alone():
        for i in range(STEPS):
            p.copy_(p0)
            st.copy_(s0)
            ctx.wass_update(p, st, g, H, eta)

    a = timed(fused)
    last = float(elbo[-1].item())
    flagged = 0
    try:
        ctx.synchronize()
    except MiviError as e:
        flagged = e.status
    try:
        b = timed(composed, composed_steps)
    except Exception as e:   # torch.linalg.cholesky raises where the library flags
        b = (float("nan"),) * 3
        print(f"composed leg failed: {type(e).__name__}", file=sys.stderr)
    c = timed(estimator)
    _, _, Hm = ctx.gauss_expected_grad_hess(p0, 0, 0, g, H, second_order=second)
    rounds = rounds_of(s0.view(d, d).to(f64), Hm.to(f64), eta_t)
    upd = timed(update_alone)
    try:
        ctx.synchronize()
    except MiviError as e:
        flagged = flagged or e.status
    nT = (d + 63) // 64
    launches = 2 * nT + 2 * MAX_ROUNDS + 5
    line = json.dumps(dict(d=d, n=n, dtype=np.dtype(dtype).name, branch="order2" if second else "stein", stepsize=eta, steps_per_call=STEPS,
                           composed_steps_per_call=composed_steps, launches_per_update=launches, rounds=rounds, fused_us=round(a[0], 2),
                           composed_us=round(b[0], 2), estimator_us=round(c[0], 2), update_alone_us=round(upd[0], 2),
                           fused_min_max=[round(a[1], 2), round(a[2], 2)], composed_min_max=[round(b[1], 2), round(b[2], 2)],
                           estimator_min_max=[round(c[1], 2), round(c[2], 2)], update_min_max=[round(upd[1], 2), round(upd[2], 2)],
                           elbo_last=last, status=flagged))
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
        case(10, 1, second, 1e-3, sink=sink)
    if not small_only:
        for second in (False, True):
            case(1024, 256, second, 1e-3, sink=sink)
