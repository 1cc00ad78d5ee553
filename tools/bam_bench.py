"""FisherMinBatchMatch steps at d = 10, B = 32 and d = 1024, B = 64 (f32, dense-Gaussian target): microseconds per step, median over 9
repeats of 100-step runs after a warm-up, wall clock around a synchronised run (the protocol of tools/natgrad_bench.py), all legs in one
process.
    (a) mivi_bam_steps in 100-step calls
    (b) the same step composed from mivi_bam_moments and torch on the device tensors: the RANK-B restatement in torch (Q and Zt by hand,
        torch.linalg.eigh of the B x B matrix, torch.linalg.cholesky), in float64 like the library's update -- not the literal
        torch.cov and d x d matrix square root, which would be the weaker opponent
    (c) mivi_bam_moments alone
and (d) mivi_bam_update alone on fixed (u, G), which with the launch count gives the update's share per launch.  Every step restarts the
iteration count at 1 + step, as a run does.  One JSON line per case; `python tools/bam_bench.py [small] [out.jsonl]` appends them to the
file as well."""
import json, statistics, sys, time
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


def case(d, B, dtype=np.float32, sink=None):
    from advancedvi_jl_amd._lib import MiviError
    L = np.tril(np.eye(d) + 1.0 / (2 * d)).astype(dtype)
    prob = avi.DenseNormalProblem(np.full(d, 5, dtype), L)
    params, _ = avi.destructure(avi.FullRankGaussian(np.zeros(d, dtype), np.eye(d, dtype=dtype)))
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, B, 0, 1)
    ctx.set_problem(prob)
    p0 = ctx.to_device(params)
    p = p0.clone()
    s0 = ctx.bam_init(p0).clone()
    st = s0.clone()
    u, G = ctx.empty(d * B), ctx.empty(d * B)
    fisher, elbo = ctx.empty(STEPS), ctx.empty(STEPS)
    f64 = torch.float64

    def fused():
        p.copy_(p0)
        st.copy_(s0)
        ctx.bam_steps(p, st, 0, 1, STEPS, B, fisher, elbo)

    def composed():
        p.copy_(p0)
        st.copy_(s0)
        for i in range(STEPS):
            uu, GG, _, _, _ = ctx.bam_moments(p, i, B, u, G)
            lam = float(dtype(d * B / (1 + i)))
            m, C = p[:d].to(f64), p[d:].view(d, d).t().to(f64)
            Sig = st.view(d, d).to(f64)
            Um, Gm = uu.view(B, d).t().to(f64), GG.view(B, d).t().to(f64)
            z = C @ Um + m[:, None]
            zbar, gbar = z.mean(1), Gm.mean(1)
            al, be = (lam / (B - 1)) ** 0.5, (lam / ((1 + lam) * B)) ** 0.5
            Q = al * (Gm - gbar[:, None]) + be * gbar[:, None]
            Zt = al * (z - zbar[:, None]) + be * (zbar - m)[:, None]
            M = Zt.t() @ Q
            SQ = Sig @ Q
            K = Q.t() @ SQ + M.t() @ M
            w, E = torch.linalg.eigh(0.5 * (K + K.t()))
            a = 0.5 + torch.sqrt(torch.clamp(w, min=0.0) + 0.25)
            Y = ((SQ + Zt @ M) @ E) / a
            Sp = Sig + Zt @ Zt.t() - Y @ Y.t()
            Sp = 0.5 * (Sp + Sp.t())
            p[:d] = (m / (1 + lam) + lam / (1 + lam) * (Sp @ gbar + zbar)).to(p.dtype)
            p[d:] = torch.linalg.cholesky(Sp).t().reshape(-1).to(p.dtype)
            st.copy_(Sp.reshape(-1).to(p.dtype))

    def moments():
        for i in range(STEPS):
            ctx.bam_moments(p0, i, B, u, G)

    def update_alone():
        for i in range(STEPS):
            p.copy_(p0)
            st.copy_(s0)
            ctx.bam_update(p, st, u, G, B, float(dtype(d * B)))

    a = timed(fused)
    last = (float(fisher[-1].item()), float(elbo[-1].item()))
    flagged = 0
    try:
        ctx.synchronize()
    except MiviError as e:
        flagged = e.status
    try:
        b = timed(composed)
    except Exception as e:   # torch.linalg.cholesky raises where the library flags
        b = (float("nan"),) * 3
        print(f"composed leg failed: {type(e).__name__}", file=sys.stderr)
    c = timed(moments)
    ctx.bam_moments(p0, 0, B, u, G)
    upd = timed(update_alone)
    try:
        ctx.synchronize()
    except MiviError as e:
        flagged = flagged or e.status
    nT = (d + 63) // 64
    line = json.dumps(dict(d=d, n=B, dtype=np.dtype(dtype).name, steps_per_call=STEPS, launches_per_update=2 * nT + 6, fused_us=round(a[0], 2),
                           composed_us=round(b[0], 2), moments_us=round(c[0], 2), update_alone_us=round(upd[0], 2),
                           update_us_per_launch=round(upd[0] / (2 * nT + 6), 2), fused_min_max=[round(a[1], 2), round(a[2], 2)],
                           composed_min_max=[round(b[1], 2), round(b[2], 2)], moments_min_max=[round(c[1], 2), round(c[2], 2)],
                           fisher_last=last[0], elbo_last=last[1], status=flagged))
    print(line, flush=True)
    if sink:
        with open(sink, "a") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    small_only = "small" in args
    sink = next((a for a in args if a != "small"), None)
    case(10, 32, sink=sink)
    if not small_only:
        case(1024, 64, sink=sink)
