"""Low-rank family: microseconds per mivi_estimate_gradient at d = 1024, M = 256, f32, diagonal and dense Gaussian targets, r in {4, 16, 64},
closed-form and sticking-the-landing entropy -- against, in the same process on the same device,
    (fullrank)  the full-rank family's single-call estimate at the same d, M, target and estimator,
    (torch)     the same low-rank estimate composed from torch matmuls on device tensors (draws by torch.randn, A = I + U' D^-2 U and its
                inverse in float64 like the library's prep, everything else float32).
Every figure is the median of CALLS single calls, each timed by a host clock around {call, device synchronise}, after WARM warm-up calls;
the legs of a case alternate over ROUNDS rounds and the spread of a leg's round medians is recorded next to it (`spread`: max - min).
One JSON line per case; `python tools/lowrank_bench.py [out.jsonl]` appends them to the file as well (profiles/lowrank_bench.jsonl)."""
import json, statistics, sys, time
import numpy as np
sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
import torch
import advancedvi_jl_amd as avi

D, M, CALLS, WARM, ROUNDS = 1024, 256, 200, 20, 3
LOG2PI = float(np.log(2 * np.pi))


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


def torch_estimate(params, r, stl, tgt):
    """One estimate of the low-rank family in torch (float32 device tensors): value and the flat gradient."""
    d = D
    m, Dg, U = params[:d], params[d:2 * d], params[2 * d:].view(r, d).t()
    E = torch.randn(d + r, M, device=params.device, dtype=params.dtype)
    u1, u2 = E[:d], E[d:]
    Dc = Dg[:, None]
    Z = Dc * u1 + U @ u2 + m[:, None]
    if tgt[0] == "diag":
        R = (Z - tgt[1][:, None]) * tgt[2][:, None]
        G = -R * tgt[2][:, None]
        ell = -0.5 * (R * R).sum(0)
    else:
        R = Z - tgt[1][:, None]
        G = -(tgt[2] @ R)
        ell = 0.5 * (R * G).sum(0)
    A = torch.eye(r, device=params.device, dtype=torch.float64) + (U.t() @ (U / (Dc * Dc))).double()
    Ainv = torch.linalg.inv(A)
    half_logdet = 0.5 * torch.logdet(A)
    if stl:
        t = u1 + (U @ u2) / Dc
        s = (U.t() @ (t / Dc)).double()
        x = Ainv @ s
        logq = -0.5 * d * LOG2PI - torch.log(Dg).sum() - half_logdet - 0.5 * ((t * t).sum(0).double() - (s * x).sum(0))
        V = (t - (U @ x.float()) / Dc) / Dc
        Cg = G + V
        value = -ell.mean() + logq.mean()
        gD, gU = (Cg * u1).mean(1), Cg @ u2.t() / M
    else:
        Cg = G
        value = -ell.mean() - (0.5 * d * (1 + LOG2PI) + torch.log(Dg).sum() + half_logdet)
        UA = U @ Ainv.float()
        gD = (Cg * u1).mean(1) + 1 / Dg - (UA * U).sum(1) / Dg ** 3
        gU = Cg @ u2.t() / M + UA / (Dc * Dc)
    return value, -torch.cat([Cg.mean(1), gD, gU.t().reshape(-1)])


def case(kind, r, ent, sink=None):
    dt = np.float32
    rng = np.random.default_rng(1)
    mean = rng.normal(size=D).astype(dt)
    if kind == "diag":
        std = rng.uniform(0.5, 2.0, size=D).astype(dt)
        prob = avi.DiagNormalProblem(mean, std)
    else:
        L = (np.tril(rng.normal(size=(D, D)) * (0.2 / np.sqrt(D))) + np.eye(D)).astype(dt)
        prob = avi.DenseNormalProblem(mean, L)
    q_lr = avi.LowRankGaussian(rng.normal(size=D).astype(dt), rng.uniform(0.5, 1.5, size=D).astype(dt), (0.7 * rng.normal(size=(D, r))).astype(dt))
    q_fr = avi.FullRankGaussian(q_lr.location, np.diag(q_lr.scale_diag) + np.tril(rng.normal(size=(D, D)) * (0.3 / np.sqrt(D)), -1).astype(dt))
    c_lr = avi.MiviContext(dt, avi.LOWRANK, D, M, ent.code, 1, rank=r)
    c_fr = avi.MiviContext(dt, avi.FULLRANK, D, M, ent.code, 1)
    c_lr.set_problem(prob)
    c_fr.set_problem(prob)
    p_lr, p_fr = c_lr.to_device(avi.destructure(q_lr)[0]), c_fr.to_device(avi.destructure(q_fr)[0])
    v_lr, g_lr, v_fr, g_fr = c_lr.empty(1), c_lr.empty(c_lr.params_len), c_fr.empty(1), c_fr.empty(c_fr.params_len)
    dev = p_lr.device
    if kind == "diag":
        tgt = ("diag", torch.tensor(mean, device=dev), torch.tensor(1 / std, device=dev))
    else:
        Li = np.linalg.inv(L.astype(np.float64))
        tgt = ("dense", torch.tensor(mean, device=dev), torch.tensor((Li.T @ Li).astype(dt), device=dev))
    stl = ent.code == 3
    idx = [0]

    def lowrank():
        idx[0] += 1
        c_lr.estimate_gradient(p_lr, idx[0], v_lr, g_lr)

    def fullrank():
        idx[0] += 1
        c_fr.estimate_gradient(p_fr, idx[0], v_fr, g_fr)

    def composed():
        torch_estimate(p_lr, r, stl, tgt)

    legs = {"lowrank": lowrank, "fullrank": fullrank, "torch": composed}
    med = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            med[k].append(timed(fn))
    rec = {"bench": "lowrank_estimate_gradient", "d": D, "M": M, "dtype": "f32", "target": kind, "rank": r, "entropy": type(ent).__name__,
           "calls": CALLS, "rounds": ROUNDS}
    for k in legs:
        rec[k + "_us"] = round(statistics.median(med[k]), 2)
        rec[k + "_spread_us"] = round(max(med[k]) - min(med[k]), 2)
    c_lr.close()
    c_fr.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


if __name__ == "__main__":
    sink = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
    for kind in ("diag", "dense"):
        for r in (4, 16, 64):
            for ent in (avi.ClosedFormEntropy(), avi.StickingTheLandingEntropy()):
                case(kind, r, ent, sink)
