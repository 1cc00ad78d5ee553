"""Block-diagonal family: microseconds per mivi_estimate_gradient, f32, diagonal-Gaussian target, closed-form and sticking-the-landing
entropy, at d = 1024, M = 256 with b in {4, 16, 64} and at d = 65536, M = 256, b = 32 -- against, in the same process on the same device,
    (two_kernel) the two-kernel route at the same target: an exp bijector on coordinate 0 alone keeps the estimate off the fused kernel (it
                 adds the bijector's two small launches and the target's own kernel: that IS the route every other target takes),
    (meanfield / fullrank) the other square-scale families' single-call estimate at the same d, M, target and estimator (d = 1024 only),
    (torch)      the same estimate composed from torch.bmm on device tensors (draws by torch.randn; d a multiple of b).
Every figure is device time: two events around CALLS back-to-back calls, divided by CALLS, after WARM warm-up calls; the legs of a case
alternate over ROUNDS rounds, the median of the rounds is reported and their spread (max - min) next to it.
One JSON line per case; `python tools/blockdiag_bench.py [out.jsonl]` appends them to the file as well (profiles/blockdiag_bench.jsonl)."""
import json, statistics, sys
import numpy as np
sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
import torch
import advancedvi_jl_amd as avi

M, CALLS, WARM, ROUNDS = 256, 100, 10, 5
LOG2PI = float(np.log(2 * np.pi))


def timed(fn):
    for _ in range(WARM):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS


def torch_estimate(mu, Cb, stl, mean, istd):
    """One estimate in torch: Cb (nb, b, b) lower-triangular blocks; value and the gradient pieces."""
    nb, b, _ = Cb.shape
    E = torch.randn(nb, b, M, device=mu.device, dtype=mu.dtype)
    Z = torch.bmm(Cb, E) + mu.view(nb, b, 1)
    R = (Z - mean.view(nb, b, 1)) * istd.view(nb, b, 1)
    W = -R * istd.view(nb, b, 1)
    ell = -0.5 * (R * R).sum((0, 1))
    diag = torch.diagonal(Cb, dim1=1, dim2=2)
    if stl:
        W = W + torch.linalg.solve_triangular(Cb.transpose(1, 2), E, upper=True)
        value = -ell.mean() - (0.5 * (E * E).sum((0, 1)).mean() + 0.5 * nb * b * LOG2PI + torch.log(diag).sum())
        dC = -torch.tril(torch.bmm(W, E.transpose(1, 2))) / M
    else:
        value = -ell.mean() - (0.5 * nb * b * (1 + LOG2PI) + torch.log(diag).sum())
        dC = -torch.tril(torch.bmm(W, E.transpose(1, 2))) / M - torch.diag_embed(1 / diag)
    return value, -W.mean(2), dC


def case(d, b, ent, sink=None):
    dt = np.float32
    rng = np.random.default_rng(1)
    mean, std = rng.normal(size=d).astype(dt), rng.uniform(0.5, 2.0, size=d).astype(dt)
    prob = avi.DiagNormalProblem(mean, std)
    nb = d // b
    blocks = np.tril(rng.normal(size=(nb, b, b)) * (0.3 / np.sqrt(b)), -1) + np.eye(b) * rng.uniform(0.5, 1.5, size=(nb, b, 1))
    q = avi.BlockDiagGaussian(rng.normal(size=d).astype(dt), list(blocks.astype(dt)))
    ctxs = {"fused": (avi.MiviContext(dt, avi.BLOCKDIAG, d, M, ent.code, 1, block=b), prob, q),
            "two_kernel": (avi.MiviContext(dt, avi.BLOCKDIAG, d, M, ent.code, 1, block=b),
                           avi.TransformedProblem(prob, avi.StackedBijector([(0, 1, "exp"), (1, d, "identity")])), q)}
    if d <= 2048:
        ctxs["meanfield"] = (avi.MiviContext(dt, avi.MEANFIELD, d, M, ent.code, 1), prob, avi.MeanFieldGaussian(q.location, q.var() ** 0.5))
        ctxs["fullrank"] = (avi.MiviContext(dt, avi.FULLRANK, d, M, ent.code, 1), prob, avi.FullRankGaussian(q.location, q.dense_scale()))
    legs, idx = {}, [0]
    for name, (c, pr, qq) in ctxs.items():
        c.set_problem(pr)
        p, v, g = c.to_device(avi.destructure(qq)[0]), c.empty(1), c.empty(c.params_len)

        def leg(c=c, p=p, v=v, g=g):
            idx[0] += 1
            c.estimate_gradient(p, idx[0], v, g)
        legs[name] = leg
    dev = torch.device("cuda", 0)
    t_mu, t_C = torch.tensor(q.location, device=dev), torch.tensor(blocks.astype(dt), device=dev)
    t_mean, t_istd = torch.tensor(mean, device=dev), torch.tensor(1 / std, device=dev)
    legs["torch"] = lambda: torch_estimate(t_mu, t_C, ent.code == 3, t_mean, t_istd)
    med = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            med[k].append(timed(fn))
    rec = {"bench": "blockdiag_estimate_gradient", "d": d, "M": M, "block": b, "dtype": "f32", "target": "diag", "entropy": type(ent).__name__,
           "calls": CALLS, "rounds": ROUNDS}
    for k in legs:
        rec[k + "_us"] = round(statistics.median(med[k]), 2)
        rec[k + "_spread_us"] = round(max(med[k]) - min(med[k]), 2)
    for c, _, _ in ctxs.values():
        c.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


if __name__ == "__main__":
    sink = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
    for d, b in ((1024, 4), (1024, 16), (1024, 64), (65536, 32)):
        for ent in (avi.ClosedFormEntropy(), avi.StickingTheLandingEntropy()):
            case(d, b, ent, sink)
