"""Which route a `mivi_optimize_loop` call runs on: the table of launch-free loops is walked in priority order and the first row that takes
the call and launches wins; everything else is the graph of launches.  One 3-step call per row at the smallest shapes
that reach it, read back through mivi_batch_info(ctx, NULL, 7); a hipGraph is recorded (what = 4 grows) exactly when the route is 0.  The
expected routes are what the if-ladder this table replaced took for the same calls.  (A lost exchange: tests/test_gpu_loop_oracle.py.)"""
import numpy as np
import pytest

import advancedvi_jl_amd as avi
from tests.helpers import SEED

pytestmark = pytest.mark.gpu

GRAPH, MF_SGD, LR_SMALL, MF_GEN, FR_SMALL, FR_ROWS, MF_FUNNEL_SGD = range(7)   # DeviceLoopId, include/mivi.h (mivi_batch_info what = 7)
DESCENT, ADAM, DOG, DOWG, COCOB = range(5)
NONE, CLIP, PROX = range(3)
STL = avi.StickingTheLandingEntropy.code


def _diag(d, dtype):
    return avi.DiagNormalProblem(np.linspace(-1.0, 1.0, d).astype(dtype), np.linspace(0.5, 1.5, d).astype(dtype))


def _logreg(dtype=np.float32):
    rng = np.random.default_rng(5)
    return avi.LogRegProblem((rng.normal(size=(32, 4)) / 2.0).astype(dtype), (rng.uniform(size=32) < 0.5).astype(np.uint8), "logsigma_normal", 1.0)


def _q0(family, d, dtype, rank=0):
    mu = np.linspace(-0.3, 0.3, d).astype(dtype)
    if family == avi.MEANFIELD:
        return avi.MeanFieldGaussian(mu, np.ones(d, dtype))
    if family == avi.FULLRANK:
        return avi.FullRankGaussian(mu, np.eye(d, dtype=dtype))
    return avi.MvLocationScaleLowRank(mu, np.ones(d, dtype), np.full((d, rank), 0.1, dtype))


def _route(ctx, p0, rule, op=NONE, averager=0, beta=(0.9, 0.999), batches=False):
    """(route of one 3-step call -- 2 steps over a schedule of two batches --, hipGraphs it recorded, its tensors).  The caller keeps the
    tensors alive until the context's cases are done, so no two calls of a context share a graph key by address."""
    p = ctx.to_device(p0).clone()
    st = None
    if rule == ADAM:
        st = ctx.empty(2 * p.numel()).zero_()
    elif rule in (DOG, DOWG):
        st = ctx.dog_state()
        ctx.dog_init(p, st, 1e-2)
    elif rule == COCOB:
        st = ctx.empty(5 * p.numel()).zero_()
        st[4 * p.numel():] = p
    ap = p.clone() if averager else None
    before = ctx.graph_recordings()
    run = ctx.optimize_loop_batches if batches else ctx.optimize_loop
    run(p, 2 if batches else 3, 7, 0, rule=rule, op=op, averager=averager, eta=100.0 if rule == COCOB else 1e-3, beta=beta, clip_epsilon=1e-5, opt_state=st, avg_params=ap)
    ctx.synchronize()
    assert np.isfinite(p.cpu().numpy()).all()
    return int(ctx.lib.mivi_batch_info(ctx.h, None, 7)), ctx.graph_recordings() - before, (p, st, ap)


def _check(ctx, p0, cases):
    keep = []
    for want, kw in cases:
        got, recorded, tensors = _route(ctx, p0, **kw)
        keep.append(tensors)
        assert got == want, (kw, got, want)
        assert recorded == (1 if want == GRAPH else 0), (kw, got, recorded)
    ctx.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_mean_field_diag_routes(dtype):
    p0, _ = avi.destructure(_q0(avi.MEANFIELD, 8, dtype))
    ctx = avi.MiviContext(dtype, avi.MEANFIELD, 8, 4, 0, SEED)
    ctx.set_problem(_diag(8, dtype))
    _check(ctx, p0, [(MF_SGD, dict(rule=DESCENT)), (MF_SGD, dict(rule=ADAM, op=CLIP)), (MF_GEN, dict(rule=ADAM, beta=(0.8, 0.999))),
                     (MF_GEN, dict(rule=DOWG, op=PROX, averager=1)), (GRAPH, dict(rule=COCOB))])
    ctx = avi.MiviContext(dtype, avi.MEANFIELD, 8, 4, 0, SEED)   # an exp bijector block: the loops have no Stacked-bijector handling
    ctx.set_problem(avi.TransformedProblem(_diag(8, dtype), avi.StackedBijector([(0, 2, "exp")])))
    _check(ctx, p0, [(GRAPH, dict(rule=DESCENT))])


def test_full_rank_routes():
    f32 = np.float32
    p0, _ = avi.destructure(_q0(avi.FULLRANK, 10, f32))
    ctx = avi.MiviContext(f32, avi.FULLRANK, 10, 1, 0, SEED)
    ctx.set_problem(_diag(10, f32))
    _check(ctx, p0, [(FR_SMALL, dict(rule=DESCENT)), (FR_SMALL, dict(rule=DOG)), (GRAPH, dict(rule=COCOB))])
    p0, _ = avi.destructure(_q0(avi.FULLRANK, 64, f32))
    ctx = avi.MiviContext(f32, avi.FULLRANK, 64, 8, 0, SEED)
    ctx.set_problem(_diag(64, f32))
    _check(ctx, p0, [(FR_ROWS, dict(rule=ADAM)), (FR_ROWS, dict(rule=DOWG, op=CLIP, averager=1)), (GRAPH, dict(rule=COCOB))])
    ctx = avi.MiviContext(f32, avi.FULLRANK, 64, 8, STL, SEED)
    ctx.set_problem(_diag(64, f32))
    _check(ctx, p0, [(GRAPH, dict(rule=ADAM))])
    p0, _ = avi.destructure(_q0(avi.FULLRANK, 64, np.float64))
    ctx = avi.MiviContext(np.float64, avi.FULLRANK, 64, 8, 0, SEED)
    ctx.set_problem(_diag(64, np.float64))
    _check(ctx, p0, [(GRAPH, dict(rule=ADAM))])


def test_funnel_routes():
    f32 = np.float32
    p0, _ = avi.destructure(_q0(avi.MEANFIELD, 8, f32))
    ctx = avi.MiviContext(f32, avi.MEANFIELD, 8, 8, 0, SEED)
    ctx.set_problem(avi.FunnelProblem(8, 1.5))
    _check(ctx, p0, [(MF_FUNNEL_SGD, dict(rule=ADAM)), (GRAPH, dict(rule=COCOB))])
    ctx = avi.MiviContext(f32, avi.MEANFIELD, 8, 8, 0, SEED)
    ctx.set_problem(avi.TransformedProblem(avi.FunnelConstrainedProblem(8, 1.5), avi.StackedBijector([(0, 1, "exp"), (1, 8, "identity")])))
    _check(ctx, p0, [(GRAPH, dict(rule=ADAM))])


def test_logreg_routes():
    f32 = np.float32
    p0, _ = avi.destructure(_q0(avi.MEANFIELD, 5, f32))
    ctx = avi.MiviContext(f32, avi.MEANFIELD, 5, 4, 0, SEED)
    ctx.set_problem(_logreg())
    _check(ctx, p0, [(LR_SMALL, dict(rule=DOWG)), (GRAPH, dict(rule=COCOB))])
    ctx = avi.MiviContext(f32, avi.MEANFIELD, 5, 4, 0, SEED)   # a schedule of two batches: the rows are read through the schedule
    ctx.set_problem(_logreg())
    ctx.set_batch_schedule(np.arange(32).reshape(2, 16))
    _check(ctx, p0, [(GRAPH, dict(rule=DOWG, batches=True))])


def test_low_rank_and_laplace_base_run_on_the_graph():
    f32 = np.float32
    p0, _ = avi.destructure(_q0(avi.LOWRANK, 8, f32, rank=2))
    ctx = avi.MiviContext(f32, avi.LOWRANK, 8, 4, 0, SEED, rank=2)
    ctx.set_problem(_diag(8, f32))
    _check(ctx, p0, [(GRAPH, dict(rule=DESCENT))])
    p0, _ = avi.destructure(_q0(avi.MEANFIELD, 8, f32))
    ctx = avi.MiviContext(f32, avi.MEANFIELD, 8, 4, 0, SEED)
    ctx.set_problem(_diag(8, f32))
    ctx.set_base_dist(avi.Laplace())
    _check(ctx, p0, [(GRAPH, dict(rule=DESCENT))])
