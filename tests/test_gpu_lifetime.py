"""Device memory belongs to the context that allocated it (csrc/mivi_internal.h DevBuf): whatever a context did, mivi_destroy returns
every allocation it made.  The library counts the device allocations it holds in this process (mivi_batch_info what = 5, kept by its one
allocate / free pair), so each scenario reads the count through a small probe context, lets one context (or two) touch the buffers named
in its docstring at the smallest shapes that reach them, closes it and asks for the SAME count -- an equality with no margin.  The count
must also have been larger while the scenario's contexts lived, so a counter that never moves cannot pass.

The streams, events and graph execs the library creates have owners of the same kind (Stream, Event, GraphExec) and a count of their own
(mivi_batch_info what = 6): every scenario asks for the same equality on it, and the scenarios that must create handles -- children with
their streams and fork / join events, the capture stream and a cached graph, the two exchange pipelines -- also for its growth.  The
timing entries hold only temporaries (two events, a graph), so theirs is the equality alone.

A child context of the lane-batched routes borrows the parent's target vectors and its status word instead of owning copies; the second
test changes the parent's target under living children and asks for the single calls' results."""
import gc

import numpy as np
import pytest

import advancedvi_jl_amd as avi
from tests import natgrad_ref as NR
from tests.helpers import SEED, assert_batch_matches_single, make_family, make_problem

pytestmark = pytest.mark.gpu

F32 = np.float32
STL = 3   # MIVI_ENT_STL


def _ctx(family, d, M, kind, ent=0, dtype=F32, seed=0, **kw):
    """(context with the `kind` target set, device parameters, rng)"""
    rng = np.random.default_rng(900 + d + seed)
    q, _ = make_family(rng, d, family, dtype)
    ctx = avi.MiviContext(dtype, family, d, M, ent, SEED, **kw)
    if kind is not None:
        ctx.set_problem(make_problem(rng, kind, d, dtype)[0])
    return ctx, ctx.to_device(avi.destructure(q)[0]), rng


def meanfield_f64_loop():
    """mean-field f64, d = 5: diagonal target, then the funnel; a single estimate and a 3-step DoG loop on each (gen_scratch, dog_part, snap)"""
    ctx, p, rng = _ctx(avi.MEANFIELD, 5, 8, "diag", dtype=np.float64)
    for kind in ("diag", "funnel"):
        ctx.set_problem(make_problem(rng, kind, 5, np.float64)[0])
        ctx.estimate_gradient(p, 1)
        x = p.clone()
        st = ctx.dog_state()
        ctx.dog_init(x, st, 1e-6)
        ctx.optimize_loop(x, 3, 0, 0, rule=2, opt_state=st)
        ctx.synchronize()
    return [ctx]


def fullrank_stl_children_stein():
    """full-rank f32, d = 64, sticking the landing, diagonal then dense target: a single estimate, a batch of 8 (children, kid_out, the
    lanes' tables), the Stein estimator (stein_*, lds_tabSt)"""
    ctx, p, rng = _ctx(avi.FULLRANK, 64, 64, None, STL)
    v, g = ctx.empty(1), ctx.empty(ctx.params_len)
    for kind in ("diag", "dense"):
        ctx.set_problem(make_problem(rng, kind, 64, F32)[0])
        ctx.estimate_gradient(p, 1)
        ctx.estimate_gradient_n(p, 2, 8, v, g)
        ctx.gauss_expected_grad_hess(p, 3)
        ctx.synchronize()
    return [ctx]


def engine_batches():
    """the batch engine: d = 128 with the dense target, every estimate of a batch of 4, then a sharded batch of 4 on one rank (fb.parts);
    d = 256 sticking the landing (fb.Tinv, fb.TA, fb.Eye)"""
    ctx, p, _ = _ctx(avi.FULLRANK, 128, 128, "dense")
    assert ctx.batch_takes_engine(p)
    ctx.estimate_gradient_each(p, 1, 4)
    ctx.comm_init(None, 0, 1)
    ctx.estimate_gradient_dist_n(p, 5, 4, ctx.empty(1), ctx.empty(ctx.params_len))
    ctx.synchronize()
    stl, ps, _ = _ctx(avi.FULLRANK, 256, 128, "diag", STL)
    assert stl.batch_takes_engine(ps)
    stl.estimate_gradient_each(ps, 1, 4)
    stl.synchronize()
    return [ctx, stl]


def engine_sharded_with_communicator():
    """the batch engine's sharded batch behind a communicator of one rank, full-rank f32 d = 128: 90 estimates are two engine steps, the
    all-reduce + finalisation of each on the engine's exchange pipeline (fb_pipe: a stream and four events)"""
    ctx, p, _ = _ctx(avi.FULLRANK, 128, 128, "diag")
    ctx.comm_init(ctx.comm_unique_id(), 0, 1)
    ctx.comm_set_route("allreduce")
    ctx.estimate_gradient_dist_n(p, 3, 90, ctx.empty(1), ctx.empty(ctx.params_len))
    ctx.synchronize()
    return [ctx]


def profile_entries():
    """the three timing entries, full-rank f32 d = 128: a product and a VJP stage (two timing events and a temporary graph each), the
    engine's kernels, the sharded step on one rank without a communicator"""
    ctx, p, _ = _ctx(avi.FULLRANK, 128, 128, "diag")
    ctx.profile_kernel(2, p, 2)
    ctx.profile_kernel(3, p, 2)
    ctx.profile_batch(p, 4, 2)
    ctx.profile_dist(p, 4)
    ctx.synchronize()
    return [ctx]


def _p2p(detach):
    ctx, p, _ = _ctx(avi.FULLRANK, 64, 64, "diag")
    ctx.p2p_attach([ctx.p2p_export(0, 1)])
    ctx.estimate_gradient_dist(p, 1)
    ctx.estimate_gradient_dist_n(p, 2, 8, ctx.empty(1), ctx.empty(ctx.params_len))
    ctx.synchronize()
    if detach:
        ctx.p2p_detach()
    return [ctx]


def p2p_world_one_detached():
    """one rank's peer-to-peer areas, full-rank f32 d = 64: a sharded estimate and a batch of 8 (dist_ring, p2p_*), detached before close"""
    return _p2p(True)


def p2p_world_one_left_attached():
    """the same, and close() finds the areas still attached"""
    return _p2p(False)


def logreg_planes_and_rows():
    """logistic regression f32, n = 2000, d = 64: n (d - 1) >= 1e5, so the planes of X exist (lr_XA, lr_XB); 256 selected rows; the second-
    order Gaussian expectation (h2_acc); then a data set of n = 64, the branch that drops the planes"""
    d = 64
    ctx, p, rng = _ctx(avi.FULLRANK, d, 16, None)
    for n in (2000, 64):
        X = (rng.normal(size=(n, d - 1)) / np.sqrt(d)).astype(F32)
        prob = avi.LogRegProblem(X, (rng.uniform(size=n) < 0.5).astype(np.uint8), "logsigma_normal", 1.0)
        ctx.set_problem(prob)
        ctx.estimate_gradient(p, 1)
        if n == 2000:
            ctx.set_problem(prob.subsample(rng.permutation(n)[:256]))
            ctx.estimate_gradient(p, 2)
            ctx.gauss_expected_grad_hess(p, 3, second_order=True)
        ctx.synchronize()
    return [ctx]


def lowrank_estimate_sample_logpdf():
    """low-rank d = 32, rank = 4: an estimate, sample, logpdf of 10 points (lowr_*, lp_*)"""
    d, r = 32, 4
    rng = np.random.default_rng(941)
    q = avi.LowRankGaussian(rng.normal(size=d).astype(F32), rng.uniform(0.5, 1.5, size=d).astype(F32), (0.7 * rng.normal(size=(d, r))).astype(F32))
    ctx = avi.MiviContext(F32, avi.LOWRANK, d, 16, 0, SEED, rank=r)
    ctx.set_problem(make_problem(rng, "diag", d, F32)[0])
    p = ctx.to_device(avi.destructure(q)[0])
    ctx.estimate_gradient(p, 1)
    ctx.sample(p, 2)
    ctx.logpdf(p, rng.normal(size=(d, 10)).astype(F32))
    ctx.synchronize()
    return [ctx]


def laplace_base_then_normal():
    """Laplace base, sticking the landing, mean-field and full-rank d = 32 (bd_U, bd_R); back to the Normal base, another estimate"""
    out = []
    for family in (avi.MEANFIELD, avi.FULLRANK):
        ctx, p, _ = _ctx(family, 32, 16, "diag", STL)
        for dist in (avi.Laplace(), avi.Normal()):
            ctx.set_base_dist(dist)
            ctx.estimate_gradient(p, 1)
            ctx.synchronize()
        out.append(ctx)
    return out


def stacked_bijector_blocks():
    """Stacked bijector with a truncated and an ordered block, d = 12: an estimate, constrained draws, their constrained logpdf through the
    _host entry (bij_*)"""
    d = 12
    ctx, p, rng = _ctx(avi.FULLRANK, d, 8, None)
    bij = avi.StackedBijector([(0, 4, "truncated", (0.0, 1.0)), (4, 8, "ordered"), (8, d, "identity")])
    ctx.set_problem(avi.TransformedProblem(make_problem(rng, "diag", d, F32)[0], bij))
    ctx.estimate_gradient(p, 1)
    X = ctx.sample_constrained(p, 2).cpu().numpy()
    ctx.logpdf_constrained_host(p.cpu().numpy(), X)
    ctx.synchronize()
    return [ctx]


def score_gradient():
    """the score-gradient estimate, full-rank d = 16 (sg_*)"""
    ctx, p, _ = _ctx(avi.FULLRANK, 16, 16, "diag")
    ctx.estimate_score_gradient(p, 1)
    ctx.synchronize()
    return [ctx]


def measure_space_host_updates():
    """one _host update each of square-root NGD, natural gradient, batch and match, Wasserstein at d = 40 (ms_*, ngd_est, natgrad_host, bam_host)"""
    d, n = 40, 8
    ctx, p, rng = _ctx(avi.FULLRANK, d, 1, "diag", dtype=np.float64)   # (batch and match asks for a target even where it evaluates none)
    params = p.cpu().numpy()
    g = rng.normal(size=d)
    H = NR.congruent_hessian(params[d:].reshape(d, d, order="F"), rng, symmetric=True)
    ctx.sqrt_ngd_update_host(params, g, H, 0.05)
    ctx.natgrad_update_host(params, ctx.natgrad_init(p).cpu().numpy(), g, H, 0.3)
    Sigma = ctx.wass_init(p).cpu().numpy()
    ctx.wass_update_host(params, Sigma, g, H, 0.1)
    u = rng.normal(size=(d, n))
    ctx.bam_update_host(params, Sigma, u, -u, float(d * n))
    return [ctx]


SCENARIOS = [meanfield_f64_loop, fullrank_stl_children_stein, engine_batches, p2p_world_one_detached, p2p_world_one_left_attached,
             logreg_planes_and_rows, lowrank_estimate_sample_logpdf, laplace_base_then_normal, stacked_bijector_blocks, score_gradient,
             measure_space_host_updates, engine_sharded_with_communicator, profile_entries]
# (scenario, it must leave handles on its contexts)
HANDLE_SCENARIOS = [(fullrank_stl_children_stein, True), (p2p_world_one_detached, True), (p2p_world_one_left_attached, True),
                    (engine_sharded_with_communicator, True), (profile_entries, False)]


def _probe():
    gc.collect()   # (contexts an earlier test dropped without close())
    probe = avi.MiviContext(F32, avi.MEANFIELD, 8, 1, 0, SEED)
    return probe, probe.live_allocations()


def _run(scenario, count):
    """count() before the scenario, with its contexts alive, after their close()"""
    n0 = count()
    ctxs = scenario()
    alive = count()
    for c in ctxs:
        c.close()
    del ctxs
    gc.collect()
    return n0, alive, count()


@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda s: s.__name__)
def test_destroy_returns_every_allocation(scenario):
    probe, _ = _probe()
    (n0, h0), (alive, h_alive), (n1, h1) = _run(scenario, lambda: (probe.live_allocations(), probe.live_handles()))
    probe.close()
    print(f"[lifetime] {scenario.__name__}: {n0} allocations before, {alive} with the scenario's contexts alive, {n1} after close(); "
          f"handles {h0}, {h_alive}, {h1}")
    assert alive > n0
    assert n1 == n0
    assert h1 == h0


@pytest.mark.parametrize("scenario,grows", HANDLE_SCENARIOS, ids=[s.__name__ for s, _ in HANDLE_SCENARIOS])
def test_destroy_returns_every_handle(scenario, grows):
    probe, _ = _probe()
    n0, alive, n1 = _run(scenario, probe.live_handles)
    probe.close()
    print(f"[lifetime] {scenario.__name__}: {n0} handles before, {alive} with the scenario's contexts alive, {n1} after close()")
    assert not grows or alive > n0
    assert n1 == n0


def test_children_borrow_the_parents_target():
    """full-rank f32, d = 64, n_mc = 64: a batch of 8 creates the children, which borrow the target; a NEW diagonal target on the parent, and
    the same batch must give what single calls on a second context with that target give (tests/helpers.py assert_batch_matches_single);
    close() then returns everything, the children's buffers included."""
    probe, n0 = _probe()
    h0 = probe.live_handles()
    d, M, n, idx = 64, 64, 8, 3
    ctx, p, rng = _ctx(avi.FULLRANK, d, M, "diag")
    ref = avi.MiviContext(F32, avi.FULLRANK, d, M, 0, SEED)
    v, g = ctx.empty(1), ctx.empty(ctx.params_len)
    ctx.estimate_gradient_n(p, idx, n, v, g)
    ctx.synchronize()
    prob2 = avi.DiagNormalProblem((2.0 + rng.normal(size=d)).astype(F32), rng.uniform(0.3, 0.6, size=d).astype(F32))
    ctx.set_problem(prob2)
    ref.set_problem(prob2)
    g.fill_(float("nan"))
    ctx.estimate_gradient_n(p, idx, n, v, g)
    ctx.synchronize()
    v1, g1 = ref.estimate_gradient(p, idx + n - 1)
    ref.synchronize()
    assert_batch_matches_single(v.item(), v1.item(), g.cpu().numpy(), g1.cpu().numpy(), engine=ctx.batch_takes_engine(p), what="new target")
    assert probe.live_allocations() > n0
    assert probe.live_handles() > h0   # (the children's streams, the fork / join events, the capture stream, the cached graph)
    ctx.close()
    ref.close()
    gc.collect()
    n1, h1 = probe.live_allocations(), probe.live_handles()
    probe.close()
    assert n1 == n0
    assert h1 == h0
