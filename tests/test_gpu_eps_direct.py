"""The batch engine's draws (csrc/kernels_fullrank_batch.hip k_fb_eps: every thread draws the two Philox blocks its fragment lane holds, no LDS
tile; tril(C)'s planes laid out by rider workgroups of a call's first draw launch) across the steps of a call (api_batch.hip
fb_batch).  163 estimates = three steps of 55 / 55 / 53 lanes: draws with and without riders, and a shorter last step with its own work table.
Shapes: the smallest the engine takes (128, 128), a padded geometry (160, 160: zero planes in the padding blocks), more 64-row blocks than
the four fragments of a draw workgroup (256, 128).
  * every estimate against the single call at the same index (tests/helpers.py: the batch tolerances);
  * a lane's tiles do not depend on the step it rides in: the 163-estimate call equals, bitwise, calls of at most 80 estimates (one step)
    over the same indices;
  * no stale plane is ever read: repeated calls and a call at other indices in between, bitwise;
  * the sum(eps^2) partials through the value workgroups: the Monte-Carlo entropy and a sticking-the-landing estimator;
  * objective mode (lanes = consecutive blocks of samples of one estimate) against the chunked route."""
import numpy as np
import pytest

import advancedvi_jl_amd as avi
from tests.helpers import SEED, assert_batch_matches_single, make_family, make_problem

pytestmark = pytest.mark.gpu

N, IDX0 = 163, 11
SHAPES = [(128, 128), (160, 160), (256, 128)]
_cache = {}


def _setup(d, M, ent):
    rng = np.random.default_rng(5 + d + M)
    q, _ = make_family(rng, d, avi.FULLRANK, np.float32)
    prob, _ = make_problem(rng, "diag", d, np.float32)
    params, _ = avi.destructure(q)
    ctx = avi.MiviContext(np.float32, avi.FULLRANK, d, M, ent, SEED)
    ctx.set_problem(prob)
    return ctx, params


def _each(ctx, p, idx0, n):
    vals, grads = ctx.estimate_gradient_each(p, idx0, n)
    ctx.synchronize()
    return vals.cpu().numpy(), grads.cpu().numpy()


def _results(d, M, ent):
    """Computed once per configuration and left unchanged: the 163-estimate call, and the single calls at the same indices."""
    key = (d, M, ent)
    if key not in _cache:
        ctx, params = _setup(d, M, ent)
        p = ctx.to_device(params)
        engine = bool(ctx.batch_takes_engine(p))
        vals, grads = _each(ctx, p, IDX0, N)
        ctx.close()
        ref, _ = _setup(d, M, ent)
        pr = ref.to_device(params)
        v1, g1 = np.zeros(N, np.float32), np.zeros_like(grads)
        for i in range(N):
            v, g = ref.estimate_gradient(pr, IDX0 + i)
            v1[i], g1[i] = v.item(), g.cpu().numpy()
        ref.close()
        for a in (vals, grads, v1, g1):
            a.setflags(write=False)
        _cache[key] = dict(engine=engine, vals=vals, grads=grads, v1=v1, g1=g1)
    return _cache[key]


def _assert_equals_single_calls(r, engine):
    for i in range(N):
        assert_batch_matches_single(r["vals"][i], r["v1"][i], r["grads"][i], r["g1"][i], engine, i)


@pytest.mark.parametrize("d,M", SHAPES)
def test_every_estimate_of_three_steps_equals_the_single_call(d, M):
    r = _results(d, M, 0)
    assert r["engine"]
    _assert_equals_single_calls(r, True)
    if d == 160:   # the padding rows / samples contribute nothing: rows of the gradient are the family's 160, all finite
        assert np.all(np.isfinite(r["grads"])) and np.all(np.isfinite(r["vals"]))


@pytest.mark.parametrize("d,M", SHAPES)
def test_a_lane_does_not_depend_on_the_step_it_rides_in(d, M):
    """Bitwise: the three-step call against single-step calls of 80 / 80 / 3 estimates."""
    r = _results(d, M, 0)
    ctx, params = _setup(d, M, 0)
    p = ctx.to_device(params)
    vs, gs = [], []
    for lo in range(0, N, 80):
        v, g = _each(ctx, p, IDX0 + lo, min(80, N - lo))
        vs.append(v)
        gs.append(g)
    ctx.close()
    assert np.array_equal(np.concatenate(vs), r["vals"])
    assert np.array_equal(np.concatenate(gs), r["grads"])


def test_no_stale_plane_is_read():
    d, M = 128, 128
    r = _results(d, M, 0)
    ctx, params = _setup(d, M, 0)
    p = ctx.to_device(params)
    v_a, g_a = _each(ctx, p, IDX0, N)
    v_b, g_b = _each(ctx, p, IDX0, N)
    v_o, g_o = _each(ctx, p, IDX0 + 1000, N)
    v_c, g_c = _each(ctx, p, IDX0, N)
    ctx.close()
    for v, g in ((v_a, g_a), (v_b, g_b), (v_c, g_c)):
        assert np.array_equal(v, r["vals"]) and np.array_equal(g, r["grads"])
    assert not np.array_equal(v_o, v_a) and not np.array_equal(g_o, g_a)
    # the call at other indices overlaps this one by none of its estimates; shifted by one step it shares 108 of them
    ctx, _ = _setup(d, M, 0)
    v_s, g_s = _each(ctx, ctx.to_device(params), IDX0 + 55, N)
    ctx.close()
    assert np.array_equal(v_s[:N - 55], r["vals"][55:]) and np.array_equal(g_s[:N - 55], r["grads"][55:])


def test_monte_carlo_entropy_through_the_value_workgroups():
    """The value holds sum(eps^2) / 2: the draw workgroups' partials (one per 64 x 32 block), summed by the lanes' value workgroups."""
    r = _results(128, 128, avi.MonteCarloEntropy.code)
    assert r["engine"]
    _assert_equals_single_calls(r, True)


@pytest.mark.parametrize("d,M", [(128, 128), (256, 128)])
def test_sticking_the_landing_estimator(d, M):
    """(128, 128) is not a shape whose sticking-the-landing batches the engine takes (the generic route: the single calls, bitwise);
    (256, 128) is the smallest that it does (three steps, W += C^-T eps as one more product per lane)."""
    r = _results(d, M, avi.StickingTheLandingEntropy.code)
    assert r["engine"] == (d == 256)
    if r["engine"]:
        _assert_equals_single_calls(r, True)
    else:
        assert np.array_equal(r["vals"], r["v1"]) and np.array_equal(r["grads"], r["g1"])


def test_objective_mode_against_the_chunked_route():
    """estimate_objective with 163 blocks of 128 samples: three steps of lanes on the engine; a context whose n_mc is not an engine shape
    takes the chunked route over the same (estimate index, sample column) stream (tests/test_gpu_objective_engine.py: 2e-6)."""
    d, M = 128, 128
    rng = np.random.default_rng(d + M)
    q, _ = make_family(rng, d, avi.FULLRANK, np.float32, mu_scale=0.3)
    prob, _ = make_problem(rng, "diag", d, np.float32)
    params, _ = avi.destructure(q)
    eng = avi.MiviContext(np.float32, avi.FULLRANK, d, M, 0, SEED)
    chk = avi.MiviContext(np.float32, avi.FULLRANK, d, 96, 0, SEED)
    eng.set_problem(prob)
    chk.set_problem(prob)
    pe, pc = eng.to_device(params), chk.to_device(params)
    assert eng.batch_takes_engine(pe)
    for ent in (-1, 0, 1):
        ve = float(eng.estimate_objective(pe, 7, n_samples=N * M, entropy=ent).item())
        vc = float(chk.estimate_objective(pc, 7, n_samples=N * M, entropy=ent).item())
        assert abs(ve - vc) <= 2e-6 * max(abs(vc), 1.0), (ent, ve, vc)
    eng.close()
    chk.close()
