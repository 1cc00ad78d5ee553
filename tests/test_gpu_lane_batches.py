"""The lane-batched second-generation route as the DEFAULT routing still reaches it (no environment switch): one-GPU batches the batch
engine refuses -- d below 128, the dense target off whole 128-tiles -- and the pipelined peer-to-peer sharded batch at world 1.  Four
contexts' product kernels go out as one launch (k_fr_prod32m at these shapes), likewise their VJP kernels (k_fr_vjp32m), first draws and
closing value kernels; every batch must equal the single calls of a second context, bitwise on one GPU.  Each one-GPU case first asserts
that the engine does NOT take the configuration, so a routing change fails here instead of silently testing the engine."""
import numpy as np
import pytest

import advancedvi_jl_amd as avi
from tests.helpers import SEED, assert_batch_matches_single, make_family, make_problem

pytestmark = pytest.mark.gpu


def _pair(d, M, kind, ent, seed):
    rng = np.random.default_rng(seed)
    q, _ = make_family(rng, d, avi.FULLRANK, np.float32)
    prob, _ = make_problem(rng, kind, d, np.float32)
    params, _ = avi.destructure(q)
    ctx = avi.MiviContext(np.float32, avi.FULLRANK, d, M, ent, SEED)
    ctx.set_problem(prob)
    ref = avi.MiviContext(np.float32, avi.FULLRANK, d, M, ent, SEED)
    ref.set_problem(prob)
    return ctx, ref, ctx.to_device(params), ref.to_device(params)


def _check_batches(ctx, ref, p, pr, lengths, ulps, idx=3):
    assert not ctx.batch_takes_engine(p)
    v, g = ctx.empty(1), ctx.empty(ctx.params_len)
    for n in lengths:
        g.fill_(float("nan"))
        ctx.estimate_gradient_n(p, idx, n, v, g)
        ctx.synchronize()
        v1, g1 = ref.estimate_gradient(pr, idx + n - 1)
        assert_batch_matches_single(v.item(), v1.item(), g.cpu().numpy(), g1.cpu().numpy(), engine=False, what=n, ulps=ulps)
        idx += n + 2   # (a gap: the next call is not in order -- the device-side counter is set again)


@pytest.mark.parametrize("kind", ["diag", "dense"])
def test_smallest_shape_every_step_pattern_equals_single_calls(kind):
    """(64, 128): one 64-row block, below the engine's d >= 128.  One full step of four lanes, a partial step, the 4 -> 8 context switch at
    12, two branches, partial last steps on both branches."""
    ctx, ref, p, pr = _pair(64, 128, kind, 0, 31)
    _check_batches(ctx, ref, p, pr, (4, 5, 8, 11, 12, 13, 20, 27), ulps=0)
    ctx.close()
    ref.close()


def test_dense_target_off_whole_tiles_equals_single_calls():
    """(192, 128): the engine refuses the dense target off whole 128-tiles."""
    ctx, ref, p, pr = _pair(192, 128, "dense", 0, 32)
    _check_batches(ctx, ref, p, pr, (4, 7, 20), ulps=0)
    ctx.close()
    ref.close()


def test_stl_without_the_second_generation_solve_takes_forked_chains():
    """(64, 128), sticking-the-landing: stl2_shape_ok is false at d = 64, so the batch runs as forked chains with one context per branch.
    The value may land one f32 spacing apart (the Monte Carlo entropy's sum(eps^2) note of tests/test_gpu_batches.py)."""
    ctx, ref, p, pr = _pair(64, 128, "diag", 3, 33)
    _check_batches(ctx, ref, p, pr, (16, 21), ulps=1)
    ctx.close()
    ref.close()


def test_pipelined_p2p_batches_at_world_one_then_a_one_gpu_batch():
    """estimate_gradient_dist_n on the peer-to-peer route at world 1: the lane-batched compute chain beside the persistent exchange kernel
    (length 3 is shorter than a group: the one-at-a-time chain).  The sharded finalisation sums in another order than the one-GPU value
    kernel: the tolerances of test_mixed_call_sequences_keep_every_result_exact.  Then one in-order one-GPU batch on the same context: the
    children change their index stride."""
    ctx, ref, p, pr = _pair(64, 128, "diag", 0, 34)
    ctx.p2p_attach([ctx.p2p_export(0, 1)])
    ctx.comm_set_route("p2p")
    v, g = ctx.empty(1), ctx.empty(ctx.params_len)
    idx = 7
    for n in (3, 4, 9, 20):
        g.fill_(float("nan"))
        ctx.estimate_gradient_dist_n(p, idx, n, v, g)
        ctx.synchronize()
        v1, g1 = ref.estimate_gradient(pr, idx + n - 1)
        gn, g1n = g.cpu().numpy(), g1.cpu().numpy()
        assert abs(float(v.item()) - float(v1.item())) <= 2e-6 * abs(float(v1.item())), n
        assert np.linalg.norm(gn - g1n) <= 5e-6 * max(1.0, float(np.linalg.norm(g1n))), n
        idx += n
    _check_batches(ctx, ref, p, pr, (20,), ulps=0, idx=idx)
    ctx.close()
    ref.close()
