"""A schedule of minibatches resident on the device (mivi_logreg_set_batch_schedule / mivi_logreg_seek_batch): the estimates read the
selected batch's rows of the resident data set through the schedule -- the fused minibatch kernel (kernels = 1, csrc/kernels_logreg_batch.hip)
or a device gather and the resident-data kernels (kernels = 2) -- against the f64 oracle on tgt.subsample(batch) with the context's own
eps, at the kernel's edges: n = 700, p in {1, 9, 33, 63} (pad columns), batches of {1, 15, 17, 64, 65, 257} rows (one-row slabs, more than
one slab), repeated rows, row 0 and row n - 1, M in {1, 24, 65}.  Inputs and the per-entry float32 yardstick: tests/batch_schedule_ref.py."""
import numpy as np
import pytest

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import _lib
from oracle import oracle as O
from tests import batch_schedule_ref as R
from tests.helpers import SEED

pytestmark = pytest.mark.gpu

TOL = {np.float32: (2e-5, 5e-5), np.float64: (1e-11, 1e-10)}      # tests/test_gpu_subsampling.py's: value (relative), gradient (norm)
IDX = 5


def _close(v, g, ref, dtype, what):
    vt, gt = TOL[dtype]
    v, g = float(v.item()), g.cpu().numpy().astype(np.float64)
    assert abs(v - ref["value"]) <= vt * abs(ref["value"]), (what, v, ref["value"])
    err = np.linalg.norm(g - ref["grad"])
    assert err <= gt * max(np.linalg.norm(ref["grad"]), 1.0), (what, err)
    return g


@pytest.mark.parametrize("p", R.PS)
@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("fam", [avi.MEANFIELD, avi.FULLRANK], ids=["meanfield", "fullrank"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_every_batch_of_a_schedule_matches_the_oracle_on_both_routes(dtype, fam, variant, p):
    """For kernels in {1, 2} and every seek_batch(k): value and gradient against the oracle on the batch's rows; route 2 bitwise equal to
    set_problem(subsample(prob, batch)) + estimate on a second context; route 1 in f32 per entry of the beta block of d/dmu within
    8 max(|float32 numpy - f64|, 2^-24 sum|terms|)."""
    d = p + 1
    prob, tgt = R.avi_problem(p, variant, dtype), R.oracle_target(p, variant)
    X, y, adj = R.data(p, variant)
    q, q_o = R.family(p, fam, dtype)
    params, _ = avi.destructure(q)
    fam_o = O.MEANFIELD if fam == avi.MEANFIELD else O.FULLRANK
    worst = 0.0
    for M in R.MS:
        ctx, other = (avi.MiviContext(dtype, fam, d, M, 0, SEED) for _ in range(2))
        ctx.set_problem(prob)
        other.set_problem(prob)
        _, eps = ctx.sample(params, IDX)
        eps = eps.cpu().numpy().astype(np.float64)
        for b in R.BATCHES:
            rows = R.schedule(b, p)
            refs = [O.estimate_gradient(O.destructure(q_o), d, fam_o, tgt.subsample(r), eps, O.ENT_CLOSED_FORM, batch_target=True) for r in rows]
            for kernels in (1, 2):
                ctx.set_batch_schedule(rows, kernels=kernels)
                assert ctx.batch_route() == kernels
                for k in (2, 0, 1):
                    ctx.seek_batch(k)
                    what = (M, b, kernels, k)
                    v, g = ctx.estimate_gradient(params, IDX)
                    gh = _close(v, g, refs[k], dtype, what)
                    if kernels == 2:
                        other.set_problem(avi.subsample(prob, rows[k]))
                        v2, g2 = other.estimate_gradient(params, IDX)
                        assert np.array_equal(v.cpu().numpy(), v2.cpu().numpy()) and np.array_equal(g.cpu().numpy(), g2.cpu().numpy()), what
                    elif dtype == np.float32:
                        ratio = R.yardstick_ratio(gh[:p], X, y, rows[k], adj * R.N / b, q_o, eps)
                        worst = max(worst, ratio)
                        assert ratio <= 8.0, (what, ratio)
        ctx.close()
        other.close()
    print(f"worst yardstick ratio {worst:.3f}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_wide_data_sets_size_the_slab_from_the_lds_or_take_the_gather(dtype):
    """The sizes at which the fused kernel takes another path: p = 511 needs more than the 64 KB a kernel gets without asking (f32: 117 KB
    for 32 rows x 24 sample columns) and, in f64, sample-column chunks (24 columns as four chunks of 6: 157 KB); at p = 2047 in f64 not
    even the minimal slab of 8 rows x 4 columns fits 160 KB and kernels = 1 takes the device gather."""
    n, b, M = 300, 65, 24
    for p, route in ((511, 1), (2047, 1 if dtype == np.float32 else 2)):
        d = p + 1
        rng = np.random.default_rng(p)
        X = (rng.normal(size=(n, p)) / np.sqrt(p)).astype(dtype)
        y = (rng.uniform(size=n) < 0.5).astype(np.uint8)
        prob, tgt = avi.LogRegProblem(X, y), O.LogRegTarget(X.astype(np.float64), y)
        q, q_o = R.family(p, avi.MEANFIELD, dtype)
        params, _ = avi.destructure(q)
        ctx = avi.MiviContext(dtype, avi.MEANFIELD, d, M, 0, SEED)
        ctx.set_problem(prob)
        _, eps = ctx.sample(params, IDX)
        eps = eps.cpu().numpy().astype(np.float64)
        rows = np.stack([rng.permutation(n)[:b], rng.integers(0, n, size=b)]).astype(np.int64)
        rows[1, -1] = n - 1
        ctx.set_batch_schedule(rows, kernels=1)
        assert ctx.batch_route() == route
        for k in (1, 0):
            ctx.seek_batch(k)
            ref = O.estimate_gradient(O.destructure(q_o), d, O.MEANFIELD, tgt.subsample(rows[k]), eps, O.ENT_CLOSED_FORM, batch_target=True)
            v, g = ctx.estimate_gradient(params, IDX)
            _close(v, g, ref, dtype, (p, k))
        ctx.close()


@pytest.mark.parametrize("kernels", [1, 2])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_objective_and_value_only_estimates_read_the_selected_batch(dtype, kernels):
    """estimate_objective (want_grad = 0: no X^T r pass) at the context's and at another sample count, the _host entries and the batched
    entries all evaluate the batch seek_batch selected."""
    p, M, b = 9, 24, 65
    d = p + 1
    prob, tgt = R.avi_problem(p, R.VARIANTS[0], dtype), R.oracle_target(p, R.VARIANTS[0])
    q, q_o = R.family(p, avi.FULLRANK, dtype)
    params, _ = avi.destructure(q)
    rows = R.schedule(b, p)
    vt, _ = TOL[dtype]
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, M, 0, SEED)
    ctx.set_problem(prob)
    _, eps = ctx.sample(params, IDX)
    eps = eps.cpu().numpy().astype(np.float64)
    ctx.set_batch_schedule(rows, kernels=kernels)
    for k in (1, 2):
        ctx.seek_batch(k)
        ref = O.estimate_gradient(O.destructure(q_o), d, O.FULLRANK, tgt.subsample(rows[k]), eps, O.ENT_CLOSED_FORM, batch_target=True)
        got = float(ctx.estimate_objective(params, IDX, entropy=avi.ClosedFormEntropy.code).item())
        assert abs(got - ref["value"]) <= vt * abs(ref["value"]), (k, got, ref["value"])
        assert abs(float(ctx.estimate_objective_host(params, IDX, entropy=avi.ClosedFormEntropy.code)) - ref["value"]) <= vt * abs(ref["value"])
        vh, gh = ctx.estimate_gradient_host(params, IDX)
        assert abs(float(vh) - ref["value"]) <= vt * abs(ref["value"])
        v1, g1 = ctx.estimate_gradient(params, IDX)
        assert np.array_equal(gh, g1.cpu().numpy())
        # all estimates of a batched call use the same batch: row i of _each is the single call at IDX + i, _n (one graph) leaves the last
        vals, grads = ctx.estimate_gradient_each(params, IDX, 3)
        ctx.synchronize()
        singles = [ctx.estimate_gradient(params, IDX + i) for i in range(3)]
        singles = [(float(v.item()), g.cpu().numpy().copy()) for v, g in singles]
        for i in range(3):
            assert float(vals[i].item()) == singles[i][0] and np.array_equal(grads[i].cpu().numpy(), singles[i][1]), (k, i)
        vb, gb = ctx.empty(1), ctx.empty(ctx.params_len)
        ctx.estimate_gradient_n(ctx.to_device(params), IDX, 3, vb, gb)
        ctx.synchronize()
        assert float(vb.item()) == singles[2][0] and np.array_equal(gb.cpu().numpy(), singles[2][1]), k
    # more samples than the context's n_mc: 2 M columns of the same eps stream
    ctx.seek_batch(0)
    big = avi.MiviContext(dtype, avi.FULLRANK, d, 2 * M, 0, SEED)
    big.set_problem(prob)
    _, eps2 = big.sample(params, IDX)
    ref2 = O.estimate_gradient(O.destructure(q_o), d, O.FULLRANK, tgt.subsample(rows[0]), eps2.cpu().numpy().astype(np.float64), O.ENT_CLOSED_FORM,
                               batch_target=True)
    got2 = float(ctx.estimate_objective(params, IDX, n_samples=2 * M, entropy=avi.ClosedFormEntropy.code).item())
    assert abs(got2 - ref2["value"]) <= vt * abs(ref2["value"])
    big.close()
    ctx.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_schedule_full_rows_schedule_on_one_context(dtype):
    """schedule -> the full data set (n_batches = 0) -> select_rows -> schedule on ONE context: every estimate matches the oracle on its
    own rows (the schedule and the row selection replace each other and share the gather buffers)."""
    p, M = 33, 24
    d = p + 1
    prob, tgt = R.avi_problem(p, R.VARIANTS[1], dtype), R.oracle_target(p, R.VARIANTS[1])
    q, q_o = R.family(p, avi.MEANFIELD, dtype)
    params, _ = avi.destructure(q)
    ctx = avi.MiviContext(dtype, avi.MEANFIELD, d, M, 0, SEED)
    ctx.set_problem(prob)
    _, eps = ctx.sample(params, IDX)
    eps = eps.cpu().numpy().astype(np.float64)

    def check(t, what):
        ref = O.estimate_gradient(O.destructure(q_o), d, O.MEANFIELD, t, eps, O.ENT_CLOSED_FORM, batch_target=True)
        v, g = ctx.estimate_gradient(params, IDX)
        _close(v, g, ref, dtype, what)

    big, small = R.schedule(257, p), R.schedule(17, p)
    ctx.set_batch_schedule(big, kernels=1)
    ctx.seek_batch(1)
    check(tgt.subsample(big[1]), "schedule, fused")
    ctx.set_batch_schedule(None)
    assert ctx.batch_route() == 0
    check(tgt, "full data set")
    ctx.set_problem(avi.subsample(prob, small[2]))
    check(tgt.subsample(small[2]), "select_rows")
    ctx.set_batch_schedule(small, kernels=2)
    assert ctx.batch_route() == 2
    check(tgt.subsample(small[0]), "schedule, gather: batch 0 after the call")
    ctx.set_batch_schedule(big, kernels=0)            # by size: far below the matrix-core threshold -> the fused kernel
    assert ctx.batch_route() == 1
    ctx.seek_batch(2)
    check(tgt.subsample(big[2]), "schedule, by size")
    ctx.set_problem(avi.subsample(prob, big[0]))      # a row selection replaces the schedule
    assert ctx.batch_route() == 0
    check(tgt.subsample(big[0]), "select_rows after a schedule")
    ctx.set_problem(prob)
    check(tgt, "full data set again")
    ctx.close()


def test_refusals_leave_the_previous_selection_in_force():
    p, M, b = 9, 24, 15
    d = p + 1
    dtype = np.float32
    prob, tgt = R.avi_problem(p, R.VARIANTS[0], dtype), R.oracle_target(p, R.VARIANTS[0])
    q, q_o = R.family(p, avi.FULLRANK, dtype)
    params, _ = avi.destructure(q)
    rows = R.schedule(b, p)
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, M, 0, SEED)
    with pytest.raises(avi.MiviError) as e:
        ctx.set_batch_schedule(rows, likeadj=2.0)
    assert e.value.status == _lib.ERR_NO_TARGET
    ctx.set_problem(prob)
    _, eps = ctx.sample(params, IDX)
    eps = eps.cpu().numpy().astype(np.float64)
    ctx.set_batch_schedule(rows, kernels=1)
    ctx.seek_batch(1)

    def still_batch_1():
        ref = O.estimate_gradient(O.destructure(q_o), d, O.FULLRANK, tgt.subsample(rows[1]), eps, O.ENT_CLOSED_FORM, batch_target=True)
        v, g = ctx.estimate_gradient(params, IDX)
        _close(v, g, ref, dtype, "after a refusal")

    bad = rows.copy()
    bad[2, 3] = R.N
    for call in (lambda: ctx.set_batch_schedule(bad), lambda: ctx.set_batch_schedule(-rows - 1), lambda: ctx.set_batch_schedule(rows, likeadj=0.0),
                 lambda: ctx.seek_batch(3), lambda: ctx.seek_batch(-1),
                 lambda: ctx.optimize_loop_batches(ctx.to_device(params).clone(), 3, 0, 0, first_batch=1, eta=1e-3),
                 lambda: ctx.optimize_loop_batches(ctx.to_device(params).clone(), 1, 0, 0, first_batch=-1, eta=1e-3)):
        with pytest.raises(avi.MiviError) as e:
            call()
        assert e.value.status == _lib.ERR_BAD_ARG, str(e.value)
        still_batch_1()
    # the entries that read the data set themselves refuse a scheduled context before touching a buffer
    with pytest.raises(avi.MiviError) as e:
        ctx.gauss_expected_grad_hess_host(params, IDX, second_order=True)
    assert e.value.status == _lib.ERR_UNSUPPORTED and "schedule" in str(e.value)
    with pytest.raises(avi.MiviError) as e:
        ctx.estimate_partials(ctx.to_device(params), IDX)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    still_batch_1()
    ctx.set_batch_schedule(None)
    ctx.gauss_expected_grad_hess_host(params, IDX, second_order=True)      # ... and take it again without one
    ctx.close()
