"""subsampling.plan_batches on the host: a run of `estimate_gradient_` steps of a SubsampledObjective planned ahead -- the batches and the
estimate indices a schedule resident on the device is built from (MiviContext.set_batch_schedule, mivi_optimize_loop_batches) -- against
the step-by-step walk of src/reshuffling.jl:38-60 it must restate; and the float32 yardstick of the fused minibatch kernel on its own
inputs (tests/batch_schedule_ref.py)."""
import numpy as np
import pytest

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import subsampling as S
from oracle import oracle as O
from tests import batch_schedule_ref as R
from tests.helpers import SEED, make_family

CASES = [(8, 1), (8, 3), (10, 4), (5, 8), (64, 16)]


def _walk(rng, sub, st, n_steps):
    """the plan's outputs from the walk `estimate_gradient_` does: a subsampling step, then the estimate's index"""
    rows, idx, infos = [], [], []
    for _ in range(n_steps):
        batch, st, inf = S.step_subsampling(rng, sub, st, True)
        rows.append(np.asarray(batch))
        idx.append(rng.next_index())
        infos.append(inf)
    return rows, idx, infos, st


def _same_state(a, b):
    return (a.epoch == b.epoch and len(a.batches) == len(b.batches) and
            all(sa == sb and np.array_equal(ba, bb) for (sa, ba), (sb, bb) in zip(a.batches, b.batches)))


@pytest.mark.parametrize("n,batchsize", CASES)
def test_plan_equals_the_step_by_step_walk(n, batchsize):
    sub = avi.ReshufflingBatchSubsampling(np.arange(n), batchsize)
    n_steps = 3 * len(sub) + 2          # (three epochs and into the fourth)
    b_eff = min(batchsize, n)
    r1, r2 = avi.PhiloxRNG(SEED, 5), avi.PhiloxRNG(SEED, 5)
    st1, st2 = S.init_subsampling(r1, sub), S.init_subsampling(r2, sub)
    rows, idx, infos, st1n = S.plan_batches(r1, sub, st1, n_steps)
    w_rows, w_idx, w_infos, st2n = _walk(r2, sub, st2, n_steps)
    assert rows.shape == (n_steps, b_eff) and rows.dtype == np.int64 and idx.dtype == np.uint64 and idx.shape == (n_steps,)
    assert all(len(b) == b_eff for b in w_rows)                      # every planned batch has b_eff rows
    assert np.array_equal(rows, np.stack(w_rows)) and [int(i) for i in idx] == w_idx and infos == w_infos
    assert _same_state(st1n, st2n) and r1.counter == r2.counter
    assert all(set(i) == {"epoch", "step"} for i in infos)
    # planning in two chunks equals planning in one
    r3 = avi.PhiloxRNG(SEED, 5)
    st3 = S.init_subsampling(r3, sub)
    cut = n_steps // 2 + 1
    ra, ia, fa, st3 = S.plan_batches(r3, sub, st3, cut)
    rb, ib, fb, st3 = S.plan_batches(r3, sub, st3, n_steps - cut)
    assert np.array_equal(np.concatenate([ra, rb]), rows) and np.array_equal(np.concatenate([ia, ib]), idx) and fa + fb == infos
    assert _same_state(st3, st1n) and r3.counter == r1.counter
    # inside a step the shuffle's index comes before the estimate's: the indices increase, and skip one exactly where an epoch ended
    gaps = np.diff(idx.astype(np.int64))
    ends = np.array([infos[t + 1]["epoch"] != infos[t]["epoch"] for t in range(n_steps - 1)])
    assert np.array_equal(gaps, np.where(ends, 2, 1))


@pytest.mark.parametrize("n,batchsize", CASES)
def test_every_epoch_of_the_plan_covers_the_data_set(n, batchsize):
    """... except for a trailing short batch, which the first batch of the next epoch replaces (drop_trailing_batch_if_too_small)."""
    sub = avi.ReshufflingBatchSubsampling(np.arange(n), batchsize)
    rng = avi.PhiloxRNG(SEED, 9)
    st = S.init_subsampling(rng, sub)
    L = len(sub)                                        # batches of a shuffle
    short = n % batchsize if n > batchsize else 0       # rows of the trailing batch that is replaced
    if short == 0:      # L steps are one shuffle (a data set below the batch size: one batch, all of it)
        rows, _, infos, _ = S.plan_batches(rng, sub, st, 3 * L)
        for e in range(3):
            assert np.array_equal(np.sort(rows[e * L:(e + 1) * L].reshape(-1)), np.arange(n))
        assert [i["step"] for i in infos[:L]] == list(range(1, L + 1))
        return
    # a shuffle's batches 1 .. L - 1 are taken, its short batch L is not: the step that would take it takes batch 1 of the next shuffle and
    # reports the next epoch, so the steps that report one epoch are that shuffle's full batches -- disjoint, all rows but `short` of them
    rows, _, infos, _ = S.plan_batches(rng, sub, st, 3 * (L - 1))
    for e in (1, 2, 3):
        mine = [t for t, inf in enumerate(infos) if inf["epoch"] == e]
        assert [infos[t]["step"] for t in mine] == list(range(1, L))
        seen = rows[mine].reshape(-1)
        assert seen.size == n - short and np.unique(seen).size == seen.size and seen.min() >= 0 and seen.max() < n


@pytest.mark.parametrize("batchsize", [1, 2, 4, 8])
def test_mean_of_the_planned_minibatch_gradients_is_the_full_gradient(batchsize):
    """test/general/subsampledobj.jl:62-89 on the planned schedule: n % batchsize == 0, the same samples for every batch -- the f64 oracle
    gradient averaged over one epoch's batches is the gradient on the whole data set."""
    n, p = 8, 3
    d = p + 1
    rng = np.random.default_rng(4)
    X = rng.normal(size=(n, p)) / np.sqrt(p)
    y = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    tgt = O.LogRegTarget(X, y, "logsigma_normal", 1.0)
    _, q_o = make_family(rng, d, avi.FULLRANK, np.float64, mu_scale=0.1)
    eps = rng.normal(size=(d, 10))
    full = O.estimate_gradient(O.destructure(q_o), d, O.FULLRANK, tgt, eps, O.ENT_CLOSED_FORM)["grad"]
    sub = avi.ReshufflingBatchSubsampling(np.arange(n), batchsize)
    prng = avi.PhiloxRNG(SEED)
    rows, _, infos, _ = S.plan_batches(prng, sub, S.init_subsampling(prng, sub), len(sub))
    assert np.array_equal(np.sort(rows.reshape(-1)), np.arange(n))
    grads = [O.estimate_gradient(O.destructure(q_o), d, O.FULLRANK, tgt.subsample(b), eps, O.ENT_CLOSED_FORM)["grad"] for b in rows]
    assert np.allclose(np.mean(grads, axis=0), full, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("fam", [avi.MEANFIELD, avi.FULLRANK], ids=["meanfield", "fullrank"])
@pytest.mark.parametrize("p", R.PS)
def test_float32_in_another_summation_order_stays_within_a_factor_of_four(p, fam):
    """The yardstick of tests/test_gpu_batch_schedule.py on its own inputs: a float32 numpy evaluation of the beta block of d value / d mu
    that adds the batch's rows in slabs of 32 (partial sums added in float64 -- the order the fused minibatch kernel documents) or of 7
    stays within 4 max(|float32 evaluation - float64|, 2^-24 sum|terms|) per entry, so the kernel's bound of 8 leaves a factor of two."""
    X, y, adj = R.data(p)
    _, q_o = R.family(p, fam, np.float32)
    worst = 0.0
    for b in R.BATCHES:
        rows = R.schedule(b, p)
        for M in R.MS:
            eps = O.philox_normal(SEED, 5, p + 1, 0, M).astype(np.float64)
            for k in range(rows.shape[0]):
                for slab in (32, 7):
                    worst = max(worst, R.yardstick_ratio(None, X, y, rows[k], adj * R.N / b, q_o, eps, slab=slab))
    assert worst <= 4.0, worst
