"""mivi_optimize_loop_many / avi.optimize_many: K independent small runs in one launch, workgroup k = run k.

The reference for run k is a single-run mivi_optimize_loop on a FRESH context created with run k's seed and target (itself pinned to the
oracle by tests/test_gpu_optimize.py and tests/test_gpu_loop_oracle.py).  Where the single run is one workgroup too, run k must equal it
bit for bit: the many-run kernel is the single-run kernel behind a prologue that moves its pointers to the run's slices."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import advancedvi_jl_amd as avi
from oracle import oracle as O
from tests.helpers import SEED

OPT = avi._optimize   # the module (the package exports the function `optimize` under that name)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MANY = 16                      # LOOP_MANY, include/mivi.h (mivi_batch_info what = 7)
LR_SMALL, FR_SMALL = 2, 4
DESCENT, ADAM, DOG, DOWG = range(4)
# rule x operator x averager: the fast class (Descent / default Adam, at most ClipScale, no averager) and the general one
COMBOS_A = [(DESCENT, 0, 0), (DESCENT, 1, 1), (DESCENT, 2, 1), (ADAM, 1, 0), (ADAM, 0, 1), (DOG, 1, 0), (DOG, 2, 1), (DOWG, 1, 1), (DOWG, 2, 0), (DOWG, 0, 0)]
# ... as tests/test_gpu_optimize.py::test_logreg_small_loop enumerates them: (dowg, prox, poly), (adam, clip, none), (descent, clip, poly), (dog, clip, none)
COMBOS_B = [(DOWG, 2, 1), (ADAM, 1, 0), (DESCENT, 1, 1), (DOG, 1, 0)]
FILL = 1e-3                    # what the tests put above the diagonal of C (small: mivi_dog_init's norm runs over the whole vector)
LDS_BYTES = 160 * 1024         # what a workgroup may take on gfx950 (hipDeviceAttributeMaxSharedMemoryPerBlock)


def _state(ctx, p, rule, alpha=1e-2):
    if rule == ADAM:
        return ctx.empty(2 * p.numel()).zero_()
    if rule in (DOG, DOWG):
        st = ctx.dog_state()
        ctx.dog_init(p, st, alpha)
        return st
    return None


def _bytes(t):
    return None if t is None else t.cpu().numpy().copy()


class Runs:
    """K runs of one shape: their seeds, first indices, step sizes, initial parameters and targets, and one fresh context per run -- the
    single-run reference -- made once and shared by every combination of a test."""

    def __init__(self, dtype, family, d, M, ent, K, make_prob, seed=3, p0s=None, tight=False):
        rng = np.random.default_rng(seed)
        self.dtype, self.family, self.d, self.M, self.ent, self.K = dtype, family, d, M, ent, K
        self.seeds = [int(s) for s in rng.integers(1, 2**63 - 1, size=K)]
        self.idx0 = [int(i) for i in rng.integers(0, 1000, size=K)]
        self.etas = [float(e) for e in rng.uniform(2e-3, 2e-2, size=K)]
        self.descent_scale = 1e-2 if tight else 1.0   # (the regression: Descent needs steps of 1e-4, as in test_logreg_small_loop)
        lo, hi, off, ms = (0.4, 0.6, 0.02, 0.1) if tight else (0.5, 1.5, 0.1, 0.3)
        self.probs = [make_prob(rng, k) for k in range(K)]
        if p0s is None:
            p0s = []
            for k in range(K):
                mu = (ms * rng.normal(size=d)).astype(dtype)
                if family == avi.FULLRANK:
                    C = (np.diag(rng.uniform(lo, hi, size=d)) + off * np.tril(rng.normal(size=(d, d)), -1)).astype(dtype)
                    p = avi.destructure(avi.FullRankGaussian(mu, C))[0].astype(dtype)
                    p[np.concatenate([np.zeros(d, bool), np.triu(np.ones((d, d), bool), 1).T.reshape(-1)])] = FILL   # above the diagonal: never read, never written
                    p0s.append(p)
                else:
                    p0s.append(avi.destructure(avi.MeanFieldGaussian(mu, rng.uniform(lo, hi, size=d).astype(dtype)))[0])
        self.p0s = [np.asarray(p, dtype=dtype) for p in p0s]
        self.ctxs = []
        for k in range(K):
            c = avi.MiviContext(dtype, family, d, M, ent, self.seeds[k])
            c.set_problem(self.probs[k])
            self.ctxs.append(c)

    def eta(self, k, rule):
        return self.etas[k] * (self.descent_scale if rule == DESCENT else 1.0)

    def close(self):
        for c in self.ctxs:
            c.close()

    def single(self, k, T, rule, op, avg, t0=0, calls=None):
        """run k alone, on its own context: (params, optimiser state, average, elbo record) as arrays"""
        c = self.ctxs[k]
        p = c.to_device(self.p0s[k]).clone()
        st = _state(c, p, rule)
        ap = p.clone() if avg else None
        elbo = c.empty(T)
        done = 0
        for n in ([T] if calls is None else calls):
            c.optimize_loop(p, n, self.idx0[k] + done, t0 + done, rule=rule, op=op, averager=avg, eta=self.eta(k, rule), clip_epsilon=1e-5,
                            opt_state=st, avg_params=ap, elbo=elbo[done:done + n])
            done += n
        c.synchronize()
        return _bytes(p), _bytes(st), _bytes(ap), _bytes(elbo)

    def many(self, ctx, T, rule, op, avg, runs=None, calls=None, **target):
        """the runs `runs` (default: all) in one mivi_optimize_loop_many call per entry of `calls` on `ctx`"""
        runs = list(range(self.K)) if runs is None else runs
        ps = [ctx.to_device(self.p0s[k]).clone() for k in runs]
        sts = [_state(ctx, p, rule) for p in ps]
        import torch
        p = torch.stack(ps).contiguous()
        st = torch.stack(sts).contiguous() if rule != DESCENT else None
        ap = p.clone() if avg else None
        elbo = ctx.empty(len(runs) * T)
        done, status = 0, np.zeros(len(runs), np.int32)
        for n in ([T] if calls is None else calls):
            e = ctx.empty(len(runs) * n)
            status |= ctx.optimize_loop_many(p, len(runs), n, [self.idx0[k] + done for k in runs], done, seeds=[self.seeds[k] for k in runs],
                                             etas=[self.eta(k, rule) for k in runs], rule=rule, op=op, averager=avg, clip_epsilon=1e-5, opt_state=st,
                                             avg_params=ap, elbo=e, **target)
            elbo.view(len(runs), T)[:, done:done + n] = e.view(len(runs), n)
            done += n
        L = len(runs)
        return (_bytes(p).reshape(L, -1), None if st is None else _bytes(st).reshape(L, -1), None if ap is None else _bytes(ap).reshape(L, -1),
                _bytes(elbo).reshape(L, T), status)


def _same(got, want, what):
    for name, a, b in zip(("params", "state", "average", "elbo"), got, want):
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            assert np.array_equal(a, b, equal_nan=True), (what, name, np.max(np.abs(a.astype(np.float64) - b.astype(np.float64))))


def _diag_prob(dtype, d):
    return lambda rng, k: avi.DiagNormalProblem(rng.normal(size=d).astype(dtype), rng.uniform(0.5, 2.0, size=d).astype(dtype))


def _targets(R, runs=None):
    runs = range(R.K) if runs is None else runs
    return dict(means=np.stack([R.probs[k].mean for k in runs]), stds=np.stack([R.probs[k].std for k in runs]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(1, 1, 0), (3, 7, 2), (10, 1, 0), (32, 24, 1), (32, 16, 3)], ids=["d1", "ragged-mc", "reference-bench", "largest-zerograd", "stl"])
def test_class_a_is_the_single_run_bit_for_bit(shape, dtype):
    """Five full-rank runs on diagonal-Gaussian targets with distinct seeds, first indices, initial C, eta and target, every rule x operator x
    averager: parameters (entries above the diagonal of C included: untouched), optimiser state, running average and ELBO record of run k
    are bitwise those of mivi_optimize_loop on a fresh context with run k's seed and target; a second call that continues (t0, indices,
    Adam's t) is bitwise one call of the total length; the route is LOOP_MANY | small full-rank."""
    d, M, ent = shape
    R = Runs(dtype, avi.FULLRANK, d, M, ent, 5, _diag_prob(dtype, d))
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, M, ent, SEED)
    ctx.set_problem(R.probs[0])
    for rule, op, avg in COMBOS_A:
        got = R.many(ctx, 5, rule, op, avg, **_targets(R))
        assert ctx.last_loop() == (MANY | FR_SMALL)
        assert not got[4].any(), (rule, op, avg, got[4])
        cont = R.many(ctx, 5, rule, op, avg, calls=[3, 2], **_targets(R))
        for k in range(R.K):
            want = R.single(k, 5, rule, op, avg)
            _same([None if g is None else g[k] for g in got[:4]], want, (rule, op, avg, k))
            _same([None if g is None else g[k] for g in cont[:4]], want, ("continued", rule, op, avg, k))
            if d > 1:
                up = np.concatenate([np.zeros(d, bool), np.triu(np.ones((d, d), bool), 1).T.reshape(-1)])
                assert np.all(got[0][k][up] == dtype(FILL))
    R.close()
    ctx.close()


def test_class_a_matches_the_oracle_restatement():
    """One f64 case held to the restatement tests/test_gpu_optimize.py::test_small_fullrank_loop uses, at its 1e-11: the oracle's gradient on
    the run's own eps (its seed, its indices), numpy Descent / Adam with the run's eta, ClipScale, three steps."""
    d, M, ent, dtype = 10, 8, 0, np.float64
    R = Runs(dtype, avi.FULLRANK, d, M, ent, 5, _diag_prob(dtype, d))
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, M, ent, SEED)
    ctx.set_problem(R.probs[0])
    low = np.concatenate([np.ones(d, bool), np.tril(np.ones((d, d), bool)).T.reshape(-1)])
    for rule in (DESCENT, ADAM):
        got = R.many(ctx, 3, rule, 1, 0, **_targets(R))
        for k in range(R.K):
            x = R.p0s[k].astype(np.float64).copy()
            x[~low] = 0.0
            ost = (np.zeros_like(x), np.zeros_like(x))
            tgt = O.DiagNormalTarget(R.probs[k].mean, R.probs[k].std)
            for t in range(3):
                _, eps = R.ctxs[k].sample(x, R.idx0[k] + t)
                ref = O.estimate_gradient(x, d, avi.FULLRANK, tgt, eps.cpu().numpy().astype(np.float64), ent)
                if rule == DESCENT:
                    x = O.descent_step(x, ref["grad"], R.eta(k, rule))
                else:
                    x, ost = O.adam_step(x, ref["grad"], ost, t + 1, R.eta(k, rule))
                x = O.clip_scale(x, d, avi.FULLRANK, 1e-5)
            err = np.max(np.abs(got[0][k][low] - x[low]))
            assert err <= 1e-11 * max(1.0, np.max(np.abs(x[low]))), (rule, k, err)
    R.close()
    ctx.close()


def test_more_runs_than_compute_units():
    """K = 260 > 256 CUs at d = 4, n_mc = 2, three steps of Adam + ClipScale + averaging: the surplus workgroups queue (nothing waits for
    another workgroup).  Runs 0, 255, 256 and 259 bitwise -- a run index that wraps or a table read at the wrong stride shows here."""
    dtype, d, M = np.float32, 4, 2
    R = Runs(dtype, avi.FULLRANK, d, M, 0, 260, _diag_prob(dtype, d))
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, M, 0, SEED)
    ctx.set_problem(R.probs[0])
    got = R.many(ctx, 3, ADAM, 1, 1, **_targets(R))
    assert not got[4].any()
    for k in (0, 255, 256, 259):
        _same([g[k] for g in got[:4]], R.single(k, 3, ADAM, 1, 1), k)
    R.close()
    ctx.close()


def _lr_lds(es, n, p, M, fr, resident):
    """lr_small_lds(G = 1) of csrc/kernels_logreg_small.hip, restated"""
    d = p + 1
    rc = 256 if M <= 16 else (128 if M <= 32 else 64)
    nloc = n + 1
    b = (16 + 64 * 4 + 2 * 64) * 8 + ((d * d if fr else d) + d + 3 * M * d + M * rc + 2 * 256) * es
    if resident:
        b += p * (nloc | 1) * es
    return b + ((nloc + 15) & ~15)


def _lr_groups(n, p, M):
    """lr_small_groups, restated: the workgroups mivi_optimize_loop splits a run over"""
    return max(1, min((n * p * M + (1 << 14) - 1) >> 14, 64, n // 16))


def _logreg_runs(dtype, fam, n, p, M, variant, K, per_run_x):
    rng0 = np.random.default_rng(21)
    X0 = (rng0.normal(size=(n, p)) / np.sqrt(p)).astype(dtype)

    def make(rng, k):
        X = (rng.normal(size=(n, p)) / np.sqrt(p)).astype(dtype) if per_run_x else X0
        beta = rng.normal(size=p) * 0.5
        y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-X.astype(np.float64) @ beta))).astype(np.uint8)
        return avi.LogRegProblem(X, y, variant=variant)
    family = avi.MEANFIELD if fam == "meanfield" else avi.FULLRANK
    return Runs(dtype, family, p + 1, M, 0, K, make, tight=True)


def _lr_target(ctx, R, per_run_x, runs=None):
    import torch
    runs = range(R.K) if runs is None else runs
    y = torch.as_tensor(np.stack([R.probs[k].y for k in runs])).to(ctx.tdevice).contiguous()
    if not per_run_x:
        return dict(y=y)   # X: the context's resident matrix
    X = torch.as_tensor(np.stack([np.ascontiguousarray(R.probs[k].X.T).reshape(-1) for k in runs])).to(ctx.tdevice).contiguous()
    return dict(y=y, X=X, x_stride=X.shape[1])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("per_run_x", [False, True], ids=["shared-X", "per-run-X"])
@pytest.mark.parametrize("case", [("fullrank", 40, 5, 2, "logsigma_normal"), ("meanfield", 40, 5, 2, "lognormal_exp_bijector"),
                                  ("fullrank", 208, 60, 1, "lognormal_exp_bijector"), ("meanfield", 208, 60, 1, "logsigma_normal")],
                         ids=["fullrank-40x5", "meanfield-40x5", "readme-sonar-fullrank", "readme-sonar-meanfield"])
def test_class_b_is_the_single_run_bit_for_bit(case, per_run_x, dtype):
    """Small logistic regressions for which lr_small_groups is 1, so the single-run loop is one workgroup too (X resident in LDS): both
    families, both variants, a shared X (the context's) with per-run y, and per-run X; the combinations of test_logreg_small_loop.  Bitwise
    the single-run loop on a fresh context with the run's seed and data; a continued call is one call of the total length."""
    fam, n, p, M, variant = case
    assert _lr_groups(n, p, M) == 1 and _lr_lds(np.dtype(dtype).itemsize, n, p, M, fam == "fullrank", True) <= LDS_BYTES
    R = _logreg_runs(dtype, fam, n, p, M, variant, 5, per_run_x)
    ctx = avi.MiviContext(dtype, R.family, p + 1, M, 0, SEED)
    ctx.set_problem(R.probs[0])
    for rule, op, avg in COMBOS_B:
        got = R.many(ctx, 4, rule, op, avg, calls=[3, 1], **_lr_target(ctx, R, per_run_x))
        assert ctx.last_loop() == (MANY | LR_SMALL)
        assert not got[4].any()
        for k in range(R.K):
            _same([None if g is None else g[k] for g in got[:4]], R.single(k, 4, rule, op, avg), (rule, op, avg, k))
    R.close()
    ctx.close()


def _smallest_streamed_n(es, p, M, fr):
    n = 16
    while _lr_lds(es, n, p, M, fr, True) <= LDS_BYTES:
        n += 1
    return n


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_class_b_streams_an_x_that_does_not_fit_the_lds(dtype):
    """The smallest n x p whose X does not fit the LDS beside the kernel's other arrays, at one sample per step (the arrays that grow with
    n_mc take LDS from X: with more samples a smaller X already streams, e.g. n near 28 300 at p = 1, n_mc = 32 in f32 -- the path is the
    same): lr_small_lds charges the run's y (n bytes) as well, so for a given n p the bytes are fewest at p = 1 -- f32: n = 31504,
    f64: n = 17155 (mean-field; 160 KiB of LDS).  Such a
    matrix holds more than 2^14 entries in either precision, so the single-run loop always splits its rows over several workgroups
    (lr_small_groups: 2) and no single-workgroup reference exists outside this entry.  Two checks instead: run k of five equals the SAME
    entry called with that run alone bit for bit (the run index, the strides, per-run y and per-run X on the streamed path), and it stays
    within test_logreg_small_loop's bound of the single-run loop (2e-4 relative in f32, 1e-9 in f64), which sums the rows in another order."""
    es = np.dtype(dtype).itemsize
    p, M = 1, 1
    n = _smallest_streamed_n(es, p, M, False)
    assert n == (31504 if dtype == np.float32 else 17155)
    assert _lr_lds(es, n, p, M, False, False) <= LDS_BYTES and _lr_groups(n, p, M) > 1
    R = _logreg_runs(dtype, "meanfield", n, p, M, "logsigma_normal", 5, True)
    ctx = avi.MiviContext(dtype, R.family, p + 1, M, 0, SEED)
    ctx.set_problem(R.probs[0])
    tol = 2e-4 if dtype == np.float32 else 1e-9
    for rule, op, avg in COMBOS_B:
        got = R.many(ctx, 3, rule, op, avg, **_lr_target(ctx, R, True))
        assert ctx.last_loop() == (MANY | LR_SMALL) and not got[4].any()
        for k in (0, 4):
            alone = R.many(ctx, 3, rule, op, avg, runs=[k], **_lr_target(ctx, R, True, runs=[k]))
            _same([None if g is None else g[k] for g in got[:4]], [None if g is None else g[0] for g in alone[:4]], (rule, k))
            want = R.single(k, 3, rule, op, avg)
            err = np.max(np.abs(got[0][k].astype(np.float64) - want[0].astype(np.float64))) / max(1.0, np.max(np.abs(want[0])))
            assert err <= tol, (rule, k, err)
    R.close()
    ctx.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", [("fullrank", 1000, 16, 2, "logsigma_normal"), ("meanfield", 3001, 16, 2, "lognormal_exp_bijector")],
                         ids=["two-workgroups-fullrank", "six-workgroups-meanfield"])
def test_class_b_one_workgroup_where_the_single_run_takes_several(case, dtype):
    """mivi_optimize_loop splits these rows over 2 and 6 workgroups; a run of mivi_optimize_loop_many is ONE workgroup, so only the order of
    the row sums differs.  Over the step counts of test_logreg_small_loop (12, then 5 more) the distance between run k and the single-run
    loop stays within the bound that test states for the single-run loop against the host-driven loop: 2e-4 relative in f32, 1e-9 in f64.
    Largest distance / bound observed on an MI355X (printed by the test): f32 2.5e-3 (two workgroups, full-rank) and 6.0e-4 (six, mean-field);
    f64 4.4e-7 and 2.4e-7."""
    fam, n, p, M, variant = case
    assert _lr_groups(n, p, M) > 1
    R = _logreg_runs(dtype, fam, n, p, M, variant, 3, False)
    ctx = avi.MiviContext(dtype, R.family, p + 1, M, 0, SEED)
    ctx.set_problem(R.probs[0])
    tol = 2e-4 if dtype == np.float32 else 1e-9
    worst = 0.0
    for rule, op, avg in COMBOS_B:
        got = R.many(ctx, 17, rule, op, avg, calls=[12, 5], **_lr_target(ctx, R, False))
        assert not got[4].any()
        for k in range(R.K):
            want = R.single(k, 17, rule, op, avg, calls=[12, 5])
            for a, b in ((got[0][k], want[0]), (got[2][k] if avg else got[0][k], want[2] if avg else want[0])):
                err = np.max(np.abs(a.astype(np.float64) - b.astype(np.float64))) / max(1.0, np.max(np.abs(b)))
                worst = max(worst, err / tol)
                assert err <= tol, (rule, op, avg, k, err)
            assert np.allclose(got[3][k], want[3], rtol=tol)
    print(f"largest distance / bound: {worst:.3g}")
    R.close()
    ctx.close()


@pytest.mark.parametrize("cls", ["A", "B"])
def test_a_diverged_run_is_isolated(cls):
    """One run of five starts with a non-positive scale diagonal entry: a status bit (bit 2), not a fault.  Its word has the bit, the other
    four runs are bitwise what they are alone, with status words zero; without status_host the call returns the single run's error."""
    dtype = np.float32
    if cls == "A":
        d, M = 6, 3
        R = Runs(dtype, avi.FULLRANK, d, M, 0, 5, _diag_prob(dtype, d))
        bad_at = d + 2 * d + 2   # C[2, 2]
    else:
        R = _logreg_runs(dtype, "meanfield", 40, 5, 2, "logsigma_normal", 5, False)
        d, M = 6, 2
        bad_at = d + 2           # sigma[2]
    R.p0s[3] = R.p0s[3].copy()
    R.p0s[3][bad_at] = -0.25
    ctx = avi.MiviContext(dtype, R.family, d, M, 0, SEED)
    ctx.set_problem(R.probs[0])
    tgt = _targets(R) if cls == "A" else _lr_target(ctx, R, False)
    got = R.many(ctx, 4, DOWG, 0, 1, **tgt)
    assert got[4][3] & 2, got[4]
    assert not got[4][[0, 1, 2, 4]].any(), got[4]
    for k in (0, 1, 2, 4):
        _same([None if g is None else g[k] for g in got[:4]], R.single(k, 4, DOWG, 0, 1), k)
    p = ctx.to_device(np.stack(R.p0s)).contiguous()
    with pytest.raises(avi.MiviError) as ei:
        ctx.optimize_loop_many(p, 5, 2, 0, 0, rule=DESCENT, op=0, eta=1e-3, want_status=False, **tgt)
    assert ei.value.status in (2, 3)
    R.close()
    ctx.close()


def _refused(ctx, d, status, K=3, plen=None, **kw):
    """the call returns `status` with a message and leaves params_dev as it was"""
    plen = ctx.params_len if plen is None else plen
    p = ctx.empty(K * plen).fill_(0.5)
    before = p.cpu().numpy().copy()
    args = dict(rule=DESCENT, op=1, eta=1e-3, clip_epsilon=1e-5)
    args.update(kw)
    n_runs = args.pop("n_runs", K)
    if args["rule"] == ADAM and "opt_state" not in args:
        args["opt_state"] = ctx.empty(2 * K * plen).zero_()
    with pytest.raises(avi.MiviError) as ei:
        ctx.optimize_loop_many(p, n_runs, 2, 0, 0, **args)
    assert ei.value.status == status, (ei.value.status, str(ei.value))
    assert len(str(ei.value)) > len("libmivi status 6: "), str(ei.value)
    assert np.array_equal(p.cpu().numpy(), before)


def test_refusals_name_their_reason_and_touch_nothing():
    UNSUPPORTED, BAD_ARG = 6, 1
    f32 = np.float32
    diag = lambda d: avi.DiagNormalProblem(np.zeros(d, f32), np.ones(d, f32))   # noqa: E731
    rng = np.random.default_rng(1)
    lr = avi.LogRegProblem(rng.normal(size=(40, 5)).astype(f32), (rng.uniform(size=40) < 0.5).astype(np.uint8))

    def ctx_of(family=avi.FULLRANK, d=6, M=2, prob=None, **kw):
        c = avi.MiviContext(f32, family, d, M, 0, SEED, **kw)
        c.set_problem(diag(d) if prob is None else prob)
        return c

    c = ctx_of()
    _refused(c, 6, UNSUPPORTED, rule=4, opt_state=c.empty(5 * 3 * c.params_len))   # COCOB
    _refused(c, 6, BAD_ARG, n_runs=0)
    _refused(c, 6, BAD_ARG, means=np.zeros((3, 6), f32), stds=np.array([[1.0] * 6, [1.0, 0.0, 1, 1, 1, 1], [1.0] * 6], f32))
    _refused(c, 6, BAD_ARG, rule=ADAM, op=2)
    c.set_base_dist(avi.Laplace())
    _refused(c, 6, UNSUPPORTED)                                                      # a non-normal base
    c.close()
    for c in (ctx_of(d=64), ctx_of(family=avi.MEANFIELD)):                           # outside classes A / B
        _refused(c, c.d, UNSUPPORTED)
        c.close()
    c = ctx_of(prob=avi.TransformedProblem(diag(6), avi.StackedBijector([(0, 5, "identity"), (5, 6, "exp")])))
    _refused(c, 6, UNSUPPORTED)                                                      # a Stacked bijector
    c.close()
    c = ctx_of(m_total=4)
    _refused(c, 6, UNSUPPORTED)                                                      # a sharded context
    c.close()
    c = ctx_of(family=avi.MEANFIELD, prob=lr)
    c.set_batch_schedule(np.arange(40).reshape(4, 10))
    _refused(c, 6, UNSUPPORTED)                                                      # a batch schedule
    c.close()
    c = ctx_of()
    import torch
    src = torch.zeros(1, dtype=torch.int64, device=c.tdevice)
    c.set_index_source(src)
    _refused(c, 6, UNSUPPORTED)                                                      # an index source
    c.set_index_source(None)
    c.close()
    c = avi.MiviContext(f32, avi.LOWRANK, 6, 2, 0, SEED, rank=2)
    c.set_problem(diag(6))
    _refused(c, 6, UNSUPPORTED)                                                      # the low-rank family
    c.close()


_NO_FUSED = """
import numpy as np, advancedvi_jl_amd as avi
c = avi.MiviContext(np.float32, avi.FULLRANK, 6, 2, 0, 7)
c.set_problem(avi.DiagNormalProblem(np.zeros(6, np.float32), np.ones(6, np.float32)))
p = c.empty(3 * c.params_len).fill_(0.5)
try:
    c.optimize_loop_many(p, 3, 2, 0, 0, rule=0, op=1, eta=1e-3, clip_epsilon=1e-5)
    print("RAN")
except avi.MiviError as e:
    print("STATUS", e.status, "UNTOUCHED", bool((p == 0.5).all().item()), "MSG", "MIVI_NO_FUSED_LOOP" in str(e))
"""


def test_no_fused_loop_switch_refuses_the_entry():
    """MIVI_NO_FUSED_LOOP=1 is read once per process: a child process with the switch set."""
    env = dict(os.environ, MIVI_NO_FUSED_LOOP="1", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", _NO_FUSED], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert "STATUS 6 UNTOUCHED True MSG True" in out.stdout, (out.stdout, out.stderr[-2000:])


@pytest.mark.parametrize("cls", ["A", "B"])
def test_null_defaults_are_the_contexts_own_values(cls):
    """Every array of mivi_many_t NULL: each run takes the context's seed, loop->estimate_idx0, loop->eta and the context's target (class B:
    its X and y).  Three runs that differ in their initial parameters only, bitwise three single-run calls on that context."""
    dtype = np.float32
    if cls == "A":
        d, M = 5, 3
        R = Runs(dtype, avi.FULLRANK, d, M, 0, 3, _diag_prob(dtype, d))
    else:
        R = _logreg_runs(dtype, "fullrank", 40, 5, 2, "logsigma_normal", 3, False)
        d, M = 6, 2
    ctx = R.ctxs[0]
    import torch
    for rule, op, avg in ((ADAM, 1, 1), (DOWG, 2, 0)):
        ps = [ctx.to_device(R.p0s[k]).clone() for k in range(3)]
        sts = [_state(ctx, p, rule) for p in ps]
        want = []
        for k in range(3):
            p, st = ps[k].clone(), sts[k].clone()
            ap, e = (p.clone() if avg else None), ctx.empty(4)
            ctx.optimize_loop(p, 4, 11, 0, rule=rule, op=op, averager=avg, eta=3e-3, clip_epsilon=1e-5, opt_state=st, avg_params=ap, elbo=e)
            ctx.synchronize()
            want.append((_bytes(p), _bytes(st), _bytes(ap), _bytes(e)))
        p, st = torch.stack(ps).contiguous(), torch.stack(sts).contiguous()
        ap, e = (p.clone() if avg else None), ctx.empty(3 * 4)
        status = ctx.optimize_loop_many(p, 3, 4, 11, 0, rule=rule, op=op, averager=avg, eta=3e-3, clip_epsilon=1e-5, opt_state=st, avg_params=ap, elbo=e)
        assert not status.any()
        for k in range(3):
            _same((_bytes(p)[k], _bytes(st)[k], None if ap is None else _bytes(ap)[k], _bytes(e).reshape(3, 4)[k]), want[k], (cls, rule, k))
    R.close()


def test_more_runs_than_one_grid_holds():
    """K = 65 540 runs exceed the 65 535 workgroups of gridDim.y: the entry launches the kernel again at a run offset.  d = 1, one sample,
    two steps of Adam; the runs on both sides of the seam bitwise (their own seed, index, eta, target and initial parameters)."""
    dtype, d, M, K = np.float32, 1, 1, 65540
    check = (0, 65534, 65535, 65536, 65539)
    rng = np.random.default_rng(8)
    seeds = rng.integers(1, 2**63 - 1, size=K).astype(np.uint64)
    idx0 = rng.integers(0, 1000, size=K).astype(np.uint64)
    etas = rng.uniform(2e-3, 2e-2, size=K)
    means, stds = rng.normal(size=(K, d)).astype(dtype), rng.uniform(0.5, 2.0, size=(K, d)).astype(dtype)
    p0 = np.stack([0.3 * rng.normal(size=K), rng.uniform(0.5, 1.5, size=K)], axis=1).astype(dtype)   # [mu, C11] per run
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, M, 0, SEED)
    ctx.set_problem(avi.DiagNormalProblem(means[0], stds[0]))
    p = ctx.to_device(p0.reshape(-1)).clone()
    st, e = ctx.empty(2 * p.numel()).zero_(), ctx.empty(K * 2)
    status = ctx.optimize_loop_many(p, K, 2, idx0, 0, seeds=seeds, etas=etas, means=means, stds=stds, rule=ADAM, op=1, clip_epsilon=1e-5, opt_state=st, elbo=e)
    assert not status.any() and ctx.last_loop() == (MANY | FR_SMALL)
    got_p, got_st, got_e = _bytes(p).reshape(K, 2), _bytes(st).reshape(K, 4), _bytes(e).reshape(K, 2)
    for k in check:
        c = avi.MiviContext(dtype, avi.FULLRANK, d, M, 0, int(seeds[k]))
        c.set_problem(avi.DiagNormalProblem(means[k], stds[k]))
        pk = c.to_device(p0[k]).clone()
        sk, ek = c.empty(4).zero_(), c.empty(2)
        c.optimize_loop(pk, 2, int(idx0[k]), 0, rule=ADAM, op=1, eta=float(etas[k]), clip_epsilon=1e-5, opt_state=sk, elbo=ek)
        c.synchronize()
        _same((got_p[k], got_st[k], None, got_e[k]), (_bytes(pk), _bytes(sk), None, _bytes(ek)), k)
        c.close()
    ctx.close()


def test_per_run_arrays_must_have_their_exact_sizes():
    """The library reads K (seeds, indices, etas), K d (means, stds), K n (y) entries: an array of another size -- a multiple of K
    included -- is refused on the host, before the call."""
    f32, K, d = np.float32, 3, 6
    ctx = avi.MiviContext(f32, avi.FULLRANK, d, 2, 0, SEED)
    ctx.set_problem(avi.DiagNormalProblem(np.zeros(d, f32), np.ones(d, f32)))
    p = ctx.empty(K * ctx.params_len).fill_(0.5)
    ok = dict(rule=DESCENT, op=1, eta=1e-3, clip_epsilon=1e-5)
    for bad in (dict(seeds=np.arange(2 * K)), dict(etas=np.ones(K + 1)), dict(means=np.zeros((K, d - 3), f32), stds=np.ones((K, d - 3), f32)),
                dict(means=np.zeros((K, d), f32), stds=np.ones((2 * K, d), f32)), dict(elbo=ctx.empty(K)), dict(avg_params=ctx.empty(K), averager=1),
                dict(rule=ADAM, opt_state=ctx.empty(K * ctx.params_len)), dict(y=ctx.empty(K * 40))):
        with pytest.raises(ValueError, match="optimize_loop_many"):
            ctx.optimize_loop_many(p, K, 2, [1, 2, 3], 0, **{**ok, **bad})
    with pytest.raises(ValueError, match="idx0"):
        ctx.optimize_loop_many(p, K, 2, [1, 2], 0, **ok)
    with pytest.raises(ValueError, match="params"):
        ctx.optimize_loop_many(p[:-1], K, 2, 0, 0, **ok)
    ctx.close()
    rng = np.random.default_rng(1)
    lr = avi.LogRegProblem(rng.normal(size=(40, 5)).astype(f32), (rng.uniform(size=40) < 0.5).astype(np.uint8))
    ctx = avi.MiviContext(f32, avi.MEANFIELD, d, 2, 0, SEED)
    ctx.set_problem(lr)
    p = ctx.empty(K * ctx.params_len).fill_(0.5)
    import torch
    y = torch.zeros(K * 40, dtype=torch.uint8, device=ctx.tdevice)
    for bad in (dict(y=y[:-1]), dict(y=y.to(torch.float32)), dict(X=ctx.empty(K * 200 - 1), x_stride=200), dict(X=ctx.empty(K * 200), x_stride=100),
                dict(X=torch.zeros(200, dtype=torch.float64, device=ctx.tdevice))):
        with pytest.raises(ValueError, match="optimize_loop_many"):
            ctx.optimize_loop_many(p, K, 2, 0, 0, **{**ok, **bad})
    assert np.all(p.cpu().numpy() == 0.5)
    ctx.close()


# ---- avi.optimize_many: element k is avi.optimize for run k ---------------------------------------------------------------------------------
def _alg(M, opt, averager=None, prox=False, entropy=None):
    if prox:
        return avi.KLMinRepGradProxDescent(avi.AutoMIVI(), n_samples=M, optimizer=opt, averager=averager)
    return avi.KLMinRepGradDescent(avi.AutoMIVI(), n_samples=M, optimizer=opt, averager=averager, operator=avi.ClipScale(), entropy=entropy)


def _fr_q(rng, d, dtype):
    C = (np.diag(rng.uniform(0.5, 1.5, size=d)) + 0.1 * np.tril(rng.normal(size=(d, d)), -1)).astype(dtype)
    return avi.FullRankGaussian((0.3 * rng.normal(size=d)).astype(dtype), C)


def _equal_triples(got, want, rng_got, rng_want, what):
    (q1, info1, st1), (q2, info2, st2) = got, want
    assert np.array_equal(st1["params"].cpu().numpy(), st2["params"].cpu().numpy()), what
    assert np.array_equal(q1.location, q2.location) and np.array_equal(np.asarray(q1.scale), np.asarray(q2.scale)), what
    assert info1 == info2, what
    assert st1["iteration"] == st2["iteration"] and rng_got.counter == rng_want.counter, what


def _class_a_group(K=4, d=10, dtype=np.float32):
    rng = np.random.default_rng(9)
    probs = [avi.DiagNormalProblem(rng.normal(size=d).astype(dtype), rng.uniform(0.5, 2, size=d).astype(dtype)) for _ in range(K)]
    qs = [_fr_q(rng, d, dtype) for _ in range(K)]
    return probs, qs


def _routes(triples):
    return [OPT._ctx_of(st["obj_st"]).last_loop() for _, _, st in triples]


@pytest.mark.parametrize("chunk", [256, 4], ids=["one-chunk", "across-chunks"])
def test_optimize_many_class_a_equals_optimize(chunk, monkeypatch):
    monkeypatch.setattr(OPT, "DEVICE_LOOP_CHUNK", chunk)
    K, T = 4, 10
    probs, qs = _class_a_group(K)
    algs = [_alg(1, avi.Adam(10.0 ** -(k + 1)), avi.PolynomialAveraging()) for k in range(K)]   # a step-size sweep
    r1 = [avi.PhiloxRNG(100 + k, 5 * k) for k in range(K)]
    r2 = [r.copy() for r in r1]
    got = avi.optimize_many(r1, algs, T, probs, qs)
    assert _routes(got)[0] == (MANY | FR_SMALL)
    for k in range(K):
        want = avi.optimize(r2[k], algs[k], T, probs[k], qs[k])
        _equal_triples(got[k], want, r1[k], r2[k], k)
        assert "diverged" not in got[k][2]
    # a warm start goes through `states`
    got2 = avi.optimize_many(r1, algs, 3, probs, qs, states=[g[2] for g in got])
    for k in range(K):
        want = avi.optimize(avi.PhiloxRNG(100 + k, 5 * k), algs[k], T + 3, probs[k], qs[k])
        assert np.array_equal(got2[k][2]["params"].cpu().numpy(), want[2]["params"].cpu().numpy()), k
        assert [i["elbo"] for i in got[k][1] + got2[k][1]] == [i["elbo"] for i in want[1]], k
        assert [i["iteration"] for i in got2[k][1]] == [1, 2, 3] and r1[k].counter == 5 * k + T + 3
    # ... also written as `optimize` allows, without q_inits: the runs are described by their states and still share the launch
    assert OPT.many_plan(algs, probs, [None] * K, [g[2] for g in got2]) is not None
    ctx0 = OPT._ctx_of(got2[0][2]["obj_st"])
    ctx0.optimize_loop(got2[0][2]["params"].clone(), 1, 0, 0, rule=0, eta=1e-3)   # (the route word now names a single-run loop)
    assert ctx0.last_loop() < MANY
    got3 = avi.optimize_many(r1, algs, 2, probs, None, states=[g[2] for g in got2])
    assert _routes(got3)[0] == (MANY | FR_SMALL)
    for k in range(K):
        want = avi.optimize(avi.PhiloxRNG(100 + k, 5 * k), algs[k], T + 5, probs[k], qs[k])
        assert np.array_equal(got3[k][2]["params"].cpu().numpy(), want[2]["params"].cpu().numpy()), k


def test_optimize_many_class_b_equals_optimize():
    K, T, n, p, dtype = 3, 6, 40, 5, np.float32
    rng = np.random.default_rng(4)
    X = rng.normal(size=(n, p)).astype(dtype)
    probs = [avi.LogRegProblem(X, (rng.uniform(size=n) < 0.5).astype(np.uint8), variant="lognormal_exp_bijector") for _ in range(K)]
    q0 = avi.MeanFieldGaussian(np.zeros(p + 1, dtype), np.full(p + 1, 0.5, dtype))
    alg = _alg(2, avi.DoWG(1e-2), avi.PolynomialAveraging(), prox=True)
    r1 = [avi.PhiloxRNG(7 + k) for k in range(K)]
    r2 = [r.copy() for r in r1]
    got = avi.optimize_many(r1, alg, T, probs, q0)
    assert _routes(got)[0] == (MANY | LR_SMALL)
    for k in range(K):
        _equal_triples(got[k], avi.optimize(r2[k], alg, T, probs[k], q0), r1[k], r2[k], k)


def test_optimize_many_falls_back_to_sequential_calls():
    """Full-rank d = 64 is outside class A: K optimize calls, the same triples."""
    K, T, d, dtype = 2, 3, 64, np.float32
    probs, qs = _class_a_group(K, d)
    alg = _alg(2, avi.Adam(1e-2), avi.NoAveraging())
    assert OPT.many_plan([alg] * K, probs, qs) is None
    r1 = [avi.PhiloxRNG(3 + k) for k in range(K)]
    r2 = [r.copy() for r in r1]
    got = avi.optimize_many(r1, alg, T, probs, qs)
    assert all(r < MANY for r in _routes(got))
    for k in range(K):
        _equal_triples(got[k], avi.optimize(r2[k], alg, T, probs[k], qs[k]), r1[k], r2[k], k)


def test_optimize_many_marks_a_diverged_run_and_returns_the_others(monkeypatch):
    """Run 1 starts from a non-positive scale diagonal (its first objective is NaN), run 2 takes Descent steps of 1e30 (finite at first,
    then not): `optimize` raises for either; optimize_many returns them with state["diverged"], `info` ending at the last finite step and
    the iteration counter there, and the other runs exactly as `optimize` returns them."""
    monkeypatch.setattr(OPT, "DEVICE_LOOP_CHUNK", 4)
    K, T, d, dtype = 4, 10, 6, np.float32
    probs, qs = _class_a_group(K, d)
    C = np.asarray(qs[1].scale).copy()
    C[2, 2] = -0.5
    qs[1] = avi.FullRankGaussian(qs[1].location, C)
    algs = [_alg(2, avi.Descent(1e30 if k == 2 else 1e-2), avi.NoAveraging()) for k in range(K)]
    r1 = [avi.PhiloxRNG(50 + k) for k in range(K)]
    r2 = [r.copy() for r in r1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = avi.optimize_many(r1, algs, T, probs, qs)
        for k in (0, 3):
            _equal_triples(got[k], avi.optimize(r2[k], algs[k], T, probs[k], qs[k]), r1[k], r2[k], k)
            assert "diverged" not in got[k][2]
        for k in (1, 2):
            with pytest.raises(RuntimeError):
                avi.optimize(r2[k], algs[k], T, probs[k], qs[k])
            _, info, st = got[k]
            assert st["diverged"] is True and len(info) < T
            assert all(np.isfinite(i["elbo"]) for i in info) and [i["iteration"] for i in info] == list(range(1, len(info) + 1))
        assert got[1][1] == [] and len(got[2][1]) >= 1
