"""Host checks of the low-rank family: the reference restatement (tests/lowrank_ref.py) against itself -- the Woodbury evaluation the
device kernels implement equals the literal `cholesky(Sigma)` / `logdet` path, autograd equals finite differences -- and the Python
mirror of src/families/location_scale_low_rank.jl (destructure / Restructure, mean / var / cov, the draw split).  No GPU.

Second part: the per-entry criterion the low-rank kernels are held to on the GPU (tests/test_gpu_lowrank_yardstick.py), checked on the CPU
at every shape (lowrank_ref.SHAPES) and class (lowrank_ref.CLASSES) of that file, on the library's own draws (oracle.philox_normal, SEED).
1. lowrank_ref.reference in float64 is the autograd restatement to TOL64 on `default` at every shape, under the five entropy kinds; its
   np.longdouble form agrees with it.  On `steep` under the Monte-Carlo entropy autograd -- cholesky of the d x d matrix D^2 + U U' --
   is 1.4e-11 from the longdouble Woodbury (relative l2; 7e-16 on `default`): no reference of a float64 context there.
2. The reference alone stays inside the criterion.  A second, independent evaluation of the yardstick -- a ninth permutation of the sample
   columns, divisions by D where the yardstick multiplies by 1 / D, A^-1 by np.linalg.inv for the Cholesky solves, the K = r product
   accumulated column by column -- scores at most F32_FACTOR / 2 = 4.  Measured worst (whole, block, entry, value) over the shapes and
   the five kinds:
       default 0.25 0.55 1.29 0.42    graded 0.57 0.93 1.45 1.12    steep 0.42 0.83 1.22 0.16    zero 0.78 0.81 1.00 0.53    far 1.00 1.00 1.38 1.00
   No class had to be narrowed and S needed no term beyond the table in tests/lowrank_ref.py.
3. Every fault of lowrank_ref.emulate scores above F32_FACTOR = 8 on the block or the entry ratio (where it leaves the gradient as it is,
   on the value's: VALUE_ONLY) on every class and under every entropy kind, but for the 30 of 150 (fault, class, kind) triples `exempt`
   names with their reasons.  Measured, lowest .. highest over the classes, kinds and FAULT_SHAPES that are not exempt:
       drop_column            1.9e3 .. 1.9e6        drop_slice               1.6e3 .. 9.3e6       row_block_1_keeps_t   157 .. 3.3e9
       clamped_factor_column  394 .. 7.6e6          gram_f32 (f64 context)   5.8e4 .. 4.3e9       logq_from_block_1     31 .. 3.4e6
   gram_f32 is scored on a FLOAT64 context.  On a float32 context it is no fault a float32 criterion can see, nor one that costs anything:
   worst (whole, block, entry, value) 1.03, 2.05, 8.49, 1.00 -- one entry of 1799 past the factor (graded 257 x 5 x 33, kind 0), every
   other case under 4.  None of the five classes makes A ill-conditioned (`steep` makes it large), so 1e-7 of A is 1e-7 of D^-1 U x: what
   the stored float32 t carries anyway.
4. What the old criterion of tests/test_gpu_lowrank.py (value, and the gradient's relative l2 at 2e-5 or 8 x the error of woodbury_eval in
   plain float32) LETS THROUGH (OLD_CRITERION_PASSES, asserted below), as relative l2 of the gradient against the bound it passed:
       `steep`, Monte-Carlo entropy, where the plain-float32 evaluation itself is off by 0.023 .. 0.93 of the gradient's norm (bound 0.18
       .. 7.5: at four of the five shapes an all-zero gradient would pass): the dropped column (2.1e-3 of 1.09 at 257 x 5 x 33, 2.6e-3 of
       0.18 at 65 x 17 x 257), the dropped slice (2.5e-2, 1.5e-2, and 2.2e-2 of 3.6 at 300 x 64 x 300), the doubled factor column (9.4e-3;
       9.1e-3 of 7.5 at 513 x 33 x 40), V = t on the rows past 256 (1.1e-2 of 2.4 at 257 x 4 x 9, 8.2e-2 at 257 x 5 x 33);
       `far`: V = t on the rows past 256 under the kinds 2, 3, 4 (2.4e-6 .. 1.4e-5 of 2e-5), log q lost from the columns >= 8 under the
       kinds 2, 3, 4 (the value, 1e8, hides it at 1e-5 relative; the value ratio is 31 .. 54); gram_f32 on a float64 context under kind 0
       (4.0e-12 of 1e-11).
   On `default`, `graded` and `zero` the old criterion does see each of these faults at these shapes: a whole 64-row block is a large share
   of a gradient of two to five such blocks."""
import functools

import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from oracle import oracle as O
from tests import lowrank_ref as R
from tests.helpers import SEED, make_problem
from tests.measure_space_cases import F32_FACTOR, TOL64


def make_lowrank(rng, d, r, dtype=np.float64, zero_factors=False):
    mu = rng.normal(size=d).astype(dtype)
    D = rng.uniform(0.5, 1.5, size=d).astype(dtype)
    U = (np.zeros((d, r)) if zero_factors else 0.7 * rng.normal(size=(d, r))).astype(dtype)
    return avi.LowRankGaussian(mu, D, U)


@pytest.mark.parametrize("d,r,M", [(10, 1, 1), (10, 2, 7), (30, 3, 10)])
def test_woodbury_equals_the_literal_path(d, r, M):
    rng = np.random.default_rng(d + r)
    q = make_lowrank(rng, d, r)
    params, _ = avi.destructure(q)
    eps = rng.normal(size=(d + r, M))
    p = torch.tensor(params)
    m, D, U = R.split(p, d, r)
    Z = R.rand(m, D, U, torch.tensor(eps))
    logq, V, x = R.woodbury_logq(params, d, r, eps)
    lit = np.array([float(R.logpdf(m, D, U, Z[:, k])) for k in range(M)])
    assert np.allclose(logq, lit, rtol=1e-12, atol=1e-12)
    Sigma = np.diag(q.scale_diag ** 2) + q.scale_factors @ q.scale_factors.T
    assert np.allclose(V, np.linalg.solve(Sigma, Z.numpy() - q.location[:, None]), rtol=1e-11, atol=1e-12)
    assert np.allclose(q.scale_factors.T @ V, x, rtol=1e-11, atol=1e-12)   # U' V = x: what the Monte-Carlo entropy's VJP uses
    # closed-form entropy: logdet(I + U' D^-2 U) against logdet(Sigma)
    ent = float(R.entropy(m, D, U))
    assert abs(ent - (0.5 * d * (1 + R.LOG2PI) + 0.5 * np.linalg.slogdet(Sigma)[1])) < 1e-11


@pytest.mark.parametrize("kind", range(5))
@pytest.mark.parametrize("target", ["diag", "dense", "funnel"])
def test_woodbury_estimators_equal_autograd(kind, target):
    """The five estimators as the kernels assemble them (value and the table of gradients) against autograd of the literal expressions."""
    d, r, M = 12, 3, 5
    rng = np.random.default_rng(17)
    q = make_lowrank(rng, d, r)
    params, _ = avi.destructure(q)
    _, tgt = make_problem(rng, target, d)
    eps = rng.normal(size=(d + r, M))
    ref = R.estimate_gradient(params, d, r, tgt, eps, kind)
    cols = [tgt.logdensity_and_gradient(ref["Z"][:, k].copy()) for k in range(M)]
    ell, G = np.array([c[0] for c in cols]), np.stack([c[1] for c in cols], axis=1)
    got = R.woodbury_eval(params, d, r, G, ell, eps, kind)
    assert abs(got["value"] - ref["value"]) <= 1e-12 * max(1.0, abs(ref["value"]))
    assert np.linalg.norm(got["grad"] - ref["grad"]) <= 1e-11 * max(1.0, np.linalg.norm(ref["grad"]))
    assert abs(R.estimate_objective(params, d, r, tgt, eps, kind) - ref["value"]) <= 1e-12 * max(1.0, abs(ref["value"]))


def test_autograd_equals_finite_differences():
    d, r, M = 6, 2, 3
    rng = np.random.default_rng(3)
    q = make_lowrank(rng, d, r)
    params, _ = avi.destructure(q)
    _, tgt = make_problem(rng, "dense", d)
    eps = rng.normal(size=(d + r, M))
    e = torch.tensor(eps)
    for kind in (R.CLOSED_FORM, R.MONTE_CARLO):   # (the other three stop gradients: no finite-difference counterpart of the whole value)
        ref = R.estimate_gradient(params, d, r, tgt, eps, kind)
        h, fd = 1e-6, np.zeros_like(params)
        for i in range(params.size):
            pp, pm = params.copy(), params.copy()
            pp[i] += h
            pm[i] -= h
            with torch.no_grad():
                fd[i] = (float(R.forward(torch.tensor(pp), d, r, tgt, e, kind)[0]) - float(R.forward(torch.tensor(pm), d, r, tgt, e, kind)[0])) / (2 * h)
        assert np.linalg.norm(fd - ref["grad"]) <= 1e-6 * max(1.0, np.linalg.norm(ref["grad"]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("r", [1, 2])
def test_family_mirror(r, dtype):
    """test/families/location_scale_low_rank.jl: d = 10, r in {1, 2}; lengths and round trip of destructure / Restructure."""
    d = 10
    rng = np.random.default_rng(r)
    q = make_lowrank(rng, d, r, dtype)
    assert q.family == avi.LOWRANK == 2 and q.rank == r and len(q) == d and q.eltype == np.dtype(dtype)
    flat, re = avi.destructure(q)
    assert flat.dtype == np.dtype(dtype) and flat.shape == (2 * d + d * r,)
    assert np.array_equal(flat[:d], q.location) and np.array_equal(flat[d:2 * d], q.scale_diag)
    assert np.array_equal(flat[2 * d:3 * d], q.scale_factors[:, 0])   # column-major factors
    q2 = re(flat)
    assert isinstance(q2, avi.MvLocationScaleLowRank) and q2.rank == r
    for a, b in ((q2.location, q.location), (q2.scale_diag, q.scale_diag), (q2.scale_factors, q.scale_factors)):
        assert a.dtype == np.dtype(dtype) and np.array_equal(a, b)
    with pytest.raises(ValueError):
        re(flat[:-1])
    Sigma = np.diag(q.scale_diag.astype(np.float64) ** 2) + q.scale_factors.astype(np.float64) @ q.scale_factors.astype(np.float64).T
    tol = 1e-6 if dtype == np.float32 else 1e-14
    assert np.array_equal(q.mean(), q.location)
    assert np.allclose(q.var(), np.diag(Sigma), rtol=tol) and np.allclose(q.cov(), Sigma, rtol=tol, atol=tol)
    assert q.mean().dtype == q.var().dtype == q.cov().dtype == np.dtype(dtype)


def test_family_rejects_bad_shapes():
    with pytest.raises(ValueError):
        avi.LowRankGaussian(np.zeros(4), np.ones(3), np.zeros((4, 2)))
    with pytest.raises(ValueError):
        avi.LowRankGaussian(np.zeros(4), np.ones(4), np.zeros((4, 0)))
    with pytest.raises(ValueError):
        avi.LowRankGaussian(np.zeros(4), np.ones(4), np.zeros((4, 65)))
    with pytest.raises(TypeError):
        avi.LowRankGaussian(np.zeros(4, dtype=np.int64), np.ones(4), np.zeros((4, 1)))


def test_draw_split_of_the_one_stream():
    """The draws of an estimate are ONE Philox stream of d + r rows per column: rows 0 .. d-1 are u1, rows d .. d+r-1 are u2, and a column
    is a pure function of (seed, index, global column)."""
    d, r, idx = 10, 3, 5
    E = O.philox_normal(SEED, idx, d + r, 0, 9)
    assert E.shape == (d + r, 9)
    assert np.array_equal(O.philox_normal(SEED, idx, d + r, 4, 9), E[:, 4:])          # columns regenerate alone
    assert not np.array_equal(E[:d], O.philox_normal(SEED, idx, d, 0, 9))              # (not the d-row stream: the block index runs over d + r rows)
    q = make_lowrank(np.random.default_rng(0), d, r)
    params, _ = avi.destructure(q)
    Z = R.rand(*R.split(torch.tensor(params), d, r), torch.tensor(E)).numpy()
    assert np.allclose(Z, q.scale_diag[:, None] * E[:d] + q.scale_factors @ E[d:] + q.location[:, None], rtol=1e-14)


# ======================================================================================================================================
# The per-entry criterion of tests/test_gpu_lowrank_yardstick.py, checked on the CPU (module docstring, second part)
# ======================================================================================================================================
KINDS = range(5)
OLD_TOL = {np.float32: (1e-5, 2e-5), np.float64: (1e-12, 1e-11)}   # tests/test_gpu_lowrank.py TOL
CLASS_ID = {k: i for i, k in enumerate(R.CLASSES)}


@functools.lru_cache(maxsize=None)
def _setup(kind, d, r, M, dtype=np.float32):
    """(params, the diagonal target on the stored m and s, draws) in the context's dtype: the library's own Philox stream"""
    rng = np.random.default_rng(d * 131 + 7 * r + M + 1000 * CLASS_ID[kind])
    mu, D, U, m, s = R.classes(kind, d, r, rng)
    tgt = O.DiagNormalTarget(m.astype(dtype), s.astype(dtype))
    return R.flat(mu, D, U, dtype), tgt, O.philox_normal(SEED, 3, d + r, 0, M, f64=dtype == np.float64).astype(dtype)


@functools.lru_cache(maxsize=None)
def _case(kind, d, r, M, ent, dtype=np.float32):
    params, tgt, eps = _setup(kind, d, r, M, dtype)
    ref = R.reference(params, d, r, tgt, eps, ent, R.wider(dtype))
    return params, tgt, eps, ref, R.envelope(params, d, r, tgt, eps, ent, dtype, ref), R.magnitude(params, d, r, tgt, eps, ent)


def _score(kind, d, r, M, ent, got, dtype=np.float32):
    """(whole, block, entry, value) of the new criterion"""
    params, tgt, eps, ref, env, mag = _case(kind, d, r, M, ent, dtype)
    u = R.U32 if dtype == np.float32 else R.U64
    whole, block, entry = R.ratios(got["grad"], env["grad"], ref["grad"], mag["grad"], d, r, u)
    return whole, block, entry, R.value_ratio(got["value"], env["value"], ref["value"], mag["value"], u)


def _old_criterion_passes(kind, d, r, M, ent, got, dtype=np.float32):
    """run_case of tests/test_gpu_lowrank.py on a result: value and whole-gradient l2 against the float64 autograd reference, the bounds TOL,
    or 8 x the error of woodbury_eval in numpy in the context's dtype for the Woodbury estimators.  (passes, relative l2, relative bound)"""
    ref, yard = _old_reference(kind, d, r, M, ent, dtype)
    vt, gt = OLD_TOL[dtype]
    gscale = max(np.linalg.norm(ref["grad"]), 1.0)
    v_bound, g_bound = vt * abs(ref["value"]), gt * gscale
    if ent >= 2:
        v_bound = max(v_bound, 8 * abs(yard["value"] - ref["value"]))
        g_bound = max(g_bound, 8 * np.linalg.norm(yard["grad"] - ref["grad"]))
    g_err = np.linalg.norm(got["grad"].astype(np.float64) - ref["grad"])
    return bool(abs(float(got["value"]) - ref["value"]) <= v_bound and g_err <= g_bound), g_err / gscale, g_bound / gscale


@functools.lru_cache(maxsize=None)
def _old_reference(kind, d, r, M, ent, dtype):
    params, tgt, eps = _setup(kind, d, r, M, dtype)
    e64 = eps.astype(np.float64)
    ref = R.estimate_gradient(params.astype(np.float64), d, r, tgt, e64, ent)
    cols = [tgt.logdensity_and_gradient(ref["Z"][:, k].copy()) for k in range(M)]
    ell, G = np.array([c[0] for c in cols]), np.stack([c[1] for c in cols], axis=1)
    return ref, R.woodbury_eval(params, d, r, G, ell, e64, ent, dtype)


# ---- 1. the reference is the autograd restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_equals_autograd_on_the_default_class(shape):
    d, r, M = shape
    params, tgt, eps = _setup("default", d, r, M)
    for ent in KINDS:
        auto = R.estimate_gradient(params, d, r, tgt, eps, ent)
        ref = R.reference(params, d, r, tgt, eps, ent, np.float64)
        assert abs(ref["value"] - auto["value"]) <= TOL64[0] * max(1.0, abs(auto["value"])), (ent, ref["value"], auto["value"])
        assert np.linalg.norm(ref["grad"] - auto["grad"]) <= TOL64[1] * max(1.0, np.linalg.norm(auto["grad"])), ent
    wide = R.reference(params, d, r, tgt, eps, R.STL, np.longdouble)   # the plain r x r Cholesky and solves in the type numpy's linalg refuses
    ref = R.reference(params, d, r, tgt, eps, R.STL, np.float64)
    assert wide["grad"].dtype == np.longdouble
    assert float(np.linalg.norm((wide["grad"] - ref["grad"]).astype(np.float64))) <= TOL64[1] * max(1.0, np.linalg.norm(ref["grad"]))


def test_autograd_is_no_reference_of_a_float64_context_on_the_class_steep():
    """cholesky(D^2 + U U') of the d x d covariance (lowrank_ref.logpdf) against the Woodbury reference in np.longdouble, relative l2 of the
    gradient: within 1e-13 on `default`, beyond TOL64's 1e-11 on `steep` under the Monte-Carlo entropy -- why the f64 cases of the GPU file
    take `reference(..., np.longdouble)`"""
    d, r, M = 257, 5, 33
    rel = {}
    for kind in ("default", "steep"):
        params, tgt, eps = _setup(kind, d, r, M)
        p64 = params.astype(np.float64)
        auto = R.estimate_gradient(p64, d, r, tgt, eps, R.MONTE_CARLO)
        wide = R.reference(p64, d, r, tgt, eps, R.MONTE_CARLO, np.longdouble)
        rel[kind] = float(np.linalg.norm((auto["grad"] - wide["grad"]).astype(np.float64)) / np.linalg.norm(auto["grad"]))
    print("[lowrank reference] autograd against the longdouble Woodbury, Monte-Carlo entropy:", rel)
    assert rel["default"] <= 1e-13 and rel["steep"] > TOL64[1], rel


# ---- 2. the reference alone stays inside the criterion -------------------------------------------------------------------------------------
NINTH = 1000 + R.N_PERM   # the seed after those of meanfield_ref.orders


@pytest.mark.parametrize("kind", R.CLASSES)
def test_an_independent_evaluation_stays_within_half_the_factor(kind):
    worst = np.zeros(4)
    for d, r, M in R.SHAPES:
        for ent in KINDS:
            params, tgt, eps = _setup(kind, d, r, M)
            got = R.emulate(params, d, r, tgt, eps, ent, np.float32, order=np.random.default_rng(NINTH).permutation(M), variant=True)
            score = _score(kind, d, r, M, ent, got)
            assert np.all(np.isfinite(got["grad"])) and np.isfinite(got["value"])
            assert max(score) <= F32_FACTOR / 2, (kind, d, r, M, ent, score)
            worst = np.maximum(worst, score)
    print(f"[lowrank criterion] independent evaluation, worst of {kind} (whole, block, entry, value):", np.round(worst, 2).tolist())


# ---- 3. the faults ---------------------------------------------------------------------------------------------------------------------------
FAULT_SHAPES = {"drop_column": [(257, 5, 33), (65, 17, 257)], "drop_slice": [(257, 5, 33), (65, 17, 257), (300, 64, 300)],
                "row_block_1_keeps_t": [(257, 4, 9), (257, 5, 33), (513, 33, 40)], "clamped_factor_column": [(65, 17, 257), (513, 33, 40)],
                "gram_f32": [(257, 5, 33), (65, 17, 257)], "logq_from_block_1": [(257, 5, 33), (65, 17, 257)]}
CLOSED_KINDS = (R.CLOSED_FORM, R.CLOSED_FORM_ZERO_GRAD)
VALUE_ONLY = {"logq_from_block_1": KINDS, "gram_f32": (R.CLOSED_FORM_ZERO_GRAD,)}   # the gradient reads neither log q nor, under kind 1, A


def fault_dtype(name):
    """the context a fault is scored on: float32, but float64 for gram_f32 -- the header's "f64 for either element type" is what that fault
    breaks, and on a float32 context it breaks nothing the criterion could be asked to see (test_a_float32_gram_... below)"""
    return np.float64 if name == "gram_f32" else np.float32


def exempt(name, kind, ent):
    """the (fault, class, entropy kind) triples on which a fault changes nothing, or nothing a criterion of the context's precision can see:
        row_block_1_keeps_t, logq_from_block_1 under the closed-form kinds: neither V nor log q is formed
        gram_f32 on `zero`: A = I exactly in either type
        logq_from_block_1 on `graded` under the kinds 2, 3, 4: the value there is about 1e10 (rows with |z| near 1e3 and s near 0.1), one
            float32 spacing of it is 1e3, and the mean of log q is a few hundred
        gram_f32 under kind 1 on `graded` and `far`: A enters the value's 1/2 logdet A alone, a few units at 1e-7 relative, and the value
            is 1e10 / 1e8 -- below one float64 spacing of the terms it is summed from (S of the value)"""
    if name in ("row_block_1_keeps_t", "logq_from_block_1") and ent in CLOSED_KINDS:
        return True
    if name == "gram_f32" and kind in ("graded", "far") and ent == R.CLOSED_FORM_ZERO_GRAD:
        return True
    return (name, kind) in (("gram_f32", "zero"), ("logq_from_block_1", "graded"))


def _fault(name, d, r, M):
    rng = np.random.default_rng(d + r + M)
    return (name, int(rng.integers(0, (d + 63) // 64)), int(rng.integers(0, R.lowr_vjp_slices(M)))) if name == "drop_column" else (name,)


def fault_scores(name, kind, ent, dtype=None):
    """[(d, r, M, whole, block, entry, value, the old criterion lets it through, its l2, its bound)]"""
    dtype = fault_dtype(name) if dtype is None else dtype
    out = []
    for d, r, M in FAULT_SHAPES[name]:
        params, tgt, eps = _setup(kind, d, r, M, dtype)
        got = R.emulate(params, d, r, tgt, eps, ent, dtype, _fault(name, d, r, M))
        out.append((d, r, M) + _score(kind, d, r, M, ent, got, dtype) + _old_criterion_passes(kind, d, r, M, ent, got, dtype))
    return out


@pytest.mark.parametrize("kind", R.CLASSES)
@pytest.mark.parametrize("name", R.FAULTS)
def test_every_fault_is_seen_per_entry_or_per_block(name, kind):
    """(where a fault leaves the gradient as it is -- log q is never read by it, nor is A under the entropy kind 1 -- the value's ratio is
    the one asked: VALUE_ONLY)"""
    passed_old = set()
    for ent in KINDS:
        for d, r, M, whole, block, entry, value, old, old_l2, old_bound in fault_scores(name, kind, ent):
            print(f"[lowrank fault] {name} {kind} {d} {r} {M} ent{ent}: whole {whole:.3g}, block {block:.3g}, entry {entry:.3g}, value {value:.3g}; "
                  f"old l2 {old_l2:.2e} of {old_bound:.2e}{' PASSES' if old else ''}")
            if exempt(name, kind, ent):
                continue
            if old:
                passed_old.add(ent)
            seen = value if ent in VALUE_ONLY.get(name, ()) else max(block, entry)
            assert seen > F32_FACTOR, (name, kind, d, r, M, ent, whole, block, entry, value)
    assert passed_old == set(OLD_CRITERION_PASSES.get((name, kind), ())), (name, kind, sorted(passed_old))


def test_a_float32_gram_is_inside_the_criterion_of_a_float32_context():
    """why gram_f32 is scored on a float64 context: none of the five classes makes A ill-conditioned (`steep` makes it LARGE: every
    eigenvalue near |U|^2 / D^2), so 1e-7 of A is 1e-7 of x and of D^-1 U x -- the rounding the stored float32 t carries anyway"""
    worst = np.zeros(4)
    for kind in R.CLASSES:
        for ent in KINDS:
            for sc in fault_scores("gram_f32", kind, ent, np.float32):
                worst = np.maximum(worst, sc[3:7])
    print("[lowrank fault] gram_f32 on a float32 context, worst (whole, block, entry, value):", np.round(worst, 2).tolist())
    # measured 1.03, 2.05, 8.49, 1.0: ONE entry of 1799 (graded 257 x 5 x 33, kind 0) past the factor, every other case under 4 -- against
    # 157 .. 3.9e6 for the faults that lose a term.  Not a fault a float32 criterion can be built to see.
    assert max(worst[0], worst[1], worst[3]) <= F32_FACTOR / 2 and worst[2] <= 2 * F32_FACTOR, worst


def test_the_exempt_share_stays_under_one_quarter():
    triples = [(n, k, e) for n in R.FAULTS for k in R.CLASSES for e in KINDS]
    n_exempt = sum(exempt(*t) for t in triples)
    print(f"[lowrank fault] {n_exempt} of {len(triples)} (fault, class, kind) triples are exempt")
    assert 4 * n_exempt < len(triples), (n_exempt, len(triples))


# (fault, class) -> the entropy kinds under which run_case of tests/test_gpu_lowrank.py lets the faulted float32 result through at one shape
# of FAULT_SHAPES or more
OLD_CRITERION_PASSES = {("drop_column", "steep"): (2,), ("drop_slice", "steep"): (2,), ("clamped_factor_column", "steep"): (2,),
                        ("row_block_1_keeps_t", "steep"): (2,), ("row_block_1_keeps_t", "far"): (2, 3, 4), ("logq_from_block_1", "far"): (2, 3, 4),
                        ("gram_f32", "far"): (0,)}


# ---- 4. the shape rules ------------------------------------------------------------------------------------------------------------------------
def test_stages_restate_the_launchers():
    st = {s: R.stages(*s) for s in R.SHAPES}
    assert st[(257, 4, 9)]["gram_kernel"] is False and st[(257, 5, 33)]["gram_kernel"] is True and st[(257, 5, 33)]["gram_ragged_tile"]
    assert st[(257, 4, 9)]["row_blocks_256"] == 2 and st[(513, 33, 40)]["row_blocks_256"] == 3 and st[(65, 17, 257)]["row_blocks_64"] == 2
    assert st[(257, 5, 33)]["slice_columns"] == [17, 16] and st[(65, 17, 257)]["slice_columns"] == [33] * 7 + [26]
    assert st[(300, 64, 300)]["slice_columns"] == [38] * 7 + [34] and st[(1, 1, 1)]["slice_columns"] == [1]
    assert (st[(65, 17, 257)]["factor_blocks"], st[(65, 17, 257)]["last_factor_block"]) == (2, 1)
    assert (st[(513, 33, 40)]["factor_blocks"], st[(513, 33, 40)]["last_factor_block"]) == (3, 1)
    assert (st[(257, 4, 9)]["column_tiles_8"], st[(257, 4, 9)]["last_tile_8"]) == (2, 1)
    assert st[(3, 2, 5)]["philox_tail"] == 1 and st[(3, 2, 5)]["u2_straddles_block"] and st[(2, 5, 9)]["u2_straddles_block"]
    assert [R.lowr_vjp_slices(M) for M in (1, 32, 33, 128, 224, 225, 257, 4096)] == [1, 1, 2, 4, 7, 8, 8, 8]
