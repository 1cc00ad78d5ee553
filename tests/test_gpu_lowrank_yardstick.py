"""The low-rank Gaussian kernels (csrc/kernels_lowrank.hip, driven by csrc/api_lowrank.hip) held PER ENTRY to a float32 yardstick on parameter
classes that span decades (tests/lowrank_ref.py classes), at the smallest shapes that reach every block, pass, slice and tail the kernels
have.  tests/test_gpu_lowrank.py bounds the whole gradient's relative l2 by 2e-5, or by 8 x the error of a plain-float32 numpy Woodbury
evaluation; tests/test_lowrank_ref_host.py has what that admits (a column, a slice, a doubled factor column or V = t on the rows past 256,
all let through on the class `steep` under the Monte-Carlo entropy, where the plain-float32 evaluation is off by a sixth of the gradient).

Shapes (d, r, M) -- lowrank_ref.SHAPES; test_the_shape_list_reaches_every_mechanism asserts the right-hand column from lowrank_ref.stages:
    (257, 4, 9)     row block 1 of k_lowr_sample / k_lowr_xv holding one row; the prep workgroup's own Gram at its largest rank, a second
                    i += 64 pass; two column tiles of 8, the second holding one column
    (257, 5, 33)    k_lowr_gram with a ragged 4 x 4 tile; a second i += 256 pass of one row (k_lowr_gram, k_lowr_s, sum log D); two VJP
                    slices of 17 and 16 columns
    (65, 17, 257)   a second 64-row VJP block of one row; a second factor-column block holding one column (kk[j] clamped to r - 1, the
                    store guarded); 8 slices of 33 columns, the last of 26
    (513, 33, 40)   three row blocks; the Cholesky trailing update beyond its 16 x 16 threads; a third factor-column block of one column
    (300, 64, 300)  the maximum rank; 8 slices of 38 columns, the last of 34
    (3, 2, 5), (2, 5, 9)   (d + r) % 4 != 0 with u2 straddling a Philox block; r > d
    (1, 1, 1)       the smallest shape
Routes (no environment switch; the family has ONE route per entry, so a case asserts what its shape reaches, from `stages`, and -- the
batch -- that no graph was recorded):
    single      mivi_estimate_gradient: every shape x entropy kinds {0, 2, 3} on `default`; every class x the five kinds at (257, 5, 33) and
                (65, 17, 257); `graded` and `steep` x kinds {2, 3} at (513, 33, 40)
    targets     at (257, 5, 33) x kinds {0, 3}: the dense Gaussian (make_problem), the funnel (mu scaled by 0.3, as the funnel tests do), and
                the diagonal target behind StackedBijector([identity on the first half, exp on the second]).  There the class `graded` is
                NARROWED on the exp rows to D = 10^U(-2, -0.5), |U_ik| = D_i 10^U(-1, 0): |z| stays under about 6, so exp(z) and
                exp(z)^2 / s^2 stay finite in float32 (the reason tests/test_gpu_meanfield_yardstick.py narrows its class); the identity
                rows keep D = 10^U(-2, 2)
    f64         u = 2^-53, a float64 yardstick, the np.longdouble reference: every shape x kind 3 on `graded`; `steep` x kind 2 at
                (257, 5, 33) -- where float64 autograd through cholesky(D^2 + U U') is itself off by 1.4e-11 (the host test)
    sample      ctx.sample: Z per entry within 8 u (|D u1| + |U| |u2| + |m|) of D u1 + U u2 + m in the next wider type, both dtypes
    batch       estimate_gradient_n, the last of 5 estimates against the draws of its own index, at (257, 5, 33) and (65, 17, 257).  The
                entry is the single calls in sequence on one set of scratch buffers (api_batch.hip), and test_gpu_lowrank.py already
                holds it bitwise to single calls at (30, 3, 10); what is asked HERE is that the fifth estimate, run over buffers four
                estimates have used, is still right per entry at shapes with more than one row block and slice, and that it is the
                estimate of idx0 + 4 -- the criterion of the single case at the same shape, shared, states both
    descent     one Descent step of optimize_steps (rule 0, eta = 2^12, no ClipScale) at (257, 5, 33) on `graded`: the gradient recovered
                as (p - p') / eta in float64 with 2^-24 |p'_i| / eta added to every denominator for the one rounding of the stored
                parameter -- the only direct check of the gradient the updating loop consumes
    objective   estimate_objective at n_samples = 300 on `steep`, kinds {2, 3}, d = 257: the value only; k_lowr_xv then runs with one row
                block and no V
Left out, and why: ctx.logpdf on given points (tests/test_gpu_logpdf.py holds it to its own yardstick); the non-normal bases and sharded
contexts (both refused on this family: tests/test_gpu_lowrank.py, tests/test_gpu_basedist.py).

Criterion, every case: the draws are the device's own (ctx.sample, read back); ref = lowrank_ref.reference on them and on the stored
parameters in the next wider type, env = lowrank_ref.envelope (per entry the largest distance of eight orders of the sample columns of the
yardstick: E, Z, t, V, G and the K = r product in the context's type, everything of size r and every sum over d or M in float64), S =
lowrank_ref.magnitude.  The four numbers printed -- whole, block (64 rows of dm, of dD or of one factor column: what one VJP workgroup
owns), entry (lowrank_ref.ratios) and value -- are at most F32_FACTOR = 8 (tests/measure_space_cases.py), the results are finite and the
value within VALUE_RTOL (f64: TOL64).

Worst ratios measured on the MI355X per route (whole, block, entry, value), with the case that gave each (class d x r x M, entropy kind):
    route               cases  whole  block  entry  value   (worst cases)
    single, every shape  24    1.07   2.50   2.50   0.61    (default 1 x 1 x 1 ent 3; the same ent 0, twice; default 3 x 2 x 5 ent 0)
    single, every class  48    0.57   1.33   2.71   0.34    (far 257 x 5 x 33 ent 3, twice; the same ent 0; far 65 x 17 x 257 ent 0)
    target, dense         2    0.08   0.10   0.33   0.02    (default 257 x 5 x 33 ent 0)
    target, funnel        2    0.08   0.22   0.51   0.08    (ent 3; ent 0, three times)
    target, bijector      4    0.83   1.26   2.28   0.18    (default ent 3; graded ent 0; default ent 0; graded ent 0)
    single f64            9    0.55   0.91   2.12   1.06    (graded 257 x 4 x 9; graded 2 x 5 x 9; graded 257 x 4 x 9; graded 2 x 5 x 9)
    batch, last of 5      2    0.40   0.92   1.69   0.11    (graded 257 x 5 x 33, three times; graded 65 x 17 x 257)
    descent               2    0.35   0.70   1.19   0.07    (graded 257 x 5 x 33 ent 0; ent 3, twice; ent 0)
    objective             2    -      -      -      0.00    (steep 257 x 5 x 300: below 0.005 under both kinds)
    sample                8    -      -      4.28   -       (graded 513 x 33 x 40 f64; f32 at most 3.75, default 513 x 33 x 40)
No ratio above the factor, and only the sample's above 4: an r = 33 chain of fused multiply-adds in the element type against ONE rounding
of the sum of the magnitudes, the worst of 20520 entries.  Nothing in csrc/kernels_lowrank.hip had to change.  On `steep` under the kinds
2 .. 4 the value's ratio (and, under kind 2, the whole-gradient ratio) reads 0.00: S carries |t|^2 + |s|' |x| and Va (|u1| + D Va), forms
that cancel to 1e-4 of their terms there, so the floor is coarse and VALUE_RTOL and the block and entry ratios are what binds.
All 105 cases of the file run in 0.8 s in one process on the MI355X host (the first, which loads the library, 0.2 s; the slowest after
it, f64 at 300 x 64 x 300 with its np.longdouble reference, 0.1 s)."""
import zlib

import numpy as np
import pytest

import advancedvi_jl_amd as avi
from oracle import oracle as O
from tests import lowrank_ref as R
from tests.helpers import SEED, make_problem
from tests.measure_space_cases import F32_FACTOR, TOL64, VALUE_RTOL

pytestmark = pytest.mark.gpu

IDX = 77                 # the estimate every case is checked on (the batch: idx0 = IDX - count + 1), so cases that share a setup share a reference
BIJ_BLOCKS = lambda d: [(0, d // 2, "identity"), (d // 2, d, "exp")]
_setups, _criteria = {}, {}


def _setup(kind, d, r, dtype, target="diag"):
    """(params in the context's dtype, problem, oracle target on the stored numbers).  target: "diag" (the class's m, s), "dense", "funnel",
    "bij" (the diagonal target behind BIJ_BLOCKS)"""
    key = (kind, d, r, np.dtype(dtype).name, target)
    if key not in _setups:
        rng = np.random.default_rng(zlib.crc32(f"{kind} {target}".encode()) + 131 * d + r)
        mu, D, U, m, s = R.classes(kind, d, r, rng)
        if target == "funnel":
            mu = 0.3 * mu
        if target == "bij" and kind == "graded":
            h = d - d // 2
            D[d // 2:] = 10.0 ** rng.uniform(-2.0, -0.5, size=h)
            U[d // 2:] = rng.choice([-1.0, 1.0], size=(h, r)) * D[d // 2:, None] * 10.0 ** rng.uniform(-1.0, 0.0, size=(h, r))
        params = R.flat(mu, D, U, dtype)
        if target == "funnel":
            prob, tgt = avi.FunnelProblem(d, 1.5), O.FunnelStackedTarget(d, 1.5)
        elif target == "dense":
            prob, tgt = make_problem(rng, "dense", d, dtype)
        else:
            m, s = m.astype(dtype), s.astype(dtype)
            prob, tgt = avi.DiagNormalProblem(m, s), O.DiagNormalTarget(m, s)
            if target == "bij":
                prob, tgt = avi.TransformedProblem(prob, avi.StackedBijector(BIJ_BLOCKS(d))), O.StackedBijectorTarget(tgt, BIJ_BLOCKS(d))
        _setups[key] = (params, prob, tgt)
    return _setups[key]


def _context(kind, d, r, M, ent, dtype=np.float32, target="diag"):
    params, prob, tgt = _setup(kind, d, r, dtype, target)
    ctx = avi.MiviContext(dtype, avi.LOWRANK, d, M, ent, SEED, rank=r)
    ctx.set_problem(prob)
    assert ctx.params_len == 2 * d + d * r
    return ctx, params, tgt


def _draws(ctx, p, idx=IDX):
    return ctx.sample(p, idx)[1].cpu().numpy().copy()


def _unit(dtype):
    return R.U32 if dtype == np.float32 else R.U64


def _criterion(kind, d, r, M, ent, dtype, target, params, tgt, eps):
    """(ref, env, S) of the estimate IDX of one setup, computed once and left unchanged; a second case must have drawn the same numbers"""
    key = (kind, d, r, M, ent, np.dtype(dtype).name, target)
    if key not in _criteria:
        ref = R.reference(params, d, r, tgt, eps, ent, R.wider(dtype))
        _criteria[key] = (zlib.crc32(eps.tobytes()), ref, R.envelope(params, d, r, tgt, eps, ent, dtype, ref), R.magnitude(params, d, r, tgt, eps, ent))
    assert _criteria[key][0] == zlib.crc32(eps.tobytes()), "the draws of this estimate differ between two routes"
    return _criteria[key][1:]


def _hold(route, kind, d, r, M, ent, params, tgt, eps, value, grad, dtype=np.float32, target="diag", extra=None):
    ref, env, mag = _criterion(kind, d, r, M, ent, dtype, target, params, tgt, eps)
    u = _unit(dtype)
    vr = R.value_ratio(value, env["value"], ref["value"], mag["value"], u)
    if grad is None:   # a value-only route
        whole = block = entry = 0.0
    else:
        g = np.asarray(grad)
        assert np.all(np.isfinite(g))
        whole, block, entry = R.ratios(g, env["grad"], ref["grad"], mag["grad"], d, r, u, extra)
    print(f"[lowrank yardstick] {route} {kind} {d} {r} {M} ent{ent}: {whole:.2f}, {block:.2f}, {entry:.2f}, {vr:.2f}")
    assert np.isfinite(float(value))
    vtol = VALUE_RTOL if dtype == np.float32 else TOL64[0]
    assert abs(float(value) - float(ref["value"])) <= vtol * max(abs(float(ref["value"])), 1.0), (float(value), float(ref["value"]))
    assert max(whole, block, entry, vr) <= F32_FACTOR, (route, kind, d, r, M, ent, whole, block, entry, vr)


def run_single(route, kind, d, r, M, ent, dtype=np.float32, target="diag"):
    ctx, params, tgt = _context(kind, d, r, M, ent, dtype, target)
    p = ctx.to_device(params)
    eps = _draws(ctx, p)
    v, g = ctx.estimate_gradient(p, IDX)
    ctx.synchronize()
    v, g = float(v.item()), g.cpu().numpy().copy()
    ctx.close()
    _hold(route, kind, d, r, M, ent, params, tgt, eps, v, g, dtype, target)


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


# ---- the shape list reaches what it is meant to ------------------------------------------------------------------------------------------------
def test_the_shape_list_reaches_every_mechanism():
    st = {s: R.stages(*s) for s in R.SHAPES}
    # block 1 and up of both 256-row kernels (one of them holding ONE row), three row blocks, and a second 64-row VJP block of one row
    assert st[(257, 4, 9)]["row_blocks_256"] == 2 and st[(513, 33, 40)]["row_blocks_256"] == 3 and st[(65, 17, 257)]["row_blocks_64"] == 2
    # r = 4 and r = 5 on their two Gram routes, each past one pass of its loop over d (i += 64 lanes in the prep workgroup, i += 256 in k_lowr_gram)
    assert not st[(257, 4, 9)]["gram_kernel"] and st[(257, 4, 9)]["passes_64"] > 1
    assert st[(257, 5, 33)]["gram_kernel"] and st[(257, 5, 33)]["gram_ragged_tile"] and st[(257, 5, 33)]["row_blocks_256"] == 2
    assert max(r for _, r, _ in R.SHAPES if not R.stages(1, r, 1)["gram_kernel"]) == 4 and min(r for _, r, _ in R.SHAPES if r > 4) == 5
    # a ragged second factor-column block (16 < r < 32) and a ragged third
    assert (st[(65, 17, 257)]["factor_blocks"], st[(65, 17, 257)]["last_factor_block"]) == (2, 1)
    assert (st[(513, 33, 40)]["factor_blocks"], st[(513, 33, 40)]["last_factor_block"]) == (3, 1) and st[(513, 33, 40)]["cholesky_beyond_16"]
    # eight slices of more than 32 columns with a shorter last one; two slices; one
    assert st[(65, 17, 257)]["slice_columns"] == [33] * 7 + [26] and st[(300, 64, 300)]["slice_columns"] == [38] * 7 + [34]
    assert st[(257, 5, 33)]["slice_columns"] == [17, 16] and st[(1, 1, 1)]["slice_columns"] == [1]
    # the tails: a column tile of 8 holding one column, M % 4 and M % 8 tails, a Philox block shared by u1 and u2, r > d, the maximum rank
    assert st[(257, 4, 9)]["last_tile_8"] == 1 and st[(257, 5, 33)]["last_tile_4"] == 1 and st[(300, 64, 300)]["last_tile_8"] == 4
    assert st[(3, 2, 5)]["u2_straddles_block"] and st[(2, 5, 9)]["u2_straddles_block"] and st[(3, 2, 5)]["philox_tail"] != 0
    assert any(r > d for d, r, _ in R.SHAPES) and max(r for _, r, _ in R.SHAPES) == 64 and (1, 1, 1) in R.SHAPES


# ---- single calls ------------------------------------------------------------------------------------------------------------------------------
SINGLE = ([("default", d, r, M, ent) for d, r, M in R.SHAPES for ent in (0, 2, 3)] +
          [(k, d, r, M, ent) for k in R.CLASSES for d, r, M in [(257, 5, 33), (65, 17, 257)] for ent in range(5) if not (k == "default" and ent in (0, 2, 3))] +
          [(k, 513, 33, 40, ent) for k in ("graded", "steep") for ent in (2, 3)])


@pytest.mark.parametrize("kind,d,r,M,ent", SINGLE, ids=_ids(SINGLE))
def test_single_call(kind, d, r, M, ent):
    run_single("single", kind, d, r, M, ent)


TARGETS = [("default", t, ent) for t in ("dense", "funnel", "bij") for ent in (0, 3)] + [("graded", "bij", ent) for ent in (0, 3)]


@pytest.mark.parametrize("kind,target,ent", TARGETS, ids=_ids(TARGETS))
def test_other_targets(kind, target, ent):
    run_single(f"target-{target}", kind, 257, 5, 33, ent, target=target)


F64 = [("graded", d, r, M, 3) for d, r, M in R.SHAPES] + [("steep", 257, 5, 33, 2)]


@pytest.mark.parametrize("kind,d,r,M,ent", F64, ids=_ids(F64))
def test_float64_single_call(kind, d, r, M, ent):
    run_single("single-f64", kind, d, r, M, ent, np.float64)


# ---- routes beyond the single call -----------------------------------------------------------------------------------------------------------------
SAMPLE = [(k, d, r, M, t) for k in ("default", "graded") for d, r, M in [(257, 4, 9), (513, 33, 40)] for t in ("f32", "f64")]


@pytest.mark.parametrize("kind,d,r,M,tname", SAMPLE, ids=_ids(SAMPLE))
def test_sample_per_entry(kind, d, r, M, tname):
    dtype = np.float32 if tname == "f32" else np.float64
    assert R.stages(d, r, M)["row_blocks_256"] > 1
    ctx, params, _ = _context(kind, d, r, M, 0, dtype)
    Z, eps = ctx.sample(ctx.to_device(params), IDX)
    Z, eps = Z.cpu().numpy().copy(), eps.cpu().numpy().copy()
    ctx.close()
    wide = R.wider(dtype)
    m, D, U = R.split(params.astype(wide), d, r)
    u1, u2 = eps[:d].astype(wide), eps[d:].astype(wide)
    ref = D[:, None] * u1 + U @ u2 + m[:, None]
    S = np.abs(D[:, None] * u1) + np.abs(U) @ np.abs(u2) + np.abs(m)[:, None]
    ratio = float(np.max(np.abs(Z.astype(wide) - ref) / (wide(_unit(dtype)) * S)))
    print(f"[lowrank yardstick] sample {kind} {d} {r} {M} {tname}: entry {ratio:.2f}")
    assert np.all(np.isfinite(Z)) and ratio <= F32_FACTOR, ratio


@pytest.mark.parametrize("d,r,M", [(257, 5, 33), (65, 17, 257)], ids=["257-5-33", "65-17-257"])
def test_last_estimate_of_a_batch(d, r, M):
    kind, ent, count = "graded", 3, 5
    st = R.stages(d, r, M)
    assert st["slices"] > 1 and max(st["row_blocks_256"], st["row_blocks_64"]) > 1
    ctx, params, tgt = _context(kind, d, r, M, ent)
    p = ctx.to_device(params)
    eps = _draws(ctx, p)
    v, g = ctx.empty(1), ctx.empty(ctx.params_len)
    ctx.estimate_gradient_n(p, IDX - count + 1, count, v, g)
    ctx.synchronize()
    assert ctx.graph_recordings() == 0   # the single calls, one after the other
    vh, gh = float(v.item()), g.cpu().numpy().copy()
    ctx.close()
    _hold(f"batch[{count}]", kind, d, r, M, ent, params, tgt, eps, vh, gh)


@pytest.mark.parametrize("ent", [0, 3], ids=["ent0", "ent3"])
def test_one_descent_step_of_the_device_loop(ent):
    kind, d, r, M, eta = "graded", 257, 5, 33, 2.0 ** 12
    ctx, params, tgt = _context(kind, d, r, M, ent)
    p = ctx.to_device(params).clone()
    eps = _draws(ctx, p)
    elbo = ctx.empty(1)
    ctx.optimize_steps(p, None, IDX, 0, 1, 0, eta, 0.0, elbo)   # (clip_epsilon <= 0: no ClipScale)
    ctx.synchronize()
    after = p.cpu().numpy().astype(np.float64)
    value = -float(elbo.item())
    ctx.close()
    g = (params.astype(np.float64) - after) / eta
    _hold("descent", kind, d, r, M, ent, params, tgt, eps, value, g, extra=R.U32 * np.abs(after) / eta)


@pytest.mark.parametrize("ent", [2, 3], ids=["ent2", "ent3"])
def test_estimate_objective_value(ent):
    kind, d, r, n = "steep", 257, 5, 300
    assert R.stages(d, r, n)["row_blocks_256"] == 2   # (a gradient estimate would run k_lowr_xv over two row blocks; the value runs one, without V)
    sampler, params, tgt = _context(kind, d, r, n, ent)
    eps = _draws(sampler, sampler.to_device(params))
    sampler.close()
    ctx, _, _ = _context(kind, d, r, 33, ent)
    v = ctx.estimate_objective(ctx.to_device(params), IDX, n_samples=n)
    ctx.synchronize()
    v = float(v.item())
    ctx.close()
    _hold("objective", kind, d, r, n, ent, params, tgt, eps, v, None)
