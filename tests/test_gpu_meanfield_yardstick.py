"""The mean-field kernels (csrc/kernels_meanfield.hip) on every route they have, held PER ENTRY to a float32 yardstick on parameter classes
that span decades (tests/meanfield_ref.py family_and_target).  A mean-field gradient entry belongs to one workgroup (rows 4b .. 4b + 3) and
nothing mixes rows, so the older tests' whole-gradient relative l2 at 2e-5 .. 4e-5 divides one workgroup's fault by the norm of all 2d
entries (tests/test_meanfield_ref_host.py has the figures: a column lost from one row, a last chunk lost from one quad, a neighbour's
sigma -- all let through on the classes `graded` and `far`).

Routes (shapes select them; no environment switch is used; every case first asserts the route it means to test, from mf_main_impl's shape
rule restated as meanfield_ref.n_cc(d, M) and, for the launch-free batches, from ctx.graph_recordings() == 0 after a batch of six or more)
    single     k_mf_main alone (n_cc == 1): M <= 256, or d >= 2045 (a thread then takes two columns and more)
    split      k_mf_main over gridDim.y column chunks + k_mf_colreduce (n_cc > 1)
    partials   estimate_partials + finalize, on one context and on three shards (m_offset = r M / 3) whose partials are added in float64
    batch      estimate_gradient_n at fixed parameters: k_mf_sgd_loop<T, -1> (diagonal target, M <= 4096; estimate lanes beyond 32 estimates),
               the last estimate's value and gradient against the draws of idx0 + count - 1; (6, 4097) must NOT take the loop
    descent    one Descent step of k_mf_sgd_loop<T, 0> (optimize_steps, rule 0, eta = 2^12, no ClipScale): the gradient recovered as
               (p - p') / eta in float64, with 2^-24 |p'_i| / eta added to every denominator for the one rounding of the stored parameter --
               the only direct check of the gradient the updating loops consume (their other tests compare after Adam, which divides the
               gradient by its own running magnitude; for M > 256 and d < 2045 the loop sums sixteen-term threads in f32 where the single
               call sums f64 chunks)
    funnel     k_mf_main<T, true> single calls and k_mf_funnel_loop batches (one-wave workgroups at M <= 64, four waves beyond)
    memory     the gradient read from memory: the dense-Gaussian target (make_problem's L and one of class spd2), and the diagonal target
               behind StackedBijector([identity on the first half, exp on the second]).  Its class `graded` is NARROWED on the exp rows to
               sigma = 10^U(-3, 0) (|z| stays under about 8, exp(z) and exp(z)^2 / s^2 finite in float32); the identity rows keep 10^U(-3, 3)
    f64        the single and split shape lists on one class each, one funnel and one batch case: u = 2^-53, a float64 yardstick, an
               np.longdouble reference
Left out, and why:
    the non-normal bases, the score estimator: other kernels (csrc/kernels_basedist.hip, kernels_score.hip) with restatements of their
        own; the criterion carries over, the expressions do not (the low-rank family has its own: tests/test_gpu_lowrank_yardstick.py)
    k_mf_gen_loop and the funnel's updating loop (k_mf_funnel_sgd_loop): tests/test_gpu_optimize.py holds both to sequences of single
        calls plus update launches -- BITWISE for Descent and Adam wherever the loop and the single call share a summation order (the
        funnel loop always: M <= 256; k_mf_gen_loop for M <= 256 or d >= 2045), and only through the update rule (the step of a
        scale-invariant rule hides a scaled gradient; DoG / DoWG to the rounding of their norms) where they do not (M > 256 with d < 2045).
        The descent route above covers k_mf_sgd_loop's column work, which k_mf_gen_loop repeats line by line.

Criterion, every case: the draws are the device's own (ctx.sample, read back); ref = meanfield_ref.gradient on them and on the stored
parameters in the next wider type, env = meanfield_ref.envelope (per entry the largest distance of eight summation orders of the
yardstick), S = meanfield_ref.magnitude.  The four numbers printed -- whole, quad, entry (meanfield_ref.ratios) and value -- are at most
F32_FACTOR = 8 (tests/measure_space_cases.py: another order of evaluation and nothing more), the results are finite and the value within
VALUE_RTOL (f64: TOL64).

Worst ratios measured on the MI355X per route (whole, quad, entry, value), with the case that gave each (class d x M, entropy kind):
    route              cases  whole  quad   entry  value   (worst cases)
    single             43     0.92   2.95   3.68   0.63    (graded 130 x 33 ent 1; graded 1024 x 256 ent 3; far 1024 x 256 ent 0; the same)
    split              16     1.08   2.27   2.83   1.40    (graded 130 x 300 ent 0; graded 1600 x 2000 ent 0; the same; graded 6 x 4096 ent 0)
    partials            2     1.03   2.03   2.99   0.15    (graded 130 x 300 ent 3; graded 130 x 33 ent 0; the same; the same)
    partials, 3 shards  1     0.19   2.02   2.35   0.23    (graded 64 x 96 ent 3)
    batch (loop)       27     1.02   2.36   2.37   1.15    (count 1: graded 130 x 300 ent 3; graded 1024 x 256 ent 3; the same; graded 6 x 4096 ent 3)
    batch (graph)       1     0.39   0.69   1.00   0.26    (default 6 x 4097 ent 0, six estimates)
    descent             8     0.57   1.05   1.12   1.15    (graded 130 x 300 ent 0, three times; graded 6 x 4096 ent 3)
    funnel             48     0.32   1.16   1.33   0.31    (wide 130 x 64 ent 0; funnel 1024 x 3 ent 0; funnel 1024 x 3 ent 3; wide 130 x 64 ent 0)
    funnel batch        8     0.30   0.67   0.73   0.30    (count 1, wide 130 x 64 ent 3)
    memory, dense L     2     0.28   0.65   1.00   0.02    (default 70 x 19)
    memory, spd2 L      2     0.09   0.17   0.31   0.01    (default 70 x 19)
    memory, bijector    4     0.91   1.44   3.30   0.56    (graded 130 x 33 ent 0)
    single f64         12     1.33   4.26   4.51   1.00    (graded 130 x 256; graded 1024 x 33; graded 2049 x 300; graded 2 x 33)
    split f64           4     0.82   2.94   4.06   2.10    (graded 40 x 513 ent 3; graded 1600 x 2000 ent 3, three times)
    funnel f64          1     0.32   0.61   0.77   0.34    (wide 130 x 64 ent 3)
    batch f64           1     0.81   2.38   2.85   0.21    (graded 130 x 300 ent 3, five estimates)
The whole file takes six seconds; the slowest case (f64, 1600 x 2000, an np.longdouble reference of 3.2 million terms) 0.6 s.
Above 4: three f64 cases on the class `graded` (entry 4.26 at 1024 x 33, 4.51 at 2049 x 300, 4.06 at 1600 x 2000).  Each is the worst of
2048 .. 4098 per-entry quotients against an envelope of only eight orders, and the device differs from the yardstick by more than the order
of the sums: it multiplies twice by the stored 1 / s where the yardstick divides twice by s -- a relative error common to all samples of a
row, which no permutation of the columns reproduces -- and forms z by one fused multiply-add.  In float64 numpy on the same classes and
shapes (the library's draws from oracle.philox_normal) a NINTH permutation of the yardstick's own sum scores 2.1 .. 2.8 per entry, and the
yardstick with (z - m) (1 / s) (1 / s) in place of the two divisions 2.6 .. 3.6; the f32 contexts, where u S_i is coarser against the same
eight orders, stay at 3.7.  No route exceeds the factor; nothing in csrc/kernels_meanfield.hip had to change."""
import zlib

import numpy as np
import pytest

import advancedvi_jl_amd as avi
from oracle import oracle as O
from tests import meanfield_ref as Mf
from tests import product_ref as Pr
from tests.helpers import SEED, make_problem
from tests.measure_space_cases import F32_FACTOR, TOL64, VALUE_RTOL

pytestmark = pytest.mark.gpu

IDX = 77                 # the estimate every case is checked on (batches: idx0 = IDX - count + 1), so cases that share a setup share a reference
BIJ_BLOCKS = lambda d: [(0, d // 2, "identity"), (d // 2, d, "exp")]
_setups, _criteria = {}, {}


def _setup(kind, d, dtype, target="diag"):
    """(params in the context's dtype, problem, oracle target on the stored numbers).  target: "diag" (family_and_target's m, s), "funnel",
    "dense" / "spd2" (the dense target's factor), "bij" (the diagonal target behind BIJ_BLOCKS)"""
    key = (kind, d, np.dtype(dtype).name, target)
    if key not in _setups:
        rng = np.random.default_rng(zlib.crc32(f"{kind} {target}".encode()) + d)
        mu, sigma, m, s = Mf.family_and_target(kind, d, rng)
        if target == "bij" and kind == "graded":
            sigma[d // 2:] = 10.0 ** rng.uniform(-3.0, 0.0, size=d - d // 2)
        params = np.concatenate([mu, sigma]).astype(dtype)
        if target == "funnel":
            prob, tgt = avi.FunnelProblem(d, 1.5), O.FunnelStackedTarget(d, 1.5)
        elif target == "dense":
            prob, tgt = make_problem(rng, "dense", d, dtype)
        elif target == "spd2":
            mm, L = rng.normal(size=d).astype(dtype), Pr.scale_matrix("spd2", d, rng).astype(dtype)
            prob, tgt = avi.DenseNormalProblem(mm, L), O.DenseNormalTarget(mm, L)
        else:
            m, s = m.astype(dtype), s.astype(dtype)
            prob, tgt = avi.DiagNormalProblem(m, s), O.DiagNormalTarget(m, s)
            if target == "bij":
                prob, tgt = avi.TransformedProblem(prob, avi.StackedBijector(BIJ_BLOCKS(d))), O.StackedBijectorTarget(tgt, BIJ_BLOCKS(d))
        _setups[key] = (params, prob, tgt)
    return _setups[key]


def _context(kind, d, M, ent, dtype=np.float32, target="diag", **shard):
    params, prob, tgt = _setup(kind, d, dtype, target)
    ctx = avi.MiviContext(dtype, avi.MEANFIELD, d, M, ent, SEED, **shard)
    ctx.set_problem(prob)
    return ctx, params, tgt


def _draws(ctx, p, idx=IDX):
    return ctx.sample(p, idx)[1].cpu().numpy().copy()


def _criterion(kind, d, M, ent, dtype, target, params, tgt, eps):
    """(ref, env, S) of the estimate IDX of one setup, computed once and left unchanged; a second case must have drawn the same numbers"""
    key = (kind, d, M, ent, np.dtype(dtype).name, target)
    if key not in _criteria:
        ref = Mf.gradient(params, d, tgt, eps, ent, Mf.wider(dtype))
        _criteria[key] = (zlib.crc32(eps.tobytes()), ref, Mf.envelope(params, d, tgt, eps, ent, dtype, ref), Mf.magnitude(params, d, tgt, eps, ent))
    assert _criteria[key][0] == zlib.crc32(eps.tobytes()), "the draws of this estimate differ between two routes"
    return _criteria[key][1:]


def _hold(route, kind, d, M, ent, params, tgt, eps, value, grad, dtype=np.float32, target="diag", extra=None):
    ref, env, mag = _criterion(kind, d, M, ent, dtype, target, params, tgt, eps)
    u = Mf.U32 if dtype == np.float32 else Mf.U64
    g = np.asarray(grad)
    whole, quad, entry = Mf.ratios(g, env["grad"], ref["grad"], mag["grad"], d, u, extra)
    vr = Mf.value_ratio(value, env["value"], ref["value"], mag["value"], u)
    print(f"[meanfield yardstick] {route} {kind} {d} {M} ent{ent}: {whole:.2f}, {quad:.2f}, {entry:.2f}, {vr:.2f}")
    assert np.all(np.isfinite(g)) and np.isfinite(float(value))
    vtol = VALUE_RTOL if dtype == np.float32 else TOL64[0]
    assert abs(float(value) - float(ref["value"])) <= vtol * max(abs(float(ref["value"])), 1.0), (float(value), float(ref["value"]))
    assert max(whole, quad, entry, vr) <= F32_FACTOR, (route, kind, d, M, ent, whole, quad, entry, vr)


def run_single(route, kind, d, M, ent=0, dtype=np.float32, target="diag"):
    split = Mf.n_cc(d, M)[0] > 1
    assert split == (route.startswith("split")), (route, Mf.n_cc(d, M))
    ctx, params, tgt = _context(kind, d, M, ent, dtype, target)
    p = ctx.to_device(params)
    eps = _draws(ctx, p)
    v, g = ctx.estimate_gradient(p, IDX)
    ctx.synchronize()
    v, g = float(v.item()), g.cpu().numpy().copy()
    ctx.close()
    _hold(route, kind, d, M, ent, params, tgt, eps, v, g, dtype, target)


def run_batch(route, kind, d, M, ent, count, dtype=np.float32, target="diag", loop=True):
    ctx, params, tgt = _context(kind, d, M, ent, dtype, target)
    p = ctx.to_device(params)
    eps = _draws(ctx, p)
    v, g = ctx.empty(1), ctx.empty(2 * d)
    ctx.estimate_gradient_n(p, IDX - count + 1, count, v, g)
    ctx.synchronize()
    vh, gh = float(v.item()), g.cpu().numpy().copy()
    if count < 6:
        ctx.estimate_gradient_n(p, 500, 6, ctx.empty(1), ctx.empty(2 * d))
        ctx.synchronize()
    assert (ctx.graph_recordings() == 0) == loop, (ctx.graph_recordings(), loop)
    ctx.close()
    _hold(f"{route}[{count}]", kind, d, M, ent, params, tgt, eps, vh, gh, dtype, target)


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


# ---- single launch ---------------------------------------------------------------------------------------------------------------------------
# d % 4 tails and one-row shapes at M = 33; M = 1, 255, 256; d4 >= 512 (two columns per thread and a 300-column tail); every class
SINGLE_SHAPES = [(d, 33) for d in (1, 2, 3, 5, 1023, 1024, 1025)] + [(130, 1), (130, 255), (130, 256), (2048, 257), (2049, 300)]
SINGLE = ([("default", d, M, ent) for d, M in SINGLE_SHAPES for ent in (0, 3)] +
          [(k, d, M, ent) for k in Mf.CLASSES for d, M in [(130, 33), (1024, 256)] for ent in (0, 3)] +
          [("graded", 130, 33, ent) for ent in (1, 2, 4)])


@pytest.mark.parametrize("kind,d,M,ent", SINGLE, ids=_ids(SINGLE))
def test_single_launch(kind, d, M, ent):
    run_single("single", kind, d, M, ent)


# ---- split columns + k_mf_colreduce ------------------------------------------------------------------------------------------------------------
# a 44-column last chunk; a ONE-column last chunk; sixteen chunks; the chunk count capped at 3 with chunks of 768
SPLIT_SHAPES = [(130, 300), (40, 513), (6, 4096), (1600, 2000)]
SPLIT = [(k, d, M, ent) for d, M in SPLIT_SHAPES for k in ("default", "graded") for ent in (0, 3)]


@pytest.mark.parametrize("kind,d,M,ent", SPLIT, ids=_ids(SPLIT))
def test_split_columns_and_colreduce(kind, d, M, ent):
    run_single("split", kind, d, M, ent)


def test_shape_rule_sends_the_split_shapes_where_the_cases_say():
    assert [Mf.n_cc(d, M) for d, M in SPLIT_SHAPES] == [(2, 256), (3, 256), (16, 256), (3, 768)]
    assert all(Mf.n_cc(d, M)[0] == 1 for d, M in SINGLE_SHAPES)


# ---- the partials route -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d,M,ent", [("graded", 130, 33, 0), ("graded", 130, 300, 3)], ids=["single", "split"])
def test_partials_then_finalize(kind, d, M, ent):
    ctx, params, tgt = _context(kind, d, M, ent)
    p = ctx.to_device(params)
    eps = _draws(ctx, p)
    v, g = ctx.finalize(p, ctx.estimate_partials(p, IDX))
    ctx.synchronize()
    v, g = float(v.item()), g.cpu().numpy().copy()
    ctx.close()
    _hold("partials", kind, d, M, ent, params, tgt, eps, v, g)


def test_partials_of_three_shards_added_in_float64():
    kind, d, M, ent = "graded", 64, 96, 3
    ctx, params, tgt = _context(kind, d, M, ent)
    eps = _draws(ctx, ctx.to_device(params))
    ctx.close()
    shards = [_context(kind, d, M // 3, ent, m_offset=r * (M // 3), m_total=M)[0] for r in range(3)]
    p = shards[0].to_device(params)
    total = np.zeros(shards[0].partials_len, dtype=np.float64)
    for sh in shards:
        part = sh.estimate_partials(p, IDX)
        sh.synchronize()
        total += part.cpu().numpy().astype(np.float64)
    v, g = shards[0].finalize(p, shards[0].to_device(total))
    shards[0].synchronize()
    v, g = float(v.item()), g.cpu().numpy().copy()
    for sh in shards:
        sh.close()
    _hold("partials-3-shards", kind, d, M, ent, params, tgt, eps, v, g)


# ---- launch-free batches at fixed parameters -----------------------------------------------------------------------------------------------------
BATCH = [(d, M, ent, count) for d, M in [(1024, 256), (130, 300), (6, 4096)] for ent in (0, 2, 3) for count in (1, 5, 40)]


@pytest.mark.parametrize("d,M,ent,count", BATCH, ids=_ids(BATCH))
def test_launch_free_batch_at_fixed_parameters(d, M, ent, count):
    run_batch("batch", "graded" if ent == 3 else "default", d, M, ent, count)


def test_one_column_past_the_loop_takes_the_graph_of_launches():
    run_batch("batch-graph", "default", 6, 4097, 0, 6, loop=False)


# ---- one Descent step of the device loop ------------------------------------------------------------------------------------------------------------
DESCENT = [(k, d, M, ent) for d, M in [(130, 300), (6, 4096)] for k in ("default", "graded") for ent in (0, 3)]


@pytest.mark.parametrize("kind,d,M,ent", DESCENT, ids=_ids(DESCENT))
def test_one_descent_step_of_the_device_loop(kind, d, M, ent):
    eta = 2.0 ** 12
    ctx, params, tgt = _context(kind, d, M, ent)
    p = ctx.to_device(params).clone()
    eps = _draws(ctx, p)
    elbo = ctx.empty(1)
    ctx.optimize_steps(p, None, IDX, 0, 1, 0, eta, 0.0, elbo)   # (clip_epsilon <= 0: no ClipScale)
    ctx.synchronize()
    assert ctx.graph_recordings() == 0
    after = p.cpu().numpy().astype(np.float64)
    value = -float(elbo.item())
    ctx.close()
    g = (params.astype(np.float64) - after) / eta
    _hold("descent", kind, d, M, ent, params, tgt, eps, value, g, extra=Mf.U32 * np.abs(after) / eta)


# ---- the fused funnel target ------------------------------------------------------------------------------------------------------------------------
FUNNEL = [(k, d, M, ent) for d in (5, 6, 130, 1024) for M in (3, 64, 200) for k in Mf.FUNNEL_CLASSES for ent in (0, 3)]
FUNNEL_BATCH = [(k, 130, M, 3 if k == "wide" else 0, count) for M in (64, 200) for k in Mf.FUNNEL_CLASSES for count in (1, 40)]


@pytest.mark.parametrize("kind,d,M,ent", FUNNEL, ids=_ids(FUNNEL))
def test_funnel_single_calls(kind, d, M, ent):
    run_single("funnel", kind, d, M, ent, target="funnel")


@pytest.mark.parametrize("kind,d,M,ent,count", FUNNEL_BATCH, ids=_ids(FUNNEL_BATCH))
def test_funnel_launch_free_batch(kind, d, M, ent, count):
    run_batch("funnel-batch", kind, d, M, ent, count, target="funnel")


# ---- the gradient from memory ------------------------------------------------------------------------------------------------------------------------
MEMORY = [("default", d, M, 0, L) for d, M in [(70, 19), (256, 64)] for L in ("dense", "spd2")] + [(k, 130, 33, ent, "bij") for k in ("default", "graded") for ent in (0, 3)]


@pytest.mark.parametrize("kind,d,M,ent,target", MEMORY, ids=_ids(MEMORY))
def test_gradient_from_memory(kind, d, M, ent, target):
    run_single(f"memory-{target}", kind, d, M, ent, target=target)


# ---- f64 ------------------------------------------------------------------------------------------------------------------------------------------
F64 = [("single", "graded", d, M, 0) for d, M in SINGLE_SHAPES] + [("split", "graded", d, M, 3) for d, M in SPLIT_SHAPES]


@pytest.mark.parametrize("route,kind,d,M,ent", F64, ids=_ids(F64))
def test_float64_single_calls(route, kind, d, M, ent):
    run_single(f"{route}-f64", kind, d, M, ent, np.float64)


def test_float64_funnel():
    run_single("funnel-f64", "wide", 130, 64, 3, np.float64, "funnel")


def test_float64_batch():
    run_batch("batch-f64", "graded", 130, 300, 3, 5, np.float64)
