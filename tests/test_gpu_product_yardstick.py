"""The three products every estimate of the full-rank family runs -- Z = m + C eps, dC = tril(W eps') / M and, for the dense-Gaussian target,
W = -P (Z - m) -- on every route they have, held to a float32 yardstick on scale matrices of every class (tests/product_ref.py scale_matrix:
the five of the solve yardstick plus `colgraded`, columns spanning six decades), whole, per 64-row block and per 64-column block of dC.
The older tests of these kernels compare the whole gradient in relative l2 at 2e-5 .. 4e-5 on one class of scale matrix: about 100 times
what the kernels deliver, and blind to a lost plane, a wrong scale or a mis-indexed block (tests/test_product_ref_host.py has the figures).

Routes (shapes select them; no environment switch is used; every case first asserts the route it means to test)
    gen0      first generation (csrc/kernels_fullrank.hip and the small-shape kernels): f32 with d % 64 != 0 or M % 128 != 0, and all of f64;
              ctx.fullrank_route(M) gives generation 0
    gen1      k_fr_prod32 / k_fr_vjp32 (csrc/kernels_fullrank_lds.hip): f32, d % 64 == 0, M % 128 == 0, d M <= 1024 x 512; three-way bf16 split;
              fullrank_route gives (1, True)
    gen3      k_fr_prod64 / k_fr_vjp64: the same beyond d M = 1024 x 512; fullrank_route gives (3, True)
    engine    mivi_estimate_gradient_each on the batch engine (csrc/kernels_fullrank_batch.hip, csrc/fr_planes.h): two-way f16 planes with
              power-of-two scales, the accumulator re-based at the 128-wide block boundaries; ctx.batch_takes_engine and
              ctx.profile_batch(p, 2, 1)["product"] > 0 (["dense_product"] > 0 for the dense target); n = 5, estimates 0 and 4 checked
Left out: the lane-batched second-generation route, the forked chains and the launch-free loops are held BITWISE to the single calls by
tests/test_gpu_lane_batches.py, tests/test_gpu_batches.py and tests/test_gpu_optimize.py, so they inherit this criterion; the Stein outer
product is under the solve yardstick (tests/test_gpu_solve_yardstick.py), as are the entropy kinds 3 and 4.

Criterion, every f32 case: ref64 = product_ref.gradient in float64 on the f32-stored parameters and the device's own draws (ctx.sample),
yard = the same expression in float32 (numpy float32 matrix products).  The three numbers of product_ref.ratios -- |got - ref64| /
max(|yard - ref64|, 2^-24 |ref64|) over the whole gradient, the worst over the 64-row blocks of dmu and dC, the worst over the 64-column
blocks of dC -- are at most F32_FACTOR = 8 (tests/measure_space_cases.py: a different summation order and nothing more); the result is
finite, exactly zero above the diagonal, and the value within the existing relative 1e-5.  f64: TOL64 of tests/test_gpu_parity.py.

Worst ratios measured on the MI355X (whole, rows, cols), per route, with the case that gave each:
    route     consumer                     whole   rows    cols    (worst cases)
    gen0      diagonal target, ent 0       1.13    2.74    2.61    (graded 64 x 100; colgraded 70 x 19; default 200 x 33)
    gen0      diagonal target, ent 1, 2    1.10    1.23    2.61    (default 200 x 33)
    gen0      dense target, both L         0.95    4.05    1.28    (L spd2, colgraded 70 x 19; L of make_problem, graded 70 x 19; as whole)
    gen1      diagonal target, ent 0       0.72    4.23    1.39    (graded 64 x 128; graded 1024 x 512; graded 1024 x 512)
    gen1      diagonal target, ent 2       0.71    1.26    0.72    (default 256 x 128)
    gen1      dense target, both L         0.64    1.57    0.76    (L of make_problem, 256 x 128)
    gen3      diagonal target, ent 0       0.74    7.58    1.05    (graded 1088 x 512; graded 2048 x 384; colgraded 1088 x 512)
    gen3      dense target                 0.69    2.12    0.79    (default 1088 x 512)
    engine    diagonal target, ent 0       1.72    7.30    1.90    (graded 128 x 1024; graded 2048 x 128; colgraded 128 x 1024)
    engine    diagonal target, ent 2       0.84    2.38    0.85    (default 256 x 128)
    engine    dense target, both L         0.93    2.75    0.95    (L of make_problem: 128 x 128; 1024 x 256; 1024 x 256)
    gen0 f64  diagonal target              3.8e-16 relative l2     (default 256 x 128)
Every case takes under two seconds.  The two row numbers near the factor are blocks of dmu on the class `graded` at d = 2048 (rows 1920 ..
of gen3 2048 x 384, rows 1088 .. of the engine's estimate 4 at 2048 x 128; the worst row block of dC alone is 0.95 and 1.20 there): one row
of such a block outweighs the others by decades, so the number is the quotient of two single rounding errors, and its mean over the
samples cancels twentyfold.  Another order of that one sum is enough for the figure: in numpy, the yardstick's own W summed sequentially
instead of pairwise over the 384 samples of graded 2048 x 384, everything else unchanged, gives 4.5 .. 6.6 there (three draws); the
emulations of the split products give 1.6 .. 4.1.  That is a summation order, what the factor is for, but it leaves these two cases little
room.  The column blocks of dC stay at 2.6 and the whole gradient at 1.7 on every route.

On the CPU (tests/test_product_ref_host.py, float32 numpy emulations of the two documented schemes): with nothing removed at most 0.81
whole and 3.27 per block on every class; the f16 scheme with one cross term removed from one product 38 .. 2158 per block on every class
(whole 0.8 .. 13 on spd4: only the per-block numbers see it there), the bf16x3 scheme with lo.hi removed 14 .. 109 per block on default,
spd2, graded and colgraded -- everywhere or, on default, graded and colgraded, in a single 64-row block (21 .. 109).  The whole-gradient
l2 of every bf16x3 removal (3e-8 .. 1.8e-5) and of the f16 removals on spd2, spd4 and ar999 (6e-8 .. 3.4e-5) is at or under what the
older tests allow."""
import functools
import zlib

import numpy as np
import pytest

import advancedvi_jl_amd as avi
from oracle import oracle as O
from tests import product_ref as Pr
from tests.helpers import SEED, make_problem
from tests.measure_space_cases import F32_FACTOR, TOL64, VALUE_RTOL

pytestmark = pytest.mark.gpu

ALL = Pr.KINDS
L_CLASSES = ("dense", "spd2")     # the dense target's factor: make_problem's (identity + small lower part) and one of class spd2 (kappa_2(P) = 1e4)


@functools.lru_cache(maxsize=4)
def _setup(kind, d, dtype, target):
    """(params in the context's dtype, problem, oracle target): C of class `kind`, a normal mu; target "diag": make_problem's m and s,
    "dense": make_problem's m and L, "spd2": a normal m and L = scale_matrix("spd2")"""
    rng = np.random.default_rng(zlib.crc32(f"{kind} {target}".encode()) + d)
    C = Pr.scale_matrix(kind, d, rng).astype(dtype)
    mu = rng.normal(size=d).astype(dtype)
    if target in ("diag", "dense"):
        prob, tgt = make_problem(rng, target, d, dtype)
    else:
        m, L = rng.normal(size=d).astype(dtype), Pr.scale_matrix(target, d, rng).astype(dtype)
        prob, tgt = avi.DenseNormalProblem(m, L), O.DenseNormalTarget(m, L)
    params, _ = avi.destructure(avi.FullRankGaussian(mu, C))
    assert params.dtype == dtype
    return params, prob, tgt


def _context(kind, d, M, ent, target, dtype=np.float32):
    params, prob, tgt = _setup(kind, d, dtype, target)
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, M, ent, SEED)
    ctx.set_problem(prob)
    return ctx, params, tgt


def _draws(ctx, p, idx):
    _, eps = ctx.sample(p, idx)
    return eps.cpu().numpy().copy()


def _hold(route, consumer, kind, d, M, params, tgt, eps, ent, value, grad):
    ref, yard = (Pr.gradient(params, d, tgt, eps, ent, t) for t in (np.float64, np.float32))
    g = np.asarray(grad).astype(np.float64)
    whole, rows, cols = Pr.ratios(g, yard["grad"], ref["grad"], d)
    print(f"[product yardstick] {route} {consumer} {kind} {d} {M}: {whole:.2f}, {rows:.2f}, {cols:.2f}")
    assert np.all(np.isfinite(g)) and np.isfinite(float(value))
    assert np.all(np.triu(g[d:].reshape(d, d, order="F"), 1) == 0.0)
    assert abs(float(value) - float(ref["value"])) <= VALUE_RTOL * abs(float(ref["value"])), (float(value), float(ref["value"]))
    assert whole <= F32_FACTOR and rows <= F32_FACTOR and cols <= F32_FACTOR, (route, consumer, kind, d, M, whole, rows, cols)


def run_single(generation, kind, d, M, ent=0, target="diag", idx=3):
    ctx, params, tgt = _context(kind, d, M, ent, target)
    assert ctx.fullrank_route(M) == (generation, generation != 0), (ctx.fullrank_route(M), generation)
    p = ctx.to_device(params)
    eps = _draws(ctx, p, idx)
    v, g = ctx.estimate_gradient(p, idx)
    ctx.synchronize()
    v, g = float(v.item()), g.cpu().numpy()
    ctx.close()
    _hold(f"gen{generation}", f"{target}-ent{ent}", kind, d, M, params, tgt, eps, ent, v, g)


def run_engine(kind, d, M, ent=0, target="diag", n=5, idx0=11):
    ctx, params, tgt = _context(kind, d, M, ent, target)
    p = ctx.to_device(params)
    assert ctx.batch_takes_engine(p)
    us = ctx.profile_batch(p, 2, 1)
    assert us["product"] > 0 and (us["dense_product"] > 0) == (target != "diag") and us["stl_product"] == 0, us
    eps = {i: _draws(ctx, p, idx0 + i) for i in (0, n - 1)}
    vals, grads = ctx.estimate_gradient_each(p, idx0, n)
    ctx.synchronize()
    vals, grads = vals.cpu().numpy(), grads.cpu().numpy()
    ctx.close()
    for i in (0, n - 1):
        _hold("engine", f"{target}-ent{ent}[{i}]", kind, d, M, params, tgt, eps[i], ent, vals[i], grads[i])


def _ids(route, cases):
    return [f"{route}-{k}-{d}x{M}" for k, d, M in cases]


# ---- first generation, f32: ragged d, or a sample count that is no multiple of 128 ------------------------------------------------------------
GEN0_KINDS = ("default", "graded", "colgraded", "ar999")
GEN0 = [(k, d, M) for d, M in [(70, 19), (200, 33), (320, 20), (64, 100)] for k in GEN0_KINDS]
GEN0_DENSE = [(k, d, M, L) for d, M in [(70, 19), (200, 33)] for L in L_CLASSES for k in GEN0_KINDS]


@pytest.mark.parametrize("kind,d,M", GEN0, ids=_ids("gen0", GEN0))
def test_first_generation_products(kind, d, M):
    run_single(0, kind, d, M)


@pytest.mark.parametrize("ent", [O.ENT_CLOSED_FORM_ZERO_GRAD, O.ENT_MONTE_CARLO])
def test_first_generation_products_under_the_other_entropy_kinds(ent):
    run_single(0, "default", 200, 33, ent)


@pytest.mark.parametrize("kind,d,M,L", GEN0_DENSE, ids=[f"gen0-{L}-{k}-{d}x{M}" for k, d, M, L in GEN0_DENSE])
def test_first_generation_products_with_the_dense_target(kind, d, M, L):
    run_single(0, kind, d, M, target=L)


# ---- second generation, 32 x 32 tiles: d M <= 1024 x 512 ----------------------------------------------------------------------------------------
GEN1 = [(k, 256, 128) for k in ALL] + [(k, d, M) for d, M in [(64, 128), (512, 384), (1024, 512)] for k in ("graded", "ar999")]


@pytest.mark.parametrize("kind,d,M", GEN1, ids=_ids("gen1", GEN1))
def test_second_generation_prod32_and_vjp32(kind, d, M):
    run_single(1, kind, d, M)


def test_second_generation_prod32_under_the_monte_carlo_entropy():
    run_single(1, "default", 256, 128, O.ENT_MONTE_CARLO)


@pytest.mark.parametrize("L", L_CLASSES)
def test_second_generation_prod32_with_the_dense_target(L):
    run_single(1, "default", 256, 128, target=L)


# ---- second generation, 64 x 64 tiles: beyond d M = 1024 x 512 ------------------------------------------------------------------------------------
GEN3 = [(k, d, M) for d, M in [(1088, 512), (2048, 384)] for k in ("default", "graded", "colgraded")]


@pytest.mark.parametrize("kind,d,M", GEN3, ids=_ids("gen3", GEN3))
def test_second_generation_prod64_and_vjp64(kind, d, M):
    run_single(3, kind, d, M)


def test_second_generation_prod64_with_the_dense_target():
    run_single(3, "default", 1088, 512, target="dense")


# ---- the batch engine ----------------------------------------------------------------------------------------------------------------------------
# 160 x 160: padded geometry; 1024 x 256: the north star; 128 x 1024: eight re-basing boundaries in the VJP; 2048 x 128: the longest product chain
ENGINE = [(k, 256, 128) for k in ALL] + [(k, d, M) for d, M in [(128, 128), (160, 160), (1024, 256), (128, 1024), (2048, 128)]
                                         for k in ("graded", "colgraded")]
ENGINE_DENSE = [("default", 128, 128, "dense"), ("default", 128, 128, "spd2"), ("default", 256, 256, "dense"), ("default", 1024, 256, "dense")]


@pytest.mark.parametrize("kind,d,M", ENGINE, ids=_ids("engine", ENGINE))
def test_engine_products_under_every_estimate_of_a_batch(kind, d, M):
    run_engine(kind, d, M)


def test_engine_products_under_the_monte_carlo_entropy():
    run_engine("default", 256, 128, O.ENT_MONTE_CARLO)


@pytest.mark.parametrize("kind,d,M,L", ENGINE_DENSE, ids=[f"engine-{L}-{k}-{d}x{M}" for k, d, M, L in ENGINE_DENSE])
def test_engine_products_with_the_dense_target(kind, d, M, L):
    run_engine(kind, d, M, target=L)


# ---- f64: first generation only; the risk is indexing, not splitting ---------------------------------------------------------------------------------
F64 = [(k, d, M) for d, M in [(70, 19), (200, 33), (256, 128)] for k in ("default", "graded", "colgraded")]


@pytest.mark.parametrize("kind,d,M", F64, ids=_ids("gen0-f64", F64))
def test_float64_products(kind, d, M):
    vt, gt = TOL64
    ctx, params, tgt = _context(kind, d, M, 0, "diag", np.float64)
    assert ctx.fullrank_route(M)[0] == 0
    eps = _draws(ctx, params, 3)
    v, g = ctx.estimate_gradient(params, 3)
    v, g = float(v.item()), g.cpu().numpy().copy()
    ctx.close()
    ref = Pr.gradient(params, d, tgt, eps, 0)
    print(f"[product yardstick] gen0 f64 {kind} {d} {M}: {np.linalg.norm(g - ref['grad']) / max(np.linalg.norm(ref['grad']), 1.0):.2e}")
    assert np.all(np.isfinite(g)) and np.all(np.triu(g[d:].reshape(d, d, order="F"), 1) == 0.0)
    assert abs(v - ref["value"]) <= vt * abs(ref["value"]), (v, ref["value"])
    assert np.linalg.norm(g - ref["grad"]) <= gt * max(np.linalg.norm(ref["grad"]), 1.0)
