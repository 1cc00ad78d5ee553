"""The triangular solve C^T X = R under its three public results -- the sticking-the-landing gradient (W += C^-T eps), the Stein Hessian
(C^-T mean(u g')) and the full-rank score gradient (C^-T E diag(f - fbar)) -- on every route it has, held to a float32 yardstick on
scale matrices of every conditioning (tests/solve_ref.py scale_matrix: kappa_2 from 4 to 1e6), whole and per 64-row block.

Routes (shapes select them; no environment switch is used)
    G2        k_stl_solve64<NB> + k_stl_update32 (csrc/kernels_stl.hip): f32, d in {256, 512, 1024, 2048}, right-hand sides % 32 == 0
              (NB = d / 128 = 2, 4, 8, 16).  The Stein Hessian's right-hand sides are the d columns of mean(u g').
    G1        k_stl_prep + k_stl_solve_la16 (csrc/kernels_fullrank.hip): every other shape, f32 and f64
    fallback  d > 2304 in f32: the column-block kernel
    engine    mivi_estimate_gradient_each on the batch engine: C^-T formed once per call, then two-way f16 planes (csrc/fr_planes.h)
The id of a case names the route that the rule of stl2_shape_ok (csrc/kernels_stl.hip) selects for it, restated in `route_of`; the engine
cases assert that the engine's STL product runs.

Criterion, every f32 case: ref64 = the float64 helper on the f32-stored parameters and the device's own draws (ctx.sample), yard = the same
helper in float32 (LAPACK substitution).  Both numbers of solve_ref.block_ratios -- |got - ref64| / max(|yard - ref64|, 2^-24 |ref64|) over
the whole result and the worst over the 64-row blocks of dmu, dC resp. H -- are at most F32_FACTOR = 8 (tests/test_gpu_scoregrad.py: a
different summation order and nothing more).  tests/test_solve_ref_host.py shows the factor admissible (float32 emulations of the
documented algorithms: at most 4.0) and with teeth (inverted blocks cut to 16 significant bits: 33 at the least).  Values (ELBO, average
log pi) stay on the existing relative 1e-5.  f64 (G1 only): the tolerances of tests/test_gpu_parity.py, 1e-12 and 1e-11.

Worst ratios measured on the MI355X (whole, worst block), per route:
    route     consumer                      whole   worst block   (worst case)
    G2        STL gradient, ent 3           1.39    3.37          (ar999: 2048 x 32 whole, 512 x 96 per block)
    G2        STL gradient, ent 4           0.80    1.20          (graded 256 x 64)
    G2        Stein Hessian                 0.99    1.44          (spd4 / graded, d = 2048)
    G2        score gradient                0.95    2.42          (ar999 256 x 64)
    G1        STL gradient, ent 3           1.18    1.82          (graded: 70 x 19 whole, 200 x 33 per block)
    G1        Stein Hessian                 1.51    1.52          (spd4 70 x 19)
    G1        score gradient                1.20    1.79          (ar999 200 x 19)
    fallback  Stein Hessian                 0.47    1.06          (spd2 2400 x 8)
    engine    every estimate, ent 3 and 4   1.28    4.27          (ar999 512 x 128 whole, graded 256 x 128 per block)
    G1 f64    STL gradient / Stein Hessian  7.3e-16 / 1.1e-15 relative l2 (ar999 200 x 33)
Teeth on the device, a one-off experiment on a build that is not kept: with the `lo` x `hi` product of the pre-split operand taken out of
mfma16_pre (csrc/kernels_stl.hip) every G2 and engine case but one leaves the factor (21 to 140 whole, 39 to 336 per block; the score
gradient at spd2 1024 x 32 stays at 2.4, 3.9) and every G1 / fallback case keeps its ratio, while the 287 tests of test_gpu_stein,
test_gpu_each, test_gpu_fuzz, test_gpu_parity and test_gpu_single_call_sweep still pass at their tolerances."""
import functools
import zlib

import numpy as np
import pytest

import advancedvi_jl_amd as avi
from oracle import oracle as O
from tests import scoregrad_ref as R
from tests import solve_ref as S
from tests.helpers import SEED, make_problem

pytestmark = pytest.mark.gpu

F32_FACTOR = 8.0                 # tests/test_gpu_scoregrad.py
VALUE_RTOL = 1e-5                # tests/test_gpu_parity.py, tests/test_gpu_stein.py (f32)
TOL64 = (1e-12, 1e-11)           # tests/test_gpu_parity.py TOL[np.float64]
ALL = S.KINDS


def route_of(d, n_rhs, dtype=np.float32):
    """stl2_shape_ok / launch_fr_stl restated: which solve takes n_rhs right-hand sides at dimension d"""
    if dtype == np.float32 and d in (256, 512, 1024, 2048) and n_rhs % 32 == 0:
        return "G2"
    return "fallback" if dtype == np.float32 and d > 2304 else "G1"


@functools.lru_cache(maxsize=6)
def _setup(kind, d, dtype):
    """(params in the context's dtype, oracle family, problem, oracle target): C of class `kind`, make_family's mu, make_problem's m and s"""
    rng = np.random.default_rng(zlib.crc32(kind.encode()) + d)
    C = S.scale_matrix(kind, d, rng).astype(dtype)
    mu = rng.normal(size=d).astype(dtype)
    prob, tgt = make_problem(rng, "diag", d, dtype)
    params, _ = avi.destructure(avi.FullRankGaussian(mu, C))
    assert params.dtype == dtype
    return params, O.MvLocationScale(mu.astype(np.float64), C.astype(np.float64)), prob, tgt


def _context(kind, d, M, ent, dtype=np.float32):
    params, q_o, prob, tgt = _setup(kind, d, dtype)
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, M, ent, SEED)
    ctx.set_problem(prob)
    return ctx, params, q_o, tgt


def _draws(ctx, p, idx):
    _, eps = ctx.sample(p, idx)
    return eps.cpu().numpy().copy()


def _hold(route, consumer, kind, d, M, got, yard, ref):
    whole, block = S.block_ratios(got, yard, ref, d)
    print(f"[solve yardstick] {route} {consumer} {kind} {d} {M}: {whole:.2f}, {block:.2f}")
    assert np.all(np.isfinite(got))
    assert whole <= F32_FACTOR and block <= F32_FACTOR, (route, consumer, kind, d, M, whole, block)


def _value(got, ref, floor=0.0):
    assert abs(float(got) - float(ref)) <= VALUE_RTOL * max(abs(float(ref)), floor), (float(got), float(ref))


def run_stl(kind, d, M, ent, idx=3):
    ctx, params, _, tgt = _context(kind, d, M, ent)
    p = ctx.to_device(params)
    eps = _draws(ctx, p, idx)
    v, g = ctx.estimate_gradient(p, idx)
    ctx.synchronize()
    v, g = float(v.item()), g.cpu().numpy().astype(np.float64)
    ctx.close()
    ref, yard = (S.stl_gradient(params, d, tgt, eps, ent, t) for t in (np.float64, np.float32))
    assert np.all(np.triu(g[d:].reshape(d, d, order="F"), 1) == 0.0)
    _value(v, ref["value"])
    _hold(route_of(d, M), f"ent{ent}", kind, d, M, g, yard["grad"], ref["grad"])


def run_stein(kind, d, n, idx=5):
    ctx, params, q_o, tgt = _context(kind, d, n, 0)
    p = ctx.to_device(params)
    eps = _draws(ctx, p, idx)
    lp, g, H = ctx.gauss_expected_grad_hess(p, idx)
    ctx.synchronize()
    lp, g, H = float(lp.item()), g.cpu().numpy().astype(np.float64), H.cpu().numpy().astype(np.float64)
    ctx.close()
    (lp_ref, g_ref, H_ref), (_, _, H_yard) = (S.stein_hessian(q_o, tgt, eps, t) for t in (np.float64, np.float32))
    _value(lp, lp_ref, 1.0)                                                         # tests/test_gpu_stein.py: against max(|logpi|, 1)
    assert np.linalg.norm(g - g_ref) <= 2e-5 * max(np.linalg.norm(g_ref), 1.0)     # tests/test_gpu_stein.py TOL (no solve in it)
    _hold(route_of(d, d), "stein", kind, d, n, H, H_yard, H_ref)


def run_score(kind, d, M, idx=7):
    ctx, params, _, tgt = _context(kind, d, M, 0)
    p = ctx.to_device(params)
    eps = _draws(ctx, p, idx)
    _, e, g = ctx.estimate_score_gradient(p, idx)
    ctx.synchronize()
    e, g = float(e.item()), g.cpu().numpy().astype(np.float64)
    ctx.close()
    ref, yard = (R.closed_form(params, d, avi.FULLRANK, tgt, eps, t) for t in (np.float64, np.float32))
    _value(e, ref["elbo"])
    _hold(route_of(d, M), "score", kind, d, M, g, yard["grad"], ref["grad"])


def _ids(route, consumer, cases):
    return [f"{route}-{consumer}-{k}-{d}x{M}" for k, d, M in cases]


# ---- G2: k_stl_solve64<2, 4, 8, 16> -------------------------------------------------------------------------------------------------------
G2_STL = [(k, d, M) for d, M in [(256, 32), (512, 32), (1024, 32), (2048, 32), (512, 96)] for k in ALL]
G2_ZG = [(k, 256, 64) for k in ("spd4", "graded")]
G2_STEIN = [(k, d, 32) for d in (256, 512, 1024, 2048) for k in ("spd4", "graded")]


@pytest.mark.parametrize("kind,d,M", G2_STL, ids=_ids("G2", "ent3", G2_STL))
def test_second_generation_solve_under_the_stl_gradient(kind, d, M):
    assert route_of(d, M) == "G2"
    run_stl(kind, d, M, O.ENT_STL)


@pytest.mark.parametrize("kind,d,M", G2_ZG, ids=_ids("G2", "ent4", G2_ZG))
def test_second_generation_solve_under_the_zero_gradient_stl_estimator(kind, d, M):
    assert route_of(d, M) == "G2"
    run_stl(kind, d, M, O.ENT_STL_ZERO_GRAD)


@pytest.mark.parametrize("kind,d,n", G2_STEIN, ids=_ids("G2", "stein", G2_STEIN))
def test_second_generation_solve_with_d_right_hand_sides_under_the_stein_hessian(kind, d, n):
    assert route_of(d, d) == "G2"
    run_stein(kind, d, n)


# ---- the score gradient: G2 and G1 ----------------------------------------------------------------------------------------------------------
SCORE = [(k, d, M) for d, M in [(256, 64), (1024, 32), (200, 19)] for k in ("spd2", "ar999")]


@pytest.mark.parametrize("kind,d,M", SCORE, ids=[f"{route_of(d, M)}-score-{k}-{d}x{M}" for k, d, M in SCORE])
def test_solve_under_the_score_gradient(kind, d, M):
    assert route_of(d, M) == ("G1" if d == 200 else "G2")
    run_score(kind, d, M)


# ---- G1 in f32: ragged d, or a sample count that is no multiple of 32 --------------------------------------------------------------------------
G1 = [(k, d, M) for d, M in [(70, 19), (200, 33), (320, 20), (256, 24)] for k in ("default", "spd4", "graded")]


@pytest.mark.parametrize("kind,d,M", G1, ids=_ids("G1", "ent3", G1))
def test_first_generation_solve_under_the_stl_gradient(kind, d, M):
    assert route_of(d, M) == "G1"
    run_stl(kind, d, M, O.ENT_STL)


@pytest.mark.parametrize("kind,d,n", G1, ids=[f"{route_of(d, d)}-stein-{k}-{d}x{n}" for k, d, n in G1])
def test_first_generation_shapes_under_the_stein_hessian(kind, d, n):
    """(d right-hand sides: d = 256 is the second-generation solve again, whatever n is)"""
    assert route_of(d, d) == ("G2" if d == 256 else "G1")
    run_stein(kind, d, n)


# ---- beyond the MFMA solve -------------------------------------------------------------------------------------------------------------------
def test_column_block_fallback_under_the_stein_hessian():
    assert route_of(2400, 2400) == "fallback"
    run_stein("spd2", 2400, 8)


# ---- the batch engine: C^-T planes ----------------------------------------------------------------------------------------------------------
ENGINE = [(k, d, 128, ent) for d in (256, 512) for ent in (O.ENT_STL, O.ENT_STL_ZERO_GRAD) for k in ALL]


@pytest.mark.parametrize("kind,d,M,ent", ENGINE, ids=[f"engine-ent{e}-{k}-{d}x{M}" for k, d, M, e in ENGINE])
def test_engine_planes_of_the_inverse_under_every_estimate_of_a_batch(kind, d, M, ent):
    n, idx0 = 5, 11
    ctx, params, _, tgt = _context(kind, d, M, ent)
    p = ctx.to_device(params)
    assert ctx.profile_batch(p, 2, 1)["stl_product"] > 0      # the configuration takes the engine and its STL product
    eps = {i: _draws(ctx, p, idx0 + i) for i in (0, n - 1)}
    vals, grads = ctx.estimate_gradient_each(p, idx0, n)
    ctx.synchronize()
    vals, grads = vals.cpu().numpy(), grads.cpu().numpy()
    ctx.close()
    for i in (0, n - 1):
        ref, yard = (S.stl_gradient(params, d, tgt, eps[i], ent, t) for t in (np.float64, np.float32))
        g = grads[i].astype(np.float64)
        assert np.all(np.triu(g[d:].reshape(d, d, order="F"), 1) == 0.0)
        _value(vals[i], ref["value"])
        _hold("engine", f"ent{ent}[{i}]", kind, d, M, g, yard["grad"], ref["grad"])


# ---- f64: G1 only; the risk is indexing, not splitting (kappa 2^-53 is 1e-13 at the most here) --------------------------------------------------
F64 = [(k, d, M) for d, M in [(70, 19), (200, 33)] for k in ("default", "spd2", "ar999")]


@pytest.mark.parametrize("kind,d,M", F64, ids=_ids("G1", "f64", F64))
def test_float64_solve_under_the_stl_gradient_and_the_stein_hessian(kind, d, M):
    vt, gt = TOL64
    ctx, params, q_o, tgt = _context(kind, d, M, O.ENT_STL, np.float64)
    eps = _draws(ctx, params, 3)
    v, g = ctx.estimate_gradient(params, 3)
    v, g = float(v.item()), g.cpu().numpy().copy()
    ref = S.stl_gradient(params, d, tgt, eps, O.ENT_STL)
    print(f"[solve yardstick] G1 f64 ent3 {kind} {d} {M}: {np.linalg.norm(g - ref['grad']) / max(np.linalg.norm(ref['grad']), 1.0):.2e}")
    assert abs(v - ref["value"]) <= vt * abs(ref["value"]), (v, ref["value"])
    assert np.linalg.norm(g - ref["grad"]) <= gt * max(np.linalg.norm(ref["grad"]), 1.0)
    eps = _draws(ctx, params, 5)
    lp, g, H = ctx.gauss_expected_grad_hess(params, 5)
    lp, g, H = float(lp.item()), g.cpu().numpy().copy(), H.cpu().numpy().copy()
    ctx.close()
    lp_ref, g_ref, H_ref = S.stein_hessian(q_o, tgt, eps)
    print(f"[solve yardstick] G1 f64 stein {kind} {d} {M}: {np.linalg.norm(H - H_ref) / max(np.linalg.norm(H_ref), 1.0):.2e}")
    assert abs(lp - lp_ref) <= vt * max(abs(lp_ref), 1.0)
    assert np.linalg.norm(g - g_ref) <= gt * max(np.linalg.norm(g_ref), 1.0)
    assert np.linalg.norm(H - H_ref) <= gt * max(np.linalg.norm(H_ref), 1.0)
