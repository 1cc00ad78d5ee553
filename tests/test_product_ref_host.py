"""Host-side checks of tests/product_ref.py, the yardstick of tests/test_gpu_product_yardstick.py: the float64 gradient equals the oracle's
for the entropy kinds without a solve and both Gaussian targets, the float32 one tracks it, the class `colgraded` is what it states, and
the criterion itself -- at most FACTOR x the float32 numpy yardstick over the whole gradient, per 64-row block and per 64-column block of
dC -- is ADMISSIBLE (float32 emulations of the two documented split-operand schemes stay under FACTOR / 2 on every class) and HAS TEETH
(the same emulations with one term of one product left out, everywhere or in a single 64-row block, leave it).  No GPU.

Measured here (numpy float32 emulations; `block` = the larger of the row-block and the column-block number; whole / block):
    nothing removed, six classes x {128 x 128, 256 x 384, 256 x 128, 1024 x 256}, diagonal target
        f16 planes   0.46 .. 0.81 / 0.77 .. 3.27  (block: colgraded 1024 x 256)
        bf16x3       0.40 .. 0.79 / 0.73 .. 3.07  (block: graded 256 x 128)
      the whole-gradient relative l2 is 3e-8 .. 2e-7.  Dense target (default class, L of make_problem and of class spd2, 128 x 128 and
      256 x 256): at most 0.79 / 1.70.  The worst blocks are blocks of dmu on the graded classes: one row dominates such a block, so the
      number is the quotient of two single rounding errors, and it moves with the draws -- another seed gave 4.35 for the f16 planes at
      graded 128 x 128 (error 6 x 2^-24 of that entry, the yardstick's 1.4 x 2^-24); the seeds are the ones of the first measurement.
    f16 scheme, the cross term hi.lo left out of the product `sample` or `vjp` (256 x 384 and 1024 x 256), asserted on EVERY class
        everywhere             default 255 .. 661 / 296 .. 747   graded 322 .. 603 / 536 .. 2158   colgraded 362 .. 615 / 549 .. 1969
                               spd2 56 .. 555 / 115 .. 730       ar999 111 .. 490 / 160 .. 555     spd4 0.98 .. 12.8 / 78 .. 759
        last 64-row block only default 165 .. 260 / 296 .. 683   graded 208 .. 214 / 461 .. 1000   colgraded 132 .. 227 / 519 .. 1233
                               spd2 35 .. 163 / 62 .. 319        ar999 74 .. 150 / 147 .. 531      spd4 0.80 .. 4.25 / 38 .. 266
      on spd4 the whole ratio stays inside the factor (l2 6e-8 .. 8e-7) and only the per-block numbers show the loss; on spd2 and ar999
      the l2 is 2e-6 .. 3.4e-5, at or under the 2e-5 .. 4e-5 of the older parity tests.
        product `dense` (default class, both L, 128 x 128 and 256 x 256): everywhere 485 .. 694 / 506 .. 745, one block 317 .. 601 / 505 .. 745
    bf16x3 scheme, lo.hi -- the smallest of the six kept terms -- left out of the product `sample` or `vjp` (same shapes)
        everywhere             default 23 .. 33 / 30 .. 47       graded 27 .. 60 / 37 .. 106       colgraded 28 .. 41 / 41 .. 109
                               spd2 5.2 .. 27 / 14 .. 35         (these four asserted)
                               ar999 8.7 .. 24 / 15 .. 27        spd4 0.57 .. 0.88 / 10 .. 33      NOT asserted
        last 64-row block only default 10 .. 14 / 24 .. 47       graded 6.2 .. 14 / 21 .. 59       colgraded 6.8 .. 33 / 41 .. 109   (asserted)
                               ar999 5.1 .. 7.1 / 11 .. 25       spd2 2.5 .. 7.4 / 5.1 .. 15       spd4 0.56 .. 0.66 / 2.3 .. 14     NOT asserted
      spd2 and spd4 do not leave the factor in every one-block case, and at 128 x 128 spd4 stays at 2.6 per block with the term removed
      everywhere; ar999 left it in every case here, but with 11 against 8 at the least, and the study this criterion came from saw 3 .. 7
      on that class: too close to assert.  The l2 of all these removals is 3e-8 .. 1.8e-5: none is visible at 2e-5.
        product `dense`: everywhere 38 .. 69 / 181 .. 264, one block 21 .. 50 / 160 .. 216"""
import functools
import zlib

import numpy as np
import pytest

import advancedvi_jl_amd as avi
from oracle import oracle as O
from tests import product_ref as Pr
from tests import solve_ref as S
from tests.helpers import make_family, make_problem
from tests.measure_space_cases import F32_FACTOR as FACTOR

SHAPES = [(128, 128), (256, 384), (256, 128), (1024, 256)]
TEETH_SHAPES = [(256, 384), (1024, 256)]          # several 128-blocks in each direction
DENSE_SHAPES = [(128, 128), (256, 256)]


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b))


# ---- the float64 helper is the oracle's function -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", ["diag", "dense"])
@pytest.mark.parametrize("ent", Pr.NO_SOLVE)
def test_gradient_f64_equals_the_oracle(ent, target):
    rng = np.random.default_rng(70 + ent)
    d, M = 13, 9
    _, q = make_family(rng, d, avi.FULLRANK)
    _, tgt = make_problem(rng, target, d)
    eps = rng.normal(size=(d, M))
    params = O.destructure(q)
    ref = O.estimate_gradient(params, d, avi.FULLRANK, tgt, eps, ent)
    got = Pr.gradient(params, d, tgt, eps, ent)
    assert abs(got["value"] - ref["value"]) <= 1e-12 * abs(ref["value"])
    assert _rel(got["grad"], ref["grad"]) <= 1e-12
    assert np.all(np.triu(got["grad"][d:].reshape(d, d, order="F"), 1) == 0.0)
    with pytest.raises(ValueError):
        Pr.gradient(params, d, tgt, eps, O.ENT_STL)


def test_dense_precision_is_the_inverse_covariance():
    rng = np.random.default_rng(5)
    _, tgt = make_problem(rng, "dense", 17)
    P = Pr.dense_precision(tgt.L)
    assert _rel(P, tgt.prec) <= 1e-13 and np.array_equal(P, P.T)


@pytest.mark.parametrize("target", ["diag", "dense"])
def test_float32_gradient_tracks_the_float64_one(target):
    """the dtype argument: float32 at every step -- kappa d 2^-24 = 4 x 16 x 6e-8 = 4e-6 at the most on the well-conditioned class"""
    rng = np.random.default_rng(13)
    d, M = 16, 32
    _, q = make_family(rng, d, avi.FULLRANK, np.float32)
    _, tgt = make_problem(rng, target, d, np.float32)
    eps = rng.normal(size=(d, M)).astype(np.float32)
    p = O.destructure(q).astype(np.float32)
    for ent in Pr.NO_SOLVE:
        a, b = Pr.gradient(p, d, tgt, eps, ent, np.float32), Pr.gradient(p, d, tgt, eps, ent, np.float64)
        assert a["grad"].dtype == np.float32 and b["grad"].dtype == np.float64
        assert 0.0 < _rel(a["grad"], b["grad"]) <= 1e-5 and abs(float(a["value"]) - b["value"]) <= 1e-5 * abs(b["value"])
        for emulate in (Pr.emulate_f16_products, Pr.emulate_bf16x3_products):
            e = emulate(p, d, tgt, eps, ent)
            assert e["grad"].dtype == np.float32 and _rel(e["grad"], b["grad"]) <= 1e-5
            assert abs(float(e["value"]) - b["value"]) <= 1e-5 * abs(b["value"])


# ---- the classes ----------------------------------------------------------------------------------------------------------------------------------
def test_colgraded_class_and_the_solve_classes_unchanged():
    assert S.KINDS == ("default", "spd2", "spd4", "ar999", "graded") and Pr.KINDS == S.KINDS + ("colgraded",)
    for kind in S.KINDS:
        assert np.array_equal(Pr.scale_matrix(kind, 70, np.random.default_rng(1)), S.scale_matrix(kind, 70, np.random.default_rng(1)))
    d = 256
    C = Pr.scale_matrix("colgraded", d, np.random.default_rng(d))
    assert C.dtype == np.float64 and np.all(np.triu(C, 1) == 0.0) and np.all(np.diag(C) > 0.0)
    assert np.all(np.isfinite(C.astype(np.float32))) and np.all(np.diag(C.astype(np.float32)) > 0.0)
    col = np.max(np.abs(C), axis=0)
    assert col.max() / col.min() >= 1e4                                  # columns spanning several decades
    last = np.abs(C[-1])                                                 # ... so one ROW holds entries of very different size:
    assert np.count_nonzero(last[last > 0.0] < 2.0 ** -15 * last.max()) >= d // 16   # many lie below 2^-15 of the row's maximum


def test_the_three_split_pieces_are_exact():
    x = (np.random.default_rng(2).normal(size=1000) * 10.0 ** np.random.default_rng(3).uniform(-6, 6, size=1000)).astype(np.float32)
    p = Pr._planes_bf16x3(x)
    assert np.array_equal(p["hi"] + p["mid"] + p["lo"], x)
    for v in p.values():
        assert np.all(v.view(np.uint32) & np.uint32(0xFFFF) == 0) and np.all((v == 0.0) | (np.sign(v) == np.sign(x)))
    with pytest.raises(ValueError):
        Pr._dropped(("vjp", "lo.lo", None), "vjp", Pr.F16_TERMS)


def test_column_block_number_sees_a_lost_column_block():
    """an error confined to the 64 columns 64 .. 127 of dC spreads over every row block and vanishes there; the column number keeps it"""
    rng = np.random.default_rng(4)
    d = 200
    dC = np.tril(rng.normal(size=(d, d))) * (10.0 ** np.repeat([0.0, -3.0, 0.0, 0.0], [64, 64, 64, 8]))[None, :]
    ref = np.concatenate([rng.normal(size=d), dC.reshape(-1, order="F")])
    yard = ref * (1.0 + 2.0 ** -22 * rng.normal(size=ref.size))
    got = yard.copy()
    bad = dC.copy()
    bad[:, 64:128] *= 1.0 + 2.0 ** -14
    got[d:] = bad.reshape(-1, order="F")
    whole, rows, cols = Pr.ratios(got, yard, ref, d)
    assert whole <= 1.01 and rows <= 1.01 and cols >= 100.0
    assert Pr.ratios(yard, yard, ref, d) == (1.0, 1.0, 1.0)


# ---- the factor is admissible and has teeth ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _case(kind, d, M, target):
    """(params, oracle target, eps, float64 gradient, float32 yardstick) on float32-stored inputs"""
    rng = np.random.default_rng(d + zlib.crc32(kind.encode()) % 997)
    C = Pr.scale_matrix(kind, d, rng).astype(np.float32)
    mu = rng.normal(size=d).astype(np.float32)
    if target == "diag":
        _, tgt = make_problem(rng, "diag", d, np.float32)
    elif target == "dense":
        _, tgt = make_problem(rng, "dense", d, np.float32)
    else:
        tgt = O.DenseNormalTarget(rng.normal(size=d).astype(np.float32), Pr.scale_matrix(target, d, rng).astype(np.float32))
    params = np.concatenate([mu, C.reshape(-1, order="F")])
    eps = rng.normal(size=(d, M)).astype(np.float32)
    ref, yard = (Pr.gradient(params, d, tgt, eps, 0, t)["grad"] for t in (np.float64, np.float32))
    return params, tgt, eps, ref, yard


def _measure(kind, d, M, target, emulate, drop=None):
    params, tgt, eps, ref, yard = _case(kind, d, M, target)
    whole, rows, cols = Pr.ratios(emulate(params, d, tgt, eps, 0, drop)["grad"], yard, ref, d)
    name = "f16" if emulate is Pr.emulate_f16_products else "bf16x3"
    print(f"[product emulation] {target} {kind} {d} x {M} {name} {drop}: {whole:.2f}, {rows:.2f}, {cols:.2f}")
    return whole, max(rows, cols)


ADMISSIBLE = [(k, d, M, "diag") for k in Pr.KINDS for d, M in SHAPES] + [("default", d, M, L) for L in ("dense", "spd2") for d, M in DENSE_SHAPES]


@pytest.mark.parametrize("kind,d,M,target", ADMISSIBLE, ids=[f"{t}-{k}-{d}x{M}" for k, d, M, t in ADMISSIBLE])
def test_the_factor_is_admissible(kind, d, M, target):
    """both emulations with nothing removed stay within FACTOR / 2 of the float32 yardstick, whole, per row block and per column block"""
    for emulate in (Pr.emulate_f16_products, Pr.emulate_bf16x3_products):
        whole, block = _measure(kind, d, M, target, emulate)
        assert whole <= FACTOR / 2 and block <= FACTOR / 2, (emulate.__name__, whole, block)


@pytest.mark.parametrize("d,M", TEETH_SHAPES)
@pytest.mark.parametrize("kind", Pr.KINDS)
def test_the_factor_sees_a_lost_f16_cross_term(kind, d, M):
    """hi.lo left out of the sample product or of the VJP, everywhere or in the last 64-row block only: the per-block number leaves the
    factor on EVERY class (the whole ratio does not: spd4 stays at 1 .. 13)"""
    for product in ("sample", "vjp"):
        for block in (None, d // 64 - 1):
            _, worst = _measure(kind, d, M, "diag", Pr.emulate_f16_products, (product, "hi.lo", block))
            assert worst > FACTOR, (product, block, worst)


@pytest.mark.parametrize("d,M", TEETH_SHAPES)
@pytest.mark.parametrize("kind", Pr.KINDS)
def test_the_factor_sees_a_lost_bf16_term_where_the_class_allows(kind, d, M):
    """lo.hi, the smallest of the six kept terms, left out of one product: everywhere -- the per-block number leaves the factor on default,
    spd2, graded and colgraded; in one 64-row block -- on default, graded and colgraded.  The other classes are measured and printed, not
    asserted (the module's docstring has the figures)."""
    for product in ("sample", "vjp"):
        for block in (None, d // 64 - 1):
            _, worst = _measure(kind, d, M, "diag", Pr.emulate_bf16x3_products, (product, "lo.hi", block))
            if kind in ("default", "graded", "colgraded") or (block is None and kind == "spd2"):
                assert worst > FACTOR, (product, block, worst)


@pytest.mark.parametrize("d,M", DENSE_SHAPES)
@pytest.mark.parametrize("target", ["dense", "spd2"])
def test_the_factor_sees_a_lost_term_of_the_dense_product(target, d, M):
    for emulate, term in ((Pr.emulate_f16_products, "hi.lo"), (Pr.emulate_bf16x3_products, "lo.hi")):
        for block in (None, d // 64 - 1):
            _, worst = _measure("default", d, M, target, emulate, ("dense", term, block))
            assert worst > FACTOR, (term, block, worst)
