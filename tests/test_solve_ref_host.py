"""Host-side checks of tests/solve_ref.py, the yardstick of tests/test_gpu_solve_yardstick.py: the float64 helpers equal the oracle, the
float32 ones track them, the classes of scale matrices have the condition numbers they state, and the criterion itself -- at most
FACTOR x the float32 LAPACK yardstick, whole and per 64-row block -- is ADMISSIBLE (float32 emulations of the documented block-inverse
and f16-plane algorithms stay under it on every class) and HAS TEETH (the same emulation with its inverted blocks cut to 16 significant
bits, what losing the `lo` plane of a three-way bf16 split does, exceeds it on every class).  No GPU."""
import functools

import numpy as np
import pytest

import advancedvi_jl_amd as avi
from oracle import oracle as O
from tests import solve_ref as S
from tests.helpers import make_family, make_problem

FACTOR = 8.0      # tests/test_gpu_scoregrad.py F32_FACTOR: a different summation order and nothing more
SEEDS = (0, 1, 2)


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b))


# ---- the float64 helpers are the oracle's functions -------------------------------------------------------------------------------------
@pytest.mark.parametrize("ent", [0, 1, 2, 3, 4])
def test_stl_gradient_f64_equals_the_oracle(ent):
    rng = np.random.default_rng(40 + ent)
    d, M = 13, 9
    _, q = make_family(rng, d, avi.FULLRANK)
    _, tgt = make_problem(rng, "diag", d)
    eps = rng.normal(size=(d, M))
    params = O.destructure(q)
    ref = O.estimate_gradient(params, d, avi.FULLRANK, tgt, eps, ent)
    got = S.stl_gradient(params, d, tgt, eps, ent)
    assert abs(got["value"] - ref["value"]) <= 1e-13 * abs(ref["value"])
    assert _rel(got["grad"], ref["grad"]) <= 1e-13
    assert np.all(np.triu(got["grad"][d:].reshape(d, d, order="F"), 1) == 0.0)
    assert _rel(got["X"], O.c_inv_t_eps(q, eps)) <= 1e-13


@pytest.mark.parametrize("kind", ["diag", "dense"])
def test_stein_hessian_f64_equals_the_oracle(kind):
    rng = np.random.default_rng(50)
    d, n = 11, 7
    _, q = make_family(rng, d, avi.FULLRANK)
    _, tgt = make_problem(rng, kind, d)
    u = rng.normal(size=(d, n))
    lp_ref, g_ref, H_ref = O.gaussian_expectation_gradient_and_hessian(q, tgt, u)
    lp, g, H = S.stein_hessian(q, tgt, u)
    assert abs(lp - lp_ref) <= 1e-13 * abs(lp_ref) and _rel(g, g_ref) <= 1e-13 and _rel(H, H_ref) <= 1e-13


@pytest.mark.parametrize("variant", ["logsigma_normal", "lognormal_exp_bijector"])
@pytest.mark.parametrize("n,p", [(1, 4), (65, 6)])
def test_logreg_hessian_order2_f64_equals_the_oracle(n, p, variant):
    rng = np.random.default_rng(60 + n)
    d, M = p + 1, 5
    _, q = make_family(rng, d, avi.FULLRANK, mu_scale=0.2)
    X = rng.normal(size=(n, p)) / np.sqrt(p)
    y = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    eps = rng.normal(size=(d, M))
    _, _, H_ref = O.gaussian_expectation_gradient_and_hessian_order2(q, O.LogRegTarget(X, y, variant, 1.7), eps)
    H = S.logreg_hessian_order2(O.destructure(q), d, X, y, variant, 1.7, eps)
    assert _rel(H, H_ref) <= 1e-13
    assert np.array_equal(H[p, :p], H[:p, p])


def test_float32_helpers_track_the_float64_ones():
    """the dtype argument: on the well-conditioned class the float32 results are the float64 ones to float32 rounding of d-term sums,
    kappa d 2^-24 = 4 x 16 x 6e-8 = 4e-6 at the most"""
    rng = np.random.default_rng(12)
    d, M = 16, 32
    _, q = make_family(rng, d, avi.FULLRANK, np.float32)
    _, tgt = make_problem(rng, "diag", d, np.float32)
    eps = rng.normal(size=(d, M)).astype(np.float32)
    p = O.destructure(q).astype(np.float32)
    for ent in (3, 4):
        a, b = S.stl_gradient(p, d, tgt, eps, ent, np.float32), S.stl_gradient(p, d, tgt, eps, ent, np.float64)
        assert a["grad"].dtype == np.float32 and a["X"].dtype == np.float32 and b["grad"].dtype == np.float64
        assert 0.0 < _rel(a["grad"], b["grad"]) <= 1e-5 and abs(float(a["value"]) - b["value"]) <= 1e-5 * abs(b["value"])
    (la, ga, Ha), (lb, gb, Hb) = S.stein_hessian(q, tgt, eps, np.float32), S.stein_hessian(q, tgt, eps, np.float64)
    assert Ha.dtype == np.float32 and 0.0 < _rel(Ha, Hb) <= 1e-5 and _rel(ga, gb) <= 1e-5 and abs(float(la) - lb) <= 1e-5 * abs(lb)
    X = (rng.normal(size=(70, d - 1)) / np.sqrt(d - 1)).astype(np.float32)
    for variant in ("logsigma_normal", "lognormal_exp_bijector"):
        Ha, Hb = (S.logreg_hessian_order2(p, d, X, None, variant, 1.7, eps, t) for t in (np.float32, np.float64))
        assert Ha.dtype == np.float32 and 0.0 < _rel(Ha, Hb) <= 1e-5


# ---- the classes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [70, 256])
def test_condition_numbers_of_the_classes(d):
    cond = {k: float(np.linalg.cond(S.scale_matrix(k, d, np.random.default_rng(d)))) for k in S.KINDS}
    print(f"[solve classes] d={d}: " + "  ".join(f"{k} {v:.3g}" for k, v in cond.items()))
    for kind, stated in (("default", 4.0), ("spd2", 1e2), ("spd4", 1e4)):
        assert stated / 2 <= cond[kind] <= 2 * stated, (kind, cond[kind])
    # the spectrum of the AR(1) correlation lies in ((1 - rho) / (1 + rho), (1 + rho) / (1 - rho)), kappa(C) = sqrt(kappa(Sigma))
    assert 50.0 <= cond["ar999"] <= 1999.0
    assert cond["graded"] >= 1e4                       # rows spanning several decades
    for kind in S.KINDS:
        C = S.scale_matrix(kind, d, np.random.default_rng(1))
        assert C.dtype == np.float64 and np.all(np.triu(C, 1) == 0.0) and np.all(np.diag(C) > 0.0)
        assert np.all(np.isfinite(C.astype(np.float32))) and np.all(np.diag(C.astype(np.float32)) > 0.0)


# ---- the emulations solve the system, on every path they have -----------------------------------------------------------------------------
@pytest.mark.parametrize("d,bs", [(70, 32), (200, 32), (64, 64), (192, 64), (256, 64), (256, 32)])
def test_emulations_solve_the_system(d, bs):
    rng = np.random.default_rng(d + bs)
    C = S.scale_matrix("default", d, rng).astype(np.float32)
    R = rng.normal(size=(d, 19)).astype(np.float32)
    ref = S.solve_ct(C.astype(np.float64), R.astype(np.float64))
    X = S.emulate_block_inverse_solve(C, R, bs)
    assert X.dtype == np.float32 and _rel(X, ref) <= 4.0 * d * 2.0 ** -24          # kappa d u
    assert 2.0 ** -18 <= _rel(S.emulate_block_inverse_solve(C, R, bs, keep_bits=16), ref) <= 2.0 ** -12   # the truncation is what is left
    if bs == 64:
        assert _rel(S.emulate_engine_solve(C, R), ref) <= 4.0 * d * 2.0 ** -22      # two-way f16 planes: 2^-22 per term


def test_truncate_bits_and_the_power_of_two_scale():
    x = np.float32(1.0) + np.float32(2.0 ** -16) + np.float32(2.0 ** -20)
    assert S.truncate_bits(np.array([x, -x]), 24).tolist() == [float(x), -float(x)]
    assert S.truncate_bits(np.array([x, -x]), 17).tolist() == [1.0 + 2.0 ** -16, -(1.0 + 2.0 ** -16)]
    assert S.truncate_bits(np.array([x, -x]), 16).tolist() == [1.0, -1.0]
    amax = np.array([1.0, 0.75, 2.0 ** -20, 3.0e4, 1.999], dtype=np.float32)
    s = S._pow2_scale(amax)
    assert np.all((s * amax >= 2.0 ** 13) & (s * amax < 2.0 ** 14)) and np.all(np.frexp(s)[0] == 0.5)


def test_block_ratios_see_an_error_confined_to_one_block_row():
    """X grows upward through the back-substitution: an error of a few float32 roundings of a SMALL block row vanishes in the whole-vector norm."""
    rng = np.random.default_rng(3)
    d = 200
    ref = rng.normal(size=(d, d)) * np.repeat(10.0 ** np.array([3.0, 0.0, 0.0, -3.0]), [64, 64, 64, 8])[:, None]
    yard = ref * (1.0 + 2.0 ** -22 * rng.normal(size=(d, d)))
    got = yard.copy()
    got[192:] = ref[192:] * (1.0 + 2.0 ** -14)
    whole, worst = S.block_ratios(got, yard, ref, d)
    assert whole <= 1.01 and worst >= 100.0
    assert S.block_ratios(yard, yard, ref, d) == (1.0, 1.0)
    # a flat gradient is (dmu, dC column-major): an error in the rows 64 .. 127 of dmu only
    gref = np.concatenate([rng.normal(size=d), np.tril(ref).reshape(-1, order="F")])
    gyard = gref * (1.0 + 2.0 ** -24)
    ggot = gyard.copy()
    ggot[64:128] *= 1.0 + 2.0 ** -18
    whole, worst = S.block_ratios(ggot, gyard, gref, d)
    assert whole <= 1.01 and worst >= 32.0
    # the floor: a yardstick that happens to be exact does not tighten the bound below float32 output rounding
    assert S.block_ratios(ref * (1.0 + 2.0 ** -24), ref, ref, d) == pytest.approx((1.0, 1.0))


# ---- the factor is admissible and has teeth ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ratios(kind, d, seed):
    """For the class, the size and the seed: {name: (whole, worst block)} of the emulated solves against the float32 yardstick."""
    rng = np.random.default_rng(1000 * seed + d)
    C = S.scale_matrix(kind, d, rng).astype(np.float32)
    mu = rng.normal(size=d).astype(np.float32)
    _, tgt = make_problem(rng, "diag", d, np.float32)
    params = np.concatenate([mu, C.reshape(-1, order="F")])
    out = {}
    for M in (32, 64, 128):
        eps = rng.normal(size=(d, M)).astype(np.float32)
        r64, r32 = S.stl_gradient(params, d, tgt, eps, 3, np.float64), S.stl_gradient(params, d, tgt, eps, 3, np.float32)

        def both(X, name):
            out[f"{name} X M={M}"] = S.block_ratios(X, r32["X"], r64["X"], d)
            out[f"{name} grad M={M}"] = S.block_ratios(S.stl_gradient_with_solve(params, d, tgt, eps, 3, X), r32["grad"], r64["grad"], d)

        if M == 128:
            both(S.emulate_engine_solve(C, eps), "engine")
            continue
        for bs in (64, 32):
            both(S.emulate_block_inverse_solve(C, eps, bs), f"block{bs}")
        both(S.emulate_block_inverse_solve(C, eps, 64, keep_bits=16), "cut16")
    return out


@pytest.mark.parametrize("d", [256, 512])
@pytest.mark.parametrize("kind", S.KINDS)
def test_the_factor_is_admissible(kind, d):
    """both emulations -- the block-inverse solve (64- and 32-row blocks) and the engine's f16 planes of C^-T -- stay within FACTOR x the
    float32 LAPACK yardstick, in the forward error of X and in the STL gradient, whole and per 64-row block"""
    worst = {}
    for seed in SEEDS:
        for name, (whole, block) in _ratios(kind, d, seed).items():
            if not name.startswith("cut16"):
                key = name.split(" M=")[0]
                worst[key] = tuple(max(a, b) for a, b in zip(worst.get(key, (0.0, 0.0)), (whole, block)))
    print(f"[solve emulation] {kind} d={d}: " + "  ".join(f"{k} {w:.2f}, {b:.2f}" for k, (w, b) in worst.items()))
    for name, (whole, block) in worst.items():
        assert whole <= FACTOR and block <= FACTOR, (name, whole, block)


@pytest.mark.parametrize("d", [256, 512])
@pytest.mark.parametrize("kind", S.KINDS)
def test_the_factor_has_teeth(kind, d):
    """inverted blocks cut to 16 significant bits: the gradient leaves the factor, whole and per block, on every class, size and seed"""
    low = (np.inf, np.inf)
    for seed in SEEDS:
        for name, r in _ratios(kind, d, seed).items():
            if name.startswith("cut16 grad"):
                low = tuple(min(a, b) for a, b in zip(low, r))
                assert r[0] > FACTOR and r[1] > FACTOR, (name, seed, r)
    print(f"[solve emulation] {kind} d={d}: blocks cut to 16 bits, smallest gradient ratio {low[0]:.1f}, {low[1]:.1f}")
