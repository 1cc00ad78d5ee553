"""CPU checks of tests/meanfield_ref.py, the per-entry float32 yardstick the mean-field kernels are held to on the GPU
(tests/test_gpu_meanfield_yardstick.py).  No GPU, a few seconds.

1. gradient(..., np.float64) is oracle.estimate_gradient to 1e-13 for the diagonal, funnel and dense targets under the five entropy kinds;
   the exp-bijector case is pinned against torch autograd of the literal forward.
2. Float32 numpy emulations of the three DOCUMENTED summation orders (meanfield_ref.emulate: single launch, split columns whose chunks go
   to f64, the loop's one chunk with sixteen sequential terms per thread at M = 4096) stay at or under F32_FACTOR = 8 on every class at
   EMU_SHAPES under the entropy kinds 0 and 3.
   Measured, worst over the shapes and both kinds (whole, quad, entry, value):
       class     single launch and loop        split columns
       default   0.82  3.01  3.25  0.13        0.42  0.95  1.88  0.11
       graded    1.81  3.06  3.84  1.55        1.47  2.33  2.33  0.61
       far       2.08  3.29  4.04  1.00        1.01  2.76  2.88  0.15
       near      0.44  1.61  3.06  0.16        0.16  0.64  1.04  0.01
   (the loop's one chunk IS the single launch's order whenever that does not split; at (130, 300) and (130, 4096) it is the sixteen-term
   thread against the f64 chunks.)  Against |ONE float32 evaluation - ref| per entry instead of the envelope the single launch at
   (1024, 256) scores 32 (default), 45 (graded), 50 (far), 94 (near); against the envelope 2.2, 3.2, 3.2, 1.2.
3. Every injected fault scores above F32_FACTOR on the entry or the quad ratio, on every class (exempt: a dropped column on the class
   `near` under the entropy kinds 3 and 4, where W cancels to 1e-3 of a term by construction).
   Measured, max(quad, entry) per fault over the classes and FAULT_SHAPES, lowest .. highest, and the relative l2 of the whole gradient
   the older tests bound by 4e-5:
       one column dropped in one row         1.4e3 .. 5.1e5 (near, kinds 3 / 4, exempt: 3.3 .. 155)     l2 6.1e-8 .. 5.1e-3
       last chunk dropped in the last quad   239 .. 2.2e6                                               l2 2.7e-5 .. 9.3e-2
       eps / sigma dropped in one row        105 .. 1.1e7                                               l2 2.7e-8 .. 0.95
       row d - 1 with row d - 2's sigma      227 .. 1.7e7                                               l2 2.8e-8 .. 0.33
       1 / M from the first chunk's count    4.4e3 .. 2.5e8                                             l2 3.9e-7 .. 37
       funnel row 0 left unwritten           1.2e6 .. 3.8e6                                             l2 0.53 .. 1.0
   The whole-gradient l2 at 4e-5 LETS THROUGH (OLD_CRITERION_PASSES, asserted below): the dropped column on default (130 x 300, 1024 x 256,
   130 x 4096), graded (every shape, at most 8.2e-6) and far (1024 x 256, 130 x 4096); the dropped last chunk on graded 130 x 300; the
   dropped eps / sigma on graded (both shapes) and far 1024 x 256; the neighbour's sigma on graded (every shape, 2.8e-8 at 130 x 33) and
   far; the local count on graded (130 x 300 and, under kind 0, 130 x 4096: 3.9e-7 where the quad ratio is 8.7e7).  The unwritten funnel
   row 0 it sees: that row carries most of the funnel's gradient norm."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import meanfield_ref as Mf
from tests.helpers import SEED, make_problem
from tests.measure_space_cases import F32_FACTOR

OLD_GRAD_RTOL = 4e-5  # tests/test_gpu_meanfield_sweep.py: ||g - ref|| <= 4e-5 max(||ref||, 1)
EMU_SHAPES = [(7, 1), (1023, 1), (130, 4), (130, 33), (130, 300), (1024, 256), (130, 4096)]
ENTS = (O.ENT_CLOSED_FORM, O.ENT_STL)


@functools.lru_cache(maxsize=None)
def _case(kind, d, M, ent):
    """(params f32, target on the f32-stored m and s, eps f32, ref, env, S) of one class and shape: the draws are the library's own Philox
    stream (oracle.philox_normal) rounded to float32"""
    rng = np.random.default_rng(d * 131 + M + 7 * CLASS_ID[kind])
    mu, sigma, m, s = Mf.family_and_target(kind, d, rng)
    params = np.concatenate([mu, sigma]).astype(np.float32)
    tgt = O.FunnelStackedTarget(d, 1.5) if m is None else O.DiagNormalTarget(m.astype(np.float32), s.astype(np.float32))
    eps = O.philox_normal(SEED, 3, d, 0, M).astype(np.float32)
    ref = Mf.gradient(params, d, tgt, eps, ent, np.float64)
    return params, tgt, eps, ref, Mf.envelope(params, d, tgt, eps, ent, np.float32, ref), Mf.magnitude(params, d, tgt, eps, ent)


CLASS_ID = {k: i for i, k in enumerate(Mf.CLASSES + Mf.FUNNEL_CLASSES)}


def _score(kind, d, M, ent, got):
    params, tgt, eps, ref, env, mag = _case(kind, d, M, ent)
    whole, quad, entry = Mf.ratios(got["grad"], env["grad"], ref["grad"], mag["grad"], d, Mf.U32)
    value = Mf.value_ratio(got["value"], env["value"], ref["value"], mag["value"], Mf.U32)
    old = float(np.linalg.norm(got["grad"].astype(np.float64) - ref["grad"]) / max(np.linalg.norm(ref["grad"]), 1.0))
    return whole, quad, entry, value, old


# ---- 1. the float64 restatement is the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ent", range(5))
@pytest.mark.parametrize("target", ["diag", "funnel", "dense"])
def test_float64_gradient_is_the_oracle(target, ent):
    for d, M in [(5, 1), (37, 19)]:
        rng = np.random.default_rng(11 * d + ent)
        tgt = make_problem(rng, target, d)[1]
        mu, sigma = (0.3 if target == "funnel" else 1.0) * rng.normal(size=d), rng.uniform(0.5, 1.5, size=d)
        params = np.concatenate([mu, sigma])
        eps = O.philox_normal(SEED, 5, d, 0, M)
        ref = O.estimate_gradient(params, d, O.MEANFIELD, tgt, eps, ent)
        got = Mf.gradient(params, d, tgt, eps, ent, np.float64)
        assert abs(got["value"] - ref["value"]) <= 1e-13 * max(1.0, abs(ref["value"]))
        assert np.max(np.abs(got["grad"] - ref["grad"])) <= 1e-13 * max(1.0, np.max(np.abs(ref["grad"])))
        perm = Mf.gradient(params, d, tgt, eps, ent, np.float64, np.random.default_rng(1).permutation(M))
        assert np.max(np.abs(perm["grad"] - ref["grad"])) <= 1e-13 * max(1.0, np.max(np.abs(ref["grad"])))
        wide = Mf.gradient(params, d, tgt, eps, ent, np.longdouble)
        assert wide["grad"].dtype == np.longdouble and np.max(np.abs(wide["grad"] - ref["grad"])) <= 1e-13 * max(1.0, np.max(np.abs(ref["grad"])))


@pytest.mark.parametrize("ent", range(5))
def test_exp_bijector_gradient_matches_autograd_of_the_literal_forward(ent):
    """value = -(mean_m [log pi(binv(z_m)) + sum_exp-rows z_m] + entropy) written out in torch float64 with z = mu + sigma eps; the entropy's
    stopped copies (kinds 1, 3, 4) are detached parameters, as the reference's q_stop"""
    d, M = 9, 13
    rng = np.random.default_rng(17 + ent)
    inner = make_problem(rng, "diag", d)[1]
    blocks = [(0, d // 2, "identity"), (d // 2, d, "exp")]
    tgt = O.StackedBijectorTarget(inner, blocks)
    params = np.concatenate([0.5 * rng.normal(size=d), rng.uniform(0.5, 1.5, size=d)])
    eps = O.philox_normal(SEED, 9, d, 0, M)
    got = Mf.gradient(params, d, tgt, eps, ent, np.float64)
    ref = O.estimate_gradient(params, d, O.MEANFIELD, tgt, eps, ent)
    assert np.max(np.abs(got["grad"] - ref["grad"])) <= 1e-13 * max(1.0, np.max(np.abs(ref["grad"])))
    tp = torch.tensor(params, dtype=torch.float64, requires_grad=True)
    te = torch.tensor(eps, dtype=torch.float64)
    mu, sg = tp[:d], tp[d:]
    mu_s, sg_s = mu.detach(), sg.detach()
    Z = mu[:, None] + sg[:, None] * te
    mask = torch.tensor(tgt.mask)[:, None]
    X = torch.where(mask, torch.exp(Z), Z)
    m, s = torch.tensor(inner.mean)[:, None], torch.tensor(inner.std)[:, None]
    ell = -0.5 * torch.sum(((X - m) / s) ** 2, dim=0) - torch.sum(torch.log(s)) - 0.5 * d * Mf.LOG2PI + torch.sum(torch.where(mask, Z, torch.zeros_like(Z)), dim=0)

    def neg_logq(mu_, sg_):   # -log q(z) of the diagonal family
        return torch.mean(torch.sum(0.5 * ((Z - mu_[:, None]) / sg_[:, None]) ** 2, dim=0)) + 0.5 * d * Mf.LOG2PI + torch.sum(torch.log(sg_))

    closed = lambda sg_: d * 0.5 * (1.0 + Mf.LOG2PI) + torch.sum(torch.log(sg_))
    entropy = {0: lambda: closed(sg), 1: lambda: closed(sg_s), 2: lambda: neg_logq(mu, sg), 3: lambda: neg_logq(mu_s, sg_s),
               4: lambda: neg_logq(mu_s, sg_s) - closed(sg) + closed(sg_s)}[ent]()
    value = -(torch.mean(ell) + entropy)
    value.backward()
    value = float(value.detach())
    assert abs(value - float(got["value"])) <= 1e-12 * max(1.0, abs(value))
    tg = tp.grad.numpy()
    assert np.max(np.abs(got["grad"] - tg)) <= 1e-12 * max(1.0, np.max(np.abs(tg))), np.max(np.abs(got["grad"] - tg))


def test_shape_rule_of_the_single_call():
    """the shapes the GPU test relies on: (chunks, columns per chunk)"""
    assert Mf.n_cc(130, 256) == (1, 256) and Mf.n_cc(2048, 257) == (1, 512) and Mf.n_cc(2049, 300) == (1, 512)
    assert Mf.n_cc(130, 300) == (2, 256) and Mf.n_cc(40, 513) == (3, 256) and Mf.n_cc(6, 4096) == (16, 256)
    assert Mf.n_cc(1600, 2000) == (3, 768) and Mf.n_cc(130, 4096) == (16, 256) and Mf.n_cc(6, 4097) == (17, 256)


# ---- 2. the documented summation orders stay within the factor ---------------------------------------------------------------------------------------
def _routes(d, M):
    return ("single", "loop") if Mf.n_cc(d, M)[0] == 1 else ("split", "loop")


@pytest.mark.parametrize("kind", Mf.CLASSES)
def test_documented_summation_orders_stay_within_the_factor(kind):
    worst = {}
    for d, M in EMU_SHAPES:
        for ent in ENTS:
            params, tgt, eps, _, _, _ = _case(kind, d, M, ent)
            for route in _routes(d, M):
                whole, quad, entry, value, old = _score(kind, d, M, ent, Mf.emulate(params, d, tgt, eps, ent, route))
                print(f"[meanfield emulation] {route} {kind} {d} {M} ent{ent}: {whole:.2f}, {quad:.2f}, {entry:.2f}, {value:.2f}")
                worst[route] = np.maximum(worst.get(route, np.zeros(4)), [whole, quad, entry, value])
                assert max(whole, quad, entry, value) <= F32_FACTOR, (route, kind, d, M, ent, whole, quad, entry, value)
    print(f"[meanfield emulation] worst of {kind} (whole, quad, entry, value):", {r: np.round(w, 2).tolist() for r, w in worst.items()})


# ---- 3. the faults -------------------------------------------------------------------------------------------------------------------------------
FAULT_SHAPES = {"drop_column": [(130, 33), (130, 300), (1024, 256), (130, 4096)], "drop_last_chunk": [(130, 300), (130, 4096)],
                "drop_stl": [(130, 33), (1024, 256)], "wrong_sigma": [(130, 33), (1023, 1)], "local_count": [(130, 300), (130, 4096)]}


def _fault(name, d, M):
    rng = np.random.default_rng(d + M)
    row = int(rng.integers(0, d))
    return {"drop_column": (name, row, int(rng.integers(0, M))), "drop_last_chunk": (name,), "drop_stl": (name, row), "wrong_sigma": (name,),
            "local_count": (name, int(rng.integers(0, (d + 3) // 4)))}[name]


def fault_scores(name, kind):
    """[(d, M, ent, route, whole, quad, entry, relative l2 of the whole gradient)] of one fault on one class"""
    out = []
    for d, M in FAULT_SHAPES[name]:
        for ent in ((O.ENT_STL,) if name == "drop_stl" else ENTS):
            params, tgt, eps, _, _, _ = _case(kind, d, M, ent)
            route = _routes(d, M)[0]
            whole, quad, entry, _, old = _score(kind, d, M, ent, Mf.emulate(params, d, tgt, eps, ent, route, _fault(name, d, M)))
            out.append((d, M, ent, route, whole, quad, entry, old))
    return out


@pytest.mark.parametrize("kind", Mf.CLASSES)
@pytest.mark.parametrize("name", Mf.FAULTS)
def test_every_fault_is_seen_per_entry_or_per_quad(name, kind):
    passed_old = 0
    for d, M, ent, route, whole, quad, entry, old in fault_scores(name, kind):
        print(f"[meanfield fault] {name} {kind} {d} {M} ent{ent} {route}: whole {whole:.3g}, quad {quad:.3g}, entry {entry:.3g}, old l2 {old:.2e}")
        passed_old += old <= OLD_GRAD_RTOL
        if name == "drop_column" and kind == "near" and ent in Mf.STL:
            continue   # W cancels to 1e-3 of a term: the column is invisible by construction
        assert max(quad, entry) > F32_FACTOR, (name, kind, d, M, ent, whole, quad, entry)
    if (name, kind) in OLD_CRITERION_PASSES:
        assert passed_old > 0, (name, kind)


# fault x class pairs on which the whole-gradient relative l2 at 4e-5 lets the faulted emulation through at one shape of FAULT_SHAPES or more
OLD_CRITERION_PASSES = {("drop_column", "default"), ("drop_column", "graded"), ("drop_column", "far"), ("drop_last_chunk", "graded"),
                        ("drop_stl", "graded"), ("drop_stl", "far"), ("wrong_sigma", "graded"), ("wrong_sigma", "far"), ("local_count", "graded")}


def test_funnel_row_zero_left_unwritten_is_seen():
    """the funnel's row 0 belongs to another workgroup than rows 1 .. 3 (the value workgroup): the float32 yardstick with entries 0 and d
    left at zero"""
    for kind in Mf.FUNNEL_CLASSES:
        for d, M in [(6, 3), (130, 64), (1024, 200)]:
            for ent in ENTS:
                params, tgt, eps, ref, env, mag = _case(kind, d, M, ent)
                got = Mf.gradient(params, d, tgt, eps, ent, np.float32)
                whole, quad, entry = Mf.ratios(got["grad"], env["grad"], ref["grad"], mag["grad"], d, Mf.U32)
                assert max(whole, quad, entry) <= 1.0 + 1e-12   # (one of the envelope's own orders)
                g = got["grad"].copy()
                g[0] = g[d] = 0.0
                whole, quad, entry = Mf.ratios(g, env["grad"], ref["grad"], mag["grad"], d, Mf.U32)
                old = float(np.linalg.norm(g.astype(np.float64) - ref["grad"]) / max(np.linalg.norm(ref["grad"]), 1.0))
                print(f"[meanfield fault] funnel_row0 {kind} {d} {M} ent{ent}: whole {whole:.3g}, quad {quad:.3g}, entry {entry:.3g}, old l2 {old:.2e}")
                assert max(quad, entry) > F32_FACTOR, (kind, d, M, ent, whole, quad, entry)


def test_one_float32_evaluation_is_no_per_entry_denominator():
    """why the envelope: against |ONE float32 evaluation - ref| per entry (floored at 2^-24 |ref|) the documented order scores far above
    the factor on every class, against the envelope of eight under it"""
    d, M, ent = 1024, 256, 0
    for kind in Mf.CLASSES:
        params, tgt, eps, ref, env, mag = _case(kind, d, M, ent)
        got = Mf.emulate(params, d, tgt, eps, ent, "single")["grad"].astype(np.float64)
        one = np.abs(Mf.gradient(params, d, tgt, eps, ent, np.float32)["grad"].astype(np.float64) - ref["grad"])
        single = float(np.max(np.abs(got - ref["grad"]) / np.maximum(one, Mf.U32 * np.abs(ref["grad"]))))
        entry = Mf.ratios(got, env["grad"], ref["grad"], mag["grad"], d, Mf.U32)[2]
        print(f"[meanfield emulation] {kind}: per entry against one float32 evaluation {single:.1f}, against the envelope {entry:.2f}")
        assert single > F32_FACTOR >= entry, (kind, single, entry)
