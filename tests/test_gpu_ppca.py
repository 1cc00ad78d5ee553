"""The probabilistic PCA target (mivi_set_target_ppca, csrc/kernels_ppca.hip) on the library's own draws against the float64 oracle with
tests/ppca_ref.py as the target: bound = max(TOL x scale, 8 x |the restatement in the context's dtype - float64|) on the value, the whole
gradient, and the W, Z, mu, a and s blocks each alone (the criterion of tests/test_gpu_hglm.py).  The other routes are held to the SAME
model as a host plugin on one context, by the same bound.  DESIGN.md section 8."""
import re

import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import _lib
from oracle import oracle as O
from tests.helpers import SEED, OraclePlugin
from tests.ppca_ref import LOG2PI, PPCARef
from tests.test_gpu_blockdiag import TOL
from tests.test_gpu_softmax import _family

gpu, DTYPES = pytest.mark.gpu, [np.float32, np.float64]
CF, STL, MID = avi.ClosedFormEntropy(), avi.StickingTheLandingEntropy(), (100, 12, 4, 7)   # MID: (N, D, k, M)
# one entry; a partial row tile with k and D no multiples of 4; D over two waves with a partial block of 16 columns (70 = 4 x 16 + 6: blocks
# 0, 1 | 2, 3 | 4 | none) and k past one block of 16; both limits (153 KB of LDS in f64); 1000 rows: ceil(1000 / 256) = 4 slices of 256, 256,
# 256 and 232 rows, the f32 accumulators flushed twice in each; and 70 samples, which the capped case below cuts into chunks of 64 + 6
SHAPES = [(1, 1, 1, 1), (17, 5, 3, 5), (40, 70, 17, 3), (20, 512, 32, 2), (1000, 6, 2, 3), (33, 9, 4, 70)]
PRI = dict(prior_std=1.3, mean_std=4.0, noise_scale=0.8)


def make_data(shape, kind, ard, dtype):
    N, D, k, M = shape
    rng = np.random.default_rng(1000 * N + 10 * D + k)
    d = D * k + N * k + D + (k if ard else 0) + 1
    loc, scale = rng.normal(size=d) * 0.5, rng.uniform(0.3, 0.9, size=d)
    loc[-1], big, shrink = (-3.0, 1e3, 0.02) if kind == "large" else (0.2, 1.0, 1.0)   # "large": |y| about 10^3 at s = -3: e^{-2s} (y - pred)^2 about 4 x 10^8
    Y = (big * (rng.normal(size=(N, k)) @ rng.normal(size=(k, D)) / np.sqrt(k) + 0.3 * rng.normal(size=(N, D)))).astype(dtype)
    mask = (rng.uniform(size=(N, D)) >= 0.3).astype(np.uint8) if kind == "mask" else None   # 30 % of the entries missing, row 3 and column 5 entirely
    if kind == "mask":
        mask[3 % N, :], mask[:, 5 % D] = 0, 0
        Y[mask == 0] = np.nan   # (never read)
    return Y, mask, avi.MeanFieldGaussian(loc.astype(dtype), (shrink * scale).astype(dtype))


def check(value, grad, params, ref_tgt, yard_tgt, eps, ent, dtype, tag):
    d = ref_tgt.dimension()
    ref, yard = (O.estimate_gradient(params.astype(np.float64), d, O.MEANFIELD, t, eps, ent.code) for t in (ref_tgt, yard_tgt))
    _, vt, gt = TOL[dtype]
    rg, yg = ref["grad"], yard["grad"]
    assert np.isfinite(ref["value"]) and np.all(np.isfinite(rg)) and np.isfinite(value) and np.all(np.isfinite(grad))
    bound = lambda ix, scale: max(gt * scale, 8 * np.linalg.norm(yg[ix] - rg[ix]))   # noqa: E731
    ratios = {"value": abs(value - ref["value"]) / max(vt * abs(ref["value"]), 8 * abs(yard["value"] - ref["value"])),
              "whole": np.linalg.norm(grad - rg) / bound(slice(None), max(np.linalg.norm(rg), 1.0))}
    oz, om = ref_tgt.D * ref_tgt.k, (ref_tgt.D + ref_tgt.N) * ref_tgt.k
    blk = {"W": np.r_[0:oz], "Z": np.r_[oz:om], "mu": np.r_[om:om + ref_tgt.D], "a": np.r_[om + ref_tgt.D:d - 1], "s": np.r_[d - 1:d]}
    blk = {name: ix for name, ix in blk.items() if ix.size}   # (no a block without ARD)
    floor = np.linalg.norm(rg) / np.sqrt(len(blk))
    for name, ix in blk.items():   # (the location gradient's blocks)
        ratios[name] = np.linalg.norm(grad[ix] - rg[ix]) / bound(ix, max(np.linalg.norm(rg[ix]), floor))
    worst = max(ratios, key=ratios.get)
    print(f"[ppca] {tag} {np.dtype(dtype).name} ent{ent.code}: value {ratios['value']:.3f} whole {ratios['whole']:.3f} worst {worst} {ratios[worst]:.3f}")
    assert ratios[worst] <= 1.0, ratios
    return rg


def run_case(shape, kind, ard, ent, dtype, likeadj=1.0, rows=None, cap=0):
    N, D, k, M = shape
    Y, mask, q = make_data(shape, kind, ard, dtype)
    prob = avi.PPCAProblem(Y, k, mask, ard, likeadj=likeadj, **PRI)
    params = avi.destructure(q)[0]
    ctx = avi.MiviContext(dtype, avi.MEANFIELD, prob.dimension(), M, ent.code, SEED)
    ctx.set_problem(prob if rows is None else prob.subsample(rows))
    ctx.ppca_set_part_cap(cap)   # (0: the default)
    eps = ctx.sample(params, 3)[1].cpu().numpy().astype(np.float64)
    value, grad = ctx.estimate_gradient(params, 3)
    ctx.synchronize()
    la = likeadj if rows is None else likeadj * N / len(rows)
    tgts = [PPCARef(Y, k, mask, ard, likeadj=la, rows=rows, dtype=t, **PRI) for t in (np.float64, dtype)]
    rg = check(float(value.item()), grad.cpu().numpy().astype(np.float64), params, *tgts, eps, ent, dtype, f"{shape} {kind} ard{int(ard)}")
    return ctx, prob, params, value.clone(), grad.clone(), rg


@pytest.mark.parametrize("ard", [False, True])
def test_reference_gradient_is_autograd_of_its_value(ard):
    N, D, k, rng, rows, la = 9, 5, 3, np.random.default_rng(5), np.array([7, 0, 4, 2, 8]), 2.5
    mask = (rng.uniform(size=(N, D)) < 0.7).astype(np.uint8)
    mask[4, :], mask[:, 1] = 0, 0   # a selected row and a column with nothing observed
    ref = PPCARef(rng.normal(size=(N, D)), k, mask, ard, likeadj=la, rows=rows, **PRI)
    prob = avi.PPCAProblem(ref.Y, k, mask, ard, likeadj=la, **PRI)
    z = torch.tensor(rng.normal(size=ref.dimension()) * 0.5, dtype=torch.float64, requires_grad=True)
    oz, om, hn = D * k, D * k + N * k, np.log(2.0) - 0.5 * LOG2PI
    W, Z, mu, s, m = z[:oz].reshape(k, D).T, z[oz:om].reshape(N, k)[rows], z[om:om + D], z[-1], torch.tensor(mask[rows], dtype=torch.float64)
    res = m * (torch.tensor(ref.Y[rows]) - mu - Z @ W.T)
    val = (la * (-0.5 * (res * res).sum() * (-2 * s).exp() - m.sum() * (s + 0.5 * LOG2PI) - 0.5 * (Z * Z).sum() - len(rows) * 0.5 * k * LOG2PI)
           - 0.5 * (mu * mu).sum() / 4.0 ** 2 - D * (np.log(4.0) + 0.5 * LOG2PI) + hn - np.log(0.8) - (2 * s).exp() / (2 * 0.8 ** 2) + s)
    a = z[om + D:om + D + k]   # (with ARD)
    val = val + ((-0.5 * (W * W).sum(0) * (-2 * a).exp() - D * (a + 0.5 * LOG2PI) + hn - np.log(1.3) - (2 * a).exp() / (2 * 1.3 ** 2) + a).sum() if ard
                 else -0.5 * (W * W).sum() / 1.3 ** 2 - D * k * (np.log(1.3) + 0.5 * LOG2PI))
    val.backward()
    v, g = ref.logdensity_and_gradient(z.detach().numpy())
    Wu, Zu, muu, au, su = prob.unpack(g)
    assert prob.dimension() == ref.dimension() and Wu.shape == (D, k) and Zu.shape == (N, k) and muu.shape == (D,) and (au is None) != ard and su == g[-1]
    assert np.array_equal(Wu[:, 1], g[D:2 * D]) and np.array_equal(Zu[2], g[oz + 2 * k:oz + 3 * k])
    assert v == pytest.approx(val.item(), rel=1e-13) and np.allclose(g, z.grad.numpy(), rtol=1e-11, atol=1e-12)
    assert not np.any(Zu[np.setdiff1d(np.arange(N), rows)]) and np.any(Zu[4])   # (row 4: the prior term alone)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("shape,kind,ent", [(s, "default", STL) for s in SHAPES] + [(SHAPES[2], "default", CF), (MID, "mask", STL), (MID, "large", STL)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v if isinstance(v, str) else f"ent{v.code}")
def test_shapes_and_data_classes(shape, kind, ent, ard, dtype):
    run_case(shape, kind, ard, ent, dtype)[0].close()


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kw", [dict(likeadj=7.5), dict(rows=[5, 99, 64, 0, 42, 3, 17, 63, 80])], ids=["likeadj", "rows"])
def test_likeadj_and_row_subset(kw, dtype):
    (N, D, k, M), (ctx, prob, params, v, g, rg) = MID, run_case(MID, "mask", True, CF, dtype, **kw)
    if "rows" in kw:
        # rows outside the selection: the target's gradient is EXACTLY zero -- closed form: a zero location gradient, the scale's the entropy's alone
        out = (D * k + k * np.setdiff1d(np.arange(N), kw["rows"])[:, None] + np.arange(k)).ravel()
        gn, d = g.cpu().numpy().astype(np.float64), prob.dimension()
        assert not np.any(gn[out]) and np.any(gn[D * k + k * 3:D * k + k * 4]) and np.allclose(gn[d + out], rg[d + out], rtol=8 * np.finfo(dtype).eps, atol=0)
        for bad, msg in (([0, 100], "out of range"), ([4, 9, 4], "repeated")):   # a failed call leaves the selection in force unchanged
            with pytest.raises(avi.MiviError, match=msg):
                ctx.set_problem(prob.subsample(bad))
            assert torch.equal(ctx.estimate_gradient(params, 3)[1], g)
        ctx.set_problem(prob)   # b = 0: back to the full set, bitwise what a fresh context gives
        full = run_case(MID, "mask", True, CF, dtype)
        v0, g0 = ctx.estimate_gradient(params, 3)
        assert torch.equal(v0, full[3]) and torch.equal(g0, full[4]) and not torch.equal(g0, g)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_bitwise_repeat_device_data_and_part_cap(dtype):
    (N, D, k, M), (ctx, prob, params, v, g, _), (Y, mask, _) = MID, run_case(MID, "mask", False, CF, dtype), make_data(MID, "mask", False, dtype)
    assert all(torch.equal(a, b) for a, b in zip(ctx.estimate_gradient(params, 3), (v, g)))
    dev = avi.PPCAProblem(torch.as_tensor(np.ascontiguousarray(Y.T)).cuda(), k, torch.as_tensor(np.ascontiguousarray(mask.T)).cuda(), **PRI)
    ctx.set_problem(dev)   # (D, N) contiguous = N x D column-major
    assert all(torch.equal(a, b) for a, b in zip(ctx.estimate_gradient(params, 3), (v, g)))
    # one slice: chunks of 3, 3 and 1 samples; and the 70 samples of the last shape as one chunk or as 64 + 6
    many = [run_case(SHAPES[5], "default", False, STL, dtype, cap=c) for c in (0, 64 * (9 * 4 + 9 + 3) * 8)] + [run_case(MID, "mask", False, CF, dtype, cap=3 * (D * k + D + 3) * 8)]
    assert torch.equal(many[0][4], many[1][4]) and torch.equal(many[0][3], many[1][3]) and torch.equal(many[2][3], v) and torch.equal(many[2][4], g)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route", ["fullrank", "lowrank", "blockdiag", "realnvp", "exp", "objective", "score"])
def test_routes_equal_the_same_model_as_a_plugin(route, dtype):
    """One context; the built-in target, then OraclePlugin(PPCARef) in float64 (the reference) and in the context's dtype (the restatement)."""
    (N, D, k, M), (Y, mask, _) = (20, 6, 2, 7), make_data((20, 6, 2, 7), "mask", True, dtype)   # d = 61: small enough for the full-rank family
    d = D * k + N * k + D + k + 1
    q = _family(route, d, dtype, np.random.default_rng(7))
    params = avi.destructure(q)[0]
    ctx = avi.MiviContext.for_family(q, M, STL.code, SEED)
    wrap = (lambda pr: avi.TransformedProblem(pr, avi.StackedBijector([(0, 5, "exp"), (5, d, "identity")]))) if route == "exp" else (lambda pr: pr)

    def run(prob):
        ctx.set_problem(wrap(prob))
        out = {"objective": lambda: [ctx.estimate_objective(params, 3, 50, avi.MonteCarloEntropy.code)],
               "score": lambda: ctx.estimate_score_gradient(params, 3)[:2]}.get(route, lambda: ctx.estimate_gradient(params, 3))()
        ctx.synchronize()
        return [t.cpu().numpy().astype(np.float64).ravel() for t in out]

    got = run(avi.PPCAProblem(Y, k, mask, True, **PRI))
    ref, yard = (run(OraclePlugin(PPCARef(Y, k, mask, True, dtype=t, **PRI))) for t in (np.float64, dtype))
    ctx.close()
    _, vt, gt = TOL[dtype]
    for i, (a, r, w) in enumerate(zip(got, ref, yard)):
        tol, scale = (vt, np.linalg.norm(r)) if a.size == 1 else (gt, max(np.linalg.norm(r), 1.0))
        ratio = np.linalg.norm(a - r) / max(tol * scale, 8 * np.linalg.norm(w - r))
        print(f"[ppca] route {route} {np.dtype(dtype).name} output {i}: ratio {ratio:.3f}")
        assert np.all(np.isfinite(a)) and ratio <= 1.0, (route, i, ratio)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_device_loop_equals_host_loop_and_subsampled_steps(dtype):
    (N, D, k, M), (Y, mask, q) = MID, make_data(MID, "mask", True, dtype)
    q0 = avi.MeanFieldGaussian(dtype(0.1) * q.location, np.full(len(q.location), 0.1, dtype))
    prob = avi.PPCAProblem(Y, k, mask, True)
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), optimizer=avi.Adam(1e-2), n_samples=M, operator=avi.ClipScale())
    q_dev, info_dev, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 5, prob, q0)
    q_host, info_host, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 5, prob, q0, device_loop=False)
    assert np.array_equal(avi.destructure(q_dev)[0], avi.destructure(q_host)[0]) and [i["elbo"] for i in info_dev] == [i["elbo"] for i in info_host]
    assert not np.array_equal(avi.destructure(q_dev)[0], avi.destructure(q0)[0])
    sub = avi.KLMinRepGradDescent(avi.AutoMIVI(), optimizer=avi.Adam(1e-2), n_samples=M, operator=avi.ClipScale(),
                                  subsampling=avi.ReshufflingBatchSubsampling(np.arange(N), 32))
    q_sub, info_sub, state = avi.optimize(avi.PhiloxRNG(SEED), sub, 5, prob, q0)
    assert "mivi_ppca_select_rows" in state["route_note"] and len(info_sub) == 5 and np.all(np.isfinite(avi.destructure(q_sub)[0]))


@gpu
def test_creation_errors_and_refusals_by_message():
    n, D, k, M = 6, 2, 1, 4
    d = D * k + n * k + D + 1   # 11: also the d of a 3 -> 2 -> 1 network, a softmax regression with p = 5, C = 2 and a GLM with p = 3, J = 7
    ctx = avi.MiviContext(np.float32, avi.FULLRANK, d, M, 0, SEED)
    lib, h, nan = ctx.lib, ctx.h, float("nan")
    Y, ones = np.zeros((n, D), np.float32, order="F"), np.ones((n, D), np.uint8, order="F")
    Ynan, m2, m0 = np.where(np.arange(n)[:, None] == 1, np.float32(nan), Y), ones + (np.arange(n)[:, None] == 2).astype(np.uint8), ones * (np.arange(n)[:, None] != 1).astype(np.uint8)
    model = lambda k=k, ard=0, ps=1.0, ms=1.0, ns=1.0, la=1.0: _lib.MiviPpca(k, ard, ps, ms, ns, la)   # noqa: E731
    call = lambda cfg, Yv, mv, nv, Dv: lib.mivi_set_target_ppca(h, _lib.C.byref(cfg), np.asfortranarray(Yv).ctypes.data,   # noqa: E731
                                                                  None if mv is None else np.asfortranarray(mv).ctypes.data, nv, Dv, 0)
    ok = (Y, None, n, D)
    for cfg, args, msg in ((model(), (Y, None, 0, D), "n must be"), (model(), (Y, None, n, 0), r"D must lie in \[1, 512\]"), (model(), (Y, None, n, 513), "D must lie"),
                           (model(k=0), ok, r"k must lie in \[1, 32\]"), (model(k=33), ok, "k must lie"), (model(k=2), ok, r"\+ 1, 19"), (model(ard=1), ok, r"\+ 1, 12"),
                           (model(ps=0.0), ok, "prior_std must be"), (model(ps=nan), ok, "prior_std"), (model(ms=-1.0), ok, "mean_std must be"),
                           (model(ms=float("inf")), ok, "mean_std"), (model(ns=0.0), ok, "noise_scale must be"), (model(ns=nan), ok, "noise_scale"),
                           (model(la=0.0), ok, "likelihood adjustment"), (model(la=nan), ok, "likelihood adjustment"), (model(), (Y, m2, n, D), "mask entry is not 0 or 1"),
                           (model(), (Ynan, None, n, D), "observed y is not finite"), (model(), (Ynan, ones, n, D), "observed y is not finite")):
        assert call(cfg, *args) == _lib.ERR_BAD_ARG, msg
        assert re.search(msg, lib.mivi_last_error(h).decode()), (msg, lib.mivi_last_error(h))
    assert call(model(), Ynan, m0, n, D) == 0   # (the NaNs are not observed)
    prob = avi.PPCAProblem(Y, k)
    ctx.set_problem(prob)
    buf, idx = ctx.empty(4 * d * d + 64), np.zeros(2, np.int64)
    for bad, la, msg in (([0, n], 1.0, "out of range"), ([-1], 1.0, "out of range"), ([1, 1], 1.0, "repeated"), ([0], 0.0, "likelihood adjustment")):
        bad = np.asarray(bad, np.int64)
        assert lib.mivi_ppca_select_rows(h, bad.ctypes.data, bad.size, la) == _lib.ERR_BAD_ARG and msg in lib.mivi_last_error(h).decode()
    P = ctx._p(buf)
    for name, args in {"mivi_gauss_expected_grad_hess2": (P, 0, 0, P, P, P), "mivi_logreg_seek_batch": (0,), "mivi_logreg_select_rows": (idx.ctypes.data, 2, 1.0),
                       "mivi_softmax_select_rows": (idx.ctypes.data, 2, 1.0), "mivi_bnn_select_rows": (idx.ctypes.data, 2, 1.0),
                       "mivi_hglm_select_rows": (idx.ctypes.data, 2, 1.0)}.items():
        assert getattr(lib, name)(h, *args) == _lib.ERR_UNSUPPORTED, name
        assert "probabilistic PCA target" in lib.mivi_last_error(h).decode() and name in lib.mivi_last_error(h).decode()
    for name, refused in (("mivi_optimize_loop_many", lambda: ctx.optimize_loop_many(buf[:2 * ctx.params_len], 2, 2, 0, 0)),
                          ("mivi_optimize_loop_batches", lambda: ctx.optimize_loop_batches(buf, 2, 0, 0)),
                          ("mivi_logreg_set_batch_schedule", lambda: ctx.set_batch_schedule(np.zeros((1, 2), np.int64), likeadj=1.0))):
        with pytest.raises(avi.MiviError, match=name + ".*probabilistic PCA target") as e:
            refused()
        assert e.value.status == _lib.ERR_UNSUPPORTED
    X3, y8 = np.zeros((8, 3), np.float32), np.zeros(8, np.float32)   # the other targets' contexts refuse the entry, by name
    for other, words in ((avi.BNNProblem(X3, y8, (2,)), "Bayesian neural network target"),   # the other targets' contexts refuse the entry, by name
                         (avi.SoftmaxRegProblem(np.zeros((8, 5), np.float32), np.zeros(8, np.uint8), 2), "softmax regression target"),
                         (avi.HierGLMProblem(X3, y8, np.arange(8) % 7, 7), "hierarchical GLM target")):
        ctx.set_problem(other)
        assert lib.mivi_ppca_select_rows(h, idx.ctypes.data, 1, 1.0) == _lib.ERR_UNSUPPORTED
        assert "mivi_ppca_select_rows" in lib.mivi_last_error(h).decode() and words in lib.mivi_last_error(h).decode()
    ctx.set_problem(avi.DiagNormalProblem(np.zeros(d, np.float32), np.ones(d, np.float32)))   # replaced cleanly: the entry has no target again
    assert lib.mivi_ppca_select_rows(h, None, 0, 1.0) == _lib.ERR_NO_TARGET
    ctx.close()
