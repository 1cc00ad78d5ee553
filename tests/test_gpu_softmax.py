"""The softmax regression target (mivi_set_target_softmax, csrc/kernels_softmax.hip) on the library's own draws against the float64 oracle
with tests/softmax_ref.py as the target: bound = max(TOL x scale, 8 x |the restatement in the context's dtype - float64|) on the value, the
whole gradient, every class block of the location gradient and the s entry alone (the criterion of tests/test_gpu_blockdiag.py).  The other
routes are held to the SAME model as a host plugin on one context, by the same bound (RealNVP takes d <= 128: p = 7 there).  DESIGN.md section 8."""
import re

import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import _lib
from oracle import oracle as O
from tests.helpers import SEED, OraclePlugin
from tests.softmax_ref import LOG2PI, SoftmaxRef
from tests.test_gpu_blockdiag import TOL

gpu = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
CF, STL = avi.ClosedFormEntropy(), avi.StickingTheLandingEntropy()
MID = (100, 17, 16, 7)
# the issue's shapes (65 / 130 rows, p = 17 / 33 / 70, C = 17, M = 5 / 3: past the row tile, the row slices, the staged chunk of p, the feature tile, the
# column tile, the sample groups), then C = 33 (three column tiles, one sample per group) and 16500 rows (slices of 528: past the 512-row flush of f32 sums)
SHAPES = [(1, 1, 2, 1), (17, 3, 2, 5), (65, 5, 3, 16), MID, (64, 16, 17, 3), (130, 33, 64, 2), (300, 70, 5, 33), (20, 4, 33, 3), (16500, 3, 2, 2)]


def make_data(n, p, C, M, kind, dtype, seed=0):
    rng = np.random.default_rng(1000 * n + 10 * p + C + seed)
    X = (rng.normal(size=(n, p)) / np.sqrt(p)).astype(dtype)
    y = rng.integers(0, C - 1 if kind == "unseen" else C, size=n).astype(np.uint8)   # unseen: class C - 1 is absent
    q = avi.MeanFieldGaussian((rng.normal(size=p * C + 1) * 0.7).astype(dtype), rng.uniform(0.3, 0.9, size=p * C + 1).astype(dtype))
    if kind == "saturated":   # |Lambda| reaches 100
        B = q.location[:p * C].astype(np.float64).reshape(p, C, order="F")
        X = (X * (100.0 / np.abs(X.astype(np.float64) @ B).max())).astype(dtype)
    return X, y, q


def check(value, grad, params, d, p, C, eps, ref_tgt, yard_tgt, ent, dtype, tag):
    ref = O.estimate_gradient(params.astype(np.float64), d, O.MEANFIELD, ref_tgt, eps, ent.code)
    yard = O.estimate_gradient(params.astype(np.float64), d, O.MEANFIELD, yard_tgt, eps, ent.code)
    _, vt, gt = TOL[dtype]
    rg, yg = ref["grad"], yard["grad"]
    assert np.isfinite(value) and np.all(np.isfinite(grad))
    bound = lambda ix, scale: max(gt * scale, 8 * np.linalg.norm(yg[ix] - rg[ix]))
    ratios = {"value": abs(value - ref["value"]) / max(vt * abs(ref["value"]), 8 * abs(yard["value"] - ref["value"])),
              "whole": np.linalg.norm(grad - rg) / bound(slice(None), max(np.linalg.norm(rg), 1.0))}
    floor = np.linalg.norm(rg) / np.sqrt(C + 1)
    for name, ix in [(f"class{c}", np.r_[c * p:(c + 1) * p]) for c in range(C)] + [("s", np.r_[d - 1:d])]:
        ratios[name] = np.linalg.norm(grad[ix] - rg[ix]) / bound(ix, max(np.linalg.norm(rg[ix]), floor))
    worst = max(ratios, key=ratios.get)
    print(f"[softmax] {tag} {np.dtype(dtype).name} ent{ent.code}: value {ratios['value']:.3f} whole {ratios['whole']:.3f} worst {worst} {ratios[worst]:.3f}")
    assert ratios[worst] <= 1.0, ratios


def run_case(shape, kind, ent, dtype, variant="logsigma_normal", likeadj=1.0, rows=None, cap=0):
    n, p, C, M = shape
    X, y, q = make_data(n, p, C, M, kind, dtype)
    d, params = p * C + 1, avi.destructure(q)[0]
    ctx = avi.MiviContext(dtype, avi.MEANFIELD, d, M, ent.code, SEED)
    prob = avi.SoftmaxRegProblem(X, y, C, variant, likeadj)
    ctx.set_problem(prob if rows is None else prob.subsample(rows))
    if cap:
        ctx.softmax_set_plane_cap(cap)
    eps = ctx.sample(params, 3)[1].cpu().numpy().astype(np.float64)
    value, grad = ctx.estimate_gradient(params, 3)
    ctx.synchronize()
    sel = slice(None) if rows is None else np.asarray(rows)
    la = likeadj if rows is None else likeadj * n / len(rows)
    tgts = [SoftmaxRef(X[sel], y[sel], C, variant, la, dtype=t) for t in (np.float64, dtype)]
    check(float(value.item()), grad.cpu().numpy().astype(np.float64), params, d, p, C, eps, *tgts, ent, dtype, f"{shape} {kind}")
    return ctx, prob, params, value.clone(), grad.clone()


def test_reference_gradient_is_autograd_of_its_value():
    for (n, p, C), variant in (((7, 3, 2), "logsigma_normal"), ((12, 4, 5), "lognormal_exp_bijector")):
        rng = np.random.default_rng(n)
        ref = SoftmaxRef(rng.normal(size=(n, p)), rng.integers(0, C, size=n), C, variant, likeadj=2.5)
        z = torch.tensor(rng.normal(size=p * C + 1) * 0.5, dtype=torch.float64, requires_grad=True)
        X, y, s = torch.tensor(ref.X), torch.tensor(ref.y), z[p * C]
        B = z[:p * C].reshape(C, p).T
        lp = -0.5 * p * C * LOG2PI - p * C * s - 0.5 * (B * B).sum() * torch.exp(-2 * s) + ((-0.5 * np.log(18 * np.pi) - torch.exp(2 * s) / 18) if variant == "logsigma_normal" else (-s - np.log(3.0) - 0.5 * LOG2PI - s * s / 18 + s))
        val = 2.5 * torch.log_softmax(X @ B, dim=1)[torch.arange(n), y].sum() + lp
        val.backward()
        v, g = ref.logdensity_and_gradient(z.detach().numpy())
        assert v == pytest.approx(float(val), rel=1e-13) and np.allclose(g, z.grad.numpy(), rtol=1e-12, atol=1e-13)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ent", [CF, STL], ids=["closed", "stl"])
@pytest.mark.parametrize("kind", ["default", "saturated", "unseen"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_and_data_classes(shape, kind, ent, dtype):
    run_case(shape, kind, ent, dtype)[0].close()


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kw", [dict(variant="lognormal_exp_bijector"), dict(likeadj=7.5), dict(rows=[5, 99, 5, 0, 42, 42, 64, 63, 17])], ids=["variant1", "likeadj", "rows"])
def test_variant_likeadj_and_row_subset(kw, dtype):
    ctx, prob, params, v, g = run_case(MID, "default", STL, dtype, **kw)
    if "rows" in kw:   # b = 0: back to the full set, bitwise what a context that never selected gives
        ctx.set_problem(prob)
        full = run_case(MID, "default", STL, dtype)
        v0, g0 = ctx.estimate_gradient(params, 3)
        assert torch.equal(v0, full[3]) and torch.equal(g0, full[4]) and not torch.equal(g0, g)
        with pytest.raises(avi.MiviError, match="out of range"):   # a failed call leaves the selection unchanged
            ctx.set_problem(prob.subsample([0, 100]))
        assert torch.equal(ctx.estimate_gradient(params, 3)[1], g0)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_bitwise_repeat_device_data_and_plane_cap(dtype):
    n, p, C, M = MID
    ctx, prob, params, v, g = run_case(MID, "default", CF, dtype)
    assert all(torch.equal(a, b) for a, b in zip(ctx.estimate_gradient(params, 3), (v, g)))
    X, y, _ = make_data(*MID, "default", dtype)
    dev = avi.SoftmaxRegProblem(torch.as_tensor(np.ascontiguousarray(X.T)).cuda(), torch.as_tensor(y).cuda(), C)   # (p, n) contiguous = n x p column-major
    ctx.set_problem(dev)
    assert all(torch.equal(a, b) for a, b in zip(ctx.estimate_gradient(params, 3), (v, g)))
    cap = 3 * n * C * np.dtype(dtype).itemsize   # three samples per chunk: chunks of 3, 3 and 1 (a partly filled column group in each)
    capped = run_case(MID, "default", CF, dtype, cap=cap)
    assert torch.equal(capped[3], v) and torch.equal(capped[4], g)


def _family(name, d, dtype, rng):
    mu, sig = (rng.normal(size=d) * 0.5).astype(dtype), rng.uniform(0.3, 0.9, size=d).astype(dtype)
    make = {"fullrank": lambda: avi.FullRankGaussian(mu, (np.tril(rng.normal(size=(d, d)) * (0.2 / np.sqrt(d)), -1) + np.diag(sig)).astype(dtype)),
            "lowrank": lambda: avi.LowRankGaussian(mu, sig, (rng.normal(size=(d, 5)) * 0.05).astype(dtype)),
            "blockdiag": lambda: avi.BlockDiagGaussian(mu, [(np.tril(rng.normal(size=(k, k)) * 0.05) + 0.5 * np.eye(k)).astype(dtype) for _, k, _ in avi.blockdiag_layout(d, 17)[0]]),
            "realnvp": lambda: avi.RealNVP(d, (16,), 2, eltype=dtype, rng=3)}
    return make.get(name, lambda: avi.MeanFieldGaussian(mu, sig))()


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route", ["meanfield", "fullrank", "lowrank", "blockdiag", "realnvp", "exp", "ordered", "objective", "score"])
def test_routes_equal_the_same_model_as_a_plugin(route, dtype):
    """One context; the built-in target, then OraclePlugin(SoftmaxRef) in float64 (the reference) and in the context's dtype (the restatement)."""
    n, p, C, M = (100, 7, 16, 7) if route == "realnvp" else MID
    X, y, _ = make_data(n, p, C, M, "default", dtype)
    d, rng = p * C + 1, np.random.default_rng(7)
    q = _family(route, d, dtype, rng)
    params = avi.destructure(q)[0]
    ctx = avi.MiviContext.for_family(q, M, STL.code, SEED)
    bij = {"exp": [(0, 5, "exp"), (5, d, "identity")], "ordered": [(0, p, "identity"), (p, 2 * p, "ordered"), (2 * p, d, "identity")]}.get(route)
    wrap = (lambda pr: avi.TransformedProblem(pr, avi.StackedBijector(bij))) if bij else (lambda pr: pr)

    def run(prob):
        ctx.set_problem(wrap(prob))
        out = {"objective": lambda: [ctx.estimate_objective(params, 3, 50, avi.MonteCarloEntropy.code)],
               "score": lambda: ctx.estimate_score_gradient(params, 3)[:2]}.get(route, lambda: ctx.estimate_gradient(params, 3))()
        ctx.synchronize()
        return [t.cpu().numpy().astype(np.float64).ravel() for t in out]

    got = run(avi.SoftmaxRegProblem(X, y, C))
    ref, yard = (run(OraclePlugin(SoftmaxRef(X, y, C, dtype=t))) for t in (np.float64, dtype))
    ctx.close()
    _, vt, gt = TOL[dtype]
    for k, (a, r, w) in enumerate(zip(got, ref, yard)):
        tol, scale = (vt, np.linalg.norm(r)) if a.size == 1 else (gt, max(np.linalg.norm(r), 1.0))
        ratio = np.linalg.norm(a - r) / max(tol * scale, 8 * np.linalg.norm(w - r))
        print(f"[softmax] route {route} {np.dtype(dtype).name} output {k}: ratio {ratio:.3f}")
        assert np.all(np.isfinite(a)) and ratio <= 1.0, (route, k, ratio)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_device_loop_equals_host_loop_and_subsampled_steps(dtype):
    n, p, C, M = MID
    X, y, q = make_data(*MID, "default", dtype)
    q0 = avi.MeanFieldGaussian(dtype(0.1) * q.location, np.full(p * C + 1, 0.1, dtype))   # (a start at which ten Descent steps stay finite)
    prob = avi.SoftmaxRegProblem(X, y, C)
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), optimizer=avi.Descent(1e-3), n_samples=M, operator=avi.ClipScale())
    q_dev, info_dev, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 10, prob, q0)
    q_host, info_host, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 10, prob, q0, device_loop=False)
    assert np.array_equal(avi.destructure(q_dev)[0], avi.destructure(q_host)[0]) and [i["elbo"] for i in info_dev] == [i["elbo"] for i in info_host]
    sub = avi.KLMinRepGradDescent(avi.AutoMIVI(), optimizer=avi.Descent(1e-3), n_samples=M, operator=avi.ClipScale(),
                                  subsampling=avi.ReshufflingBatchSubsampling(np.arange(n), 32))
    q_sub, info_sub, state = avi.optimize(avi.PhiloxRNG(SEED), sub, 5, prob, q0)
    assert "mivi_softmax_select_rows" in state["route_note"] and len(info_sub) == 5 and np.all(np.isfinite(avi.destructure(q_sub)[0]))


@gpu
def test_creation_errors_and_refusals_by_message():
    n, p, C, M, d = 8, 3, 4, 4, 13
    ctx = avi.MiviContext(np.float32, avi.FULLRANK, d, M, 0, SEED)
    lib, h = ctx.lib, ctx.h
    X, y = np.zeros((n, p), np.float32, order="F"), np.zeros(n, np.uint8)
    bad = np.array([0, 1, 4, 0, 0, 0, 0, 0], np.uint8)
    for args, msg in (((X, y, 0, C, 0, 1.0), "n must be"), ((X, y, n, 1, 0, 1.0), r"\[2, 64\]"), ((X, y, n, 65, 0, 1.0), r"\[2, 64\]"),
                      ((X, y, n, 5, 0, 1.0), "multiple of n_classes"), ((X, bad, n, C, 0, 1.0), "label"), ((X, y, n, C, 2, 1.0), "variant"),
                      ((X, y, n, C, 0, 0.0), "likelihood adjustment")):
        assert lib.mivi_set_target_softmax(h, args[0].ctypes.data, args[1].ctypes.data, *args[2:], 0) == _lib.ERR_BAD_ARG, msg
        assert re.search(msg, lib.mivi_last_error(h).decode()), (msg, lib.mivi_last_error(h))
    ctx.set_problem(avi.SoftmaxRegProblem(X, y, C))
    buf, idx = ctx.empty(4 * d * d + 64), np.zeros(2, np.int64)
    P = ctx._p(buf)
    for name, args in {"mivi_gauss_expected_grad_hess2": (P, 0, 0, P, P, P), "mivi_logreg_seek_batch": (0,), "mivi_logreg_select_rows": (idx.ctypes.data, 2, 1.0)}.items():
        assert getattr(lib, name)(h, *args) == _lib.ERR_UNSUPPORTED, name
        assert "softmax regression target" in lib.mivi_last_error(h).decode() and name in lib.mivi_last_error(h).decode()
    for name, refused in (("mivi_optimize_loop_many", lambda: ctx.optimize_loop_many(buf[:2 * ctx.params_len], 2, 2, 0, 0)),
                          ("mivi_optimize_loop_batches", lambda: ctx.optimize_loop_batches(buf, 2, 0, 0)),
                          ("mivi_logreg_set_batch_schedule", lambda: ctx.set_batch_schedule(np.zeros((1, 2), np.int64), likeadj=1.0))):
        with pytest.raises(avi.MiviError, match=name + ".*softmax regression target") as e:
            refused()
        assert e.value.status == _lib.ERR_UNSUPPORTED
    ctx.set_problem(avi.DiagNormalProblem(np.zeros(d, np.float32), np.ones(d, np.float32)))   # replaced cleanly: the rows entry has no target again
    assert lib.mivi_softmax_select_rows(h, None, 0, 1.0) == _lib.ERR_NO_TARGET
    ctx.close()
