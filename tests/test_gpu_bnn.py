"""The Bayesian neural network target (mivi_set_target_bnn, csrc/kernels_bnn.hip) on the library's own draws against the float64 oracle with
tests/bnn_ref.py as the target: bound = max(TOL x scale, 8 x |the restatement in the context's dtype - float64|) on the value, the whole
gradient and every parameter block of the location gradient (each W_l and each b_l alone; the criterion of tests/test_gpu_softmax.py).  The
other routes are held to the SAME model as a host plugin on one context, by the same bound (RealNVP takes d <= 128).  DESIGN.md section 8."""
import re

import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import _lib
from oracle import oracle as O
from tests.bnn_ref import BNNRef
from tests.helpers import SEED, OraclePlugin
from tests.test_gpu_blockdiag import TOL
from tests.test_gpu_softmax import _family

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
LIKS = ["bernoulli", "normal"]
CF, STL = avi.ClosedFormEntropy(), avi.StickingTheLandingEntropy()
MID, SMALL = (100, 7, (16, 5), 7), (100, 3, (8, 4), 7)   # (n, p, hidden, M); SMALL: d = 73 for RealNVP
# one row and one unit; a partial row tile; widths on and just past a 16-tile with a second group of row tiles; every limit (the LDS maximum);
# 700 rows: ceil(700 / 256) = 3 slices of 240, 240 and 220 rows -- a partial last tile, and a flush of the f32 sums every 128 rows
SHAPES = [(1, 1, (1,), 1), (17, 3, (5,), 5), (65, 17, (16, 17), 3), (40, 64, (64, 64, 64), 2), (700, 5, (20,), 2)]
ids = lambda s: "x".join(map(str, s[:2])) + "x" + "-".join(map(str, s[2])) + f"x{s[3]}"   # noqa: E731


def make_data(shape, lik, kind, dtype):
    n, p, hidden, M = shape
    rng = np.random.default_rng(1000 * n + 10 * p + sum(hidden))
    X = (rng.normal(size=(n, p)) / np.sqrt(p)).astype(dtype)
    y = (rng.integers(0, 2, size=n) if lik == "bernoulli" else rng.normal(size=n)).astype(dtype)
    d = BNNRef(X, y, hidden).dimension()
    loc, scale = rng.normal(size=d) * 0.7, rng.uniform(0.3, 0.9, size=d)
    if kind == "saturated":   # |pre-activations| reach 20 (tanh' underflows), |f| reaches 100 (sigma saturates), at the location
        a, scale = X.astype(np.float64), scale * 0.02
        for k, (W, b) in enumerate(BNNRef(X, y, hidden).unpack(loc)):   # (views of loc)
            s = (20.0 if k < len(hidden) else 100.0) / np.abs(a @ W.T + b).max()
            W *= s
            b *= s
            a = np.tanh(a @ W.T + b)
    return X, y, avi.MeanFieldGaussian(loc.astype(dtype), scale.astype(dtype))


def check(value, grad, params, ref_tgt, yard_tgt, eps, ent, dtype, tag):
    d = ref_tgt.dimension()
    ref, yard = (O.estimate_gradient(params.astype(np.float64), d, O.MEANFIELD, t, eps, ent.code) for t in (ref_tgt, yard_tgt))
    _, vt, gt = TOL[dtype]
    rg, yg = ref["grad"], yard["grad"]
    assert np.isfinite(ref["value"]) and np.all(np.isfinite(rg)) and np.isfinite(value) and np.all(np.isfinite(grad))
    bound = lambda ix, scale: max(gt * scale, 8 * np.linalg.norm(yg[ix] - rg[ix]))
    ratios = {"value": abs(value - ref["value"]) / max(vt * abs(ref["value"]), 8 * abs(yard["value"] - ref["value"])),
              "whole": np.linalg.norm(grad - rg) / bound(slice(None), max(np.linalg.norm(rg), 1.0))}
    blocks, off = [], 0
    for k, (i, o) in enumerate(zip(ref_tgt.widths, ref_tgt.widths[1:])):
        blocks += [(f"W{k + 1}", np.r_[off:off + o * i]), (f"b{k + 1}", np.r_[off + o * i:off + o * (i + 1)])]
        off += o * (i + 1)
    floor = np.linalg.norm(rg) / np.sqrt(len(blocks))
    for name, ix in blocks:
        ratios[name] = np.linalg.norm(grad[ix] - rg[ix]) / bound(ix, max(np.linalg.norm(rg[ix]), floor))
    worst = max(ratios, key=ratios.get)
    print(f"[bnn] {tag} {np.dtype(dtype).name} ent{ent.code}: value {ratios['value']:.3f} whole {ratios['whole']:.3f} worst {worst} {ratios[worst]:.3f}")
    assert ratios[worst] <= 1.0, ratios


def run_case(shape, lik, kind, ent, dtype, likeadj=1.0, rows=None, cap=0):
    n, p, hidden, M = shape
    X, y, q = make_data(shape, lik, kind, dtype)
    kw = dict(likelihood=lik, noise=0.7, prior_std=1.3)
    prob = avi.BNNProblem(X, y, hidden, likeadj=likeadj, **kw)
    params = avi.destructure(q)[0]
    ctx = avi.MiviContext(dtype, avi.MEANFIELD, prob.dimension(), M, ent.code, SEED)
    ctx.set_problem(prob if rows is None else prob.subsample(rows))
    if cap:
        ctx.bnn_set_part_cap(cap)
    eps = ctx.sample(params, 3)[1].cpu().numpy().astype(np.float64)
    value, grad = ctx.estimate_gradient(params, 3)
    ctx.synchronize()
    sel = slice(None) if rows is None else np.asarray(rows)
    la = likeadj if rows is None else likeadj * n / len(rows)
    tgts = [BNNRef(X[sel], y[sel], hidden, likeadj=la, dtype=t, **kw) for t in (np.float64, dtype)]
    check(float(value.item()), grad.cpu().numpy().astype(np.float64), params, *tgts, eps, ent, dtype, f"{ids(shape)} {lik} {kind}")
    return ctx, prob, params, value.clone(), grad.clone()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lik", LIKS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_shapes(shape, lik, dtype):
    run_case(shape, lik, "default", CF, dtype)[0].close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lik", LIKS)
@pytest.mark.parametrize("kind", ["default", "saturated"])
def test_data_classes_sticking_the_landing(kind, lik, dtype):
    run_case(MID, lik, kind, STL, dtype)[0].close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kw", [dict(likeadj=7.5), dict(rows=[5, 99, 5, 0, 42, 42, 64, 63, 17])], ids=["likeadj", "rows"])
def test_likeadj_and_row_subset(kw, dtype):
    ctx, prob, params, v, g = run_case(MID, "bernoulli", "default", STL, dtype, **kw)
    if "rows" in kw:   # b = 0: back to the full set, bitwise what a context that never selected gives
        ctx.set_problem(prob)
        full = run_case(MID, "bernoulli", "default", STL, dtype)
        v0, g0 = ctx.estimate_gradient(params, 3)
        assert torch.equal(v0, full[3]) and torch.equal(g0, full[4]) and not torch.equal(g0, g)
        with pytest.raises(avi.MiviError, match="out of range"):   # a failed call leaves the selection unchanged
            ctx.set_problem(prob.subsample([0, 100]))
        assert torch.equal(ctx.estimate_gradient(params, 3)[1], g0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bitwise_repeat_device_data_and_part_cap(dtype):
    n, p, hidden, M = MID
    ctx, prob, params, v, g = run_case(MID, "normal", "default", CF, dtype)
    assert all(torch.equal(a, b) for a, b in zip(ctx.estimate_gradient(params, 3), (v, g)))
    X, y, _ = make_data(MID, "normal", "default", dtype)
    dev = avi.BNNProblem(torch.as_tensor(np.ascontiguousarray(X.T)).cuda(), torch.as_tensor(y).cuda(), hidden, "normal", noise=0.7, prior_std=1.3)
    ctx.set_problem(dev)   # (p, n) contiguous = n x p column-major
    assert all(torch.equal(a, b) for a, b in zip(ctx.estimate_gradient(params, 3), (v, g)))
    capped = run_case(MID, "normal", "default", CF, dtype, cap=3 * prob.dimension() * 8)   # one slice: chunks of 3, 3 and 1 samples
    assert torch.equal(capped[3], v) and torch.equal(capped[4], g)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route", ["meanfield", "fullrank", "lowrank", "blockdiag", "realnvp", "exp", "objective", "score"])
def test_routes_equal_the_same_model_as_a_plugin(route, dtype):
    """One context; the built-in target, then OraclePlugin(BNNRef) in float64 (the reference) and in the context's dtype (the restatement)."""
    shape = SMALL if route == "realnvp" else MID
    (n, p, hidden, M), (X, y, _) = shape, make_data(shape, "bernoulli", "default", dtype)
    d = BNNRef(X, y, hidden).dimension()
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

    got = run(avi.BNNProblem(X, y, hidden))
    ref, yard = (run(OraclePlugin(BNNRef(X, y, hidden, dtype=t))) for t in (np.float64, dtype))
    ctx.close()
    _, vt, gt = TOL[dtype]
    for k, (a, r, w) in enumerate(zip(got, ref, yard)):
        tol, scale = (vt, np.linalg.norm(r)) if a.size == 1 else (gt, max(np.linalg.norm(r), 1.0))
        ratio = np.linalg.norm(a - r) / max(tol * scale, 8 * np.linalg.norm(w - r))
        print(f"[bnn] route {route} {np.dtype(dtype).name} output {k}: ratio {ratio:.3f}")
        assert np.all(np.isfinite(a)) and ratio <= 1.0, (route, k, ratio)


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_loop_equals_host_loop_and_subsampled_steps(dtype):
    n, p, hidden, M = MID
    X, y, q = make_data(MID, "bernoulli", "default", dtype)
    q0 = avi.MeanFieldGaussian(dtype(0.1) * q.location, np.full(len(q.location), 0.1, dtype))
    prob = avi.BNNProblem(X, y, hidden)
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), optimizer=avi.Adam(1e-2), n_samples=M, operator=avi.ClipScale())
    q_dev, info_dev, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 5, prob, q0)
    q_host, info_host, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 5, prob, q0, device_loop=False)
    assert np.array_equal(avi.destructure(q_dev)[0], avi.destructure(q_host)[0]) and [i["elbo"] for i in info_dev] == [i["elbo"] for i in info_host]
    assert not np.array_equal(avi.destructure(q_dev)[0], avi.destructure(q0)[0])
    sub = avi.KLMinRepGradDescent(avi.AutoMIVI(), optimizer=avi.Adam(1e-2), n_samples=M, operator=avi.ClipScale(),
                                  subsampling=avi.ReshufflingBatchSubsampling(np.arange(n), 32))
    q_sub, info_sub, state = avi.optimize(avi.PhiloxRNG(SEED), sub, 5, prob, q0)
    assert "mivi_bnn_select_rows" in state["route_note"] and len(info_sub) == 5 and np.all(np.isfinite(avi.destructure(q_sub)[0]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_new", [1, 17, 65])
def test_forward_against_the_reference(n_new, dtype):
    n, p, hidden, M = MID
    X, y, q = make_data(MID, "bernoulli", "default", dtype)
    prob, rng = avi.BNNProblem(X, y, hidden), np.random.default_rng(n_new)
    ctx = avi.MiviContext(dtype, avi.MEANFIELD, prob.dimension(), M, CF.code, SEED)
    ctx.set_problem(prob)
    Z, Xnew = ctx.sample(avi.destructure(q)[0], 3, want_eps=False), rng.normal(size=(n_new, p)).astype(dtype)
    f = prob.predict(Z, Xnew, ctx).cpu().numpy().astype(np.float64)
    Zh = Z.cpu().numpy().astype(np.float64)
    ref, yard = (np.stack([BNNRef(X, y, hidden, dtype=t).forward(Zh[:, m], Xnew)[0] for m in range(M)]).astype(np.float64) for t in (np.float64, dtype))
    assert f.shape == (M, n_new) and np.linalg.norm(f - ref) <= max(TOL[dtype][1] * max(np.linalg.norm(ref), 1.0), 8 * np.linalg.norm(yard - ref))
    assert np.array_equal(prob.predict(Zh.astype(dtype), Xnew).cpu().numpy(), f.astype(dtype))   # (a context made for the call)
    ctx.close()


def test_creation_errors_and_refusals_by_message():
    n, p, M, d = 8, 3, 4, 4 * 4 + 2 * 5 + 3   # 3 -> 4 -> 2 -> 1
    ctx = avi.MiviContext(np.float32, avi.FULLRANK, d, M, 0, SEED)
    lib, h = ctx.lib, ctx.h
    X, y, nan = np.zeros((n, p), np.float32, order="F"), np.zeros(n, np.float32), float("nan")
    bad = np.array([0, 1, 2, 0, 0, 0, 0, 0], np.float32)
    net = lambda H=2, hid=(4, 2, 0), lik=0, noise=1.0, ps=1.0, la=1.0: _lib.MiviBnn(H, (3 * _lib.C.c_int32)(*hid), lik, noise, ps, la)   # noqa: E731
    for cfg, args, msg in ((net(), (X, y, 0, p), "n must be"), (net(), (X, y, n, 0), r"p must lie in \[1, 64\]"), (net(), (X, y, n, 65), r"p must lie"),
                           (net(H=0), (X, y, n, p), r"n_hidden must lie in \[1, 3\]"), (net(H=4), (X, y, n, p), "n_hidden"),
                           (net(hid=(4, 65, 0)), (X, y, n, p), r"width must lie in \[1, 64\]"), (net(hid=(0, 2, 0)), (X, y, n, p), "width"),
                           (net(hid=(4, 3, 0)), (X, y, n, p), "parameter count, 35"), (net(lik=2), (X, y, n, p), "unknown likelihood"),
                           (net(lik=1, noise=0.0), (X, y, n, p), "noise must be"), (net(noise=nan), (X, y, n, p), "noise"),
                           (net(ps=-1.0), (X, y, n, p), "prior_std must be"), (net(ps=float("inf")), (X, y, n, p), "prior_std"),
                           (net(la=0.0), (X, y, n, p), "likelihood adjustment"), (net(la=nan), (X, y, n, p), "likelihood adjustment"),
                           (net(), (X, bad, n, p), "label is not 0 or 1")):
        assert lib.mivi_set_target_bnn(h, _lib.C.byref(cfg), args[0].ctypes.data, args[1].ctypes.data, *args[2:], 0) == _lib.ERR_BAD_ARG, msg
        assert re.search(msg, lib.mivi_last_error(h).decode()), (msg, lib.mivi_last_error(h))
    assert lib.mivi_set_target_bnn(h, _lib.C.byref(net(lik=1)), X.ctypes.data, bad.ctypes.data, n, p, 0) == 0   # (a Normal's y is any number)
    ctx.set_problem(avi.BNNProblem(X, y, (4, 2)))
    buf, idx = ctx.empty(4 * d * d + 64), np.zeros(2, np.int64)
    P = ctx._p(buf)
    for name, args in {"mivi_gauss_expected_grad_hess2": (P, 0, 0, P, P, P), "mivi_logreg_seek_batch": (0,), "mivi_logreg_select_rows": (idx.ctypes.data, 2, 1.0),
                       "mivi_softmax_select_rows": (idx.ctypes.data, 2, 1.0)}.items():
        assert getattr(lib, name)(h, *args) == _lib.ERR_UNSUPPORTED, name
        assert "Bayesian neural network target" in lib.mivi_last_error(h).decode() and name in lib.mivi_last_error(h).decode()
    for name, refused in (("mivi_optimize_loop_many", lambda: ctx.optimize_loop_many(buf[:2 * ctx.params_len], 2, 2, 0, 0)),
                          ("mivi_optimize_loop_batches", lambda: ctx.optimize_loop_batches(buf, 2, 0, 0)),
                          ("mivi_logreg_set_batch_schedule", lambda: ctx.set_batch_schedule(np.zeros((1, 2), np.int64), likeadj=1.0))):
        with pytest.raises(avi.MiviError, match=name + ".*Bayesian neural network target") as e:
            refused()
        assert e.value.status == _lib.ERR_UNSUPPORTED
    ctx.set_problem(avi.DiagNormalProblem(np.zeros(d, np.float32), np.ones(d, np.float32)))   # replaced cleanly: the entries have no target again
    assert lib.mivi_bnn_select_rows(h, None, 0, 1.0) == _lib.ERR_NO_TARGET and lib.mivi_bnn_forward(h, P, 1, P, 1, P) == _lib.ERR_NO_TARGET
    ctx.close()
