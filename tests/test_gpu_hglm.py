"""The hierarchical GLM target (mivi_set_target_hglm, csrc/kernels_hglm.hip) on the library's own draws against the float64 oracle with
tests/hglm_ref.py as the target: bound = max(TOL x scale, 8 x |the restatement in the context's dtype - float64|) on the value, the whole
gradient, and the beta block, the u block and the s entry each alone (the criterion of tests/test_gpu_softmax.py and test_gpu_bnn.py).  The
other routes are held to the SAME model as a host plugin on one context, by the same bound.  DESIGN.md section 8."""
import re

import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import _lib
from oracle import oracle as O
from tests.helpers import SEED, OraclePlugin
from tests.hglm_ref import LOG2PI, HierGLMRef
from tests.test_gpu_blockdiag import TOL
from tests.test_gpu_softmax import _family

gpu = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
LIKS = ["bernoulli", "poisson"]
CF, STL = avi.ClosedFormEntropy(), avi.StickingTheLandingEntropy()
MID = (100, 7, 12, 7)   # (n, p, J, M)
# one row, one group; partial row and sample tiles with several groups inside one tile; p and M past one tile with groups straddling the
# row tiles; J > n (no rows for groups 0, 1, J - 2, J - 1 and most of the middle); p at its limit (two waves per workgroup in f64) with
# singleton groups; two sample groups of 64; and 1000 rows: ceil(1000 / 256) = 4 slices of 256 rows (an f32 flush every 128) with the
# sizes below for groups 0 .. 7 -- group 1 (ordered rows 100 .. 599) covers slice 1 and both neighbours' edges, group 3 starts on row 768 = 3 x 256
SHAPES = [(1, 1, 1, 1), (17, 3, 4, 5), (70, 17, 3, 17), (20, 2, 50, 3), (40, 256, 40, 2), (33, 5, 2, 70), (1000, 5, 8, 3)]
SIZES = {(1000, 8): [100, 500, 168, 32, 50, 0, 150, 0]}


def make_data(shape, lik, kind, dtype):
    n, p, J, M = shape
    rng = np.random.default_rng(1000 * n + 10 * p + J)
    X = (rng.normal(size=(n, p)) / np.sqrt(p)).astype(dtype)
    if (n, J) in SIZES:
        groups = np.repeat(np.arange(J), SIZES[n, J])   # (sizes by group id: the kernel walks the rows in id order)
    else:
        groups = rng.permutation(J) if J == n else rng.integers(2, J - 2, size=n) if J > n else rng.integers(0, J, size=n)
    groups = rng.permutation(groups).astype(np.int32)   # (ids in no order)
    offset = None if lik == "bernoulli" and kind == "default" else rng.normal(size=n).astype(dtype)
    loc, scale = np.r_[rng.normal(size=p) * 0.7, rng.normal(size=J) * 0.5, 0.2], rng.uniform(0.3, 0.9, size=p + J + 1)
    if kind == "saturated":   # at the location |eta| reaches about 30 (Bernoulli: sigma saturates) / eta about 15 (Poisson: counts to 3 x 10^6)
        X = (X * ((28.0 if lik == "bernoulli" else 12.0) / np.abs(X.astype(np.float64) @ loc[:p]).max())).astype(dtype)
        scale = scale * 0.02
    eta = X.astype(np.float64) @ loc[:p] + loc[p:p + J][groups] + (0 if offset is None else offset)
    y = (rng.integers(0, 2, size=n) if lik == "bernoulli" else rng.poisson(np.exp(eta))).astype(dtype)
    assert np.array_equal(y.astype(np.float32), y.astype(np.float64))   # exactly representable in f32
    return X, y, groups, offset, avi.MeanFieldGaussian(loc.astype(dtype), scale.astype(dtype))


def check(value, grad, params, ref_tgt, yard_tgt, eps, ent, dtype, tag):
    d, p = ref_tgt.dimension(), ref_tgt.X.shape[1]
    ref, yard = (O.estimate_gradient(params.astype(np.float64), d, O.MEANFIELD, t, eps, ent.code) for t in (ref_tgt, yard_tgt))
    _, vt, gt = TOL[dtype]
    rg, yg = ref["grad"], yard["grad"]
    assert np.isfinite(ref["value"]) and np.all(np.isfinite(rg)) and np.isfinite(value) and np.all(np.isfinite(grad))
    bound = lambda ix, scale: max(gt * scale, 8 * np.linalg.norm(yg[ix] - rg[ix]))   # noqa: E731
    ratios = {"value": abs(value - ref["value"]) / max(vt * abs(ref["value"]), 8 * abs(yard["value"] - ref["value"])),
              "whole": np.linalg.norm(grad - rg) / bound(slice(None), max(np.linalg.norm(rg), 1.0))}
    floor = np.linalg.norm(rg) / np.sqrt(3)
    for name, ix in (("beta", np.r_[0:p]), ("u", np.r_[p:d - 1]), ("s", np.r_[d - 1:d])):   # (the location gradient's blocks)
        ratios[name] = np.linalg.norm(grad[ix] - rg[ix]) / bound(ix, max(np.linalg.norm(rg[ix]), floor))
    worst = max(ratios, key=ratios.get)
    print(f"[hglm] {tag} {np.dtype(dtype).name} ent{ent.code}: value {ratios['value']:.3f} whole {ratios['whole']:.3f} worst {worst} {ratios[worst]:.3f}")
    assert ratios[worst] <= 1.0, ratios


def run_case(shape, lik, kind, ent, dtype, likeadj=1.0, rows=None, cap=0):
    n, p, J, M = shape
    X, y, groups, offset, q = make_data(shape, lik, kind, dtype)
    kw = dict(likelihood=lik, prior_std=1.3, tau_scale=0.8)
    prob = avi.HierGLMProblem(X, y, groups, J, offset=offset, likeadj=likeadj, **kw)
    params = avi.destructure(q)[0]
    ctx = avi.MiviContext(dtype, avi.MEANFIELD, prob.dimension(), M, ent.code, SEED)
    ctx.set_problem(prob if rows is None else prob.subsample(rows))
    if cap:
        ctx.hglm_set_part_cap(cap)
    eps = ctx.sample(params, 3)[1].cpu().numpy().astype(np.float64)
    value, grad = ctx.estimate_gradient(params, 3)
    ctx.synchronize()
    sel = slice(None) if rows is None else np.asarray(rows)
    la = likeadj if rows is None else likeadj * n / len(rows)
    tgts = [HierGLMRef(X[sel], y[sel], groups[sel], J, offset=None if offset is None else offset[sel], likeadj=la, dtype=t, **kw) for t in (np.float64, dtype)]
    check(float(value.item()), grad.cpu().numpy().astype(np.float64), params, *tgts, eps, ent, dtype, f"{shape} {lik} {kind}")
    return ctx, prob, params, value.clone(), grad.clone()


@pytest.mark.parametrize("lik", LIKS)
def test_reference_gradient_is_autograd_of_its_value(lik):
    n, p, J, rng = 23, 4, 6, np.random.default_rng(5)
    groups = rng.integers(1, J - 2, size=n)   # groups 0, J - 2 and J - 1 have no rows
    y = rng.integers(0, 2, size=n) if lik == "bernoulli" else rng.poisson(2.0, size=n)
    ref = HierGLMRef(rng.normal(size=(n, p)), y, groups, J, lik, rng.normal(size=n), prior_std=1.3, tau_scale=0.8, likeadj=2.5)
    prob = avi.HierGLMProblem(ref.X, ref.y, groups, J, lik, ref.offset, 1.3, 0.8, 2.5)
    z = torch.tensor(rng.normal(size=p + J + 1) * 0.5, dtype=torch.float64, requires_grad=True)
    beta, u, s = z[:p], z[p:p + J], z[p + J]
    eta, yt = torch.tensor(ref.X) @ beta + u[torch.tensor(groups)] + torch.tensor(ref.offset), torch.tensor(ref.y)
    ll = (yt * eta - torch.nn.functional.softplus(eta)).sum() if lik == "bernoulli" else (yt * eta - eta.exp() - torch.lgamma(yt + 1)).sum()
    val = (2.5 * ll - 0.5 * (beta * beta).sum() / 1.3 ** 2 - p * (np.log(1.3) + 0.5 * LOG2PI) - 0.5 * (u * u).sum() * (-2 * s).exp() - J * (s + 0.5 * LOG2PI)
           + np.log(2.0) - 0.5 * LOG2PI - np.log(0.8) - (2 * s).exp() / (2 * 0.8 ** 2) + s)
    val.backward()
    v, g = ref.logdensity_and_gradient(z.detach().numpy())
    assert prob.dimension() == ref.dimension() == p + J + 1 and [np.size(b) for b in prob.unpack(g)] == [p, J, 1]
    assert v == pytest.approx(val.item(), rel=1e-13) and np.allclose(g, z.grad.numpy(), rtol=1e-11, atol=1e-12)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ent", [CF, STL], ids=["cf", "stl"])
@pytest.mark.parametrize("lik", LIKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes(shape, lik, ent, dtype):
    run_case(shape, lik, "default", ent, dtype)[0].close()


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lik", LIKS)
@pytest.mark.parametrize("kind", ["default", "saturated"])
def test_data_classes(kind, lik, dtype):
    run_case(MID, lik, kind, STL, dtype)[0].close()


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kw", [dict(likeadj=7.5), dict(rows=[5, 99, 5, 0, 42, 42, 64, 63, 17])], ids=["likeadj", "rows"])
def test_likeadj_and_row_subset(kw, dtype):
    ctx, prob, params, v, g = run_case(MID, "poisson", "default", STL, dtype, **kw)
    if "rows" in kw:   # (nine rows, twelve groups: some have none.)  A failed call leaves the selection in force unchanged
        with pytest.raises(avi.MiviError, match="out of range"):
            ctx.set_problem(prob.subsample([0, 100]))
        assert torch.equal(ctx.estimate_gradient(params, 3)[1], g)
        ctx.set_problem(prob)   # b = 0: back to the full set, bitwise what a fresh context gives
        full = run_case(MID, "poisson", "default", STL, dtype)
        v0, g0 = ctx.estimate_gradient(params, 3)
        assert torch.equal(v0, full[3]) and torch.equal(g0, full[4]) and not torch.equal(g0, g)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_bitwise_repeat_device_data_and_part_cap(dtype):
    n, p, J, M = MID
    ctx, prob, params, v, g = run_case(MID, "poisson", "default", CF, dtype)
    assert all(torch.equal(a, b) for a, b in zip(ctx.estimate_gradient(params, 3), (v, g)))
    X, y, groups, offset, _ = make_data(MID, "poisson", "default", dtype)
    # device-resident data is read through the group ordering that host data is STORED in: the same values in the same order, so bitwise
    dev = avi.HierGLMProblem(torch.as_tensor(np.ascontiguousarray(X.T)).cuda(), torch.as_tensor(y).cuda(), groups, J, "poisson",
                             torch.as_tensor(offset).cuda(), prior_std=1.3, tau_scale=0.8)
    ctx.set_problem(dev)   # (p, n) contiguous = n x p column-major
    assert all(torch.equal(a, b) for a, b in zip(ctx.estimate_gradient(params, 3), (v, g)))
    capped = run_case(MID, "poisson", "default", CF, dtype, cap=3 * (p + 3 + J) * 8)   # one slice: chunks of 3, 3 and 1 samples
    assert torch.equal(capped[3], v) and torch.equal(capped[4], g)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route", ["fullrank", "lowrank", "blockdiag", "realnvp", "exp", "objective", "score"])
def test_routes_equal_the_same_model_as_a_plugin(route, dtype):
    """One context; the built-in target, then OraclePlugin(HierGLMRef) in float64 (the reference) and in the context's dtype (the restatement)."""
    (n, p, J, M), (X, y, groups, offset, _) = MID, make_data(MID, "poisson", "default", dtype)
    d = p + J + 1
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

    got = run(avi.HierGLMProblem(X, y, groups, J, "poisson", offset))
    ref, yard = (run(OraclePlugin(HierGLMRef(X, y, groups, J, "poisson", offset, dtype=t))) for t in (np.float64, dtype))
    ctx.close()
    _, vt, gt = TOL[dtype]
    for k, (a, r, w) in enumerate(zip(got, ref, yard)):
        tol, scale = (vt, np.linalg.norm(r)) if a.size == 1 else (gt, max(np.linalg.norm(r), 1.0))
        ratio = np.linalg.norm(a - r) / max(tol * scale, 8 * np.linalg.norm(w - r))
        print(f"[hglm] route {route} {np.dtype(dtype).name} output {k}: ratio {ratio:.3f}")
        assert np.all(np.isfinite(a)) and ratio <= 1.0, (route, k, ratio)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_device_loop_equals_host_loop_and_subsampled_steps(dtype):
    n, p, J, M = MID
    X, y, groups, offset, q = make_data(MID, "bernoulli", "default", dtype)
    q0 = avi.MeanFieldGaussian(dtype(0.1) * q.location, np.full(len(q.location), 0.1, dtype))
    prob = avi.HierGLMProblem(X, y, groups, J)
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), optimizer=avi.Adam(1e-2), n_samples=M, operator=avi.ClipScale())
    q_dev, info_dev, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 5, prob, q0)
    q_host, info_host, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 5, prob, q0, device_loop=False)
    assert np.array_equal(avi.destructure(q_dev)[0], avi.destructure(q_host)[0]) and [i["elbo"] for i in info_dev] == [i["elbo"] for i in info_host]
    assert not np.array_equal(avi.destructure(q_dev)[0], avi.destructure(q0)[0])
    sub = avi.KLMinRepGradDescent(avi.AutoMIVI(), optimizer=avi.Adam(1e-2), n_samples=M, operator=avi.ClipScale(),
                                  subsampling=avi.ReshufflingBatchSubsampling(np.arange(n), 32))
    q_sub, info_sub, state = avi.optimize(avi.PhiloxRNG(SEED), sub, 5, prob, q0)
    assert "mivi_hglm_select_rows" in state["route_note"] and len(info_sub) == 5 and np.all(np.isfinite(avi.destructure(q_sub)[0]))


@gpu
def test_creation_errors_and_refusals_by_message():
    n, p, J, M = 8, 3, 7, 4
    d = p + J + 1   # 11: also the d of a 3 -> 2 -> 1 network and of a softmax regression with p = 5, C = 2
    ctx = avi.MiviContext(np.float32, avi.FULLRANK, d, M, 0, SEED)
    lib, h = ctx.lib, ctx.h
    X, y, grp, nan = np.zeros((n, p), np.float32, order="F"), np.zeros(n, np.float32), np.arange(n, dtype=np.int32) % J, float("nan")
    y2, yneg, yhalf, gbad = y + np.float32(2) * (np.arange(n) == 1), y - (np.arange(n) == 2), y + np.float32(0.5), grp + J * (np.arange(n, dtype=np.int32) == 3)
    model = lambda lik=0, J=J, ps=1.0, ts=1.0, la=1.0: _lib.MiviHglm(lik, J, ps, ts, la)   # noqa: E731
    for cfg, (yv, gv, nv, pv), msg in ((model(), (y, grp, 0, p), "n must be"), (model(), (y, grp, n, 0), r"p must lie in \[1, 256\]"), (model(), (y, grp, n, 257), "p must lie"),
                                       (model(J=0), (y, grp, n, p), "n_groups must be"), (model(J=5), (y, grp, n, p), r"p \+ n_groups \+ 1, 9"),
                                       (model(), (y, gbad, n, p), "group id lies outside"), (model(), (y, -grp - 1, n, p), "group id"),
                                       (model(lik=2), (y, grp, n, p), "unknown likelihood"), (model(ps=0.0), (y, grp, n, p), "prior_std must be"),
                                       (model(ps=nan), (y, grp, n, p), "prior_std"), (model(ts=-1.0), (y, grp, n, p), "tau_scale must be"),
                                       (model(ts=float("inf")), (y, grp, n, p), "tau_scale"), (model(la=0.0), (y, grp, n, p), "likelihood adjustment"),
                                       (model(la=nan), (y, grp, n, p), "likelihood adjustment"), (model(), (y2, grp, n, p), "label is not 0 or 1"),
                                       (model(lik=1), (yneg, grp, n, p), "negative or not an integer"), (model(lik=1), (yhalf, grp, n, p), "not an integer")):
        gv = np.ascontiguousarray(gv, dtype=np.int32)
        assert lib.mivi_set_target_hglm(h, _lib.C.byref(cfg), X.ctypes.data, yv.ctypes.data, None, gv.ctypes.data, nv, pv, 0) == _lib.ERR_BAD_ARG, msg
        assert re.search(msg, lib.mivi_last_error(h).decode()), (msg, lib.mivi_last_error(h))
    assert lib.mivi_set_target_hglm(h, _lib.C.byref(model(lik=1)), X.ctypes.data, y2.ctypes.data, None, grp.ctypes.data, n, p, 0) == 0   # (a count of 2)
    ctx.set_problem(avi.HierGLMProblem(X, y, grp, J))
    buf, idx = ctx.empty(4 * d * d + 64), np.zeros(2, np.int64)
    P = ctx._p(buf)
    for name, args in {"mivi_gauss_expected_grad_hess2": (P, 0, 0, P, P, P), "mivi_logreg_seek_batch": (0,), "mivi_logreg_select_rows": (idx.ctypes.data, 2, 1.0),
                       "mivi_softmax_select_rows": (idx.ctypes.data, 2, 1.0), "mivi_bnn_select_rows": (idx.ctypes.data, 2, 1.0)}.items():
        assert getattr(lib, name)(h, *args) == _lib.ERR_UNSUPPORTED, name
        assert "hierarchical GLM target" in lib.mivi_last_error(h).decode() and name in lib.mivi_last_error(h).decode()
    for name, refused in (("mivi_optimize_loop_many", lambda: ctx.optimize_loop_many(buf[:2 * ctx.params_len], 2, 2, 0, 0)),
                          ("mivi_optimize_loop_batches", lambda: ctx.optimize_loop_batches(buf, 2, 0, 0)),
                          ("mivi_logreg_set_batch_schedule", lambda: ctx.set_batch_schedule(np.zeros((1, 2), np.int64), likeadj=1.0))):
        with pytest.raises(avi.MiviError, match=name + ".*hierarchical GLM target") as e:
            refused()
        assert e.value.status == _lib.ERR_UNSUPPORTED
    for other, words in ((avi.BNNProblem(X, y, (2,)), "Bayesian neural network target"),   # the other targets' contexts refuse the entry, by name
                         (avi.SoftmaxRegProblem(np.zeros((n, 5), np.float32), np.zeros(n, np.uint8), 2), "softmax regression target")):
        ctx.set_problem(other)
        assert lib.mivi_hglm_select_rows(h, idx.ctypes.data, 2, 1.0) == _lib.ERR_UNSUPPORTED
        assert "mivi_hglm_select_rows" in lib.mivi_last_error(h).decode() and words in lib.mivi_last_error(h).decode()
    ctx.set_problem(avi.DiagNormalProblem(np.zeros(d, np.float32), np.ones(d, np.float32)))   # replaced cleanly: the entry has no target again
    assert lib.mivi_hglm_select_rows(h, None, 0, 1.0) == _lib.ERR_NO_TARGET
    ctx.close()
