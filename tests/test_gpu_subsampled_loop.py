"""Whole steps of a SubsampledObjective on the device (mivi_optimize_loop_batches, `optimize(..., subsampling=...)`): step t evaluates batch
first_batch + t of the resident schedule and draws at that batch's own estimate index.  Against an INDEPENDENT f64 trajectory on the planned
batches and indices (the oracle gradient on the device's own eps -> the numpy rules of tests/test_gpu_loop_oracle.py), against the
host-driven `step` loop (device_loop=False), and the C ABI of the three entries."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import _lib, subsampling as S
from oracle import oracle as O
from tests.helpers import SEED

OPT = avi._optimize      # (the module: the package exports the function `optimize` under that name)
gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, P, M = 96, 5, 4
D = P + 1
RULES = {"descent": 0, "adam": 1, "dowg": 3}
OPS = {"none": 0, "clip": 1, "prox": 2}
COMBOS = [("descent", "none", "none"), ("adam", "clip", "none"), ("dowg", "prox", "poly")]


def _data(dtype=np.float32):
    rng = np.random.default_rng(21)
    X = (rng.normal(size=(N, P)) / np.sqrt(P)).astype(dtype)
    y = (rng.uniform(size=N) < 0.5).astype(np.uint8)
    return avi.LogRegProblem(X, y, "logsigma_normal", 1.0), O.LogRegTarget(X.astype(np.float64), y, "logsigma_normal", 1.0)


def _q0(family, dtype=np.float32):
    rng = np.random.default_rng(22)
    mu = (0.1 * rng.normal(size=D)).astype(dtype)
    if family == avi.MEANFIELD:
        return avi.MeanFieldGaussian(mu, np.full(D, 0.6, dtype))
    return avi.FullRankGaussian(mu, (0.6 * np.eye(D) + 0.05 * np.tril(rng.normal(size=(D, D)), -1)).astype(dtype))


def _plan(batchsize, n_steps, counter=40):
    sub = avi.ReshufflingBatchSubsampling(np.arange(N), batchsize)
    rng = avi.PhiloxRNG(SEED, counter)
    return S.plan_batches(rng, sub, S.init_subsampling(rng, sub), n_steps)


def _oracle_trajectory(ctx, p0, family, tgt, rows, idx, combo, eta, alpha, clip_eps, avg_eta=8.0):
    """`step` (src/algorithms/common.jl:69-104) in f64, step t on tgt.subsample(rows[t]) with the device's eps of estimate idx[t]"""
    rule, op, avg = combo
    x = p0.astype(np.float64)
    dstate = (x.copy(), 0.0, alpha * (1.0 + float(np.linalg.norm(x))))
    ast = (np.zeros_like(x), np.zeros_like(x))
    xbar, elbos = None, []
    for t in range(len(idx)):
        _, eps = ctx.sample(x.astype(p0.dtype), int(idx[t]))
        ref = O.estimate_gradient(x.astype(p0.dtype).astype(np.float64), D, family, tgt.subsample(rows[t]), eps.cpu().numpy().astype(np.float64), 0)
        elbos.append(-ref["value"])
        g = ref["grad"]
        if rule == "descent":
            x = O.descent_step(x, g, eta)
        elif rule == "adam":
            x, ast = O.adam_step(x, g, ast, t + 1, eta)
        else:
            x, dstate = O.dog_step(x, g, dstate, 1)
        if op == "clip":
            x = O.clip_scale(x, D, family, clip_eps)
        elif op == "prox":
            x = O.proximal_location_scale_entropy(x, D, family, O.stepsize_from_optimizer_state(rule, eta=eta, v=dstate[1], r=dstate[2]))
        if avg == "poly":
            w = (avg_eta + 1.0) / ((t + 1) + avg_eta)
            xbar = x.copy() if xbar is None else (1.0 - w) * xbar + w * x
    return x, xbar, np.array(elbos)


def _device_loop(ctx, p0, combo, T, idx0, first_batch, eta, alpha, clip_eps):
    rule, op, avg = combo
    p = ctx.to_device(p0).clone()
    st = None
    if rule == "adam":
        st = ctx.empty(2 * p.numel()).zero_()
    elif rule == "dowg":
        st = ctx.dog_state()
        ctx.dog_init(p, st, alpha)
    ap = p.clone() if avg == "poly" else None
    elbo = ctx.empty(T)
    ctx.optimize_loop_batches(p, T, idx0, 0, first_batch=first_batch, rule=RULES[rule], op=OPS[op], averager=1 if avg == "poly" else 0, eta=eta,
                              clip_epsilon=clip_eps, opt_state=st, avg_params=ap, elbo=elbo)
    ctx.synchronize()
    return p.cpu().numpy().astype(np.float64), (ap.cpu().numpy().astype(np.float64) if ap is not None else None), elbo.cpu().numpy().astype(np.float64)


def _check(got, want, family, combo, tol=5e-6):
    """tests/test_gpu_loop_oracle.py::_check's criterion"""
    (g, gbar, gel), (x, xbar, el) = got, want
    low = np.ones(g.size, bool) if family == avi.MEANFIELD else np.concatenate([np.ones(D, bool), np.tril(np.ones((D, D), bool)).T.reshape(-1)])
    assert np.max(np.abs(g[low] - x[low])) <= tol * max(1.0, np.max(np.abs(x))), (combo, np.max(np.abs(g[low] - x[low])))
    if xbar is not None:
        assert np.max(np.abs(gbar[low] - xbar[low])) <= tol * max(1.0, np.max(np.abs(xbar))), combo
    assert np.allclose(gel, el, rtol=2e-5, atol=1e-4), (combo, gel, el)


@gpu
@pytest.mark.parametrize("combo", COMBOS, ids=["-".join(c) for c in COMBOS])
@pytest.mark.parametrize("family", [avi.MEANFIELD, avi.FULLRANK], ids=["meanfield", "fullrank"])
@pytest.mark.parametrize("kernels", [1, 2])
def test_the_loop_over_batches_follows_the_oracle(kernels, family, combo):
    """T = 3 steps from batch 0, and three steps from another first batch: with batchsize = 20 the steps 3, 4, 5 cross the end of the
    epoch, where the short trailing batch is replaced by the first batch of the next shuffle."""
    prob, tgt = _data()
    p0, _ = avi.destructure(_q0(family))
    ctx = avi.MiviContext(np.float32, family, D, M, 0, SEED)
    ctx.set_problem(prob)
    for batchsize, first in ((16, 0), (20, 3)):
        rows, idx, infos, _ = _plan(batchsize, 8)
        assert rows.shape == (8, batchsize)
        ctx.set_batch_schedule(rows, idx, kernels=kernels)
        assert ctx.batch_route() == kernels              # which route runs (mivi_logreg_kernels)
        want = _oracle_trajectory(ctx, p0, family, tgt, rows[first:first + 3], idx[first:first + 3], combo, 1e-3, 1e-2, 1e-5)
        got = _device_loop(ctx, p0, combo, 3, 12345, first, 1e-3, 1e-2, 1e-5)    # (idx0 is not read: the schedule carries the indices)
        _check(got, want, family, combo)
    if batchsize == 20:
        assert infos[4]["epoch"] == 2 and infos[4]["step"] == 1 and infos[3]["epoch"] == 1
    # a schedule without indices: step t draws at estimate_idx0 + t
    ctx.set_batch_schedule(rows, None, kernels=kernels)
    want = _oracle_trajectory(ctx, p0, family, tgt, rows[1:4], np.arange(70, 73), combo, 1e-3, 1e-2, 1e-5)
    got = _device_loop(ctx, p0, combo, 3, 70, 1, 1e-3, 1e-2, 1e-5)
    _check(got, want, family, combo)
    ctx.close()


@gpu
@pytest.mark.parametrize("family", [avi.MEANFIELD, avi.FULLRANK], ids=["meanfield", "fullrank"])
def test_plain_loop_on_a_scheduled_context_evaluates_the_selected_batch(family):
    """mivi_optimize_loop (not _batches) on a scheduled context: every step on the batch seek_batch selected -- never the whole-loop kernel
    of the small logistic regressions, whose route test must see the schedule (this shape is one it takes without one)."""
    prob, tgt = _data()
    p0, _ = avi.destructure(_q0(family))
    ctx = avi.MiviContext(np.float32, family, D, M, 0, SEED)
    ctx.set_problem(prob)
    rows, idx, _, _ = _plan(16, 4)
    ctx.set_batch_schedule(rows, idx, kernels=1)
    ctx.seek_batch(2)
    combo = ("descent", "none", "none")
    want = _oracle_trajectory(ctx, p0, family, tgt, np.stack([rows[2]] * 3), np.arange(70, 73), combo, 1e-3, 1e-2, 1e-5)
    p = ctx.to_device(p0).clone()
    elbo = ctx.empty(3)
    n_rec = ctx.graph_recordings()
    ctx.optimize_loop(p, 3, 70, 0, rule=0, eta=1e-3, elbo=elbo)
    ctx.synchronize()
    assert ctx.graph_recordings() == n_rec + 1          # the graph of launches
    _check((p.cpu().numpy().astype(np.float64), None, elbo.cpu().numpy().astype(np.float64)), want, family, combo)
    ctx.close()


def _same_sub_state(a, b):
    return (a.epoch == b.epoch and len(a.batches) == len(b.batches) and
            all(sa == sb and np.array_equal(ba, bb) for (sa, ba), (sb, bb) in zip(a.batches, b.batches)))


@gpu
@pytest.mark.parametrize("batchsize", [16, 20])
@pytest.mark.parametrize("family", [avi.MEANFIELD, avi.FULLRANK], ids=["meanfield", "fullrank"])
@pytest.mark.parametrize("kernels", [2, 1, 0])
def test_optimize_with_subsampling_runs_on_the_device_and_equals_the_host_loop(kernels, family, batchsize, monkeypatch):
    """2.5 epochs in chunks of four steps, then a warm start from the returned state: the device loop and the host-driven `step` loop
    (mivi_logreg_select_rows + the single entries) give the same parameters -- bitwise with the device gather forced (the same kernels on
    the same gathered rows), to the loop criterion with the fused minibatch kernel -- the same (epoch, step, iteration) infos, and leave
    the rng counter and the subsampling state equal."""
    monkeypatch.setattr(OPT, "DEVICE_LOOP_CHUNK", 4)
    monkeypatch.setattr(OPT, "SUBSAMPLED_KERNELS", kernels)
    prob, _ = _data()
    q0 = _q0(family)
    sub = avi.ReshufflingBatchSubsampling(np.arange(N), batchsize)
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), n_samples=M, optimizer=avi.Adam(1e-2), operator=avi.ClipScale(), averager=avi.PolynomialAveraging(),
                                  subsampling=sub)
    steps = int(2.5 * (N // batchsize))
    runs = []
    for dev in (True, False):
        rng = avi.PhiloxRNG(SEED)
        q1, i1, st = avi.optimize(rng, alg, steps, prob, q0, device_loop=dev)
        ctx = OPT._ctx_of(st["obj_st"])
        if dev:
            assert ctx.batch_route() == (kernels or 1)      # (by size: the fused kernel at this shape)
            assert ctx.graph_recordings() <= 2              # chunks of 4, 4, ... and one shorter: the schedule is replaced in place
        c1, s1 = rng.counter, st["obj_st"].sub_st
        q2, i2, st2 = avi.optimize(rng, alg, 7, prob, None, state=st, device_loop=dev)
        runs.append((q1, i1, c1, s1, q2, i2, rng.counter, st2["obj_st"].sub_st, st2["iteration"]))
        ctx.close()
    a, b = runs
    assert a[2] == b[2] and a[6] == b[6] and a[8] == b[8] == steps + 7
    assert _same_sub_state(a[3], b[3]) and _same_sub_state(a[7], b[7])
    for ia, ib in ((a[1], b[1]), (a[5], b[5])):
        assert [(x["epoch"], x["step"], x["iteration"]) for x in ia] == [(x["epoch"], x["step"], x["iteration"]) for x in ib]
        assert [x["iteration"] for x in ia] == list(range(1, len(ia) + 1))
    for qa, qb, ia, ib in ((a[0], b[0], a[1], b[1]), (a[4], b[4], a[5], b[5])):
        ea, eb = np.array([float(x["elbo"]) for x in ia]), np.array([float(x["elbo"]) for x in ib])
        la, lb, sa, sb = qa.location, qb.location, np.asarray(qa.scale), np.asarray(qb.scale)
        if kernels == 2:
            assert np.array_equal(la, lb) and np.array_equal(sa, sb) and np.array_equal(ea, eb)
        else:
            top = max(1.0, np.max(np.abs(lb)), np.max(np.abs(sb)))
            assert np.max(np.abs(la - lb)) <= 5e-6 * top and np.max(np.abs(sa - sb)) <= 5e-6 * top
            assert np.allclose(ea, eb, rtol=2e-5, atol=1e-4)


@gpu
@pytest.mark.parametrize("kernels", [2, 1])
def test_a_transformed_logreg_with_subsampling_runs_on_the_device(kernels, monkeypatch):
    """The data behind a TransformedProblem (a Stacked bijector around the logistic regression: the explicit-sample route around the same
    target launch): `subsample` forwards to the wrapped problem, and the device loop equals the host-driven one."""
    monkeypatch.setattr(OPT, "SUBSAMPLED_KERNELS", kernels)
    prob, _ = _data()
    tp = avi.TransformedProblem(prob, avi.StackedBijector([(0, P, "identity"), (P, D, "exp")]))
    sub_tp = avi.subsample(tp, [3, 1])
    assert isinstance(sub_tp, avi.TransformedProblem) and isinstance(sub_tp.prob, avi.LogRegSubset) and sub_tp.bijector is tp.bijector
    sub = avi.ReshufflingBatchSubsampling(np.arange(N), 16)
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), n_samples=M, optimizer=avi.Adam(1e-2), operator=avi.ClipScale(), averager=avi.NoAveraging(), subsampling=sub)
    out = []
    for dev in (True, False):
        q, info, st = avi.optimize(avi.PhiloxRNG(SEED), alg, 8, tp, _q0(avi.MEANFIELD), device_loop=dev)
        ctx = OPT._ctx_of(st["obj_st"])
        assert ctx.batch_route() == (kernels if dev else 0)
        ctx.close()
        out.append((q.location, np.asarray(q.scale), np.array([float(i["elbo"]) for i in info]), [(i["epoch"], i["step"]) for i in info]))
    (la, sa, ea, fa), (lb, sb, eb, fb) = out
    assert fa == fb
    if kernels == 2:
        assert np.array_equal(la, lb) and np.array_equal(sa, sb) and np.array_equal(ea, eb)
    else:
        top = max(1.0, np.max(np.abs(lb)), np.max(np.abs(sb)))
        assert np.max(np.abs(la - lb)) <= 5e-6 * top and np.max(np.abs(sa - sb)) <= 5e-6 * top and np.allclose(ea, eb, rtol=2e-5, atol=1e-4)


@gpu
def test_what_keeps_the_host_loop():
    """device_loop=False, a callback and a plugin model take the host-driven loop as before (no schedule is ever set)."""
    prob, tgt = _data()
    sub = avi.ReshufflingBatchSubsampling(np.arange(N), 16)
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), n_samples=M, optimizer=avi.Adam(1e-2), operator=avi.ClipScale(), subsampling=sub)
    assert OPT._device_loop_codes(alg, None, (), prob) is not None
    assert OPT._device_loop_codes(alg, None, (), avi.TransformedProblem(prob, avi.StackedBijector([(0, P, "identity"), (P, D, "exp")]))) is not None
    assert OPT._device_loop_codes(alg, lambda **kw: None, (), prob) is None
    assert OPT._device_loop_codes(alg, None, (), avi.DiagNormalProblem(np.zeros(D), np.ones(D))) is None
    seen = []
    _, info, st = avi.optimize(avi.PhiloxRNG(SEED), alg, 3, prob, _q0(avi.MEANFIELD), callback=lambda **kw: seen.append(kw["iteration"]))
    ctx = OPT._ctx_of(st["obj_st"])
    assert seen == [1, 2, 3] and ctx.batch_route() == 0 and info[-1]["epoch"] == 1
    ctx.close()


def test_the_three_entries_are_exported_and_bound_with_the_headers_signatures(lib):
    """In the manner of tests/test_abi_and_host.py: declared in include/mivi.h, exported by libmivi.so, bound in _lib.SIGNATURES with the
    header's parameter classes; the schedule struct has the header's layout."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mivi.h")).read(), flags=re.S)
    want = {"mivi_logreg_set_batch_schedule": ["ptr", "ptr"], "mivi_logreg_seek_batch": ["ptr", "i32"],
            "mivi_optimize_loop_batches": ["ptr", "ptr", "ptr", "i32"]}
    cls = {C.c_void_p: "ptr", C.c_int32: "i32", C.c_int64: "i64", C.c_uint64: "u64", C.c_double: "f64"}
    for name, params in want.items():
        m = re.search(r"mivi_status_t\s+" + name + r"\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in include/mivi.h"
        decl = ["ptr" if "*" in a else ("i32" if "int32_t" in a else "?") for a in m.group(1).split(",")]
        assert decl == params, (name, decl)
        assert hasattr(lib, name), f"libmivi.so does not export {name}"
        res, args = _lib.SIGNATURES[name]
        assert cls[res] == "i32" and [cls[a] for a in args] == params, name
    body = re.search(r"typedef struct mivi_batch_schedule \{(.*?)\} mivi_batch_schedule_t;", src, flags=re.S).group(1)
    fields = [re.sub(r"\s+", " ", f).strip() for f in body.split(";") if f.strip()]
    assert [f.split()[-1].lstrip("*") for f in fields] == [n for n, _ in _lib.MiviBatchSchedule._fields_]
    kinds = ["ptr" if "*" in f else {"int64_t": "i64", "int32_t": "i32", "double": "f64"}[f.split()[0]] for f in fields]
    assert kinds == [cls[t] for _, t in _lib.MiviBatchSchedule._fields_]
    assert C.sizeof(_lib.MiviBatchSchedule) == 40 and _lib.MiviBatchSchedule.likeadj.offset == 32
