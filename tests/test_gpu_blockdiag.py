"""The block-diagonal family (MIVI_BLOCKDIAG) against the float64 FULL-RANK oracle on the dense embedding of the blocks, on the library's own
draws, by the criterion of tests/test_gpu_lowrank.py (TOL; code >= 2: at least 8 x `yardstick`), whole vector and per block.  DESIGN.md section 8."""
import ctypes as C

import numpy as np
import pytest

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import _lib
from oracle import oracle as O
from tests.helpers import SEED, OraclePlugin, make_problem, rel_err

pytestmark = pytest.mark.gpu

TOL = {np.float32: (1e-6, 1e-5, 2e-5), np.float64: (1e-14, 1e-12, 1e-11)}   # samples, value, gradient
ENTROPIES = [avi.ClosedFormEntropy(), avi.ClosedFormEntropyZeroGradient(), avi.MonteCarloEntropy(), avi.StickingTheLandingEntropy(), avi.StickingTheLandingEntropyZeroGradient()]
SHAPES = [(7, 1, 3), (10, 2, 1), (10, 16, 7), (48, 16, 16), (50, 17, 33), (100, 40, 20), (130, 64, 70), (256, 32, 1040), (4099, 5, 17)]
DTYPES = [np.float32, np.float64]
DIRECT = {0: 1.0, 1: 0.0, 2: 1.0, 3: 0.0, 4: -1.0}


def make_bd(rng, d, b, dtype):
    blocks = []
    for lo, bk, _ in avi.blockdiag_layout(d, b)[0]:
        B = np.tril(rng.normal(size=(bk, bk)) * (0.3 / np.sqrt(bk)))
        B[np.diag_indices(bk)] = rng.uniform(0.5, 1.5, size=bk)
        blocks.append(B)
    return avi.BlockDiagGaussian(rng.normal(size=d).astype(dtype), blocks)


def embed(params, d, b):   # [mu; vec C] of the dense d x d scale that carries the blocks (float64)
    C_ = np.zeros((d, d))
    for lo, bk, off in avi.blockdiag_layout(d, b)[0]:
        C_[lo:lo + bk, lo:lo + bk] = np.tril(params[off:off + bk * bk].astype(np.float64).reshape(bk, bk, order="F"))
    return np.concatenate([params[:d].astype(np.float64), C_.reshape(-1, order="F")])


def extract(dense, d, b):   # the block entries of a dense [dmu; vec dC] in the family's layout
    G = dense[d:].reshape(d, d, order="F")
    return np.concatenate([dense[:d]] + [G[lo:lo + bk, lo:lo + bk].reshape(-1, order="F") for lo, bk, _ in avi.blockdiag_layout(d, b)[0]])


def yardstick(params, d, b, G, ell, eps, kind, dtype):   # the estimate's expressions block by block, every array and sum in `dtype`
    T = np.dtype(dtype).type
    p, G, eps, M = params.astype(dtype), G.astype(dtype), eps.astype(dtype), eps.shape[1]
    grad, logdet = np.zeros_like(p), T(0)
    grad[:d] = -G.sum(axis=1) / T(M)
    for lo, bk, off in avi.blockdiag_layout(d, b)[0]:
        Ck = np.tril(p[off:off + bk * bk].reshape(bk, bk, order="F"))
        W = G[lo:lo + bk] + (np.linalg.solve(Ck.T, eps[lo:lo + bk]).astype(dtype) if kind >= 3 else T(0))
        dC = -np.tril(W @ eps[lo:lo + bk].T) / T(M) - T(DIRECT[kind]) * np.diag(T(1) / np.diagonal(Ck))
        grad[off:off + bk * bk] = dC.reshape(-1, order="F")
        logdet += np.log(np.diagonal(Ck)).sum(dtype=dtype)
    ent = T(0.5 * d * (1 + np.log(2 * np.pi))) if kind < 2 else (T(0.5) * (eps * eps).sum(dtype=dtype) / T(M) + T(0.5 * d * np.log(2 * np.pi)))
    return float(-(ell.astype(dtype).sum(dtype=dtype) / T(M) + ent + logdet)), grad.astype(np.float64)


def run_case(d, b, M, kind, ent, dtype, idx=3, plugin=False, bijector=False):
    rng = np.random.default_rng(99 + d + 7 * M + 13 * b)
    q = make_bd(rng, d, b, dtype)
    prob, tgt = make_problem(rng, kind, d, dtype)
    prob = OraclePlugin(tgt) if plugin else prob
    if bijector:
        blocks = [(0, 3, "exp"), (3, d, "identity")]
        prob, tgt = avi.TransformedProblem(prob, avi.StackedBijector(blocks)), O.StackedBijectorTarget(tgt, blocks)
    params, (layout, plen) = avi.destructure(q)[0], avi.blockdiag_layout(d, b)
    ctx = avi.MiviContext(dtype, avi.BLOCKDIAG, d, M, ent.code, SEED, block=b)
    ctx.set_problem(prob)
    assert ctx.params_len == plen == params.shape[0] and ctx.partials_len == 0
    Z, eps = (t.cpu().numpy().astype(np.float64) for t in ctx.sample(params, idx))
    value, grad = ctx.estimate_gradient(params, idx)
    ctx.synchronize()
    value, grad = float(value.item()), grad.cpu().numpy().astype(np.float64)
    ctx.close()
    ref = O.estimate_gradient(embed(params, d, b), d, O.FULLRANK, tgt, eps, ent.code)
    rg = extract(ref["grad"], d, b)
    st, vt, gt = TOL[dtype]
    assert rel_err(eps, O.philox_normal(SEED, idx, d, 0, M, f64=dtype == np.float64)) < st and rel_err(Z, ref["Z"]) < st
    yv, yg = yardstick(params, d, b, ref["G"], ref["ell"], eps, ent.code, dtype) if ent.code >= 2 else (ref["value"], rg)
    v_bound = max(vt * abs(ref["value"]), 8 * abs(yv - ref["value"]))
    bound = lambda sl, scale: max(gt * scale, 8 * np.linalg.norm(yg[sl] - rg[sl]))
    whole = np.linalg.norm(grad - rg) / bound(slice(None), max(np.linalg.norm(rg), 1.0))
    worst = 0.0
    for lo, bk, off in layout:
        ix = np.r_[lo:lo + bk, off:off + bk * bk]   # the block's (dmu_k, dC_k)
        scale = max(np.linalg.norm(rg[ix]), np.linalg.norm(rg) / np.sqrt(len(layout)))
        worst = max(worst, np.linalg.norm(grad[ix] - rg[ix]) / bound(ix, scale))
        up = grad[off:off + bk * bk].reshape(bk, bk, order="F")[np.triu_indices(bk, 1)]
        assert np.all(up == 0.0)   # exact zeros above a block's diagonal
    vr = abs(value - ref["value"]) / v_bound
    print(f"[blockdiag] {(d, b, M)} {kind} ent{ent.code} {np.dtype(dtype).name}: ratios value {vr:.3f}, whole {whole:.3f}, block {worst:.3f}")
    assert vr <= 1.0 and whole <= 1.0 and worst <= 1.0, (vr, whole, worst)
    return params, value, grad, prob


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ent", ENTROPIES, ids=lambda e: type(e).__name__)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_diag_target_all_estimators_all_shapes(shape, ent, dtype):
    params, value, grad, prob = run_case(*shape, "diag", ent, dtype)
    if shape[1] == 1:   # b = 1 IS the mean-field family: [mu; sigma]
        ctx = avi.MiviContext(dtype, avi.MEANFIELD, shape[0], shape[2], ent.code, SEED)
        ctx.set_problem(prob)
        v, g = ctx.estimate_gradient(params, 3)
        assert abs(float(v.item()) - value) <= TOL[dtype][1] * abs(value) and rel_err(g.cpu().numpy().astype(np.float64), grad) < TOL[dtype][2]
        ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ent", [avi.ClosedFormEntropy(), avi.StickingTheLandingEntropy()], ids=lambda e: type(e).__name__)
@pytest.mark.parametrize("kind,plugin,bijector", [("dense", False, False), ("logreg0", False, False), ("funnel", False, False), ("dense", True, False),
                                                  ("dense", False, True)], ids=["dense", "logreg", "funnel", "plugin", "stacked"])
def test_other_targets_take_the_two_kernel_route(kind, plugin, bijector, ent, dtype):
    run_case(50, 17, 33, kind, ent, dtype, plugin=plugin, bijector=bijector)
    if kind == "dense" and not plugin:   # one sample tile: the VJP on the one-slice path that writes the gradient itself
        run_case(100, 40, 12, kind, ent, dtype, bijector=bijector)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(50, 17, 33), (100, 40, 20), (4099, 5, 17)], ids=lambda s: "x".join(map(str, s)))
def test_logpdf_and_std_of_own_samples_and_far_points(shape, dtype):
    d, b, M = shape
    q = make_bd(np.random.default_rng(3 + d), d, b, dtype)
    params, _ = avi.destructure(q)
    ctx = avi.MiviContext(dtype, avi.BLOCKDIAG, d, M, 0, SEED, block=b)
    Z = ctx.sample(params, 2)[0].cpu().numpy()
    mu, C_ = embed(params, d, b)[:d], embed(params, d, b)[d:].reshape(d, d, order="F")
    for pts in (Z, (q.location[:, None] + 10 * (Z - q.location[:, None])).astype(dtype)):   # own samples; points 10 scales away
        logq, std = (t.cpu().numpy().astype(np.float64) for t in ctx.logpdf(params, pts, std=True))
        x = np.linalg.solve(C_, pts.astype(np.float64) - mu[:, None])
        ref = -0.5 * (x * x).sum(axis=0) - 0.5 * d * np.log(2 * np.pi) - np.log(np.diagonal(C_)).sum()
        yq, yx = q.logpdf(pts, want_std=True)   # the same expressions in the context's dtype
        for name, got, want, yard in (("logq", logq, ref, yq), ("std", std, x, yx)):
            ratio = rel_err(got, want) / max(TOL[dtype][0], 8 * rel_err(yard.astype(np.float64), want))
            print(f"[blockdiag] logpdf {shape} {np.dtype(dtype).name} {name}: ratio {ratio:.3f}")
            assert ratio <= 1.0
    assert np.array_equal(avi.logpdf(q, Z).cpu().numpy(), ctx.logpdf(params, Z).cpu().numpy())   # the public entry is the same launch
    ctx.close()


def _ctx(d, b, M, ent, dtype, prob):
    ctx = avi.MiviContext(dtype, avi.BLOCKDIAG, d, M, ent.code, SEED, block=b)
    ctx.set_problem(prob)
    return ctx


@pytest.mark.parametrize("dtype", DTYPES)
def test_bitwise_repeats_batches_and_routes(dtype):
    import torch
    d, b, M = 256, 32, 1040
    rng = np.random.default_rng(5)
    pa, pb = (avi.destructure(make_bd(rng, d, b, dtype))[0] for _ in range(2))
    prob = make_problem(rng, "diag", d, dtype)[0]
    ctx = _ctx(d, b, M, avi.StickingTheLandingEntropy(), dtype, prob)
    a1 = [t.clone() for t in ctx.estimate_gradient(pa, 7)]
    b1 = [t.clone() for t in ctx.estimate_gradient(pb, 7)]
    a2 = [t.clone() for t in ctx.estimate_gradient(pa, 7)]   # A, B, A on a warm context
    assert all(torch.equal(x, y) for x, y in zip(a1, a2)) and not torch.equal(a1[1], b1[1])
    singles = [[t.clone() for t in ctx.estimate_gradient(pa, 7 + i)] for i in range(3)]
    values, grads = ctx.estimate_gradient_each(pa, 7, 3)
    v_last, g_last = ctx.empty(1), ctx.empty(ctx.params_len)
    ctx.estimate_gradient_n(ctx.to_device(pa), 7, 3, v_last, g_last)
    ctx.synchronize()
    for i, (v, g) in enumerate(singles):
        assert torch.equal(values[i:i + 1], v) and torch.equal(grads[i], g)
    assert torch.equal(v_last, singles[-1][0]) and torch.equal(g_last, singles[-1][1])
    ctx.close()
    # the same density as a dense target with a diagonal factor: the two-kernel route (MODE 0, the dense target's kernels, MODE 1)
    two = _ctx(d, b, M, avi.StickingTheLandingEntropy(), dtype, avi.DenseNormalProblem(prob.mean, np.diag(prob.std).astype(dtype)))
    v2, g2 = two.estimate_gradient(pa, 7)
    two.synchronize()
    assert abs(float(v2.item()) - float(a1[0].item())) <= 2 * TOL[dtype][1] * abs(float(v2.item()))   # (each route is within TOL of the truth)
    assert rel_err(g2.cpu().numpy().astype(np.float64), a1[1].cpu().numpy().astype(np.float64)) < 2 * TOL[dtype][2]
    two.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("opt,op,averager", [
    (avi.Descent(1e-3), avi.ClipScale(), avi.NoAveraging()), (avi.Adam(0.01), avi.ClipScale(), avi.PolynomialAveraging()),
    (avi.DoG(), avi.ClipScale(), avi.NoAveraging()), (avi.Descent(1e-3), avi.ProximalLocationScaleEntropy(), avi.NoAveraging()),
    (avi.DoWG(), avi.ProximalLocationScaleEntropy(), avi.PolynomialAveraging())], ids=["descent-clip", "adam-clip-poly", "dog-clip", "descent-prox", "dowg-prox-poly"])
def test_device_loop_equals_host_loop(opt, op, averager, dtype):
    d, b = 50, 17
    rng = np.random.default_rng(21)
    prob = make_problem(rng, "dense", d, dtype)[0]
    q0 = make_bd(rng, d, b, dtype)
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), optimizer=opt, n_samples=6, averager=averager, operator=op)
    q_dev, info_dev, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 25, prob, q0)
    q_host, info_host, _ = avi.optimize(avi.PhiloxRNG(SEED), alg, 25, prob, q0, device_loop=False)
    x, y = avi.destructure(q_dev)[0], avi.destructure(q_host)[0]
    if isinstance(opt, avi.DoG):   # DoG / DoWG: the two norms are summed in another order on the device (tests/test_gpu_flow.py)
        assert rel_err(x, y) < (1e-5 if dtype == np.float32 else 1e-12)
    else:
        assert np.array_equal(x, y) and [i["elbo"] for i in info_dev] == [i["elbo"] for i in info_host]


@pytest.mark.parametrize("dtype", DTYPES)
def test_clip_scale_clamps_only_the_block_diagonals(dtype):
    d, b = 50, 17
    layout, plen = avi.blockdiag_layout(d, b)
    ctx = avi.MiviContext(dtype, avi.BLOCKDIAG, d, 4, 0, SEED, block=b)
    params = (np.random.default_rng(1).normal(size=plen) * 1e-3).astype(dtype)
    want = params.copy()
    for lo, bk, off in layout:
        ix = off + np.arange(bk) * (bk + 1)
        want[ix] = np.maximum(want[ix], dtype(0.05))
    assert np.array_equal(avi.ClipScale(0.05).apply(ctx, ctx.to_device(params).clone()).cpu().numpy(), want)
    ctx.close()


def test_creation_errors():
    def status(block, family=avi.BLOCKDIAG, **kw):
        try:
            avi.MiviContext(np.float32, family, 8, 4, 0, 1, block=block, **kw).close()
            return 0
        except avi.MiviError as e:
            return e.status
    assert status(0) == status(65) == _lib.ERR_BAD_ARG and status(1) == status(64) == status(4, m_total=4) == 0
    assert status(4, m_offset=4) == status(4, m_total=8) == _lib.ERR_UNSUPPORTED
    cfg = _lib.MiviConfig(_lib.F32, 5, 8, 4, 0, 0, C.c_uint64(1), 0, 0, None, 0, 0)
    assert _lib.load().mivi_create(C.byref(cfg), C.byref(C.c_void_p())) == _lib.ERR_BAD_ARG


def test_unsupported_entries_refuse_the_family():
    d, b, M = 8, 4, 4
    prob = avi.DiagNormalProblem(np.zeros(d, np.float32), np.ones(d, np.float32))
    ctx = _ctx(d, b, M, avi.ClosedFormEntropy(), np.float32, prob)
    lib, h = ctx.lib, ctx.h
    buf = ctx.empty(4 * (d * d + d * M) + 64)
    host, dbl = np.zeros(4 * (d * d + d * M) + 64, dtype=np.float32), (C.c_double * 8)()
    P, Hp = ctx._p(buf), host.ctypes.data
    calls = {"mivi_estimate_score_gradient": (P, 0, P, P, P), "mivi_estimate_score_gradient_host": (Hp, 0, Hp, Hp, Hp),
             "mivi_gauss_expected_grad_hess": (P, 0, 0, P, P, P), "mivi_gauss_expected_grad_hess2": (P, 0, 0, P, P, P),
             "mivi_sqrt_ngd_update": (P, P, P, 0.1, P), "mivi_natgrad_init": (P, P), "mivi_bam_init": (P, P), "mivi_wass_init": (P, P),
             "mivi_estimate_partials": (P, 0, P), "mivi_estimate_gradient_dist": (P, 0, P, P), "mivi_profile_batch": (P, 1, 1, dbl),
             "mivi_set_base_dist": (1, 0.0), "mivi_logreg_seek_batch": (0,)}
    for name, args in calls.items():
        assert getattr(lib, name)(h, *args) == _lib.ERR_UNSUPPORTED, name
        msg = lib.mivi_last_error(h).decode()
        assert "MIVI_BLOCKDIAG" in msg and name.replace("_host", "") in msg, (name, msg)
    for refused in (lambda: ctx.optimize_loop_many(buf[:2 * ctx.params_len], 2, 2, 0, 0), lambda: ctx.optimize_loop_batches(buf, 2, 0, 0),
                    lambda: ctx.set_batch_schedule(np.zeros((1, 2), np.int64), likeadj=1.0)):
        with pytest.raises(avi.MiviError, match="MIVI_BLOCKDIAG") as e:
            refused()
        assert e.value.status == _lib.ERR_UNSUPPORTED
    ctx.close()
    q = make_bd(np.random.default_rng(0), d, b, np.float32)
    with pytest.raises(TypeError, match="block-diagonal"):
        avi.optimize(avi.PhiloxRNG(SEED), avi.KLMinScoreGradDescent(avi.AutoMIVI(), n_samples=4, operator=avi.ClipScale()), 2, prob, q)
    with pytest.raises(TypeError, match="block-diagonal"):
        avi.optimize_many([avi.PhiloxRNG(SEED)], avi.KLMinRepGradDescent(avi.AutoMIVI(), n_samples=4, operator=avi.ClipScale()), 2, [prob], [q])
    with pytest.raises(TypeError, match="block-diagonal"):
        avi.optimize(avi.PhiloxRNG(SEED), avi.KLMinRepGradDescent(avi.AutoMIVI(), n_samples=4, subsampling=object()), 2, prob, q)
    for alg in (avi.KLMinSqrtNaturalGradDescent, avi.KLMinNaturalGradDescent, avi.KLMinWassFwdBwd):
        with pytest.raises(TypeError, match="FullRankGaussian"):
            avi.optimize(avi.PhiloxRNG(SEED), alg(0.1), 2, prob, q)
