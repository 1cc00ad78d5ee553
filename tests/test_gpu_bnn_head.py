"""The multi-output head of the Bayesian neural network target (mivi_bnn_t.n_out >= 2: k_bnn_rows_head / k_bnn_forward_head) on the library's
own draws against HeadRef -- the model in torch on the CPU with autograd, in float64 and in the context's dtype -- by `check` of
tests/test_gpu_bnn.py: bound = max(TOL x scale, 8 x |restatement - float64|) on the value, the whole gradient and every W_l / b_l block."""
import re

import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from tests.helpers import SEED
from tests.test_gpu_blockdiag import TOL
from tests.test_gpu_bnn import check

pytestmark = pytest.mark.gpu
DTYPES, LIKS = [np.float32, np.float64], ["categorical", "normal"]
CF, STL, KW = avi.ClosedFormEntropy(), avi.StickingTheLandingEntropy(), dict(noise=0.7, prior_std=1.3)
MID = (100, 7, (16, 5), 3, 7)   # (n, p, hidden, C, M)
# the minimum of everything; a partial row tile and C < 16 (padded classes must stay out of the softmax); C just past a tile (a second output
# tile), several row tiles; the widest head that fits in f64; three hidden layers (13 dW tiles per wave); slices of 240, 240 and 220 rows and
# the f32 flush every 128 rows; every limit at once (16 dW tiles per wave), f32 only: over the LDS limit in f64
SHAPES = [(1, 1, (1,), 2, 1), (17, 3, (5,), 3, 5), (65, 17, (16, 17), 17, 3), (40, 64, (64, 64), 64, 2), (40, 16, (64, 64, 64), 64, 2), (700, 5, (20,), 4, 2)]
CASES = [(s, t) for s in SHAPES for t in DTYPES] + [((40, 64, (64, 64, 64), 64, 2), np.float32)]
ids = lambda c: f"{c[0][0]}x{c[0][1]}x" + "-".join(map(str, c[0][2])) + f"x{c[0][3]}x{c[0][4]}-{np.dtype(c[1]).name}"   # noqa: E731


class HeadRef:
    """The oracle targets' interface over torch.autograd: y holds labels (categorical) or is n x C (normal)."""
    def __init__(self, X, y, hidden, C, lik, noise=1.0, prior_std=1.0, likeadj=1.0, dtype=np.float64):
        self.t = torch.float64 if dtype == np.float64 else torch.float32
        self.X, y = torch.as_tensor(np.asarray(X, np.float64)).to(self.t), torch.as_tensor(np.asarray(y, np.float64))
        self.y, self.widths = y.long() if lik == "categorical" else y.to(self.t), (self.X.shape[1],) + tuple(hidden) + (C,)
        self.lik, self.noise, self.prior_std, self.likeadj = lik, noise, prior_std, likeadj

    def dimension(self):
        return sum(o * (i + 1) for i, o in zip(self.widths, self.widths[1:]))

    def forward(self, z, X=None):
        a, z, off = self.X if X is None else torch.as_tensor(np.asarray(X, np.float64)).to(self.t), torch.as_tensor(z).to(self.t), 0
        for k, (i, o) in enumerate(zip(self.widths, self.widths[1:])):
            a = a @ z[off:off + o * i].reshape(i, o) + z[off + o * i:off + o * (i + 1)]   # (column-major o x i read as (i, o) row-major)
            a, off = torch.tanh(a) if k < len(self.widths) - 2 else a, off + o * (i + 1)
        return a

    def logdensity_and_gradient(self, z):
        z = torch.tensor(np.asarray(z, np.float64), dtype=self.t, requires_grad=True)
        f, log2pi = self.forward(z), float(np.log(2 * np.pi))
        ll = (-torch.nn.functional.cross_entropy(f, self.y, reduction="sum") if self.lik == "categorical" else
              -0.5 * ((self.y - f) ** 2).sum() / self.noise ** 2 - f.numel() * (np.log(self.noise) + 0.5 * log2pi))
        v = self.likeadj * ll - 0.5 * (z * z).sum() / self.prior_std ** 2 - z.numel() * (np.log(self.prior_std) + 0.5 * log2pi)
        return float(v.detach()), torch.autograd.grad(v, z)[0].numpy().astype(np.float64)

    def logdensity(self, z):
        return self.logdensity_and_gradient(z)[0]


def make_data(shape, lik, dtype, saturated=False):
    n, p, hidden, C, M = shape
    rng = np.random.default_rng(1000 * n + 10 * p + sum(hidden) + C)
    X = (rng.normal(size=(n, p)) / np.sqrt(p)).astype(dtype)
    y = (rng.integers(0, C, size=n) if lik == "categorical" else rng.normal(size=(n, C))).astype(dtype)
    ref = HeadRef(X, y, hidden, C, lik)
    loc, scale = rng.normal(size=ref.dimension()) * 0.7, rng.uniform(0.3, 0.9, size=ref.dimension())
    if saturated:   # |logit| reaches 100 at the location: the output layer's block of theta is the last C (n_H + 1) entries
        loc[-C * (hidden[-1] + 1):] *= 100.0 / float(ref.forward(loc).abs().max())
        scale *= 0.02
    prob = avi.BNNProblem(X, y, hidden, likelihood=lik, n_classes=C if lik == "categorical" else None, **KW)
    return X, y, avi.MeanFieldGaussian(loc.astype(dtype), scale.astype(dtype)), prob


def run_case(shape, lik, ent, dtype, likeadj=1.0, rows=None, cap=0, saturated=False):
    n, p, hidden, C, M = shape
    X, y, q, prob = make_data(shape, lik, dtype, saturated)
    prob.likeadj, params = likeadj, avi.destructure(q)[0]
    ctx = avi.MiviContext(dtype, avi.MEANFIELD, prob.dimension(), M, ent.code, SEED)
    ctx.set_problem(prob if rows is None else prob.subsample(rows))
    ctx.bnn_set_part_cap(cap)
    eps = ctx.sample(params, 3)[1].cpu().numpy().astype(np.float64)
    value, grad = ctx.estimate_gradient(params, 3)
    ctx.synchronize()
    sel, la = (slice(None), likeadj) if rows is None else (np.asarray(rows), likeadj * n / len(rows))
    tgts = [HeadRef(X[sel], y[sel], hidden, C, lik, likeadj=la, dtype=t, **KW) for t in (np.float64, dtype)]
    check(float(value.item()), grad.cpu().numpy().astype(np.float64), params, *tgts, eps, ent, dtype, f"head {shape} {lik}")
    return ctx, prob, params, value.clone(), grad.clone()


@pytest.mark.parametrize("lik", LIKS)
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_shapes(case, lik):
    run_case(case[0], lik, CF, case[1])[0].close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kw", [dict(saturated=True), dict(likeadj=7.5, rows=[5, 99, 5, 0, 42, 42, 64, 63, 17])], ids=["saturated", "rows-likeadj"])
def test_saturated_logits_and_row_subset_with_likeadj(kw, dtype):
    run_case(MID, "categorical", STL, dtype, **kw)[0].close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_bitwise_repeat_device_data_and_part_cap(dtype):
    ctx, prob, params, v, g = run_case(MID, "normal", CF, dtype)
    assert all(torch.equal(a, b) for a, b in zip(ctx.estimate_gradient(params, 3), (v, g)))
    X, y = (torch.as_tensor(np.ascontiguousarray(a.T)).cuda() for a in make_data(MID, "normal", dtype)[:2])   # (p, n) and (k, n) contiguous
    ctx.set_problem(avi.BNNProblem(X, y, MID[2], "normal", **KW))
    assert ctx.problem.n_out == MID[3] and all(torch.equal(a, b) for a, b in zip(ctx.estimate_gradient(params, 3), (v, g)))
    capped = run_case(MID, "normal", CF, dtype, cap=3 * prob.dimension() * 8)   # one slice: chunks of 3, 3 and 1 samples
    assert torch.equal(capped[3], v) and torch.equal(capped[4], g)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lik", LIKS)
def test_predict_and_the_device_loop(lik, dtype):
    (n, p, hidden, C, M), n_new = MID, 17
    X, y, q, prob = make_data(MID, lik, dtype)
    ctx = avi.MiviContext(dtype, avi.MEANFIELD, prob.dimension(), M, CF.code, SEED)
    ctx.set_problem(prob)
    Z, Xnew = ctx.sample(avi.destructure(q)[0], 3, want_eps=False), np.random.default_rng(n_new).normal(size=(n_new, p)).astype(dtype)
    f, Zh = prob.predict(Z, Xnew, ctx).cpu().numpy().astype(np.float64), Z.cpu().numpy().astype(np.float64)
    ref, yard = (np.stack([HeadRef(X, y, hidden, C, lik, dtype=t).forward(Zh[:, m], Xnew).numpy() for m in range(M)]).astype(np.float64) for t in (np.float64, dtype))
    assert f.shape == (M, n_new, C) and np.linalg.norm(f - ref) <= max(TOL[dtype][1] * max(np.linalg.norm(ref), 1.0), 8 * np.linalg.norm(yard - ref))
    ctx.close()
    q0 = avi.FullRankGaussian(dtype(0.1) * q.location, (0.1 * np.eye(len(q.location))).astype(dtype))   # full rank: the device loop equals the host loop
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI(), optimizer=avi.Adam(1e-2), n_samples=M, operator=avi.ClipScale())
    (q_dev, info_dev, _), (q_host, info_host, _) = (avi.optimize(avi.PhiloxRNG(SEED), alg, 5, prob, q0, **k) for k in ({}, dict(device_loop=False)))
    assert np.array_equal(avi.destructure(q_dev)[0], avi.destructure(q_host)[0]) and [i["elbo"] for i in info_dev] == [i["elbo"] for i in info_host]
    assert not np.array_equal(avi.destructure(q_dev)[0], avi.destructure(q0)[0])


def test_errors_by_message_and_the_unchanged_one_output_path():
    n, p, M, d1, d3 = 8, 3, 4, 4 * 4 + 2 * 5 + 3, 4 * 4 + 2 * 5 + 3 * 3   # 3 -> 4 -> 2 -> 1 and -> 3
    ctx, one = (avi.MiviContext(np.float32, avi.MEANFIELD, d, M, 0, SEED) for d in (d3, d1))
    X, y = np.zeros((n, p), np.float32, order="F"), np.zeros(n, np.float32)
    net = lambda *n_out: avi._lib.MiviBnn(2, (3 * avi._lib.C.c_int32)(4, 2, 0), 0, 1.0, 1.0, 1.0, *n_out)   # noqa: E731
    set_target = lambda c, cfg, labels: c.lib.mivi_set_target_bnn(c.h, avi._lib.C.byref(cfg), X.ctypes.data, labels.ctypes.data, n, p, 0)   # noqa: E731
    for c, cfg, labels, msg in ((ctx, net(65), y, r"n_out must lie in \[0, 64\]"), (ctx, net(-1), y, "n_out must lie"), (ctx, net(3), y + 0.5, "categorical label"),
                                (ctx, net(3), y + 3, r"categorical label is not an integer in \[0, 3\)"), (one, net(3), y, "parameter count, 35")):
        assert set_target(c, cfg, labels) == avi._lib.ERR_BAD_ARG and re.search(msg, c.lib.mivi_last_error(c.h).decode()), (msg, c.lib.mivi_last_error(c.h))
    assert set_target(ctx, net(3), y + 2) == 0 and net().n_out == 0 and set_target(one, net(), y) == 0   # (six positional values: the one-output network)
    ctx.close(), one.close()
    big = avi.BNNProblem(np.zeros((n, 64)), y, (64, 64, 64), "categorical", n_classes=64)   # f64: over the LDS limit, both byte counts in the message
    ctx = avi.MiviContext(np.float64, avi.MEANFIELD, big.dimension(), 2, 0, SEED)
    with pytest.raises(avi.MiviError, match="needs 187552 bytes of LDS, the limit is 163840"):
        ctx.set_problem(big)
    ctx.close()
    for kw in (dict(likelihood="categorical"), dict(likelihood="normal", n_classes=3), dict(likelihood="categorical", n_classes=1)):
        with pytest.raises(ValueError, match="n_classes"):
            avi.BNNProblem(X, y, (4, 2), **kw)
