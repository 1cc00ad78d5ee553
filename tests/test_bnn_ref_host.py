"""tests/bnn_ref.py, the reference of tests/test_gpu_bnn.py, pinned to torch.autograd of its own value (no GPU)."""
import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from tests.bnn_ref import LOG2PI, BNNRef


@pytest.mark.parametrize("likelihood", ["bernoulli", "normal"])
@pytest.mark.parametrize("n,p,hidden", [(7, 3, (2,)), (12, 4, (5, 3)), (5, 2, (3, 4, 2))])
def test_reference_gradient_is_autograd_of_its_value(n, p, hidden, likelihood):
    rng = np.random.default_rng(n)
    y = rng.integers(0, 2, size=n) if likelihood == "bernoulli" else rng.normal(size=n)
    ref = BNNRef(rng.normal(size=(n, p)), y, hidden, likelihood, noise=0.7, prior_std=1.3, likeadj=2.5)
    prob = avi.BNNProblem(ref.X, ref.y, hidden, likelihood, noise=0.7, prior_std=1.3, likeadj=2.5)
    d = ref.dimension()
    assert prob.dimension() == d
    z = torch.tensor(rng.normal(size=d) * 0.5, dtype=torch.float64, requires_grad=True)
    a, off = torch.tensor(ref.X), 0
    for k, (o, i) in enumerate(prob.layers()):   # the layout of include/mivi.h, written out independently of unpack
        W, b = z[off:off + o * i].reshape(i, o).T, z[off + o * i:off + o * (i + 1)]
        a, off = a @ W.T + b, off + o * (i + 1)
        a = torch.tanh(a) if k < len(hidden) else a
    f, yt = a[:, 0], torch.tensor(ref.y)
    ll = ((yt * f - torch.nn.functional.softplus(f)).sum() if likelihood == "bernoulli" else
          -0.5 * (((yt - f) / 0.7) ** 2).sum() - n * np.log(0.7) - 0.5 * n * LOG2PI)
    val = 2.5 * ll - 0.5 * (z * z).sum() / 1.3 ** 2 - d * np.log(1.3) - 0.5 * d * LOG2PI
    val.backward()
    v, g = ref.logdensity_and_gradient(z.detach().numpy())
    assert v == pytest.approx(val.item(), rel=1e-13) and np.allclose(g, z.grad.numpy(), rtol=1e-11, atol=1e-12)
    assert np.allclose(ref.forward(z.detach().numpy())[0], f.detach().numpy(), rtol=1e-13, atol=1e-14)
    for (W, b), (Wr, br) in zip(prob.unpack(z.detach().numpy()), ref.unpack(z.detach().numpy())):
        assert np.array_equal(W, Wr) and np.array_equal(b, br)
