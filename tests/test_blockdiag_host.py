"""Host checks of the block-diagonal family: destructure / restructure, the layout against a brute-force count, the dense embedding."""
import numpy as np
import pytest

import advancedvi_jl_amd as avi

SHAPES = [(7, 1), (10, 2), (10, 16), (48, 16), (50, 17), (130, 64), (4099, 5)]


def make_bd(rng, d, b, dtype=np.float64):
    sizes = [min(b, d - lo) for lo in range(0, d, b)]
    blocks = [np.tril(rng.normal(size=(s, s)) * 0.3, -1) + np.diag(rng.uniform(0.5, 1.5, size=s)) for s in sizes]
    return avi.BlockDiagGaussian(rng.normal(size=d).astype(dtype), blocks)


@pytest.mark.parametrize("d,b", SHAPES)
def test_layout_against_a_brute_force_count(d, b):
    layout, plen = avi.blockdiag_layout(d, b)
    owner = np.arange(d) // b   # the block of every coordinate
    sizes = np.bincount(owner)
    assert [bk for _, bk, _ in layout] == sizes.tolist() and [lo for lo, _, _ in layout] == [k * b for k in range(len(sizes))]
    assert plen == d + sum(int(s) ** 2 for s in sizes)
    assert [off for _, _, off in layout] == [d + sum(int(s) ** 2 for s in sizes[:k]) for k in range(len(sizes))]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("d,b", SHAPES[:-1])
def test_destructure_restructure_round_trip(d, b, dtype):
    q = make_bd(np.random.default_rng(d + b), d, b, dtype)
    flat, re = avi.destructure(q)
    assert q.family == avi.BLOCKDIAG == 5 and flat.dtype == dtype and flat.shape == (avi.blockdiag_layout(d, b)[1],)
    q2 = re(flat)
    assert isinstance(q2, avi.BlockDiagGaussian) and q2.block == q.block and np.array_equal(q2.location, q.location)
    assert all(np.array_equal(x, y) for x, y in zip(q2.blocks, q.blocks)) and np.array_equal(avi.destructure(q2)[0], flat)
    with pytest.raises(ValueError):
        re(flat[:-1])


@pytest.mark.parametrize("d,b", SHAPES[:-1])
def test_dense_embedding_reproduces_the_block_form(d, b):
    q = make_bd(np.random.default_rng(3), d, b)
    full = avi.FullRankGaussian(q.location, q.dense_scale())
    assert np.isclose(q.entropy(), full.entropy(), rtol=1e-13)
    assert np.allclose(q.cov(), full.cov(), rtol=1e-13, atol=0) and np.allclose(q.var(), full.var(), rtol=1e-13)
    assert np.array_equal(q.mean(), full.mean())
    z = np.random.default_rng(4).normal(size=(d, 5)) * 3
    x = np.linalg.solve(full.scale, z - q.location[:, None])
    lq, std = q.logpdf(z, want_std=True)
    assert np.allclose(std, x, rtol=1e-10, atol=1e-12)
    assert np.allclose(lq, -0.5 * (x * x).sum(0) - 0.5 * d * np.log(2 * np.pi) - np.log(np.diagonal(full.scale)).sum(), rtol=1e-12)
    off = np.ones((d, d), bool)
    for lo, bk, _ in avi.blockdiag_layout(d, b)[0]:
        off[lo:lo + bk, lo:lo + bk] = False
    assert np.all(q.cov()[off] == 0.0)   # no covariance across blocks
