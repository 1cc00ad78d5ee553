"""FisherMinBatchMatch without a GPU: the two forms of tests/bam_ref.py agree on the fixtures the GPU tests use (a condition on the
fixtures: the device builds the rank-B form and is checked against the literal expression), the restatement recovers a dense Gaussian target
exactly, the header and the library carry the new entries, and the constructor and `init` refuse what the reference refuses."""
import os
import re

import numpy as np
import pytest

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import _lib
from oracle import oracle as O
from tests import bam_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DS = (3, 10, 44, 45, 64, 65, 130)
BS = (2, 5, 8, 32, 64)
ENTRIES = ("mivi_bam_init", "mivi_bam_moments", "mivi_bam_moments_host", "mivi_estimate_fisher", "mivi_estimate_fisher_host", "mivi_bam_update",
           "mivi_bam_update_host", "mivi_bam_steps")


def _case(d, B):
    m, C, u, G = R.random_case(d, B, 1000 * d + B)
    return m, C @ C.T, C @ u + m[:, None], G


@pytest.mark.parametrize("lam", [0.25, 4.0])
@pytest.mark.parametrize("d", DS)
def test_the_two_forms_agree(d, lam):
    for B in BS:
        err = R.discrepancy(*_case(d, B), lam)
        print(f"[bam forms] d {d} B {B} lambda {lam}: m {err[0]:.1e} C {err[1]:.1e} Sigma {err[2]:.1e}")
        assert max(err) <= 1e-11, (d, B, err)


@pytest.mark.parametrize("d", [3, 10])
def test_the_two_forms_agree_at_iteration_one(d):
    for B in BS:
        err = R.discrepancy(*_case(d, B), float(d * B))
        print(f"[bam forms] d {d} B {B} lambda {d * B}: m {err[0]:.1e} C {err[1]:.1e} Sigma {err[2]:.1e}")
        assert max(err) <= 1e-11, (d, B, err)


def _dense_target(d, seed):
    rng = np.random.default_rng(seed)
    L = np.tril(rng.normal(size=(d, d)) * (0.2 / np.sqrt(d))) + np.eye(d)
    return O.DenseNormalTarget(rng.normal(size=d), L)


@pytest.mark.parametrize("dtype,bound", [(np.float64, 1e-24), (np.float32, 1e-11)], ids=["f64", "f32"])
@pytest.mark.parametrize("d,B", [(5, 32), (20, 8)])
def test_exact_recovery_on_a_dense_gaussian(d, B, dtype, bound):
    """The batch-and-match fixed point of a Gaussian target is the target itself, from any batch: after 1000 steps the squared distance
    to (mean, L) is rounding -- (2^-53)^2 resp. (2^-24)^2 per entry, times the entries and a conditioning factor of a few hundred."""
    tgt = _dense_target(d, 7 + d)
    rng = np.random.default_rng(11)
    draws = [rng.normal(size=(d, B)) for _ in range(1000)]
    (m, C, _), infos = R.steps(np.zeros(d), np.eye(d), draws, tgt, dtype=dtype)
    d0 = np.sum(tgt.mean ** 2) + np.sum((np.eye(d) - tgt.L) ** 2)
    dl = np.sum((m - tgt.mean) ** 2) + np.sum((C - tgt.L) ** 2)
    print(f"[bam recovery] d {d} B {B} {np.dtype(dtype).name}: ratio {dl / d0:.1e}, last fisher {infos[-1]['covweighted_fisher']:.1e}")
    assert dl <= bound * d0
    assert [i["iteration"] for i in infos] == list(range(1, 1001))


@pytest.mark.parametrize("B", [10, 32])
def test_the_fixed_point_under_batch_size_one_subsampling(B):
    """test/models/subsamplednormals.jl, batch size 1, T = 1000: each step's target is ONE of the normals with the likelihood scaled by
    n_data, so the iterate settles near the posterior mean but at a scale of its own -- 0.10 to 0.11 of the initial squared distance,
    whatever the seed and the draws.  That is why the GPU test of this case (tests/test_gpu_bam.py) cannot ask the project's 0.1 and
    asks 0.12 and agreement with this restatement instead; the reference asks 1/2."""
    from tests.natgrad_ref import SubsampledNormals
    n_data = 8
    model = SubsampledNormals(np.random.default_rng(3).normal(size=n_data))
    mt, Lt = model.mus.mean(), np.sqrt(1.0 / n_data)
    ratios = []
    for seed in range(6):
        rng = np.random.default_rng(seed)
        m, C, S, order = np.zeros(1), np.eye(1), np.eye(1), []
        for t in range(1, 1001):
            if not order:
                order = list(rng.permutation(n_data))
            (m, C, S), _ = R.step(m, C, S, rng.normal(size=(1, B)), model.subsample([order.pop()]), t)
        ratios.append(((m[0] - mt) ** 2 + (C[0, 0] - Lt) ** 2) / (mt ** 2 + (1.0 - Lt) ** 2))
    print(f"[bam subsampled fixed point] B {B}: {np.round(ratios, 4)}")
    assert 0.10 <= min(ratios) and max(ratios) <= 0.11


def test_header_and_library_export_the_entries():
    src = open(os.path.join(ROOT, "include", "mivi.h")).read()
    assert re.search(r"#define\s+MIVI_BAM_MAX_SAMPLES\s+(\d+)", src).group(1) == str(avi.BAM_MAX_SAMPLES)
    assert avi.BAM_MAX_SAMPLES >= 64
    lib = avi.load_library()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


def test_constructor():
    alg = avi.FisherMinBatchMatch()
    assert alg.n_samples == 32 and alg.subsampling is None
    assert "FisherMinBatchMatch(n_samples=32" in repr(alg)
    for bad in (0, 1, -3, 2.0, avi.BAM_MAX_SAMPLES + 1):
        with pytest.raises(ValueError):
            avi.FisherMinBatchMatch(n_samples=bad)
    assert avi.FisherMinBatchMatch(n_samples=avi.BAM_MAX_SAMPLES).n_samples == avi.BAM_MAX_SAMPLES


def test_init_refusals():
    class Order0:
        def dimension(self):
            return 5

        def logdensity(self, z):
            return -0.5 * float(np.sum(np.asarray(z) ** 2))

        def capabilities(self):
            return avi.LogDensityOrder(0)

    alg = avi.FisherMinBatchMatch(n_samples=4)
    with pytest.raises(ValueError, match="requires at least first-order differentiation capability"):
        avi.init(avi.PhiloxRNG(1), alg, avi.FullRankGaussian(np.zeros(5), np.eye(5)), Order0())
    prob = avi.DiagNormalProblem(np.zeros(5), np.ones(5))
    with pytest.raises(TypeError, match="FisherMinBatchMatch"):
        avi.init(avi.PhiloxRNG(1), alg, avi.MeanFieldGaussian(np.zeros(5), np.ones(5)), prob)
