"""The two measure-space updates work in ONE scratch pair of the context (csrc/mivi_internal.h: ms_work, ms_part), which each ensures to its
own need and which holds nothing between calls.  So calls of both interleaved on one context -- at d = 65, the smallest size on two tiles,
where the natural-gradient update's float64 scratch is the larger and its vectors lie where the square-root update keeps its ticket -- must
give, bit for bit, what each call gives on a context of its own, and a repeated square-root update must reproduce the first."""
import numpy as np
import pytest
import torch

import advancedvi_jl_amd as avi
from tests import natgrad_ref as R
from tests.helpers import SEED, make_family
from tests.measure_space_cases import DTYPES, flat

pytestmark = pytest.mark.gpu


def _on(ctx, call, *arrays):
    """The call on device copies of the host arrays: the copies after it and what it returned."""
    dev = [ctx.to_device(a).clone() for a in arrays]
    ret = call(ctx, *dev)
    ctx.synchronize()
    return dev + [ret]


@DTYPES
def test_interleaved_updates_are_the_updates_of_their_own_contexts(dtype):
    d = 65
    rng = np.random.default_rng(700 + d)
    q, _ = make_family(rng, d, avi.FULLRANK, dtype)
    params, _ = avi.destructure(q)
    g = rng.normal(size=d).astype(dtype)
    H_sqrt = flat((rng.normal(size=(d, d)) - np.eye(d)).astype(dtype))                                     # as tests/test_gpu_sqrt_ngd.py
    H_nat = flat(R.congruent_hessian(params[d:].reshape(d, d, order="F"), rng).astype(dtype))             # as tests/test_gpu_natgrad.py

    def sqrt(c, p, gd, Hd):
        return c.sqrt_ngd_update(p, gd, Hd, 0.05)

    def init(c, p):
        return c.natgrad_init(p)

    def nat(ensure):
        return lambda c, p, st, gd, Hd: c.natgrad_update(p, st, gd, Hd, 0.3, ensure)

    def new_ctx():
        return avi.MiviContext(dtype, avi.FULLRANK, d, 1, 0, SEED)

    shared = new_ctx()
    got, want = [], []

    def both(call, *arrays):
        got.append(_on(shared, call, *arrays))
        own = new_ctx()
        want.append(_on(own, call, *arrays))
        own.close()
        return got[-1]

    both(sqrt, params, g, H_sqrt)
    st0 = both(init, params)[-1].cpu().numpy()
    after = both(nat(True), params, st0, g, H_nat)
    both(sqrt, params, g, H_sqrt)
    both(nat(False), after[0].cpu().numpy(), after[1].cpu().numpy(), g, H_nat)
    shared.close()
    for i, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)), i
    assert all(torch.equal(x, y) for x, y in zip(got[0], got[3]))          # the repeated square-root update is the first
    assert not np.array_equal(got[0][0].cpu().numpy(), params) and not np.array_equal(got[4][0].cpu().numpy(), got[2][0].cpu().numpy())   # (updates at all)
