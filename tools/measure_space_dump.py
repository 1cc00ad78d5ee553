"""Every result array of the measure-space entries (sqrt_ngd / natgrad: update, init, the _host forms, 3-step _steps) over the size
boundaries of their kernels, both dtypes, into one .npz -- to compare two builds of the library bit for bit:
    python tools/measure_space_dump.py out.npz            on each build
    python tools/measure_space_dump.py a.npz b.npz        compares: every array np.array_equal, prints the count, exit status 1 on a difference
Inputs as in tests/test_gpu_sqrt_ngd.py and tests/test_gpu_natgrad.py (test_update_matches_restatement, test_steps_are_the_single_calls_bitwise)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import advancedvi_jl_amd as avi
from tests import natgrad_ref as R
from tests.helpers import SEED, make_family
from tests.measure_space_cases import dense_ctx, flat

SIZES = (1, 5, 44, 45, 48, 49, 64, 65, 130)
DTYPES = (np.float32, np.float64)


def updates(out, dtype, d):
    tag = f"{np.dtype(dtype).name}/d{d}"
    ctx = avi.MiviContext(dtype, avi.FULLRANK, d, 1, 0, SEED)
    rng = np.random.default_rng(700 + d)
    q, _ = make_family(rng, d, avi.FULLRANK, dtype)
    params, _ = avi.destructure(q)
    g = rng.normal(size=d).astype(dtype)
    H = (rng.normal(size=(d, d)) - np.eye(d)).astype(dtype)
    p = ctx.to_device(params).clone()
    ent = ctx.sqrt_ngd_update(p, ctx.to_device(g), ctx.to_device(flat(H)), 0.05)
    ctx.synchronize()
    out[f"{tag}/sqrt/params"], out[f"{tag}/sqrt/entropy"] = p.cpu().numpy(), ent.cpu().numpy()
    out[f"{tag}/sqrt_host/params"], out[f"{tag}/sqrt_host/entropy"] = ctx.sqrt_ngd_update_host(params, g, H, 0.05)
    st0 = ctx.natgrad_init(ctx.to_device(params).clone()).cpu().numpy().copy()
    ctx.synchronize()
    out[f"{tag}/init/state"] = st0
    rng = np.random.default_rng(800 + d)
    g = rng.normal(size=d).astype(dtype)
    H = R.congruent_hessian(params[d:].reshape(d, d, order="F"), rng).astype(dtype)
    for ensure in (True, False):
        rule = "ensure" if ensure else "plain"
        p, st = ctx.to_device(params).clone(), ctx.to_device(st0).clone()
        ent = ctx.natgrad_update(p, st, ctx.to_device(g), ctx.to_device(flat(H)), 0.3, ensure)
        ctx.synchronize()
        out[f"{tag}/natgrad_{rule}/params"], out[f"{tag}/natgrad_{rule}/state"], out[f"{tag}/natgrad_{rule}/entropy"] = p.cpu().numpy(), st.cpu().numpy(), ent.cpu().numpy()
        ph, sh, eh = ctx.natgrad_update_host(params, st0, g, H, 0.3, ensure)
        out[f"{tag}/natgrad_host_{rule}/params"], out[f"{tag}/natgrad_host_{rule}/state"], out[f"{tag}/natgrad_host_{rule}/entropy"] = ph, sh, eh
    ctx.close()


def steps(out, dtype, d, n, second):
    tag = f"{np.dtype(dtype).name}/d{d}n{n}/{'order2' if second else 'stein'}"
    ctx, params, _, _ = dense_ctx(d, n, dtype, second)
    p = ctx.to_device(params).clone()
    elbo = ctx.sqrt_ngd_steps(p, 11, 3, 0.05, n_samples=n, second_order=second)
    ctx.synchronize()
    out[f"{tag}/sqrt_steps/params"], out[f"{tag}/sqrt_steps/elbo"] = p.cpu().numpy(), elbo.cpu().numpy()
    p = ctx.to_device(params).clone()
    st = ctx.natgrad_init(p)
    elbo = ctx.natgrad_steps(p, st, 11, 3, 0.02, True, n_samples=n, second_order=second)
    ctx.synchronize()
    out[f"{tag}/natgrad_steps/params"], out[f"{tag}/natgrad_steps/state"], out[f"{tag}/natgrad_steps/elbo"] = p.cpu().numpy(), st.cpu().numpy(), elbo.cpu().numpy()
    ctx.close()


def dump(path):
    out = {}
    for dtype in DTYPES:
        for d in SIZES:
            updates(out, dtype, d)
        for d, n in ((5, 10), (70, 64)):
            for second in (False, True):
                steps(out, dtype, d, n, second)
    np.savez(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"{len(out)} arrays -> {path}")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    differ = [k for k in sorted(set(A.files) | set(B.files)) if k not in A.files or k not in B.files or not np.array_equal(A[k], B[k])]
    print(f"{len(A.files)} / {len(B.files)} arrays, {len(differ)} differ" + "".join(f"\n  {k}" for k in differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[1:3]) if len(sys.argv) > 2 else dump(sys.argv[1]))
