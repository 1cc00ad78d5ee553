"""Every result array of the entries whose host launchers go through by_dtype or the sample-chunk walk (csrc/mivi_internal.h,
csrc/api_common.h), both dtypes, at the smallest shapes that reach each launcher, into one .npz -- to compare two builds bit for bit:
    python tools/launch_layer_dump.py out.npz            on each build
    python tools/launch_layer_dump.py a.npz b.npz        compares: every array np.array_equal, prints the count, exit status 1 on a difference
A case the library refuses is recorded as its error text (the two builds must refuse alike).  The table of launchers and the cases that
reach them: profiles/launch_layer_refactor.md."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import advancedvi_jl_amd as avi
from tests.helpers import SEED, make_family, make_problem
from tests.measure_space_cases import logreg
from tools import measure_space_dump as MS

DTYPES = (np.float32, np.float64)
FAMILIES = ((avi.MEANFIELD, "mf"), (avi.FULLRANK, "fr"))
RULES = {"descent": 0, "adam": 1, "dog": 2, "dowg": 3, "cocob": 4}
OPS = {"none": 0, "clip": 1, "prox": 2}


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


class Dump:
    def __init__(self):
        self.out = {}

    def case(self, tag, fn):
        """fn() -> dict name -> array (device tensors are synchronised and copied)"""
        try:
            res = fn()
            for k, v in res.items():
                self.out[f"{tag}/{k}"] = host(v).copy()
        except avi.MiviError as e:
            self.out[f"{tag}/refused"] = np.array(str(e))
            print(f"refused: {tag}: {e}")


def setup(dtype, family, d, n_mc, kind, entropy=0, seed=0, order=1, bijector=None):
    rng = np.random.default_rng(1000 + 7 * d + seed)
    q, _ = make_family(rng, d, family, dtype)
    params, _ = avi.destructure(q)
    if kind == "logreg2":
        prob = logreg(order=2)
    elif kind == "funnel":
        prob = avi.FunnelProblem(d, 1.5, order=order)
    else:
        prob, _ = make_problem(rng, kind, d, dtype)
        if order != 1:
            prob = type(prob)(*((prob.mean, prob.std) if kind == "diag" else (prob.mean, prob.L)), order=order)
    if bijector is not None:
        prob = avi.TransformedProblem(prob, bijector)
    ctx = avi.MiviContext(dtype, family, d, n_mc, entropy, SEED)
    ctx.set_problem(prob)
    return ctx, params


def single_estimates(D, dtype):
    dn = np.dtype(dtype).name

    def est(tag, ctx, params, idx=3):
        def run():
            v, g = ctx.estimate_gradient(params, idx)
            vh, gh = ctx.estimate_gradient_host(params, idx + 1)
            ob = ctx.estimate_objective(params, idx + 2)
            ctx.synchronize()
            return dict(value=v, grad=g, value_host=vh, grad_host=gh, objective=ob)
        D.case(tag, run)
        ctx.close()

    for family, fn in FAMILIES:
        for d in (5, 33, 64, 130):
            for n in (8, 64):
                est(f"{dn}/est/{fn}/diag/d{d}n{n}", *setup(dtype, family, d, n, "diag"))
        for d, n in ((33, 8), (64, 64), (70, 24)):   # dense target; ragged d and n: f32 takes the first-generation route too
            est(f"{dn}/est/{fn}/dense/d{d}n{n}", *setup(dtype, family, d, n, "dense"))
        est(f"{dn}/est/{fn}/mc_entropy/d33n8", *setup(dtype, family, 33, 8, "diag", entropy=avi.MonteCarloEntropy.code))
        est(f"{dn}/est/{fn}/logreg/d5n8", *setup(dtype, family, 5, 8, "logreg0"))
        est(f"{dn}/est/{fn}/logreg1/d9n16", *setup(dtype, family, 9, 16, "logreg1"))
        est(f"{dn}/est/{fn}/funnel/d8n8", *setup(dtype, family, 8, 8, "funnel"))
        est(f"{dn}/est/{fn}/funnel/d64n64", *setup(dtype, family, 64, 64, "funnel"))
        bij = avi.StackedBijector([(0, 2, "identity"), (2, 5, "exp")])
        est(f"{dn}/est/{fn}/stacked/d5n8", *setup(dtype, family, 5, 8, "diag", bijector=bij))
    for d, n in ((33, 8), (96, 48), (256, 32)):   # sticking the landing: the LDS-resident solves (f32 and f64 routes), the second-generation solve
        est(f"{dn}/est/fr/stl/d{d}n{n}", *setup(dtype, avi.FULLRANK, d, n, "diag", entropy=avi.StickingTheLandingEntropy.code))


def other_entries(D, dtype):
    dn = np.dtype(dtype).name
    for family, fn in FAMILIES:
        for kind, d, n in (("diag", 5, 8), ("dense", 33, 16), ("diag", 64, 64)):
            ctx, params = setup(dtype, family, d, n, kind)

            def run():
                v, e, g = ctx.estimate_score_gradient(params, 5)
                ctx.synchronize()
                return dict(value=v, elbo=e, grad=g)
            D.case(f"{dn}/score/{fn}/{kind}/d{d}n{n}", run)
            ctx.close()
    # (the sampled second-order branch, logistic regression and funnel, adds its f64 sums with atomics, one wave per sample: only with ONE sample
    # is their order, and so the last bit of a float64 Hessian, the same from run to run of one build)
    cases = [("diag", 5, 16, False, 1), ("dense", 33, 16, False, 1), ("diag", 64, 128, False, 1), ("diag", 5, 16, True, 2), ("dense", 33, 16, True, 2),
             ("logreg2", 4, 1, True, 2), ("funnel", 8, 1, True, 2), ("logreg2", 4, 16, False, 1), ("funnel", 8, 16, False, 1)]
    for kind, d, n, second, order in cases:
        ctx, params = setup(dtype, avi.FULLRANK, d, n, kind, order=order)

        def run():
            l, g, H = ctx.gauss_expected_grad_hess(params, 7, n, second_order=second)
            ctx.synchronize()
            lh, gh, Hh = ctx.gauss_expected_grad_hess_host(params, 8, n, second_order=second)
            return dict(logpi=l, grad=g, hess=H.contiguous(), logpi_host=lh, grad_host=gh, hess_host=Hh)
        D.case(f"{dn}/grad_hess/{kind}/d{d}n{n}/{'order2' if second else 'stein'}", run)
        ctx.close()


def chunk_boundaries(D, dtype):
    dn = np.dtype(dtype).name
    d = 8
    for family, fn in FAMILIES:
        ctx, params = setup(dtype, family, d, 8, "diag")
        for n in (16384, 16385, 40000):
            def run():
                res = dict(objective=ctx.estimate_objective(params, 9, n), objective_mc=ctx.estimate_objective(params, 9, n, entropy=avi.MonteCarloEntropy.code))
                if family == avi.FULLRANK:
                    res["logpi"], res["grad"], H = ctx.gauss_expected_grad_hess(params, 9, n)
                    res["hess"] = H.contiguous()
                    res["logpi2"], res["grad2"], H2 = ctx.gauss_expected_grad_hess(params, 9, n, second_order=True)
                    res["hess2"] = H2.contiguous()
                    res["fisher"] = ctx.estimate_fisher(params, 9, n)
                    res["fisher_host"] = ctx.estimate_fisher_host(params, 9, n)
                ctx.synchronize()
                return res
            D.case(f"{dn}/chunks/{fn}/n{n}", run)
        ctx.close()
    # engine lanes plus a remainder (f32: 15 lanes of 128 and 80 samples through the walk, which starts at off0 = 1920; f64: the plain route)
    ctx, params = setup(dtype, avi.FULLRANK, 128, 128, "diag")
    D.case(f"{dn}/chunks/engine/d128n128s2000", lambda: dict(objective=ctx.estimate_objective(params, 9, 2000), objective_host=ctx.estimate_objective_host(params, 9, 2000)))
    ctx.close()


def optimiser_updates(D, dtype):
    dn = np.dtype(dtype).name
    for family, fn, d in ((avi.MEANFIELD, "mf", 5), (avi.FULLRANK, "fr", 5), (avi.FULLRANK, "fr", 128)):   # d = 128: 16512 parameters, the multi-workgroup DoG path
        ctx, params = setup(dtype, family, d, 8, "diag")
        rng = np.random.default_rng(40 + d)
        grad = ctx.to_device(rng.normal(size=params.size).astype(dtype))

        def run():
            res = {}
            p = ctx.to_device(params).clone()
            ctx.descent_update(p, grad, 1e-2)
            res["descent"] = p.clone()
            ctx.clip_scale(p, 0.9)
            res["clip"] = p.clone()
            ctx.prox_scale_entropy(p, 1e-2)
            res["prox"] = p.clone()
            st = ctx.empty(2 * p.numel()).zero_()
            for t in (1, 2):
                ctx.adam_update(p, grad, st, t, 1e-2)
            res["adam"], res["adam_state"] = p.clone(), st.clone()
            st = ctx.empty(5 * p.numel()).zero_()
            st[4 * p.numel():] = p
            for _ in range(2):
                ctx.cocob_update(p, grad, st)
            res["cocob"], res["cocob_state"] = p.clone(), st.clone()
            for kind in (0, 1):
                st = ctx.dog_state()
                ctx.dog_init(p, st, 1e-2)
                for _ in range(2):
                    ctx.dog_update(p, grad, st, kind)
                ctx.prox_scale_entropy(p, 0.0, st, kind)
                res[f"dog{kind}"], res[f"dog{kind}_state"] = p.clone(), st.clone()
            y = ctx.to_device(params).clone()
            ctx.axpby(y, 0.25, p, 0.75)
            res["axpby"] = y
            ctx.synchronize()
            return res
        D.case(f"{dn}/update/{fn}/d{d}", run)
        # the loop as a graph of launches or launch-free, whichever the library takes: rule x operator x PolynomialAveraging (launch_poly_average, the fused DoG tail)
        for rule, op, avg in (("descent", "clip", 1), ("adam", "clip", 1), ("cocob", "clip", 1), ("dog", "clip", 1), ("dowg", "prox", 1), ("dog", "none", 0), ("descent", "prox", 0)):
            D.case(f"{dn}/loop/{fn}/d{d}/{rule}-{op}-{avg}", lambda: loop(ctx, params, rule, op, avg, 3))
        ctx.close()


def loop(ctx, params, rule, op, avg, T, eta=1e-2):
    p = ctx.to_device(params).clone()
    st = None
    if rule == "adam":
        st = ctx.empty(2 * p.numel()).zero_()
    elif rule in ("dog", "dowg"):
        st = ctx.dog_state()
        ctx.dog_init(p, st, 1e-2)
    elif rule == "cocob":
        st = ctx.empty(5 * p.numel()).zero_()
        st[4 * p.numel():] = p
    ap = p.clone() if avg else None
    elbo = ctx.empty(T)
    ctx.optimize_loop(p, T, 70, 0, rule=RULES[rule], op=OPS[op], averager=avg, eta=100.0 if rule == "cocob" else eta, clip_epsilon=1e-5, opt_state=st, avg_params=ap, elbo=elbo)
    ctx.synchronize()
    res = dict(params=p, elbo=elbo)
    if st is not None:
        res["state"] = st
    if ap is not None:
        res["average"] = ap
    return res


def fused_loops(D, dtype):
    dn = np.dtype(dtype).name
    shapes = (("mf", avi.MEANFIELD, 64, 8, "diag"), ("mf_ragged", avi.MEANFIELD, 70, 19, "diag"), ("fr_small", avi.FULLRANK, 16, 8, "diag"), ("fr_rows", avi.FULLRANK, 40, 8, "diag"),
              ("lr_small", avi.MEANFIELD, 5, 8, "logreg0"), ("lr_small_fr", avi.FULLRANK, 5, 8, "logreg0"), ("mf_funnel", avi.MEANFIELD, 64, 8, "funnel"))
    for name, family, d, n, kind in shapes:
        ctx, params = setup(dtype, family, d, n, kind)
        for rule, op, avg in (("descent", "clip", 0), ("adam", "clip", 0), ("dog", "clip", 1), ("dowg", "prox", 1), ("cocob", "none", 0)):
            D.case(f"{dn}/fused/{name}/{rule}-{op}-{avg}", lambda: loop(ctx, params, rule, op, avg, 5, eta=1e-3 if kind == "funnel" else 1e-2))   # (the funnel diverges at 1e-2)

        def batch():   # estimates at fixed parameters: the launch-free batches of the mean-field routes
            p, v, g = ctx.to_device(params), ctx.empty(1), ctx.empty(ctx.params_len)
            ctx.estimate_gradient_n(p, 11, 5, v, g)
            vals, grads = ctx.estimate_gradient_each(p, 11, 5)
            ctx.synchronize()
            return dict(value=v, grad=g, values=vals, grads=grads)
        D.case(f"{dn}/fused/{name}/batch", batch)
        ctx.close()


def measure_space(D, dtype):
    dn = np.dtype(dtype).name
    for d in (5, 65):
        B = 8
        ctx, params = setup(dtype, avi.FULLRANK, d, B, "dense")

        def run():
            p = ctx.to_device(params).clone()
            st = ctx.bam_init(p)
            res = dict(init=st.clone())
            u, G, f, l, e = ctx.bam_moments(p, 13, B)
            res.update(u=u, G=G, fisher=f, logpi=l, elbo=e)
            uh, Gh, fh, lh, eh = ctx.bam_moments_host(params, 13, B)
            res.update(u_host=uh, G_host=Gh, fisher_host=fh, logpi_host=lh, elbo_host=eh)
            res["entropy"] = ctx.bam_update(p, st, u, G, B, float(d * B) / 3.0)
            res["params"], res["state"] = p.clone(), st.clone()
            ph, sh, enth = ctx.bam_update_host(params, host(res["init"]), uh, Gh, float(d * B) / 3.0)
            res.update(params_host=ph, state_host=sh, entropy_host=enth)
            fs, es = ctx.bam_steps(p, st, 20, 2, 3, B)
            ctx.synchronize()
            res.update(steps_fisher=fs, steps_elbo=es, steps_params=p, steps_state=st)
            return res
        D.case(f"{dn}/bam/d{d}", run)
        ctx.close()
    sub = {}
    for d in (5, 45, 65):   # the square-root and natural-gradient updates (one-workgroup and tile paths) and their _steps drivers
        MS.updates(sub, dtype, d)
    for second in (False, True):
        MS.steps(sub, dtype, 5, 10, second)
    D.out.update({f"ms/{k}": host(v).copy() for k, v in sub.items()})


def sharded(D, dtype):
    dn = np.dtype(dtype).name
    for family, fn, d in ((avi.MEANFIELD, "mf", 5), (avi.FULLRANK, "fr", 33)):
        ctx, params = setup(dtype, family, d, 8, "diag", entropy=avi.MonteCarloEntropy.code)

        def run():
            p = ctx.to_device(params)
            part = ctx.estimate_partials(p, 23)
            v, g = ctx.finalize(p, part)
            n = ctx.slice_len(1)
            padded = ctx.empty(n).zero_()
            padded[:ctx.partials_len] = part
            fin = ctx.finalize_slice(p, padded, 0, 1)
            v2, g2 = ctx.unpack_final(fin)
            ctx.synchronize()
            return dict(partials=part, value=v, grad=g, slice=fin, value_unpacked=v2, grad_unpacked=g2)
        D.case(f"{dn}/sharded/{fn}/d{d}", run)

        def p2p():   # the peer-to-peer exchange kernel at world 1
            ctx.p2p_attach([ctx.p2p_export(0, 1)])
            ctx.comm_set_route("p2p")
            v, g = ctx.estimate_gradient_dist(params, 24)
            ctx.synchronize()
            return dict(value=v, grad=g)
        D.case(f"{dn}/sharded/{fn}/d{d}/p2p", p2p)
        ctx.close()


def dump(path):
    D = Dump()
    for dtype in DTYPES:
        for part in (single_estimates, other_entries, chunk_boundaries, optimiser_updates, fused_loops, measure_space, sharded):
            part(D, dtype)
            print(f"{np.dtype(dtype).name} {part.__name__}: {len(D.out)} arrays so far", flush=True)
    np.savez(path, **{k: np.asarray(v) for k, v in D.out.items()})
    print(f"{len(D.out)} arrays ({sum(k.endswith('/refused') for k in D.out)} refusals) -> {path}")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    differ = [k for k in sorted(set(A.files) | set(B.files)) if k not in A.files or k not in B.files or not np.array_equal(A[k], B[k], equal_nan=A[k].dtype.kind == "f")]
    print(f"{len(A.files)} / {len(B.files)} arrays, {len(differ)} differ" + "".join(f"\n  {k}" for k in differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[1:3]) if len(sys.argv) > 2 else dump(sys.argv[1]))
