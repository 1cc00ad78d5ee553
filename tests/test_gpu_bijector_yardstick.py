"""The stacked-bijector kernels -- k_bijx_fwd / k_bijx_bwd / k_bijx_inv / k_bijx_fin (csrc/kernels_bijector.hip) and the legacy k_bij_fwd /
k_bij_bwd (csrc/kernels_targets.hip) -- held PER ENTRY to a float32 yardstick at the DEFAULT helper scales and on two wider classes
(tests/bijector_ref.py make_case: default, wide, far).  tests/test_gpu_bijector_kinds.py bounds the l2 distance of the whole gradient by 8 x
that of one float32 evaluation, both maximised over five estimates, on families whose scales are 0.4 x the helpers': a relative error of
1e-3 in a whole row of W passes that on nine of fourteen rows tried, and so does a backward pass that takes e^eta from x - lb on the class far
(tests/test_bijector_ref_host.py prints the figures).

Criterion (tests/bijector_ref.py): ref is the restatement in the next wider type (float64 for an f32 context, np.longdouble for f64) on
the device's own draws, S the first-order magnitude of every entry, u = 2^-24 / 2^-53, the factor F32_FACTOR = 8 of
tests/measure_space_cases.py.
    forward    ctx.sample_constrained on every layout x class x dtype (mean-field, M = 9): per entry |X - forward(eta)| <= 8 u S from the
               returned eta; X inside the closed bounds; X non-decreasing along every ordered block and strictly increasing wherever
               the reference, rounded to the element type, is (in f32 the class far has increments of 1e-3 next to a spacing of 0.06,
               so most of its rows tie).  The one exception is f64 on the class wide (e^-30 added to 1e13): the DOCUMENTED scan order
               (Hillis-Steele: every prefix a differently associated tree of at most log2(256) = 8 additions) is not monotone there
               in float64 numpy either -- tests/test_bijector_ref_host.py shows steps of -1 to -3 spacings on exactly the layouts 257,
               512 and 300 and none on default and far -- so there the assertion is step >= -8 spacings (the depth of the tree) and a
               strict increase wherever the reference's step exceeds the two neighbours' allowances 8 u S.  The device gave -1
               spacing on those three layouts; a tie and a decrease both answer -inf in logpdf_constrained
    eta = 0    a mean-field two-sided row with location 0 and the smallest positive scale of the element type: sigma eps rounds to 0 or
               to +- one spacing of zero, so the kernels meet eta = 0 exactly and both neighbours: `forward` on it, and `backward` with
               entropy kind 1 (no 1 / sigma anywhere in the gradient) at M = 33
    backward   a recording plugin on the host-callback route hands back a prescribed (ell_k, G[:, k]) (bijector_ref.graded_probe:
               |G| = 10^U(-3, 3), the signs alternating inside the ordered blocks).  The x it recorded is held per entry like `forward`
               (the only check of the forward kernel inside the estimate route: `save` set, `ld` written).  Mean-field, entropy kind 0,
               M = 1: grad[:d] = -W[:, 0] with nothing summed, per entry |W - backward(eta, G)| <= 8 u S; the value is
               -(ell + ladj + entropy), which holds ladj of the column.  M = 9, and the full-rank family at M = 1: bijector_ref.ratios
               against max(envelope of eight column orders, u S) -- dm per entry, dsigma per entry, dC per row and per 64-row block
    estimate   estimate_gradient on the device targets (bijector_ref.estimate_cases): the ratios and the value's ratio at most the
               factor, finite results, exact zeros above the diagonal of dC; on the class default the value also within VALUE_RTOL /
               TOL64 (the classes wide and far put x ~ 1e6 .. 1e13 in front of a target ten units away: the value's distance is the
               rounding of x, which the envelope carries and a fixed relative tolerance cannot)
    batch, descent   the last of five estimates of estimate_gradient_n, and one Descent step of optimize_steps with the gradient
               recovered as (p - p') / eta (eta = 2^12; 2^-24 |p'| / eta added to every denominator), at d = 257 on default
    inverse    ctx.logpdf_constrained at the X of `forward` (layouts 257 and 513 x {default, far} x both families x both dtypes), bitwise
               equal to logpdf_constrained_host; the stored points are exact, per column |got - ref| <= 8 max(|yard - ref|, u S) with yard
               = the float64 evaluation with eta rounded to the element type (bijector_ref.logpdf_yard); a column the reference finds
               outside the support (float32 points of far that tie with a bound or a neighbour) must be exactly -inf
    f64        every layout once per section.
    other      at d = 257 on default: the low-rank family (r = 5) by tests/lowrank_ref.py's own reference, envelope, magnitude and ratios
               around BijectorTarget; Laplace and TDist(5) by this file's criterion on the base's draws (closed-form entropy: the gradient
               is the Gaussian expression on U; tests/basedist_ref.py has no per-entry envelope and supplies the value's reference); the
               score estimator (it reads the bijector through log pi(x) + ladj alone) by bijector_ref.score_gradient / score_envelope /
               score_magnitude: the same ratios, dm per entry, and the value's and the elbo's
Each case prints `[bijector yardstick] route class layout family M ent: whole, block/row, entry, value`.  Every full-rank case asserts the
kernel generation it ran on (mivi_fullrank_route: 0, the first-generation kernels -- M = 33 and M = 1 are no multiples of 32).

Worst ratios measured on the MI355X per route (whole, block/row, entry, value), with the case that gave each (class layout family/target
M, entropy kind); forward and inverse have one number, in the column it belongs to:
    route             cases  whole  blk/row  entry  value   (worst cases)
    forward f32        40      -      -      1.33    -      (default 5; the row at eta = 0: 1.33)
    forward f64        40      -      -      2.95    -      (wide 512; the row at eta = 0: 1.42)
    backward f32      118     2.23   4.58    4.55   0.93    (default 300 fullrank M = 1, three times; wide 1-ordered fullrank M = 1;
                                                             the row at eta = 0: 0.89 1.48 1.33 0.31)
    backward f64       14     1.37   3.55    3.55   1.00    (default 1-lower; default legacy257, twice; default 1-identity;
                                                             the row at eta = 0: 0.97 1.00 1.42 0.75)
    estimate f32      188     2.62   3.37    5.28   1.11    (default 5 meanfield/diag M = 1 ent 3; default legacy257 meanfield/diag ent 3;
                                                             default legacy257 fullrank/diag ent 3; default 257 fullrank/diag ent 0)
    estimate f64       13     1.00   2.95    4.49   1.41    (default 1-lower; default legacy257 meanfield/diag ent 3; default 513 fullrank/diag
                                                             ent 0; default 1-lower)
    batch of five       2     1.09   1.90    2.90   1.11    (default 257 fullrank/diag)
    descent             2     0.95   1.27    1.86   1.11    (default 257 fullrank/diag; meanfield/diag; fullrank/diag, twice)
    inverse f32         8      -      -       -     0.45    (default 257 meanfield)
    inverse f64         8      -      -       -     0.77    (default 513 meanfield)
    low-rank r = 5      2     1.09   1.10    4.54   4.87    (default 257 ent 0, twice; ent 3; ent 0)
    Laplace             2     0.90   1.77    2.58   0.96    (default 257 fullrank/diag; meanfield/diag; fullrank/diag, twice)
    TDist(5)            2     0.97   3.09    3.07   0.80    (default 257 fullrank/diag)
    score               2     0.41   1.09    1.18   2.08    (default 257 fullrank/diag)
No ratio exceeds the factor (worst 5.28: an entry of dm behind the legacy kernels with the full-rank family, which had never been held per
entry); neither csrc/kernels_bijector.hip nor csrc/kernels_targets.hip had to change.  Per class, f32 (whole, block/row, entry, value):
backward default 2.23 4.58 4.55 0.53, wide 1.27 2.03 2.28 0.93, far 0.98 1.63 1.44 0.87; estimate default 2.62 3.37 5.28 1.11, wide 0.99 1.84
2.37 0.29, far 0.04 1.00 2.59 0.00; forward default 1.33, wide 1.12, far 0.95.  So the candidates that reading the code could not rule out
-- e^eta in the element type at |eta| near 30, the one rounding of the float64 scan under the graded probe, the two-sided row at
eta = +-1e-6 (all three in `wide`) and at eta = 0 exactly -- stay below 3; the default scales, which DESIGN.md called unheld, give the largest ratios.  The one
finding is the float64 order of `forward` above.
The whole file (441 cases) takes 8 seconds; the slowest case 0.2 s (the first, which loads the library, 1.8 s)."""
import zlib

import numpy as np
import pytest

import advancedvi_jl_amd as avi
from oracle import oracle as O
from tests import bijector_ref as BR
from tests.helpers import SEED
from tests.measure_space_cases import F32_FACTOR, TOL64, VALUE_RTOL

pytestmark = pytest.mark.gpu

IDX = 77
M_FWD = 9
_cases, _criteria = {}, {}
fam_id = lambda f: "meanfield" if f == avi.MEANFIELD else "fullrank"   # noqa: E731
dt_id = lambda t: "f32" if t == np.float32 else "f64"                  # noqa: E731


def _unit(dtype):
    return BR.U32 if dtype == np.float32 else BR.U64


def _case(cls, name, family, target, dtype):
    key = (cls, name, family, target, np.dtype(dtype).name)
    if key not in _cases:
        _cases[key] = BR.make_case(cls, name, family, target, dtype)
    return _cases[key]


def _problem(c, dtype):
    inner = c["inner"]
    if isinstance(inner, O.DiagNormalTarget):
        return avi.DiagNormalProblem(inner.mean.astype(dtype), inner.std.astype(dtype))
    return avi.DenseNormalProblem(inner.mean.astype(dtype), inner.L.astype(dtype))


def _context(c, dtype, M, ent, problem):
    ctx = avi.MiviContext(dtype, c["family"], c["d"], M, ent, SEED)
    if problem is not None:
        ctx.set_problem(problem)
    ctx.set_bijector(avi.StackedBijector(c["blocks"]))
    return ctx


def _hold_forward(what, blocks, eta, X, dtype, cls="default"):
    """X against forward(eta) in the wider type, per entry; the bounds and the order"""
    wide = BR.wider(dtype)
    ref, _ = BR.forward(blocks, eta.astype(wide), wide)
    Sx, _ = BR.magnitude_forward(blocks, eta)
    r = BR.entry_ratio(X, ref, Sx, _unit(dtype))
    assert np.all(np.isfinite(X)), what
    rounded = ref.astype(dtype)
    for lo, hi, kind, (lb, ub) in BR.normalise(blocks):
        if kind == "truncated":
            assert np.all(X[lo:hi] >= lb) and np.all(X[lo:hi] <= ub), (what, lo, hi)
        if kind == "ordered" and hi - lo >= 2:
            step = np.diff(X[lo:hi], axis=0)
            if dtype == np.float32 or cls != "wide":   # non-decreasing, and strictly increasing wherever the rounded reference is
                assert np.all(step >= 0) and np.all(step[np.diff(rounded[lo:hi], axis=0) > 0] > 0), (what, lo, hi)
            else:   # float64 on `wide`: the documented scan order itself is monotone only to the depth of its tree (module docstring, `forward`)
                room = F32_FACTOR * _unit(dtype) * (Sx[lo + 1:hi] + Sx[lo:hi - 1])
                assert np.all(step >= -np.log2(256) * np.spacing(np.abs(X[lo + 1:hi]))), (what, lo, hi)
                assert np.all(step[np.diff(ref[lo:hi], axis=0) > room] > 0), (what, lo, hi)
    return r


# ---- forward ---------------------------------------------------------------------------------------------------------------------------------
FORWARD = [(cls, name, dtype) for cls in BR.CLASSES for name in BR.LAYOUTS for dtype in (np.float32, np.float64)]


@pytest.mark.parametrize("cls,name,dtype", FORWARD, ids=[f"{c}-{n}-{dt_id(t)}" for c, n, t in FORWARD])
def test_forward(cls, name, dtype):
    c = _case(cls, name, avi.MEANFIELD, "diag", dtype)
    ctx = _context(c, dtype, M_FWD, 0, None)
    X, eta = ctx.sample_constrained(c["params"], IDX, want_eta=True)
    X, eta = X.cpu().numpy().copy(), eta.cpu().numpy().copy()
    ctx.close()
    r = _hold_forward(("forward", cls, name), c["blocks"], eta, X, dtype, cls)
    print(f"[bijector yardstick] forward-{dt_id(dtype)} {cls} {name} meanfield {M_FWD} ent0: 0.00, 0.00, {r:.2f}, 0.00")
    assert r <= F32_FACTOR, (cls, name, r)


def test_the_layouts_reach_the_mechanisms_they_are_listed_for():
    BR.assert_layouts_reach_their_mechanisms()


# ---- backward, isolated ------------------------------------------------------------------------------------------------------------------------
class ProbePlugin:
    """a LogDensityProblems plugin (host-callback route) that records the x of every call and hands back the next column of a table"""

    def __init__(self, d, ell, G):
        self.d, self.ell, self.G, self.seen = d, np.asarray(ell, dtype=np.float64), np.asarray(G, dtype=np.float64), []

    def dimension(self):
        return self.d

    def logdensity_and_gradient(self, x):
        k = len(self.seen)
        self.seen.append(np.array(x, dtype=np.float64))
        return float(self.ell[k]), self.G[:, k]


def run_backward(cls, name, family, M, dtype=np.float32, ent=0, c=None):
    c = _case(cls, name, family, "diag", dtype) if c is None else c
    d, blocks, u = c["d"], c["blocks"], _unit(dtype)
    ell, G = BR.graded_probe(d, blocks, M, np.random.default_rng(zlib.crc32(f"{cls} {name} {M}".encode())), dtype)
    plugin = ProbePlugin(d, ell, G)
    ctx = _context(c, dtype, M, ent, plugin)
    p = ctx.to_device(c["params"])
    eta, eps = ctx.sample(p, IDX)
    eta, eps = eta.cpu().numpy().copy(), eps.cpu().numpy().copy()
    v, g = ctx.estimate_gradient(p, IDX)
    ctx.synchronize()
    v, g = float(v.item()), g.cpu().numpy().copy()
    ctx.close()
    assert len(plugin.seen) == M and np.all(np.isfinite(g)) and np.isfinite(v)
    seen = np.stack(plugin.seen, axis=1)
    rx = _hold_forward(("backward: recorded x", cls, name), blocks, eta, seen.astype(dtype), dtype, cls)   # column k of the table met column k of the draws
    args = (c["params"], d, family, None, blocks, eps, ent)
    wide = BR.wider(dtype)
    ref = BR.gradient(*args, wide, probe=(ell, G))
    env, mag = BR.envelope(*args, dtype, ref, probe=(ell, G)), BR.magnitude(*args, probe=(ell, G))
    r = BR.ratios(g, env["grad"], ref["grad"], mag["grad"], d, family, u)
    vr = BR.value_ratio(v, env["value"], ref["value"], mag["value"], u)
    rw = 0.0
    if M == 1 and family == avi.MEANFIELD and ent == 0:   # nothing is summed: W itself, against u S alone
        rw = BR.entry_ratio(-g[:d], BR.backward(blocks, eta.astype(wide), G.astype(wide), wide)[:, 0], BR.magnitude_backward(blocks, eta, G)[:, 0], u)
        _, Sl = BR.magnitude_forward(blocks, eta)
        sig = np.abs(c["params"][d:].astype(np.float64))
        vr = max(vr, BR.value_ratio(v, 0.0, ref["value"], abs(float(ell[0])) + Sl[0] + 0.5 * d * (1.0 + BR.LOG2PI) + np.sum(np.abs(np.log(sig))), u))
    print(f"[bijector yardstick] backward-{dt_id(dtype)} {cls} {name} {fam_id(family)} {M} ent{ent}: {r['whole']:.2f}, {max(r['block'], r['row']):.2f}, "
          f"{max(r['entry'], rw, rx):.2f}, {vr:.2f}")
    assert max(max(r.values()), rw, rx, vr) <= F32_FACTOR, (cls, name, family, M, r, rw, rx, vr)
    return eta


BACKWARD = [(cls, name, fam, M) for cls in BR.CLASSES for name in BR.LAYOUTS for fam, M in ((avi.MEANFIELD, 1), (avi.MEANFIELD, 9), (avi.FULLRANK, 1))]


@pytest.mark.parametrize("cls,name,family,M", BACKWARD, ids=[f"{c}-{n}-{fam_id(f)}-{M}" for c, n, f, M in BACKWARD])
def test_backward_isolated_by_a_recording_plugin(cls, name, family, M):
    run_backward(cls, name, family, M)


@pytest.mark.parametrize("name", list(BR.LAYOUTS))
def test_backward_isolated_f64(name):
    run_backward("default", name, avi.MEANFIELD, 9, np.float64)


# ---- eta = 0 exactly, and +- one spacing of zero -----------------------------------------------------------------------------------------------
def _zero_case(dtype):
    """layout 5 on default with row 3 (truncated(-1, 2)) at location 0 and the smallest positive scale of the element type"""
    c = dict(_case("default", "5", avi.MEANFIELD, "diag", dtype))
    params = c["params"].copy()
    params[3], params[c["d"] + 3] = 0.0, np.spacing(dtype(0.0))
    c["params"] = params
    return c


def _assert_reaches_zero(eta, dtype):
    tiny = np.spacing(dtype(0.0))
    assert {-tiny, dtype(0.0), tiny} <= set(np.unique(eta[3])) and np.max(np.abs(eta[3])) <= 8 * tiny, np.unique(eta[3])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=dt_id)
def test_forward_at_eta_zero(dtype):
    c = _zero_case(dtype)
    ctx = _context(c, dtype, BR.M_EST, 0, None)
    X, eta = ctx.sample_constrained(c["params"], IDX, want_eta=True)
    X, eta = X.cpu().numpy().copy(), eta.cpu().numpy().copy()
    ctx.close()
    _assert_reaches_zero(eta, dtype)
    r = _hold_forward(("forward at eta = 0",), c["blocks"], eta, X, dtype)
    print(f"[bijector yardstick] forward-{dt_id(dtype)} zero 5 meanfield {BR.M_EST} ent0: 0.00, 0.00, {r:.2f}, 0.00")
    assert r <= F32_FACTOR and np.all(X[3][eta[3] == 0] == dtype(0.5))   # (the midpoint of (-1, 2), exactly)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=dt_id)
def test_backward_at_eta_zero(dtype):
    _assert_reaches_zero(run_backward("zero", "5", avi.MEANFIELD, BR.M_EST, dtype, ent=1, c=_zero_case(dtype)), dtype)


# ---- estimate -----------------------------------------------------------------------------------------------------------------------------------
def _criterion(c, cls, name, target, M, ent, dtype, eps):
    """(ref, env, S) of the estimate IDX of one setup, computed once and left unchanged; a second route must have drawn the same numbers"""
    key = (cls, name, c["family"], target, M, ent, np.dtype(dtype).name)
    if key not in _criteria:
        args = (c["params"], c["d"], c["family"], c["inner"], c["blocks"], eps, ent)
        ref = BR.gradient(*args, BR.wider(dtype), order=np.arange(M))
        _criteria[key] = (zlib.crc32(eps.tobytes()), ref, BR.envelope(*args, dtype, ref), BR.magnitude(*args))
    assert _criteria[key][0] == zlib.crc32(eps.tobytes()), "the draws of this estimate differ between two routes"
    return _criteria[key][1:]


def _hold(route, c, cls, name, target, M, ent, dtype, eps, value, grad, extra=None, note=""):
    d, family, u = c["d"], c["family"], _unit(dtype)
    ref, env, mag = _criterion(c, cls, name, target, M, ent, dtype, eps)
    g = np.asarray(grad)
    r = BR.ratios(g, env["grad"], ref["grad"], mag["grad"], d, family, u, extra)
    vr = BR.value_ratio(value, env["value"], ref["value"], mag["value"], u)
    print(f"[bijector yardstick] {route}-{dt_id(dtype)} {cls} {name} {fam_id(family)}/{target} {M} ent{ent}{note}: {r['whole']:.2f}, "
          f"{max(r['block'], r['row']):.2f}, {r['entry']:.2f}, {vr:.2f}")
    assert np.all(np.isfinite(g)) and np.isfinite(float(value))
    if family == avi.FULLRANK:
        assert np.all(np.triu(g[d:].reshape(d, d, order="F"), 1) == 0.0)
    if cls == "default":
        vtol = VALUE_RTOL if dtype == np.float32 else TOL64[0]
        assert abs(float(value) - float(ref["value"])) <= vtol * max(abs(float(ref["value"])), 1.0), (float(value), float(ref["value"]))
    assert max(max(r.values()), vr) <= F32_FACTOR, (route, cls, name, family, target, M, ent, r, vr)


def run_estimate(cls, name, family, target, ent, M, dtype=np.float32):
    c = _case(cls, name, family, target, dtype)
    ctx = _context(c, dtype, M, ent, _problem(c, dtype))
    p = ctx.to_device(c["params"])
    eps = ctx.sample(p, IDX)[1].cpu().numpy().copy()
    v, g = ctx.estimate_gradient(p, IDX)
    ctx.synchronize()
    v, g = float(v.item()), g.cpu().numpy().copy()
    note = ""
    if family == avi.FULLRANK:   # M = 33 / M = 1: no multiple of 32, the first-generation full-rank kernels (generation 0 of mivi_fullrank_route)
        assert ctx.fullrank_route()[0] == 0
        note = " gen0"
    ctx.close()
    _hold("estimate", c, cls, name, target, M, ent, dtype, eps, v, g, note=note)


ESTIMATE = BR.estimate_cases()


@pytest.mark.parametrize("cls,name,family,target,ent,M", ESTIMATE, ids=[f"{c}-{n}-{fam_id(f)}-{t}-ent{e}-{M}" for c, n, f, t, e, M in ESTIMATE])
def test_estimate_on_device_targets(cls, name, family, target, ent, M):
    run_estimate(cls, name, family, target, ent, M)


ESTIMATE_F64 = [(name, (avi.MEANFIELD, avi.FULLRANK)[k % 2], ("diag", "dense")[(k // 2) % 2], (0, 3)[(k // 4) % 2]) for k, name in enumerate(BR.LAYOUTS)]


@pytest.mark.parametrize("name,family,target,ent", ESTIMATE_F64, ids=[f"{n}-{fam_id(f)}-{t}-ent{e}" for n, f, t, e in ESTIMATE_F64])
def test_estimate_f64(name, family, target, ent):
    run_estimate("default", name, family, target, ent, BR.M_EST, np.float64)


# ---- the last of five estimates of a batch; one Descent step -------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", BR.FAMILIES, ids=fam_id)
def test_last_estimate_of_a_batch_of_five(family):
    cls, name, target, ent, M, dtype = "default", "257", "diag", 0, BR.M_EST, np.float32
    c = _case(cls, name, family, target, dtype)
    ctx = _context(c, dtype, M, ent, _problem(c, dtype))
    p = ctx.to_device(c["params"])
    eps = ctx.sample(p, IDX)[1].cpu().numpy().copy()
    v, g = ctx.empty(1), ctx.empty(ctx.params_len)
    ctx.estimate_gradient_n(p, IDX - 4, 5, v, g)
    ctx.synchronize()
    vh, gh = float(v.item()), g.cpu().numpy().copy()
    ctx.close()
    _hold("batch[5]", c, cls, name, target, M, ent, dtype, eps, vh, gh)


@pytest.mark.parametrize("family", BR.FAMILIES, ids=fam_id)
def test_one_descent_step(family):
    cls, name, target, ent, M, dtype, eta = "default", "257", "diag", 0, BR.M_EST, np.float32, 2.0 ** 12
    c = _case(cls, name, family, target, dtype)
    ctx = _context(c, dtype, M, ent, _problem(c, dtype))
    p = ctx.to_device(c["params"]).clone()
    eps = ctx.sample(p, IDX)[1].cpu().numpy().copy()
    elbo = ctx.empty(1)
    ctx.optimize_steps(p, None, IDX, 0, 1, 0, eta, 0.0, elbo)   # (rule 0: Descent; clip_epsilon <= 0: no ClipScale)
    ctx.synchronize()
    after = p.cpu().numpy().astype(np.float64)
    value = -float(elbo.item())
    ctx.close()
    g = (c["params"].astype(np.float64) - after) / eta
    _hold("descent", c, cls, name, target, M, ent, dtype, eps, value, g, extra=BR.U32 * np.abs(after) / eta)


# ---- inverse --------------------------------------------------------------------------------------------------------------------------------------
INVERSE = [(cls, name, fam, dtype) for cls in ("default", "far") for name in ("257", "513") for fam in BR.FAMILIES for dtype in (np.float32, np.float64)]


@pytest.mark.parametrize("cls,name,family,dtype", INVERSE, ids=[f"{c}-{n}-{fam_id(f)}-{dt_id(t)}" for c, n, f, t in INVERSE])
def test_inverse(cls, name, family, dtype):
    c = _case(cls, name, family, "diag", dtype)
    d, blocks, u = c["d"], c["blocks"], _unit(dtype)
    ctx = _context(c, dtype, M_FWD, 0, None)
    p = ctx.to_device(c["params"])
    X = ctx.sample_constrained(p, IDX).cpu().numpy().copy()
    got = ctx.logpdf_constrained(p, X).cpu().numpy().copy()
    got_h = ctx.logpdf_constrained_host(c["params"], X)
    ctx.close()
    assert np.array_equal(got, got_h, equal_nan=True)
    wide = BR.wider(dtype)
    ref = BR.logpdf_constrained(c["params"], d, family, blocks, X.astype(wide), wide)
    yard = BR.logpdf_yard(c["params"], d, family, blocks, X, dtype)
    inside = np.isfinite(np.asarray(ref, dtype=np.float64))
    assert np.all(got[~inside] == -np.inf) and np.all(np.isfinite(got[inside])), (cls, name, got, inside)
    Sp = BR.magnitude_logpdf_constrained(c["params"], d, family, blocks, X)
    r = BR.entry_ratio(got[inside], ref[inside], Sp[inside], u, env=np.abs(yard[inside].astype(wide) - ref[inside]))
    print(f"[bijector yardstick] inverse-{dt_id(dtype)} {cls} {name} {fam_id(family)} {M_FWD} ent0 inside {int(inside.sum())}/{M_FWD}: 0.00, 0.00, 0.00, {r:.2f}")
    assert r <= F32_FACTOR, (cls, name, family, r)


# ---- other routes behind the same kernels, d = 257 on default -------------------------------------------------------------------------------------
def test_low_rank_family():
    """r = 5: tests/lowrank_ref.py's own reference, envelope, magnitude and ratios (whole, 64-row block, entry) around BijectorTarget"""
    from tests import lowrank_ref as LR
    name, r, M, dtype = "257", 5, BR.M_EST, np.float32
    d, blocks = BR.LAYOUTS[name]
    rng = np.random.default_rng(257 + r)
    mu, D, U, m, s = LR.classes("default", d, r, rng)
    params = LR.flat(mu, D, U, dtype)
    m, s = m.astype(dtype), s.astype(dtype)
    tgt = BR.BijectorTarget(O.DiagNormalTarget(m, s), blocks)
    for ent in (0, 3):
        ctx = avi.MiviContext(dtype, avi.LOWRANK, d, M, ent, SEED, rank=r)
        ctx.set_problem(avi.TransformedProblem(avi.DiagNormalProblem(m, s), avi.StackedBijector(blocks)))
        p = ctx.to_device(params)
        eps = ctx.sample(p, IDX)[1].cpu().numpy().copy()
        v, g = ctx.estimate_gradient(p, IDX)
        ctx.synchronize()
        v, g = float(v.item()), g.cpu().numpy().copy()
        ctx.close()
        ref = LR.reference(params, d, r, tgt, eps, ent, np.float64)
        env, mag = LR.envelope(params, d, r, tgt, eps, ent, dtype, ref), LR.magnitude(params, d, r, tgt, eps, ent)
        whole, block, entry = LR.ratios(g, env["grad"], ref["grad"], mag["grad"], d, r, BR.U32)
        vr = LR.value_ratio(v, env["value"], ref["value"], mag["value"], BR.U32)
        print(f"[bijector yardstick] lowrank-f32 default {name} lowrank{r}/diag {M} ent{ent}: {whole:.2f}, {block:.2f}, {entry:.2f}, {vr:.2f}")
        assert np.all(np.isfinite(g)) and abs(v - float(ref["value"])) <= VALUE_RTOL * max(abs(float(ref["value"])), 1.0)
        assert max(whole, block, entry, vr) <= F32_FACTOR, (ent, whole, block, entry, vr)


@pytest.mark.parametrize("family", BR.FAMILIES, ids=fam_id)
@pytest.mark.parametrize("dist", [avi.Laplace(), avi.TDist(5.0)], ids=repr)
def test_non_normal_bases(dist, family):
    """Laplace and TDist(5), closed-form entropy: with W = G the gradient is the Gaussian expression on the base's own draws U (only the value's
    entropy term knows the base), so it is held by THIS file's envelope, magnitude and ratios with eps := U -- tests/basedist_ref.py has no
    per-entry envelope; the value is held by its estimate_gradient in float64 with this file's envelope and magnitude"""
    from tests import basedist_ref as B
    cls, name, target, ent, M, dtype = "default", "257", "diag", 0, BR.M_EST, np.float32
    c = _case(cls, name, family, target, dtype)
    d = c["d"]
    ctx = avi.MiviContext(dtype, family, d, M, ent, SEED)
    ctx.set_base_dist(dist)
    ctx.set_problem(_problem(c, dtype))
    ctx.set_bijector(avi.StackedBijector(c["blocks"]))
    p = ctx.to_device(c["params"])
    U = ctx.sample(p, IDX)[1].cpu().numpy().copy()
    v, g = ctx.estimate_gradient(p, IDX)
    ctx.synchronize()
    v, g = float(v.item()), g.cpu().numpy().copy()
    ctx.close()
    args = (c["params"], d, family, c["inner"], c["blocks"], U, ent)
    ref = BR.gradient(*args, np.float64, order=np.arange(M))
    env, mag = BR.envelope(*args, dtype, ref), BR.magnitude(*args)
    r = BR.ratios(g, env["grad"], ref["grad"], mag["grad"], d, family, BR.U32)
    vref = B.estimate_gradient(c["params"].astype(np.float64), d, family, BR.BijectorTarget(c["inner"], c["blocks"]), U.astype(np.float64), ent, B.base_of(dist))
    assert np.linalg.norm(vref["grad"] - ref["grad"]) <= 1e-11 * np.linalg.norm(ref["grad"])   # (the two float64 references agree on the gradient)
    vr = BR.value_ratio(v, env["value"], vref["value"], mag["value"], BR.U32)
    print(f"[bijector yardstick] {dist!r}-f32 {cls} {name} {fam_id(family)}/{target} {M} ent{ent}: {r['whole']:.2f}, {max(r['block'], r['row']):.2f}, {r['entry']:.2f}, {vr:.2f}")
    assert np.all(np.isfinite(g)) and abs(v - vref["value"]) <= VALUE_RTOL * max(abs(vref["value"]), 1.0)
    assert max(max(r.values()), vr) <= F32_FACTOR, (dist, family, r, vr)


@pytest.mark.parametrize("family", BR.FAMILIES, ids=fam_id)
def test_score_gradient_estimator(family):
    """ScoreGradELBO reads the bijector through the VALUES log pi(x) + ladj alone (k_bijx_fwd; the backward kernel adds ld to ell and no
    more).  tests/scoregrad_ref.py has no per-entry envelope, so this file's is used: bijector_ref.score_gradient in float64 is the
    reference, score_envelope the eight column orders of its float32 evaluation, score_magnitude the floor -- dm per entry, dsigma per
    entry or dC per row and block, whole, and the value's and the elbo's ratios."""
    cls, name, target, M, dtype = "default", "257", "diag", BR.M_EST, np.float32
    c = _case(cls, name, family, target, dtype)
    d = c["d"]
    ctx = _context(c, dtype, M, 0, _problem(c, dtype))
    p = ctx.to_device(c["params"])
    eps = ctx.sample(p, IDX)[1].cpu().numpy().copy()
    v, e, g = ctx.estimate_score_gradient(p, IDX)
    ctx.synchronize()
    v, e, g = float(v.item()), float(e.item()), g.cpu().numpy().copy()
    ctx.close()
    args = (c["params"], d, family, c["inner"], c["blocks"], eps)
    ref = BR.score_gradient(*args, np.float64)
    env, mag = BR.score_envelope(*args, dtype, ref), BR.score_magnitude(*args)
    r = BR.ratios(g, env["grad"], ref["grad"], mag["grad"], d, family, BR.U32)
    rv, re = BR.value_ratio(v, env["value"], ref["value"], mag["value"], BR.U32), BR.value_ratio(e, env["elbo"], ref["elbo"], mag["elbo"], BR.U32)
    print(f"[bijector yardstick] score-f32 {cls} {name} {fam_id(family)}/{target} {M} ent0: {r['whole']:.2f}, {max(r['block'], r['row']):.2f}, {r['entry']:.2f}, {max(rv, re):.2f}")
    assert np.all(np.isfinite(g)) and max(max(r.values()), rv, re) <= F32_FACTOR, (family, r, rv, re)
