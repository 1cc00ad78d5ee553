"""CPU-side checks of the boundary: the C-ABI library loads without a GPU and exports every symbol
include/mivi.h declares; the host-side RNG restatement inside the library matches the numpy oracle
bit-exactly; host-side mirror logic (families, constructors, error behaviour).  No GPU compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import _lib
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "mivi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mivi_[a-z0-9_]+)\s*\(", src)) - {"mivi_logdensity_and_gradient_fn", "mivi_logdensity_fn"})


def test_library_loads_and_exports_every_declared_symbol(lib):
    names = header_functions()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"libmivi.so does not export {n}"
        assert n in _lib.SIGNATURES, f"{n} is declared in mivi.h but not bound in _lib.SIGNATURES"
    for n in _lib.SIGNATURES:
        assert n in names, f"{n} is bound but not declared in include/mivi.h"
    assert lib.mivi_version() == 1


def _c_class(decl):
    """coarse class of a C parameter / return declaration of include/mivi.h"""
    t = decl.strip()
    if "*" in t or "[" in t or t.startswith("mivi_logdensity"):
        return "ptr"
    for key, cls in (("uint64_t", "u64"), ("int64_t", "i64"), ("int32_t", "i32"), ("mivi_status_t", "i32"), ("double", "f64"), ("void", "void")):
        if re.search(r"\b" + key + r"\b", t):
            return cls
    raise AssertionError(f"unclassified C declaration: {decl!r}")


def _jl_class(t):
    """the same classes for a Julia ccall type"""
    t = t.strip()
    if t.startswith(("Ptr{", "Ref{")) or t in ("Any", "Cstring", "Ptr"):
        return "ptr"
    return {"Int32": "i32", "Cint": "i32", "UInt64": "u64", "Int64": "i64", "Float64": "f64", "Cdouble": "f64", "Cvoid": "void"}[t]


def header_signatures():
    """name -> (return class, [parameter classes]) from include/mivi.h"""
    src = open(os.path.join(ROOT, "include", "mivi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[ \*]+)(mivi_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        if name.endswith("_fn") or "typedef" in ret:
            continue
        out[name] = (_c_class(ret), [] if args in ("", "void") else [_c_class(a) for a in args.split(",")])
    return out


def header_prototypes():
    """name -> number of parameters, from include/mivi.h (comments stripped)."""
    src = open(os.path.join(ROOT, "include", "mivi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(mivi_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        name, args = m.group(1), m.group(2).strip()
        if name.endswith("_fn"):
            continue
        out[name] = 0 if args in ("", "void") else len(args.split(","))
    return out


def test_julia_wrapper_ccalls_match_the_header():
    """julia/MIVI.jl cannot be executed here (no Julia in the image); what can be checked is that every ccall names an entry
    point include/mivi.h declares and passes as many arguments as the prototype has, with an argument-type tuple of that length."""
    protos = header_prototypes()
    sigs = header_signatures()
    txt = open(os.path.join(ROOT, "advancedvi.jl_amd", "julia", "MIVI.jl")).read()
    calls = list(re.finditer(r"ccall\(\(:(mivi_[a-z0-9_]+),\s*libmivi\),\s*(\w+),\s*\(", txt))
    assert len(calls) >= 12
    seen = set()
    for m in calls:
        name = m.group(1)
        assert name in protos, f"MIVI.jl calls {name}, which include/mivi.h does not declare"
        # the argument-type tuple: balanced parentheses starting at the '(' the regex ended on
        i = m.end() - 1
        depth, j = 0, i
        while True:
            depth += txt[j] == "("
            depth -= txt[j] == ")"
            if depth == 0:
                break
            j += 1
        tup = txt[i + 1:j]
        parts, depth, cur = [], 0, ""
        for ch in tup:
            if ch in "({":
                depth += 1
            if ch in ")}":
                depth -= 1
            if ch == "," and depth == 0:
                parts.append(cur)
                cur = ""
            else:
                cur += ch
        if cur.strip():
            parts.append(cur)
        assert len(parts) == protos[name], f"{name}: {len(parts)} argument types in MIVI.jl, {protos[name]} parameters in mivi.h"
        # ... and every argument (and the return value) is of the prototype's class: pointer / int32 / int64 / uint64 / double
        ret_c, par_c = sigs[name]
        assert _jl_class(m.group(2)) == ret_c, f"{name}: returns {m.group(2)} in MIVI.jl, {ret_c} in mivi.h"
        for k, (jt, cc) in enumerate(zip(parts, par_c)):
            assert _jl_class(jt) == cc, f"{name}: argument {k} is {jt.strip()} in MIVI.jl, {cc} in mivi.h"
        seen.add(name)
    for must in ("mivi_create", "mivi_destroy", "mivi_set_target_callback", "mivi_estimate_gradient_host", "mivi_estimate_objective_host",
                 "mivi_set_bijector_stacked", "mivi_comm_unique_id", "mivi_comm_init", "mivi_estimate_gradient_dist",
                 "mivi_gauss_expected_grad_hess_host", "mivi_gauss_expected_grad_hess2_host", "mivi_set_target_hess_callback", "mivi_logreg_select_rows", "mivi_optimize_loop", "mivi_set_target_diag_gauss",
                 "mivi_set_target_dense_gauss", "mivi_set_target_funnel", "mivi_comm_enable_p2p", "mivi_estimate_gradient_dist_n"):
        assert must in seen, f"MIVI.jl does not bind {must}"


def test_config_struct_layout_matches_header():
    # int32 x6, uint64, int32 x2, void*, int32 x2  (natural alignment)
    assert C.sizeof(_lib.MiviConfig) == 56
    assert _lib.MiviConfig.seed.offset == 24 and _lib.MiviConfig.stream.offset == 40


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libmivi.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.load()


def test_no_gpu_means_error_not_fallback(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        avi.MiviContext(np.float32, avi.MEANFIELD, 4, 4, 0, 1)
    cfg = _lib.MiviConfig(0, 0, 4, 4, 0, 0, 1, 0, 0, None, 0, 0)
    h = C.c_void_p()
    assert lib.mivi_create(C.byref(cfg), C.byref(h)) == _lib.ERR_HIP


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "advancedvi.jl_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".jl")):
                txt = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", txt, flags=re.M), f
                assert "libmivi_oracle" not in txt and "mivi_oracle.c" not in txt, f


def test_graph_capture_has_one_owner():
    """Stream capture, instantiation and the intermediate hipGraph_t live in ONE translation unit (csrc/api_graph.hip); the routes name
    neither them nor the capture stream, and the cache key is typed (no integer kinds, nothing packed into a double)."""
    csrc = os.path.join(ROOT, "advancedvi.jl_amd", "csrc")
    hip = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(".hip")}
    owners = {tok: [f for f, txt in hip.items() if tok in txt]
              for tok in ("hipStreamBeginCapture", "hipStreamEndCapture", "hipGraphInstantiate", "hipGraphDestroy(")}
    assert all(len(fs) == 1 for fs in owners.values()), owners
    assert len({fs[0] for fs in owners.values()}) == 1, owners
    owner = owners["hipStreamBeginCapture"][0]
    for f, txt in hip.items():
        lines = [ln for ln in txt.splitlines() if "cap_stream" in ln]
        if f == owner:
            assert lines, f
        else:   # (the context's destruction releases it without naming it: the member is a Stream)
            assert not lines, (f, lines)
    abi = [(f, txt) for f, txt in hip.items() if f.startswith("api_")]   # (the kernels have `kind`s of their own)
    for f, txt in abi + [(h, open(os.path.join(csrc, h)).read()) for h in ("api_common.h", "mivi_internal.h")]:
        assert not re.search(r"\bkind\s*(==|!=|=)\s*\d", txt), f
        assert not re.search(r"\bbegin_capture\b|\bend_capture\b", txt), f
    internal = open(os.path.join(csrc, "mivi_internal.h")).read()
    cache = re.search(r"struct GraphKey \{.*?\n\};.*?struct GraphCache \{.*?\n\};", internal, flags=re.S).group(0)
    assert not re.search(r"\b(p0|p1|aux0|aux1)\b", cache), cache


def test_environment_switches_have_one_table():
    """The environment is read in ONE translation unit (csrc/api_core.hip: kSwitchTable behind switches(), csrc/switches.h).  The table, the
    switch paragraph of DESIGN.md and the cases of tests/test_gpu_ab_switches.py name the same switches, and the switches retired with the
    routes only they reached are named nowhere in the sources, tests and tools."""
    csrc = os.path.join(ROOT, "advancedvi.jl_amd", "csrc")
    src = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    assert [f for f, txt in src.items() if "getenv(" in txt] == ["api_core.hip"]
    table = re.search(r"const SwitchRow kSwitchTable\[\] = \{\n(.*?)\n\};", src["api_core.hip"], flags=re.S).group(1)
    release, dev = table.split("#ifdef MIVI_DEV")
    row = r'\{"(MIVI_\w+)", SW_\w+, SW\(\w+\), [^"]*"[^"]+"\}'
    release, dev = re.findall(row, release), re.findall(row, dev)
    names = set(release) | set(dev)
    assert len(release) + len(dev) == len(names) == table.count('{"'), table   # (every row parsed, no name twice)
    assert set(dev) == {"MIVI_FB_DBG", "MIVI_FB_KNOCK", "MIVI_FB_RING", "MIVI_KNOCK", "MIVI_STL_STAMPS"}
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    para = re.search(r"\*\*Environment switches\.\*\*.*?(\n\n|\Z)", design, flags=re.S).group(0)
    kept, cut = para.split("Cut in round 5")
    assert set(re.findall(r"`(MIVI_\w+)`", kept)) - {"MIVI_DEV"} == names, sorted(set(re.findall(r"`(MIVI_\w+)`", kept)) ^ names)
    retired = ["MIVI_" + n for n in ("FR_F32MFMA", "F64_VALU", "LR_F32_XTR", "LOGREG_GENERIC", "LOGREG_MFMA")]   # (in pieces: this file is searched too)
    assert set(retired) <= set(re.findall(r"`(MIVI_\w+)`", cut)), cut
    import tests.test_gpu_ab_switches as ab
    tested = {kv.split("=")[0] for c in ab.CASES if c for kv in c[0].split(",")}
    untested = set(release) - {"MIVI_FORCE_EXCHANGE_LOST", "MIVI_RCCL_LIB"} - tested
    assert not untested, sorted(untested)
    tools = os.path.join(ROOT, "tools")
    searched = [os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))]
    searched += [os.path.join(ROOT, "tests", f) for f in sorted(os.listdir(os.path.join(ROOT, "tests"))) if f.endswith(".py")]
    searched += [os.path.join(tools, f) for f in sorted(os.listdir(tools)) if f.endswith((".py", ".sh"))]
    for path in searched:
        txt = open(path).read()
        assert not [n for n in retired if n in txt], path


def test_stream_and_event_handles_have_one_owner():
    """Streams and events are created and destroyed in ONE translation unit (csrc/api_core.hip: make_stream, make_event, handle_destroy),
    a hipGraphExec is destroyed in the graph unit only; every other unit holds them in a Stream / Event / GraphExec (csrc/mivi_internal.h).
    No unit but api_core.hip assigns a context's stream (StreamScope and LaneScope of api_common.h do it for a scope), and the context
    keeps no own_stream flag: the name survives as the mivi_config_t field."""
    csrc = os.path.join(ROOT, "advancedvi.jl_amd", "csrc")
    hip = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(".hip")}
    owner_of = {"hipStreamCreate": "api_core.hip", "hipExtStreamCreateWithCUMask": "api_core.hip", "hipStreamDestroy": "api_core.hip",
                "hipEventCreate": "api_core.hip", "hipEventDestroy": "api_core.hip", "hipGraphExecDestroy": "api_graph.hip",
                "->stream = ": "api_core.hip"}
    for tok, owner in owner_of.items():
        named_in = [f for f, txt in hip.items() if tok in txt]
        assert named_in == [owner], (tok, named_in)
    for f, txt in hip.items():
        stray = [ln for ln in txt.splitlines() if re.search(r"(?<!cfg\.)(?<!cfg->)\bown_stream\b", ln)]
        assert not stray, (f, stray)


def test_precision_dispatch_is_written_once():
    """A kernel that exists for float and double is launched through by_dtype (csrc/mivi_internal.h), where its name carries the element
    type as a template parameter.  Only a launcher whose two precisions take different routes may name `k_x<float` and `k_x<double`."""
    csrc = os.path.join(ROOT, "advancedvi.jl_amd", "csrc")
    src = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(".hip"))
    both = set(re.findall(r"\b(k_\w+)<float", src)) & set(re.findall(r"\b(k_\w+)<double", src))
    assert both == {
        # launch_fr_stl (kernels_fullrank.hip): the 16-column solve is taken by f64 only within its own LDS bound (d <= 1024; f32:
        # d <= 2304), so each precision tests for its route and prepares its transposed scale there
        "k_stl_prep",
        "k_stl_solve_la16",
    }, sorted(both)


def test_host_philox_matches_oracle_bit_exact(lib):
    rng = np.random.default_rng(0)
    for _ in range(50):
        ctr = rng.integers(0, 2 ** 32, size=4, dtype=np.uint64).astype(np.uint32)
        key = rng.integers(0, 2 ** 32, size=2, dtype=np.uint64).astype(np.uint32)
        out = (C.c_uint32 * 4)()
        lib.mivi_philox4x32_10((C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), out)
        assert list(out) == [int(x) for x in O.philox4x32_10(ctr, (int(key[0]), int(key[1])))]


@pytest.mark.parametrize("d", [1, 4, 7, 37, 64])
def test_host_eps_stream_matches_oracle(lib, d):
    seed, idx, M = 0x38BEF07CF9CC549D, 12345678901, 9
    ref_bits = O.philox_bits(seed, idx, d, 3, 3 + M)
    for dtype, f64, tol in ((_lib.F32, False, 4e-6), (_lib.F64, True, 1e-14)):
        ref = O.philox_normal(seed, idx, d, 3, 3 + M, f64=f64)
        for m in range(M):
            bits = (C.c_uint32 * d)()
            lib.mivi_eps_bits_host(seed, idx, d, 3 + m, 0, d, bits)
            assert np.array_equal(np.array(bits, dtype=np.uint32), ref_bits[:, m])
            out = (C.c_double * d)()
            lib.mivi_eps_host(seed, idx, d, 3 + m, 0, d, dtype, out)
            assert np.max(np.abs(np.array(out) - ref[:, m])) < tol


def test_family_constructors_and_destructure():
    """test/families/location_scale.jl:146-155 on the host mirror."""
    d = 5
    for dt in (np.float32, np.float64):
        q = avi.MeanFieldGaussian(np.zeros(d, dt), np.ones(d, dt))
        p, re_ = avi.destructure(q)
        assert p.shape == (2 * d,) and p.dtype == dt and q.eltype == dt and len(q) == d
        q2 = re_(p)
        assert np.array_equal(q2.location, q.location) and np.array_equal(q2.scale, q.scale)
        L = np.tril(np.arange(1, d * d + 1, dtype=dt).reshape(d, d))
        qf = avi.FullRankGaussian(np.arange(d, dtype=dt), L + np.triu(np.ones((d, d), dt), 1))
        assert np.array_equal(qf.scale, L)   # LowerTriangular projection
        pf, ref_ = avi.destructure(qf)
        assert pf.shape == (d + d * d,) and np.array_equal(pf, O.destructure(O.MvLocationScale(qf.location, L)))
        assert np.array_equal(ref_(pf).scale, L)
    with pytest.raises(TypeError):
        avi.MeanFieldGaussian(np.zeros(3), np.eye(3))
    with pytest.raises(TypeError):
        avi.MvLocationScale(np.zeros(3, dtype=np.int32), np.ones(3))
    with pytest.raises(ValueError):
        avi.MvLocationScale(np.zeros(3), np.ones(4))


def test_objective_and_algorithm_constructors():
    obj = avi.RepGradELBO(10)
    assert isinstance(obj.entropy, avi.ClosedFormEntropy) and obj.n_samples == 10        # repgradelbo.jl:72-74
    assert repr(avi.RepGradELBO(3, entropy=avi.StickingTheLandingEntropy())) == \
        "RepGradELBO(entropy=StickingTheLandingEntropy(), n_samples=3)"
    with pytest.raises(ValueError):
        avi.RepGradELBO(0)
    with pytest.raises(TypeError):
        avi.RepGradELBO(3, entropy="closed")
    alg = avi.KLMinRepGradDescent(avi.AutoMIVI())                                       # constructors.jl:58-66 defaults
    assert alg.objective.n_samples == 1 and isinstance(alg.optimizer, avi.DoWG)
    assert isinstance(alg.averager, avi.PolynomialAveraging) and isinstance(alg.operator, avi.IdentityOperator)
    assert avi.ADVI is avi.KLMinRepGradDescent
    with pytest.raises(TypeError):   # ZeroGradient estimators belong to KLMinRepGradProxDescent (constructors.jl:60)
        avi.KLMinRepGradDescent(avi.AutoMIVI(), entropy=avi.ClosedFormEntropyZeroGradient())
    codes = [e.code for e in (avi.ClosedFormEntropy(), avi.ClosedFormEntropyZeroGradient(), avi.MonteCarloEntropy(),
                              avi.StickingTheLandingEntropy(), avi.StickingTheLandingEntropyZeroGradient())]
    assert codes == [O.ENT_CLOSED_FORM, O.ENT_CLOSED_FORM_ZERO_GRAD, O.ENT_MONTE_CARLO, O.ENT_STL, O.ENT_STL_ZERO_GRAD]


def test_rng_counter_semantics():
    r = avi.PhiloxRNG(5)
    assert [r.next_index() for _ in range(3)] == [0, 1, 2]
    c = r.copy()
    assert c.next_index() == 3 and r.next_index() == 3


def test_order0_plugin_is_rejected_only_without_a_target_ad():
    """AutoMIVI(target_ad=None): strict mode, the TypeError comes before any native resource exists (with the default
    target_ad="forwarddiff" the problem is wrapped instead: tests/test_forwarddiff_host.py, test_gpu_baseline_configs.py)."""
    class Order0:
        def dimension(self):
            return 2

        def logdensity(self, z):
            return 0.0

    q = avi.MeanFieldGaussian(np.zeros(2), np.ones(2))
    p, re_ = avi.destructure(q)
    with pytest.raises(TypeError, match="LogDensityOrder"):
        avi.init(avi.PhiloxRNG(1), avi.RepGradELBO(2), avi.AutoMIVI(target_ad=None), q, Order0(), p, re_)


def test_shard_plan():
    from advancedvi_jl_amd.distributed import ShardPlan, partials_len
    for n, w in ((1024, 8), (10, 3), (7, 7), (512, 1)):
        plan = ShardPlan(n, w)
        ranges = [plan.range(r) for r in range(w)]
        assert ranges[0][0] == 0 and ranges[-1][1] == n
        assert all(ranges[i][1] == ranges[i + 1][0] for i in range(w - 1))
        assert max(plan.count(r) for r in range(w)) - min(plan.count(r) for r in range(w)) <= 1
    with pytest.raises(ValueError):
        ShardPlan(3, 4)
    assert partials_len(4, 0) == 10 and partials_len(4, 1) == 16


def test_p2p_geometry_invariants_and_host_restatement():
    """The peer-to-peer exchange's geometry (mivi_p2p_geometry, host-only): every rank must derive the same slices / chunks, the two
    scalars must lie in one slice, 16-byte vectors must never straddle a slice or chunk boundary; the oracle restates it."""
    from advancedvi_jl_amd.distributed import p2p_geometry
    from oracle import oracle as O
    for L in list(range(4, 80)) + [2050, 4098, 131330, 525826, 2098178, 525826 + 1, 525826 + 3]:
        for R in range(1, 9):
            n, cn, G, vs = p2p_geometry(L, R)
            assert (n, cn, G, vs) == O.p2p_geometry(L, R)
            assert n % 4 == 0 and cn % 4 == 0 and n * R >= L and G * cn >= n and 1 <= G <= 255
            assert (L - 2) // n == (L - 1) // n == vs and 0 <= vs < R


@pytest.mark.parametrize("family,d", [(0, 5), (0, 700), (1, 3), (1, 40)])
@pytest.mark.parametrize("R", [1, 2, 3, 8])
def test_p2p_exchange_restatement_equals_allreduce_then_finalize(family, d, R):
    """oracle.p2p_exchange (the chunked push / reduce / unpack protocol of csrc/kernels_p2p.hip restated on the host, double-buffered
    over three epochs) == finalize(sum of the rank partials) on every rank, bit-identical across ranks."""
    from oracle import oracle as O
    rng = np.random.default_rng(100 * d + R)
    L = (2 * d if family == 0 else d + d * (d + 1) // 2) + 2
    if family == 0:
        params = np.concatenate([rng.normal(size=d), rng.uniform(0.5, 2.0, size=d)])
    else:
        Cm = np.tril(rng.normal(size=(d, d)) * 0.1)
        Cm[np.diag_indices(d)] = rng.uniform(0.5, 2.0, size=d)
        params = np.concatenate([rng.normal(size=d), Cm.reshape(-1, order="F")])
    M_total = 16 * R
    epochs = [[rng.normal(size=L) for _ in range(R)] for _ in range(3)]
    for ent in (0, 3, 4):
        res = O.p2p_exchange(epochs, params, d, family, ent, M_total)
        for parts, per_rank in zip(epochs, res):
            v_ref, g_ref = O.finalize_partials(np.sum(parts, axis=0), params, d, family, ent, M_total)
            for v, g in per_rank:
                assert np.isfinite(v) and np.all(np.isfinite(g))
                assert abs(v - v_ref) <= 1e-12 * max(1.0, abs(v_ref)) and np.max(np.abs(g - g_ref)) <= 1e-12 * max(1.0, np.max(np.abs(g_ref)))
                assert v == per_rank[0][0] and np.array_equal(g, per_rank[0][1])
