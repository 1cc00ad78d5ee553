"""Thin object wrapper over the libmivi C ABI (include/mivi.h).  Device memory and the HIP stream
come from torch (plumbing only); every computation is a libmivi kernel."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .families import FULLRANK, LOWRANK, MEANFIELD, NSF, REALNVP
from . import problems as P

NATGRAD_SMALL_D = 44   # MIVI_NATGRAD_SMALL_D (include/mivi.h): up to this d mivi_natgrad_update is the one-workgroup kernel, above it the tile path
BAM_MAX_SAMPLES = 64   # MIVI_BAM_MAX_SAMPLES (include/mivi.h): the most samples mivi_bam_update / mivi_bam_steps take

_NP2MIVI = {np.dtype(np.float32): _lib.F32, np.dtype(np.float64): _lib.F64}


def _torch():
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("libmivi needs a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")
    return torch


def torch_dtype(np_dtype):
    torch = _torch()
    return torch.float32 if np.dtype(np_dtype) == np.float32 else torch.float64


class MiviContext:
    """One RepGradELBO estimator instance on one GPU (mivi_create ... mivi_destroy)."""

    def __init__(self, dtype, family, d, n_mc, entropy, seed, device=0, m_offset=0, m_total=0, stream=None, rank=0, flow=None):
        """flow: (hidden_dims, n_layers) of a REALNVP context (mivi_create_flow), (hidden_dims, n_layers, n_bins, bound) of an NSF
        context (mivi_create_spline_flow); not read for the other families."""
        torch = _torch()
        self.lib = _lib.load()
        self.np_dtype = np.dtype(dtype)
        self.family, self.d, self.n_mc, self.entropy = int(family), int(d), int(n_mc), int(entropy)
        self.device = int(device)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF   # the Philox seed of every draw of this context
        self.rank = int(rank)  # columns of scale_factors (the low-rank family; not read for the others)
        self.tdtype = torch_dtype(self.np_dtype)
        self.tdevice = torch.device("cuda", self.device)
        if stream is None:
            stream = torch.cuda.current_stream(self.tdevice).cuda_stream
        cfg = _lib.MiviConfig(_NP2MIVI[self.np_dtype], self.family, self.d, self.n_mc, self.entropy, self.device,
                              C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), int(m_offset), int(m_total), C.c_void_p(stream), 0, self.rank)
        h = C.c_void_p()
        if self.family == REALNVP:
            if flow is None:
                raise ValueError("a REALNVP context needs flow = (hidden_dims, n_layers)")
            hidden = [int(w) for w in flow[0]]
            if not 1 <= len(hidden) <= 3:
                raise ValueError("RealNVP: one to three hidden layers")
            self.flow = (tuple(hidden), int(flow[1]))
            arch = _lib.MiviFlow(int(flow[1]), len(hidden), (C.c_int32 * 3)(*(hidden + [0] * (3 - len(hidden)))))
            st = self.lib.mivi_create_flow(C.byref(cfg), C.byref(arch), C.byref(h))
            if st == 6:   # MIVI_ERR_UNSUPPORTED before a context exists to carry the message
                sharded = int(m_offset) != 0 or int(m_total) not in (0, self.n_mc)
                raise _lib.MiviError(st, "mivi_create_flow: the RealNVP family has no sharded form (m_offset / m_total)" if sharded else
                                         "mivi_create_flow: a flow has no entropy(q) -- the estimators that work on it are MonteCarloEntropy "
                                         "and StickingTheLandingEntropy")
        elif self.family == NSF:
            if flow is None or len(flow) != 4:
                raise ValueError("an NSF context needs flow = (hidden_dims, n_layers, n_bins, bound)")
            hidden = [int(w) for w in flow[0]]
            if not 1 <= len(hidden) <= 3:
                raise ValueError("NeuralSplineFlow: one to three hidden layers")
            self.flow = (tuple(hidden), int(flow[1]), int(flow[2]), float(flow[3]))
            arch = _lib.MiviSplineFlow(int(flow[1]), len(hidden), (C.c_int32 * 3)(*(hidden + [0] * (3 - len(hidden)))), int(flow[2]), float(flow[3]))
            st = self.lib.mivi_create_spline_flow(C.byref(cfg), C.byref(arch), C.byref(h))
            if st == 6:   # MIVI_ERR_UNSUPPORTED before a context exists to carry the message
                sharded = int(m_offset) != 0 or int(m_total) not in (0, self.n_mc)
                raise _lib.MiviError(st, "mivi_create_spline_flow: the neural spline flow family has no sharded form (m_offset / m_total)" if sharded else
                                         "mivi_create_spline_flow: a flow has no entropy(q) -- the estimators that work on it are MonteCarloEntropy "
                                         "and StickingTheLandingEntropy")
        else:
            st = self.lib.mivi_create(C.byref(cfg), C.byref(h))
        _lib.check(self.lib, None, st)
        self.h = h
        self.m_total = int(m_total) if m_total else self.n_mc
        self._keep = []      # keep-alive for callbacks / borrowed device arrays
        self.problem = None

    # -- lifetime ---------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.mivi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, st):
        _lib.check(self.lib, self.h, st)

    @property
    def params_len(self):
        return int(self.lib.mivi_params_len(self.h))

    @property
    def partials_len(self):
        return int(self.lib.mivi_partials_len(self.h))

    def synchronize(self):
        self._chk(self.lib.mivi_synchronize(self.h))

    # -- tensors ----------------------------------------------------------------------------------
    def to_device(self, x):
        torch = _torch()
        if isinstance(x, torch.Tensor):
            if x.device != self.tdevice or x.dtype != self.tdtype or not x.is_contiguous():
                x = x.to(device=self.tdevice, dtype=self.tdtype).contiguous()
            return x
        return torch.as_tensor(np.ascontiguousarray(x, dtype=self.np_dtype)).to(self.tdevice)

    def empty(self, n):
        return _torch().empty(int(n), dtype=self.tdtype, device=self.tdevice)

    @staticmethod
    def _p(t):
        return C.c_void_p(t.data_ptr())

    # -- targets ----------------------------------------------------------------------------------
    def set_problem(self, prob, values_only=False):
        """values_only: the caller evaluates nothing but `logdensity` (ScoreGradELBO) -- a generic problem without a gradient is then
        registered through mivi_set_target_value_callback instead of a gradient callback that raises."""
        if P.dimension(prob) != self.d:
            raise ValueError("dimension(prob) does not match the variational family")
        dt = self.np_dtype
        if isinstance(prob, P.TransformedProblem):   # inner target first, then the Stacked bijector around it
            self.set_problem(prob.prob, values_only=values_only)
            self.set_bijector(prob.bijector)
            self.problem = prob
            return
        self.set_bijector(None)
        if not isinstance(prob, (P.LogRegProblem, P.LogRegSubset)):
            self._lr_full = None   # another target kind replaces the resident data set
        if isinstance(prob, P.DiagNormalProblem):
            m = np.ascontiguousarray(prob.mean, dtype=dt)
            s = np.ascontiguousarray(np.broadcast_to(prob.std, m.shape), dtype=dt)
            self._chk(self.lib.mivi_set_target_diag_gauss(self.h, m.ctypes.data, s.ctypes.data))
        elif isinstance(prob, P.DenseNormalProblem):
            m = np.ascontiguousarray(prob.mean, dtype=dt)
            L = np.asfortranarray(prob.L, dtype=dt)
            self._chk(self.lib.mivi_set_target_dense_gauss(self.h, m.ctypes.data, L.ctypes.data))
        elif isinstance(prob, P.LogRegProblem) and getattr(self, "_lr_full", None) is prob:
            self._chk(self.lib.mivi_logreg_select_rows(self.h, None, 0, 1.0))   # already resident: back to all rows
        elif isinstance(prob, P.LogRegProblem):
            self._lr_full = prob
            torch = _torch()
            X = prob.X
            if isinstance(X, torch.Tensor):   # device-resident, column-major n x p expected
                Xd, yd = X, prob.y
                n = X.shape[1] if getattr(prob, "x_is_colmajor_tensor", False) else X.shape[0]
                self._keep += [Xd, yd]
                self._chk(self.lib.mivi_set_target_logreg(self.h, self._p(Xd), self._p(yd), n,
                                                          P.LogRegProblem.VARIANTS[prob.variant], prob.likeadj, 1))
            else:
                Xf = np.asfortranarray(X, dtype=dt)
                y = np.ascontiguousarray(prob.y, dtype=np.uint8)
                self._chk(self.lib.mivi_set_target_logreg(self.h, Xf.ctypes.data, y.ctypes.data, Xf.shape[0],
                                                          P.LogRegProblem.VARIANTS[prob.variant], prob.likeadj, 0))
        elif isinstance(prob, P.LogRegSubset):
            if getattr(self, "_lr_full", None) is not prob.parent:   # upload the full data set once, then only select rows
                self.set_problem(prob.parent)
            self._chk(self.lib.mivi_logreg_select_rows(self.h, prob.batch.ctypes.data, prob.batch.size, prob.likeadj))
        elif isinstance(prob, P.FunnelProblem):
            self._chk(self.lib.mivi_set_target_funnel(self.h, prob.sigma_v))
        elif isinstance(prob, P.FunnelConstrainedProblem):
            self._chk(self.lib.mivi_set_target_funnel_constrained(self.h, prob.sigma_v))
        else:
            self._set_callback(prob, values_only=values_only)
        self.problem = prob

    def set_base_dist(self, dist):
        """mivi_set_base_dist: the base distribution of the location-scale family -- families.Normal() (None: the same), Laplace() or
        TDist(nu).  Normal() on a context that never left it changes nothing."""
        code, nu = (0, 0.0) if dist is None else (int(dist.code), float(dist.nu))
        self._chk(self.lib.mivi_set_base_dist(self.h, code, nu))

    def set_bijector(self, bij):
        """mivi_set_bijector_stacked: a P.StackedBijector around whatever target is set (None removes it); one with a truncated or an
        ordered block goes through mivi_set_bijector_stacked_ex."""
        if bij is None:
            self._chk(self.lib.mivi_set_bijector_stacked(self.h, 0, None, None))
            return
        rng = np.ascontiguousarray([[lo, hi] for lo, hi, _ in bij.blocks], dtype=np.int32)
        kinds = np.ascontiguousarray([P.StackedBijector.KINDS[k] for _, _, k in bij.blocks], dtype=np.int32)
        if bij.is_legacy:
            self._chk(self.lib.mivi_set_bijector_stacked(self.h, len(bij.blocks), rng.ctypes.data, kinds.ctypes.data))
            return
        bounds = np.ascontiguousarray(bij.bounds, dtype=np.float64).reshape(-1)   # truncated / ordered blocks: the _ex entry
        self._chk(self.lib.mivi_set_bijector_stacked_ex(self.h, len(bij.blocks), rng.ctypes.data, kinds.ctypes.data, bounds.ctypes.data))

    def _set_callback(self, prob, values_only=False):
        has_grad = hasattr(prob, "logdensity_and_gradient") or hasattr(prob, "logdensity_and_gradient_batch")
        if not has_grad and not hasattr(prob, "logdensity"):
            raise TypeError("generic targets must implement logdensity (LogDensityOrder 0: values only -- estimate_objective) or "
                            "logdensity_and_gradient (LogDensityOrder >= 1); see INTEGRATION.md")
        dt = self.np_dtype

        def as_mat(ptr, d, M):
            buf = (C.c_char * (d * M * dt.itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dt).reshape((d, M), order="F")

        def fg(user, Zp, d, M, ellp, Gp):
            try:
                if not has_grad:   # an order-0 problem set directly on a context: values only (objectives.init wraps it in ADgradient)
                    raise TypeError("the target only implements logdensity (LogDensityOrder{0}()): a gradient estimate needs "
                                    "logdensity_and_gradient -- wrap it in ADgradient(\"forwarddiff\", prob), as init(..., AutoMIVI(), ...) does")
                Z = as_mat(Zp, d, M)
                ell = as_mat(ellp, 1, M)
                G = as_mat(Gp, d, M)
                if hasattr(prob, "logdensity_and_gradient_batch"):
                    l, g = prob.logdensity_and_gradient_batch(Z)
                    ell[0, :] = l
                    G[:, :] = g
                else:
                    for m in range(M):
                        l, g = prob.logdensity_and_gradient(Z[:, m])   # column view, like eachcol(samples)
                        ell[0, m] = l
                        G[:, m] = g
                return 0
            except Exception as e:  # no exceptions across the ABI
                self._cb_error = e
                return 1

        def fv(user, Zp, d, M, ellp):
            try:
                Z = as_mat(Zp, d, M)
                ell = as_mat(ellp, 1, M)
                for m in range(M):
                    ell[0, m] = prob.logdensity(Z[:, m])
                return 0
            except Exception as e:
                self._cb_error = e
                return 1

        def fh(user, Zp, d, M, ellp, Gp, Hp):   # second-order plugin: ell, G and the SUM of the Hessians over the M columns
            try:
                Z = as_mat(Zp, d, M)
                ell = as_mat(ellp, 1, M)
                G = as_mat(Gp, d, M)
                H = as_mat(Hp, d, d)
                Hacc = np.zeros((d, d), dtype=np.float64)   # (the chunk's sum in f64, rounded once to the context's dtype)
                for m in range(M):
                    l, g, h = prob.logdensity_gradient_and_hessian(Z[:, m])
                    ell[0, m] = l
                    G[:, m] = g
                    Hacc += np.asarray(h, dtype=np.float64)
                H[:, :] = Hacc
                return 0
            except Exception as e:
                self._cb_error = e
                return 1

        cfg = _lib.LOGDENSITY_AND_GRADIENT_FN(fg)
        cfv = _lib.LOGDENSITY_FN(fv) if hasattr(prob, "logdensity") else C.cast(None, _lib.LOGDENSITY_FN)
        cfh = (_lib.LOGDENSITY_GRADIENT_AND_HESSIAN_FN(fh) if hasattr(prob, "logdensity_gradient_and_hessian")
               else C.cast(None, _lib.LOGDENSITY_GRADIENT_AND_HESSIAN_FN))
        self._keep += [cfg, cfv, cfh]
        self._cb_error = None
        if values_only and hasattr(prob, "logdensity") and (not has_grad or P.capabilities(prob) < P.LogDensityOrder(1)):
            self._chk(self.lib.mivi_set_target_value_callback(self.h, cfv, None))   # order 0: no gradient function behind the ABI at all
            return
        self._chk(self.lib.mivi_set_target_callback(self.h, cfg, cfv, None))
        self._chk(self.lib.mivi_set_target_hess_callback(self.h, cfh, None))

    def _raise_cb(self, st):
        err = getattr(self, "_cb_error", None)
        if st != 0 and err is not None:
            self._cb_error = None
            raise err
        self._chk(st)

    # -- hot path ---------------------------------------------------------------------------------
    def sample(self, params, idx, want_eps=True):
        p = self.to_device(params)
        Z = self.empty(self.d * self.n_mc)
        de = self.d + (self.rank if self.family == LOWRANK else 0)   # low-rank: the draws are (u1 (d); u2 (rank)) per column
        eps = self.empty(de * self.n_mc) if want_eps else None
        self._chk(self.lib.mivi_sample(self.h, self._p(p), idx, self._p(Z), self._p(eps) if want_eps else None))
        # d x M column-major -> torch (M, d) row-major view transposed
        Zv = Z.view(self.n_mc, self.d).t()
        return (Zv, eps.view(self.n_mc, de).t()) if want_eps else Zv

    def _points(self, Z):
        """the d x n points of logpdf as column-major device storage: (flat tensor of d * n elements, n).  A (d, n) matrix (numpy or
        tensor; the transposed view `sample` returns is taken as it is), a vector of d (n = 1), or the flat column-major storage."""
        torch = _torch()
        if not isinstance(Z, torch.Tensor):
            Z = np.asarray(Z)
        if Z.ndim == 2:
            if Z.shape[0] != self.d:
                raise ValueError(f"logpdf: points must be (d, n) with d = {self.d}, got {tuple(Z.shape)}")
            Z = Z.t() if isinstance(Z, torch.Tensor) else Z.T   # (n, d): row-major storage of this IS the column-major d x n
        elif Z.ndim != 1 or Z.shape[0] % self.d:
            raise ValueError(f"logpdf: points must be (d, n), (d,) or flat d * n with d = {self.d}, got {tuple(Z.shape)}")
        Zd = self.to_device(Z).reshape(-1)
        return Zd, Zd.numel() // self.d

    def logpdf(self, params, Z, out=None, std=None):
        """mivi_logpdf: log q(z_k) for the n columns of Z (see _points) as a device tensor of n values; needs no target and ignores a
        bijector (q lives on the unconstrained scale).  std: None -- not wanted; True or a flat device tensor of d * n elements -- the
        standardised points u = C^-1 (z - mu) are written too and (logq, u as a (d, n) view) is returned (not on the low-rank family)."""
        p = self.to_device(params)
        Zd, n = self._points(Z)
        out = self.empty(n) if out is None else out
        if std is True:
            std = self.empty(self.d * n)
        self._chk(self.lib.mivi_logpdf(self.h, self._p(p), self._p(Zd), n, self._p(out), self._p(std) if std is not None else None))
        return out if std is None else (out, std.view(n, self.d).t())

    def logpdf_host(self, params, Z, want_std=False):
        """mivi_logpdf_host: numpy in, numpy out, synchronous; Z (d, n).  Returns logq (n) or (logq, u (d, n))."""
        p = np.ascontiguousarray(params, dtype=self.np_dtype)
        Zh = np.asfortranarray(np.asarray(Z, dtype=self.np_dtype).reshape(self.d, -1))
        n = Zh.shape[1]
        out = np.zeros(n, dtype=self.np_dtype)
        stdh = np.zeros((self.d, n), dtype=self.np_dtype, order="F") if want_std else None
        self._chk(self.lib.mivi_logpdf_host(self.h, p.ctypes.data, Zh.ctypes.data, n, out.ctypes.data, stdh.ctypes.data if want_std else None))
        return (out, stdh) if want_std else out

    def sample_constrained(self, params, idx, want_eta=False):
        """mivi_sample_constrained: X = binv(z) for the draws z `sample` returns at `idx`, pushed through the bijector that is set, as a
        (d, n_mc) view; want_eta: (X, z)."""
        p = self.to_device(params)
        X = self.empty(self.d * self.n_mc)
        eta = self.empty(self.d * self.n_mc) if want_eta else None
        self._chk(self.lib.mivi_sample_constrained(self.h, self._p(p), idx, self._p(X), self._p(eta) if want_eta else None))
        Xv = X.view(self.n_mc, self.d).t()
        return (Xv, eta.view(self.n_mc, self.d).t()) if want_eta else Xv

    def logpdf_constrained(self, params, X, out=None):
        """mivi_logpdf_constrained: logpdf of the transformed distribution at the n constrained points X (see _points): log q(b(x)) -
        logabsdetjac(binv, b(x)) as a device tensor of n values; -inf outside the support, NaN for a NaN point."""
        p = self.to_device(params)
        Xd, n = self._points(X)
        out = self.empty(n) if out is None else out
        self._chk(self.lib.mivi_logpdf_constrained(self.h, self._p(p), self._p(Xd), n, self._p(out)))
        return out

    def logpdf_constrained_host(self, params, X):
        """mivi_logpdf_constrained_host: numpy in, numpy out, synchronous; X (d, n)."""
        p = np.ascontiguousarray(params, dtype=self.np_dtype)
        Xh = np.asfortranarray(np.asarray(X, dtype=self.np_dtype).reshape(self.d, -1))
        n = Xh.shape[1]
        out = np.zeros(n, dtype=self.np_dtype)
        self._chk(self.lib.mivi_logpdf_constrained_host(self.h, p.ctypes.data, Xh.ctypes.data, n, out.ctypes.data))
        return out

    def estimate_gradient(self, params, idx, value=None, grad=None):
        p = self.to_device(params)
        value = self.empty(1) if value is None else value
        grad = self.empty(self.params_len) if grad is None else grad
        self._raise_cb(self.lib.mivi_estimate_gradient(self.h, self._p(p), idx, self._p(value), self._p(grad)))
        return value, grad

    def estimate_score_gradient(self, params, idx, value=None, elbo=None, grad=None):
        """mivi_estimate_score_gradient: (value = the VarGrad objective, elbo = mean(log pi - log q), gradient) of estimate `idx`."""
        p = self.to_device(params)
        value = self.empty(1) if value is None else value
        elbo = self.empty(1) if elbo is None else elbo
        grad = self.empty(self.params_len) if grad is None else grad
        self._raise_cb(self.lib.mivi_estimate_score_gradient(self.h, self._p(p), idx, self._p(value), self._p(elbo), self._p(grad)))
        return value, elbo, grad

    def estimate_gradient_n(self, params, idx0, count, value, grad):
        self._chk(self.lib.mivi_estimate_gradient_n(self.h, self._p(params), idx0, int(count), self._p(value), self._p(grad)))

    def estimate_gradient_each(self, params, idx0, count, values=None, grads=None, want_grads=True):
        """Every estimate of the batch idx0 .. idx0 + count - 1 at the same parameters (mivi_estimate_gradient_each):
        values T[count], grads (count, params_len) -- row i equals mivi_estimate_gradient(idx0 + i): bitwise on the generic route, to rounding (1e-6 / 2e-6) on the batch engine."""
        p = self.to_device(params)
        values = self.empty(int(count)) if values is None else values
        if grads is None and want_grads:
            grads = self.empty(int(count) * self.params_len)
        self._chk(self.lib.mivi_estimate_gradient_each(self.h, self._p(p), idx0, int(count), self._p(values), self._p(grads) if grads is not None else None))
        return values, (grads.view(int(count), self.params_len) if grads is not None else None)

    def estimate_objective(self, params, idx, n_samples=0, entropy=-1, value=None):
        p = self.to_device(params)
        value = self.empty(1) if value is None else value
        self._raise_cb(self.lib.mivi_estimate_objective(self.h, self._p(p), idx, int(n_samples), int(entropy), self._p(value)))
        return value

    def gauss_expected_grad_hess(self, params, idx, n_samples=0, grad=None, hess=None, second_order=False):
        """(logpi_avg T[1], grad T[d], hess (d, d)) of mivi_gauss_expected_grad_hess (Stein / Price branch) or, with
        `second_order`, of mivi_gauss_expected_grad_hess2 (sample average of the Hessians); `hess[i, j]` is the matrix entry."""
        p = self.to_device(params)
        logpi = self.empty(1)
        grad = self.empty(self.d) if grad is None else grad
        hess = self.empty(self.d * self.d) if hess is None else hess
        fn = self.lib.mivi_gauss_expected_grad_hess2 if second_order else self.lib.mivi_gauss_expected_grad_hess
        self._raise_cb(fn(self.h, self._p(p), idx, int(n_samples), self._p(logpi), self._p(grad), self._p(hess)))
        return logpi, grad, hess.view(self.d, self.d).t()   # column-major d x d

    def sqrt_ngd_update(self, params, grad, hess, stepsize, entropy=None):
        """mivi_sqrt_ngd_update: the square-root natural-gradient update of the device tensor `params` ([m; vec C]) in place from
        grad (d) and hess (d*d column-major, as gauss_expected_grad_hess fills it); returns entropy(q') as a 1-element device tensor."""
        entropy = self.empty(1) if entropy is None else entropy
        hess = hess.t() if hess.dim() == 2 else hess   # the (d, d) matrix view gauss_expected_grad_hess returns -> its column-major storage
        if not hess.is_contiguous():
            hess = hess.contiguous()
        self._chk(self.lib.mivi_sqrt_ngd_update(self.h, self._p(params), self._p(grad), self._p(hess), float(stepsize), self._p(entropy)))
        return entropy

    def sqrt_ngd_update_host(self, params, grad, hess, stepsize):
        """mivi_sqrt_ngd_update_host on numpy arrays: params ([m; vec C]), grad (d), hess ((d, d) matrix); returns (params', entropy(q'))."""
        p = np.array(params, dtype=self.np_dtype, copy=True)
        g = np.ascontiguousarray(grad, dtype=self.np_dtype)
        H = np.asfortranarray(hess, dtype=self.np_dtype)
        ent = np.zeros(1, dtype=self.np_dtype)
        self._chk(self.lib.mivi_sqrt_ngd_update_host(self.h, p.ctypes.data, g.ctypes.data, H.ctypes.data, float(stepsize), ent.ctypes.data))
        return p, ent[0]

    # the _host entries (what julia/MIVI.jl calls on every step): numpy arrays in, numpy arrays out, synchronous
    def estimate_gradient_host(self, params, idx):
        """mivi_estimate_gradient_host: (value, grad (params_len)) of estimate `idx` at the host vector `params`."""
        p = np.ascontiguousarray(params, dtype=self.np_dtype)
        value = np.zeros(1, dtype=self.np_dtype)
        grad = np.zeros(self.params_len, dtype=self.np_dtype)
        self._raise_cb(self.lib.mivi_estimate_gradient_host(self.h, p.ctypes.data, idx, value.ctypes.data, grad.ctypes.data))
        return value[0], grad

    def estimate_objective_host(self, params, idx, n_samples=0, entropy=-1):
        """mivi_estimate_objective_host: the objective value; a non-finite one is returned as it is (only a non-positive scale raises)."""
        p = np.ascontiguousarray(params, dtype=self.np_dtype)
        value = np.zeros(1, dtype=self.np_dtype)
        self._raise_cb(self.lib.mivi_estimate_objective_host(self.h, p.ctypes.data, idx, int(n_samples), int(entropy), value.ctypes.data))
        return value[0]

    def gauss_expected_grad_hess_host(self, params, idx, n_samples=0, second_order=False):
        """mivi_gauss_expected_grad_hess_host / _hess2_host: (logpi_avg, grad (d), hess (d, d)); `hess[i, j]` is the matrix entry."""
        p = np.ascontiguousarray(params, dtype=self.np_dtype)
        logpi = np.zeros(1, dtype=self.np_dtype)
        grad = np.zeros(self.d, dtype=self.np_dtype)
        hess = np.zeros((self.d, self.d), dtype=self.np_dtype, order="F")   # column-major d x d
        fn = self.lib.mivi_gauss_expected_grad_hess2_host if second_order else self.lib.mivi_gauss_expected_grad_hess_host
        self._raise_cb(fn(self.h, p.ctypes.data, idx, int(n_samples), logpi.ctypes.data, grad.ctypes.data, hess.ctypes.data))
        return logpi[0], grad, hess

    def estimate_score_gradient_host(self, params, idx, want_elbo=True):
        """mivi_estimate_score_gradient_host: (value, elbo, grad (params_len)); want_elbo False passes NULL for elbo_h and returns None there."""
        p = np.ascontiguousarray(params, dtype=self.np_dtype)
        value = np.zeros(1, dtype=self.np_dtype)
        elbo = np.zeros(1, dtype=self.np_dtype) if want_elbo else None
        grad = np.zeros(self.params_len, dtype=self.np_dtype)
        self._raise_cb(self.lib.mivi_estimate_score_gradient_host(self.h, p.ctypes.data, idx, value.ctypes.data,
                                                                  elbo.ctypes.data if want_elbo else None, grad.ctypes.data))
        return value[0], (elbo[0] if want_elbo else None), grad

    def sqrt_ngd_steps(self, params, idx0, count, stepsize, n_samples=0, second_order=False, elbo=None):
        """mivi_sqrt_ngd_steps: `count` iterations {estimator (index idx0 + t), update} on the device tensor `params`; returns elbo (count)."""
        elbo = self.empty(int(count)) if elbo is None else elbo
        self._raise_cb(self.lib.mivi_sqrt_ngd_steps(self.h, self._p(params), idx0, int(count), int(n_samples), 1 if second_order else 0,
                                                    float(stepsize), self._p(elbo)))
        return elbo

    def natgrad_init(self, params, state=None):
        """mivi_natgrad_init: the device tensor [S; Sigma] (2 d^2: precision C^-T C^-1 and covariance C C', column-major) of the device
        parameters `params` ([m; vec C])."""
        state = self.empty(2 * self.d * self.d) if state is None else state
        self._chk(self.lib.mivi_natgrad_init(self.h, self._p(params), self._p(state)))
        return state

    def natgrad_update(self, params, state, grad, hess, stepsize, ensure_posdef=True, entropy=None):
        """mivi_natgrad_update: the natural-gradient update of the device tensors `params` ([m; vec C]) and `state` ([S; Sigma]) in place
        from grad (d) and hess (d*d column-major, as gauss_expected_grad_hess fills it); returns entropy(q') as a 1-element device tensor.
        The new scale C' is the LOWER Cholesky factor of Sigma' (the reference's is an upper-triangular factor of the same Sigma')."""
        entropy = self.empty(1) if entropy is None else entropy
        hess = hess.t() if hess.dim() == 2 else hess   # the (d, d) matrix view gauss_expected_grad_hess returns -> its column-major storage
        if not hess.is_contiguous():
            hess = hess.contiguous()
        self._chk(self.lib.mivi_natgrad_update(self.h, self._p(params), self._p(state), self._p(grad), self._p(hess), float(stepsize),
                                               1 if ensure_posdef else 0, self._p(entropy)))
        return entropy

    def natgrad_update_host(self, params, state, grad, hess, stepsize, ensure_posdef=True):
        """mivi_natgrad_update_host on numpy arrays: params ([m; vec C]), state ([S; Sigma], 2 d^2), grad (d), hess ((d, d) matrix); returns
        (params', state', entropy(q'))."""
        p = np.array(params, dtype=self.np_dtype, copy=True)
        st = np.array(state, dtype=self.np_dtype, copy=True)
        g = np.ascontiguousarray(grad, dtype=self.np_dtype)
        H = np.asfortranarray(hess, dtype=self.np_dtype)
        ent = np.zeros(1, dtype=self.np_dtype)
        self._chk(self.lib.mivi_natgrad_update_host(self.h, p.ctypes.data, st.ctypes.data, g.ctypes.data, H.ctypes.data, float(stepsize),
                                                    1 if ensure_posdef else 0, ent.ctypes.data))
        return p, st, ent[0]

    def natgrad_steps(self, params, state, idx0, count, stepsize, ensure_posdef=True, n_samples=0, second_order=False, elbo=None):
        """mivi_natgrad_steps: `count` iterations {estimator (index idx0 + t), update} on the device tensors `params` and `state`; returns
        elbo (count)."""
        elbo = self.empty(int(count)) if elbo is None else elbo
        self._raise_cb(self.lib.mivi_natgrad_steps(self.h, self._p(params), self._p(state), idx0, int(count), int(n_samples),
                                                   1 if second_order else 0, float(stepsize), 1 if ensure_posdef else 0, self._p(elbo)))
        return elbo

    # -- FisherMinBatchMatch (mivi_bam_*: fisherminbatchmatch.jl) -----------------------------------------------------------------
    def bam_init(self, params, state=None):
        """mivi_bam_init: the device tensor Sigma = C C' (d^2, column-major, triangles bitwise mirrored) of the device parameters `params`."""
        state = self.empty(self.d * self.d) if state is None else state
        self._chk(self.lib.mivi_bam_init(self.h, self._p(params), self._p(state)))
        return state

    def bam_moments(self, params, idx, n_samples, u=None, G=None):
        """mivi_bam_moments: (u, G, fisher, logpi_avg, elbo) of estimate `idx` at the device tensor `params`; u and G are flat device
        tensors (d * n_samples, column-major: `.view(n_samples, d).t()` is the d x n matrix), the three values 1-element device tensors."""
        n = int(n_samples)
        u = self.empty(self.d * max(n, 0)) if u is None else u
        G = self.empty(self.d * max(n, 0)) if G is None else G
        vals = self.empty(3)
        self._raise_cb(self.lib.mivi_bam_moments(self.h, self._p(params), idx, n, self._p(u), self._p(G), self._p(vals[0:1]), self._p(vals[1:2]),
                                                 self._p(vals[2:3])))
        return u, G, vals[0:1], vals[1:2], vals[2:3]

    def bam_moments_host(self, params, idx, n_samples):
        """mivi_bam_moments_host on a numpy parameter vector: (u (d, n), G (d, n), fisher, logpi_avg, elbo)."""
        n = int(n_samples)
        p = np.ascontiguousarray(params, dtype=self.np_dtype)
        u = np.zeros((self.d, max(n, 0)), dtype=self.np_dtype, order="F")
        G = np.zeros((self.d, max(n, 0)), dtype=self.np_dtype, order="F")
        vals = np.zeros(3, dtype=self.np_dtype)
        it = vals.itemsize
        self._raise_cb(self.lib.mivi_bam_moments_host(self.h, p.ctypes.data, idx, n, u.ctypes.data, G.ctypes.data, vals.ctypes.data,
                                                      vals.ctypes.data + it, vals.ctypes.data + 2 * it))
        return u, G, vals[0], vals[1], vals[2]

    def estimate_fisher(self, params, idx, n_samples, value=None):
        """mivi_estimate_fisher: the covariance-weighted Fisher divergence estimate, any n_samples >= 2; a 1-element device tensor."""
        p = self.to_device(params)
        value = self.empty(1) if value is None else value
        self._raise_cb(self.lib.mivi_estimate_fisher(self.h, self._p(p), idx, int(n_samples), self._p(value)))
        return value

    def estimate_fisher_host(self, params, idx, n_samples):
        p = np.ascontiguousarray(params, dtype=self.np_dtype)
        value = np.zeros(1, dtype=self.np_dtype)
        self._raise_cb(self.lib.mivi_estimate_fisher_host(self.h, p.ctypes.data, idx, int(n_samples), value.ctypes.data))
        return value[0]

    def bam_update(self, params, state, u, G, n_samples, lam, entropy=None):
        """mivi_bam_update: (m, C, Sigma) -> (m', C', Sigma') in place on the device tensors `params` and `state` from the flat device
        tensors u and G (d * n_samples, column-major, read-only); returns entropy(q') as a 1-element device tensor."""
        entropy = self.empty(1) if entropy is None else entropy
        self._chk(self.lib.mivi_bam_update(self.h, self._p(params), self._p(state), self._p(u), self._p(G), int(n_samples), float(lam),
                                           self._p(entropy)))
        return entropy

    def bam_update_host(self, params, state, u, G, lam):
        """mivi_bam_update_host on numpy arrays: params ([m; vec C]), state (Sigma, d^2 or (d, d)), u and G ((d, n) matrices); returns
        (params', state' (flat, column-major), entropy(q'))."""
        p = np.array(params, dtype=self.np_dtype, copy=True)
        st = np.array(np.asarray(state).reshape(-1, order="F"), dtype=self.np_dtype, copy=True)
        uu, GG = np.asfortranarray(u, dtype=self.np_dtype), np.asfortranarray(G, dtype=self.np_dtype)
        ent = np.zeros(1, dtype=self.np_dtype)
        self._chk(self.lib.mivi_bam_update_host(self.h, p.ctypes.data, st.ctypes.data, uu.ctypes.data, GG.ctypes.data, int(uu.shape[1]), float(lam),
                                                ent.ctypes.data))
        return p, st, ent[0]

    def bam_steps(self, params, state, idx0, iteration0, count, n_samples, fisher=None, elbo=None):
        """mivi_bam_steps: `count` whole steps {objective (index idx0 + t), update (lambda = d n / (iteration0 + t))} on the device tensors
        `params` and `state`; returns (fisher (count), elbo (count)), both at the iterate each step started from."""
        fisher = self.empty(int(count)) if fisher is None else fisher
        elbo = self.empty(int(count)) if elbo is None else elbo
        self._raise_cb(self.lib.mivi_bam_steps(self.h, self._p(params), self._p(state), idx0, int(iteration0), int(count), int(n_samples),
                                               self._p(fisher), self._p(elbo)))
        return fisher, elbo

    # -- KLMinWassFwdBwd (mivi_wass_*: klminwassfwdbwd.jl) ----------------------------------------------------------------------
    def wass_init(self, params, state=None):
        """mivi_wass_init: the device tensor Sigma = C C' (d^2, column-major, triangles bitwise mirrored) of the device parameters `params`."""
        state = self.empty(self.d * self.d) if state is None else state
        self._chk(self.lib.mivi_wass_init(self.h, self._p(params), self._p(state)))
        return state

    def wass_update(self, params, state, grad, hess, stepsize, entropy=None):
        """mivi_wass_update: the proximal (forward-backward) update of the device tensors `params` ([m; vec C]) and `state` (Sigma) in place
        from grad (d) and hess (d*d column-major, as gauss_expected_grad_hess fills it); returns entropy(q') as a 1-element device tensor."""
        entropy = self.empty(1) if entropy is None else entropy
        hess = hess.t() if hess.dim() == 2 else hess   # the (d, d) matrix view gauss_expected_grad_hess returns -> its column-major storage
        if not hess.is_contiguous():
            hess = hess.contiguous()
        self._chk(self.lib.mivi_wass_update(self.h, self._p(params), self._p(state), self._p(grad), self._p(hess), float(stepsize),
                                            self._p(entropy)))
        return entropy

    def wass_update_host(self, params, state, grad, hess, stepsize):
        """mivi_wass_update_host on numpy arrays: params ([m; vec C]), state (Sigma, d^2 or (d, d)), grad (d), hess ((d, d) matrix); returns
        (params', state' (flat, column-major), entropy(q'))."""
        p = np.array(params, dtype=self.np_dtype, copy=True)
        st = np.array(np.asarray(state).reshape(-1, order="F"), dtype=self.np_dtype, copy=True)
        g = np.ascontiguousarray(grad, dtype=self.np_dtype)
        H = np.asfortranarray(hess, dtype=self.np_dtype)
        ent = np.zeros(1, dtype=self.np_dtype)
        self._chk(self.lib.mivi_wass_update_host(self.h, p.ctypes.data, st.ctypes.data, g.ctypes.data, H.ctypes.data, float(stepsize),
                                                 ent.ctypes.data))
        return p, st, ent[0]

    def wass_steps(self, params, state, idx0, count, stepsize, n_samples=0, second_order=False, elbo=None):
        """mivi_wass_steps: `count` iterations {estimator (index idx0 + t), update} on the device tensors `params` and `state`; returns
        elbo (count)."""
        elbo = self.empty(int(count)) if elbo is None else elbo
        self._raise_cb(self.lib.mivi_wass_steps(self.h, self._p(params), self._p(state), idx0, int(count), int(n_samples),
                                                1 if second_order else 0, float(stepsize), self._p(elbo)))
        return elbo

    def estimate_partials(self, params, idx, partials=None):
        p = self.to_device(params)
        partials = self.empty(self.partials_len) if partials is None else partials
        self._raise_cb(self.lib.mivi_estimate_partials(self.h, self._p(p), idx, self._p(partials)))
        return partials

    def finalize(self, params, partials, value=None, grad=None):
        p = self.to_device(params)
        value = self.empty(1) if value is None else value
        grad = self.empty(self.params_len) if grad is None else grad
        self._chk(self.lib.mivi_finalize(self.h, self._p(p), self._p(partials), self._p(value), self._p(grad)))
        return value, grad

    def set_logreg_route(self, route):
        """0 = by problem size, 1 = matrix-core kernels, 2 = VALU kernels (built-in logistic regression, f32)."""
        self._chk(self.lib.mivi_set_logreg_route(self.h, int(route)))

    def set_index_source(self, idx_tensor):
        """idx_tensor: 1-element int64/uint64 device tensor added to every estimate index (None to unset)."""
        self._idx_src = idx_tensor
        self._chk(self.lib.mivi_set_index_source(self.h, self._p(idx_tensor) if idx_tensor is not None else None))

    def profile_kernel(self, which, params, reps):
        """ms per launch of one pipeline stage, hipEvent-timed on the context's stream (mivi_profile_kernel)."""
        ms = C.c_double(0.0)
        self._chk(self.lib.mivi_profile_kernel(self.h, int(which), self._p(params), int(reps), C.byref(ms)))
        return ms.value

    def batch_lanes(self, count):
        """Estimates per launch the batch engine uses for a `count`-estimate call (mivi_batch_lanes)."""
        return int(self.lib.mivi_batch_lanes(self.h, int(count)))

    def batch_takes_engine(self, params):
        """True when batches of estimates at this configuration run on the batch engine (mivi_batch_info what = 0)."""
        return int(self.lib.mivi_batch_info(self.h, self._p(params), 0)) == 1

    def graph_recordings(self):
        """hipGraphs recorded into the context's graph cache so far (mivi_batch_info what = 4): unchanged across two calls = the second replayed."""
        return int(self.lib.mivi_batch_info(self.h, None, 4))

    def live_allocations(self):
        """Device allocations the library holds right now in this process, over all contexts (mivi_batch_info what = 5): equal before a
        context's creation and after its close() = the context returned everything."""
        return int(self.lib.mivi_batch_info(self.h, None, 5))

    def live_handles(self):
        """Streams, events and graph execs the library holds right now in this process, over all contexts (mivi_batch_info what = 6):
        equal before a context's creation and after its close() = the context destroyed every handle it created."""
        return int(self.lib.mivi_batch_info(self.h, None, 6))

    def exchange_lost(self):
        """True once a launch-free loop's grid-wide exchange was lost on this context: the loops with a per-step exchange are then not taken
        again, their graph-of-launches equivalents run instead (mivi_batch_info what = 3)."""
        return int(self.lib.mivi_batch_info(self.h, None, 3)) == 1

    def split_products(self):
        """Matrix-pipe products per product block of the engine's split-operand contractions (mivi_batch_info what = 1)."""
        return int(self.lib.mivi_batch_info(self.h, None, 1))

    def plane_bytes(self):
        """Bytes per operand-plane element of the batch engine (mivi_batch_info what = 2)."""
        return int(self.lib.mivi_batch_info(self.h, None, 2))

    def profile_batch(self, params, lanes, reps):
        """Average launch duration (us) of the batch engine's kernels for `lanes` estimates (mivi_profile_batch):
        dict(eps=.., product=.., vjp=.., dense_product=.., stl_product=..) -- dense_product 0 unless the target is the dense Gaussian,
        stl_product 0 unless the estimator is one of the sticking-the-landing ones."""
        us = (C.c_double * 5)()
        self._chk(self.lib.mivi_profile_batch(self.h, self._p(params), int(lanes), int(reps), us))
        return dict(eps=us[0], product=us[1], vjp=us[2], dense_product=us[3], stl_product=us[4])

    # -- sharded finalisation / collective behind the ABI ----------------------------------------------------------
    def slice_len(self, world):
        return int(self.lib.mivi_slice_len(self.h, int(world)))

    def finalize_slice(self, params, slice_sum, rank, world, out=None):
        out = self.empty(self.slice_len(world)) if out is None else out
        self._chk(self.lib.mivi_finalize_slice(self.h, self._p(params), self._p(slice_sum), int(rank), int(world), self._p(out)))
        return out

    def unpack_final(self, packed_final, value=None, grad=None):
        value = self.empty(1) if value is None else value
        grad = self.empty(self.params_len) if grad is None else grad
        self._chk(self.lib.mivi_unpack_final(self.h, self._p(packed_final), self._p(value), self._p(grad)))
        return value, grad

    def comm_unique_id(self):
        buf = (C.c_char * 128)()
        _lib.check(self.lib, self.h, self.lib.mivi_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, unique_id, rank, world):
        self._chk(self.lib.mivi_comm_init(self.h, unique_id, int(rank), int(world)))

    # -- the exchange written for xGMI (kernels_p2p.hip) ------------------------------------------------------------------
    P2P_HANDLE_BYTES = 256
    ROUTES = {"auto": 0, "allreduce": 1, "rsag": 2, "p2p": 3}

    def p2p_export(self, rank, world):
        buf = (C.c_char * self.P2P_HANDLE_BYTES)()
        self._chk(self.lib.mivi_p2p_export(self.h, int(rank), int(world), buf))
        return bytes(buf)

    def p2p_attach(self, handles):
        """handles: the `world` blobs of p2p_export in rank order (bytes or a list of bytes)."""
        blob = b"".join(handles) if isinstance(handles, (list, tuple)) else bytes(handles)
        self._chk(self.lib.mivi_p2p_attach(self.h, blob))

    def p2p_detach(self):
        self._chk(self.lib.mivi_p2p_detach(self.h))

    def p2p_set_pipeline(self, on):
        """False: serial steps; True (default): the persistent exchange kernel beside the compute chain."""
        self._chk(self.lib.mivi_p2p_set_pipeline(self.h, 1 if on else 0))

    def p2p_set_spin_budget(self, polls):
        self._chk(self.lib.mivi_p2p_set_spin_budget(self.h, int(polls)))

    def comm_enable_p2p(self):
        self._chk(self.lib.mivi_comm_enable_p2p(self.h))

    def p2p_selfcheck(self, params, idx=3):
        """mivi_p2p_selfcheck: the peer-to-peer exchange against the RCCL all-reduce on one sharded estimate, collectively; returns
        dict(value_rel, grad_rel_l2, verified).  Only a verified context takes the peer-to-peer route automatically at world > 1."""
        out = (C.c_double * 3)()
        self._chk(self.lib.mivi_p2p_selfcheck(self.h, self._p(params), int(idx), out))
        return dict(value_rel=out[0], grad_rel_l2=out[1], verified=bool(out[2]))

    def comm_set_route(self, route):
        self._chk(self.lib.mivi_comm_set_route(self.h, self.ROUTES.get(route, route)))

    def comm_route(self):
        return {0: "none", 1: "allreduce", 2: "rsag", 3: "p2p"}[int(self.lib.mivi_comm_route(self.h))]

    def p2p_exchange(self, params, partials, value, grad, phases=7):
        """partials = None: direct mode (p2p_partials_direct stored the vector into the owners' staging areas)."""
        self._chk(self.lib.mivi_p2p_exchange(self.h, self._p(params), self._p(partials) if partials is not None else None, self._p(value),
                                             self._p(grad), int(phases)))

    def p2p_stats(self, reset=False):
        """Exchange diagnostics since the last reset (mivi_p2p_stats): waits in us, groups served, bytes per peer and estimate."""
        out = (C.c_double * 6)()
        self._chk(self.lib.mivi_p2p_stats(self.h, out, 1 if reset else 0))
        return dict(wait_handover_us=out[0], wait_pushes_us=out[1], wait_finals_us=out[2], groups=int(out[3]), bytes_per_peer_per_estimate=out[4],
                    slice_elements=int(out[5]))

    def p2p_partials_direct(self, params, idx):
        self._chk(self.lib.mivi_p2p_partials_direct(self.h, self._p(params), int(idx)))

    def estimate_gradient_dist_n(self, params, idx0, count, value, grad):
        self._chk(self.lib.mivi_estimate_gradient_dist_n(self.h, self._p(params), idx0, int(count), self._p(value), self._p(grad)))

    def profile_dist(self, params, reps):
        """us per estimate: dict(partials, exchange, serial, pipelined) (mivi_profile_dist; every rank calls it collectively)."""
        out = (C.c_double * 4)()
        self._chk(self.lib.mivi_profile_dist(self.h, self._p(params), int(reps), out))
        return dict(partials=out[0], exchange=out[1], serial=out[2], pipelined=out[3])

    def estimate_gradient_dist(self, params, idx, value=None, grad=None):
        p = self.to_device(params)
        value = self.empty(1) if value is None else value
        grad = self.empty(self.params_len) if grad is None else grad
        self._raise_cb(self.lib.mivi_estimate_gradient_dist(self.h, self._p(p), idx, self._p(value), self._p(grad)))
        return value, grad

    def fullrank_route(self, n_samples=0):
        """(generation, bf16x3): which full-rank kernels run for n_samples per launch (mivi_fullrank_route)."""
        r = int(self.lib.mivi_fullrank_route(self.h, int(n_samples)))
        return r & 3, bool(r & 16)

    def logreg_kernels(self, n_samples=0):
        """dict(mfma, logits_planes, xtr_planes): which kernels the native logistic-regression target's contractions run (mivi_logreg_kernels)."""
        r = int(self.lib.mivi_logreg_kernels(self.h, int(n_samples)))
        return dict(mfma=bool(r & 1), logits_planes=bool(r & 2), xtr_planes=bool(r & 4))

    # -- next to the hot path ---------------------------------------------------------------------
    def clip_scale(self, params, epsilon):
        self._chk(self.lib.mivi_clip_scale(self.h, self._p(params), float(epsilon)))

    def prox_scale_entropy(self, params, stepsize=0.0, dog_state=None, dog_kind=0):
        self._chk(self.lib.mivi_prox_scale_entropy(self.h, self._p(params), float(stepsize),
                                                   self._p(dog_state) if dog_state is not None else None, int(dog_kind)))

    def descent_update(self, params, grad, eta):
        self._chk(self.lib.mivi_descent_update(self.h, self._p(params), self._p(grad), float(eta)))

    def adam_update(self, params, grad, state, t, eta, beta1=0.9, beta2=0.999, eps=1e-8):
        self._chk(self.lib.mivi_adam_update(self.h, self._p(params), self._p(grad), self._p(state), int(t), eta, beta1, beta2, eps))

    def cocob_update(self, params, grad, state, alpha=100.0):
        self._chk(self.lib.mivi_cocob_update(self.h, self._p(params), self._p(grad), self._p(state), float(alpha)))

    def axpby(self, y, a, x, b):
        self._chk(self.lib.mivi_axpby(self.h, self._p(y), float(a), self._p(x), float(b), y.numel()))

    def dog_state(self):
        torch = _torch()
        return torch.zeros(int(self.lib.mivi_dog_state_bytes(self.h)), dtype=torch.uint8, device=self.tdevice)

    def dog_init(self, params, state, alpha):
        self._chk(self.lib.mivi_dog_init(self.h, self._p(params), self._p(state), float(alpha)))

    def dog_update(self, params, grad, state, kind):
        self._chk(self.lib.mivi_dog_update(self.h, self._p(params), self._p(grad), self._p(state), int(kind)))

    def optimize_loop(self, params, n_steps, idx0, t0, rule=0, op=0, averager=0, eta=0.0, beta=(0.9, 0.999), adam_eps=1e-8,
                      clip_epsilon=0.0, avg_eta=8.0, opt_state=None, avg_params=None, elbo=None):
        """mivi_optimize_loop: n_steps iterations of {estimate, update, operator, averager} on the device."""
        import ctypes as C
        l = _lib.MiviLoop(int(rule), int(op), int(averager), int(n_steps), float(eta), float(beta[0]), float(beta[1]),
                          float(adam_eps), float(clip_epsilon), float(avg_eta),
                          self._p(opt_state) if opt_state is not None else None,
                          self._p(avg_params) if avg_params is not None else None, int(idx0), int(t0),
                          self._p(elbo) if elbo is not None else None)
        self._chk(self.lib.mivi_optimize_loop(self.h, self._p(params), C.byref(l)))

    def last_loop(self):
        """The route the last optimize_loop / optimize_loop_many call ran on (mivi_batch_info what = 7): 0 the graph of launches, a
        launch-free loop's id, or 16 | that id after optimize_loop_many."""
        return int(self.lib.mivi_batch_info(self.h, None, 7))

    def optimize_loop_many(self, params, n_runs, n_steps, idx0, t0, seeds=None, etas=None, means=None, stds=None, y=None, X=None,
                           x_stride=0, rule=0, op=0, averager=0, eta=0.0, beta=(0.9, 0.999), adam_eps=1e-8, clip_epsilon=0.0, avg_eta=8.0,
                           opt_state=None, avg_params=None, elbo=None, want_status=True):
        """mivi_optimize_loop_many: n_runs independent runs of optimize_loop in one launch, workgroup k = run k.  Run-major device arrays:
        params [K params_len], opt_state K single-run states, avg_params [K params_len], elbo [K n_steps].  idx0: one first estimate
        index or K of them; seeds / etas: K values or None (the context's seed, `eta`); means / stds: [K, d] host arrays (diagonal-Gaussian
        target) or None; y: device uint8 [K n], X: device matrix or K of them x_stride elements apart (logistic regression) or None.
        Returns the runs' status words (int32[K]: bit 1 non-finite objective, bit 2 non-positive scale); want_status=False: None, and a set
        bit raises as optimize_loop does."""
        K = int(n_runs)
        keep = []
        torch = _torch()

        def host(a, dt, count, name):   # a per-run host array of EXACTLY `count` entries (the library reads that many)
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            if a.size != count:
                raise ValueError(f"optimize_loop_many: {name} holds {a.size} entries, {count} are needed for {K} runs")
            keep.append(a)
            return a.ctypes.data

        def dev(t, dt, at_least, name, exact=True):   # a device array of the element type and size the kernel indexes
            if t is None:
                return
            if not isinstance(t, torch.Tensor) or t.device != self.tdevice or t.dtype != dt or not t.is_contiguous():
                raise ValueError(f"optimize_loop_many: {name} must be a contiguous {dt} tensor on {self.tdevice}")
            if (t.numel() != at_least) if exact else (t.numel() < at_least):
                raise ValueError(f"optimize_loop_many: {name} holds {t.numel()} entries, {at_least} are needed for {K} runs")

        if K >= 1:
            plen = self.params_len
            dev(params, self.tdtype, K * plen, "params")
            dev(avg_params, self.tdtype, K * plen, "avg_params")
            dev(elbo, self.tdtype, K * int(n_steps), "elbo")
            if opt_state is not None and int(rule) == 1:
                dev(opt_state, self.tdtype, 2 * K * plen, "opt_state")
            elif opt_state is not None and int(rule) in (2, 3):
                dev(opt_state, torch.uint8, K * int(self.lib.mivi_dog_state_bytes(self.h)), "opt_state")
            lr = getattr(self, "_lr_full", None)
            if (y is not None or X is not None) and lr is None:
                raise ValueError("optimize_loop_many: y / X are for a context with a LogRegProblem")
            if lr is not None:
                n, p = lr.n_rows(), self.d - 1
                dev(y, torch.uint8, K * n, "y")
                if X is not None and int(x_stride) != 0 and int(x_stride) < n * p:
                    raise ValueError("optimize_loop_many: x_stride must be 0 (one shared X) or at least n (d - 1)")
                dev(X, self.tdtype, (K - 1) * int(x_stride) + n * p, "X", exact=False)

        idx_arr = None if np.ndim(idx0) == 0 else idx0
        status = np.zeros(K, dtype=np.int32) if want_status else None
        m = _lib.MiviMany(K, host(seeds, np.uint64, K, "seeds"), host(idx_arr, np.uint64, K, "idx0"), host(etas, np.float64, K, "etas"),
                          host(means, self.np_dtype, K * self.d, "means"), host(stds, self.np_dtype, K * self.d, "stds"),
                          self._p(y) if y is not None else None, self._p(X) if X is not None else None, int(x_stride),
                          status.ctypes.data if want_status else None)
        l = _lib.MiviLoop(int(rule), int(op), int(averager), int(n_steps), float(eta), float(beta[0]), float(beta[1]),
                          float(adam_eps), float(clip_epsilon), float(avg_eta),
                          self._p(opt_state) if opt_state is not None else None,
                          self._p(avg_params) if avg_params is not None else None, int(idx0) if idx_arr is None else 0, int(t0),
                          self._p(elbo) if elbo is not None else None)
        self._chk(self.lib.mivi_optimize_loop_many(self.h, self._p(params), C.byref(l), C.byref(m)))
        return status

    # -- a schedule of minibatches resident on the device (the built-in logistic regression) ----------
    def set_batch_schedule(self, rows, estimate_idx=None, likeadj=None, kernels=0):
        """mivi_logreg_set_batch_schedule: rows int[n_batches, batch] (0-based rows of the resident data set), estimate_idx
        uint64[n_batches] or None, likeadj = n_data / batch (None: the data set's row count over `batch`).  rows = None or an empty
        schedule removes it (the full data set again).  After the call the target is batch 0."""
        if rows is None or np.size(rows) == 0:
            sched = _lib.MiviBatchSchedule(None, None, 0, 0, 0, 1.0)
            self._chk(self.lib.mivi_logreg_set_batch_schedule(self.h, C.byref(sched)))
            return
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        if rows.ndim != 2:
            raise ValueError("rows must be a matrix: one row of data-set indices per batch")
        n_batches, batch = rows.shape
        idx = None
        if estimate_idx is not None:
            idx = np.ascontiguousarray(estimate_idx, dtype=np.uint64)
            if idx.shape != (n_batches,):
                raise ValueError("estimate_idx must hold one index per batch")
        if likeadj is None:
            full = getattr(self, "_lr_full", None)
            if full is None:
                raise ValueError("likeadj is needed: the context holds no LogRegProblem to take n_data from")
            likeadj = full.likeadj * full.n_rows() / batch   # (what LogRegSubset gives a batch of that size)
        sched = _lib.MiviBatchSchedule(rows.ctypes.data, idx.ctypes.data if idx is not None else None, batch, n_batches, int(kernels),
                                       float(likeadj))
        self._chk(self.lib.mivi_logreg_set_batch_schedule(self.h, C.byref(sched)))

    def seek_batch(self, k):
        """mivi_logreg_seek_batch: the target becomes batch k of the schedule (host-side: no device work)."""
        self._chk(self.lib.mivi_logreg_seek_batch(self.h, int(k)))

    def batch_route(self, n_samples=0):
        """Which kernels evaluate the selected batch of a scheduled context for n_samples per launch: 1 the fused minibatch kernel,
        2 the device gather + the resident-data kernels; 0 without a schedule (mivi_logreg_kernels, bits 3 and 4)."""
        r = int(self.lib.mivi_logreg_kernels(self.h, int(n_samples)))
        return 1 if r & 8 else (2 if r & 16 else 0)

    def optimize_loop_batches(self, params, n_steps, idx0, t0, first_batch=0, rule=0, op=0, averager=0, eta=0.0, beta=(0.9, 0.999),
                              adam_eps=1e-8, clip_epsilon=0.0, avg_eta=8.0, opt_state=None, avg_params=None, elbo=None):
        """mivi_optimize_loop_batches: optimize_loop where step t evaluates batch first_batch + t of the schedule (and draws at that
        batch's estimate index when the schedule carries them; at idx0 + t otherwise)."""
        l = _lib.MiviLoop(int(rule), int(op), int(averager), int(n_steps), float(eta), float(beta[0]), float(beta[1]),
                          float(adam_eps), float(clip_epsilon), float(avg_eta),
                          self._p(opt_state) if opt_state is not None else None,
                          self._p(avg_params) if avg_params is not None else None, int(idx0), int(t0),
                          self._p(elbo) if elbo is not None else None)
        self._chk(self.lib.mivi_optimize_loop_batches(self.h, self._p(params), C.byref(l), int(first_batch)))

    def optimize_steps(self, params, opt_state, idx0, t0, n_steps, rule, eta, clip_epsilon, elbo=None):
        st = self.lib.mivi_optimize_steps(self.h, self._p(params), self._p(opt_state) if opt_state is not None else None,
                                          idx0, int(t0), int(n_steps), int(rule), float(eta), float(clip_epsilon),
                                          self._p(elbo) if elbo is not None else None)
        self._chk(st)
