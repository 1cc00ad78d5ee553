// libmivi C ABI, part 10: KLMinSqrtNaturalGradDescent (src/algorithms/klminsqrtnaturalgraddescent.jl) -- the square-root natural-gradient
// update on the device-resident [m; vec C] (kernels_ngd.hip) and whole steps {estimator, update} without a host round trip.  A step is the
// existing estimator entry (mivi_gauss_expected_grad_hess / _hess2) into context-owned buffers followed by the update, whose last launch also
// forms elbo = logpi_avg + entropy(q') (klminsqrtnaturalgraddescent.jl:119) and the sticky flags: launches are fused, arithmetic is not, so
// mivi_sqrt_ngd_steps is bitwise the single calls.
#include "api_common.h"

static mivi_status_t ngd_update(mivi_ctx *c, void *params, const void *grad, const void *hess, double stepsize, const void *logpi, void *entropy,
                                void *elbo) {
  mivi_status_t s;
  if (ngd_work_bytes(c) && ((s = ensure(c, c->ngd_work, ngd_work_bytes(c), false)) || (s = ensure(c, c->ngd_part, ngd_part_bytes(c), false)))) return s;
  launch_ngd_update(c, params, grad, hess, stepsize, logpi, entropy, elbo);
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

mivi_status_t ngd_est(mivi_ctx *c, NgdEst *e) {
  const size_t es = c->esize, d = (size_t)c->cfg.d, goff = (d * es + 15) / 16 * 16;
  const mivi_status_t s = ensure(c, c->ngd_est, 16 + goff + d * d * es, false);
  if (s) return s;
  char *b = (char *)c->ngd_est.p;
  *e = NgdEst{b, b + 16, b + 16 + goff};
  return MIVI_OK;
}

extern "C" {

mivi_status_t mivi_sqrt_ngd_update(mivi_ctx_t *c, void *params, const void *grad, const void *hess, double stepsize, void *entropy) {
  if (!c || !params || !grad || !hess) return MIVI_ERR_BAD_ARG;
  if (c->cfg.family != MIVI_FULLRANK)
    return fail(c, MIVI_ERR_UNSUPPORTED, "sqrt_ngd_update takes a triangular scale (full-rank family)");
  (void)hipSetDevice(c->cfg.device);
  return ngd_update(c, params, grad, hess, stepsize, nullptr, entropy, nullptr);
}

mivi_status_t mivi_sqrt_ngd_update_host(mivi_ctx_t *c, void *params_h, const void *grad_h, const void *hess_h, double stepsize, void *entropy_h) {
  if (!c || !params_h || !grad_h || !hess_h) return MIVI_ERR_BAD_ARG;
  if (c->cfg.family != MIVI_FULLRANK)
    return fail(c, MIVI_ERR_UNSUPPORTED, "sqrt_ngd_update takes a triangular scale (full-rank family)");
  (void)hipSetDevice(c->cfg.device);
  const size_t es = c->esize, d = (size_t)c->cfg.d;
  NgdEst e;   // (its scalar: the entropy)
  mivi_status_t s;
  if ((s = ngd_est(c, &e)) || (s = stage_params(c, params_h))) return s;
  HIPCHK(c, hipMemcpyAsync(e.grad, grad_h, d * es, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(e.hess, hess_h, d * d * es, hipMemcpyHostToDevice, c->stream));
  if ((s = ngd_update(c, c->tmp_params.p, e.grad, e.hess, stepsize, nullptr, e.scalar, nullptr))) return s;
  return fetch_results(c, {{params_h, c->tmp_params.p, (size_t)mivi_params_len(c) * es}, {entropy_h, e.scalar, es}}, true);
}

mivi_status_t mivi_sqrt_ngd_steps(mivi_ctx_t *c, void *params, uint64_t idx0, int32_t count, int32_t n_samples, int32_t second_order,
                                  double stepsize, void *elbo) {
  if (!c || !params || count < 0) return MIVI_ERR_BAD_ARG;
  if (c->cfg.family != MIVI_FULLRANK)
    return fail(c, MIVI_ERR_UNSUPPORTED, "sqrt_ngd_steps: KLMinSqrtNaturalGradDescent takes a triangular scale (full-rank family)");
  if (c->cfg.m_offset != 0 || (c->cfg.m_total != 0 && c->cfg.m_total != c->cfg.n_mc))
    return fail(c, MIVI_ERR_UNSUPPORTED, "sqrt_ngd_steps: a sharded context is not supported (the update needs the whole estimate)");
  if (c->target == TGT_NONE) return fail(c, MIVI_ERR_NO_TARGET, "no target set");
  (void)hipSetDevice(c->cfg.device);
  NgdEst e;   // (its scalar: logpi_avg)
  mivi_status_t s;
  if ((s = ngd_est(c, &e))) return s;
  for (int32_t t = 0; t < count; ++t) {
    // (the estimator entries refuse what they cannot do -- no Hessian / a Stacked bijector for the second-order branch, d beyond the solve --
    // before they launch anything, so a refused call leaves the parameters untouched)
    s = second_order ? mivi_gauss_expected_grad_hess2(c, params, idx0 + (uint64_t)t, n_samples, e.scalar, e.grad, e.hess)
                     : mivi_gauss_expected_grad_hess(c, params, idx0 + (uint64_t)t, n_samples, e.scalar, e.grad, e.hess);
    if (s) return s;
    if ((s = ngd_update(c, params, e.grad, e.hess, stepsize, e.scalar, nullptr, elbo ? (char *)elbo + (size_t)t * c->esize : nullptr))) return s;
  }
  return MIVI_OK;
}

}  // extern "C"
