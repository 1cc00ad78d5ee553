// libmivi C ABI, part 11: KLMinNaturalGradDescent (src/algorithms/klminnaturalgraddescent.jl) -- the state of `init` (:83-87) and the
// natural-gradient update of `step` (:129-145) on the device-resident [m; vec C] and [S; Sigma] (kernels_natgrad.hip), and whole steps
// {estimator, update} without a host round trip.  As in api_ngd.hip a step is the existing estimator entry into context-owned buffers followed
// by the update, whose last launch also forms elbo = logpi_avg + entropy(q') (:145) and the sticky flags: launches are fused, arithmetic is
// not, so mivi_natgrad_steps is bitwise the single calls.  The scale convention (a LOWER-triangular C', where the reference's new scale is
// upper triangular) is stated in kernels_natgrad.hip and include/mivi.h.
#include "api_common.h"

static mivi_status_t natgrad_scratch(mivi_ctx *c) {
  mivi_status_t s;
  if (natgrad_work_bytes(c) && ((s = ensure(c, c->natgrad_work, natgrad_work_bytes(c), false)) || (s = ensure(c, c->natgrad_part, natgrad_part_bytes(c), false))))
    return s;
  return MIVI_OK;
}

static mivi_status_t natgrad_update(mivi_ctx *c, void *params, void *state, const void *grad, const void *hess, double stepsize, int ensure_posdef,
                                    const void *logpi, void *entropy, void *elbo) {
  const mivi_status_t s = natgrad_scratch(c);
  if (s) return s;
  launch_natgrad_update(c, params, state, grad, hess, stepsize, ensure_posdef, logpi, entropy, elbo);
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

extern "C" {

mivi_status_t mivi_natgrad_init(mivi_ctx_t *c, const void *params, void *state) {
  if (!c || !params || !state) return MIVI_ERR_BAD_ARG;
  if (c->cfg.family != MIVI_FULLRANK) return fail(c, MIVI_ERR_UNSUPPORTED, "natgrad_init takes a triangular scale (full-rank family)");
  (void)hipSetDevice(c->cfg.device);
  const mivi_status_t s = natgrad_scratch(c);
  if (s) return s;
  launch_natgrad_init(c, const_cast<void *>(params), state);
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

mivi_status_t mivi_natgrad_update(mivi_ctx_t *c, void *params, void *state, const void *grad, const void *hess, double stepsize,
                                  int32_t ensure_posdef, void *entropy) {
  if (!c || !params || !state || !grad || !hess) return MIVI_ERR_BAD_ARG;
  if (c->cfg.family != MIVI_FULLRANK) return fail(c, MIVI_ERR_UNSUPPORTED, "natgrad_update takes a triangular scale (full-rank family)");
  (void)hipSetDevice(c->cfg.device);
  return natgrad_update(c, params, state, grad, hess, stepsize, ensure_posdef, nullptr, entropy, nullptr);
}

mivi_status_t mivi_natgrad_update_host(mivi_ctx_t *c, void *params_h, void *state_h, const void *grad_h, const void *hess_h, double stepsize,
                                       int32_t ensure_posdef, void *entropy_h) {
  if (!c || !params_h || !state_h || !grad_h || !hess_h) return MIVI_ERR_BAD_ARG;
  if (c->cfg.family != MIVI_FULLRANK) return fail(c, MIVI_ERR_UNSUPPORTED, "natgrad_update takes a triangular scale (full-rank family)");
  (void)hipSetDevice(c->cfg.device);
  const size_t es = c->esize, d = (size_t)c->cfg.d;
  NgdEst e;   // (its scalar: the entropy)
  mivi_status_t s;
  if ((s = ngd_est(c, &e)) || (s = ensure(c, c->natgrad_host, 2 * d * d * es, false)) || (s = stage_params(c, params_h))) return s;
  HIPCHK(c, hipMemcpyAsync(c->natgrad_host.p, state_h, 2 * d * d * es, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(e.grad, grad_h, d * es, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(e.hess, hess_h, d * d * es, hipMemcpyHostToDevice, c->stream));
  if ((s = natgrad_update(c, c->tmp_params.p, c->natgrad_host.p, e.grad, e.hess, stepsize, ensure_posdef, nullptr, e.scalar, nullptr))) return s;
  return fetch_results(
      c, {{params_h, c->tmp_params.p, (size_t)mivi_params_len(c) * es}, {state_h, c->natgrad_host.p, 2 * d * d * es}, {entropy_h, e.scalar, es}}, true);
}

mivi_status_t mivi_natgrad_steps(mivi_ctx_t *c, void *params, void *state, uint64_t idx0, int32_t count, int32_t n_samples, int32_t second_order,
                                 double stepsize, int32_t ensure_posdef, void *elbo) {
  if (!c || !params || !state || count < 0) return MIVI_ERR_BAD_ARG;
  if (c->cfg.family != MIVI_FULLRANK)
    return fail(c, MIVI_ERR_UNSUPPORTED, "natgrad_steps: KLMinNaturalGradDescent takes a triangular scale (full-rank family)");
  if (c->cfg.m_offset != 0 || (c->cfg.m_total != 0 && c->cfg.m_total != c->cfg.n_mc))
    return fail(c, MIVI_ERR_UNSUPPORTED, "natgrad_steps: a sharded context is not supported (the update needs the whole estimate)");
  if (c->target == TGT_NONE) return fail(c, MIVI_ERR_NO_TARGET, "no target set");
  (void)hipSetDevice(c->cfg.device);
  NgdEst e;   // (its scalar: logpi_avg)
  mivi_status_t s;
  if ((s = ngd_est(c, &e)) || (s = natgrad_scratch(c))) return s;   // (everything that can fail for want of memory, before any launch)
  for (int32_t t = 0; t < count; ++t) {
    // (the estimator entries refuse what they cannot do before they launch anything, so a refused call leaves parameters and state untouched)
    s = second_order ? mivi_gauss_expected_grad_hess2(c, params, idx0 + (uint64_t)t, n_samples, e.scalar, e.grad, e.hess)
                     : mivi_gauss_expected_grad_hess(c, params, idx0 + (uint64_t)t, n_samples, e.scalar, e.grad, e.hess);
    if (s) return s;
    if ((s = natgrad_update(c, params, state, e.grad, e.hess, stepsize, ensure_posdef, e.scalar, nullptr,
                            elbo ? (char *)elbo + (size_t)t * c->esize : nullptr)))
      return s;
  }
  return MIVI_OK;
}

}  // extern "C"
