// libmivi C ABI: the extended Stacked bijector -- truncated(lb, ub) and ordered blocks (kernels_bijector.hip) next to identity / exp -- and
// the constrained approximation Bijectors.TransformedDistribution(q, binv) people sample from and score
// (docs/src/tutorials/basic.md:210-247, constrained.md:228-231): mivi_sample_constrained, mivi_logpdf_constrained[_host].
// Every estimate route reaches the new kinds through launch_bij_forward / launch_bij_backward (kernels_targets.hip), which dispatch on
// mivi_ctx::bij_ext; a bijector of identity / exp blocks alone is handed to mivi_set_bijector_stacked and launches what it always did.
#include "api_common.h"

// the device copy of the per-coordinate description (codes, bounds); the legacy setter leaves it to the first constrained rand / logpdf
static mivi_status_t bij_tables(mivi_ctx *c) {
  if (c->bij_tab) return MIVI_OK;
  const size_t d = c->cfg.d;
  mivi_status_t s;
  if ((s = ensure(c, c->bij_code, d, false)) || (s = ensure(c, c->bij_bnd, 2 * d * sizeof(double), false))) return s;
  HIPCHK(c, hipStreamSynchronize(c->stream));   // a launch in flight may still read the old tables
  HIPCHK(c, hipMemcpy(c->bij_code.p, c->bij_code_h.data(), d, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->bij_bnd.p, c->bij_bnd_h.data(), 2 * d * sizeof(double), hipMemcpyHostToDevice));
  c->bij_ord = false;
  for (uint8_t k : c->bij_code_h) c->bij_ord = c->bij_ord || k == BIJ_ORD;
  c->bij_tab = true;
  return MIVI_OK;
}

mivi_status_t mivi_set_bijector_stacked_ex(mivi_ctx_t *c, int32_t n_blocks, const int32_t *ranges, const int32_t *kinds, const double *bounds) {
  if (!c || n_blocks < 0 || (n_blocks > 0 && (!ranges || !kinds))) return MIVI_ERR_BAD_ARG;
  const int d = c->cfg.d;
  std::vector<uint8_t> code(d, BIJ_ID), seen(d, 0);
  std::vector<double> bnd(2 * (size_t)d, 0.0);
  std::vector<int32_t> legacy(n_blocks > 0 ? n_blocks : 0, 0);   // the same blocks in the legacy entry's kinds, if that is all they are
  bool ext = false;
  for (int b = 0; b < n_blocks; ++b) {
    const int lo = ranges[2 * b], hi = ranges[2 * b + 1], kd = kinds[b];
    if (lo < 0 || hi > d || lo > hi) return fail(c, MIVI_ERR_BAD_ARG, "stacked bijector: block range outside [0, d)");
    if (kd < MIVI_BIJ_IDENTITY || kd > MIVI_BIJ_ORDERED)
      return fail(c, MIVI_ERR_BAD_ARG, "stacked bijector: kind must be 0 (identity), 1 (exp), 2 (truncated) or 3 (ordered)");
    uint8_t first = BIJ_ID, rest = BIJ_ID;
    double lb = 0.0, ub = 0.0;
    if (kd == MIVI_BIJ_EXP) {
      first = rest = BIJ_LOWER;
      legacy[b] = MIVI_BIJ_EXP;
    } else if (kd == MIVI_BIJ_TRUNCATED) {
      if (!bounds) return fail(c, MIVI_ERR_BAD_ARG, "stacked bijector: a truncated block needs bounds_host");
      lb = bounds[2 * b];
      ub = bounds[2 * b + 1];
      if (isnan(lb) || isnan(ub)) return fail(c, MIVI_ERR_BAD_ARG, "stacked bijector: a bound of a truncated block is NaN");
      if (!(lb < ub)) return fail(c, MIVI_ERR_BAD_ARG, "stacked bijector: a truncated block needs lb < ub");
      const bool has_lb = !isinf(lb), has_ub = !isinf(ub);
      first = rest = has_lb && has_ub ? BIJ_BOTH : has_lb ? BIJ_LOWER : has_ub ? BIJ_UPPER : BIJ_ID;   // (lb = -inf, ub = +inf: identity)
      ext = ext || (first != BIJ_ID && hi > lo);
    } else if (kd == MIVI_BIJ_ORDERED && hi - lo >= 2) {   // (a block of length 1 is identity)
      first = BIJ_ORD_HEAD;
      rest = BIJ_ORD;
      ext = true;
    }
    for (int i = lo; i < hi; ++i) {
      if (seen[i]) return fail(c, MIVI_ERR_BAD_ARG, "stacked bijector: blocks overlap");
      seen[i] = 1;
      code[i] = i == lo ? first : rest;
      bnd[2 * (size_t)i] = isinf(lb) ? 0.0 : lb;
      bnd[2 * (size_t)i + 1] = isinf(ub) ? 0.0 : ub;
    }
  }
  // identity / exp blocks alone (a truncated(-inf, +inf) or a one-coordinate ordered block is identity): the legacy entry, its kernels, its buffers
  if (!ext) return mivi_set_bijector_stacked(c, n_blocks, ranges, legacy.data());
  (void)hipSetDevice(c->cfg.device);
  invalidate_graph(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));   // an estimate in flight may still read the old tables
  c->bij_code_h = code;
  c->bij_bnd_h = bnd;
  c->bij_tab = false;
  if (mivi_status_t s = bij_tables(c)) {   // the tables could not be placed: no bijector at all, not half of the old one and half of this
    c->bij_on = c->bij_ext = c->bij_ord = false;
    c->bij_code_h.assign((size_t)d, (uint8_t)BIJ_ID);
    c->bij_bnd_h.assign(2 * (size_t)d, 0.0);
    return s;
  }
  c->bij_on = c->bij_ext = true;
  c->cap_M = 0;   // (re)allocate the work buffers incl. the per-column log-Jacobian sums and the saved eta
  return MIVI_OK;
}

mivi_status_t mivi_sample_constrained(mivi_ctx_t *c, const void *params, uint64_t idx, void *X, void *eta) {
  if (!c || !params || !X) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t s = mivi_sample(c, params, idx, X, nullptr)) return s;
  if (!c->bij_on) {   // no bijector: X = eta
    if (eta) HIPCHK(c, hipMemcpyAsync(eta, X, (size_t)c->cfg.d * c->cfg.n_mc * c->esize, hipMemcpyDeviceToDevice, c->stream));
    return MIVI_OK;
  }
  if (mivi_status_t s = bij_tables(c)) return s;
  launch_bijx_forward(c, c->cfg.n_mc, X, eta, nullptr);
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

mivi_status_t mivi_logpdf_constrained(mivi_ctx_t *c, const void *params, const void *X, int64_t n, void *logq) {
  if (!c) return MIVI_ERR_BAD_ARG;
  if (!params || !X || !logq) return fail(c, MIVI_ERR_BAD_ARG, "mivi_logpdf_constrained: params, X and logq must not be NULL");
  if (n < 1 || n > (int64_t)0x7fffffff - kSampleChunk) return fail(c, MIVI_ERR_BAD_ARG, "mivi_logpdf_constrained: n must be in [1, 2^31 - 16385]");
  if (!c->bij_on) return mivi_logpdf(c, params, X, n, logq, nullptr);
  (void)hipSetDevice(c->cfg.device);
  const size_t d = c->cfg.d, es = c->esize;
  const size_t cap = n < kSampleChunk ? (size_t)n : (size_t)kSampleChunk, eb = (d * cap * es + 15) / 16 * 16;
  mivi_status_t s;
  if ((s = bij_tables(c)) || (s = ensure(c, c->bij_scr, eb + cap * (sizeof(double) + sizeof(int)), false))) return s;
  char *eta = (char *)c->bij_scr.p;
  double *ladj = (double *)(eta + eb);
  // eta = b(x) a chunk at a time in front of the density of q, minus logabsdetjac(binv, eta) behind it: the parameter-only stage runs once
  const LogpdfBij bij{(const char *)X, eta, ladj, (int *)(ladj + cap)};
  if ((s = logpdf_launches(c, params, nullptr, (int)n, (char *)logq, nullptr, &bij))) return s;
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

mivi_status_t mivi_logpdf_constrained_host(mivi_ctx_t *c, const void *params_h, const void *X_h, int64_t n, void *logq_h) {
  if (!c) return MIVI_ERR_BAD_ARG;
  if (!params_h || !X_h || !logq_h) return fail(c, MIVI_ERR_BAD_ARG, "mivi_logpdf_constrained_host: params, X and logq must not be NULL");
  if (n < 1 || n > (int64_t)0x7fffffff - kSampleChunk) return fail(c, MIVI_ERR_BAD_ARG, "mivi_logpdf_constrained_host: n must be in [1, 2^31 - 16385]");
  (void)hipSetDevice(c->cfg.device);
  const size_t es = c->esize, xb = (size_t)c->cfg.d * (size_t)n * es;
  mivi_status_t s = ensure(c, c->lp_host, xb + ((size_t)n * es + 15) / 16 * 16, false);
  if (s || (s = stage_params(c, params_h))) return s;
  char *Xd = (char *)c->lp_host.p, *qd = Xd + xb;
  HIPCHK(c, hipMemcpyAsync(Xd, X_h, xb, hipMemcpyHostToDevice, c->stream));
  if ((s = mivi_logpdf_constrained(c, c->tmp_params.p, Xd, n, qd))) return s;
  return fetch_results(c, {{logq_h, qd, (size_t)n * es}}, true);
}
