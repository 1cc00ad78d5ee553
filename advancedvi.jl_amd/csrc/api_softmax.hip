// libmivi C ABI, the softmax (multinomial logistic) regression target (include/mivi.h): mivi_set_target_softmax, the row selection
// mivi_softmax_select_rows (AdvancedVI.subsample) and the residual plane's cap.  The target is a GENERIC one: eval_generic_target
// (api_estimate.hip) evaluates it on explicit samples through launch_sm_target (kernels_softmax.hip), so every route that serves a callback
// target by explicit samples serves it, on the device; the target is a row of kTargets (api_common.h), whose refuse_target guards the entries that cannot.
#include "api_common.h"

mivi_status_t mivi_set_target_softmax(mivi_ctx_t *c, const void *X, const uint8_t *y, int64_t n, int32_t n_classes, int32_t variant,
                                      double likeadj, int32_t on_device) {
  if (!c || !X || !y) return MIVI_ERR_BAD_ARG;
  if (n < 1) return fail(c, MIVI_ERR_BAD_ARG, "softmax regression: n must be at least 1");
  if (n_classes < 2 || n_classes > MIVI_SOFTMAX_MAX_CLASSES) return fail(c, MIVI_ERR_BAD_ARG, "softmax regression: n_classes must lie in [2, 64]");
  const int d = c->cfg.d;
  if (d - 1 < n_classes || (d - 1) % n_classes != 0) return fail(c, MIVI_ERR_BAD_ARG, "softmax regression: d - 1 must be a positive multiple of n_classes (d = p n_classes + 1)");
  if (variant != 0 && variant != 1) return fail(c, MIVI_ERR_BAD_ARG, "softmax regression: unknown variant (0 logsigma_normal, 1 lognormal_exp_bijector)");
  if (!(likeadj > 0.0)) return fail(c, MIVI_ERR_BAD_ARG, "softmax regression: likelihood adjustment must be positive");
  if (!on_device)
    for (int64_t r = 0; r < n; ++r)
      if (y[r] >= n_classes) return fail(c, MIVI_ERR_BAD_ARG, "softmax regression: a label is not below n_classes");
  (void)hipSetDevice(c->cfg.device);
  const size_t p = (size_t)(d - 1) / n_classes;
  invalidate_graph(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));   // an estimate in flight may still read the previous data set
  if (on_device) {
    c->sm_X = X;
    c->sm_y = y;
  } else {
    mivi_status_t s;
    if ((s = ensure(c, c->sm_X_own, (size_t)n * p * c->esize, false)) || (s = ensure(c, c->sm_y_own, (size_t)n, false))) return s;
    HIPCHK(c, hipMemcpy(c->sm_X_own.p, X, (size_t)n * p * c->esize, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->sm_y_own.p, y, (size_t)n, hipMemcpyHostToDevice));
    c->sm_X = c->sm_X_own.p;
    c->sm_y = (const uint8_t *)c->sm_y_own.p;
  }
  c->sm_rows.set_full(n, likeadj);
  c->sm_C = n_classes;
  c->sm_variant = variant;
  c->lr_sched_n = c->lr_sched_k = 0;   // (a logistic regression's schedule of batches goes with its target)
  c->t_const = 0.0;
  c->target = TGT_SOFTMAX;
  return MIVI_OK;
}

mivi_status_t mivi_softmax_select_rows(mivi_ctx_t *c, const int64_t *idx, int64_t b, double likeadj) {
  if (!c || b < 0 || (b > 0 && !idx)) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_rows_of_other_target(c, "mivi_softmax_select_rows", TGT_SOFTMAX)) return rs;
  if (c->target != TGT_SOFTMAX) return fail(c, MIVI_ERR_NO_TARGET, "no softmax regression target set");
  (void)hipSetDevice(c->cfg.device);
  if (b > 0 && !(likeadj > 0.0)) return fail(c, MIVI_ERR_BAD_ARG, "likelihood adjustment must be positive");
  return select_rows(c, c->sm_rows, idx, b, likeadj, false);
}

mivi_status_t mivi_softmax_set_plane_cap(mivi_ctx_t *c, int64_t bytes) { return set_rows_cap(c, &mivi_ctx::sm_rows, bytes); }
