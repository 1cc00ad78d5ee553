// libmivi C ABI, the softmax (multinomial logistic) regression target (include/mivi.h): mivi_set_target_softmax, the row selection
// mivi_softmax_select_rows (AdvancedVI.subsample) and the residual plane's cap.  The target is a GENERIC one: eval_generic_target
// (api_estimate.hip) evaluates it on explicit samples through launch_sm_target (kernels_softmax.hip), so every route that serves a callback
// target by explicit samples serves it, on the device; the entries that cannot are guarded by refuse_softmax (api_common.h).
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
  c->sm_n = c->sm_nr = n;
  c->sm_sel = false;
  c->sm_C = n_classes;
  c->sm_variant = variant;
  c->sm_likeadj = c->sm_likeadj_full = likeadj;
  c->lr_sched_n = c->lr_sched_k = 0;   // (a logistic regression's schedule of batches goes with its target)
  c->t_const = 0.0;
  c->target = TGT_SOFTMAX;
  return MIVI_OK;
}

mivi_status_t mivi_softmax_select_rows(mivi_ctx_t *c, const int64_t *idx, int64_t b, double likeadj) {
  if (!c || b < 0 || (b > 0 && !idx)) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_bnn(c, "mivi_softmax_select_rows (its rows are selected by mivi_bnn_select_rows)")) return rs;
  if (mivi_status_t rs = refuse_hglm(c, "mivi_softmax_select_rows (its rows are selected by mivi_hglm_select_rows)")) return rs;
  if (mivi_status_t rs = refuse_ppca(c, "mivi_softmax_select_rows (its rows are selected by mivi_ppca_select_rows)")) return rs;
  if (c->target != TGT_SOFTMAX) return fail(c, MIVI_ERR_NO_TARGET, "no softmax regression target set");
  (void)hipSetDevice(c->cfg.device);
  if (b > 0) {   // (checked before anything changes: a failed call leaves the previous selection in force)
    if (!(likeadj > 0.0)) return fail(c, MIVI_ERR_BAD_ARG, "likelihood adjustment must be positive");
    for (int64_t j = 0; j < b; ++j)
      if (idx[j] < 0 || idx[j] >= c->sm_n) return fail(c, MIVI_ERR_BAD_ARG, "batch row index out of range");
  }
  invalidate_graph(c);
  if (b == 0) {   // back to the full data set
    c->sm_sel = false;
    c->sm_nr = c->sm_n;
    c->sm_likeadj = c->sm_likeadj_full;
    return MIVI_OK;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));   // the previous estimate may still be reading the index vector
  if (mivi_status_t s = upload(c, c->sm_idx, idx, (size_t)b * sizeof(int64_t))) {   // (a grown vector is a new one: the old selection is gone)
    c->sm_sel = false;
    c->sm_nr = c->sm_n;
    c->sm_likeadj = c->sm_likeadj_full;
    return s;
  }
  c->sm_sel = true;
  c->sm_nr = b;
  c->sm_likeadj = likeadj;
  return MIVI_OK;
}

mivi_status_t mivi_softmax_set_plane_cap(mivi_ctx_t *c, int64_t bytes) {
  if (!c || bytes < 0) return MIVI_ERR_BAD_ARG;
  invalidate_graph(c);   // (a recorded graph holds the chunks of the cap it was recorded under)
  c->sm_cap = (size_t)bytes;
  return MIVI_OK;
}
