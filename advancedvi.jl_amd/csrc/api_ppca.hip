// libmivi C ABI, the probabilistic PCA / Bayesian factor model target (include/mivi.h): mivi_set_target_ppca, the row selection
// mivi_ppca_select_rows (AdvancedVI.subsample) and the partial planes' cap.  The target is a GENERIC one: eval_generic_target
// (api_estimate.hip) evaluates it on explicit samples through launch_ppca_target (kernels_ppca.hip); the target is a row of kTargets
// (api_common.h), whose refuse_target guards the entries that cannot serve it.
#include <cmath>

#include "api_common.h"

static bool ppca_positive(double v) { return std::isfinite(v) && v > 0.0; }

mivi_status_t mivi_set_target_ppca(mivi_ctx_t *c, const mivi_ppca_t *mp, const void *Y, const uint8_t *mask, int64_t n, int32_t D, int32_t on_device) {
  if (!c || !mp || !Y) return MIVI_ERR_BAD_ARG;
  const mivi_ppca_t m = *mp;
  if (n < 1) return fail(c, MIVI_ERR_BAD_ARG, "probabilistic PCA: n must be at least 1");
  if (D < 1 || D > MIVI_PPCA_MAX_D) return fail(c, MIVI_ERR_BAD_ARG, "probabilistic PCA: D must lie in [1, 512]");
  if (m.k < 1 || m.k > MIVI_PPCA_MAX_K) return fail(c, MIVI_ERR_BAD_ARG, "probabilistic PCA: k must lie in [1, 32]");
  const long long d = (long long)D * m.k + (long long)n * m.k + D + (m.ard ? m.k : 0) + 1;
  if (c->cfg.d != d)
    return fail(c, MIVI_ERR_BAD_ARG, ("probabilistic PCA: the context's d must be D k + n k + D + (k with ARD) + 1, " + std::to_string(d)).c_str());
  if (!ppca_positive(m.prior_std)) return fail(c, MIVI_ERR_BAD_ARG, "probabilistic PCA: prior_std must be positive and finite");
  if (!ppca_positive(m.mean_std)) return fail(c, MIVI_ERR_BAD_ARG, "probabilistic PCA: mean_std must be positive and finite");
  if (!ppca_positive(m.noise_scale)) return fail(c, MIVI_ERR_BAD_ARG, "probabilistic PCA: noise_scale must be positive and finite");
  if (!ppca_positive(m.likeadj)) return fail(c, MIVI_ERR_BAD_ARG, "probabilistic PCA: likelihood adjustment must be positive and finite");
  const size_t ne = (size_t)n * D;
  if (!on_device)
    for (size_t i = 0; i < ne; ++i) {
      if (mask && mask[i] > 1) return fail(c, MIVI_ERR_BAD_ARG, "probabilistic PCA: a mask entry is not 0 or 1");
      if (mask && !mask[i]) continue;
      if (!std::isfinite(c->cfg.dtype == MIVI_F32 ? (double)((const float *)Y)[i] : ((const double *)Y)[i]))
        return fail(c, MIVI_ERR_BAD_ARG, "probabilistic PCA: an observed y is not finite");
    }
  (void)hipSetDevice(c->cfg.device);
  invalidate_graph(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));   // an estimate in flight may still read the previous data set
  if (on_device) {
    c->pp_Y = Y;
    c->pp_mask = mask;
  } else {
    if (c->target == TGT_PPCA) c->target = TGT_NONE;   // its buffers are rewritten below: a HIP failure on the way leaves NO target, not a mixed one
    mivi_status_t s;
    if ((s = upload(c, c->pp_Y_own, Y, ne * c->esize)) || (mask && (s = upload(c, c->pp_mask_own, mask, ne)))) return s;
    c->pp_Y = c->pp_Y_own.p;
    c->pp_mask = mask ? c->pp_mask_own.p : nullptr;
  }
  c->pp = m;
  c->pp_D = D;
  c->pp_rows.set_full(n, m.likeadj);
  c->lr_sched_n = c->lr_sched_k = 0;   // (a logistic regression's schedule of batches goes with its target)
  c->t_const = 0.0;
  c->target = TGT_PPCA;
  return MIVI_OK;
}

mivi_status_t mivi_ppca_select_rows(mivi_ctx_t *c, const int64_t *idx, int64_t b, double likeadj) {
  if (!c || b < 0 || (b > 0 && !idx)) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_rows_of_other_target(c, "mivi_ppca_select_rows", TGT_PPCA)) return rs;
  if (c->target != TGT_PPCA) return fail(c, MIVI_ERR_NO_TARGET, "no probabilistic PCA target set");
  (void)hipSetDevice(c->cfg.device);
  if (b > 0 && !ppca_positive(likeadj)) return fail(c, MIVI_ERR_BAD_ARG, "likelihood adjustment must be positive and finite");
  return select_rows(c, c->pp_rows, idx, b, likeadj, true);   // (every row owns its latent z_r: no repeats)
}

mivi_status_t mivi_ppca_set_part_cap(mivi_ctx_t *c, int64_t bytes) { return set_rows_cap(c, &mivi_ctx::pp_rows, bytes); }
