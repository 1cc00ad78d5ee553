// libmivi C ABI, the low-rank Gaussian family (MIVI_LOWRANK; src/families/location_scale_low_rank.jl): one RepGradELBO estimate as a
// sequence of launches of kernels_lowrank.hip, rand and logpdf.  The host layer reaches them through the family's row of kFamilies
// (api_common.h), which also says which groups of entries refuse the family.
#include "api_common.h"

mivi_status_t lowrank_check_config(const mivi_config_t *cfg) {
  if (cfg->family != MIVI_LOWRANK) return MIVI_OK;   // (rank is read for this family only)
  if (cfg->rank < 1 || cfg->rank > MIVI_LOWRANK_MAX_RANK) return MIVI_ERR_BAD_ARG;
  if (cfg->m_offset != 0 || (cfg->m_total != 0 && cfg->m_total != cfg->n_mc)) return MIVI_ERR_UNSUPPORTED;   // no sharded low-rank estimates
  return MIVI_OK;
}

int64_t params_len_lowrank(const mivi_ctx *c) { return 2 * (int64_t)c->cfg.d + (int64_t)c->cfg.d * (int64_t)c->cfg.rank; }

// the family's scratch for cap samples per launch (ensure_work): the draws, V = Sigma^-1 (z - m), the prep block, f64 [s; x; |t|^2; log q]
mivi_status_t ensure_work_lowrank(mivi_ctx *c, int cap) {
  const size_t d = c->cfg.d, r = c->cfg.rank, es = c->esize;
  mivi_status_t s;
  if ((s = ensure(c, c->lowr_E, (d + r) * cap * es, false)) || (s = ensure(c, c->lowr_V, d * cap * es, false)) ||
      (s = ensure(c, c->lowr_prep, lowr_prep_doubles((int)d, (int)r) * sizeof(double), false)) ||
      (s = ensure(c, c->lowr_sx, (2 * r + 2) * cap * sizeof(double), false)) ||
      (s = ensure(c, c->lowr_part, 8 * (2 * d + d * r) * sizeof(double), false)))
    return s;
  return MIVI_OK;
}

// One estimate over M samples (no allocation, no host synchronisation with a built-in target: capturable):
//   [gram ->] draws + prep -> sample [-> bijector] -> target [-> bijector] [-> Woodbury: s; x, log q, V] [-> VJP partials] -> finish (gradient, value)
mivi_status_t run_estimate_lowrank(mivi_ctx *c, const void *params, const RngArgs &rng, int M, int want_grad, const OutArgs &out, ValueIn &vin) {
  const int ek = out.ent_kind;
  const bool closed = ek == MIVI_ENT_CLOSED_FORM || ek == MIVI_ENT_CLOSED_FORM_ZERO_GRAD;
  launch_lowr_draw_prep(c, rng, M, params);
  launch_lowr_sample(c, params, M, c->Z.p, !closed);
  if (mivi_status_t s = target_behind_bijector(c, M, want_grad, c->cur, vin)) return s;
  if (!closed) launch_lowr_woodbury(c, params, M, want_grad != 0);
  launch_lowr_vjp_finish(c, params, M, want_grad, vin, out);
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

// rand(rng, q, n_mc) (location_scale_low_rank.jl:66-100): Z (d x n_mc) and the draws (u1; u2) as eps ((d + r) x n_mc)
mivi_status_t sample_lowrank(mivi_ctx *c, const void *params, uint64_t idx, void *Z, void *eps) {
  const int M = c->cfg.n_mc;
  launch_lowr_draw_prep(c, rng_of(c, idx), M, nullptr);
  launch_lowr_sample(c, params, M, Z, false);
  if (eps)
    HIPCHK(c, hipMemcpyAsync(eps, c->lowr_E.p, (size_t)(c->cfg.d + c->cfg.rank) * M * c->esize, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

// logpdf(q, z) (logpdf_launches): t = D^-1 (z - m), then the estimators' own parameter preparation and Woodbury stage on t
mivi_status_t logpdf_lowrank(mivi_ctx *c, const void *params, const char *Z, int n, char *logq, char *, const LogpdfBij *bij) {
  const size_t d = c->cfg.d, es = c->esize;
  const int cap = n < kSampleChunk ? n : kSampleChunk;
  const size_t r = c->cfg.rank, t_bytes = (d * cap * es + 15) / 16 * 16;
  mivi_status_t s;
  if ((s = ensure(c, c->lp_scal, lowr_prep_doubles((int)d, (int)r) * sizeof(double), false)) ||
      (s = ensure(c, c->lp_work, t_bytes + (2 * r + 2) * cap * sizeof(double), false)))
    return s;
  const LowrPoints pts{c->lp_work.p, (double *)c->lp_scal.p, (double *)((char *)c->lp_work.p + t_bytes), (size_t)cap};
  launch_lowr_draw_prep(c, rng_of(c, 0), 0, params, pts.prep);   // the parameter half alone: A^-1, sum log D, 1/2 logdet A, the scale flag
  return logpdf_chunks(c, Z, n, logq, bij, [&](const SampleChunk &k, const char *z, char *lq) {
    launch_lp_lowr_t(c, params, z, k.Mc, pts.t);
    launch_lowr_woodbury(c, params, k.Mc, false, &pts);
    launch_lp_store(c, k.Mc, lowr_logq_of(c, pts), lq);
  });
}
