// libmivi C ABI, the block-diagonal Gaussian family (MIVI_BLOCKDIAG; MvLocationScale with a block-diagonal LowerTriangular scale, defined
// in include/mivi.h): creation, one RepGradELBO estimate as launches of kernels_blockdiag.hip, rand and logpdf.  The host layer reaches
// them through the family's row of kFamilies (api_common.h), which also says which groups of entries refuse the family.
#include "api_common.h"

mivi_status_t mivi_create_blockdiag(const mivi_config_t *cfg, const mivi_blockdiag_t *bd, mivi_ctx_t **out) {
  if (!cfg || !bd || !out) return MIVI_ERR_BAD_ARG;
  if (cfg->family != MIVI_BLOCKDIAG) return MIVI_ERR_BAD_ARG;
  if (bd->block < 1 || bd->block > MIVI_BLOCKDIAG_MAX_BLOCK) return MIVI_ERR_BAD_ARG;
  if (cfg->d < 1 || cfg->n_mc < 1) return MIVI_ERR_BAD_ARG;
  if ((int64_t)cfg->d * (int64_t)((cfg->n_mc + 63) / 64 * 64) > MIVI_BLOCKDIAG_MAX_PLANE) return MIVI_ERR_BAD_ARG;   // the d x n_mc planes
  if (cfg->m_offset != 0 || (cfg->m_total != 0 && cfg->m_total != cfg->n_mc)) return MIVI_ERR_UNSUPPORTED;   // no sharded estimates
  mivi_ctx_t *c = nullptr;
  const mivi_status_t s = create_context(cfg, nullptr, &c, bd->block);
  if (s) return s;
  if (!bd_prepare(c)) {
    (void)hipGetLastError();
    (void)mivi_destroy(c);
    return MIVI_ERR_HIP;
  }
  *out = c;
  return MIVI_OK;
}

int64_t params_len_blockdiag(const mivi_ctx *c) { return c->bd.plen; }

// the family's scratch (ensure_work): the value's partials, and the VJP's f64 partials where a launch takes slices of the sample axis
mivi_status_t ensure_work_blockdiag(mivi_ctx *c, int cap) {
  const int ns = bd_slices(c->bd, cap);
  mivi_status_t s;
  if ((s = ensure(c, c->bd_sc, bd_sc_bytes(c->bd), false)) || (ns > 1 && (s = ensure(c, c->bd_part, (size_t)ns * (size_t)c->bd.plen * sizeof(double), false))))
    return s;
  return MIVI_OK;
}

// One estimate over M samples (no allocation, no host synchronisation with a built-in target: capturable).
//   diagonal-Gaussian target, no bijector, a gradient wanted:  ONE kernel (draws, Z, target, VJP)  [-> finish]  -> value
//   otherwise:  forward (draws, Z) [-> bijector] -> target [-> bijector] [-> VJP on the redrawn tiles [-> finish]] -> value
mivi_status_t run_estimate_blockdiag(mivi_ctx *c, const void *params, const RngArgs &rng, int M, int want_grad, const OutArgs &out, ValueIn &vin) {
  if (want_grad && c->target == TGT_DIAG_GAUSS && !c->bij_on) {
    launch_bd_grad(c, params, rng, M, true, vin, out);
  } else {
    launch_bd_forward(c, params, rng, M, c->Z.p, nullptr, true);
    if (mivi_status_t s = target_behind_bijector(c, M, want_grad, c->cur, vin)) return s;
    if (want_grad) launch_bd_grad(c, params, rng, M, false, vin, out);
    else bd_wire_value(c, M, false, vin);
  }
  launch_value_only(c, params, vin, out);
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

// rand(rng, q, n_mc): Z (d x n_mc) and the base draws eps (d x n_mc)
mivi_status_t sample_blockdiag(mivi_ctx *c, const void *params, uint64_t idx, void *Z, void *eps) {
  launch_bd_forward(c, params, rng_of(c, idx), c->cfg.n_mc, Z, eps, false);
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

// logpdf(q, z) (logpdf_launches): the forward substitution C_k X_k = Z_k - mu_k per unit in LDS (k_bd_logpdf, kernels_blockdiag.hip), f64 X
// and sums; the unit chunks' f64 partials per column, then their sum
mivi_status_t logpdf_blockdiag(mivi_ctx *c, const void *params, const char *Z, int n, char *logq, char *std, const LogpdfBij *bij) {
  const size_t d = c->cfg.d, es = c->esize;
  const int cap = n < kSampleChunk ? n : kSampleChunk;
  if (mivi_status_t s = ensure(c, c->lp_work, (size_t)bd_logpdf_chunks(c->bd) * cap * sizeof(double), false)) return s;
  return logpdf_chunks(c, Z, n, logq, bij, [&](const SampleChunk &k, const char *z, char *lq) {
    launch_bd_logpdf(c, params, z, k.Mc, lq, std ? std + (size_t)k.off * d * es : nullptr, (double *)c->lp_work.p);
  });
}
