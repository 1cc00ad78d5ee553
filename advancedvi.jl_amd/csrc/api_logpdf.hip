// libmivi C ABI: Distributions.logpdf(q, z) at points the CALLER supplies (src/families/location_scale.jl:59-63,
// src/families/location_scale_low_rank.jl:45-68) -- what importance weights, a PSIS diagnostic or held-out scores need of a fitted q.
// The estimators only ever form log q at their own draws, where u = C^-1 (z - mu) is known; here it has to be solved for:
//   mean-field : u = (z - mu) / sigma, one streaming kernel
//   full-rank  : the forward block substitution C X = Z - mu (k_lp_fwd16, kernels_logpdf.hip) on the inverted diagonal blocks of k_stl_prep
//   block-diag : the forward substitution C_k X_k = Z_k - mu_k per unit in LDS (logpdf_blockdiag, api_blockdiag.hip)
//   low-rank   : t = D^-1 (z - m), then the estimators' own parameter preparation and Woodbury stage on t (logpdf_lowrank, api_lowrank.hip)
//   flows      : eps = T^-1(z) through the inverse layers, log q beside it (logpdf_flow, api_flow.hip)
// The call works in scratch of its own (mivi_ctx::lp_*), launches on the context's stream and touches neither the estimate buffers, the
// eps speculation, the buffer parity nor a cached graph: estimates around it are bitwise what they are without it.
#include "api_common.h"

// the launches of one call: the parameter-only stage once, then the columns kSampleChunk at a time (logpdf_chunks, api_common.h); a family
// of kFamilies has them in its own unit
mivi_status_t logpdf_launches(mivi_ctx *c, const void *params, const char *Z, int n, char *logq, char *std, const LogpdfBij *bij) {
  if (const FamilyRow *row = family_row(c)) return row->logpdf(c, params, Z, n, logq, std, bij);
  const size_t d = c->cfg.d, es = c->esize;
  const int cap = n < kSampleChunk ? n : kSampleChunk;
  mivi_status_t s;
  if ((s = ensure(c, c->lp_scal, 64, false))) return s;
  double *scal = (double *)c->lp_scal.p;
  if (c->cfg.family == MIVI_MEANFIELD) {
    launch_lp_logdet(c, params, scal);
    return logpdf_chunks(c, Z, n, logq, bij, [&](const SampleChunk &k, const char *pts, char *lq) {
      launch_lp_mf(c, params, pts, k.Mc, lq, std ? std + (size_t)k.off * d * es : nullptr, scal);
    });
  }
  // full-rank: X of a chunk stays in LDS (f64) while 16 columns of it fit; past that it lives in an f64 scratch of a chunk's shape
  const bool need_xg = !lp_fwd_x_in_lds(c);
  if ((s = ensure(c, c->lp_dinv, (d + 31) / 32 * 1024 * es, false)) || (need_xg && (s = ensure(c, c->lp_work, d * cap * sizeof(double), false)))) return s;
  launch_stl_dinv32(c, params, c->lp_dinv.p);
  launch_lp_logdet(c, params, scal);
  return logpdf_chunks(c, Z, n, logq, bij, [&](const SampleChunk &k, const char *pts, char *lq) {
    launch_lp_fwd(c, params, pts, k.Mc, c->lp_dinv.p, lq, std ? std + (size_t)k.off * d * es : nullptr, need_xg ? (double *)c->lp_work.p : nullptr, scal);
  });
}

mivi_status_t mivi_logpdf(mivi_ctx_t *c, const void *params, const void *Z, int64_t n, void *logq, void *std) {
  if (!c) return MIVI_ERR_BAD_ARG;
  if (!params || !Z || !logq) return fail(c, MIVI_ERR_BAD_ARG, "mivi_logpdf: params, Z and logq must not be NULL");
  if (n < 1 || n > (int64_t)0x7fffffff - kSampleChunk) return fail(c, MIVI_ERR_BAD_ARG, "mivi_logpdf: n must be in [1, 2^31 - 16385]");
  if (std)
    if (mivi_status_t rs = refuse(c, LACKS_STD, "mivi_logpdf with std_dev (the family has no square scale to standardise by)")) return rs;
  (void)hipSetDevice(c->cfg.device);
  if (mivi_status_t s = logpdf_launches(c, params, (const char *)Z, (int)n, (char *)logq, (char *)std, nullptr)) return s;
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

mivi_status_t mivi_logpdf_host(mivi_ctx_t *c, const void *params_h, const void *Z_h, int64_t n, void *logq_h, void *std_h) {
  if (!c) return MIVI_ERR_BAD_ARG;
  if (!params_h || !Z_h || !logq_h) return fail(c, MIVI_ERR_BAD_ARG, "mivi_logpdf_host: params, Z and logq must not be NULL");
  if (n < 1 || n > (int64_t)0x7fffffff - kSampleChunk) return fail(c, MIVI_ERR_BAD_ARG, "mivi_logpdf_host: n must be in [1, 2^31 - 16385]");
  if (std_h)
    if (mivi_status_t rs = refuse(c, LACKS_STD, "mivi_logpdf_host with std_host (the family has no square scale to standardise by)")) return rs;
  (void)hipSetDevice(c->cfg.device);
  const size_t es = c->esize, zb = (size_t)c->cfg.d * (size_t)n * es, qb = ((size_t)n * es + 15) / 16 * 16;
  mivi_status_t s = ensure(c, c->lp_host, zb + qb + (std_h ? zb : 0), false);
  if (s || (s = stage_params(c, params_h))) return s;
  char *Zd = (char *)c->lp_host.p, *qd = Zd + zb, *sd = std_h ? qd + qb : nullptr;
  HIPCHK(c, hipMemcpyAsync(Zd, Z_h, zb, hipMemcpyHostToDevice, c->stream));
  if ((s = mivi_logpdf(c, c->tmp_params.p, Zd, n, qd, sd))) return s;
  return fetch_results(c, {{logq_h, qd, (size_t)n * es}, {std_h, sd, zb}}, true);
}
