// libmivi C ABI: Distributions.logpdf(q, z) at points the CALLER supplies (src/families/location_scale.jl:59-63,
// src/families/location_scale_low_rank.jl:45-68) -- what importance weights, a PSIS diagnostic or held-out scores need of a fitted q.
// The estimators only ever form log q at their own draws, where u = C^-1 (z - mu) is known; here it has to be solved for:
//   mean-field : u = (z - mu) / sigma, one streaming kernel
//   full-rank  : the forward block substitution C X = Z - mu (k_lp_fwd16, kernels_logpdf.hip) on the inverted diagonal blocks of k_stl_prep
//   low-rank   : t = D^-1 (z - m), then the estimators' own parameter preparation and Woodbury stage (kernels_lowrank.hip) on t
// The call works in scratch of its own (mivi_ctx::lp_*), launches on the context's stream and touches neither the estimate buffers, the
// eps speculation, the buffer parity nor a cached graph: estimates around it are bitwise what they are without it.
#include "api_common.h"

// the points of chunk k: the caller's, or -- mivi_logpdf_constrained -- eta = b(x) of the caller's constrained points, left in the hook's scratch
static const char *chunk_points(mivi_ctx *c, const SampleChunk &k, const char *Z, const LogpdfBij *bij) {
  const size_t off = (size_t)k.off * c->cfg.d * c->esize;
  if (!bij) return Z + off;
  launch_bijx_inverse(c, k.Mc, bij->X + off, bij->eta, bij->ladj, bij->flag);
  return bij->eta;
}
// ... and what follows its density: logq <- logq - ladj, or -inf / NaN by the column's flag
static void chunk_finish(mivi_ctx *c, const SampleChunk &k, char *logq, const LogpdfBij *bij) {
  if (bij) launch_bijx_finish(c, k.Mc, logq + (size_t)k.off * c->esize, bij->ladj, bij->flag);
}

// the launches of one call: the parameter-only stage once, then the columns kSampleChunk at a time
mivi_status_t logpdf_launches(mivi_ctx *c, const void *params, const char *Z, int n, char *logq, char *std, const LogpdfBij *bij) {
  const size_t d = c->cfg.d, es = c->esize;
  const int cap = n < kSampleChunk ? n : kSampleChunk;
  mivi_status_t s;
  if (is_flow(c))   // eps = T^-1(z) through the inverse layers, log q beside it: no parameter-only stage, no scratch
    return for_each_chunk(c, 0, n, 0, 1, [&](const SampleChunk &k) -> mivi_status_t {
      launch_flow_inverse(c, params, chunk_points(c, k, Z, bij), k.Mc, logq + (size_t)k.off * es);
      chunk_finish(c, k, logq, bij);
      return MIVI_OK;
    });
  if (c->cfg.family == MIVI_LOWRANK) {
    const size_t r = c->cfg.rank, t_bytes = (d * cap * es + 15) / 16 * 16;
    if ((s = ensure(c, c->lp_scal, lowr_prep_doubles((int)d, (int)r) * sizeof(double), false)) ||
        (s = ensure(c, c->lp_work, t_bytes + (2 * r + 2) * cap * sizeof(double), false)))
      return s;
    const LowrPoints pts{c->lp_work.p, (double *)c->lp_scal.p, (double *)((char *)c->lp_work.p + t_bytes), (size_t)cap};
    launch_lowr_draw_prep(c, rng_of(c, 0), 0, params, pts.prep);   // the parameter half alone: A^-1, sum log D, 1/2 logdet A, the scale flag
    return for_each_chunk(c, 0, n, 0, 1, [&](const SampleChunk &k) -> mivi_status_t {
      launch_lp_lowr_t(c, params, chunk_points(c, k, Z, bij), k.Mc, pts.t);
      launch_lowr_woodbury(c, params, k.Mc, false, &pts);
      launch_lp_store(c, k.Mc, lowr_logq_of(c, pts), logq + (size_t)k.off * es);
      chunk_finish(c, k, logq, bij);
      return MIVI_OK;
    });
  }
  if ((s = ensure(c, c->lp_scal, 64, false))) return s;
  double *scal = (double *)c->lp_scal.p;
  if (c->cfg.family == MIVI_MEANFIELD) {
    launch_lp_logdet(c, params, scal);
    return for_each_chunk(c, 0, n, 0, 1, [&](const SampleChunk &k) -> mivi_status_t {
      launch_lp_mf(c, params, chunk_points(c, k, Z, bij), k.Mc, logq + (size_t)k.off * es, std ? std + (size_t)k.off * d * es : nullptr, scal);
      chunk_finish(c, k, logq, bij);
      return MIVI_OK;
    });
  }
  // full-rank: X of a chunk stays in LDS (f64) while 16 columns of it fit; past that it lives in an f64 scratch of a chunk's shape
  const bool need_xg = !lp_fwd_x_in_lds(c);
  if ((s = ensure(c, c->lp_dinv, (d + 31) / 32 * 1024 * es, false)) || (need_xg && (s = ensure(c, c->lp_work, d * cap * sizeof(double), false)))) return s;
  launch_stl_dinv32(c, params, c->lp_dinv.p);
  launch_lp_logdet(c, params, scal);
  return for_each_chunk(c, 0, n, 0, 1, [&](const SampleChunk &k) -> mivi_status_t {
    launch_lp_fwd(c, params, chunk_points(c, k, Z, bij), k.Mc, c->lp_dinv.p, logq + (size_t)k.off * es, std ? std + (size_t)k.off * d * es : nullptr,
                  need_xg ? (double *)c->lp_work.p : nullptr, scal);
    chunk_finish(c, k, logq, bij);
    return MIVI_OK;
  });
}

mivi_status_t mivi_logpdf(mivi_ctx_t *c, const void *params, const void *Z, int64_t n, void *logq, void *std) {
  if (!c) return MIVI_ERR_BAD_ARG;
  if (!params || !Z || !logq) return fail(c, MIVI_ERR_BAD_ARG, "mivi_logpdf: params, Z and logq must not be NULL");
  if (n < 1 || n > (int64_t)0x7fffffff - kSampleChunk) return fail(c, MIVI_ERR_BAD_ARG, "mivi_logpdf: n must be in [1, 2^31 - 16385]");
  if (std)
    if (mivi_status_t rs = refuse_lowrank(c, "mivi_logpdf with std_dev (the family has no square scale to standardise by)")) return rs;
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
    if (mivi_status_t rs = refuse_lowrank(c, "mivi_logpdf_host with std_host (the family has no square scale to standardise by)")) return rs;
  (void)hipSetDevice(c->cfg.device);
  const size_t es = c->esize, zb = (size_t)c->cfg.d * (size_t)n * es, qb = ((size_t)n * es + 15) / 16 * 16;
  mivi_status_t s = ensure(c, c->lp_host, zb + qb + (std_h ? zb : 0), false);
  if (s || (s = stage_params(c, params_h))) return s;
  char *Zd = (char *)c->lp_host.p, *qd = Zd + zb, *sd = std_h ? qd + qb : nullptr;
  HIPCHK(c, hipMemcpyAsync(Zd, Z_h, zb, hipMemcpyHostToDevice, c->stream));
  if ((s = mivi_logpdf(c, c->tmp_params.p, Zd, n, qd, sd))) return s;
  return fetch_results(c, {{logq_h, qd, (size_t)n * es}, {std_h, sd, zb}}, true);
}
