// libmivi C ABI, parts 10 to 12: the measure-space algorithms on the device-resident [m; vec C] --
//   KLMinSqrtNaturalGradDescent (src/algorithms/klminsqrtnaturalgraddescent.jl): the square-root natural-gradient update (kernels_ngd.hip);
//   KLMinNaturalGradDescent (src/algorithms/klminnaturalgraddescent.jl): the state [S; Sigma] of `init` (:83-87) and the natural-gradient
//     update of `step` (:129-145) (kernels_natgrad.hip; its scale convention, a LOWER-triangular C' where the reference's new scale is upper
//     triangular, is stated there and in include/mivi.h);
//   FisherMinBatchMatch (src/algorithms/fisherminbatchmatch.jl): the state Sigma of `init` (:76), the per-sample objective (:81-111) and the
//     batch-and-match update of `step` (:143-155) (kernels_bam.hip; below, after the shared helpers);
//   KLMinWassFwdBwd (src/algorithms/klminwassfwdbwd.jl): the state Sigma of `init` (:75, batch and match's launch) and the proximal update of
//     `step` (:105-114) (kernels_wass.hip)
// -- and whole steps {estimator, update} without a host round trip.  A step is the existing estimator entry (mivi_gauss_expected_grad_hess /
// _hess2) into context-owned buffers followed by the update, whose last launch also forms elbo = logpi_avg + entropy(q') and the sticky
// flags: launches are fused, arithmetic is not, so the _steps entries are bitwise the single calls.  The algorithms differ in the update
// alone (Update); the guards, the step loop and the _host staging are written once.
#include "api_common.h"

#include <string>

namespace {

// the estimator outputs of the step loops and the inputs of the _host updates -- c->ngd_est, sized: [scalar (16 bytes: entropy or
// logpi_avg); grad (d); hess (d x d), 16-byte aligned behind grad]
struct NgdEst { char *scalar, *grad, *hess; };

mivi_status_t ngd_est(mivi_ctx *c, NgdEst *e) {
  const size_t es = c->esize, d = (size_t)c->cfg.d, goff = (d * es + 15) / 16 * 16;
  const mivi_status_t s = ensure(c, c->ngd_est, 16 + goff + d * d * es, false);
  if (s) return s;
  char *b = (char *)c->ngd_est.p;
  *e = NgdEst{b, b + 16, b + 16 + goff};
  return MIVI_OK;
}

// Which update.  The three work in the context's one scratch pair, which holds nothing between calls: each ensures it to its own need.
enum class Algorithm { SqrtNgd, NatGrad, Wass };

struct Update {
  Algorithm alg;
  void *state;         // SqrtNgd: none; NatGrad: [S; Sigma]; Wass: Sigma
  int ensure_posdef;   // NatGrad

  // the elements of `state`
  static size_t state_len(const mivi_ctx *c, Algorithm alg) {
    const size_t d = (size_t)c->cfg.d;
    switch (alg) {
      case Algorithm::NatGrad: return 2 * d * d;
      case Algorithm::Wass: return d * d;
      default: return 0;
    }
  }
  mivi_status_t scratch(mivi_ctx *c) const {
    size_t work = 0, part = 0;
    switch (alg) {
      case Algorithm::SqrtNgd: work = ngd_work_bytes(c), part = ngd_part_bytes(c); break;
      case Algorithm::NatGrad: work = natgrad_work_bytes(c), part = natgrad_part_bytes(c); break;
      case Algorithm::Wass: work = wass_work_bytes(c), part = wass_part_bytes(c); break;
    }
    if (!work) return MIVI_OK;   // (the one-workgroup kernels need none)
    const mivi_status_t s = ensure(c, c->ms_work, work, false);
    return s ? s : ensure(c, c->ms_part, part, false);
  }
  mivi_status_t operator()(mivi_ctx *c, void *params, const void *grad, const void *hess, double stepsize, const void *logpi, void *entropy,
                           void *elbo) const {
    const mivi_status_t s = scratch(c);
    if (s) return s;
    switch (alg) {
      case Algorithm::SqrtNgd: launch_ngd_update(c, params, grad, hess, stepsize, logpi, entropy, elbo); break;
      case Algorithm::NatGrad: launch_natgrad_update(c, params, state, grad, hess, stepsize, ensure_posdef, logpi, entropy, elbo); break;
      case Algorithm::Wass: launch_wass_update(c, params, state, grad, hess, stepsize, logpi, entropy, elbo); break;
    }
    HIPCHK(c, hipGetLastError());
    return MIVI_OK;
  }
};

}  // namespace

// who: the entry's name, for the _steps entries "<entry>: <algorithm>"
static mivi_status_t need_fullrank(mivi_ctx *c, const char *who) {
  if (c->cfg.family == MIVI_FULLRANK) return MIVI_OK;
  return fail(c, MIVI_ERR_UNSUPPORTED, (std::string(who) + " takes a triangular scale (full-rank family)").c_str());
}

// a step needs the whole estimate on this context, and a target to estimate on
static mivi_status_t need_whole_estimate(mivi_ctx *c, const char *entry) {
  if (c->cfg.m_offset != 0 || (c->cfg.m_total != 0 && c->cfg.m_total != c->cfg.n_mc))
    return fail(c, MIVI_ERR_UNSUPPORTED, (std::string(entry) + ": a sharded context is not supported (the update needs the whole estimate)").c_str());
  if (c->target == TGT_NONE) return fail(c, MIVI_ERR_NO_TARGET, "no target set");
  return MIVI_OK;
}

// count iterations {estimator (index idx0 + t) -> update}
static mivi_status_t run_steps(mivi_ctx *c, const char *entry, const char *algorithm, const Update &update, void *params, uint64_t idx0, int32_t count,
                               int32_t n_samples, int32_t second_order, double stepsize, void *elbo) {
  mivi_status_t s;
  if ((s = need_fullrank(c, (std::string(entry) + ": " + algorithm).c_str())) || (s = need_whole_estimate(c, entry))) return s;
  (void)hipSetDevice(c->cfg.device);
  NgdEst e;   // (its scalar: logpi_avg)
  // Everything that can fail for want of memory, before any launch.  (mivi_sqrt_ngd_steps used to ensure its scratch inside the first
  // iteration, after the estimator had launched: the one change in observable order, and only where an allocation fails.)
  if ((s = ngd_est(c, &e)) || (s = update.scratch(c))) return s;
  for (int32_t t = 0; t < count; ++t) {
    // (the estimator entries refuse what they cannot do -- no Hessian / a Stacked bijector for the second-order branch, d beyond the solve --
    // before they launch anything, so a refused call leaves parameters and state untouched)
    s = second_order ? mivi_gauss_expected_grad_hess2(c, params, idx0 + (uint64_t)t, n_samples, e.scalar, e.grad, e.hess)
                     : mivi_gauss_expected_grad_hess(c, params, idx0 + (uint64_t)t, n_samples, e.scalar, e.grad, e.hess);
    if (s) return s;
    if ((s = update(c, params, e.grad, e.hess, stepsize, e.scalar, nullptr, elbo ? (char *)elbo + (size_t)t * c->esize : nullptr))) return s;
  }
  return MIVI_OK;
}

// the _host form of an update: parameters, g and H (and the state of an update that carries one) staged into context-owned buffers, the
// update, the results back
static mivi_status_t update_host(mivi_ctx *c, const char *entry, Algorithm alg, void *params_h, void *state_h, const void *grad_h, const void *hess_h,
                                 double stepsize, int ensure_posdef, void *entropy_h) {
  mivi_status_t s;
  if ((s = need_fullrank(c, entry))) return s;
  (void)hipSetDevice(c->cfg.device);
  const size_t es = c->esize, d = (size_t)c->cfg.d, sb = Update::state_len(c, alg) * es;
  NgdEst e;   // (its scalar: the entropy)
  if ((s = ngd_est(c, &e)) || (state_h && (s = ensure(c, c->natgrad_host, sb, false))) || (s = stage_params(c, params_h))) return s;
  if (state_h) HIPCHK(c, hipMemcpyAsync(c->natgrad_host.p, state_h, sb, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(e.grad, grad_h, d * es, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(e.hess, hess_h, d * d * es, hipMemcpyHostToDevice, c->stream));
  const Update update{alg, state_h ? c->natgrad_host.p : nullptr, ensure_posdef};
  if ((s = update(c, c->tmp_params.p, e.grad, e.hess, stepsize, nullptr, e.scalar, nullptr))) return s;
  return fetch_results(c, {{params_h, c->tmp_params.p, (size_t)mivi_params_len(c) * es}, {state_h, c->natgrad_host.p, sb}, {entropy_h, e.scalar, es}}, true);
}

// ---- FisherMinBatchMatch (src/algorithms/fisherminbatchmatch.jl; kernels_bam.hip) ------------------------------------------------------------------
// What every batch-and-match entry refuses before anything launches.  n_samples < 0: the entry takes none; bounded: the update's rank bound.
static mivi_status_t need_bam(mivi_ctx *c, const char *entry, int32_t n_samples, bool bounded) {
  mivi_status_t s;
  if ((s = need_fullrank(c, (std::string(entry) + ": FisherMinBatchMatch").c_str())) || (s = need_whole_estimate(c, entry))) return s;
  if (c->bij_on)
    return fail(c, MIVI_ERR_UNSUPPORTED, (std::string(entry) + ": a Stacked bijector is set (FisherMinBatchMatch requires unconstrained support)").c_str());
  if (n_samples < 0) return MIVI_OK;
  if (n_samples < 2) return fail(c, MIVI_ERR_BAD_ARG, (std::string(entry) + ": n_samples < 2 (the corrected sample covariance is undefined)").c_str());
  if (bounded && n_samples > MIVI_BAM_MAX_SAMPLES)
    return fail(c, MIVI_ERR_UNSUPPORTED, (std::string(entry) + ": n_samples > MIVI_BAM_MAX_SAMPLES (the update's eigenproblem is one workgroup's)").c_str());
  return MIVI_OK;
}

static mivi_status_t bam_moments_too_many(mivi_ctx *c) {   // bam_moments is one chunk's work
  return fail(c, MIVI_ERR_UNSUPPORTED, ("bam_moments: more than " + std::to_string(kSampleChunk) + " samples (mivi_estimate_fisher takes any number)").c_str());
}

// the update's scratch and room for `tiles` objective partials in the same pair
static mivi_status_t bam_scratch(mivi_ctx *c, bool update, int tiles) {
  mivi_status_t s;
  if (update && (s = ensure(c, c->ms_work, bam_work_bytes(c), false))) return s;
  const size_t pb = update ? bam_part_bytes(c) : 0, tb = (size_t)tiles * sizeof(double);
  return ensure(c, c->ms_part, pb > tb ? pb : tb, false);
}

// One chunk of the objective's sampling stage: the Mc draws of `r` (an estimate's columns from r.m_offset on) in the context's eps plane (leading
// dimension dP), the gradients in c->W, [sum logpi, ..] in c->tmp_out -- the Stein estimator's call -- and the chunk's tile partials.
static mivi_status_t bam_chunk(mivi_ctx *c, const void *params, const RngArgs &r, int Mc, double *part) {
  const mivi_status_t s = run_estimate(c, params, r, Mc, 1, chunk_partials_out(c, c->tmp_out.p, Mc), nullptr, nullptr, true);
  if (s) return s;
  launch_bam_fisher(c, params, Mc, c->eps[c->cur].p, (size_t)c->dP, c->W.p, part);
  return MIVI_OK;
}

// rand_batch_match_samples_with_objective! for n <= one chunk; the scratch is the caller's to ensure.  u / G (nullable): compact copies.
static mivi_status_t bam_moments(mivi_ctx *c, const void *params, uint64_t idx, int32_t n, void *u, void *G, void *fisher, void *logpi, void *elbo) {
  mivi_status_t s;
  if ((s = bam_chunk(c, params, rng_of(c, idx), n, (double *)c->ms_part.p))) return s;
  launch_bam_objective(c, params, (const double *)c->ms_part.p, bam_fisher_tiles(c, n), (double)n, c->tmp_out.p, fisher, logpi, elbo);
  const size_t es = c->esize, d = (size_t)c->cfg.d;
  if (u) HIPCHK(c, hipMemcpy2DAsync(u, d * es, c->eps[c->cur].p, (size_t)c->dP * es, d * es, (size_t)n, hipMemcpyDeviceToDevice, c->stream));
  if (G) HIPCHK(c, hipMemcpyAsync(G, c->W.p, d * (size_t)n * es, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

static mivi_status_t bam_update(mivi_ctx *c, void *params, void *state, const void *u, size_t ldu, const void *G, int32_t n, double lambda, void *entropy) {
  launch_bam_update(c, params, state, u, ldu, G, n, lambda, entropy);
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

// the _host entries' device staging: [Sigma (d x d); u (d x n); G (d x n); three scalars of 16 bytes]
struct BamHost { char *state, *u, *G, *scalar; };
static mivi_status_t bam_host(mivi_ctx *c, int32_t n, BamHost *h) {
  const size_t es = c->esize, d = (size_t)c->cfg.d, nn = n > 0 ? (size_t)n : 0;
  const size_t sb = (d * d * es + 15) / 16 * 16, ub = (d * nn * es + 15) / 16 * 16;
  const mivi_status_t s = ensure(c, c->bam_host, sb + 2 * ub + 48, false);
  if (s) return s;
  char *b = (char *)c->bam_host.p;
  *h = BamHost{b, b + sb, b + sb + ub, b + sb + 2 * ub};
  return MIVI_OK;
}

extern "C" {

mivi_status_t mivi_bam_init(mivi_ctx_t *c, const void *params, void *state) {
  if (!c || !params || !state) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_bam_init")) return rs;
  const mivi_status_t s = need_bam(c, "bam_init", -1, false);
  if (s) return s;
  (void)hipSetDevice(c->cfg.device);
  launch_bam_init(c, params, state);
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

mivi_status_t mivi_bam_moments(mivi_ctx_t *c, const void *params, uint64_t idx, int32_t n_samples, void *u, void *G, void *fisher, void *logpi_avg,
                               void *elbo) {
  if (!c || !params || !u || !G || !fisher || !logpi_avg || !elbo) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_bam_moments")) return rs;
  mivi_status_t s;
  if ((s = need_bam(c, "bam_moments", n_samples, false))) return s;
  if (n_samples > kSampleChunk) return bam_moments_too_many(c);
  (void)hipSetDevice(c->cfg.device);
  if ((s = bam_scratch(c, false, bam_fisher_tiles(c, n_samples)))) return s;
  return bam_moments(c, params, idx, n_samples, u, G, fisher, logpi_avg, elbo);
}

mivi_status_t mivi_bam_moments_host(mivi_ctx_t *c, const void *params_h, uint64_t idx, int32_t n_samples, void *u_h, void *G_h, void *fisher_h,
                                    void *logpi_avg_h, void *elbo_h) {
  if (!c || !params_h || !u_h || !G_h || !fisher_h || !logpi_avg_h || !elbo_h) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_bam_moments_host")) return rs;
  mivi_status_t s;
  if ((s = need_bam(c, "bam_moments", n_samples, false))) return s;
  if (n_samples > kSampleChunk) return bam_moments_too_many(c);
  (void)hipSetDevice(c->cfg.device);
  BamHost h;
  if ((s = bam_host(c, n_samples, &h)) || (s = bam_scratch(c, false, bam_fisher_tiles(c, n_samples))) || (s = stage_params(c, params_h))) return s;
  if ((s = bam_moments(c, c->tmp_params.p, idx, n_samples, h.u, h.G, h.scalar, h.scalar + 16, h.scalar + 32))) return s;
  const size_t es = c->esize, ub = (size_t)c->cfg.d * (size_t)n_samples * es;
  return fetch_results(c, {{u_h, h.u, ub}, {G_h, h.G, ub}, {fisher_h, h.scalar, es}, {logpi_avg_h, h.scalar + 16, es}, {elbo_h, h.scalar + 32, es}}, true);
}

mivi_status_t mivi_estimate_fisher(mivi_ctx_t *c, const void *params, uint64_t idx, int32_t n_samples, void *value) {
  if (!c || !params || !value) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_estimate_fisher")) return rs;
  mivi_status_t s;
  if ((s = need_bam(c, "estimate_fisher", n_samples, false))) return s;
  (void)hipSetDevice(c->cfg.device);
  int tiles = 0;
  (void)for_each_chunk(c, idx, n_samples, 0, 1, [&](const SampleChunk &k) -> mivi_status_t { tiles += bam_fisher_tiles(c, k.Mc); return MIVI_OK; });
  if ((s = bam_scratch(c, false, tiles))) return s;
  double *part = (double *)c->ms_part.p;
  s = for_each_chunk(c, idx, n_samples, 0, 1, [&](const SampleChunk &k) -> mivi_status_t {
    const mivi_status_t se = bam_chunk(c, params, k.rng, k.Mc, part);
    part += bam_fisher_tiles(c, k.Mc);
    return se;
  });
  if (s) return s;
  launch_bam_objective(c, params, (const double *)c->ms_part.p, tiles, (double)n_samples, nullptr, value, nullptr, nullptr);
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

mivi_status_t mivi_estimate_fisher_host(mivi_ctx_t *c, const void *params_h, uint64_t idx, int32_t n_samples, void *value_h) {
  if (!c || !params_h || !value_h) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_estimate_fisher_host")) return rs;
  mivi_status_t s;
  if ((s = need_bam(c, "estimate_fisher", n_samples, false))) return s;
  (void)hipSetDevice(c->cfg.device);
  BamHost h;
  if ((s = bam_host(c, 0, &h)) || (s = stage_params(c, params_h))) return s;
  if ((s = mivi_estimate_fisher(c, c->tmp_params.p, idx, n_samples, h.scalar))) return s;
  return fetch_results(c, {{value_h, h.scalar, c->esize}}, false);   // (a non-finite value is returned as it is, like mivi_estimate_objective_host)
}

mivi_status_t mivi_bam_update(mivi_ctx_t *c, void *params, void *state, const void *u, const void *G, int32_t n_samples, double lambda, void *entropy) {
  if (!c || !params || !state || !u || !G || !(lambda > 0.0)) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_bam_update")) return rs;
  mivi_status_t s;
  if ((s = need_bam(c, "bam_update", n_samples, true))) return s;
  (void)hipSetDevice(c->cfg.device);
  if ((s = bam_scratch(c, true, 0))) return s;
  return bam_update(c, params, state, u, (size_t)c->cfg.d, G, n_samples, lambda, entropy);
}

mivi_status_t mivi_bam_update_host(mivi_ctx_t *c, void *params_h, void *state_h, const void *u_h, const void *G_h, int32_t n_samples, double lambda,
                                   void *entropy_h) {
  if (!c || !params_h || !state_h || !u_h || !G_h || !(lambda > 0.0)) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_bam_update_host")) return rs;
  mivi_status_t s;
  if ((s = need_bam(c, "bam_update", n_samples, true))) return s;
  (void)hipSetDevice(c->cfg.device);
  const size_t es = c->esize, d = (size_t)c->cfg.d, sb = d * d * es, ub = d * (size_t)n_samples * es;
  BamHost h;
  if ((s = bam_host(c, n_samples, &h)) || (s = bam_scratch(c, true, 0)) || (s = stage_params(c, params_h))) return s;
  HIPCHK(c, hipMemcpyAsync(h.state, state_h, sb, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(h.u, u_h, ub, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(h.G, G_h, ub, hipMemcpyHostToDevice, c->stream));
  if ((s = bam_update(c, c->tmp_params.p, h.state, h.u, d, h.G, n_samples, lambda, h.scalar))) return s;
  return fetch_results(c, {{params_h, c->tmp_params.p, (size_t)mivi_params_len(c) * es}, {state_h, h.state, sb}, {entropy_h, h.scalar, es}}, true);
}

mivi_status_t mivi_bam_steps(mivi_ctx_t *c, void *params, void *state, uint64_t idx0, uint64_t iteration0, int32_t count, int32_t n_samples, void *fisher,
                             void *elbo) {
  if (!c || !params || !state || count < 0 || iteration0 < 1) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_bam_steps")) return rs;
  mivi_status_t s;
  if ((s = need_bam(c, "bam_steps", n_samples, true))) return s;
  (void)hipSetDevice(c->cfg.device);
  NgdEst e;   // (its scalar: logpi_avg)
  if ((s = ngd_est(c, &e)) || (s = bam_scratch(c, true, bam_fisher_tiles(c, n_samples)))) return s;
  const size_t es = c->esize;
  for (int32_t t = 0; t < count; ++t) {
    // step t: the objective at q_t (its draws and gradients stay where the sampling stage left them), then the update reads them there
    if ((s = bam_moments(c, params, idx0 + (uint64_t)t, n_samples, nullptr, nullptr, fisher ? (char *)fisher + (size_t)t * es : nullptr, e.scalar,
                         elbo ? (char *)elbo + (size_t)t * es : nullptr)))
      return s;
    double lambda = (double)c->cfg.d * (double)n_samples / (double)(iteration0 + (uint64_t)t);
    lambda = by_dtype(c, [&](auto t) { return (double)(decltype(t))lambda; });   // convert(eltype(mu), d * n_samples / iteration) (:148)
    if ((s = bam_update(c, params, state, c->eps[c->cur].p, (size_t)c->dP, c->W.p, n_samples, lambda, nullptr))) return s;
  }
  return MIVI_OK;
}

mivi_status_t mivi_sqrt_ngd_update(mivi_ctx_t *c, void *params, const void *grad, const void *hess, double stepsize, void *entropy) {
  if (!c || !params || !grad || !hess) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_sqrt_ngd_update")) return rs;
  const mivi_status_t s = need_fullrank(c, "sqrt_ngd_update");
  if (s) return s;
  (void)hipSetDevice(c->cfg.device);
  return Update{Algorithm::SqrtNgd, nullptr, 0}(c, params, grad, hess, stepsize, nullptr, entropy, nullptr);
}

mivi_status_t mivi_sqrt_ngd_update_host(mivi_ctx_t *c, void *params_h, const void *grad_h, const void *hess_h, double stepsize, void *entropy_h) {
  if (!c || !params_h || !grad_h || !hess_h) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_sqrt_ngd_update_host")) return rs;
  return update_host(c, "sqrt_ngd_update", Algorithm::SqrtNgd, params_h, nullptr, grad_h, hess_h, stepsize, 0, entropy_h);
}

mivi_status_t mivi_sqrt_ngd_steps(mivi_ctx_t *c, void *params, uint64_t idx0, int32_t count, int32_t n_samples, int32_t second_order,
                                  double stepsize, void *elbo) {
  if (!c || !params || count < 0) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_sqrt_ngd_steps")) return rs;
  return run_steps(c, "sqrt_ngd_steps", "KLMinSqrtNaturalGradDescent", Update{Algorithm::SqrtNgd, nullptr, 0}, params, idx0, count, n_samples, second_order, stepsize, elbo);
}

mivi_status_t mivi_natgrad_init(mivi_ctx_t *c, const void *params, void *state) {
  if (!c || !params || !state) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_natgrad_init")) return rs;
  mivi_status_t s;
  if ((s = need_fullrank(c, "natgrad_init"))) return s;
  (void)hipSetDevice(c->cfg.device);
  if ((s = Update{Algorithm::NatGrad, state, 0}.scratch(c))) return s;
  launch_natgrad_init(c, const_cast<void *>(params), state);
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

mivi_status_t mivi_natgrad_update(mivi_ctx_t *c, void *params, void *state, const void *grad, const void *hess, double stepsize,
                                  int32_t ensure_posdef, void *entropy) {
  if (!c || !params || !state || !grad || !hess) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_natgrad_update")) return rs;
  const mivi_status_t s = need_fullrank(c, "natgrad_update");
  if (s) return s;
  (void)hipSetDevice(c->cfg.device);
  return Update{Algorithm::NatGrad, state, ensure_posdef}(c, params, grad, hess, stepsize, nullptr, entropy, nullptr);
}

mivi_status_t mivi_natgrad_update_host(mivi_ctx_t *c, void *params_h, void *state_h, const void *grad_h, const void *hess_h, double stepsize,
                                       int32_t ensure_posdef, void *entropy_h) {
  if (!c || !params_h || !state_h || !grad_h || !hess_h) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_natgrad_update_host")) return rs;
  return update_host(c, "natgrad_update", Algorithm::NatGrad, params_h, state_h, grad_h, hess_h, stepsize, ensure_posdef, entropy_h);
}

mivi_status_t mivi_natgrad_steps(mivi_ctx_t *c, void *params, void *state, uint64_t idx0, int32_t count, int32_t n_samples, int32_t second_order,
                                 double stepsize, int32_t ensure_posdef, void *elbo) {
  if (!c || !params || !state || count < 0) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_natgrad_steps")) return rs;
  return run_steps(c, "natgrad_steps", "KLMinNaturalGradDescent", Update{Algorithm::NatGrad, state, ensure_posdef}, params, idx0, count, n_samples, second_order, stepsize,
                   elbo);
}

mivi_status_t mivi_wass_init(mivi_ctx_t *c, const void *params, void *state) {
  if (!c || !params || !state) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_wass_init")) return rs;
  const mivi_status_t s = need_fullrank(c, "wass_init");
  if (s) return s;
  (void)hipSetDevice(c->cfg.device);
  launch_bam_init(c, params, state);   // Sigma = C C': the state of FisherMinBatchMatch's `init`
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

mivi_status_t mivi_wass_update(mivi_ctx_t *c, void *params, void *state, const void *grad, const void *hess, double stepsize, void *entropy) {
  if (!c || !params || !state || !grad || !hess) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_wass_update")) return rs;
  const mivi_status_t s = need_fullrank(c, "wass_update");
  if (s) return s;
  (void)hipSetDevice(c->cfg.device);
  return Update{Algorithm::Wass, state, 0}(c, params, grad, hess, stepsize, nullptr, entropy, nullptr);
}

mivi_status_t mivi_wass_update_host(mivi_ctx_t *c, void *params_h, void *state_h, const void *grad_h, const void *hess_h, double stepsize,
                                    void *entropy_h) {
  if (!c || !params_h || !state_h || !grad_h || !hess_h) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_wass_update_host")) return rs;
  return update_host(c, "wass_update", Algorithm::Wass, params_h, state_h, grad_h, hess_h, stepsize, 0, entropy_h);
}

mivi_status_t mivi_wass_steps(mivi_ctx_t *c, void *params, void *state, uint64_t idx0, int32_t count, int32_t n_samples, int32_t second_order,
                              double stepsize, void *elbo) {
  if (!c || !params || !state || count < 0) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_wass_steps")) return rs;
  return run_steps(c, "wass_steps", "KLMinWassFwdBwd", Update{Algorithm::Wass, state, 0}, params, idx0, count, n_samples, second_order, stepsize, elbo);
}

}  // extern "C"
