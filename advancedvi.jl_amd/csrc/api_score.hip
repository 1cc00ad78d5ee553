// libmivi C ABI, part 9: the score-gradient ELBO estimator (ScoreGradELBO, src/algorithms/scoregradelbo.jl; driven by
// KLMinScoreGradDescent = BBVI, src/algorithms/constructors.jl:199-233).  It needs only the VALUES log pi(z_m), so it is the estimator
// for targets without a gradient (mivi_set_target_value_callback).  A driver of its own beside run_estimate: explicit samples ->
// per-sample target values -> f64 statistics and centred weights (kernels_score.hip) -> gradient.
//   full rank : k_eps, sample (Z), [bijector], target values, k_sg_norms, k_sg_stats, k_sg_scale, the sticking-the-landing solve with
//               rhs = -E diag(f - fbar), the first-generation VJP with no direct entropy term
//   mean field: k_mf_sample (Z), [bijector], target values, k_sg_norms, k_sg_stats, k_sg_mf_grad  (eps is redrawn from Philox)
#include "api_common.h"

mivi_status_t mivi_set_target_value_callback(mivi_ctx_t *c, mivi_logdensity_fn fv, void *user) {
  if (!c || !fv) return MIVI_ERR_BAD_ARG;
  c->cb_grad = nullptr;
  c->cb_value = fv;
  c->cb_user = user;
  c->t_const = 0.0;
  c->target = TGT_CALLBACK;
  invalidate_graph(c);
  return MIVI_OK;
}

static mivi_status_t run_score_estimate(mivi_ctx *c, const void *params, uint64_t idx, void *value, void *elbo, void *grad) {
  if (c->target == TGT_NONE) return fail(c, MIVI_ERR_NO_TARGET, "no target set");
  if (c->cfg.m_offset != 0 || (c->cfg.m_total != 0 && c->cfg.m_total != c->cfg.n_mc))
    return fail(c, MIVI_ERR_UNSUPPORTED, "score gradient: a sharded context is not supported (the centring f - mean(f) needs every sample)");
  const int M = c->cfg.n_mc, d = c->cfg.d;
  const size_t es = c->esize;
  const bool full = c->cfg.family == MIVI_FULLRANK;
  mivi_status_t s = ensure_work(c, M);
  if (s) return s;
  if (!fr_prepare(c, M)) return fail(c, MIVI_ERR_HIP, "full-rank work tables: allocation or upload failed");
  const bool stl2 = full && stl2_shape_ok(c, M);
  if (full) {
    const int dP = c->dP;
    if (!stl_lds_fits(c, dP) && !stl16_lds_fits(c, dP))
      return fail(c, MIVI_ERR_UNSUPPORTED, "score gradient: d too large for the LDS-resident solve");
    // the solve's operands, as ensure_work sizes them for the sticking-the-landing estimators (no-ops on such a context)
    if ((s = ensure(c, c->stl_CT, (size_t)dP * dP * es, true)) || (s = ensure(c, c->stl_Dinv, (size_t)((d + 63) / 64) * 4096 * es, false))) return s;
    if (stl2 && ((s = ensure(c, c->stl_X, ((size_t)d * c->cap_M + (size_t)(d / 2) * (d / 2)) * es + 4096, false)) ||
                 (s = ensure(c, c->stl_F, mivi::stl_pack_units(d) * 4, false))))
      return s;
    if ((s = ensure(c, c->sg_S, (size_t)dP * c->MP * es, false))) return s;
  }
  if (c->sg_cap < c->cap_M) {
    if ((s = ensure(c, c->sg_d, 3 * (size_t)c->cap_M * sizeof(double), false))) return s;
    c->sg_cap = c->cap_M;
  }
  const RngArgs rng = rng_of(c, idx);
  eps_spec_drop(c);   // (as mivi_sample)
  if (full) {
    c->he_n[0] = launch_eps(c, rng, M);
    launch_fr_sample(c, params, M, TGT_NONE, c->Z.p);
  } else {
    launch_sample_mf(c, params, rng, M, c->Z.p, nullptr, 0, nullptr);
  }
  if (c->bij_on) launch_bij_forward(c, M);   // the target sees binv(z); its logabsdetjac per sample joins log pi in k_sg_stats
  const bool dense = c->target == TGT_DENSE_GAUSS;
  ValueIn unused{};   // (this estimator reads the per-sample values themselves -- c->ell, or sg_d for the dense target -- not their partials)
  if ((s = target_on_z(c, M, dense ? 1 : 0, 0, unused))) return s;   // dense: W = G = -P R is what it has; everything else: values only
  if (dense) launch_sg_dense_ell(c, M);   // ell_m = r_m' g_m / 2
  launch_sg_norms(c, rng, M);
  launch_sg_stats(c, params, M, dense, value, elbo);
  if (full) {
    launch_sg_scale(c, M);
    if (stl2) launch_stl2(c, params, M, false, c->sg_S.p, c->W.p);
    else launch_fr_stl(c, params, M, c->sg_S.p, c->W.p);
    OutArgs o = final_out(c, nullptr, grad);
    o.ent_kind = MIVI_ENT_CLOSED_FORM_ZERO_GRAD;   // -(1/M) [W 1; tril(W E')] and nothing else
    o.M_total = M;
    o.M_local = M;
    launch_fr_vjp(c, params, M, o);
  } else {
    launch_sg_mf_grad(c, params, rng, M, grad);
  }
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

mivi_status_t mivi_estimate_score_gradient(mivi_ctx_t *c, const void *params, uint64_t idx, void *value, void *elbo, void *grad) {
  if (!c || !params || !value || !grad) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_estimate_score_gradient")) return rs;
  (void)hipSetDevice(c->cfg.device);
  return run_score_estimate(c, params, idx, value, elbo, grad);
}

mivi_status_t mivi_estimate_score_gradient_host(mivi_ctx_t *c, const void *params_h, uint64_t idx, void *value_h, void *elbo_h, void *grad_h) {
  if (!c || !params_h || !value_h || !grad_h) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_estimate_score_gradient_host")) return rs;
  (void)hipSetDevice(c->cfg.device);
  const size_t es = c->esize;
  mivi_status_t s = stage_params(c, params_h);
  if (s) return s;
  char *o = (char *)c->tmp_out.p;   // [value | elbo | gradient]
  if ((s = run_score_estimate(c, c->tmp_params.p, idx, o, o + 8, o + 16))) return s;
  return fetch_results(c, {{value_h, o, es}, {elbo_h, o + 8, es}, {grad_h, o + 16, (size_t)mivi_params_len(c) * es}}, true);
}
