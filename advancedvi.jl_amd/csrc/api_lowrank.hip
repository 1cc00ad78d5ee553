// libmivi C ABI, the low-rank Gaussian family (MIVI_LOWRANK; src/families/location_scale_low_rank.jl): one RepGradELBO estimate as a
// sequence of launches of kernels_lowrank.hip, and rand.  run_estimate (api_estimate.hip) branches here before anything that means
// "full-rank"; every entry the family does not support refuses it through refuse_lowrank (api_common.h).
#include "api_common.h"

mivi_status_t refuse_lowrank(mivi_ctx *c, const char *entry) {
  if (mivi_status_t rs = refuse_flow(c, entry)) return rs;
  if (c->cfg.family != MIVI_LOWRANK) return MIVI_OK;
  c->err = std::string(entry) + ": not supported on the low-rank family (MIVI_LOWRANK)";
  return MIVI_ERR_UNSUPPORTED;
}

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
mivi_status_t run_estimate_lowrank(mivi_ctx *c, const void *params, const RngArgs &rng, int M, int want_grad, const OutArgs &out) {
  if (out.partials_mode) return fail(c, MIVI_ERR_UNSUPPORTED, "shard partials: not supported on the low-rank family (MIVI_LOWRANK)");
  const int ek = out.ent_kind;
  const bool closed = ek == MIVI_ENT_CLOSED_FORM || ek == MIVI_ENT_CLOSED_FORM_ZERO_GRAD;
  c->pre.clear();
  const int p = c->cur;
  ValueIn vin{};
  vin.ell_const = c->t_const;
  launch_lowr_draw_prep(c, rng, M, params);
  launch_lowr_sample(c, params, M, c->Z.p, !closed);
  if (c->bij_on) launch_bij_forward(c, M);   // the target sees binv(z)
  mivi_status_t s = target_on_z(c, M, want_grad, p, vin);
  if (s) return s;
  if (c->bij_on) launch_bij_backward(c, M, want_grad, c->target != TGT_DENSE_GAUSS);
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
