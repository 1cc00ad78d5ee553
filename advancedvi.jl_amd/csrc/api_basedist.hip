// libmivi C ABI, the base distribution of the location-scale families (mivi_set_base_dist; MvLocationScale(location, scale, dist),
// src/families/location_scale.jl:15-19, docs/src/families.md:31-39, 72-101).  The entropy of a location-scale family is d H(phi) + log|C|,
// so against the normal base three things change: the draws, the per-sample sum of log phi(u) with the constant H(phi) in the value, and
// the sticking-the-landing right-hand side -psi(u).  run_estimate (api_estimate.hip) branches here before anything that draws its own
// normals; every entry outside the surface refuses a non-normal base through refuse_non_gaussian (api_common.h).
#include "api_common.h"

static const char *base_name(const mivi_ctx *c) { return c->base == MIVI_BASE_LAPLACE ? "Laplace" : "TDist"; }

mivi_status_t refuse_non_gaussian(mivi_ctx *c, const char *entry) {
  if (mivi_status_t rs = refuse_lowrank(c, entry)) return rs;
  if (mivi_status_t rs = refuse_batch_schedule(c, entry)) return rs;   // (these entries are also the ones that read a logistic regression's data set themselves)
  if (c->base == MIVI_BASE_NORMAL) return MIVI_OK;
  c->err = std::string(entry) + ": not supported with the non-normal base distribution " + base_name(c) + " (mivi_set_base_dist)";
  return MIVI_ERR_UNSUPPORTED;
}

// digamma(x), x > 0: the recurrence up to x >= 10, then the asymptotic series (error below 1e-16 there)
static double digamma_pos(double x) {
  double r = 0.0;
  while (x < 10.0) { r -= 1.0 / x; x += 1.0; }
  const double i2 = 1.0 / (x * x);
  const double ser = i2 * (1.0 / 12.0 - i2 * (1.0 / 120.0 - i2 * (1.0 / 252.0 - i2 * (1.0 / 240.0 - i2 * (1.0 / 132.0 - i2 * (691.0 / 32760.0 - i2 / 12.0))))));
  return r + log(x) - 0.5 / x - ser;
}

mivi_status_t mivi_set_base_dist(mivi_ctx_t *c, int32_t base, double nu) {
  if (!c) return MIVI_ERR_BAD_ARG;
  if (base != MIVI_BASE_NORMAL && base != MIVI_BASE_LAPLACE && base != MIVI_BASE_TDIST) return fail(c, MIVI_ERR_BAD_ARG, "mivi_set_base_dist: unknown base distribution");
  if (base == MIVI_BASE_TDIST && !(nu > 0.0 && isfinite(nu))) return fail(c, MIVI_ERR_BAD_ARG, "mivi_set_base_dist: TDist needs finite degrees of freedom nu > 0");
  if (base != MIVI_BASE_NORMAL) {
    if (c->cfg.family == MIVI_LOWRANK) return fail(c, MIVI_ERR_UNSUPPORTED, "mivi_set_base_dist: a non-normal base is not supported on the low-rank family (MIVI_LOWRANK)");
    if (mivi_status_t rs = refuse_flow(c, "mivi_set_base_dist with a non-normal base (the flow's base is the standard normal)")) return rs;
    if (c->cfg.m_offset != 0 || (c->cfg.m_total != 0 && c->cfg.m_total != c->cfg.n_mc))
      return fail(c, MIVI_ERR_UNSUPPORTED, "mivi_set_base_dist: a non-normal base is not supported on a sharded context");
  }
  if (base != MIVI_BASE_TDIST) nu = 0.0;
  if (base == c->base && nu == c->base_nu) return MIVI_OK;   // (nothing changes: a context that never left the normal base is not touched at all)
  (void)hipSetDevice(c->cfg.device);
  const double ln2 = 0.69314718055994530942, lnpi = 1.1447298858494001741;
  c->base = base;
  c->base_nu = nu;
  c->base_c0 = 0.0;
  c->base_H = 0.0;
  if (base == MIVI_BASE_LAPLACE) {
    c->base_c0 = ln2;
    c->base_H = 1.0 + ln2;
  } else if (base == MIVI_BASE_TDIST) {
    const double a = 0.5 * (nu + 1.0), b = 0.5 * nu;
    c->base_c0 = -(lgamma(a) - lgamma(b) - 0.5 * (log(nu) + lnpi));
    c->base_H = a * (digamma_pos(a) - digamma_pos(b)) + 0.5 * log(nu) + (lgamma(b) + 0.5 * lnpi - lgamma(a));   // lbeta(nu/2, 1/2), lgamma(1/2) = ln(pi)/2
  }
  c->cap_M = 0;   // (re)allocate the work buffers incl. the base's planes
  eps_spec_drop(c);
  invalidate_graph(c);
  return MIVI_OK;
}

// the base's planes for cap samples per launch (ensure_work): zeroed, the kernels keep their padding zero; one the configuration does not read is released
mivi_status_t ensure_work_base(mivi_ctx *c, int cap) {
  const size_t plane = (size_t)c->dP * (size_t)cap * c->esize;
  mivi_status_t s;
  if (c->cfg.family != MIVI_MEANFIELD) c->bd_U.release();
  else if ((s = ensure_zeroed(c, c->bd_U, plane))) return s;
  if (!stl_entropy(c)) c->bd_R.release();
  else if ((s = ensure_zeroed(c, c->bd_R, plane))) return s;
  return MIVI_OK;
}

// One estimate over M samples with a non-normal base (no allocation, no host synchronisation with a built-in target):
//   draws (U, U^T, the partials of -sum log phi; STL kinds: -psi(U)) -> sample [-> bijector] -> target [-> bijector]
//   full rank : [-> STL solve W += C^-T (-psi(U))] -> VJP -> value
//   mean field: -> gradient rows (the STL term folded in) -> value
mivi_status_t run_estimate_base(mivi_ctx *c, const void *params, const RngArgs &rng, int M, int want_grad, const OutArgs &out) {
  if (out.partials_mode) {
    c->err = std::string("shard partials: not supported with the non-normal base distribution ") + base_name(c) + " (mivi_set_base_dist)";
    return MIVI_ERR_UNSUPPORTED;
  }
  const bool full = c->cfg.family == MIVI_FULLRANK;
  const bool stl = want_grad && (out.ent_kind == MIVI_ENT_STL || out.ent_kind == MIVI_ENT_STL_ZERO_GRAD);
  if (stl && !c->bd_R.p) return fail(c, MIVI_ERR_UNSUPPORTED, "sticking-the-landing gradient on a context created with another entropy estimator");
  if (stl && full && !stl_lds_fits(c, c->dP) && !c->stl_CT.p) return fail(c, MIVI_ERR_UNSUPPORTED, "full-rank STL: d too large for the LDS-resident solve");
  c->pre.clear();
  const int p = c->cur;
  ValueIn vin{};
  vin.ell_const = c->t_const;
  vin.base = c->base;
  vin.base_c0 = c->base_c0;
  vin.base_H = c->base_H;
  void *U = full ? c->eps[p].p : c->bd_U.p;
  void *R = stl ? c->bd_R.p : nullptr;
  launch_bd_draw(c, rng, M, U, full ? c->epsT[p].p : nullptr, R);
  vin.he_part = (const double *)c->he_part[p].p;
  vin.n_he_part = eps_blocks(c, M);
  if (full) launch_fr_sample(c, params, M, TGT_NONE, c->Z.p);
  else launch_bd_mf_sample(c, params, M, U, c->Z.p);
  if (c->bij_on) launch_bij_forward(c, M);   // the target sees binv(z)
  mivi_status_t s = target_on_z(c, M, want_grad, p, vin);
  if (s) return s;
  if (c->bij_on) launch_bij_backward(c, M, want_grad, c->target != TGT_DENSE_GAUSS);
  if (want_grad) {
    if (full) {
      if (stl) {   // W += C^-T (-psi(U)): the solves of the Gaussian route (stl_term, api_estimate.hip) with the base's right-hand side
        if (stl2_shape_ok(c, M)) launch_stl2(c, params, M, false, R);
        else launch_fr_stl(c, params, M, R);
      }
      launch_fr_vjp(c, params, M, out);
      vin.ld_part = (const double *)c->ld_part[p].p;   // emitted by the VJP kernel's diagonal tiles
      vin.n_ld_part = fr_ld_blocks(c);
    } else {
      launch_bd_mf_grad(c, params, M, U, R, out);
    }
  }
  launch_value_only(c, params, vin, out);
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

// rand(rng, q, n_mc) (location_scale.jl:76-86 with the base's draws): Z (d x n_mc) and the draws u as eps (d x n_mc)
mivi_status_t sample_base(mivi_ctx *c, const void *params, uint64_t idx, void *Z, void *eps) {
  const int M = c->cfg.n_mc, d = c->cfg.d;
  const bool full = c->cfg.family == MIVI_FULLRANK;
  eps_spec_drop(c);
  void *U = full ? c->eps[0].p : c->bd_U.p;
  launch_bd_draw(c, rng_of(c, idx), M, U, full ? c->epsT[0].p : nullptr, nullptr);
  if (full) launch_fr_sample(c, params, M, TGT_NONE, Z);
  else launch_bd_mf_sample(c, params, M, U, Z);
  if (eps)
    HIPCHK(c, hipMemcpy2DAsync(eps, (size_t)d * c->esize, U, (size_t)c->dP * c->esize, (size_t)d * c->esize, M, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}
