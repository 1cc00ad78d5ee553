// libmivi C ABI, the RealNVP normalizing-flow family (MIVI_REALNVP; docs/src/tutorials/flows.md, defined in include/mivi.h): creation, one
// RepGradELBO estimate as a sequence of launches of kernels_flow.hip, and rand.  run_estimate (api_estimate.hip) branches here before
// anything that means "location-scale"; every entry the family does not support refuses it through refuse_flow (api_common.h; refuse_lowrank begins with it).
// The neural spline flow family (MIVI_NSF, mivi_create_spline_flow) is the other coupling flow: the same context with bins in its FlowArch,
// the same routes and the same refusals (is_flow), its own kernels behind the launchers (kernels_nsf.hip).
#include "api_common.h"

mivi_status_t refuse_flow(mivi_ctx *c, const char *entry) {
  if (!is_flow(c)) return MIVI_OK;
  c->err = std::string(entry) + ": not supported on the " + flow_family_name(c);
  return MIVI_ERR_UNSUPPORTED;
}

// what mivi_create_flow and mivi_create_spline_flow share: the limits of the conditioner, the estimators, no shards; K = 0: RealNVP
static mivi_status_t create_coupling_flow(const char *entry, const mivi_config_t *cfg, const mivi_flow_t *flow, int K, double B, mivi_ctx_t **out) {
  if (cfg->d < 2 || cfg->d > MIVI_FLOW_MAX_D || cfg->n_mc < 1) return MIVI_ERR_BAD_ARG;
  if (flow->n_layers < 1 || flow->n_layers > MIVI_FLOW_MAX_LAYERS || flow->n_hidden < 1 || flow->n_hidden > 3) return MIVI_ERR_BAD_ARG;
  FlowArch a{};
  a.K = K;
  a.B = B;
  a.d = cfg->d;
  a.L = flow->n_layers;
  a.H = flow->n_hidden;
  for (int j = 0; j < a.H; ++j) {
    if (flow->hidden[j] < 1 || flow->hidden[j] > MIVI_FLOW_MAX_HIDDEN) return MIVI_ERR_BAD_ARG;
    a.h[j] = flow->hidden[j];
  }
  if (cfg->entropy < 0 || cfg->entropy > MIVI_ENT_STL_ZERO_GRAD) return MIVI_ERR_BAD_ARG;
  if (cfg->entropy != MIVI_ENT_MONTE_CARLO && cfg->entropy != MIVI_ENT_STL) {
    fprintf(stderr, "libmivi: %s: a flow has no entropy(q): the estimators that work on it are MonteCarloEntropy (MIVI_ENT_MONTE_CARLO = 2) "
                    "and StickingTheLandingEntropy (MIVI_ENT_STL = 3)\n", entry);
    return MIVI_ERR_UNSUPPORTED;
  }
  if (cfg->m_offset != 0 || (cfg->m_total != 0 && cfg->m_total != cfg->n_mc)) return MIVI_ERR_UNSUPPORTED;   // no sharded flow estimates
  mivi_ctx_t *c = nullptr;
  const mivi_status_t s = create_context(cfg, &a, &c);
  if (s) return s;
  if (!flow_prepare(c)) {
    (void)hipGetLastError();
    (void)mivi_destroy(c);
    return MIVI_ERR_HIP;
  }
  *out = c;
  return MIVI_OK;
}

mivi_status_t mivi_create_flow(const mivi_config_t *cfg, const mivi_flow_t *flow, mivi_ctx_t **out) {
  if (!cfg || !flow || !out) return MIVI_ERR_BAD_ARG;
  if (cfg->family != MIVI_REALNVP) return MIVI_ERR_BAD_ARG;
  return create_coupling_flow("mivi_create_flow", cfg, flow, 0, 0.0, out);
}

mivi_status_t mivi_create_spline_flow(const mivi_config_t *cfg, const mivi_spline_flow_t *flow, mivi_ctx_t **out) {
  if (!cfg || !flow || !out) return MIVI_ERR_BAD_ARG;
  if (cfg->family != MIVI_NSF) return MIVI_ERR_BAD_ARG;
  if (flow->n_bins < 2 || flow->n_bins > MIVI_NSF_MAX_BINS || !(flow->bound > 0.0) || !std::isfinite(flow->bound)) return MIVI_ERR_BAD_ARG;
  const mivi_flow_t net = {flow->n_layers, flow->n_hidden, {flow->hidden[0], flow->hidden[1], flow->hidden[2]}};
  return create_coupling_flow("mivi_create_spline_flow", cfg, &net, flow->n_bins, flow->bound, out);
}

// the family's scratch for cap samples per launch (ensure_work): every x^l, the f64 log q per sample, the VJP's f64 partials
mivi_status_t ensure_work_flow(mivi_ctx *c, int cap) {
  const size_t d = c->cfg.d, L = c->flow.L;
  mivi_status_t s;
  if ((s = ensure(c, c->flow_X, (L + 1) * d * cap * c->esize, false)) || (s = ensure(c, c->flow_lq, (size_t)cap * sizeof(double), false)) ||
      (s = ensure(c, c->flow_part, (size_t)flow_slices(c->flow, cap) * (size_t)flow_params_len(c->flow) * sizeof(double), false)))
    return s;
  return MIVI_OK;
}

// One estimate over M samples (no allocation, no host synchronisation with a built-in target: capturable):
//   draws + forward (z, every x^l, log q) [-> bijector] -> target [-> bijector] [-> VJP partials: the STL sweep, the parameter sweep] -> finish
mivi_status_t run_estimate_flow(mivi_ctx *c, const void *params, const RngArgs &rng, int M, int want_grad, const OutArgs &out) {
  if (out.partials_mode) return fail(c, MIVI_ERR_UNSUPPORTED, (std::string("shard partials: not supported on the ") + flow_family_name(c)).c_str());
  if (out.ent_kind != MIVI_ENT_MONTE_CARLO && out.ent_kind != MIVI_ENT_STL)
    return fail(c, MIVI_ERR_UNSUPPORTED, "a flow has no entropy(q): use MonteCarloEntropy (2) or StickingTheLandingEntropy (3)");
  c->pre.clear();
  const int p = c->cur;
  ValueIn vin{};
  vin.ell_const = c->t_const;
  launch_flow_forward(c, params, rng, M, c->Z.p, nullptr, true);
  if (c->bij_on) launch_bij_forward(c, M);   // the target sees binv(z)
  mivi_status_t s = target_on_z(c, M, want_grad, p, vin);
  if (s) return s;
  if (c->bij_on) launch_bij_backward(c, M, want_grad, c->target != TGT_DENSE_GAUSS);
  launch_flow_vjp_finish(c, params, M, want_grad, vin, out);
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

// rand(rng, q, n_mc): Z (d x n_mc) and the base draws eps (d x n_mc)
mivi_status_t sample_flow(mivi_ctx *c, const void *params, uint64_t idx, void *Z, void *eps) {
  launch_flow_forward(c, params, rng_of(c, idx), c->cfg.n_mc, Z, eps, false);
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}
