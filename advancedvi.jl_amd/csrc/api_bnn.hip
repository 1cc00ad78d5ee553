// libmivi C ABI, the Bayesian neural network target (include/mivi.h): mivi_set_target_bnn, the row selection mivi_bnn_select_rows
// (AdvancedVI.subsample), the posterior predictive mivi_bnn_forward and the partial planes' cap.  The target is a GENERIC one:
// eval_generic_target (api_estimate.hip) evaluates it on explicit samples through launch_bnn_target (kernels_bnn.hip), so every route that
// serves a callback target by explicit samples serves it, on the device; the target is a row of kTargets (api_common.h), whose refuse_target
// guards the entries that cannot.
#include <cmath>

#include "api_common.h"

static bool bnn_positive(double v) { return std::isfinite(v) && v > 0.0; }

mivi_status_t mivi_set_target_bnn(mivi_ctx_t *c, const mivi_bnn_t *np, const void *X, const void *y, int64_t n, int32_t p, int32_t on_device) {
  if (!c || !np || !X || !y) return MIVI_ERR_BAD_ARG;
  const mivi_bnn_t net = *np;
  if (n < 1) return fail(c, MIVI_ERR_BAD_ARG, "Bayesian neural network: n must be at least 1");
  if (p < 1 || p > MIVI_BNN_MAX_IN) return fail(c, MIVI_ERR_BAD_ARG, "Bayesian neural network: p must lie in [1, 64]");
  if (net.n_hidden < 1 || net.n_hidden > 3) return fail(c, MIVI_ERR_BAD_ARG, "Bayesian neural network: n_hidden must lie in [1, 3]");
  if (net.n_out < 0 || net.n_out > MIVI_BNN_MAX_OUT) return fail(c, MIVI_ERR_BAD_ARG, "Bayesian neural network: n_out must lie in [0, 64] (0 and 1: one output)");
  const int n_out = net.n_out >= 2 ? net.n_out : 1;
  long long d = 0;
  int prev = p;
  for (int l = 0; l < net.n_hidden; ++l) {
    if (net.hidden[l] < 1 || net.hidden[l] > MIVI_BNN_MAX_HIDDEN) return fail(c, MIVI_ERR_BAD_ARG, "Bayesian neural network: a hidden width must lie in [1, 64]");
    d += (long long)net.hidden[l] * (prev + 1);
    prev = net.hidden[l];
  }
  d += (long long)n_out * (prev + 1);
  if (c->cfg.d != d)
    return fail(c, MIVI_ERR_BAD_ARG, ("Bayesian neural network: the context's d must be the network's parameter count, " + std::to_string(d)).c_str());
  if (net.likelihood != 0 && net.likelihood != 1) return fail(c, MIVI_ERR_BAD_ARG, "Bayesian neural network: unknown likelihood (0 Bernoulli-logit, 1 Normal)");
  if (!bnn_positive(net.noise)) return fail(c, MIVI_ERR_BAD_ARG, "Bayesian neural network: noise must be positive and finite");
  if (!bnn_positive(net.prior_std)) return fail(c, MIVI_ERR_BAD_ARG, "Bayesian neural network: prior_std must be positive and finite");
  if (!bnn_positive(net.likeadj)) return fail(c, MIVI_ERR_BAD_ARG, "Bayesian neural network: likelihood adjustment must be positive and finite");
  if (n_out >= 2) {   // the head kernels keep the output layer in LDS as one more plane: the largest f64 networks do not fit
    const size_t need = mivi::bnn_head_lds_bytes(net, p, c->esize);
    if (need > MIVI_BNN_LDS_LIMIT)
      return fail(c, MIVI_ERR_BAD_ARG, ("Bayesian neural network: the multi-output network needs " + std::to_string(need) + " bytes of LDS, the limit is " +
                                        std::to_string(MIVI_BNN_LDS_LIMIT) + " (narrower layers, fewer of them, or f32)").c_str());
  }
  if (!on_device && net.likelihood == 0)
    for (int64_t r = 0; r < n; ++r) {
      const double v = c->cfg.dtype == MIVI_F32 ? (double)((const float *)y)[r] : ((const double *)y)[r];
      if (n_out == 1 && v != 0.0 && v != 1.0) return fail(c, MIVI_ERR_BAD_ARG, "Bayesian neural network: a Bernoulli label is not 0 or 1");
      if (n_out >= 2 && !(v >= 0.0 && v < (double)n_out && v == std::floor(v)))
        return fail(c, MIVI_ERR_BAD_ARG, ("Bayesian neural network: a categorical label is not an integer in [0, " + std::to_string(n_out) + ")").c_str());
    }
  (void)hipSetDevice(c->cfg.device);
  invalidate_graph(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));   // an estimate in flight may still read the previous data set
  if (on_device) {
    c->bnn_X = X;
    c->bnn_y = y;
  } else {
    mivi_status_t s;
    if ((s = upload(c, c->bnn_X_own, X, (size_t)n * p * c->esize)) || (s = upload(c, c->bnn_y_own, y, (size_t)n * (net.likelihood == 1 ? n_out : 1) * c->esize))) return s;
    c->bnn_X = c->bnn_X_own.p;
    c->bnn_y = c->bnn_y_own.p;
  }
  c->bnn = net;
  c->bnn_p = p;
  c->bnn_rows.set_full(n, net.likeadj);
  c->lr_sched_n = c->lr_sched_k = 0;   // (a logistic regression's schedule of batches goes with its target)
  c->t_const = 0.0;
  c->target = TGT_BNN;
  return MIVI_OK;
}

mivi_status_t mivi_bnn_select_rows(mivi_ctx_t *c, const int64_t *idx, int64_t b, double likeadj) {
  if (!c || b < 0 || (b > 0 && !idx)) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_rows_of_other_target(c, "mivi_bnn_select_rows", TGT_BNN)) return rs;
  if (c->target != TGT_BNN) return fail(c, MIVI_ERR_NO_TARGET, "no Bayesian neural network target set");
  (void)hipSetDevice(c->cfg.device);
  if (b > 0 && !bnn_positive(likeadj)) return fail(c, MIVI_ERR_BAD_ARG, "likelihood adjustment must be positive and finite");
  return select_rows(c, c->bnn_rows, idx, b, likeadj, false);
}

mivi_status_t mivi_bnn_forward(mivi_ctx_t *c, const void *theta, int32_t M, const void *Xnew, int64_t n_new, void *f) {
  if (!c || !theta || !Xnew || !f) return MIVI_ERR_BAD_ARG;
  if (c->target != TGT_BNN) return fail(c, MIVI_ERR_NO_TARGET, "no Bayesian neural network target set");
  if (M < 1 || n_new < 1) return fail(c, MIVI_ERR_BAD_ARG, "mivi_bnn_forward: M and n_new must be at least 1");
  (void)hipSetDevice(c->cfg.device);
  if (!launch_bnn_forward(c, theta, M, Xnew, n_new, f)) return fail(c, MIVI_ERR_HIP, "mivi_bnn_forward: the runtime refused the kernel's LDS size");
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

mivi_status_t mivi_bnn_set_part_cap(mivi_ctx_t *c, int64_t bytes) { return set_rows_cap(c, &mivi_ctx::bnn_rows, bytes); }
