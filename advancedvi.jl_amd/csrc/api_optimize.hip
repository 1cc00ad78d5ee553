// libmivi C ABI, part 6: update rules on the device and the device-resident optimisation loop (src/optimize.jl:64-77).
#include "api_common.h"

mivi_status_t mivi_clip_scale(mivi_ctx_t *c, void *params, double epsilon) {
  if (!c || !params) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_flow(c, "mivi_clip_scale (ClipScale has no method for a family without a scale)")) return rs;
  (void)hipSetDevice(c->cfg.device);
  launch_clip(c, params, epsilon);
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}
mivi_status_t mivi_prox_scale_entropy(mivi_ctx_t *c, void *params, double stepsize, const void *dog_state, int32_t dog_kind) {
  if (!c || !params || (dog_state && dog_kind != 0 && dog_kind != 1)) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_lowrank(c, "mivi_prox_scale_entropy (the reference has no ProximalLocationScaleEntropy method for it)")) return rs;
  if (!dog_state && !(stepsize >= 0.0)) return fail(c, MIVI_ERR_BAD_ARG, "proximal step size must be non-negative");
  (void)hipSetDevice(c->cfg.device);
  launch_prox(c, params, stepsize, dog_state, dog_kind);
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}
mivi_status_t mivi_descent_update(mivi_ctx_t *c, void *params, const void *grad, double eta) {
  if (!c || !params || !grad) return MIVI_ERR_BAD_ARG;
  (void)hipSetDevice(c->cfg.device);
  launch_descent(c, params, grad, eta);
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}
mivi_status_t mivi_adam_update(mivi_ctx_t *c, void *params, const void *grad, void *state, int64_t t, double eta,
                               double b1, double b2, double eps) {
  if (!c || !params || !grad || !state || t < 1) return MIVI_ERR_BAD_ARG;
  (void)hipSetDevice(c->cfg.device);
  launch_adam(c, params, grad, state, nullptr, t, eta, b1, b2, eps);
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

mivi_status_t mivi_cocob_update(mivi_ctx_t *c, void *params, const void *grad, void *state, double alpha) {
  if (!c || !params || !grad || !state || !(alpha > 0.0)) return MIVI_ERR_BAD_ARG;
  (void)hipSetDevice(c->cfg.device);
  launch_cocob(c, params, grad, state, alpha);
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

mivi_status_t mivi_optimize_steps(mivi_ctx_t *c, void *params, void *opt_state, uint64_t idx0, int64_t t0, int32_t n_steps,
                                  int32_t rule, double eta, double clip_eps, void *elbo) {
  if (rule != 0 && rule != 1) return MIVI_ERR_BAD_ARG;
  mivi_loop_t l{};
  l.rule = rule;
  l.op = clip_eps > 0.0 ? 1 : 0;
  l.averager = 0;
  l.n_steps = n_steps;
  l.eta = eta;
  l.beta1 = 0.9;
  l.beta2 = 0.999;
  l.adam_eps = 1e-8;
  l.clip_epsilon = clip_eps;
  l.opt_state_dev = opt_state;
  l.estimate_idx0 = idx0;
  l.t0 = t0;
  l.elbo_dev = elbo;
  return mivi_optimize_loop(c, params, &l);
}

// elbo record (double, device) -> caller's T[n_steps], on the device (no host round trip inside a "launch-free" call)
__global__ void k_elbo_to_f32(int n, const double *__restrict__ rec, float *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (float)rec[i];
}
static mivi_status_t deliver_elbo(mivi_ctx *c, const double *rec, int n_steps, void *elbo) {
  if (!elbo) return MIVI_OK;
  if (c->cfg.dtype == MIVI_F64) {
    HIPCHK(c, hipMemcpyAsync(elbo, rec, (size_t)n_steps * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  } else {
    hipLaunchKernelGGL(k_elbo_to_f32, dim3((n_steps + 255) / 256), dim3(256), 0, c->stream, n_steps, rec, (float *)elbo);
    HIPCHK(c, hipGetLastError());
  }
  return MIVI_OK;
}

// One call's steps on the best route.  allow_exchange = false: the launch-free loops whose workgroups exchange partials grid-wide every step are
// skipped (their graph-of-launches equivalents run instead); *used_exchange: one of them was launched.
static mivi_status_t optimize_loop_run(mivi_ctx_t *c, void *params, const mivi_loop_t *lp, bool allow_exchange, bool *used_exchange) {
  const mivi_loop_t &l = *lp;
  const int n_steps = l.n_steps, rule = l.rule;
  if (n_steps <= 0 || rule < 0 || rule > 4 || l.op < 0 || l.op > 2 || l.averager < 0 || l.averager > 1) return MIVI_ERR_BAD_ARG;
  if (rule != 0 && !l.opt_state_dev) return fail(c, MIVI_ERR_BAD_ARG, "this optimisation rule needs opt_state_dev");
  if (l.averager == 1 && !l.avg_params_dev) return fail(c, MIVI_ERR_BAD_ARG, "PolynomialAveraging needs avg_params_dev");
  if (l.op == 2 && (rule == 1 || rule == 4)) return fail(c, MIVI_ERR_BAD_ARG, "ProximalLocationScaleEntropy does not support Adam / COCOB (Descent, DoG, DoWG: proximal_location_scale_entropy.jl:26-42)");
  if (l.op == 2)
    if (mivi_status_t rs = refuse_lowrank(c, "mivi_optimize_loop with op = 2 (the reference has no ProximalLocationScaleEntropy method for it)")) return rs;
  if (l.op == 1)
    if (mivi_status_t rs = refuse_flow(c, "mivi_optimize_loop with op = 1 (ClipScale has no method for a family without a scale; use op = 0)")) return rs;
  const bool dog = rule == 2 || rule == 3;        // the rules with two global norms per step
  if (!graph_capturable(c)) return fail(c, MIVI_ERR_UNSUPPORTED, "device-resident loop needs a built-in target");
  if (c->idx_src) return fail(c, MIVI_ERR_UNSUPPORTED, "an index source is set (mivi_set_index_source): the device-resident loop keeps its own counter");
  (void)hipSetDevice(c->cfg.device);
  mivi_status_t s = ensure_work(c, c->cfg.n_mc);
  if (s) return s;
  if (!prepare_tables(c, c->cfg.n_mc)) return fail(c, MIVI_ERR_HIP, "full-rank work tables: allocation or upload failed");
  if ((s = reserve_target(c, c->cfg.n_mc))) return s;
  const size_t plen = (size_t)mivi_params_len(c), es = c->esize;
  const double eta = l.eta, clip_eps = loop_clip_eps(l);
  void *opt_state = l.opt_state_dev;
  // internal value / grad / elbo-record buffers, and the hist / partials area: the largest any launch-free loop asks for, whichever runs
  size_t area_doubles = 0;
  for (const DeviceLoop &row : kDeviceLoops)
    if (row.hist_doubles && area_doubles < row.hist_doubles(c, n_steps)) area_doubles = row.hist_doubles(c, n_steps);
  if ((s = ensure(c, c->X, (plen + 8) * es + ((size_t)n_steps + area_doubles + 8) * sizeof(double), false))) return s;
  char *vbuf = (char *)c->X.p;
  char *gbuf = vbuf + 8 * es;
  double *rec = (double *)(((uintptr_t)(gbuf + plen * es) + 7) & ~(uintptr_t)7);
  const LoopBufs b{vbuf, gbuf, rec, rec + n_steps};
  const bool simple = rule <= 1 && l.op <= 1 && l.averager == 0;   // what the fused paths implement
  const bool general = loop_general(l);
  c->last_loop = LOOP_GRAPH;
  if (!no_device_loops(c))
    for (const DeviceLoop &row : kDeviceLoops) {
      const bool exchanges = rule >= row.exchanges_from;
      if (!row.takes(c, l, general) || (exchanges && !allow_exchange)) continue;
      if (row.reserve && (s = row.reserve(c, l))) return s;
      // every word read_status folds in: a stale flag of an earlier batch's child contexts is not this run's
      HIPCHK(c, hipMemsetAsync(c->status.p, 0, sizeof(int) * (1 + mivi_ctx::kMaxKids), c->stream));
      if (!row.launch(c, params, l, b)) continue;   // (not launched: the next row)
      c->last_loop = row.id;
      if (exchanges) *used_exchange = true;
      HIPCHK(c, hipGetLastError());
      if ((s = deliver_elbo(c, rec, n_steps, l.elbo_dev))) return s;
      return read_status(c);
    }
  // every other configuration: the steps as a graph of launches, recorded once per loop configuration
  auto record_steps = [&]() -> mivi_status_t {
    mivi_status_t s = MIVI_OK;
    Chain chn;
    chn.on = true;
    const long long *t_ptr = (const long long *)c->d_idx.p + 1;   // iterations done before this call
    // mivi_optimize_loop_batches: step i evaluates batch first + i of the schedule (launch_logreg_target passes its rows by value) and, when
    // the schedule carries them, draws at the batch's own index: a device word of the uploaded table, nothing added
    const int first = c->lr_loop_first, k_kept = c->lr_sched_k;
    const uint64_t *tab = first >= 0 && c->lr_sched_has_idx ? (const uint64_t *)c->lr_sched_idx.p + first : nullptr;
    auto rng_at = [&](uint64_t i) {
      RngArgs r = rng_of(c, tab ? 0ull : i);
      r.idx_ptr = tab ? tab + i : (const uint64_t *)c->d_idx.p;
      return r;
    };
    for (int i = 0; i < n_steps && s == MIVI_OK; ++i) {
      const RngArgs r = rng_at((uint64_t)i);
      if (first >= 0) c->lr_sched_k = first + i;
      OutArgs o = final_out(c, vbuf, gbuf);
      o.elbo_rec = rec;
      o.rec_slot = i;
      c->cur = i & 1;
      chn.has_next = (i + 1 < n_steps);
      chn.next_rng = rng_at((uint64_t)i + 1);
      // full-rank f32 MFMA path: the optimiser step (and ClipScale) rides in the VJP epilogue -- no update kernel
      const bool fuse_upd = simple && c->cfg.family == MIVI_FULLRANK && c->cfg.dtype == MIVI_F32 && hetero_ok(c, 1) &&
                            !switches().no_fused_update;
      FusedUpdate fu;
      if (fuse_upd) {
        fu.rule = rule;
        fu.params = params;
        fu.state = opt_state;
        fu.t_ptr = t_ptr;
        fu.t_base = (long long)i + 1;
        fu.eta = eta;
        fu.b1 = l.beta1;
        fu.b2 = l.beta2;
        fu.eps = l.adam_eps;
        fu.clip_eps = l.clip_epsilon;
        fu.do_clip = (l.op == 1);
      }
      s = run_estimate(c, params, r, c->cfg.n_mc, 1, o, &chn, fuse_upd ? &fu : nullptr);
      if (s) break;
      if (fuse_upd) continue;
      // Optimisers.update! (common.jl:92); ClipScale rides in the Descent / Adam kernels
      if (rule == 0) launch_descent(c, params, gbuf, eta, clip_eps);
      else if (rule == 1) launch_adam(c, params, gbuf, opt_state, (const int64_t *)t_ptr, (int64_t)i + 1, eta, l.beta1, l.beta2, l.adam_eps, clip_eps);
      else if (rule == 4) launch_cocob(c, params, gbuf, opt_state, eta /* = alpha */, clip_eps);   // rules.jl:78-96; ClipScale rides in the kernel
      else if (l.op <= 1 && launch_dog_update_fused(c, params, gbuf, opt_state, rule - 2, clip_eps,
                                                     l.averager == 1 ? l.avg_params_dev : nullptr, l.avg_eta, t_ptr, (long long)i + 1))
        continue;   // DoG / DoWG + ClipScale + averaging in one apply pass (large parameter vectors)
      else launch_dog_update(c, params, gbuf, opt_state, rule - 2);
      // operator (common.jl:93-95)
      if (l.op == 1 && dog) launch_clip(c, params, clip_eps);
      if (l.op == 2) launch_prox(c, params, eta, dog ? opt_state : nullptr, rule - 2);
      // averager (common.jl:96)
      if (l.averager == 1) launch_poly_average(c, l.avg_params_dev, params, l.avg_eta, t_ptr, (long long)i + 1);
    }
    if (s == MIVI_OK) flush_chain(c, params, &chn);
    c->cur = 0;
    c->lr_sched_k = k_kept;   // (the recorder walked it; the selected batch is the caller's)
    return s;
  };
  GraphKey key{GRAPH_LOOP, n_steps, params, vbuf};
  key.loop = l;
  key.mode = c->lr_loop_first + 1;   // (0: mivi_optimize_loop, the selected batch or the whole data set)
  if (!c->graph.matches(key)) {
    invalidate_graph(c);
    if ((s = graph_record(c, key, record_steps))) return s;
  }
  c->d_idx_valid = false;
  hipLaunchKernelGGL(k_set_u64x2, dim3(1), dim3(1), 0, c->stream, (uint64_t *)c->d_idx.p, l.estimate_idx0, (uint64_t)l.t0, 2);
  HIPCHK(c, hipMemsetAsync(c->status.p, 0, sizeof(int) * (1 + mivi_ctx::kMaxKids), c->stream));   // a stale flag of earlier estimates (this context's word or a child context's: read_status folds them all in) is not this run's
  HIPCHK(c, hipGraphLaunch(c->graph.exec.get(), c->stream));
  if ((s = deliver_elbo(c, rec, n_steps, l.elbo_dev))) return s;
  return read_status(c);
}

// `optimize`'s inner loop (src/optimize.jl:64-77) on the device.  The launch-free loops whose workgroups exchange partials every step need their
// whole grid resident: the launchers check that against the device (hipOccupancyMaxActiveBlocksPerMultiprocessor x CUs), and should an exchange
// still be lost at run time (status bit 8: another context's work took the CUs), the call restores the state it was given and runs the same
// steps on the graph of launches; the context then stays on that route.
mivi_status_t mivi_optimize_loop(mivi_ctx_t *c, void *params, const mivi_loop_t *lp) {
  if (!c || !params || !lp) return MIVI_ERR_BAD_ARG;
  const mivi_loop_t &l = *lp;
  (void)hipSetDevice(c->cfg.device);
  const size_t plen = (size_t)mivi_params_len(c), es = c->esize;
  const size_t st_bytes = !l.opt_state_dev ? 0 : (l.rule == 1 ? 2 * plen * es : (l.rule == 4 ? 5 * plen * es : (l.rule >= 2 ? (size_t)mivi_dog_state_bytes(c) : 0)));
  const size_t avg_bytes = (l.averager == 1 && l.avg_params_dev) ? plen * es : 0;
  const bool may_exchange = !c->exchange_lost && (l.rule == 2 || l.rule == 3 || c->target == TGT_FUNNEL || (c->target == TGT_LOGREG && c->lr_sched_n == 0));
  if (may_exchange && l.n_steps > 0 && l.rule >= 0 && l.rule <= 4) {
    mivi_status_t s = ensure(c, c->snap, plen * es + st_bytes + avg_bytes + 64, false);
    if (s) return s;
    char *sp = (char *)c->snap.p;
    HIPCHK(c, hipMemcpyAsync(sp, params, plen * es, hipMemcpyDeviceToDevice, c->stream));
    if (st_bytes) HIPCHK(c, hipMemcpyAsync(sp + plen * es, l.opt_state_dev, st_bytes, hipMemcpyDeviceToDevice, c->stream));
    if (avg_bytes) HIPCHK(c, hipMemcpyAsync(sp + plen * es + st_bytes, l.avg_params_dev, avg_bytes, hipMemcpyDeviceToDevice, c->stream));
  }
  bool used = false;
  c->last_status_bits = 0;   // only a bit-8 ("exchange lost") flag read by THIS call may trigger the retry below: a stale one would mask a real HIP error
  mivi_status_t s = optimize_loop_run(c, params, lp, may_exchange, &used);
  if (switches().force_exchange_lost && used && s == MIVI_OK) { s = MIVI_ERR_HIP; c->last_status_bits |= 8; }
  if (s == MIVI_ERR_HIP && used && (c->last_status_bits & 8)) {
    const char *sp = (const char *)c->snap.p;
    HIPCHK(c, hipMemcpyAsync(params, sp, plen * es, hipMemcpyDeviceToDevice, c->stream));
    if (st_bytes) HIPCHK(c, hipMemcpyAsync(l.opt_state_dev, sp + plen * es, st_bytes, hipMemcpyDeviceToDevice, c->stream));
    if (avg_bytes) HIPCHK(c, hipMemcpyAsync(l.avg_params_dev, sp + plen * es + st_bytes, avg_bytes, hipMemcpyDeviceToDevice, c->stream));
    c->exchange_lost = true;
    c->err.clear();
    used = false;
    s = optimize_loop_run(c, params, lp, false, &used);
  }
  return s;
}

// ---- mivi_optimize_loop_many: K independent runs of one shape, workgroup k = run k ---------------------------------------------------------
// c->many_buf, carved once per call: what the host uploads in ONE copy (the runs' table, their zeroed status words, the diagonal-Gaussian
// targets of the runs that bring their own), then what the kernel leaves (the f64 ELBO records [K][n_steps], the last values [K]).
struct ManyLayout {
  size_t off_status, off_mean, off_istd, up_bytes, off_rec, off_value, bytes;
};
static ManyLayout many_layout(const mivi_ctx *c, size_t K, int n_steps, bool own_target) {
  auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
  ManyLayout L;
  L.off_status = up16(K * sizeof(ManyRun));
  L.off_mean = up16(L.off_status + K * sizeof(int));
  L.off_istd = up16(L.off_mean + (own_target ? K * (size_t)c->cfg.d * c->esize : 0));
  L.up_bytes = up16(L.off_istd + (own_target ? K * (size_t)c->cfg.d * c->esize : 0));
  L.off_rec = L.up_bytes;
  L.off_value = up16(L.off_rec + K * (size_t)n_steps * sizeof(double));
  L.bytes = up16(L.off_value + (K + 8) * c->esize);
  return L;
}

// `optimize` for K independent small problems of one shape (restarts, step-size sweeps, simulated data sets: K calls of src/optimize.jl:42-94
// whose steps are src/algorithms/common.jl:69-104, at the sizes of bench/benchmarks.jl:43-94) in one launch.  Everything is validated on the
// host before anything is uploaded; the rows of kDeviceLoops that have a `launch_many` are the configurations it serves.
mivi_status_t mivi_optimize_loop_many(mivi_ctx_t *c, void *params, const mivi_loop_t *lp, const mivi_many_t *mp) {
  if (!c || !params || !lp || !mp) return MIVI_ERR_BAD_ARG;
  const mivi_loop_t &l = *lp;
  const mivi_many_t &m = *mp;
  if (m.n_runs < 1) return fail(c, MIVI_ERR_BAD_ARG, "mivi_optimize_loop_many: n_runs must be at least 1");
  if (l.n_steps > 0 && (long long)m.n_runs * l.n_steps > (1ll << 30)) return fail(c, MIVI_ERR_BAD_ARG, "mivi_optimize_loop_many: n_runs x n_steps must not exceed 2^30 (call it in chunks of steps)");
  if (l.n_steps <= 0 || l.rule < 0 || l.rule > 4 || l.op < 0 || l.op > 2 || l.averager < 0 || l.averager > 1) return fail(c, MIVI_ERR_BAD_ARG, "mivi_optimize_loop_many: n_steps, rule, op or averager out of range");
  if (l.op == 2 && l.rule == 1) return fail(c, MIVI_ERR_BAD_ARG, "ProximalLocationScaleEntropy does not support Adam (Descent, DoG, DoWG: proximal_location_scale_entropy.jl:26-42)");
  if (l.rule == 4) return fail(c, MIVI_ERR_UNSUPPORTED, "mivi_optimize_loop_many: COCOB (rule 4) has no launch-free loop");
  if (l.rule != 0 && !l.opt_state_dev) return fail(c, MIVI_ERR_BAD_ARG, "this optimisation rule needs opt_state_dev");
  if (l.averager == 1 && !l.avg_params_dev) return fail(c, MIVI_ERR_BAD_ARG, "PolynomialAveraging needs avg_params_dev");
  if (c->cfg.family == MIVI_LOWRANK) return fail(c, MIVI_ERR_UNSUPPORTED, "mivi_optimize_loop_many: the low-rank family has no launch-free loop");
  if (mivi_status_t rs = refuse_flow(c, "mivi_optimize_loop_many (the family has no launch-free loop)")) return rs;
  if (c->base != MIVI_BASE_NORMAL) return fail(c, MIVI_ERR_UNSUPPORTED, "mivi_optimize_loop_many: a non-normal base distribution has no launch-free loop");
  if (c->bij_on) return fail(c, MIVI_ERR_UNSUPPORTED, "mivi_optimize_loop_many: a Stacked bijector is set");
  if (c->cfg.m_offset != 0 || c->M_total != c->cfg.n_mc) return fail(c, MIVI_ERR_UNSUPPORTED, "mivi_optimize_loop_many: a sharded context (m_offset / m_total)");
  if (c->lr_sched_n > 0) return fail(c, MIVI_ERR_UNSUPPORTED, "mivi_optimize_loop_many: a batch schedule is set (mivi_logreg_set_batch_schedule)");
  if (c->idx_src) return fail(c, MIVI_ERR_UNSUPPORTED, "mivi_optimize_loop_many: an index source is set (mivi_set_index_source)");
  if (switches().no_fused_loop) return fail(c, MIVI_ERR_UNSUPPORTED, "mivi_optimize_loop_many: MIVI_NO_FUSED_LOOP=1 keeps the graph of launches, which has no many-run form");
  const DeviceLoop *row = nullptr;
  for (const DeviceLoop &r : kDeviceLoops)
    if (r.launch_many && r.takes_many(c, l)) { row = &r; break; }
  if (!row)
    return fail(c, MIVI_ERR_UNSUPPORTED, "mivi_optimize_loop_many: neither a small full-rank run on a diagonal-Gaussian target (d <= 32, n_mc <= 64, d n_mc <= 768; "
                                         "512 with the sticking-the-landing estimators) nor a small logistic regression that fits one workgroup");
  const bool gauss = c->target == TGT_DIAG_GAUSS;
  const size_t K = (size_t)m.n_runs, d = (size_t)c->cfg.d;
  if ((m.mean_host != nullptr) != (m.std_host != nullptr)) return fail(c, MIVI_ERR_BAD_ARG, "mivi_optimize_loop_many: mean_host and std_host come together");
  if (!gauss && m.mean_host) return fail(c, MIVI_ERR_BAD_ARG, "mivi_optimize_loop_many: mean_host / std_host are for the diagonal-Gaussian target");
  if (gauss && (m.y_dev || m.X_dev)) return fail(c, MIVI_ERR_BAD_ARG, "mivi_optimize_loop_many: y_dev / X_dev are for the logistic-regression target");
  if (m.X_dev && m.X_run_stride != 0 && m.X_run_stride < (int64_t)c->lr_n * (int64_t)(d - 1)) return fail(c, MIVI_ERR_BAD_ARG, "mivi_optimize_loop_many: X_run_stride must be 0 (one shared X) or at least n (d - 1) elements");
  const bool own_target = gauss && m.mean_host;
  const ManyLayout L = many_layout(c, K, l.n_steps, own_target);
  std::vector<char> up(L.up_bytes, 0);
  ManyRun *runs = (ManyRun *)up.data();
  for (size_t k = 0; k < K; ++k) {
    runs[k].seed = m.seed_host ? m.seed_host[k] : c->cfg.seed;
    runs[k].idx0 = m.estimate_idx0_host ? m.estimate_idx0_host[k] : l.estimate_idx0;
    runs[k].eta = m.eta_host ? m.eta_host[k] : l.eta;
    double cst = c->t_const;
    if (own_target) {   // mivi_set_target_diag_gauss's arithmetic, per run
      cst = -0.5 * (double)d * kLog2Pi;
      for (size_t i = 0; i < d; ++i) {
        const double s = host_get(m.std_host, c->cfg.dtype, k * d + i), mu = host_get(m.mean_host, c->cfg.dtype, k * d + i);
        if (!(s > 0.0)) return fail(c, MIVI_ERR_BAD_ARG, "mivi_optimize_loop_many: std must be positive");
        cst -= log(s);
        if (c->cfg.dtype == MIVI_F64) {
          ((double *)(up.data() + L.off_mean))[k * d + i] = mu;
          ((double *)(up.data() + L.off_istd))[k * d + i] = 1.0 / s;
        } else {
          ((float *)(up.data() + L.off_mean))[k * d + i] = (float)mu;
          ((float *)(up.data() + L.off_istd))[k * d + i] = (float)(1.0 / s);
        }
      }
    }
    runs[k].ell_const = cst;
  }
  (void)hipSetDevice(c->cfg.device);
  mivi_status_t s = ensure(c, c->many_buf, L.bytes, false);
  if (s) return s;
  char *base = (char *)c->many_buf.p;
  HIPCHK(c, hipStreamSynchronize(c->stream));   // (whatever read the buffer last is done: the copy below does not run on the stream)
  HIPCHK(c, hipMemcpy(base, up.data(), L.up_bytes, hipMemcpyHostToDevice));
  ManyLaunch ml{};
  ml.n_runs = m.n_runs;
  ml.runs = (const ManyRun *)base;
  ml.status = (int *)(base + L.off_status);
  ml.t_mean = own_target ? base + L.off_mean : nullptr;
  ml.t_istd = own_target ? base + L.off_istd : nullptr;
  ml.y = m.y_dev;
  ml.X = m.X_dev;
  ml.x_stride = m.X_dev ? (long long)m.X_run_stride : 0;
  double *rec = (double *)(base + L.off_rec);
  const LoopBufs b{base + L.off_value, nullptr, rec, nullptr};
  c->last_loop = LOOP_GRAPH;
  if (!row->launch_many(c, params, l, b, ml)) return fail(c, MIVI_ERR_UNSUPPORTED, "mivi_optimize_loop_many: the device refused the kernel's LDS");
  c->last_loop = LOOP_MANY | row->id;
  HIPCHK(c, hipGetLastError());
  if ((s = deliver_elbo(c, rec, (int)(K * (size_t)l.n_steps), l.elbo_dev))) return s;
  std::vector<int> st(K, 0);
  HIPCHK(c, hipMemcpyAsync(st.data(), ml.status, K * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int any = 0;
  for (size_t k = 0; k < K; ++k) {
    any |= st[k];
    if (m.status_host) m.status_host[k] = st[k];
  }
  if (m.status_host || !any) return MIVI_OK;
  if (any & 2) return fail(c, MIVI_ERR_NONPOSITIVE_SCALE, "scale diagonal is not positive in at least one run (use ClipScale)");
  return fail(c, MIVI_ERR_NONFINITE, "the objective value is not finite in at least one run: it diverged");
}

// Whole steps of a SubsampledObjective (src/algorithms/subsampledobjective.jl:64-90) on the device: the loop above over the batches
// first_batch, first_batch + 1, ... of the resident schedule.  A scheduled context takes no launch-free loop (lr_small_loop_takes sees the
// schedule), so this is the graph of launches with the batch of every step baked in (record_steps).
mivi_status_t mivi_optimize_loop_batches(mivi_ctx_t *c, void *params, const mivi_loop_t *lp, int32_t first_batch) {
  if (!c || !params || !lp) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_flow(c, "mivi_optimize_loop_batches")) return rs;
  if (c->target != TGT_LOGREG || c->lr_sched_n <= 0) return fail(c, MIVI_ERR_BAD_ARG, "mivi_optimize_loop_batches: no batch schedule set (mivi_logreg_set_batch_schedule)");
  if (first_batch < 0 || lp->n_steps <= 0 || (long long)first_batch + lp->n_steps > c->lr_sched_n)
    return fail(c, MIVI_ERR_BAD_ARG, "mivi_optimize_loop_batches: first_batch + n_steps must lie inside the schedule");
  c->lr_loop_first = first_batch;
  const mivi_status_t s = mivi_optimize_loop(c, params, lp);
  c->lr_loop_first = -1;
  return s;
}
