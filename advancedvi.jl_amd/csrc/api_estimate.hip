// libmivi C ABI, part 2: the estimate driver -- one RepGradELBO estimate as a sequence of kernel launches
// (estimate_gradient!, src/algorithms/repgradelbo.jl:151-177), mivi_sample, partials / finalisation.
#include "api_common.h"

// ---------------------------------------------------------------------------------------------
// estimate driver
// ---------------------------------------------------------------------------------------------
// a target registered with mivi_set_target_value_callback (LogDensityOrder 0) asked for its gradient
static const char *const kValueOnlyTarget =
    "the target has only a value callback (mivi_set_target_value_callback): this entry needs the target's gradient -- use "
    "mivi_estimate_score_gradient / mivi_estimate_objective, or register mivi_set_target_callback";

mivi_status_t eval_generic_target(mivi_ctx *c, int M, int want_grad) {
  switch (c->target) {
    case TGT_DIAG_GAUSS:
    case TGT_FUNNEL:
      launch_col_target(c, M, want_grad);
      return MIVI_OK;
    case TGT_LOGREG:
      if (!launch_logreg_target(c, M, want_grad)) return fail(c, MIVI_ERR_HIP, "logistic regression: scratch allocation failed");
      return MIVI_OK;
    case TGT_CALLBACK: {
      if (want_grad && !c->cb_grad) return fail(c, MIVI_ERR_UNSUPPORTED, kValueOnlyTarget);
      const size_t es = c->esize, d = c->cfg.d;
      c->h_Z.resize(d * M * es);
      c->h_G.resize(d * M * es);
      c->h_ell.resize((size_t)M * es);
      HIPCHK(c, hipMemcpyAsync(c->h_Z.data(), c->Z.p, d * M * es, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      int rc;
      if ((!want_grad && c->cb_value) || !c->cb_grad)
        rc = c->cb_value(c->cb_user, c->h_Z.data(), (int)d, M, c->h_ell.data());
      else
        rc = c->cb_grad(c->cb_user, c->h_Z.data(), (int)d, M, c->h_ell.data(), c->h_G.data());
      if (rc != 0) return fail(c, MIVI_ERR_BAD_ARG, "target callback returned non-zero");
      HIPCHK(c, hipMemcpyAsync(c->ell.p, c->h_ell.data(), (size_t)M * es, hipMemcpyHostToDevice, c->stream));
      if (want_grad) HIPCHK(c, hipMemcpyAsync(c->W.p, c->h_G.data(), d * M * es, hipMemcpyHostToDevice, c->stream));
      return MIVI_OK;
    }
    default:
      return fail(c, MIVI_ERR_NO_TARGET, "no target set");
  }
}

bool hetero_ok(const mivi_ctx *c, int want_grad, const Chain *ch) {
  if (!want_grad || c->bij_on || c->base != MIVI_BASE_NORMAL) return false;   // (a Stacked bijector, a non-normal base: the explicit-sample routes)
  // (the fused funnel target's value workgroup also finishes two gradient entries, which an optimiser step right after the
  //  estimate must already see: chained only when nothing reads the gradient between the estimates)
  if (c->cfg.family == MIVI_MEANFIELD)
    return c->target == TGT_DIAG_GAUSS || (c->target == TGT_FUNNEL && !c->funnel_constrained && ch && ch->estimates_only);
  return c->target == TGT_DIAG_GAUSS || c->target == TGT_DENSE_GAUSS;
}

// Second-generation full-rank route (kernels_fullrank_lds.hip): f32, d and M multiples of 64, fused Gaussian targets,
// 16-byte aligned parameter / gradient vectors.  Everything else (and MIVI_FR_GEN1=1) takes the first-generation kernels.
bool lds_route(const mivi_ctx *c, const void *params, int M, int want_grad, const OutArgs &out) {
  if (!lds_path_shape_ok(c, M) || c->bij_on) return false;
  if (c->target != TGT_DIAG_GAUSS && c->target != TGT_DENSE_GAUSS) return false;
  if ((uintptr_t)params & 15) return false;
  if (want_grad && !out.partials_mode && ((uintptr_t)out.grad & 15)) return false;
  return true;
}

// ---- the eps speculation (c->pre): "the VJP of estimate idx also draws eps of idx + 1, and the next call skips its eps kernel" ----
EpsLookup eps_spec_lookup(mivi_ctx *c, const RngArgs &rng, int M) {
  EpsLookup lk{};
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamGetCaptureInfo(c->stream, &cs, &lk.cap_id) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
  lk.capturing = cs == hipStreamCaptureStatusActive;
  if (!lk.capturing) lk.cap_id = 0;
  const EpsSpec &s = c->pre;
  lk.hit = s.valid && s.M == M && s.rng.seed == rng.seed && s.rng.idx_base == rng.idx_base && s.rng.idx_ptr == rng.idx_ptr &&
           s.rng.m_offset == rng.m_offset && s.capturing == lk.capturing && s.capture_id == lk.cap_id;
  return lk;
}

void eps_spec_publish(mivi_ctx *c, const RngArgs &next_rng, int M, int parity, const EpsLookup &lk) {
  c->pre.valid = true;
  c->pre.rng = next_rng;
  c->pre.M = M;
  c->pre.parity = parity;
  c->pre.capturing = lk.capturing;
  c->pre.capture_id = lk.cap_id;
}

void eps_spec_drop(mivi_ctx *c) {
  c->cur = 0;
  c->pre.clear();
}

// ---- steps the two drivers share ----
// The eps job that rides in this estimate's kernels: the chain's next estimate, the speculated one, or none.
static const EpsJob *next_eps_job(EpsJob &nx, const RngArgs &rng, int p, const Chain *ch, bool chained, bool spec) {
  if (chained && ch->has_next) {
    nx.rng = ch->next_rng;
  } else if (spec) {   // speculate that the caller asks for estimate idx + 1 next (an SGD loop does)
    nx.rng = rng;
    nx.rng.idx_base = rng.idx_base + 1ull;   // (a single call: the NEXT index, whatever stride an earlier batched call left on this context)
  } else {
    return nullptr;
  }
  nx.parity = p ^ 1;
  return &nx;
}

// Z (behind the bijector, if one is set) is in memory: evaluate the target on it and wire what it leaves into vin.
mivi_status_t target_on_z(mivi_ctx *c, int M, int want_grad, int p, ValueIn &vin) {
  if (c->target == TGT_DENSE_GAUSS) {
    launch_rt_from_z(c, M);
    launch_fr_dense_target(c, M, want_grad);
    vin.ell_part = (const double *)c->ell_part[p].p;
    vin.n_ell_part = fr_dense_blocks(c, M);
    if (c->bij_on) { vin.ell = c->bij_ld.p; vin.n_ell = M; }   // + logabsdetjac per sample
    return MIVI_OK;
  }
  if (logreg_uses_mfma(c, M)) launch_rt_from_z(c, M);   // Z^T for the MFMA route
  const mivi_status_t s = eval_generic_target(c, M, want_grad);
  if (s) return s;
  vin.ell = c->ell.p;
  vin.n_ell = M;
  return MIVI_OK;
}

// The sticking-the-landing term W += C^-T eps of a full-rank gradient estimate (nothing for the other estimators).
// dinv_done: the product kernel's riders have already inverted the diagonal blocks of C.
static mivi_status_t stl_term(mivi_ctx *c, const void *params, int M, const OutArgs &out, bool dinv_done) {
  if (out.ent_kind != MIVI_ENT_STL && out.ent_kind != MIVI_ENT_STL_ZERO_GRAD) return MIVI_OK;
  if (!stl_lds_fits(c, c->dP) && !c->stl_CT.p) return fail(c, MIVI_ERR_UNSUPPORTED, "full-rank STL: d too large for the LDS-resident solve");
  if (stl2_shape_ok(c, M)) launch_stl2(c, params, M, dinv_done);
  else launch_fr_stl(c, params, M);
  return MIVI_OK;
}

// The mean-field kernel's partials: [ell | 0.5 eps^2 | log-det], mf_nblk each, in sc_part[p].
static void wire_mf_partials(const mivi_ctx *c, int p, ValueIn &vin) {
  const double *sc = (const double *)c->sc_part[p].p;
  vin.ell_part2 = sc;
  vin.n_ell_part2 = c->mf_nblk;
  vin.he_part = sc + c->mf_nblk;
  vin.n_he_part = c->mf_nblk;
  vin.ld_part = sc + 2 * (size_t)c->mf_nblk;
  vin.n_ld_part = c->mf_nblk;
}

// One estimate on the second-generation route:
//   [k_eps unless the previous estimate's product kernel already drew this eps]
//   k_fr_prod32 / k_fr_prod64 <SAMPLE> (z, fused target, ell / log-det partials, riders: eps of the next estimate, STL operands)
//   [dense target: the same kernel <DENSE>]  [STL: back substitution]  -> k_fr_vjp32 / k_fr_vjp64 (+ this estimate's value)
static mivi_status_t run_estimate_lds(mivi_ctx *c, const void *params, const RngArgs &rng, int M, int want_grad, OutArgs out,
                                      Chain *ch, const FusedUpdate *upd, bool stop_after_target) {
  if (!lds_prepare(c, M)) return fail(c, MIVI_ERR_HIP, "full-rank work lists: allocation failed");
  ValueIn vin{};
  vin.ell_const = c->t_const;
  const bool grad_stage = want_grad && !stop_after_target;
  const bool chained = ch && ch->on && grad_stage && !out.partials_mode;
  const bool spec = !chained && want_grad;   // (also the Stein estimator's calls: stop_after_target)
  const EpsLookup lk = spec ? eps_spec_lookup(c, rng, M) : EpsLookup{};
  c->pre.clear();
  if (!chained) c->cur = lk.hit ? c->pre.parity : 0;
  const int p = c->cur;
  if (chained ? ch->first : !lk.hit) {
    c->he_n[p] = launch_eps(c, rng, M);   // (kept: on this route the product kernel's riders draw eps in blocks of their own, see below)
  }
  vin.he_part = (const double *)c->he_part[p].p;
  vin.n_he_part = c->he_n[p];
  EpsJob nx{};
  const EpsJob *next = next_eps_job(nx, rng, p, ch, chained, spec);
  const bool dense = c->target == TGT_DENSE_GAUSS;
  const bool p32 = lds_use_prod32(c, M);
  bool dinv_done = false;
  if (p32) {   // unsplit 32 x 32 tiles with the target fused into the epilogue: one kernel from eps to W
    const bool stl_here = (grad_stage && (out.ent_kind == MIVI_ENT_STL || out.ent_kind == MIVI_ENT_STL_ZERO_GRAD) && stl2_shape_ok(c, M)) ||
                          (c->want_stl_pack && c->stl_F.p);   // (the Stein estimator's solve: the riders prepare its operands too)
    // (a chain of estimates with no optimiser step in between reads the SAME parameters: the solve's parameter-only preparation of
    //  the chain's first estimate stays valid, the later ones carry no STL riders)
    const bool reuse_pack = stl_here && chained && ch->estimates_only && !ch->first;
    launch_lds_prod32(c, params, M, false, dense ? R_DENSE_R : R_DIAG, nullptr, next, grad_stage, stl_here && !reuse_pack);
    dinv_done = stl_here;
    c->stl_pack_done = stl_here;
    if (next) c->he_n[p ^ 1] = lds_prod32_eps_blocks(c, M);
    if (dense) launch_lds_prod32(c, params, M, true, R_DENSE_G, nullptr, nullptr, false);
    vin.ell_part = (const double *)c->ell_part[p].p;
    vin.n_ell_part = lds_prod32_tiles(c, M);
  } else {   // large shapes: unsplit 64 x 64 tiles, the target fused into the epilogue
    launch_lds_prod64(c, params, M, false, dense ? R_DENSE_R : R_DIAG, nullptr, next, grad_stage);
    if (next) c->he_n[p ^ 1] = lds_eps_blocks(c, M);
    if (dense) launch_lds_prod64(c, params, M, true, R_DENSE_G, nullptr, nullptr, false);
    vin.ell_part = (const double *)c->ell_part[p].p;
    vin.n_ell_part = lds_prod64_tiles(c, M);
  }
  if (ch) { ch->have_prev = false; ch->first = !chained; }
  if (grad_stage) {
    const mivi_status_t s = stl_term(c, params, M, out, dinv_done);
    if (s) return s;
    vin.ld_part = (const double *)c->ld_part[p].p;   // left by the reduce kernel (the VJP kernel may already be updating C)
    vin.n_ld_part = p32 ? fr_ld_blocks(c) : lds_ld_blocks(c);
    ValueJob self{vin, out};
    launch_lds_vjp(c, params, M, out, &self, chained ? upd : nullptr);
    if (spec) eps_spec_publish(c, nx.rng, M, p ^ 1, lk);
    HIPCHK(c, hipGetLastError());
    return MIVI_OK;
  }
  if (spec) eps_spec_publish(c, nx.rng, M, p ^ 1, lk);   // (the Stein path too: its product kernel carried the draw of idx + 1 as well)
  if (c->defer_value) {   // (Stein estimator: its accumulation kernel assembles the value partials in one of its own workgroups)
    *c->defer_value = ValueJob{vin, out};
    c->value_deferred = true;
  } else {
    launch_value_only(c, params, vin, out);
  }
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

// One estimate over M local samples. out.partials_mode selects final vs shard partials.
mivi_status_t run_estimate(mivi_ctx *c, const void *params, const RngArgs &rng, int M, int want_grad,
                                  OutArgs out, Chain *ch, const FusedUpdate *upd,
                                  bool stop_after_target) {
  if (c->target == TGT_NONE) return fail(c, MIVI_ERR_NO_TARGET, "no target set");
  if (want_grad && c->target == TGT_CALLBACK && !c->cb_grad) return fail(c, MIVI_ERR_UNSUPPORTED, kValueOnlyTarget);
  mivi_status_t s = ensure_work(c, M);
  if (s) return s;
  out.M_local = M;
  if (!out.status) out.status = (int *)c->status.p;
  const bool gen2 = c->cfg.family == MIVI_FULLRANK && c->base == MIVI_BASE_NORMAL && lds_route(c, params, M, want_grad, out);
  if (!gen2 && !fr_prepare(c, M)) return fail(c, MIVI_ERR_HIP, "full-rank work tables: allocation or upload failed");   // (cached: a compare per estimate)
  if (c->cfg.family == MIVI_LOWRANK) return run_estimate_lowrank(c, params, rng, M, want_grad, out);   // (its own kernels; nothing below knows the family)
  if (is_flow(c)) return run_estimate_flow(c, params, rng, M, want_grad, out);
  if (c->base != MIVI_BASE_NORMAL) return run_estimate_base(c, params, rng, M, want_grad, out);   // (everything below draws its own normals)
  if (gen2) return run_estimate_lds(c, params, rng, M, want_grad, out, ch, upd, stop_after_target);
  ValueIn vin{};
  vin.ell_const = c->t_const;
  const int d = c->cfg.d, d4 = (d + 3) / 4;
  const bool chained = ch && ch->on && hetero_ok(c, want_grad, ch) && !out.partials_mode;
  // single calls on the MFMA full-rank path: did the previous call's VJP kernel already generate this estimate's eps?
  // (not the Stein estimator's calls: here the draw of idx + 1 rides in the VJP kernel, which stop_after_target never launches)
  const bool spec = !chained && c->cfg.family == MIVI_FULLRANK && hetero_ok(c, want_grad) && !stop_after_target;
  const EpsLookup lk = spec ? eps_spec_lookup(c, rng, M) : EpsLookup{};
  c->pre.clear();
  if (!chained) c->cur = lk.hit ? c->pre.parity : 0;
  const int p = c->cur;
  const ValueJob *prev = (chained && ch->have_prev) ? &ch->prev : nullptr;

  if (c->cfg.family == MIVI_MEANFIELD) {
    const bool bij = c->bij_on;
    if (!bij && (c->target == TGT_DIAG_GAUSS || (c->target == TGT_FUNNEL && want_grad && !c->funnel_constrained))) {
      launch_mf_main(c, params, rng, M, want_grad, nullptr, vin, out, prev);
      if (c->target == TGT_FUNNEL) {   // row 0 and ell are finished by whoever assembles the value (FunnelFin)
        vin.fn.ab = (const double *)c->sc_part[p].p + 4 * (size_t)c->mf_nblk;
        vin.fn.n_part = c->mf_nblk;
        vin.fn.params = params;
        vin.fn.rng = rng;
        vin.fn.d4 = d4;
        vin.fn.M = M;
        vin.fn.sigma_v = c->funnel_sigma_v;
      }
      wire_mf_partials(c, p, vin);
    } else {
      launch_sample_mf(c, params, rng, M, c->Z.p, nullptr, 0, want_grad ? nullptr : (double *)c->he_part[p].p);
      if (bij) launch_bij_forward(c, M);   // the target sees binv(z)
      if ((s = target_on_z(c, M, want_grad, p, vin))) return s;
      if (bij) launch_bij_backward(c, M, want_grad, c->target != TGT_DENSE_GAUSS);
      if (want_grad) {
        launch_mf_main(c, params, rng, M, 1, c->W.p, vin, out);
        wire_mf_partials(c, p, vin);   // (ell_part2: zeros for the non-fused target; he / logdet live here)
      } else {
        vin.he_part = (const double *)c->he_part[p].p;
        vin.n_he_part = ((d4 + 255) / 256) * M;
      }
    }
  } else {
    if (chained ? ch->first : !lk.hit) launch_eps(c, rng, M);   // otherwise generated inside the previous VJP kernel
    vin.he_part = (const double *)c->he_part[p].p;
    vin.n_he_part = eps_blocks(c, M);   // (not he_n: on this route every producer of eps leaves eps_blocks partials)
    if (c->bij_on) {   // Stacked bijector: explicit samples, transformed in place around whatever target is set
      launch_fr_sample(c, params, M, TGT_NONE, c->Z.p);
      launch_bij_forward(c, M);
      if ((s = target_on_z(c, M, want_grad, p, vin))) return s;
      launch_bij_backward(c, M, want_grad, c->target != TGT_DENSE_GAUSS);
    } else if (c->target == TGT_DIAG_GAUSS) {
      launch_fr_sample(c, params, M, TGT_DIAG_GAUSS, nullptr, prev);
      vin.ell_part = (const double *)c->ell_part[p].p;
      vin.n_ell_part = fr_sample_blocks(c, M);
    } else if (c->target == TGT_DENSE_GAUSS) {
      launch_fr_sample(c, params, M, TGT_DENSE_GAUSS, c->Z.p, prev);
      launch_fr_dense_target(c, M, want_grad);
      vin.ell_part = (const double *)c->ell_part[p].p;
      vin.n_ell_part = fr_dense_blocks(c, M);
    } else {
      const bool lr32 = c->target == TGT_LOGREG && c->cfg.dtype == MIVI_F32;
      launch_fr_sample(c, params, M, lr32 ? TGT_LOGREG : TGT_NONE, c->Z.p);   // LogReg: also leaves Z^T in RT
      if ((s = eval_generic_target(c, M, want_grad))) return s;
      vin.ell = c->ell.p;
      vin.n_ell = M;
    }
    if (want_grad && !stop_after_target) {   // (the Stein estimator stops here: eps, W = grad log pi and the ell sums are ready)
      if ((s = stl_term(c, params, M, out, false))) return s;
      EpsJob nx{};
      const EpsJob *next = next_eps_job(nx, rng, p, ch, chained, spec);
      if (spec) {          // this estimate's value rides in the same kernel: no separate value launch
        ValueJob self{vin, out};
        launch_fr_vjp(c, params, M, out, next, &self);
        eps_spec_publish(c, nx.rng, M, p ^ 1, lk);
        if (ch) { ch->have_prev = false; ch->first = true; }
        HIPCHK(c, hipGetLastError());
        return MIVI_OK;
      }
      launch_fr_vjp(c, params, M, out, next, nullptr, chained ? upd : nullptr);
      vin.ld_part = (const double *)c->ld_part[p].p;   // emitted by the VJP kernel's diagonal tiles
      vin.n_ld_part = fr_ld_blocks(c);
    }
  }
  // ---- objective value (or the two scalar partials) -------------------------------------------------
  if (chained) {
    ch->prev.vin = vin;
    ch->prev.out = out;
    ch->have_prev = true;
    ch->first = false;
  } else {
    if (ch) { ch->have_prev = false; ch->first = true; }
    launch_value_only(c, params, vin, out);
  }
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

void flush_chain(mivi_ctx *c, const void *params, Chain *ch) {
  if (ch->have_prev) launch_value_only(c, params, ch->prev.vin, ch->prev.out);
  ch->have_prev = false;
}

OutArgs final_out(mivi_ctx *c, void *value, void *grad) {
  OutArgs o{};
  o.grad = grad;
  o.value = value;
  o.partials = nullptr;
  o.partials_mode = 0;
  o.ent_kind = c->cfg.entropy;
  o.M_total = c->M_total;
  o.status = (int *)c->status.p;
  return o;
}

RngArgs rng_of(mivi_ctx *c, uint64_t idx) {
  RngArgs r;
  r.seed = c->cfg.seed;
  r.idx_base = idx;
  r.idx_ptr = c->idx_src;
  r.m_offset = c->cfg.m_offset;
  return r;
}

mivi_status_t mivi_sample(mivi_ctx_t *c, const void *params, uint64_t idx, void *Z, void *eps) {
  if (!c || !params || !Z) return MIVI_ERR_BAD_ARG;
  (void)hipSetDevice(c->cfg.device);
  const int M = c->cfg.n_mc, d = c->cfg.d;
  mivi_status_t s = ensure_work(c, M);
  if (s) return s;
  if (c->cfg.family == MIVI_FULLRANK && !fr_prepare(c, M)) return fail(c, MIVI_ERR_HIP, "full-rank work tables: allocation or upload failed");
  if (c->cfg.family == MIVI_LOWRANK) return sample_lowrank(c, params, idx, Z, eps);
  if (is_flow(c)) return sample_flow(c, params, idx, Z, eps);
  if (c->base != MIVI_BASE_NORMAL) return sample_base(c, params, idx, Z, eps);
  if (c->cfg.family == MIVI_MEANFIELD) {
    launch_sample_mf(c, params, rng_of(c, idx), M, Z, eps, d, nullptr);
  } else {
    eps_spec_drop(c);
    launch_eps(c, rng_of(c, idx), M);
    launch_fr_sample(c, params, M, TGT_NONE, Z);
    if (eps)
      HIPCHK(c, hipMemcpy2DAsync(eps, (size_t)d * c->esize, c->eps[0].p, (size_t)c->dP * c->esize, (size_t)d * c->esize, M,
                                 hipMemcpyDeviceToDevice, c->stream));
  }
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

mivi_status_t mivi_estimate_gradient(mivi_ctx_t *c, const void *params, uint64_t idx, void *value, void *grad) {
  if (!c || !params || !value || !grad) return MIVI_ERR_BAD_ARG;
  (void)hipSetDevice(c->cfg.device);
  return run_estimate(c, params, rng_of(c, idx), c->cfg.n_mc, 1, final_out(c, value, grad));
}

mivi_status_t read_status(mivi_ctx *c) {
  // this context's sticky flags (word 0) and, with interleaved chains, the children's (words 1 .. n_kids of the same buffer: their kernels are
  // joined into this stream by the batch's graph) -- one copy, one wait
  int sk[1 + mivi_ctx::kMaxKids] = {};
  const int nw = 1 + c->n_kids;
  HIPCHK(c, hipMemcpyAsync(sk, c->status.p, sizeof(int) * nw, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int st = 0;
  for (int j = 0; j < nw; ++j) st |= sk[j];
  c->last_status_bits = st;
  if (st) HIPCHK(c, hipMemsetAsync(c->status.p, 0, sizeof(int) * nw, c->stream));
  if (st & 8) return fail(c, MIVI_ERR_HIP, "a device-side wait expired (peer-to-peer exchange: a peer did not arrive within the spin budget -- lost rank or unmapped buffer; a launch-free loop with a per-step exchange -- funnel target, DoG / DoWG, tile ownership: its workgroups did not run side by side)");
  if (st & 2) return fail(c, MIVI_ERR_NONPOSITIVE_SCALE, "scale diagonal is not positive (use ClipScale)");
  if (st & 1) return fail(c, MIVI_ERR_NONFINITE, "the objective value is not finite: the optimization run diverged");
  return MIVI_OK;
}

// ---- the _host boundary: parameters up into tmp_params, the device entry, results down out of tmp_out, wait ----
mivi_status_t stage_params(mivi_ctx *c, const void *params_h) {
  HIPCHK(c, hipMemcpyAsync(c->tmp_params.p, params_h, (size_t)mivi_params_len(c) * c->esize, hipMemcpyHostToDevice, c->stream));
  return MIVI_OK;
}

mivi_status_t fetch_results(mivi_ctx *c, std::initializer_list<HostCopy> res, bool with_status) {
  for (const HostCopy &r : res)
    if (r.host) HIPCHK(c, hipMemcpyAsync(r.host, r.dev, r.bytes, hipMemcpyDeviceToHost, c->stream));
  if (with_status) return read_status(c);   // waits; MIVI_ERR_NONPOSITIVE_SCALE / MIVI_ERR_NONFINITE
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MIVI_OK;
}

mivi_status_t mivi_estimate_gradient_host(mivi_ctx_t *c, const void *params_h, uint64_t idx, void *value_h, void *grad_h) {
  if (!c || !params_h || !value_h || !grad_h) return MIVI_ERR_BAD_ARG;
  (void)hipSetDevice(c->cfg.device);
  mivi_status_t s = stage_params(c, params_h);
  if (s) return s;
  char *o = (char *)c->tmp_out.p;
  if ((s = run_estimate(c, c->tmp_params.p, rng_of(c, idx), c->cfg.n_mc, 1, final_out(c, o, o + 16)))) return s;
  return fetch_results(c, {{value_h, o, c->esize}, {grad_h, o + 16, (size_t)mivi_params_len(c) * c->esize}}, true);
}

mivi_status_t mivi_estimate_partials(mivi_ctx_t *c, const void *params, uint64_t idx, void *partials) {
  if (!c || !params || !partials) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_estimate_partials")) return rs;
  (void)hipSetDevice(c->cfg.device);
  OutArgs o = final_out(c, nullptr, nullptr);
  o.partials = partials;
  o.partials_mode = 1;
  o.scalars_off = mivi_partials_len(c) - 2;
  return run_estimate(c, params, rng_of(c, idx), c->cfg.n_mc, 1, o);
}

mivi_status_t mivi_finalize(mivi_ctx_t *c, const void *params, const void *partials, void *value, void *grad) {
  if (!c || !params || !partials || !value || !grad) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_finalize")) return rs;
  (void)hipSetDevice(c->cfg.device);
  launch_finalize(c, params, partials, value, grad);
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}


