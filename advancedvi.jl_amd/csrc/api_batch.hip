// libmivi C ABI, part 5: estimates at FIXED parameters -- hipGraph chains, the lane-batched second-generation kernels and the
// third-generation batch engine (kernels_fullrank_batch.hip): mivi_estimate_gradient_n / _each.
#include "api_common.h"

bool graph_capturable(const mivi_ctx *c) {   // every device-resident target (the host callback is not)
  return c->target == TGT_DIAG_GAUSS || c->target == TGT_DENSE_GAUSS || c->target == TGT_FUNNEL || c->target == TGT_LOGREG;
}
// allocations are not allowed inside a capture: size whatever the target's launchers would otherwise grow lazily
mivi_status_t reserve_target(mivi_ctx *c, int M) {
  if (c->target == TGT_LOGREG && !logreg_reserve(c, M)) return fail(c, MIVI_ERR_HIP, "logistic regression: scratch allocation failed");
  return MIVI_OK;
}

// `cnt` chained estimates of context k at fixed parameters: indices first, first + stride, ... -- by value (idx_ptr = nullptr: an eager
// chain) or relative to the device-side counter *idx_ptr (a recording).  Every estimate but the last writes its result where the last one
// does; the chain's closing value launch is flush_chain's.
// The eps speculation is off afterwards.  (run_estimate clears c->pre on entry and sets it only on its `spec` branches, which a
// chained gradient estimate never takes: the second-generation route has spec = !chained, and the first-generation route is chained
// exactly when hetero_ok holds, which spec needs too.  So the flag can only have survived an estimate that failed before it got there.)
static mivi_status_t record_chain(mivi_ctx *k, const void *params, uint64_t first, uint64_t stride, int cnt, const uint64_t *idx_ptr, void *value,
                                  void *grad) {
  Chain chn;
  chn.on = true;
  chn.estimates_only = true;
  mivi_status_t s = MIVI_OK;
  for (int i = 0; i < cnt && s == MIVI_OK; ++i) {
    RngArgs r = rng_of(k, first + (uint64_t)i * stride);
    if (idx_ptr) r.idx_ptr = idx_ptr;
    k->cur = i & 1;
    chn.has_next = (i + 1 < cnt);
    chn.next_rng = rng_of(k, first + ((uint64_t)i + 1) * stride);
    chn.next_rng.idx_ptr = r.idx_ptr;
    s = run_estimate(k, params, r, k->cfg.n_mc, 1, final_out(k, value, grad), &chn);
  }
  if (s == MIVI_OK) flush_chain(k, params, &chn);
  k->cur = 0;
  k->pre.clear();
  return s;
}

static mivi_status_t estimate_gradient_chain(mivi_ctx *c, const void *params, uint64_t idx0, int32_t count, void *value, void *grad) {
  if (!c || !params || !value || !grad || count <= 0) return MIVI_ERR_BAD_ARG;
  const uint64_t st = (uint64_t)c->idx_stride;   // estimates idx0, idx0 + st, ... (st = 1 unless this is one of several interleaved chains)
  if (!graph_capturable(c)) return fail(c, MIVI_ERR_UNSUPPORTED, "graph batching needs a device-resident built-in target");
  if (c->idx_src) return fail(c, MIVI_ERR_UNSUPPORTED, "an index source is set (mivi_set_index_source): graph-batched calls keep their own device counter");
  (void)hipSetDevice(c->cfg.device);
  mivi_status_t s = ensure_work(c, c->cfg.n_mc);
  if (s) return s;
  if (!prepare_tables(c, c->cfg.n_mc)) return fail(c, MIVI_ERR_HIP, "full-rank work tables: allocation or upload failed");   // host->device uploads are not allowed inside the capture
  if ((s = reserve_target(c, c->cfg.n_mc))) return s;
  if (mf_diag_loop_ok(c) && !c->idx_src && !switches().no_fused_loop) {
    // rows are independent for this family / target pair: all `count` estimates run inside ONE launch (every workgroup
    // keeps its four rows and walks the estimate indices), the value partials are reduced by a second launch
    if ((s = ensure(c, c->X, mf_est_loop_scratch_doubles(c, count) * sizeof(double), false))) return s;
    const MfEstScratch w = mf_est_loop_carve(c, c->X.p, count);
    launch_mf_sgd_loop(c, const_cast<void *>(params), nullptr, idx0, 0, count, -1, 0.0, (double)NAN, w.hist, w.elbo, grad, w.lanes,
                       value);   // (the value kernel also leaves the last estimate's objective value: no launch of its own)
    HIPCHK(c, hipGetLastError());
    return MIVI_OK;
  }
  if (mf_funnel_loop_ok(c) && !c->idx_src && !switches().no_fused_loop) {
    // fused funnel target (BASELINE config 5): the cross-row sums enter row 0 and ell linearly, so the batch is launch-free too --
    // per-estimate partials to a history buffer, one finishing workgroup per estimate (k_mf_funnel_loop / _value)
    if ((s = ensure(c, c->X, mf_funnel_loop_scratch_doubles(c, count) * sizeof(double), false))) return s;
    const MfEstScratch w = mf_funnel_loop_carve(c, c->X.p, count);
    launch_mf_funnel_loop(c, params, idx0, count, w.hist, w.elbo, w.sc, value, grad, w.lanes, w.e0);
    HIPCHK(c, hipGetLastError());
    return MIVI_OK;
  }
  // The shortest batches run as an eager chain of the same launches: a graph replay carries ~25 us of fixed host cost (and its first
  // use a capture + instantiation), an eager chain ~17 us but ~0.7 us more per estimate (north star, n = 1 / 5 / 10 / 20 estimates
  // done after 31 / 93 / 168 / 314 us eagerly against 39 / 97 / 166 / 301 us replayed).  MIVI_GRAPH_MIN pins the
  // smallest batch that is captured.
  if (count < switches().graph_min && c->cfg.family == MIVI_FULLRANK) {
    if ((s = record_chain(c, params, idx0, st, count, nullptr, value, grad))) return s;
    HIPCHK(c, hipGetLastError());
    return MIVI_OK;
  }
  const GraphKey key{GRAPH_CHAIN, count, params, value, grad};
  if (!c->graph.matches(key)) {
    invalidate_graph(c);
    s = graph_record(c, key, [&]() -> mivi_status_t {
      const mivi_status_t rs = record_chain(c, params, 0, st, count, (const uint64_t *)c->d_idx.p, value, grad);
      if (rs == MIVI_OK) hipLaunchKernelGGL(k_bump_u64, dim3(1), dim3(1), 0, c->stream, (uint64_t *)c->d_idx.p, (uint64_t)count * st);
      return rs;
    });
    if (s) return s;
  }
  return graph_replay(c, idx0, (uint64_t)count * st);
}

// ---- interleaved chains ------------------------------------------------------------------------------------------------------------
mivi_status_t sync_kid(mivi_ctx *c, mivi_ctx *k, int lanes) {
  if (k->kid_gen == c->target_gen && k->idx_stride == lanes) return MIVI_OK;
  invalidate_graph(k);
  k->target = c->target;
  k->t_const = c->t_const;
  k->t_mean.borrow(c->t_mean.p, c->t_mean.bytes); k->t_istd.borrow(c->t_istd.p, c->t_istd.bytes); k->t_prec.borrow(c->t_prec.p, c->t_prec.bytes);   // views of the parent's target, re-taken whenever its generation moves
  k->M_total = c->M_total;
  if (k->target == TGT_DENSE_GAUSS && !k->RT.p) k->cap_M = 0;              // (allocates its own transposed-sample buffer)
  k->idx_stride = lanes;
  k->kid_gen = c->target_gen;
  return MIVI_OK;
}

// children of an interleaved / lane-batched batch: the same configuration, their own stream and work buffers, the target borrowed
mivi_status_t ensure_kids(mivi_ctx *c, int lanes) {
  mivi_status_t s;
  while (c->n_kids < lanes - 1) {
    mivi_config_t cfg = c->cfg;
    cfg.stream = nullptr;
    cfg.own_stream = 1;
    mivi_ctx *k = nullptr;
    if ((s = mivi_create(&cfg, &k))) return fail(c, s, "interleaved chains: child context creation failed");
    k->is_child = true;
    const int j = c->n_kids;
    k->status.borrow((char *)c->status.p + sizeof(int) * (j + 1), sizeof(int));   // the child's sticky flags: word j + 1 of the parent's status buffer
    if ((s = ensure(c, c->kid_out[j], 16 + (size_t)mivi_params_len(c) * c->esize, false)) || (s = make_event(c, c->ev_join[j], false)) ||
        (!c->ev_fork && (s = make_event(c, c->ev_fork, false)))) {
      (void)mivi_destroy(k);   // (not yet registered with the parent: nobody else would)
      return s;
    }
    c->kids[c->n_kids++] = k;
  }
  return MIVI_OK;
}

// On a cache miss, before a recording that spans the children: invalidate_graph has just bumped the generation the children were synced
// to (sync_kid), so re-stamp it; and their streams carry their table uploads, which have to be done before the capture (not on every replay).
mivi_status_t kids_before_capture(mivi_ctx *c, int lanes) {
  for (int j = 0; j < lanes - 1; ++j) {
    c->kids[j]->kid_gen = c->target_gen;
    HIPCHK(c, hipStreamSynchronize(c->kids[j]->stream));
  }
  return MIVI_OK;
}

// The fork / join of a recording with B parallel branches (at most four: see kMaxKids): branch 0 is the context's own stream; branch b > 0
// runs on the stream of child b E - 1, which joins the capture behind ONE fork event and is joined back through its own event.  The
// recording closes by advancing the device-side estimate counter by `count`.
template <class Branch> static mivi_status_t record_branches(mivi_ctx *c, int B, int E, int count, Branch &branch) {
  mivi_status_t s = MIVI_OK;
  hipError_t he = hipEventRecord(c->ev_fork.get(), c->stream);
  for (int b = 1; b < B && s == MIVI_OK && he == hipSuccess; ++b) {
    hipStream_t bs = c->kids[b * E - 1]->stream;
    he = hipStreamWaitEvent(bs, c->ev_fork.get(), 0);   // the branch's stream joins the capture
    if (he != hipSuccess) break;
    s = branch(b);
    if (s == MIVI_OK) he = hipEventRecord(c->ev_join[b * E - 1].get(), bs);
  }
  if (s == MIVI_OK && he == hipSuccess) s = branch(0);
  for (int b = 1; b < B && s == MIVI_OK && he == hipSuccess; ++b) he = hipStreamWaitEvent(c->stream, c->ev_join[b * E - 1].get(), 0);
  if (s == MIVI_OK && he == hipSuccess) hipLaunchKernelGGL(k_bump_u64, dim3(1), dim3(1), 0, c->stream, (uint64_t *)c->d_idx.p, (uint64_t)count);
  if (s) return s;
  HIPCHK(c, he);
  return MIVI_OK;
}

// ---- third-generation batch engine (kernels_fullrank_batch.hip) -------------------------------------------------------------------------
// `count` estimates at the same parameters as steps of up to switches().fb_lanes LANES: a step is four launches (eps, product + target, VJP,
// values) that cover all of its lanes.  No child contexts, no forked graph: a lane's buffers are base + lane * stride.
// MIVI_FB_LANES: estimates per step (A/B).  Per estimate (eps + product + VJP, tools/fb_lane_curve.py, north-star shape): 8 lanes 8.4 us,
// 20: 4.6, 32: 4.05, 48: 3.95, 80: 3.90, 100: 4.05, 128: 4.11 -- the triangular product is paced by its heaviest tile up to ~30 lanes, and
// beyond ~90 the step's planes (4.5 MB per lane) outgrow the 256 MB memory-side cache (the draws' writes slow down first).  So long batches
// are cut into equal steps of at most 80 lanes (100 estimates: two steps of 50).
// MIVI_FB_STL=0: the sticking-the-landing estimators keep the lane-batched second-generation kernels + solves (A/B).
static bool fb_route(const mivi_ctx *c, const void *params, const void *grad_last, const void *grads_all) {
  const bool stl = stl_entropy(c);
  return !c->is_child && c->base == MIVI_BASE_NORMAL && c->cfg.family == MIVI_FULLRANK && c->cfg.dtype == MIVI_F32 && !c->bij_on && !c->idx_src && !c->dbg &&
         (c->target == TGT_DIAG_GAUSS || c->target == TGT_DENSE_GAUSS) && (!stl || (switches().fb_stl && stl2_shape_ok(c, c->cfg.d))) &&
         fb_shape_ok(c, c->cfg.n_mc) && ((!stl && c->target == TGT_DIAG_GAUSS) || fb_whole_tiles(c, c->cfg.n_mc)) &&   // (padded geometry: the diagonal target, no STL term)
         ((uintptr_t)params & 15) == 0 && ((uintptr_t)grad_last & 15) == 0 && ((uintptr_t)grads_all & 15) == 0;
}
// value_last / grad_last: the batch's LAST estimate (mivi_estimate_gradient_n's contract), or nullptr; values_all T[count] / grads_all
// T[count * params_len]: every estimate's (mivi_estimate_gradient_each), or nullptr (lane scratch)
// obj_ent >= 0: objective mode (fb_objective): the `count` lanes are consecutive blocks of n_mc samples of estimate idx0, values only, the
// value's entropy estimator obj_ent
// dist: a SHARDED batch (mivi_estimate_gradient_dist_n on an engine shape): this context draws its n_mc columns of every estimate's n_mc x world
// samples; the VJP launch leaves the lanes' partial vectors, ONE all-reduce per step sums them over the ranks (dist_allreduce_f32: nothing
// to do on one rank), k_fb_finalize_parts turns the sums into the lanes' values and gradients.
static mivi_status_t fb_batch(mivi_ctx *c, const void *params, uint64_t idx0, int count, void *value_last, void *grad_last, void *values_all,
                              void *grads_all, int obj_ent = -1, bool dist = false) {
  mivi_status_t s;
  const int M = c->cfg.n_mc, d = c->cfg.d;
  if ((s = ensure_work(c, M))) return s;
  // sharded batches with a communicator: steps of at most 24 lanes, so that a 100-estimate call is five steps whose all-reduces (on
  // fb_pipe.stream, the partial vectors double-buffered) run UNDER the next steps' kernels -- across ranks the exchange, not the kernels, paces
  // the batch
  const bool overlap = dist && c->comm != nullptr;
  const int Lmax = (overlap && c->comm_world > 1) ? (switches().fb_lanes < 24 ? switches().fb_lanes : 24) : switches().fb_lanes;   // (one rank: nothing to hide, the widest steps)
  const int steps = (count + Lmax - 1) / Lmax, L = (count + steps - 1) / steps, Llast = count - (steps - 1) * L;
  if (overlap && (s = ensure_pipe(c, c->fb_pipe, false))) return s;
  const size_t plen = (size_t)mivi_params_len(c);
  const int dG = (d + 127) / 128 * 128, MG = (M + 127) / 128 * 128;   // the engine's geometry: whole 128 x 128 tiles (kernels_fullrank_batch.hip fb_pad)
  FbTables &t = c->fb;
  if (t.cap_L < L || t.cap_M != M) {
    invalidate_graph(c);
    const size_t pw = fb_plane_words(c, M) * 4;
    if ((s = ensure(c, t.CA, fb_cplane_words(c) * 4, false)) || (s = ensure(c, t.epsP, (size_t)L * pw, false)) ||
        (s = ensure(c, t.WV, (size_t)L * pw, false)) ||
        (s = ensure(c, t.ell, (size_t)L * (dG / 32) * (MG / 32) * sizeof(double), false)) ||
        (s = ensure(c, t.he, (size_t)L * (dG / 64) * (MG / 32) * sizeof(double), false)) ||
        (s = ensure(c, t.ld, 2 * (size_t)(dG / 32) * sizeof(double) + 64, false)) || (s = ensure(c, t.values, (size_t)L * 4 + 64, false)) ||
        (s = ensure(c, t.cscale, 2 * (size_t)dG * 4, false)) || (s = ensure(c, t.winv, (size_t)L * (MG / 128) * dG * 4, false)))
      return s;
    if ((s = ensure_zeroed(c, t.grads, (size_t)L * plen * 4))) return s;   // (the lanes' scratch gradients rely on exact zeros above the diagonal that no kernel writes)
    t.cap_L = L;
    t.cap_M = M;
    t.cap_LR = 0;
  }
  const size_t part_len = dist ? fb_part_len(c) : 0;
  if (dist && t.cap_LP < L) {
    invalidate_graph(c);
    if ((s = ensure(c, t.parts, 2 * (size_t)L * part_len * 4, false))) return s;   // (two sets: the all-reduce of step s under the kernels of step s + 1)
    t.cap_LP = L;
  }
  const bool dense = c->target == TGT_DENSE_GAUSS;
  if (dense) {   // R = Z - m planes per lane; the planes of P once per target
    if (t.cap_LR < L) {
      invalidate_graph(c);
      if ((s = ensure(c, t.RP, (size_t)L * fb_plane_words(c, M) * 4, false)) || (s = ensure(c, t.PA, fb_cplane_words(c) * 4, false)) ||
          (s = ensure(c, t.pscale, 2 * (size_t)d * 4, false)) || (s = ensure(c, t.rinv, (size_t)L * (d / 128) * M * 4, false)))
        return s;
      t.cap_LR = L;
      t.PA_valid = false;
    }
    if (!t.PA_valid) {
      fb_launch_pplanes(c, c->stream);
      t.PA_valid = true;
    }
  }
  const bool values_only = obj_ent >= 0 || (!grads_all && !grad_last);
  const bool stl = !values_only && stl_entropy(c);   // (a value needs no gradient term)
  if (stl) {
    // W += C^-T eps: inside a call the parameters are fixed, so C^-T is formed ONCE -- the solve kernels (kernels_stl.hip) on the identity's d
    // columns -- and the term is one more triangular product per lane (k_fb_prod<FB_STL_U>)
    const size_t es = 4;
    if (!t.Eye.p) {
      std::vector<float> eye((size_t)d * d, 0.f);
      for (int i = 0; i < d; ++i) eye[(size_t)i * d + i] = 1.f;
      if ((s = ensure(c, t.Eye, (size_t)d * d * es, false))) return s;
      HIPCHK(c, hipMemcpy(t.Eye.p, eye.data(), (size_t)d * d * es, hipMemcpyHostToDevice));
    }
    const bool grow = !t.Tinv.p || c->stl_X.bytes < ((size_t)d * d + (size_t)(d / 2) * (d / 2)) * es + 4096 || !c->stl_F.p;
    if (grow) {
      invalidate_graph(c);
      if ((s = ensure(c, t.Tinv, (size_t)d * d * es, false)) || (s = ensure(c, t.TA, fb_cplane_words(c) * 4, false)) || (s = ensure(c, t.tscale, 2 * (size_t)d * 4, false)) ||
          (s = ensure(c, c->stl_X, ((size_t)d * d + (size_t)(d / 2) * (d / 2)) * es + 4096, false)) ||
          (s = ensure(c, c->stl_F, mivi::stl_pack_units(d) * 4, false)))
        return s;
    }
    launch_stl2(c, params, d, false, t.Eye.p, t.Tinv.p, true);
    fb_launch_tplanes(c, c->stream);
  }
  const FbTab *tabF = fb_prepare(c, M, L), *tabL = Llast != L ? fb_prepare(c, M, Llast) : tabF;
  if (Llast != L) tabF = fb_prepare(c, M, L);   // (re-resolve: four table slots, round robin)
  if (!tabF || !tabL) return fail(c, MIVI_ERR_HIP, "batch engine: work table allocation failed");
  auto make_step = [&](int st) {
    FbStep fs{};
    fs.params = params;
    fs.M = M;
    fs.L = st == steps - 1 ? Llast : L;
    fs.tab = st == steps - 1 ? tabL : tabF;
    fs.rng = rng_of(c, obj_ent >= 0 ? idx0 : idx0 + (uint64_t)st * L);
    fs.obj = obj_ent >= 0 ? 1 : 0;
    fs.ent_kind = obj_ent;
    fs.values_only = values_only ? 1 : 0;
    if (obj_ent >= 0) fs.rng.m_offset += st * L * M;
    if (grads_all) { fs.grads = (char *)grads_all + (size_t)st * L * plen * 4; fs.grad_stride = (long long)plen; fs.write_upper = 1; }
    else { fs.grads = t.grads.p; fs.grad_stride = (long long)plen; fs.write_upper = 0; }
    if (values_all) { fs.values = (char *)values_all + (size_t)st * L * 4; fs.value_stride = 1; }
    else { fs.values = t.values.p; fs.value_stride = 1; }
    fs.lane_last = -1;
    fs.dense = dense ? 1 : 0;
    fs.stl = stl ? 1 : 0;
    if (st == steps - 1 && (value_last || grad_last)) { fs.lane_last = Llast - 1; fs.grad_last = grad_last; fs.value_last = value_last; }
    if (dist) { fs.parts = (char *)t.parts.p + (size_t)(overlap ? (st & 1) : 0) * (size_t)t.cap_LP * part_len * 4; fs.part_stride = (long long)part_len; }
    return fs;
  };
  // One stream, no graph: per step {draws (+ tril(C)'s planes as riders of the first) -> product -> VJP + values} = three launches for up to
  // switches().fb_lanes estimates; the host is far ahead of the device.  (Measured and dropped: the batch as ONE hipGraph -- 4.45 against 4.26 us
  // per estimate in 100-estimate batches -- and the draws of step s + 1 on a second graph branch beside the products of step s: the draws
  // are bound by their 3 MB of plane writes per estimate and by the vector ALU, beside them the products ran 25 % longer: 4.58 us.)
  ExchangePipe &pipe = c->fb_pipe;
  int handed = 0;   // steps handed over to the pipe's stream so far
  auto step = [&](int st) -> mivi_status_t {
    const FbStep fs = make_step(st);
    if (overlap && (s = pipe.reuse(c, c->stream, st))) return s;   // the finalisation of step st - 2 has read this set of partial vectors
    fb_launch_eps(c, fs, st == 0, c->stream);
    fb_launch_compute(c, fs, c->stream);
    if (!dist) return MIVI_OK;
    hipStream_t xs = c->stream;
    if (overlap) {
      if ((s = pipe.hand_over(c, c->stream, st, &xs))) return s;
      handed = st + 1;
    }
    if ((s = dist_allreduce_f32(c, fs.parts, (size_t)fs.L * part_len, xs))) return s;
    fb_launch_finalize_parts(c, fs, xs);
    return overlap ? pipe.finish(c, st) : MIVI_OK;
  };
  s = MIVI_OK;
  for (int st = 0; st < steps && s == MIVI_OK; ++st) s = step(st);
  if (s) {
    pipe.join_after_error(c->stream, handed);
    return s;
  }
  if (overlap && (s = pipe.join(c, c->stream, steps))) return s;   // the batch is complete when its last two exchanges + finalisations are
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

mivi_status_t mivi::fb_objective(mivi_ctx *c, const void *params, uint64_t idx, int lanes, int entropy, void *values) {
  if (!fb_route(c, params, nullptr, nullptr) || c->M_total != c->cfg.n_mc) return MIVI_ERR_UNSUPPORTED;
  return fb_batch(c, params, idx, lanes, nullptr, nullptr, values, nullptr, entropy);
}

// Lanes per step of a `count`-estimate batch on the batch engine (equal steps of at most MIVI_FB_LANES = 80): what a roofline leg must profile.
int32_t mivi_batch_lanes(const mivi_ctx_t *c, int32_t count) {
  if (!c || count <= 0) return 0;
  const int Lmax = switches().fb_lanes, steps = (count + Lmax - 1) / Lmax;
  return (count + steps - 1) / steps;
}

int32_t mivi_batch_info(const mivi_ctx_t *c, const void *params, int32_t what) {
  if (!c) return 0;
  if (what == 1) return 3;   // fr_planes.h kSplitProducts
  if (what == 2) return 4;   // two f16 planes
  if (what == 3) return c->exchange_lost ? 1 : 0;
  if (what == 4) return c->graph_records;
  if (what == 5) return live_allocations();
  if (what == 6) return live_handles();
  if (what == 7) return c->last_loop;
  return (what == 0 && params && fb_route(c, params, nullptr, nullptr)) ? 1 : 0;
}

// Roofline leg of the batch engine: `reps` launches of each of a step's kernels for `lanes` estimates, hipEvents on the context's
// stream.  us_out[0..4] = average launch duration (us) of the draws, the product (+ fused diagonal target), the VJP (+ values), the dense
// target's product (0 with the diagonal target), the sticking-the-landing product (0 with the other estimators).
mivi_status_t mivi_profile_batch(mivi_ctx_t *c, const void *params, int32_t lanes, int32_t reps, double *us_out) {
  if (!c || !params || lanes <= 0 || reps <= 0 || !us_out) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_non_gaussian(c, "mivi_profile_batch")) return rs;
  (void)hipSetDevice(c->cfg.device);
  if (!fb_route(c, params, nullptr, nullptr)) return fail(c, MIVI_ERR_UNSUPPORTED, "mivi_profile_batch: this configuration does not take the batch engine");
  if (lanes > switches().fb_lanes) lanes = switches().fb_lanes;
  char *o = (char *)c->tmp_out.p;
  mivi_status_t s = fb_batch(c, params, 1, lanes, o, o + 16, nullptr, nullptr);   // buffers, tables, operand planes of every lane
  if (s) return s;
  const FbTab *tab = fb_prepare(c, c->cfg.n_mc, lanes);
  if (!tab) return fail(c, MIVI_ERR_HIP, "batch engine: work table allocation failed");
  FbStep fs{};
  fs.params = params; fs.M = c->cfg.n_mc; fs.L = lanes; fs.tab = tab;
  fs.rng = rng_of(c, 1);
  fs.grads = c->fb.grads.p; fs.grad_stride = (long long)mivi_params_len(c); fs.values = c->fb.values.p; fs.value_stride = 1; fs.lane_last = -1;
  fs.dense = c->target == TGT_DENSE_GAUSS ? 1 : 0;
  fs.stl = stl_entropy(c) ? 1 : 0;
  us_out[3] = us_out[4] = 0.0;
  EventTimer timer;
  for (int which = 0; which < 5; ++which) {
    if ((which == 3 && !fs.dense) || (which == 4 && !fs.stl)) continue;
    for (int r = -2; r < reps; ++r) {
      if (r == 0 && (s = timer.start(c, c->stream))) return s;
      if (which == 0) fb_launch_eps(c, fs, true, c->stream);
      else fb_launch_compute(c, fs, c->stream, which == 1 ? 1 : (which == 2 ? 2 : (which == 3 ? 4 : 8)));
    }
    double us = 0.0;
    if ((s = timer.stop_us(c, c->stream, &us))) return s;
    us_out[which] = us / reps;
  }
  HIPCHK(c, hipGetLastError());
  return MIVI_OK;
}

// mivi_estimate_gradient_dist_n on a batch-engine shape (api_dist.hip decides): every rank runs the engine on ITS sample columns, the lanes'
// partial vectors cross the ranks in one all-reduce per step
bool fb_dist_route(const mivi_ctx *c, const void *params, const void *grad) { return fb_route(c, params, grad, nullptr) && fb_whole_tiles(c, c->cfg.n_mc); }
mivi_status_t fb_batch_dist(mivi_ctx *c, const void *params, uint64_t idx0, int count, void *value, void *grad) {
  return fb_batch(c, params, idx0, count, value, grad, nullptr, nullptr, -1, true);
}

mivi_status_t mivi_estimate_gradient_each(mivi_ctx_t *c, const void *params, uint64_t idx0, int32_t count, void *values, void *grads) {
  if (!c || !params || !values || count <= 0) return MIVI_ERR_BAD_ARG;
  (void)hipSetDevice(c->cfg.device);
  if (c->target == TGT_NONE) return fail(c, MIVI_ERR_NO_TARGET, "no target set");
  if (fb_route(c, params, nullptr, grads)) return fb_batch(c, params, idx0, count, nullptr, nullptr, values, grads);
  // every other configuration: the single calls, one after the other (results are those of mivi_estimate_gradient by definition)
  const size_t plen = (size_t)mivi_params_len(c);
  mivi_status_t s = MIVI_OK;
  for (int i = 0; i < count && s == MIVI_OK; ++i)
    s = run_estimate(c, params, rng_of(c, idx0 + (uint64_t)i), c->cfg.n_mc, 1,
                     final_out(c, (char *)values + (size_t)i * c->esize, grads ? (void *)((char *)grads + (size_t)i * plen * c->esize) : c->tmp_out.p));
  return s;
}

// How mivi_estimate_gradient_n deals a batch that the engine does not take onto contexts (it only reads the context).
struct LanePlan {
  int lanes = 1;        // contexts: 1 = a single chain on the context itself
  int per_branch = 0;   // 0: forked chains, every context on a graph branch of its own; E > 0: lanes / E branches of E lane-batched contexts
};
static LanePlan lane_plan(const mivi_ctx *c, const void *params, const void *grad, int count) {
  // Several interleaved chains pay when an estimate is a short chain of latency-bound launches (the second-generation full-rank
  // kernels at the BASELINE sizes: two launches of 6-8 us that leave most CUs idle half of the time).  One chain otherwise.
  int lanes = 1;
  if (!c->is_child && c->cfg.family == MIVI_FULLRANK && c->cfg.dtype == MIVI_F32 && !c->bij_on && !c->idx_src && !c->dbg &&
      (c->target == TGT_DIAG_GAUSS || c->target == TGT_DENSE_GAUSS) && lds_path_shape_ok(c, c->cfg.n_mc) &&
      (long long)c->cfg.d * c->cfg.n_mc <= 2048LL * 512)
    lanes = 4;   // (measured at the north star, us per estimate with 1 / 2 / 3 / 4 chains: isolated 20-estimate calls 14.4 / 13.9 / 13.3 / 10.8,
                 //  100-estimate calls back to back 13.4 / 9.7 / 8.9 / 8.1 -- the product kernel's 64 KiB of LDS lets two of them, or one and
                 //  a VJP workgroup, share a CU)
  // Without a sticking-the-landing solve between the two kernels the contexts are LANE-BATCHED: E = 4 contexts per graph branch whose
  // product kernels are ONE launch (blockIdx.y = lane) and so are their VJP kernels -- half the launches per estimate, no fork / join for a
  // short batch (4 contexts, one branch: isolated 20-estimate calls 10.6 -> 9.7 us per estimate), two branches of four from twelve estimates on
  // (since the lane-batched launches are kernels of their own -- k_fr_prod32q, k_fr_vjp32s: one product + one VJP workgroup fit a CU -- the second
  // branch pays for 20-estimate calls too: 9.0 -> 8.1 us; 100-estimate calls back to back 7.0 us; 8, 12 and 16 contexts agree there).
  // MIVI_LANE_BATCH=0 keeps every context on a branch of its own (A/B reference; the STL estimators do where their solve is not the
  // second-generation one); MIVI_CHAINS = contexts.
  const int lane_env = switches().lane_batch, chains = switches().chains;
  int lane_e = 0;   // contexts per branch (0: one each)
  if (lanes > 1 && (!stl_entropy(c) || stl2_shape_ok(c, c->cfg.n_mc)) && lds_use_prod32(c, c->cfg.n_mc) && ((uintptr_t)params & 15) == 0 &&
      ((uintptr_t)grad & 15) == 0 && lane_env != 0) {
    lane_e = lane_env > 0 ? (lane_env > 4 ? 4 : lane_env) : 4;
    lanes = count < 12 ? 4 : 8;   // (isolated batches at the north star, 4 vs 8 contexts, us per estimate: 8: 10.8 / 10.4, 10: 11.0 / 11.5, 12: 9.9 / 9.4, 20: 9.1 / 8.1, 48: 8.3 / 7.2)
  }
  if (chains > 0) lanes = c->is_child ? 1 : (chains > mivi_ctx::kMaxKids + 1 ? mivi_ctx::kMaxKids + 1 : chains);
  if (lane_e > 0 && (lanes % lane_e != 0 || count < lanes)) lane_e = 0;
  if (lane_e <= 0 && lanes > 4) lanes = 4;          // (as graph BRANCHES: at most four -- see kMaxKids)
  if (lane_e > 0 && lanes / lane_e > 4) lanes = 4 * lane_e;
  while (lanes > 1 && count < 4 * lanes && lane_e <= 0) --lanes;   // (short batches: not worth the fork / join)
  LanePlan plan;
  plan.lanes = lanes;
  plan.per_branch = lanes > 1 ? lane_e : 0;
  return plan;
}

// Branch b of a lane-batched recording: contexts ctxs[b E .. b E + E) of `lanes` (global lane g serves estimates g, g + lanes, ... relative to
// ONE device counter, the parent's), their launches on the stream of the branch's first context.  Its product kernels are ONE launch per
// step (blockIdx.y = lane), and so are its first draws, STL terms, VJP kernels and the chains' closing value kernels.  The chain that holds
// the batch's LAST estimate writes the caller's buffers, the others their scratch.
static mivi_status_t record_lane_branch(mivi_ctx *c, mivi_ctx *const *ctxs, int b, int E, int lanes, const void *params, int count, void *value,
                                        void *grad) {
  mivi_ctx *const *lane = ctxs + b * E;
  const int q_last = (count - 1) % lanes;
  LaneRecorder rec(E, stl_entropy(c));
  LaneScope scope(lane, E, &rec, lane[0]->stream);
  Chain chn[4];
  for (int l = 0; l < E; ++l) { chn[l].on = true; chn[l].estimates_only = true; }
  auto n_of = [&](int gl) { return (count - gl + lanes - 1) / lanes; };   // estimates of global lane gl: gl, gl + lanes, ...
  mivi_status_t st = MIVI_OK;
  const int steps = (count + lanes - 1) / lanes;
  for (int i = 0; i < steps && st == MIVI_OK; ++i) {
    int L = 0;
    while (L < E && i < n_of(b * E + L)) ++L;
    st = lanes_step(c, lane, rec, L, i == 0, [&](int l) {
      const int gl = b * E + l;
      mivi_ctx *k = lane[l];
      RngArgs r = rng_of(k, (uint64_t)gl + (uint64_t)i * lanes);
      r.idx_ptr = (const uint64_t *)c->d_idx.p;
      k->cur = i & 1;
      chn[l].has_next = (i + 1 < n_of(gl));
      chn[l].next_rng = rng_of(k, (uint64_t)gl + ((uint64_t)i + 1) * lanes);
      chn[l].next_rng.idx_ptr = r.idx_ptr;
      char *ko = gl ? (char *)c->kid_out[gl - 1].p : (char *)c->tmp_out.p;
      return run_estimate(k, params, r, k->cfg.n_mc, 1, final_out(k, gl == q_last ? value : (void *)ko, gl == q_last ? grad : (void *)(ko + 16)), &chn[l]);
    });
  }
  rec.closing = true;   // the lanes' closing value kernels (the last estimate of every chain): one launch, before the scope gives the streams back
  for (int l = 0; l < E && st == MIVI_OK; ++l) flush_chain(lane[l], params, &chn[l]);
  if (st == MIVI_OK) launch_lanes_value(lane[0], params, rec);
  return st;
}

mivi_status_t mivi_estimate_gradient_n(mivi_ctx_t *c, const void *params, uint64_t idx0, int32_t count, void *value, void *grad) {
  if (!c || !params || !value || !grad || count <= 0) return MIVI_ERR_BAD_ARG;
  (void)hipSetDevice(c->cfg.device);
  if (c->cfg.family == MIVI_LOWRANK || is_flow(c) || c->base != MIVI_BASE_NORMAL) {   // the single calls, one after the other: no lanes, no child contexts, no engine, no graph
    mivi_status_t sl = MIVI_OK;
    for (int i = 0; i < count && sl == MIVI_OK; ++i) sl = run_estimate(c, params, rng_of(c, idx0 + (uint64_t)i), c->cfg.n_mc, 1, final_out(c, value, grad));
    return sl;
  }
  if (count >= 2 && fb_route(c, params, grad, nullptr)) return fb_batch(c, params, idx0, count, value, grad, nullptr, nullptr);
  const LanePlan plan = lane_plan(c, params, grad, count);
  const int lanes = plan.lanes;
  if (lanes <= 1) {
    if (!c->is_child && c->idx_stride != 1) { invalidate_graph(c); c->idx_stride = 1; }
    return estimate_gradient_chain(c, params, idx0, count, value, grad);
  }
  mivi_status_t s;
  if ((s = ensure_kids(c, lanes))) return s;
  if (c->idx_stride != lanes) { invalidate_graph(c); c->idx_stride = lanes; }
  for (int j = 0; j < lanes - 1; ++j)
    if ((s = sync_kid(c, c->kids[j], lanes))) return s;
  // chain q serves estimates idx0 + q, idx0 + q + lanes, ...; the chain that holds the LAST estimate writes the caller's buffers.
  // ONE hipGraph for the whole batch: the children's streams join the capture behind one fork event, so the batch is one graph
  // launch with `lanes` parallel branches and one join (two graph launches + events per call cost a 20-estimate batch what the
  // overlap gained: 14.7 us per estimate against 14.4 with one chain, 9.7 in steady state).
  if ((s = ensure_work(c, c->cfg.n_mc))) return s;
  if (!prepare_tables(c, c->cfg.n_mc)) return fail(c, MIVI_ERR_HIP, "full-rank work tables: allocation or upload failed");
  for (int j = 0; j < lanes - 1; ++j) {
    mivi_ctx *k = c->kids[j];
    if ((s = ensure_work(k, k->cfg.n_mc))) { c->err = k->err; return s; }
    if (!prepare_tables(k, k->cfg.n_mc)) return fail(c, MIVI_ERR_HIP, "full-rank work tables: allocation or upload failed");
    if (!lds_prepare(k, k->cfg.n_mc)) return fail(c, MIVI_ERR_HIP, "full-rank work lists: allocation failed");
  }
  if (!lds_prepare(c, c->cfg.n_mc)) return fail(c, MIVI_ERR_HIP, "full-rank work lists: allocation failed");
  if (plan.per_branch > 0) {   // LANE-BATCHED contexts (record_lane_branch)
    const int E = plan.per_branch, B = lanes / E;
    GraphKey key{GRAPH_LANE_BRANCHES, count, params, value, grad};
    key.lanes = lanes;
    key.per_branch = E;
    if (!c->graph.matches(key)) {
      invalidate_graph(c);
      if ((s = kids_before_capture(c, lanes))) return s;
      mivi_ctx *ctxs[1 + mivi_ctx::kMaxKids];
      ctxs[0] = c;
      for (int l = 1; l < lanes; ++l) ctxs[l] = c->kids[l - 1];
      auto branch = [&](int b) { return record_lane_branch(c, ctxs, b, E, lanes, params, count, value, grad); };
      if ((s = graph_record(c, key, [&]() { return record_branches(c, B, E, count, branch); }))) return s;
    }
    return graph_replay(c, idx0, (uint64_t)count);
  }
  GraphKey key{GRAPH_FORKED_CHAINS, count, params, value, grad};
  key.lanes = lanes;
  if (!c->graph.matches(key)) {
    invalidate_graph(c);
    if ((s = kids_before_capture(c, lanes))) return s;
    const int q_last = (count - 1) % lanes;
    auto chain = [&](int q) -> mivi_status_t {   // chain q: this context (q = 0) or child q - 1, estimates q, q + lanes, ... relative to ONE device counter (the parent's)
      mivi_ctx *k = q ? c->kids[q - 1] : c;
      char *ko = q ? (char *)c->kid_out[q - 1].p : (char *)c->tmp_out.p;
      const mivi_status_t cs = record_chain(k, params, (uint64_t)q, (uint64_t)lanes, (count - q + lanes - 1) / lanes, (const uint64_t *)c->d_idx.p,
                                            q == q_last ? value : (void *)ko, q == q_last ? grad : (void *)(ko + 16));
      if (cs && q) c->err = k->err;
      return cs;
    };
    if ((s = graph_record(c, key, [&]() { return record_branches(c, lanes, 1, count, chain); }))) return s;
  }
  // (the children's sticky status flags are folded in by mivi_synchronize / read_status)
  return graph_replay(c, idx0, (uint64_t)count);
}

