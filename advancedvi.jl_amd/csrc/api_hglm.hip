// libmivi C ABI, the hierarchical GLM target (include/mivi.h): mivi_set_target_hglm, the row selection mivi_hglm_select_rows
// (AdvancedVI.subsample) and the partial planes' cap.  The target is a GENERIC one: eval_generic_target (api_estimate.hip) evaluates it on
// explicit samples through launch_hglm_target (kernels_hglm.hip); the target is a row of kTargets (api_common.h), whose refuse_target guards
// the entries that cannot serve it.
// What is built here, on the host, is the ORDER the kernel walks the rows in: a stable ordering by group id, the segment table of the
// groups and the first and last group of every row slice -- once per data set or selection.
#include <cmath>

#include "api_common.h"

static bool hglm_positive(double v) { return std::isfinite(v) && v > 0.0; }

// The rows `idx[0 .. nr)` of the data set (idx == nullptr: all of them, nr = hg_rows.n) in group order -> hg_rows.idx, hg_grp, hg_gstart, hg_sltab
// and the lgamma constant.  A counting sort: stable, so repeats and the rows of a group keep the order they came in.
static mivi_status_t hglm_install_rows(mivi_ctx *c, const int64_t *idx, int64_t nr) {
  const int J = c->hg.n_groups;
  const bool stored_in_order = !idx && !c->hg_pos.empty();   // host data, full set: the copy on the device IS in group order
  std::vector<int64_t> gstart((size_t)J + 1, 0), rows((size_t)nr);
  std::vector<int32_t> grp((size_t)nr);
  for (int64_t j = 0; j < nr; ++j) ++gstart[(size_t)c->hg_group[idx ? idx[j] : j] + 1];
  for (int g = 0; g < J; ++g) gstart[g + 1] += gstart[g];
  std::vector<int64_t> next(gstart.begin(), gstart.end() - 1);
  double lgam = 0.0;
  for (int64_t j = 0; j < nr; ++j) {
    const int64_t r = idx ? idx[j] : j;
    const int32_t g = c->hg_group[r];
    const int64_t at = next[g]++;
    rows[at] = c->hg_pos.empty() ? r : c->hg_pos[r];
    grp[at] = g;
  }
  if (c->hg.likelihood == 1)   // (in the evaluated order: one fixed sum per data set or selection)
    for (int64_t j = 0; j < nr; ++j) lgam += c->hg_lg[idx ? idx[j] : j];
  const mivi::RowSlices geo = mivi::row_slices(nr, mivi::kHglmSliceRows, mivi::kHglmMaxSlices);
  std::vector<int32_t> sltab(2 * (size_t)geo.n_sl);
  for (int s = 0; s < geo.n_sl; ++s) {
    const int64_t rend = (s + 1) * geo.rps < nr ? (s + 1) * geo.rps : nr;
    sltab[2 * s] = grp[s * geo.rps];
    sltab[2 * s + 1] = grp[rend - 1];
  }
  mivi_status_t s;
  if ((s = upload(c, c->hg_grp, grp.data(), (size_t)nr * sizeof(int32_t))) || (s = upload(c, c->hg_gstart, gstart.data(), ((size_t)J + 1) * sizeof(int64_t))) ||
      (s = upload(c, c->hg_sltab, sltab.data(), sltab.size() * sizeof(int32_t))))
    return s;
  if (!stored_in_order && (s = upload(c, c->hg_rows.idx, rows.data(), (size_t)nr * sizeof(int64_t)))) return s;
  c->hg_rows.sel = !stored_in_order;
  c->hg_rows.nr = nr;
  c->hg_lgam = lgam;
  return MIVI_OK;
}

mivi_status_t mivi_set_target_hglm(mivi_ctx_t *c, const mivi_hglm_t *mp, const void *X, const void *y, const void *off, const int32_t *group,
                                   int64_t n, int32_t p, int32_t on_device) {
  if (!c || !mp || !X || !y || !group) return MIVI_ERR_BAD_ARG;
  const mivi_hglm_t m = *mp;
  const bool f32 = c->cfg.dtype == MIVI_F32;
  if (n < 1) return fail(c, MIVI_ERR_BAD_ARG, "hierarchical GLM: n must be at least 1");
  if (p < 1 || p > MIVI_HGLM_MAX_P) return fail(c, MIVI_ERR_BAD_ARG, "hierarchical GLM: p must lie in [1, 256]");
  if (m.n_groups < 1) return fail(c, MIVI_ERR_BAD_ARG, "hierarchical GLM: n_groups must be at least 1");
  const long long d = (long long)p + m.n_groups + 1;
  if (c->cfg.d != d) return fail(c, MIVI_ERR_BAD_ARG, ("hierarchical GLM: the context's d must be p + n_groups + 1, " + std::to_string(d)).c_str());
  if (m.likelihood != 0 && m.likelihood != 1) return fail(c, MIVI_ERR_BAD_ARG, "hierarchical GLM: unknown likelihood (0 Bernoulli-logit, 1 Poisson-log)");
  if (!hglm_positive(m.prior_std)) return fail(c, MIVI_ERR_BAD_ARG, "hierarchical GLM: prior_std must be positive and finite");
  if (!hglm_positive(m.tau_scale)) return fail(c, MIVI_ERR_BAD_ARG, "hierarchical GLM: tau_scale must be positive and finite");
  if (!hglm_positive(m.likeadj)) return fail(c, MIVI_ERR_BAD_ARG, "hierarchical GLM: likelihood adjustment must be positive and finite");
  for (int64_t r = 0; r < n; ++r)
    if (group[r] < 0 || group[r] >= m.n_groups) return fail(c, MIVI_ERR_BAD_ARG, "hierarchical GLM: a group id lies outside [0, n_groups)");
  auto at = [&](const void *v, int64_t r) { return f32 ? (double)((const float *)v)[r] : ((const double *)v)[r]; };
  if (!on_device)
    for (int64_t r = 0; r < n; ++r) {
      const double v = at(y, r);
      if (m.likelihood == 0 && v != 0.0 && v != 1.0) return fail(c, MIVI_ERR_BAD_ARG, "hierarchical GLM: a Bernoulli label is not 0 or 1");
      if (m.likelihood == 1 && !(v >= 0.0 && v == std::floor(v) && std::isfinite(v)))
        return fail(c, MIVI_ERR_BAD_ARG, "hierarchical GLM: a Poisson response is negative or not an integer");
    }
  (void)hipSetDevice(c->cfg.device);
  invalidate_graph(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));   // an estimate in flight may still read the previous data set
  if (c->target == TGT_HGLM) c->target = TGT_NONE;   // its buffers are rewritten below: a HIP failure on the way leaves NO target, not a mixed one
  const size_t es = c->esize;
  std::vector<double> lg;
  std::vector<int64_t> pos;
  mivi_status_t s;
  if (on_device) {
    if (m.likelihood == 1) {   // the lgamma constant needs y once, on the host
      std::vector<char> yh((size_t)n * es);
      HIPCHK(c, hipMemcpy(yh.data(), y, yh.size(), hipMemcpyDeviceToHost));
      lg.resize((size_t)n);
      for (int64_t r = 0; r < n; ++r) lg[r] = std::lgamma(at(yh.data(), r) + 1.0);
    }
    c->hg_X = X;
    c->hg_y = y;
    c->hg_off = off;
  } else {   // stored in group order: the full data set reads consecutive rows
    std::vector<int64_t> next((size_t)m.n_groups + 1, 0), order((size_t)n);
    for (int64_t r = 0; r < n; ++r) ++next[(size_t)group[r] + 1];
    for (int g = 0; g < m.n_groups; ++g) next[g + 1] += next[g];
    pos.resize((size_t)n);
    for (int64_t r = 0; r < n; ++r) order[pos[r] = next[group[r]]++] = r;
    if (m.likelihood == 1) {
      lg.resize((size_t)n);
      for (int64_t r = 0; r < n; ++r) lg[r] = std::lgamma(at(y, r) + 1.0);
    }
    if ((s = ensure(c, c->hg_X_own, (size_t)n * p * es, false)) || (s = ensure(c, c->hg_y_own, (size_t)n * es, false)) ||
        (off && (s = ensure(c, c->hg_off_own, (size_t)n * es, false))))
      return s;
    std::vector<char> col((size_t)n * es);
    auto put = [&](void *dst, const char *src) {   // one column of n values, permuted
      if (f32) for (int64_t j = 0; j < n; ++j) ((float *)col.data())[j] = ((const float *)src)[order[j]];
      else for (int64_t j = 0; j < n; ++j) ((double *)col.data())[j] = ((const double *)src)[order[j]];
      return hipMemcpy(dst, col.data(), col.size(), hipMemcpyHostToDevice);
    };
    for (int k = 0; k < p; ++k) HIPCHK(c, put((char *)c->hg_X_own.p + (size_t)k * n * es, (const char *)X + (size_t)k * n * es));
    HIPCHK(c, put(c->hg_y_own.p, (const char *)y));
    if (off) HIPCHK(c, put(c->hg_off_own.p, (const char *)off));
    c->hg_X = c->hg_X_own.p;
    c->hg_y = c->hg_y_own.p;
    c->hg_off = off ? c->hg_off_own.p : nullptr;
  }
  c->hg = m;
  c->hg_p = p;
  c->hg_rows.set_full(n, m.likeadj);
  c->hg_group.assign(group, group + n);
  c->hg_pos.swap(pos);
  c->hg_lg.swap(lg);
  if (mivi_status_t st = hglm_install_rows(c, nullptr, n)) return st;
  c->lr_sched_n = c->lr_sched_k = 0;   // (a logistic regression's schedule of batches goes with its target)
  c->t_const = 0.0;
  c->target = TGT_HGLM;
  return MIVI_OK;
}

mivi_status_t mivi_hglm_select_rows(mivi_ctx_t *c, const int64_t *idx, int64_t b, double likeadj) {
  if (!c || b < 0 || (b > 0 && !idx)) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_rows_of_other_target(c, "mivi_hglm_select_rows", TGT_HGLM)) return rs;
  if (c->target != TGT_HGLM) return fail(c, MIVI_ERR_NO_TARGET, "no hierarchical GLM target set");
  (void)hipSetDevice(c->cfg.device);
  if (b > 0) {   // (checked before anything changes: a failed call leaves the previous selection in force)
    if (!hglm_positive(likeadj)) return fail(c, MIVI_ERR_BAD_ARG, "likelihood adjustment must be positive and finite");
    for (int64_t j = 0; j < b; ++j)
      if (idx[j] < 0 || idx[j] >= c->hg_rows.n) return fail(c, MIVI_ERR_BAD_ARG, "batch row index out of range");
  }
  invalidate_graph(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));   // the previous estimate may still be reading the row order
  if (mivi_status_t s = hglm_install_rows(c, b > 0 ? idx : nullptr, b > 0 ? b : c->hg_rows.n)) {
    c->target = TGT_NONE;   // (an upload failed half way: the row order on the device is no selection's)
    return s;
  }
  c->hg_rows.likeadj = b > 0 ? likeadj : c->hg_rows.likeadj_full;
  return MIVI_OK;
}

mivi_status_t mivi_hglm_set_part_cap(mivi_ctx_t *c, int64_t bytes) { return set_rows_cap(c, &mivi_ctx::hg_rows, bytes); }
